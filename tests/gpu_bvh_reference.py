"""Plain numpy statement of the GPU BVH builder (cl2_build_bvh_gpu, clive2_amd/csrc/bvh_builder_gpu.hip) and a checker of the
flattened trees that depends on neither builder.  No GPU, no library: written from the comments and the code of the builder.

The library is compiled with -ffp-contract=off -fno-fast-math, so every float32 operation of the device code rounds once, in source
order, and has a numpy float32 equivalent; the algorithm is deterministic (the nearest-neighbour key is a total order on pairs, the
radix sort is stable, the scan is exact integer arithmetic).  `build` therefore states THE tree the builder is to return:

    preparation   lo, hi = float32 of the float64 bounds; centroid = float32((min + max) * 0.5) in float64; per axis
                  t = (c - a) / ext over the centroid bounds [a, b], ext = b - a in float32 (0 where ext is not > 0), NaN -> 0, clamped
                  to [0, 1], q = min(uint(t * 2^21), 2^21 - 1); key = x bits << 2 | y bits << 1 | z bits, every third bit of 63;
                  sorted order = stable argsort of the keys
    PLOC          radius 8, candidates i-1, i+1, i-2, i+2, ...; area = x*y + y*z + z*x of the union in float32; smaller area wins, at
                  an equal area the lexicographically smaller (min, max) pair of positions; mutual pairs merge into node next + rank;
                  children (lower position, its partner); survivors keep their order; ends at one cluster, at a round without a merge
                  or after 400 rounds -- and unless ONE cluster is left the PLOC work is discarded and the radix tree is built
    radix tree    over sorted positions [first, last]: A_p = key_p * 2^32 + p, b the highest bit in which A_first and A_last differ,
                  gamma the last p of the range with bit b of A_p clear, children [first, gamma] and [gamma + 1, last]
    flattening    breadth-first queue from the root; a subtree of <= max_members triangles is a leaf (its triangles left to right);
                  otherwise left = len(queue), right = 0, the larger child queued first (equal sizes: x / the left child first)
"""
import numpy as np

import clive2_amd.struct_types as st

F = np.float32
PLOC_RADIUS = 8
PLOC_MAX_ROUNDS = 400
KEY_STEPS = 2097152                   # 2^21 cells per axis


# ---- preparation ---------------------------------------------------------------------------------------------------------------------

def spread21(v):
    """21 bits -> every third bit of 63 (bit k of v lands on bit 3 k)"""
    v = np.asarray(v, np.uint64)
    out = np.zeros(v.shape, np.uint64)
    for k in range(21):
        out |= ((v >> np.uint64(k)) & np.uint64(1)) << np.uint64(3 * k)
    return out


def prepare(tmin, tmax):
    """float32 bounds, the 63-bit Morton keys and the sorted order (original indices, equal keys in index order)"""
    tmin, tmax = np.asarray(tmin, np.float64).reshape(-1, 3), np.asarray(tmax, np.float64).reshape(-1, 3)
    lo, hi = tmin.astype(F), tmax.astype(F)
    c = ((tmin + tmax) * 0.5).astype(F)
    a, b = c.min(axis=0), c.max(axis=0)
    with np.errstate(all="ignore"):
        ext = (b - a).astype(F)
        t = np.zeros_like(c)
        for k in range(3):
            if ext[k] > 0:
                t[:, k] = ((c[:, k] - a[k]).astype(F) / ext[k]).astype(F)
        t = np.where(np.isnan(t), F(0), t)
        t = np.minimum(np.maximum(t, F(0)), F(1))
        q = np.minimum((t * F(KEY_STEPS)).astype(F).astype(np.uint64), np.uint64(KEY_STEPS - 1))
    keys = (spread21(q[:, 0]) << np.uint64(2)) | (spread21(q[:, 1]) << np.uint64(1)) | spread21(q[:, 2])
    order = np.argsort(keys, kind="stable")
    return lo, hi, keys, order


# ---- PLOC ----------------------------------------------------------------------------------------------------------------------------

def _union_area(lo_a, hi_a, lo_b, hi_b):
    with np.errstate(all="ignore"):
        e = (np.maximum(hi_a, hi_b) - np.minimum(lo_a, lo_b)).astype(F)
        x, y, z = e[:, 0], e[:, 1], e[:, 2]
        return (((x * y).astype(F) + (y * z).astype(F)).astype(F) + (z * x).astype(F)).astype(F)


def ploc_neighbours(lo, hi):
    """nn[i] of one round over the clusters' boxes in list order (-1: no candidate had an area below +inf)"""
    m = len(lo)
    best = np.full(m, np.inf, F)
    arg = np.full(m, -1, np.int64)
    pos = np.arange(m)
    for off in range(1, PLOC_RADIUS + 1):
        for sgn in (-1, 1):
            j = pos + sgn * off
            ok = (j >= 0) & (j < m)
            i, j = pos[ok], j[ok]
            area = _union_area(lo[i], hi[i], lo[j], hi[j])
            better = area < best[i]
            tie = (area == best[i]) & (arg[i] >= 0)
            a0, a1 = np.minimum(i, j), np.maximum(i, j)
            b0, b1 = np.minimum(i, arg[i]), np.maximum(i, arg[i])
            better = np.where(tie, (a0 < b0) | ((a0 == b0) & (a1 < b1)), better)
            best[i[better]] = area[better]
            arg[i[better]] = j[better]
    return arg


def ploc(lo_sorted, hi_sorted):
    """The PLOC rounds over the triangles in sorted order.  Node ids 0..n-1 are the sorted triangles, n + k the k-th merge.
    Returns (children (2n-1, 2), node lo, node hi, rounds, clusters left, merges of every round)."""
    n = len(lo_sorted)
    blo, bhi = np.zeros((2 * n - 1, 3), F), np.zeros((2 * n - 1, 3), F)
    blo[:n], bhi[:n] = lo_sorted, hi_sorted
    children = np.full((2 * n - 1, 2), -1, np.int64)
    cid = np.arange(n)
    nxt, rounds, merges = n, 0, []
    while len(cid) > 1 and rounds < PLOC_MAX_ROUNDS:
        m = len(cid)
        nn = ploc_neighbours(blo[cid], bhi[cid])
        pos = np.arange(m)
        mutual = (nn >= 0) & (nn[np.maximum(nn, 0)] == pos)
        keep = ~(mutual & (nn < pos))
        first = mutual & (pos < nn)
        merged = int(first.sum())
        if merged < 1:
            break
        a, b = cid[first], cid[nn[first]]
        ids = nxt + np.arange(merged)                     # rank of the pair's lower position among this round's merges
        blo[ids], bhi[ids] = np.minimum(blo[a], blo[b]), np.maximum(bhi[a], bhi[b])
        children[ids, 0], children[ids, 1] = a, b
        out = cid.copy()
        out[first] = ids
        cid = out[keep]
        nxt += merged
        rounds += 1
        merges.append(merged)
    return children, blo, bhi, rounds, len(cid), merges


# ---- radix tree ----------------------------------------------------------------------------------------------------------------------

def radix_split(keys_sorted, first, last):
    """gamma of the range [first, last], first < last, of sorted positions"""
    a_first = (int(keys_sorted[first]) << 32) | first
    a_last = (int(keys_sorted[last]) << 32) | last
    b = (a_first ^ a_last).bit_length() - 1
    if b >= 32:
        clear = ((keys_sorted[first:last + 1] >> np.uint64(b - 32)) & np.uint64(1)) == 0
    else:
        clear = ((np.arange(first, last + 1) >> b) & 1) == 0
    return first + int(np.flatnonzero(clear)[-1])


# ---- flattening ----------------------------------------------------------------------------------------------------------------------

def _boxes(rows):
    out = np.zeros(len(rows), st.Box)
    for k, (lo, hi, left, right) in enumerate(rows):
        out["min"][k, :3], out["max"][k, :3], out["left"][k], out["right"][k] = lo, hi, left, right
    return out


def flatten_ploc(children, blo, bhi, order, max_members):
    n = len(order)
    size = np.ones(2 * n - 1, np.int64)
    for i in range(n, 2 * n - 1):
        size[i] = size[children[i, 0]] + size[children[i, 1]]
    queue, rows, perm = [2 * n - 2], [], []
    head = 0
    while head < len(queue):
        node = queue[head]
        head += 1
        if size[node] <= max_members:
            rows.append((blo[node], bhi[node], len(perm), len(perm) + int(size[node])))
            stack = [node]
            while stack:
                y = stack.pop()
                if y < n:
                    perm.append(int(order[y]))
                else:
                    stack += [int(children[y, 1]), int(children[y, 0])]
        else:
            x, y = int(children[node, 0]), int(children[node, 1])
            rows.append((blo[node], bhi[node], len(queue), 0))
            queue += [y, x] if size[x] < size[y] else [x, y]
    return _boxes(rows), np.array(perm, np.int64)


def flatten_radix(keys_sorted, lo_sorted, hi_sorted, order, max_members):
    n = len(order)
    queue, rows, perm = [(0, n - 1)], [], []
    head = 0
    while head < len(queue):
        first, last = queue[head]
        head += 1
        lo, hi = lo_sorted[first:last + 1].min(axis=0), hi_sorted[first:last + 1].max(axis=0)
        count = last - first + 1
        if count == 1 or count <= max_members:
            rows.append((lo, hi, len(perm), len(perm) + count))
            perm += [int(t) for t in order[first:last + 1]]
        else:
            g = radix_split(keys_sorted, first, last)
            left, right = (first, g), (g + 1, last)
            rows.append((lo, hi, len(queue), 0))
            queue += [right, left] if g - first + 1 < last - g else [left, right]
    return _boxes(rows), np.array(perm, np.int64)


class Prepared:
    """Everything of a build that does not depend on max_members (one PLOC run serves every leaf size)."""

    def __init__(self, tmin, tmax, method="ploc"):
        if method not in ("ploc", "lbvh"):
            raise ValueError(method)
        self.lo, self.hi, self.keys, self.order = prepare(tmin, tmax)
        self.n = n = len(self.order)
        self.keys_sorted = self.keys[self.order]
        self.lo_sorted, self.hi_sorted = self.lo[self.order], self.hi[self.order]
        self.rounds, self.clusters_left, self.merges, self.tree = 0, n, [], None
        if method == "ploc" and n > 2:
            children, blo, bhi, self.rounds, self.clusters_left, self.merges = ploc(self.lo_sorted, self.hi_sorted)
            if self.clusters_left == 1:
                self.tree = (children, blo, bhi)         # otherwise the PLOC work is discarded
        self.path = "ploc" if self.tree is not None else "radix"

    def flatten(self, max_members):
        if self.tree is not None:
            return flatten_ploc(*self.tree, self.order, max_members)
        return flatten_radix(self.keys_sorted, self.lo_sorted, self.hi_sorted, self.order, max_members)


def build(tmin, tmax, max_members, method="ploc"):
    """(boxes, perm, prepared): the tree cl2_build_bvh_gpu is to return; method "lbvh" is CLIVE2_GPU_BVH=lbvh"""
    p = Prepared(tmin, tmax, method)
    return p.flatten(max_members) + (p,)


# ---- checker -------------------------------------------------------------------------------------------------------------------------

def _need(cond, what):
    if not cond:
        raise AssertionError(what)


def check_tree(tmin, tmax, boxes, perm, max_members):
    """What the tracer and cl2_upload_scene rely on in a flattened tree, from the input bounds alone.  Bounds are compared as float
    values (fminf(-0, +0) may return either zero)."""
    lo = np.asarray(tmin, np.float64).reshape(-1, 3).astype(F)
    hi = np.asarray(tmax, np.float64).reshape(-1, 3).astype(F)
    n, nb = len(lo), len(boxes)
    perm = np.asarray(perm)
    _need(len(perm) == n and np.array_equal(np.sort(perm), np.arange(n)), "perm is not a permutation")
    left, right = boxes["left"].astype(np.int64), boxes["right"].astype(np.int64)
    inner = right == 0
    at = np.flatnonzero(inner)
    # breadth-first numbering
    kids = np.concatenate([left[inner], left[inner] + 1])
    _need(np.array_equal(np.sort(kids), np.arange(1, nb)), "children are not referenced exactly once each")
    _need((left[inner] > at).all(), "a child lies before its parent")
    _need(np.array_equal(left[inner], np.sort(left[inner])), "parents' left values do not ascend")
    # leaves
    lf = ~inner
    sizes = right[lf] - left[lf]
    _need(lf.any() and (sizes >= 1).all(), "an empty leaf")
    _need((sizes <= max_members).all(), "an oversized leaf")
    _need(sizes.sum() == n and np.array_equal(left[lf], np.concatenate([[0], np.cumsum(sizes)[:-1]])),
          "leaves are not consecutive ranges covering every triangle")
    starts = left[lf]
    bmin, bmax = boxes["min"][:, :3], boxes["max"][:, :3]
    _need(np.array_equal(np.minimum.reduceat(lo[perm], starts), bmin[lf]) and
          np.array_equal(np.maximum.reduceat(hi[perm], starts), bmax[lf]), "a leaf box is not the bounds of its triangles")
    li = left[inner]
    _need(np.array_equal(np.minimum(bmin[li], bmin[li + 1]), bmin[inner]) and
          np.array_equal(np.maximum(bmax[li], bmax[li + 1]), bmax[inner]), "an inner box is not the union of its children")
    # triangles below every box (children lie behind their parents)
    count = np.where(lf, right - left, 0)
    for i in at[::-1]:
        count[i] = count[left[i]] + count[left[i] + 1]
    _need((count[li + 1] <= count[li]).all(), "the larger subtree is at left + 1")
    _need((count[inner] > max_members).all(), "an inner box holds no more than a leaf may")
    return count
