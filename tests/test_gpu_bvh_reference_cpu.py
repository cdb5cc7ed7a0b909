"""The numpy statement of the GPU BVH builder (tests/gpu_bvh_reference.py) on its own, without a GPU: its trees pass the independent
checker on every input of tests/gpu_bvh_cases.py, the inputs take the paths they are meant to take (the guards), its top-down radix
split is the one k_hierarchy's search finds (a literal transcription of the kernel), and the checker rejects hand-made faults."""
import numpy as np
import pytest

import gpu_bvh_cases as cases
import gpu_bvh_reference as ref

F = np.float32


@pytest.mark.parametrize("case", cases.CASES, ids=repr)
def test_restated_trees_are_valid_and_take_their_path(case):
    p = case.prepared()
    case.guard(p)
    lo, hi = case.boxes()
    assert np.array_equal(np.sort(p.order), np.arange(p.n)) and (p.keys_sorted[1:] >= p.keys_sorted[:-1]).all()
    same = p.keys_sorted[1:] == p.keys_sorted[:-1]
    assert (np.diff(p.order)[same] > 0).all()                         # equal keys stay in index order
    for mm in case.members:
        boxes, perm = case.tree(mm)
        ref.check_tree(lo, hi, boxes, perm, mm)
        if mm >= p.n:
            assert len(boxes) == 1 and boxes["left"][0] == 0 and boxes["right"][0] == p.n
            assert np.array_equal(boxes["min"][0, :3], lo.astype(F).min(axis=0)) and np.array_equal(boxes["max"][0, :3], hi.astype(F).max(axis=0))
        if mm == 1:
            assert len(boxes) == 2 * p.n - 1


def test_families_take_both_paths_and_report_their_rounds():
    """the summary of the paths: every family's rounds, printed (pytest -s)"""
    for c in cases.CASES:
        p = c.prepared()
        print(f"{c.family:11s} {c.name:16s} n {p.n:6d}  path {p.path:5s}  rounds {p.rounds:3d}  clusters left {p.clusters_left}")
    paths = {(c.family, c.prepared().path) for c in cases.CASES}
    assert {("sizes", "ploc"), ("sizes", "radix"), ("lbvh", "radix"), ("ties", "ploc"), ("equal-keys", "ploc"), ("equal-keys", "radix"),
            ("degenerate", "ploc"), ("fallback", "radix")} <= paths


def test_the_grids_hold_exact_area_ties():
    """in the first round nearly every cluster has several candidates at its smallest area, and the (min, max) rule picks among them
    (the doubled grid first merges every box with its copy, in one round, and is the plain grid from then on)"""
    assert cases.by_name("grid-doubled").prepared().merges[0] == 4096
    p = cases.by_name("grid").prepared()
    lo, hi, m = p.lo_sorted, p.hi_sorted, p.n
    nn = ref.ploc_neighbours(lo, hi)
    pos = np.arange(m)
    best = ref._union_area(lo, hi, lo[nn], hi[nn])
    ties = np.zeros(m, np.int64)
    for off in range(1, ref.PLOC_RADIUS + 1):
        for j in (pos - off, pos + off):
            ok = (j >= 0) & (j < m)
            ties[ok] += ref._union_area(lo[ok], hi[ok], lo[j[ok]], hi[j[ok]]) == best[ok]
    assert (ties >= 2).mean() > 0.9
    # and the rule is the stated one: the chosen partner gives the smallest (min, max) pair among the tied candidates
    for i in pos[::37]:
        tied = [j for j in range(max(i - ref.PLOC_RADIUS, 0), min(i + ref.PLOC_RADIUS, m - 1) + 1)
                if j != i and ref._union_area(lo[i:i + 1], hi[i:i + 1], lo[j:j + 1], hi[j:j + 1])[0] == best[i]]
        assert nn[i] == min(tied, key=lambda j: (min(i, j), max(i, j)))


def test_the_lattice_tells_the_pair_rule_from_first_come(monkeypatch):
    """without the rule at equal areas (the first candidate in the order i-1, i+1, ... keeps a tie) the lattice gives another tree"""
    def first_come(lo, hi):
        m = len(lo)
        best, arg, pos = np.full(m, np.inf, F), np.full(m, -1, np.int64), np.arange(m)
        for off in range(1, ref.PLOC_RADIUS + 1):
            for sgn in (-1, 1):
                j = pos + sgn * off
                ok = (j >= 0) & (j < m)
                i, j = pos[ok], j[ok]
                area = ref._union_area(lo[i], hi[i], lo[j], hi[j])
                better = area < best[i]
                best[i[better]], arg[i[better]] = area[better], j[better]
        return arg
    case = cases.by_name("lattice")
    want, want_perm = case.tree(1)
    monkeypatch.setattr(ref, "ploc_neighbours", first_come)
    boxes, perm, p = ref.build(*case.boxes(), 1)
    assert p.path == "ploc"
    ref.check_tree(*case.boxes(), boxes, perm, 1)                      # a valid tree, but not the builder's
    assert boxes.tobytes() != want.tobytes()


# ---- the radix split against k_hierarchy ---------------------------------------------------------------------------------------------

def _delta(keys, n, i, j):
    if j < 0 or j >= n:
        return -1
    a, b = int(keys[i]), int(keys[j])
    if a != b:
        return 64 - (a ^ b).bit_length()                              # __clzll
    return 64 + 32 - (i ^ j).bit_length()                             # 64 + __clz


def _karras(keys, n, i):
    """k_hierarchy for inner node i: (first, last, gamma)"""
    d = 1 if _delta(keys, n, i, i + 1) - _delta(keys, n, i, i - 1) >= 0 else -1
    dmin = _delta(keys, n, i, i - d)
    lmax = 2
    while _delta(keys, n, i, i + lmax * d) > dmin:
        lmax *= 2
    l, t = 0, lmax // 2
    while t >= 1:
        if _delta(keys, n, i, i + (l + t) * d) > dmin:
            l += t
        t //= 2
    j = i + l * d
    dnode = _delta(keys, n, i, j)
    s, t = 0, (l + 1) // 2
    while True:
        if _delta(keys, n, i, i + (s + t) * d) > dnode:
            s += t
        if t == 1:
            break
        t = (t + 1) // 2
    gamma = i + s * d + min(d, 0)
    return min(i, j), max(i, j), gamma


def _top_down(keys):
    """every range the top-down split produces: {(first, last): gamma}"""
    out, todo = {}, [(0, len(keys) - 1)]
    while todo:
        first, last = todo.pop()
        if first < last:
            g = out[first, last] = ref.radix_split(keys, first, last)
            todo += [(first, g), (g + 1, last)]
    return out


@pytest.mark.parametrize("kind", ["distinct", "many-equal", "all-equal"])
@pytest.mark.parametrize("n", [2, 3, 9, 100, 1000])
def test_top_down_split_is_the_kernels_search(n, kind):
    rng = np.random.RandomState(n)
    if kind == "distinct":
        keys = np.cumsum(rng.randint(1, 1 << 30, n)).astype(np.uint64) << np.uint64(20)      # < 2^60, strictly ascending
    elif kind == "many-equal":
        keys = np.sort(rng.randint(0, max(2, n // 5), n).astype(np.uint64) << np.uint64(rng.randint(0, 50)))
    else:
        keys = np.full(n, 0x1249249249249249, np.uint64)
    want = _top_down(keys)
    got = {}
    for i in range(n - 1):
        first, last, gamma = _karras(keys, n, i)
        assert (first, last) not in got
        got[first, last] = gamma
        assert i in (first, last)
    assert got == want and len(got) == n - 1
    # node i sits at the split of its parent: the kernel's child links (gamma, gamma + 1) name nodes of those ranges
    for (first, last), g in got.items():
        for a, b, node in ((first, g, g), (g + 1, last, g + 1)):
            if a < b:
                assert _karras(keys, n, node)[:2] == (a, b)


# ---- the checker rejects faults ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def good():
    c = cases.by_name("ploc-257")
    lo, hi = c.boxes()
    boxes, perm = c.tree(3)
    ref.check_tree(lo, hi, boxes, perm, 3)
    return lo, hi, boxes, perm


def _rejects(good, what, boxes=None, perm=None, mm=3):
    lo, hi, b, p = good
    with pytest.raises(AssertionError, match=what):
        ref.check_tree(lo, hi, b if boxes is None else boxes, p if perm is None else perm, mm)


def test_checker_rejects_a_leaf_box_shrunk_by_one_ulp(good):
    for field, toward in (("max", -np.inf), ("min", np.inf)):
        b = good[2].copy()
        leaf = np.flatnonzero(b["right"] != 0)[5]
        b[field][leaf, 1] = np.nextafter(b[field][leaf, 1], F(toward))
        _rejects(good, "leaf box", boxes=b)


def test_checker_rejects_an_inner_box_that_is_not_the_union(good):
    b = good[2].copy()
    node = np.flatnonzero(b["right"] == 0)[3]
    b["max"][node, 0] = np.nextafter(b["max"][node, 0], F(np.inf))       # still contains everything: only the checker can tell
    _rejects(good, "inner box", boxes=b)


def test_checker_rejects_swapped_siblings(good):
    lo, hi, boxes, perm = good
    count = ref.check_tree(lo, hi, boxes, perm, 3)
    left = boxes["left"]
    # a pair of leaves of different sizes under one parent: swapping them (with their triangles) keeps everything else valid
    for node in np.flatnonzero(boxes["right"] == 0):
        a, c = left[node], left[node] + 1
        if boxes["right"][a] and boxes["right"][c] and count[a] != count[c]:
            break
    else:
        pytest.fail("no such pair")
    b, p = boxes.copy(), perm.copy()
    start = b["left"][a]
    tri_a, tri_c = p[b["left"][a]:b["right"][a]].copy(), p[b["left"][c]:b["right"][c]].copy()
    b[[a, c]] = b[[c, a]]
    b["left"][a], b["right"][a] = start, start + len(tri_c)
    b["left"][c], b["right"][c] = start + len(tri_c), start + len(tri_c) + len(tri_a)
    p[start:start + len(tri_c) + len(tri_a)] = np.concatenate([tri_c, tri_a])
    _rejects(good, "larger subtree", boxes=b, perm=p)


def test_checker_rejects_a_duplicated_perm_entry(good):
    p = good[3].copy()
    p[10] = p[11]
    _rejects(good, "permutation", perm=p)


def test_checker_rejects_an_oversized_leaf(good):
    _rejects(good, "oversized", mm=2)                                 # the tree has leaves of three
    c = cases.by_name("ploc-9")
    lo, hi = c.boxes()
    boxes, perm = c.tree(9)
    with pytest.raises(AssertionError, match="oversized"):
        ref.check_tree(lo, hi, boxes, perm, 8)


def test_checker_rejects_broken_numbering_and_small_inner_boxes(good):
    b = good[2].copy()
    inner = np.flatnonzero(b["right"] == 0)
    b["left"][inner[4]] = b["left"][inner[5]]                          # two parents of the same children
    _rejects(good, "referenced", boxes=b)
    _rejects(good, "no more than a leaf", mm=8)                        # flattened at 3: inner boxes of 4..8 triangles remain
