"""CPU restatement of the stack discipline of the 4-wide walk (clive2_amd/csrc/bvh_wide.hpp, traverse_wide_persistent), one lane
followed pass by pass, in numpy float32 with the operations of oracle/np_kernels.py.

What a lane does does not depend on the other lanes of its wave (the wave-level branches of the kernel only choose between two
forms of the same writes), so the model walks every ray on its own: the root box test, then per pass the pop loop with its prune
test, the speculative expansion of a wide node on top of the stack (SPEC), the four slab tests of a visit (`<` in the reference's
child order, `<=` nearest first), the stable 6-exchange sort on strict `>` with failing slots keyed +inf (ORDER), the pushes last to
first with the "candidate so far" rule, the second pop loop, and the triangle pairs (TRI_REPS per pass; nearest first: exact-t ties
by rank).  There is no pruning beyond the kernel's.  Besides the hit it reports what the kernel's host-side sizing must bound: the
peak stack pointer, and the pushes made at sp >= WIDE_STACK_LDS -- what the kernel counts as `spills`.

order_depth(boxes) is the structural bound of the nearest-first walk's stack, from the reference Box[] alone (scene_prep.hpp,
build_wide computes the same number on the wide nodes)."""
import numpy as np

from oracle import np_kernels as k

f32 = np.float32
WIDE_STACK_LDS = 8                      # scene_layout.hpp
WIDE_STACK_OVERFLOW = 136
WIDE_EMPTY = -0x80000000
_CAP = 1024                             # the model's own stack: far beyond anything a tree cl2_upload_scene accepts can reach


def slots_of(boxes, x):
    """The slots of reference box x in build_wide's order: child left+1 first, each inner child replaced by its two children."""
    left, right = boxes["left"], boxes["right"]
    out = []
    for c in (int(left[x]) + 1, int(left[x])):
        out += [c] if right[c] != 0 else [int(left[c]) + 1, int(left[c])]
    return out


def order_depth(boxes):
    """D(root): D(leaf) = 0, D(node) = (slots - 1) + max over the node's inner slots of D(slot).  0 for a tree without an inner root."""
    if len(boxes) < 3 or boxes["right"][0] != 0:
        return 0
    depth = np.zeros(len(boxes), np.int64)
    for x in np.flatnonzero(boxes["right"] == 0)[::-1]:                 # children have larger indices than their parent
        sl = slots_of(boxes, x)
        depth[x] = len(sl) - 1 + max([depth[s] for s in sl if boxes["right"][s] == 0], default=0)
    return int(depth[0])


def _slab(lo, hi, o, inv):
    """tmin, tmax of the slab test; lo, hi (..., 3, S), o, inv (..., 3)"""
    t0, t1 = (lo - o[..., None]) * inv[..., None], (hi - o[..., None]) * inv[..., None]
    tmn, tmx = k._min(t0, t1), k._max(t0, t1)
    tmin = k._max(k._max(tmn[..., 0, :], tmn[..., 1, :]), k._max(tmn[..., 2, :], f32(0.0)))
    tmax = k._min(tmx[..., 0, :], k._min(tmx[..., 1, :], tmx[..., 2, :]))
    return tmin, tmax


def walk(wide, root_lo, root_hi, tris, tri_rank, origin, direction, order, tri_reps=2, spec=True, stack_lds=WIDE_STACK_LDS):
    """One lane per ray.  wide: (n_wide, 8, 4) float32, tris: (n_tris, 3, 4) float32 {v0, e1, e2}, tri_rank: (n_tris + 2,) int32 as
    prepare_scene emits them; rays with finite 1/d.  Returns {tri, t, peak, spills, passes} (arrays per ray)."""
    wide = np.asarray(wide, f32).reshape(-1, 8, 4)
    refs = np.ascontiguousarray(wide[:, 6, :]).view(np.int32)
    blo, bhi = wide[:, 0:3, :], wide[:, 3:6, :]
    tris = np.asarray(tris, f32).reshape(-1, 3, 4)
    v0, e1, e2 = tris[:, 0, :3], tris[:, 1, :3], tris[:, 2, :3]
    rank = np.asarray(tri_rank, np.int64)
    o, d = np.asarray(origin, f32), np.asarray(direction, f32)
    n = len(o)
    inv = f32(1.0) / d
    assert np.isfinite(inv).all(), "the wide walk takes rays with finite 1/d only"
    inf = f32(np.inf)
    best_i, best_t = np.full(n, -1, np.int64), np.full(n, inf, f32)
    cur, tri_i, tri_end, sp = np.full(n, -1, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    st_ref, st_t = np.zeros((n, _CAP), np.int64), np.zeros((n, _CAP), f32)
    peak, spills, passes = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)

    def in_front(t, r):                                  # the prune test of a stack entry / a slot against the lane's best_t
        return t <= best_t[r] if order else t < best_t[r]

    def take(r, ref):
        node = ref >= 0
        cur[r[node]] = ref[node]
        info = ~ref[~node]
        tri_i[r[~node]] = info >> 4
        tri_end[r[~node]] = (info >> 4) + (info & 15) + 1

    def pop_loop(active):
        need = active & (cur < 0) & (tri_i >= tri_end) & (sp > 0)
        while need.any():
            r = np.flatnonzero(need)
            sp[r] -= 1
            ref, t = st_ref[r, sp[r]], st_t[r, sp[r]]
            keep = in_front(t, r)
            take(r[keep], ref[keep])
            need[r[keep]] = False
            need[r[~keep]] = sp[r[~keep]] > 0

    def push(r, ref, t):
        st_ref[r, sp[r]], st_t[r, sp[r]] = ref, t
        sp[r] += 1
        peak[r] = np.maximum(peak[r], sp[r])

    def tri_test(r, ti, tie_rule):
        """tri_test_branchless_tie (tie_rule False) / tri_test_tie_rule: returns which rays tied at exactly best_t"""
        h = k._cross(d[r], e2[ti])
        f = f32(1.0) / k._dot(e1[ti], h)
        s = o[r] - v0[ti]
        u = f * k._dot(s, h)
        q = k._cross(s, e1[ti])
        v = f * k._dot(d[r], q)
        t = f * k._dot(e2[ti], q)
        inside = ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1)) & (t > k.DELTA)
        ok = inside & (t < best_t[r])
        tie = inside & (t == best_t[r])
        if tie_rule:
            ok |= tie & (rank[1 + ti] < rank[1 + best_i[r]])
        best_i[r[ok]], best_t[r[ok]] = ti[ok], t[ok]
        return tie

    with np.errstate(all="ignore"):
        tmin, tmax = _slab(np.asarray(root_lo, f32)[:3, None], np.asarray(root_hi, f32)[:3, None], o, inv)
        active = np.ones(n, bool)
        cur[(tmin[:, 0] <= tmax[:, 0]) & (tmin[:, 0] < inf)] = 0       # best_t = +inf
        while active.any():
            passes[active] += 1
            pop_loop(active)
            specd = np.zeros(n, bool)
            vnode = cur.copy()
            if spec:
                cand = np.flatnonzero(active & (cur < 0) & (tri_i < tri_end) & (sp > 0) & (sp + 3 <= stack_lds))
                top = st_ref[cand, sp[cand] - 1]
                cand, top = cand[top >= 0], top[top >= 0]              # a wide node on top: it leaves the stack, pruned or expanded
                sp[cand] -= 1
                go = in_front(st_t[cand, sp[cand]], cand)
                specd[cand[go]] = True
                vnode[cand[go]] = top[go]
            r = np.flatnonzero(active & ((cur >= 0) | specd))
            if len(r):
                node = vnode[r]
                cur[r] = -1
                tm, tx = _slab(blo[node], bhi[node], o[r], inv[r])
                ref = refs[node].astype(np.int64)
                ok = (tm <= tx) & in_front(tm, r[:, None])
                if order:
                    tm, ref = np.where(ok, tm, inf), np.where(ok, ref, WIDE_EMPTY)
                    for a, b in ((0, 1), (1, 2), (2, 3), (0, 1), (1, 2), (0, 1)):
                        sw = tm[:, a] > tm[:, b]
                        tm[sw, a], tm[sw, b] = tm[sw, b], tm[sw, a]
                        ref[sw, a], ref[sw, b] = ref[sw, b], ref[sw, a]
                    ok = ref != WIDE_EMPTY
                next_ref, next_t = np.where(ok[:, 3], ref[:, 3], WIDE_EMPTY), tm[:, 3].copy()
                for s in (2, 1, 0):
                    p = ok[:, s] & (next_ref != WIDE_EMPTY)
                    spills[r[p]] += sp[r[p]] >= stack_lds
                    push(r[p], next_ref[p], next_t[p])
                    next_ref, next_t = np.where(ok[:, s], ref[:, s], next_ref), np.where(ok[:, s], tm[:, s], next_t)
                has = next_ref != WIDE_EMPTY
                waits = has & specd[r]                                   # the lane is busy with its leaf: the slot waits on the stack
                push(r[waits], next_ref[waits], next_t[waits])
                take(r[has & ~specd[r]], next_ref[has & ~specd[r]])
                pop_loop(active)
            for _ in range(tri_reps):
                r = np.flatnonzero(active & (tri_i < tri_end))
                if not len(r):
                    break
                i0 = tri_i[r]
                i1 = np.where(i0 + 1 < tri_end[r], i0 + 1, i0)
                tri_i[r] = i1 + 1
                two = i1 != i0
                tie = tri_test(r, i0, False)
                tie[two] |= tri_test(r[two], i1[two], False)
                if order and tie.any():
                    tri_test(r[tie], i0[tie], True)
                    tri_test(r[tie & two], i1[tie & two], True)
            active &= ~((tri_i >= tri_end) & (cur < 0) & (sp == 0))
    return {"tri": best_i.astype(np.int32), "t": best_t, "peak": peak, "spills": spills, "passes": passes}
