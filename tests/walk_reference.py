"""References of the walk tests -- TEST INFRASTRUCTURE.

    brute_force   "the nearest triangle along the ray" in float64: Moeller-Trumbore over ALL triangles, no tree, no float32.  What the
                  C oracle's traverse is checked against (tests/test_walk_cases_cpu.py), so that the device tests' "kernel == oracle"
                  cannot hide a misreading of trace.metal:106-176 that both share.
    walk_log      the reference's walk (trace.metal:144-176) in numpy float32, operation for operation as oracle/np_kernels.py's
                  traverse, which also says what each ray met on its way: a NaN slab value in a visited box, a == 0 on a tested
                  triangle, and its box and triangle test counts.  Its hits must equal the C oracle's byte for byte.
    tied          for each ray the records that a triangle test over ALL triangles accepts at exactly the winning t."""
import numpy as np

from oracle.np_kernels import DELTA, _cross, _dot, _max, _min, f32


def brute_force(o, d, triangles, group=None, chunk=2048):
    """Float64 closest hit of every ray over all triangles.  group[i] names triangle i's set of coincident copies (default: every
    triangle its own): the second hit is the nearest one OUTSIDE the winner's set.  Returns a dict of arrays:

        tri, t          the nearest hit (-1, inf: none); tri2, t2: the second
        edge            the winner's distance from its edges in barycentric terms: min(u, v, 1 - u - v)
        sine            the sine of the angle between the ray and the winner's plane: |d . n| / (|d| |n|)
        near_miss       for a ray without a hit: some triangle is hit when its edges are moved out by 1e-3 (barycentric) and DELTA
                        is halved -- such a miss is not a well-conditioned one"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    v0 = triangles["v0"][:, :3].astype(np.float64)
    e1 = triangles["v1"][:, :3].astype(np.float64) - v0
    e2 = triangles["v2"][:, :3].astype(np.float64) - v0
    nrm = np.cross(e1, e2)
    nlen = np.linalg.norm(nrm, axis=1)
    group = np.arange(len(v0)) if group is None else np.asarray(group)
    n = len(o)
    out = {"tri": np.full(n, -1, np.int64), "t": np.full(n, np.inf), "tri2": np.full(n, -1, np.int64), "t2": np.full(n, np.inf),
           "edge": np.zeros(n), "sine": np.zeros(n), "near_miss": np.zeros(n, bool)}
    delta = float(DELTA)
    for at in range(0, n, chunk):
        oo, dd = o[at:at + chunk, None, :], d[at:at + chunk, None, :]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            h = np.cross(dd, e2[None])
            a = (e1[None] * h).sum(axis=2)
            f = np.where(a != 0, 1.0 / np.where(a != 0, a, 1.0), np.nan)           # a degenerate or parallel triangle is no hit
            s = oo - v0[None]
            u = f * (s * h).sum(axis=2)
            q = np.cross(s, e1[None])
            v = f * (dd * q).sum(axis=2)
            t = f * (e2[None] * q).sum(axis=2)
            hit = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > delta)
            near = (u >= -1e-3) & (v >= -1e-3) & (u + v <= 1 + 1e-3) & (t > delta / 2)
        th = np.where(hit, t, np.inf)
        rows = np.arange(len(th))
        w = th.argmin(axis=1)
        tw = th[rows, w]
        has = np.isfinite(tw)
        others = np.where(group[None, :] == group[w][:, None], np.inf, th)
        w2 = others.argmin(axis=1)
        sl = slice(at, at + len(th))
        out["tri"][sl] = np.where(has, w, -1)
        out["t"][sl] = tw
        out["tri2"][sl] = np.where(np.isfinite(others[rows, w2]), w2, -1)
        out["t2"][sl] = others[rows, w2]
        uw, vw = u[rows, w], v[rows, w]
        out["edge"][sl] = np.where(has, np.minimum(np.minimum(uw, vw), 1 - uw - vw), 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            sine = np.abs((dd[:, 0] * nrm[w]).sum(axis=1)) / (np.linalg.norm(dd[:, 0], axis=1) * nlen[w])
        out["sine"][sl] = np.where(has, sine, 0)
        out["near_miss"][sl] = ~has & near.any(axis=1)
    return out


def well_conditioned(bf):
    """The rays on which float32 and float64 must name the same triangle: the second hit more than 1e-3 t behind the first, the winner
    hit more than 1e-3 from its edges, the ray more than 1e-2 (sine) off its plane; a miss: no near miss."""
    hit = bf["tri"] >= 0
    t = np.where(hit, bf["t"], 0.0)
    good = hit & (bf["t2"] - t > 1e-3 * t) & (bf["edge"] > 1e-3) & (bf["sine"] > 1e-2)
    return np.where(hit, good, ~bf["near_miss"])


def walk_log(o, d, boxes, triangles, tested=False):
    """The reference's walk per ray in float32.  Returns a dict: tri, t, u, v (the hit records), nan_slab (a slab product of a visited
    box was NaN), zero_a (a == 0 on a tested triangle), box_tests, tri_tests (per ray); with `tested` also tested[ray, triangle]: the
    walk ran the triangle's test for that ray (its leaf was entered)."""
    n = len(o)
    seen = np.zeros((n, len(triangles)), bool) if tested else None
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        inv = f32(1.0) / d
        bmin, bmax = boxes["min"][:, :3].astype(f32), boxes["max"][:, :3].astype(f32)
        left, right = boxes["left"].astype(np.int64), boxes["right"].astype(np.int64)
        v0 = triangles["v0"][:, :3].astype(f32)
        e1 = triangles["v1"][:, :3].astype(f32) - v0
        e2 = triangles["v2"][:, :3].astype(f32) - v0
        best_i = np.full(n, -1, np.int32)
        best_t = np.full(n, np.inf, f32)
        bu, bv = np.zeros(n, f32), np.zeros(n, f32)
        nan_slab, zero_a = np.zeros(n, bool), np.zeros(n, bool)
        box_tests, tri_tests = np.zeros(n, np.int64), np.zeros(n, np.int64)
        stack = np.zeros((n, 64), np.int64)
        sp = np.ones(n, np.int64)
        while True:
            act = np.flatnonzero((sp > 0) & (sp < 64))
            if len(act) == 0:
                break
            sp[act] -= 1
            node = stack[act, sp[act]]
            box_tests[act] += 1
            t0 = (bmin[node] - o[act]) * inv[act]
            t1 = (bmax[node] - o[act]) * inv[act]
            nan_slab[act] |= np.isnan(t0).any(axis=1) | np.isnan(t1).any(axis=1)
            tmn, tmx = _min(t0, t1), _max(t0, t1)
            tmin = _max(_max(tmn[:, 0], tmn[:, 1]), _max(tmn[:, 2], f32(0.0)))
            tmax = _min(_min(tmx[:, 0], tmx[:, 1]), _min(tmx[:, 2], f32(np.inf)))
            go = (tmin <= tmax) & (tmin < best_t[act])
            inner = go & (right[node] == 0)
            ia = act[inner]
            stack[ia, sp[ia]] = left[node[inner]]
            stack[ia, sp[ia] + 1] = left[node[inner]] + 1
            sp[ia] += 2
            leaf = go & (right[node] != 0)
            la, ln = act[leaf], node[leaf]
            if len(la):
                for k in range(int((right[ln] - left[ln]).max())):
                    tri = left[ln] + k
                    m = tri < right[ln]
                    r, ti = la[m], tri[m]
                    tri_tests[r] += 1
                    if tested:
                        seen[r, ti] = True
                    h = _cross(d[r], e2[ti])
                    a = _dot(e1[ti], h)
                    zero_a[r] |= a == 0
                    f = f32(1.0) / a
                    s = o[r] - v0[ti]
                    u = f * _dot(s, h)
                    ok = ~((u < 0) | (u > 1))
                    q = _cross(s, e1[ti])
                    v = f * _dot(d[r], q)
                    ok &= ~((v < 0) | (u + v > 1))
                    t = f * _dot(e2[ti], q)
                    ok &= (t > DELTA) & (t < best_t[r])
                    rr = r[ok]
                    best_i[rr] = ti[ok]
                    best_t[rr] = t[ok]
                    bu[rr] = u[ok]
                    bv[rr] = v[ok]
    return {"tri": best_i, "t": best_t, "u": bu, "v": bv, "nan_slab": nan_slab, "zero_a": zero_a, "box_tests": box_tests,
            "tri_tests": tri_tests, "tested": seen}


def below_threshold(o, d, triangles):
    """Per ray: some triangle passes the u, v tests of the walk's triangle test (float32) with 0 < t <= DELTA -- a hit that only the
    `t > DELTA` rule rejects; and the same with t == DELTA exactly."""
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    v0 = triangles["v0"][:, :3].astype(f32)
    e1 = triangles["v1"][:, :3].astype(f32) - v0
    e2 = triangles["v2"][:, :3].astype(f32) - v0
    below, at = np.zeros(len(o), bool), np.zeros(len(o), bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for x in range(len(v0)):
            h = _cross(d, e2[x])
            f = f32(1.0) / _dot(e1[x], h)
            s = o - v0[x]
            u = f * _dot(s, h)
            q = _cross(s, e1[x])
            v = f * _dot(d, q)
            t = f * _dot(e2[x], q)
            inside = ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1))
            below |= inside & (t > 0) & ~(t > DELTA)
            at |= inside & (t == DELTA)
    return below, at


def tied(o, d, triangles, best_t):
    """(n_rays, n_triangles) bool: the triangle test of the walk (visibility_reference.tri_hit, float32) accepts the triangle at
    exactly best_t's bits.  All False for a ray without a hit."""
    from visibility_reference import tri_hit
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    v0 = triangles["v0"][:, :3].astype(f32)
    e1 = triangles["v1"][:, :3].astype(f32) - v0
    e2 = triangles["v2"][:, :3].astype(f32) - v0
    out = np.zeros((len(o), len(v0)), bool)
    want = np.asarray(best_t, f32).view(np.uint32)
    has = np.isfinite(best_t)
    for x in range(len(v0)):
        ok, t = tri_hit(o, d, v0[x], e1[x], e2[x])
        out[:, x] = ok & has & (t.view(np.uint32) == want)
    return out
