"""Numpy restatement of the seeded visibility query (csrc/bvh_wide.hpp, VIS) -- TEST INFRASTRUCTURE.

A ray (o, d) with finite 1/d has a target triangle T.  hit(X) is the walk's triangle test (ray_triangle_intersect, trace.metal:117-142,
in float32 and in the kernel's order: the operations of oracle/np_kernels.py's traverse, taken from there by import).  The ray is
VISIBLE iff

    hit(T) is ok, with distance t_T, and
    no triangle X != T of an ENTERED leaf is a BLOCKER, where
        a leaf is entered iff its own box passes `tmin <= tmax && tmin <= t_T` (the slab test of trace.metal:150-156), and
        X is a blocker iff hit(X) is ok and (t_X < t_T, or t_X == t_T and rank[X] < rank[T]);

rank[X] = X's position in the reference's visit order (the child at left + 1 first, a leaf's triangles in index order).  Nothing here
walks a tree: every leaf of scene.boxes is tried, whatever its ancestors do, so the verdict is order-free by construction.

Also here: the ray sets of tests/test_visibility_cpu.py (their input check) and tests/test_gpu_visibility.py (the probe), made once
with the C oracle, so that both files see the same rays."""
import functools

import numpy as np

from oracle.np_kernels import DELTA, _cross, _dot, _max, _min, _normalize, f32


def visit_rank(boxes, n_tris=None):
    """rank[t] of every triangle: its position in the reference's visit order (trace.metal:157-160 pushes left, then left + 1: the
    child at left + 1 is popped first)."""
    left, right = boxes["left"].astype(np.int64), boxes["right"].astype(np.int64)
    n_tris = int(right.max()) if n_tris is None else n_tris
    rank = np.full(n_tris, -1, np.int64)
    nxt = 0
    stack = [0]
    while stack:
        b = stack.pop()
        if right[b] == 0:
            stack.append(int(left[b])); stack.append(int(left[b]) + 1)
        else:
            for t in range(int(left[b]), int(right[b])):
                if rank[t] < 0:
                    rank[t] = nxt; nxt += 1
    return rank


def tri_hit(o, d, v0, e1, e2):
    """(ok, t): ray_triangle_intersect against records {v0, v1 - v0, v2 - v0}, one triangle per ray, float32, the kernel's order."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        h = _cross(d, e2)
        a = _dot(e1, h)
        f = f32(1.0) / a
        s = o - v0
        u = f * _dot(s, h)
        ok = ~((u < 0) | (u > 1))
        q = _cross(s, e1)
        v = f * _dot(d, q)
        ok &= ~((v < 0) | (u + v > 1))
        t = f * _dot(e2, q)
        ok &= t > DELTA
    return ok, t.astype(f32)


def slab(o, inv, lo, hi):
    """(tmin, tmax) of one box for every ray: trace.metal:150-156 (MSL min / max)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t0, t1 = (lo - o) * inv, (hi - o) * inv
        tmn, tmx = _min(t0, t1), _max(t0, t1)
        tmin = _max(_max(tmn[:, 0], tmn[:, 1]), _max(tmn[:, 2], f32(0.0)))
        tmax = _min(_min(tmx[:, 0], tmx[:, 1]), _min(tmx[:, 2], f32(np.inf)))
    return tmin, tmax


def visible(scene, origin, direction, targets):
    """The verdict of the definition above for every ray, for one or several target arrays at once (the slab values of a leaf are
    computed once per ray).  targets: (n,) or (k, n) int, every entry a triangle index.  Rays must have finite 1/d."""
    boxes, tris = scene.boxes, scene.triangles
    o, d = np.ascontiguousarray(origin, f32), np.ascontiguousarray(direction, f32)
    T = np.atleast_2d(np.asarray(targets, np.int64))
    n = len(o)
    assert T.shape[1] == n and (T >= 0).all() and (T < len(tris)).all()
    with np.errstate(divide="ignore"):
        inv = (f32(1.0) / d).astype(f32)
    assert np.isfinite(inv).all(), "the definition covers rays with finite 1/d"
    v0 = tris["v0"][:, :3].astype(f32)
    e1 = tris["v1"][:, :3].astype(f32) - v0
    e2 = tris["v2"][:, :3].astype(f32) - v0
    rank = visit_rank(boxes, len(tris))
    out = []
    hits = [tri_hit(o, d, v0[t], e1[t], e2[t]) for t in T]
    blocked = [np.zeros(n, bool) for _ in T]
    bmin, bmax = boxes["min"][:, :3].astype(f32), boxes["max"][:, :3].astype(f32)
    for leaf in np.flatnonzero(boxes["right"] != 0):
        tmin, tmax = slab(o, inv, bmin[leaf], bmax[leaf])
        inside = tmin <= tmax
        for k, t in enumerate(T):
            ok_T, t_T = hits[k]
            idx = np.flatnonzero(inside & ok_T & (tmin <= t_T))          # rays of this target set that enter the leaf
            if len(idx) == 0:
                continue
            for x in range(int(boxes["left"][leaf]), int(boxes["right"][leaf])):
                ok_x, t_x = tri_hit(o[idx], d[idx], v0[x], e1[x], e2[x])
                tt = t_T[idx]
                blk = ok_x & (t[idx] != x) & ((t_x < tt) | ((t_x == tt) & (rank[x] < rank[t[idx]])))
                blocked[k][idx[blk]] = True
    for k in range(len(T)):
        out.append(hits[k][0] & ~blocked[k])
    return out[0] if np.ndim(targets) == 1 else np.stack(out)


# ---- the scene and the ray sets of the probe tests ----
SEED = 20240928          # the default of make_seeds: the pipeline set's seed (tests/test_visibility_cpu.py has the input check)


@functools.lru_cache(maxsize=None)
def glass(subdiv, w, h):
    """Cornell box + rough-glass icosphere (subdivision 3: 1,280 triangles; 4: config-3 geometry)."""
    import clive2_amd as c2
    from clive2_amd.load import get_materials
    from clive2_amd.meshes import icosphere
    mats = get_materials()
    mats["alpha"][5] = 0.1
    v, f = icosphere(subdiv, radius=2.0, center=(0.0, 1.0, 0.0))
    return c2.create_scene(w, h, np.array([0, 1.5, 6]), np.array([0, 0, -1]), file_specs=[dict(mesh=(v, f), material=5)], materials=mats)


def exact_closest_hit(scene, o, d):
    """(triangle, t) of the reference's walk (the C oracle)."""
    from clive2_amd import struct_types as st
    from oracle import oracle as orc
    rays = np.zeros(len(o), dtype=st.Ray)
    rays["origin"][:, :3] = o
    rays["direction"][:, :3] = d
    with np.errstate(divide="ignore"):
        rays["inv_direction"][:, :3] = f32(1.0) / np.asarray(d, f32)
    bi, bt, _, _, _ = orc.traverse(rays, scene.boxes, scene.triangles)
    return bi, bt


def connection_rays(scene, samples=2, seed=SEED):
    """(origin, direction, target) of the t >= 2 connection rays of `samples` samples: light vertex s-1 toward camera vertex t-1, for
    every pair the two subpaths are long enough for; target = the camera vertex's triangle.  From the C oracle's Path[]."""
    from oracle import oracle as orc
    W, H = scene.pixel_width, scene.pixel_height
    r = orc.OracleRenderer(scene, seeds=orc.make_seeds(W * H, seed=seed))
    os_, ds, ts = [], [], []
    for _ in range(samples):
        r.run_sample()
        lp, cp = r.out_light_paths, r.out_camera_paths
        len_l, len_c = lp["length"].astype(np.int32), cp["length"].astype(np.int32)
        o_l = lp["rays"]["origin"][:, :6, :3].astype(f32)
        o_c = cp["rays"]["origin"][:, :6, :3].astype(f32)
        tri_c = cp["rays"]["triangle"][:, :6].astype(np.int32)
        for s in range(1, 7):
            for t in range(2, 7):
                m = (len_l >= s) & (len_c >= t) & (tri_c[:, t - 1] >= 0)
                a, b = o_l[m, s - 1], o_c[m, t - 1]
                v = b - a
                ok = (_dot(v, v) > 0)
                with np.errstate(divide="ignore", invalid="ignore"):
                    dn = _normalize(v[ok]).astype(f32)
                    fin = np.isfinite(f32(1.0) / dn).all(axis=1) & np.isfinite(dn).all(axis=1)
                os_.append(a[ok][fin]); ds.append(dn[fin]); ts.append(tri_c[m, t - 1][ok][fin])
    return np.concatenate(os_), np.concatenate(ds), np.concatenate(ts)


def aimed_rays(scene):
    """Rays from four points of the room AT the vertices and edge midpoints of the mesh (material 5): where two to six triangles meet,
    several are hit at exactly the same t.  Returns (origin, direction, neighbour): neighbour[j] = a triangle that shares the point
    ray j is aimed at, and not the exact closest hit where another sharer exists."""
    t = scene.triangles
    mesh_idx = np.flatnonzero(t["material"] == 5)
    v = [t[k][mesh_idx, :3].astype(f32) for k in ("v0", "v1", "v2")]
    pts = np.concatenate([v[0], v[1], v[2], (v[0] + v[1]) / 2, (v[1] + v[2]) / 2, (v[2] + v[0]) / 2]).astype(f32)
    owner = np.tile(mesh_idx, 6)
    uniq, inv_idx = np.unique(pts, axis=0, return_inverse=True)
    inv_idx = inv_idx.reshape(-1)
    sharers = [[] for _ in range(len(uniq))]
    for p, tri in zip(inv_idx, owner):
        sharers[p].append(int(tri))
    os_, ds = [], []
    for origin in ([0.0, 1.5, 6.0], [3.5, 4.0, 3.0], [-3.0, 0.5, -3.5], [0.25, 8.5, 0.5]):
        o = np.broadcast_to(np.asarray(origin, f32), uniq.shape).copy()
        os_.append(o); ds.append(_normalize((uniq - o).astype(f32)).astype(f32))
    o, d = np.concatenate(os_), np.concatenate(ds)
    with np.errstate(divide="ignore"):
        fin = np.isfinite(f32(1.0) / d).all(axis=1)
    point = np.tile(np.arange(len(uniq)), 4)[fin]
    o, d = o[fin], d[fin]
    hit, _ = exact_closest_hit(scene, o, d)
    neighbour = np.array([next((x for x in sharers[p] if x != h), sharers[p][0]) for p, h in zip(point, hit)], np.int32)
    return o, d, neighbour


@functools.lru_cache(maxsize=None)
def probe_sets():
    """The ray sets a-d of the probe test on the subdivision-3 glass scene at 64 x 36: {name: (origin, direction, target)}, and the
    exact closest hit of every ray {name: triangle}.  Made once per process."""
    scene = glass(3, 64, 36)
    o, d, true_t = connection_rays(scene)
    hit, _ = exact_closest_hit(scene, o, d)
    has = hit >= 0                                          # (a connection ray ends on a surface: every one has a hit)
    rng = np.random.RandomState(7)
    other = ((true_t + 1 + rng.randint(0, len(scene.triangles) - 1, len(true_t))) % len(scene.triangles)).astype(np.int32)
    sets = {"a_true_targets": (o, d, true_t),
            "b_closest_hit": (o[has], d[has], hit[has]),
            "c_random_other": (o, d, other)}
    exact = {"a_true_targets": hit, "b_closest_hit": hit[has], "c_random_other": hit}
    ao, ad, neighbour = aimed_rays(scene)
    ahit, _ = exact_closest_hit(scene, ao, ad)
    ahas = ahit >= 0
    sets["d_aimed_closest_hit"] = (ao[ahas], ad[ahas], ahit[ahas])
    sets["d_aimed_neighbour"] = (ao, ad, neighbour)
    exact["d_aimed_closest_hit"] = ahit[ahas]
    exact["d_aimed_neighbour"] = ahit
    return scene, sets, exact


@functools.lru_cache(maxsize=None)
def probe_verdicts():
    """The restatement's verdict for every ray of probe_sets(): {name: bool array}.  Sets a, b, c share their rays."""
    scene, sets, _ = probe_sets()
    out = {}
    o, d, ta = sets["a_true_targets"]
    tb_full = ta.copy()                                     # b covers the rays with a hit: restate on all, select afterwards
    _, _, exact = probe_sets()
    has = exact["a_true_targets"] >= 0
    tb_full[has] = exact["a_true_targets"][has]
    va, vb, vc = visible(scene, o, d, np.stack([ta, tb_full, sets["c_random_other"][2]]))
    out["a_true_targets"], out["b_closest_hit"], out["c_random_other"] = va, vb[has], vc
    for name in ("d_aimed_closest_hit", "d_aimed_neighbour"):
        o, d, t = sets[name]
        out[name] = visible(scene, o, d, t)
    return out
