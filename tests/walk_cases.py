"""Adversarial scenes and rays of the walk tests (tests/test_walk_cases_cpu.py, tests/test_gpu_walk_cases.py): inputs built to sit on
the decisions of the closest-hit walks -- the slab test's NaN and `tmin <= tmax` cases, the triangle test's `u`, `v`, `u + v` and
`t > DELTA` bounds, exact-t ties between records of different leaves -- instead of the rays a render happens to generate.  Everything
is deterministic and float32.

Scenes (the Cornell room plus one mesh of material MESH_MATERIAL, 32 x 18):

    tiny       7 mesh triangles: the unit triangle and its copy, a half of each of two coplanar overlapping plates and its copy, one
               zero-area triangle: the pruned table is a flat list of leaves
    lds        half a noisy icosphere of subdivision 2 (open side up), adversarial(): 250-450 triangles, tree and triangles in LDS
    streamed   the same of subdivision 3: 1,200-2,000 triangles, the tree streams from memory, 4-wide collapse

adversarial(v, f) appends to a mesh: the unit triangle UNIT (dyadic coordinates: the `exact` rays compute u, v, t without rounding),
two coplanar overlapping axis-aligned plates, two zero-area triangles (three equal vertices; three collinear ones), two slivers (one
vertex 1e-6 off an edge) -- and then EVERY face a second time behind the originals: each hit is an exact-t tie of two records.  The
builders sort coincident triangles side by side, so most pairs share a leaf; three stacks (nine, nine and three copies of one face)
are more than a leaf's eight and are cut, which also gives leaves of odd size.  Ties between leaves come from them and from the
vertices and edges the faces share (the `aimed` rays).  coincident(scene) / twin(scene) name each triangle's copies.

Ray classes: {name: (origins, directions)}, see ray_sets(); arranged() concatenates them in three orders."""
import functools

import numpy as np

f32 = np.float32
MESH_MATERIAL = 5
W, H = 32, 18
DELTA = f32(0.0001)                                      # trace.metal:5
ORIGINS = ([0.0, 1.5, 6.0], [3.5, 4.0, 3.0], [-3.0, 0.5, -3.5], [0.25, 8.5, 0.5])      # the four origins of test_gpu_round6.py
ROOM_LO, ROOM_HI = np.array([-10, -2, -10], f32), np.array([10, 10, 10], f32)
UNIT = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1]], np.float64) + np.array([4.0, 0.0, 4.0])     # v0, v1, v2: e1 = x, e2 = z, y = 0
PLATE_Y = -1.0
PLATES = (((3.0, -5.0), (6.0, -2.0)), ((4.5, -3.5), (7.5, -0.5)))                           # (x, z) corners; they overlap


def _quad(x0, z0, x1, z1, y):
    return np.array([[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]], np.float64), np.array([[0, 1, 2], [0, 2, 3]])


def extras():
    """(vertices, faces) of the hand-made triangles: UNIT, the plates, the zero-area triangles, the slivers."""
    vs, fs = [UNIT], [np.array([[0, 1, 2]])]
    for (x0, z0), (x1, z1) in PLATES:
        v, f = _quad(x0, z0, x1, z1, PLATE_Y)
        fs.append(f + sum(len(x) for x in vs)); vs.append(v)
    point = np.array([[-5.0, 3.0, 2.0]] * 3)                                       # three equal vertices
    line = np.array([[-6.0, 1.0, -4.0], [-5.0, 1.5, -3.0], [-4.0, 2.0, -2.0]])     # three collinear ones
    sliver_a = np.array([[-4.0, 0.5, 2.0], [-3.0, 0.5, 2.0], [-3.5, 0.5 + 1e-6, 2.0]])
    sliver_b = np.array([[6.0, 4.0, -6.0], [6.0, 6.0, -4.0], [6.0 + 1e-6, 5.0, -5.0]])
    for v in (point, line, sliver_a, sliver_b):
        fs.append(np.array([[0, 1, 2]]) + sum(len(x) for x in vs)); vs.append(v)
    return np.concatenate(vs), np.concatenate(fs)


def adversarial(v, f, duplicate=True):
    ev, ef = extras()
    n = len(f)
    v, f = np.concatenate([v, ev]), np.concatenate([f, ef + len(v)])
    if not duplicate:
        return v, f
    # the builders keep coincident copies side by side, so most pairs share a leaf; a stack of nine copies is more than a leaf holds
    # (8) and has to be cut: face 0 of the mesh and the last sliver nine times each, UNIT three times
    return v, np.concatenate([f, f, np.repeat(f[[0]], 7, axis=0), f[[n]], np.repeat(f[[-1]], 7, axis=0)])


def half_blob(sub):
    """The faces of a noisy icosphere (radius 2 about (0, 1.2, 0)) whose centroid lies below its centre: a bowl, open side up."""
    from clive2_amd.meshes import noisy_blob
    v, f = noisy_blob(sub, radius=2.0, center=(0.0, 1.2, 0.0), amplitude=0.08, seed=7)
    keep = v[f][:, :, 1].mean(axis=1) < 1.2
    return v, f[keep]


def tiny_mesh():
    ev, ef = extras()
    # UNIT twice, a half of each plate twice, the zero-area triangle of three equal vertices: seven triangles.  (With the collinear
    # one or a sliver as an eighth the builder's tree keeps an inner box in the pruned table: it is no flat list of leaves.)
    return ev, ef[[0, 0, 1, 3, 1, 3, 5]]


@functools.lru_cache(maxsize=None)
def scene(name, builder="numpy", duplicate=True, open_room=False):
    """`name` in tiny / lds / streamed; `duplicate` False: every face once (the float64 check's scenes); `open_room`: without the
    front and the right wall (rays can miss everything)."""
    import clive2_amd as c2
    from clive2_amd.load import get_materials, triangles_for_box
    mats = get_materials()
    mats["alpha"][MESH_MATERIAL] = 0.1
    if name == "tiny":
        v, f = tiny_mesh()
        if not duplicate:
            f = f[[0, 2, 3, 6]]
    else:
        v, f = adversarial(*half_blob({"lds": 2, "streamed": 3}[name]), duplicate=duplicate)
    room = None
    if open_room:
        walls = triangles_for_box()
        room = walls[:4] + walls[8:]                                               # 4, 5: right wall; 6, 7: front wall
    return c2.create_scene(W, H, np.array([0, 1.5, 6]), np.array([0, 0, -1]), file_specs=[dict(mesh=(v, f), material=MESH_MATERIAL)],
                           materials=mats, bvh_builder=builder, room=room)


def corners(sc):
    t = sc.triangles
    return np.stack([t[k][:, :3].astype(f32) for k in ("v0", "v1", "v2")], axis=1)          # (n, 3, 3)


def coincident(sc):
    """group[i]: equal for triangles with the same three vertices in the same order, and only for them."""
    c = corners(sc).reshape(len(sc.triangles), 9)
    return np.unique(c, axis=0, return_inverse=True)[1].reshape(-1)


def twin(sc):
    """twin[i] = the other triangle with i's three vertices in i's order where there is exactly one, else -1."""
    inverse = coincident(sc)
    counts = np.bincount(inverse)
    out = np.full(len(inverse), -1, np.int64)
    order = np.argsort(inverse, kind="stable")
    for a, b in zip(order[:-1], order[1:]):
        if inverse[a] == inverse[b] and counts[inverse[a]] == 2:
            out[a], out[b] = b, a
    return out


def make_rays(o, d):
    """Ray records with inv_direction = 1 / d in float32 (what the oracle reads; the device's probes compute it from d)."""
    from clive2_amd import struct_types as st
    rays = np.zeros(len(o), dtype=st.Ray)
    rays["origin"][:, :3] = o
    rays["direction"][:, :3] = d
    with np.errstate(divide="ignore", over="ignore"):
        rays["inv_direction"][:, :3] = f32(1.0) / np.asarray(d, f32)
    return rays


def _unit(d):
    d = np.asarray(d, f32)
    return (d / np.sqrt((d * d).sum(axis=1, dtype=f32))[:, None]).astype(f32)


def _room_points(rng, n, margin=0.5):
    return rng.uniform(ROOM_LO + f32(margin), ROOM_HI - f32(margin), (n, 3)).astype(f32)


# ---- the classes ----
def ordinary(n, seed):
    """Uniform origins in the room, uniform directions, all three components non-zero: the control, and the float64 check's rays."""
    rng = np.random.default_rng(seed)
    d = _unit(rng.normal(size=(n, 3)))
    assert (d != 0).all()
    return _room_points(rng, n), d


def axis(sc, n=1536, seed=21):
    """One or two direction components exactly zero, +0.0 and -0.0 alike (1 / d = +inf, -inf).  A third of the origins take the
    coordinate of a zero axis from a box's min or max: (lo - o) * inv = 0 * inf = NaN in that slab.  Every 16th origin is a box corner."""
    rng = np.random.default_rng(seed)
    o = _room_points(rng, n)
    d = _unit(rng.normal(size=(n, 3)))
    zero = np.array([f32(0.0), -f32(0.0)])
    b = sc.boxes
    lo, hi = b["min"][:, :3].astype(f32), b["max"][:, :3].astype(f32)
    for j in range(n):
        k = j % 3
        if j % 2:                                                                  # two zero components: the ray runs along axis k
            d[j] = zero[rng.integers(0, 2, 3)]
            d[j, k] = f32(1.0) if j % 4 == 1 else f32(-1.0)
            zeros = [a for a in range(3) if a != k]
        else:
            d[j, k] = zero[rng.integers(0, 2)]
            d[j] = _unit(d[j:j + 1])[0]
            d[j, k] = zero[rng.integers(0, 2)]
            zeros = [k]
        box = rng.integers(0, len(b))
        if j % 3 == 0:
            for a in zeros:
                o[j, a] = (lo, hi)[rng.integers(0, 2)][box, a]
        if j % 16 == 0:
            o[j] = (lo, hi)[rng.integers(0, 2)][box]
    return o, d


def in_plane(sc, n=768, seed=22):
    """Rays that lie in the plane of axis-aligned triangles: on the floor and in the plane of the plates with d.y = +-0, on the left
    and the back wall likewise: a = 0 exactly, f = +-inf, u = NaN for every triangle of that plane.  Half of the plate-plane rays
    start inside a plate."""
    rng = np.random.default_rng(seed)
    o = _room_points(rng, n)
    d = _unit(rng.normal(size=(n, 3)))
    zero = np.array([f32(0.0), -f32(0.0)])
    planes = ((1, ROOM_LO[1]), (1, f32(PLATE_Y)), (0, ROOM_LO[0]), (2, ROOM_LO[2]))
    for j in range(n):
        a, x = planes[j % 4]
        d[j, a] = 0
        d[j] = _unit(d[j:j + 1])[0]
        d[j, a] = zero[(j // 4) % 2]
        o[j, a] = x
        if j % 8 == 1:
            (x0, z0), (x1, z1) = PLATES[(j // 8) % 2]
            o[j, 0], o[j, 2] = rng.uniform(x0, x1), rng.uniform(z0, z1)
    return o, d


def aimed(sc, material=MESH_MATERIAL):
    """From each of ORIGINS at every vertex, edge midpoint and centroid of the mesh (wide_stack_cases.aimed_rays plus the centroids):
    with every face doubled, two to twelve records tie at one t."""
    c = corners(sc)[sc.triangles["material"] == material]
    a, b, cc = c[:, 0], c[:, 1], c[:, 2]
    targets = np.unique(np.concatenate([a, b, cc, (a + b) / 2, (b + cc) / 2, (cc + a) / 2, (a + b + cc) / f32(3)]).astype(f32), axis=0)
    os_, ds = [], []
    for origin in ORIGINS:
        o = np.broadcast_to(np.asarray(origin, f32), targets.shape).copy()
        with np.errstate(invalid="ignore", divide="ignore"):
            d = _unit((targets - o).astype(f32))
        keep = (d != 0).all(axis=1) & np.isfinite(d).all(axis=1)
        os_.append(o[keep]); ds.append(d[keep])
    return np.ascontiguousarray(np.concatenate(os_)), np.ascontiguousarray(np.concatenate(ds))


EXACT_DIRS = np.array([[0.25, -0.5, 0.25], [-0.25, -0.5, 0.5], [0.5, -0.5, -0.25], [-0.125, -0.5, -0.125],
                       [0.25, 0.5, 0.25], [-0.5, 0.5, 0.125]], f32)
EXACT_POINTS = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1], [0.5, 0, 0], [0, 0, 0.5], [0.5, 0, 0.5], [0.25, 0, 0.75], [0.75, 0, 0.25],
                         [0.25, 0, 0.25], [0.125, 0, 0.5]], f32)


def exact():
    """Rays at UNIT whose u, v and t come out without a rounding error (dyadic numbers; d.y = +-0.5, so f = +-2): the hit points are
    the vertices (u, v = (0, 0), (1, 0), (0, 1)), points of all three edges (u = 0, v = 0, u + v = 1 exactly) and inner points, each
    from t = 0.5 and t = 2; and over the inner points t = DELTA itself and its two float32 neighbours (origin at DELTA / 2 above or
    below the plane).  Directions are not normalised."""
    v0 = UNIT[0].astype(f32)
    os_, ds = [], []
    for d in EXACT_DIRS:
        for p in EXACT_POINTS:
            for t in (f32(0.5), f32(2.0)):
                os_.append(v0 + p - t * d); ds.append(d)
        for p in EXACT_POINTS[8:]:
            for t in (DELTA, np.nextafter(DELTA, f32(0)), np.nextafter(DELTA, f32(1))):
                o = (v0 + p).astype(f32)
                o[1] = -(t * d[1])                                                 # exact: d.y = +-0.5; o.x, o.z stay on the hit point:
                os_.append(o); ds.append(d * np.array([0, 1, 0], f32) + np.array([2.0 ** -30, 0, 2.0 ** -30], f32))
    return np.array(os_, f32), np.array(ds, f32)


def delta(sc, per_triangle=12, seed=23):
    """Hits at t = DELTA (1 +- 2^-k), k = 1..23, and at DELTA, as nearly as float32 allows: the origin stepped back from a triangle's
    centroid along a direction through it; and origins exactly on a triangle (t = 0: the ray must leave it).  Over the mesh's
    triangles nearest the origin of coordinates (small coordinates: finer steps), the walls and exact()."""
    rng = np.random.default_rng(seed)
    c = corners(sc).astype(np.float64)
    cen = c.mean(axis=1)
    n = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    ok = np.linalg.norm(n, axis=1) > 1e-3
    pick = np.flatnonzero(ok)[np.argsort(np.abs(cen[ok]).max(axis=1), kind="stable")][:per_triangle * 3:3]
    pick = np.concatenate([pick, np.flatnonzero(ok & (sc.triangles["material"] != MESH_MATERIAL))[:6]])
    ts = [1.0] + [1.0 + s * 2.0 ** -k for k in range(1, 24) for s in (1, -1)] + [0.0]
    os_, ds = [], []
    for i in pick:
        nn = n[i] / np.linalg.norm(n[i])
        d = nn + 0.3 * rng.normal(size=3)
        d /= np.linalg.norm(d)
        for t in ts:
            os_.append(cen[i] - d * (t * float(DELTA))); ds.append(d)
    eo, ed = exact()
    o, d = np.concatenate([np.array(os_).astype(f32), eo]), np.concatenate([np.array(ds).astype(f32), ed])
    assert (d != 0).all()
    return o, d


def tiny_inverse(n=768, seed=24):
    """Direction components whose reciprocal leaves rcp_exact's fast window (exponent field of d outside [1, 252]): subnormals whose
    reciprocal overflows to inf (below 2^-128) and those whose reciprocal is finite (2^-127, 2^-128 .. : 1 / d up to 2^127 * ..), the
    smallest normals, and components of 2^126 and more (1 / d subnormal); and unnormalised directions of length 2^-20 and 2^20."""
    rng = np.random.default_rng(seed)
    o = _room_points(rng, n)
    d = _unit(rng.normal(size=(n, 3)))
    small = np.array([2.0 ** -149, 2.0 ** -140, 1e-40, 2.0 ** -129, 2.0 ** -128, 1.5 * 2.0 ** -128, 2.0 ** -127, 1.75 * 2.0 ** -127,
                      2.0 ** -126, 1.5 * 2.0 ** -126, 2.0 ** -125], np.float64).astype(f32)
    for j in range(n):
        kind = j % 4
        if kind == 0:                                                              # one tiny component
            d[j, j % 3] = small[(j // 4) % len(small)] * (1 if (j // 44) % 2 else -1)
        elif kind == 1:                                                            # two tiny components
            d[j, j % 3] = small[(j // 4) % len(small)]
            d[j, (j + 1) % 3] = -small[(j // 8) % len(small)]
        elif kind == 2:
            d[j] = d[j] * f32(2.0 ** (-20 if (j // 4) % 2 else 20))
        else:                                                                      # the whole direction scaled to the top of the range
            d[j] = d[j] * f32(2.0 ** (126 if (j // 4) % 2 else 127))
    assert np.isfinite(d).all() and (d != 0).all()
    return o, d


def outside(sc, n=768, seed=25):
    """Origins outside the root box: pointing at it, away from it, and grazing a face of it (the origin in the face's plane beyond an
    edge, the direction in that plane -- or a hair off it)."""
    rng = np.random.default_rng(seed)
    lo, hi = sc.boxes["min"][0, :3].astype(f32), sc.boxes["max"][0, :3].astype(f32)
    o = np.empty((n, 3), f32)
    d = np.empty((n, 3), f32)
    for j in range(n):
        a = j % 3
        side = (j // 3) % 2
        p = rng.uniform(lo, hi).astype(f32)
        target = rng.uniform(lo * f32(0.8), hi * f32(0.8)).astype(f32)
        p[a] = hi[a] + f32(rng.uniform(0.5, 30)) if side else lo[a] - f32(rng.uniform(0.5, 30))
        kind = (j // 6) % 3
        if kind == 0:
            o[j], d[j] = p, _unit((target - p)[None])[0]
        elif kind == 1:
            o[j], d[j] = p, _unit((p - target)[None])[0]
        else:                                                                      # grazing the face `b` of the root box
            b = (a + 1) % 3
            p[b] = hi[b] if (j // 18) % 2 else lo[b]
            t = target.copy(); t[b] = p[b]
            dd = _unit((t - p)[None])[0]
            dd[b] = f32(0.0) if (j // 36) % 2 else f32(1e-7 * (1 if (j // 72) % 2 else -1))
            o[j], d[j] = p, dd
    return o, d


ORDER = ("ordinary", "axis", "in_plane", "aimed", "delta", "tiny_inverse", "outside")


def ray_sets(sc, ordinary_n=4096, seed=11):
    return {"ordinary": ordinary(ordinary_n, seed), "axis": axis(sc), "in_plane": in_plane(sc), "aimed": aimed(sc), "delta": delta(sc),
            "tiny_inverse": tiny_inverse(), "outside": outside(sc)}


def arranged(sets, how):
    """(origins, directions, perm, spans): every class of `sets` concatenated; ray j of the arrangement is ray perm[j] of the grouped
    one (result_grouped[perm] = result_arranged), spans = {class: slice} of the GROUPED array.

        grouped       class after class
        reversed      the grouped array back to front
        interleaved   waves of 64 consecutive rays: each of the first waves holds ONE ray of axis / in_plane / tiny_inverse (at lane
                      (5 w) mod 64) among 63 ordinary ones, as long as both last; the next ones are 64 ordinary rays (all-finite
                      waves) as long as those last; the remaining rays follow in a fixed stride permutation"""
    names = [k for k in ORDER if k in sets]
    o = np.concatenate([sets[k][0] for k in names]).astype(f32)
    d = np.concatenate([sets[k][1] for k in names]).astype(f32)
    spans, at = {}, 0
    for k in names:
        spans[k] = slice(at, at + len(sets[k][0])); at += len(sets[k][0])
    n = len(o)
    if how == "grouped":
        perm = np.arange(n)
    elif how == "reversed":
        perm = np.arange(n)[::-1].copy()
    elif how == "interleaved":
        plain = list(range(spans["ordinary"].start, spans["ordinary"].stop))
        odd = [j for k in ("axis", "in_plane", "tiny_inverse") if k in spans for j in range(spans[k].start, spans[k].stop)]
        odd = odd[::7]                                                             # some of them; the others go to the strided rest
        half = len(plain) // 2
        mixed_waves = min(len(odd), half // 63)
        perm, used = [], set()
        for w in range(mixed_waves):
            wave = plain[63 * w:63 * (w + 1)]
            wave.insert((5 * w) % 64, odd[w])
            perm += wave
        first_plain = 63 * mixed_waves
        full = (len(plain) - first_plain) // 64
        perm += plain[first_plain:first_plain + 64 * full]
        used.update(perm)
        rest = np.array([j for j in range(n) if j not in used], np.int64)
        stride = 37
        while np.gcd(stride, max(len(rest), 1)) != 1:
            stride += 2
        perm = np.concatenate([np.array(perm, np.int64), rest[(np.arange(len(rest)) * stride) % max(len(rest), 1)]])
    else:
        raise ValueError(how)
    assert np.array_equal(np.sort(perm), np.arange(n))
    return o[perm], d[perm], perm, spans


def back(perm, *arrays):
    """Results of an arrangement in the grouped order."""
    out = []
    for a in arrays:
        g = np.empty_like(a)
        g[perm] = a
        out.append(g)
    return out
