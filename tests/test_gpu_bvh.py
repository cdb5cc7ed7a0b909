"""GPU BVH builder (csrc/bvh_builder_gpu.hip): a PLOC tree (round 3; the round-2 LBVH behind
CLIVE2_GPU_BVH=lbvh) emitted in the reference's flattened
Box[] / Triangle[] convention (np_flatten_bvh, src/bvh.py:329-389).  The tree differs from the reference's SAH tree,
so parity is checked the way the tracer is: render on the GPU-built tree and compare with the oracle (the reference's
stack walk, trace.metal:144-176) run on the SAME Box[]."""
import time

import numpy as np
import pytest

from tree_reference import pending_depths

pytestmark = pytest.mark.gpu
LIGHT, CAMERA = 0, 1


def _check_convention(scene, max_members=8):
    """What np_flatten_bvh guarantees and cl2_upload_scene / the reference's traversal rely on."""
    b, t = scene.boxes, scene.triangles
    nb, nt = len(b), len(t)
    inner = b["right"] == 0
    left = b["left"]
    # breadth-first numbering: children behind their parent, adjacent, every box referenced exactly once
    kids = np.concatenate([left[inner], left[inner] + 1])
    assert (left[inner] > np.flatnonzero(inner)).all() and kids.max() == nb - 1
    assert np.array_equal(np.sort(kids), np.arange(1, nb))
    assert np.array_equal(left[inner], np.sort(left[inner]))            # queue order: parents in index order
    # leaves: consecutive ranges in index order covering every triangle once, at most max_members each
    lf = ~inner
    sizes = b["right"][lf] - b["left"][lf]
    assert (sizes >= 1).all() and (sizes <= max_members).all() and sizes.sum() == nt
    assert np.array_equal(b["left"][lf], np.concatenate([[0], np.cumsum(sizes)[:-1]]))
    # every leaf box bounds the float32 vertices of its triangles, tightly
    verts = np.stack([t["v0"][:, :3], t["v1"][:, :3], t["v2"][:, :3]], axis=1)           # (nt, 3, 3)
    starts = b["left"][lf]
    lo = np.minimum.reduceat(verts.min(axis=1), starts)
    hi = np.maximum.reduceat(verts.max(axis=1), starts)
    assert np.array_equal(lo, b["min"][lf][:, :3]) and np.array_equal(hi, b["max"][lf][:, :3])
    # every inner box is exactly the union of its two children
    li = left[inner]
    assert np.array_equal(np.minimum(b["min"][li], b["min"][li + 1])[:, :3], b["min"][inner][:, :3])
    assert np.array_equal(np.maximum(b["max"][li], b["max"][li + 1])[:, :3], b["max"][inner][:, :3])
    # the reference's traversal stack: entries pending under each box (left+1 is popped first)
    pending = pending_depths(b)
    assert pending.max() + 2 <= np.log2(max(nt, 2)) + 3                   # smaller subtree first: O(log n), far below 64
    return pending.max()


def _scene(specs, w, h, builder):
    import clive2_amd as c2
    from clive2_amd.load import get_materials
    mats = get_materials()
    mats["alpha"][5] = 0.1
    return c2.create_scene(w, h, np.array([0, 1.5, 6]), np.array([0, 0, -1]), file_specs=specs, materials=mats,
                           bvh_builder=builder)


def test_gpu_built_tree_follows_the_convention_and_renders_like_the_oracle(oracle_mod):
    from clive2_amd.meshes import icosphere, noisy_blob
    from clive2_amd.renderer import Renderer, make_seeds
    specs = [dict(mesh=icosphere(3, radius=2.0, center=(0.0, 1.0, 0.0)), material=5),
             dict(mesh=noisy_blob(subdiv=2, radius=1.0, center=(-3.0, -2.0, 1.0)), material=0)]
    scene = _scene(specs, 64, 48, "gpu")
    assert len(scene.triangles) == 16 + 1280 + 320
    _check_convention(scene)
    # same triangles as the host builders produce, in another order
    ref = _scene(specs, 64, 48, "numpy")
    key = lambda t: np.sort(np.ascontiguousarray(t).view(np.uint8).reshape(len(t), -1).view([("", np.uint8, t.dtype.itemsize)]).reshape(-1))
    assert np.array_equal(key(scene.triangles), key(ref.triangles))
    assert np.array_equal(scene.boxes["min"][0], ref.boxes["min"][0]) and np.array_equal(scene.boxes["max"][0], ref.boxes["max"][0])
    seeds = make_seeds(64 * 48)
    r, o = Renderer(scene, seeds=seeds), oracle_mod.OracleRenderer(scene, seeds=seeds)
    for x in (r, o):
        x.make_light_rays(); x.make_camera_rays(); x.trace_light_rays(); x.trace_camera_rays()
    for which, want in ((LIGHT, o.out_light_paths), (CAMERA, o.out_camera_paths)):
        assert r.export_paths(which).tobytes() == want.tobytes()
    for x in (r, o):
        x.join_paths(); x.finalize_samples(); x.gather_light_image(); x.process_images()
    agg = r.export_aggregators()
    assert agg["total_contribution"].tobytes() == o.weight_aggregators["total_contribution"].tobytes()
    assert agg["weights"].tobytes() == o.weight_aggregators["weights"].tobytes()
    r.run_samples(2); o.run_sample(); o.run_sample()
    assert np.array_equal(r.get_random_buffer(), o.rand_buffer) and r.counters()["rays"] == o.rays_traced
    np.testing.assert_allclose(r.read_accumulators()[0], o.summed_image, rtol=5e-5, atol=1e-8)
    # the picture does not depend on the tree: a render on the SAH tree converges to the same image
    a, b = Renderer(scene), Renderer(ref)
    a.run_samples(64); b.run_samples(64)
    ra, rb = a.radiance, b.radiance
    assert abs(ra.mean() - rb.mean()) < 0.03 * rb.mean()


def test_gpu_builder_edge_cases():
    import ctypes as C
    from clive2_amd import _native, struct_types as st
    L = _native.lib()
    L.cl2_build_bvh_gpu.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                    C.POINTER(C.c_int64), C.c_void_p]

    def build(lo, hi, members=8, cap=None):
        n = len(lo)
        boxes = np.zeros(cap if cap is not None else 2 * n, st.Box)
        perm = np.full(n, -1, np.int64)
        nb = C.c_int64(0)
        rc = L.cl2_build_bvh_gpu(0, _native.ptr(np.ascontiguousarray(lo, np.float64)), _native.ptr(np.ascontiguousarray(hi, np.float64)),
                                 n, members, _native.ptr(boxes), len(boxes), C.byref(nb), _native.ptr(perm))
        return rc, boxes[:nb.value], perm
    rng = np.random.RandomState(3)
    # one triangle; fewer than a leaf holds; exactly one more
    for n in (1, 5, 8, 9):
        lo = rng.rand(n, 3); hi = lo + rng.rand(n, 3) * 0.1
        rc, boxes, perm = build(lo, hi)
        assert rc == 0 and np.array_equal(np.sort(perm), np.arange(n))
        assert (len(boxes) == 1) == (n <= 8)
        assert np.array_equal(boxes["min"][0][:3], lo.min(axis=0).astype(np.float32))
    # all centroids equal (every Morton key the same): the tie-break by position still builds a tree
    lo = np.tile(np.array([[0.25, 0.5, 0.75]]), (100, 1)); hi = lo + 0.5
    rc, boxes, perm = build(lo, hi)
    assert rc == 0 and np.array_equal(np.sort(perm), np.arange(100)) and len(boxes) > 13
    # one triangle per leaf, and error codes: capacity too small, bad arguments
    lo = rng.rand(64, 3); hi = lo + 0.01
    rc, boxes, perm = build(lo, hi, members=1)
    assert rc == 0 and len(boxes) == 127
    rc, _, _ = build(lo, hi, members=1, cap=10)
    assert rc < 0 and b"capacity" in L.cl2_last_error(None)
    assert L.cl2_build_bvh_gpu(99, None, None, 4, 8, None, 0, None, None) < 0


def test_gpu_builder_on_the_million_triangle_scene(oracle_mod):
    """Config-5 stand-in (1,003,536 triangles): the GPU builder's tree renders bit for bit like the oracle on the same
    Box[]; the build itself takes a fraction of a second (the host SAH builder: seconds; the reference: minutes)."""
    import ctypes as C
    from clive2_amd import meshes, _native, struct_types as st
    from clive2_amd.renderer import Renderer, make_seeds
    specs = [dict(mesh=(v, f), material=m) for v, f, m in meshes.interior_grid()]
    t0 = time.perf_counter()
    scene = _scene(specs, 96, 54, "gpu")
    t_scene = time.perf_counter() - t0
    assert len(scene.triangles) == 16 + 49 * 20480
    deepest = _check_convention(scene)
    # the builder alone, on the arrays create_scene hands it
    verts = np.stack([scene.triangles["v0"][:, :3], scene.triangles["v1"][:, :3], scene.triangles["v2"][:, :3]], axis=1).astype(np.float64)
    lo, hi = np.ascontiguousarray(verts.min(axis=1)), np.ascontiguousarray(verts.max(axis=1))
    n = len(lo)
    boxes, perm, nb = np.zeros(2 * n, st.Box), np.zeros(n, np.int64), C.c_int64(0)
    L = _native.lib()
    L.cl2_build_bvh_gpu.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                    C.POINTER(C.c_int64), C.c_void_p]
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        assert L.cl2_build_bvh_gpu(0, _native.ptr(lo), _native.ptr(hi), n, 8, _native.ptr(boxes), len(boxes), C.byref(nb), _native.ptr(perm)) == 0
        best = min(best, time.perf_counter() - t0)
    print(f"\nGPU PLOC build of {n} triangles: {best * 1e3:.0f} ms, {nb.value} boxes, deepest pending {deepest}; create_scene {t_scene:.2f} s")
    assert best < 0.25                       # 53 ms measured ("build call still < 0.1 s"); slack for a busy box
    seeds = make_seeds(96 * 54)
    r, o = Renderer(scene, seeds=seeds), oracle_mod.OracleRenderer(scene, seeds=seeds)
    for x in (r, o):
        x.make_light_rays(); x.make_camera_rays(); x.trace_light_rays(); x.trace_camera_rays()
    for which, want in ((LIGHT, o.out_light_paths), (CAMERA, o.out_camera_paths)):
        assert r.export_paths(which).tobytes() == want.tobytes()
    for x in (r, o):
        x.join_paths(); x.finalize_samples(); x.gather_light_image(); x.process_images()
    assert r.export_aggregators()["total_contribution"].tobytes() == o.weight_aggregators["total_contribution"].tobytes()
    assert r.counters()["rays"] == o.rays_traced
    np.testing.assert_allclose(r.read_accumulators()[0], o.summed_image, rtol=5e-5, atol=1e-8)


def test_ploc_tree_costs_fewer_tests_than_the_radix_tree(monkeypatch):
    """the quality of the GPU-built tree.  Same scene, same rays (same seeds): the PLOC tree needs fewer node
    tests AND fewer triangle tests per ray than the round-2 LBVH (1080p: 68.1 + 18.0 against 75.5 + 24.0; the host SAH tree:
    57.9 + 23.0 -- and renders a sample in the same time as the SAH tree, 31.4 ms, where the LBVH took 35.0)."""
    from clive2_amd import meshes
    from clive2_amd.renderer import Renderer, make_seeds
    specs = [dict(mesh=(v, f), material=m) for v, f, m in meshes.interior_grid()]
    tests = {}
    for method in ("lbvh", "ploc"):
        monkeypatch.setenv("CLIVE2_GPU_BVH", method)
        scene = _scene(specs, 96, 54, "gpu")
        _check_convention(scene)
        r = Renderer(scene, seeds=make_seeds(96 * 54))
        r.set_counting(True)
        r.run_samples(2)
        c = r.counters()
        tests[method] = (c["box_tests"] / c["counted_rays"], c["tri_tests"] / c["counted_rays"], len(scene.boxes))
        r.close()
    print("\nnode / triangle tests per ray, boxes:", tests)
    assert tests["ploc"][0] < 0.95 * tests["lbvh"][0] and tests["ploc"][1] < 0.9 * tests["lbvh"][1]
    assert tests["ploc"][2] != tests["lbvh"][2]          # two different trees were really built


def test_ploc_builder_survives_coincident_triangles():
    """Every round of PLOC merges at least the pair with the smallest (area, position, position) key; a soup of identical
    boxes merges ONE pair per round, so past a cap of rounds the builder falls back to the radix tree.  Either way the
    result is a valid tree."""
    import ctypes as C
    from clive2_amd import _native, struct_types as st
    L = _native.lib()
    L.cl2_build_bvh_gpu.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                    C.POINTER(C.c_int64), C.c_void_p]
    for n in (40, 3000):                                  # below / above the cap of rounds
        lo = np.tile(np.array([[0.25, 0.5, 0.75]]), (n, 1)); hi = lo + 0.5
        boxes, perm, nb = np.zeros(2 * n, st.Box), np.full(n, -1, np.int64), C.c_int64(0)
        assert L.cl2_build_bvh_gpu(0, _native.ptr(lo), _native.ptr(hi), n, 8, _native.ptr(boxes), len(boxes), C.byref(nb), _native.ptr(perm)) == 0
        assert np.array_equal(np.sort(perm), np.arange(n))
        b = boxes[:nb.value]
        leaves = b[b["right"] != 0]
        assert (leaves["right"] - leaves["left"]).sum() == n and (leaves["right"] - leaves["left"]).max() <= 8


def test_ploc_falls_back_when_no_union_area_is_finite():
    """boxes so large that every union area overflows float32 (+inf) give no cluster a nearest neighbour, so a
    PLOC round merges nothing.  That is not an error of the input: the radix tree (which needs no areas) is built."""
    import ctypes as C
    from clive2_amd import _native, struct_types as st
    L = _native.lib()
    L.cl2_build_bvh_gpu.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                    C.POINTER(C.c_int64), C.c_void_p]
    rng = np.random.RandomState(11)
    n = 500
    lo = rng.rand(n, 3) * 1e25; hi = lo + rng.rand(n, 3) * 1e24
    boxes, perm, nb = np.zeros(2 * n, st.Box), np.full(n, -1, np.int64), C.c_int64(0)
    rc = L.cl2_build_bvh_gpu(0, _native.ptr(lo), _native.ptr(hi), n, 8, _native.ptr(boxes), len(boxes), C.byref(nb), _native.ptr(perm))
    assert rc == 0, L.cl2_last_error(None)
    assert np.array_equal(np.sort(perm), np.arange(n))
    b = boxes[:nb.value]
    leaves = b[b["right"] != 0]
    assert (leaves["right"] - leaves["left"]).sum() == n and (leaves["right"] - leaves["left"]).max() <= 8
