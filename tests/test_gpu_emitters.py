"""GPU: the two ends of every path -- many emitters of unequal areas and every material type, light counts 1, 3, 84 and 1281, films
that are neither W / H x 1 nor level -- on the scenes of tests/emitter_scenes.py against the C oracle, which
tests/test_emitter_scenes_cpu.py holds to a float64 statement of vertex 0 and counts (its docstring has the figures: 84 of 84 and
471 of 1281 lights chosen in one sample, 55 to 814 camera vertices on emitters, emitter vertices met from the front and from the
back by the hundred, 20 to 34 light-subpath vertices on emitters of each specular material, 616 to 706 light-image pixels of 920 on
the films, no NaN vertex, no non-finite addend).

Bytes everywhere (NaNs canonicalised where bytes differ: tests/path_compare.py), but for the light image summed by float atomics,
which is held to the parity tests' rtol 5e-5, atol 1e-8 -- and to bytes under the reproducible switch, through the accumulators.

    stage by stage     the generators' rays, the RNG buffer, Path[] of both kinds, aggregators, unidirectional image, ray count, light
                       image, accumulators -- every scene and film, T40 (material table in global memory, an emitter material at
                       index 35) on two of them, planted seeds (a draw of exactly 1.0: count * 1.0 is one past the last light)
    organisations      traversal modes 0-5 serial and with pipelining 2, builders numpy / native / gpu, K = 1 and 2 streams at 67 x 33
    resolve forms      T12: the slim kernel against its parent (debug bit 27)
    strategies, layers masked_oracle.device_check on drawn cases; strategies.LAYERS, the emission layer pixel by pixel
    seeded visibility  set_connection_query(1) on lamps_streamed
    feature pass       the camera kernel's rays on the three films

plus six seeds of tools/fuzz_parity.py: random_scene(emitters=...) in tests/test_gpu_fuzz.py.  DESIGN.md 2.4 has the mutants these
tests catch and the suite before them did not."""
import numpy as np
import pytest

import denoise_reference as dr
import emitter_scenes as es
import masked_oracle as mo
from path_compare import same_paths
from test_gpu_resolve_slim import PARENT_BIT, _b, _one_sample

pytestmark = pytest.mark.gpu
LIGHT, CAMERA = 0, 1
F = np.float32
AGG = ("weights", "total_contribution", "contrib_weight_sum")
RTOL, ATOL = 5e-5, 1e-8                                    # the light image by float atomics (tests/test_gpu_fuzz.py, masked_oracle.py)


class Ref:
    """The oracle on one scene and seed buffer: sample 1 stage by stage, and two samples with the stable light sort (the order the
    device's reproducible switch sums in).  Copies, made once and never written."""

    def __init__(self, orc, sc, seeds):
        self.scene, self.seeds0 = sc, np.array(seeds, copy=True)
        o = orc.OracleRenderer(sc, seeds=seeds)
        o.make_light_rays()
        self.light_rays = o.light_ray_buffer.copy()
        o.make_camera_rays()
        self.camera_rays, self.seeds_rays = o.camera_ray_buffer.copy(), o.rand_buffer.copy()
        o.trace_light_rays(); o.trace_camera_rays()
        self.light1, self.camera1, self.seeds1 = o.out_light_paths.copy(), o.out_camera_paths.copy(), o.rand_buffer.copy()
        o.join_paths(); o.finalize_samples(); o.gather_light_image()
        self.agg1 = {f: o.weight_aggregators[f].copy() for f in AGG}
        self.uni1, self.light_image1, self.finalized1 = o.out_camera_image.copy(), o.out_light_image.copy(), o.finalized_samples.copy()
        o.process_images()
        self.rays1 = o.rays_traced
        s = orc.OracleRenderer(sc, seeds=seeds)
        s.run_sample(stable_light_sort=True)
        self.acc1 = self._acc(s)
        assert s.out_light_paths.tobytes() == self.light1.tobytes() and s.rays_traced == self.rays1
        s.run_sample(stable_light_sort=True)
        self.acc2 = self._acc(s)
        self.light2, self.camera2, self.seeds2 = s.out_light_paths.copy(), s.out_camera_paths.copy(), s.rand_buffer.copy()
        self.agg2 = {f: s.weight_aggregators[f].copy() for f in AGG}
        self.rays2 = s.rays_traced

    @staticmethod
    def _acc(o):
        return [a.copy() for a in (o.summed_image, o.summed_sample_weights, o.summed_sample_counts, o.unidirectional_image_buffer)]


@pytest.fixture(scope="module")
def refs(oracle_mod):
    made = {}

    def get(name, n_mats=12, builder="numpy", planted=False, w=es.W, h=es.H, rank=0):
        key = (name, n_mats, builder, planted, w, h, rank)
        if key not in made:
            from clive2_amd.renderer import make_seeds
            sc = es.scene(name, n_mats, builder, w, h)
            B = sc.pixel_width * sc.pixel_height
            made[key] = Ref(oracle_mod, sc, es.seeds(B, planted) if rank == 0 else make_seeds(B, rank=rank))
        return made[key]
    return get


@pytest.fixture(scope="module")
def handles():
    """One Renderer per scene, shared by the tests that leave it as they found it (settings())."""
    made = {}

    def get(name, n_mats=12, builder="numpy"):
        from clive2_amd.renderer import Renderer
        if (name, n_mats, builder) not in made:
            made[name, n_mats, builder] = Renderer(es.scene(name, n_mats, builder))
        return made[name, n_mats, builder]
    yield get
    for r in made.values():
        r.close()


def settings(r, mode=0, flags=0, query=0, pipelining=-1, reproducible=False):
    r.set_connection_query(0); r.set_debug_flags(0)
    r.set_traversal_mode(mode); r.set_debug_flags(flags); r.set_connection_query(query); r.set_pipelining(pipelining)
    r.set_reproducible(reproducible)


def start(r, seeds):
    r.set_seeds(seeds); r.reset_accumulators(); r.reset_counters()


def same(a, b):
    """the same bytes, or the same after every NaN is put into one bit pattern"""
    return a.tobytes() == b.tobytes() or mo.canonical(a) == mo.canonical(b)


def assert_two_samples(r, ref, label):
    """After run_samples(2): Path[] of both kinds, the RNG buffer, the three aggregator fields and the ray count are the oracle's."""
    for which, want in ((LIGHT, ref.light2), (CAMERA, ref.camera2)):
        assert same_paths(r.export_paths(which), want) is not None, (label, which)
    assert np.array_equal(r.get_random_buffer(), ref.seeds2), label
    agg = r.export_aggregators()
    for f in AGG:
        assert same(agg[f], ref.agg2[f]), (label, f)
    assert r.counters()["rays"] == ref.rays2, label


# ---------------------------------------------------------------- storage
def test_the_scenes_take_their_storage_routes(handles):
    """lamps_lds: tree and triangles in LDS; lamps_streamed: the tree streams from memory and has a 4-wide collapse."""
    org = handles("lamps_lds").organisation()
    assert org["tree_in_lds"] == 1 and org["lds_triangles"] == 1 and org["n_records"] == len(es.scene("lamps_lds").boxes), org
    org = handles("lamps_streamed").organisation()
    assert org["tree_in_lds"] == 0 and org["wide_nodes"] > 0 and org["pruned_records"] == 0, org


# ---------------------------------------------------------------- stage by stage
STAGED = [(name, 12, False) for name in es.CASES] + [("three_lights", 12, True), ("lamps_lds", 12, True),
                                                     ("lamps_lds", 40, False), ("three_lights", 40, False), ("lamps_streamed", 40, True)]


@pytest.mark.parametrize("name,n_mats,planted", STAGED)
def test_stage_by_stage(name, n_mats, planted, handles, refs):
    r, ref = handles(name, n_mats), refs(name, n_mats, planted=planted)
    label = (name, n_mats, planted)
    if planted:                                           # the planted entries took the LAST light (the oracle; the device below)
        rows = es.planted_entries(r.batch_size)
        assert (ref.light_rays["triangle"][rows] == ref.scene.light_triangle_indices[-1]).all()
    try:
        settings(r)
        start(r, ref.seeds0)
        r.make_light_rays()
        assert r.export_rays(LIGHT).tobytes() == ref.light_rays.tobytes(), label
        r.make_camera_rays()
        assert r.export_rays(CAMERA).tobytes() == ref.camera_rays.tobytes(), label
        assert np.array_equal(r.get_random_buffer(), ref.seeds_rays), label
        r.trace_light_rays(); r.trace_camera_rays()
        for which, want in ((LIGHT, ref.light1), (CAMERA, ref.camera1)):
            got = r.export_paths(which)
            assert got.tobytes() == want.tobytes() or same_paths(got, want) == "nans", (label, which)
        assert np.array_equal(r.get_random_buffer(), ref.seeds1), label
        r.join_paths(); r.finalize_samples(); r.gather_light_image()
        images = r.export_sample_images()
        r.process_images()
        agg = r.export_aggregators()
        for f in AGG:
            assert same(agg[f], ref.agg1[f]), (label, f)
        assert same(images["unidirectional"], ref.uni1), label
        assert same(images["finalized"][:, :3], ref.finalized1[:, :3]), label
        assert same(r.read_accumulators()[3], ref.acc1[3]), label
        assert r.counters()["rays"] == ref.rays1, label
        assert (ref.light_image1[:, :3] > 0).any()
        np.testing.assert_allclose(images["light"][:, :3], ref.light_image1[:, :3], rtol=RTOL, atol=ATOL, err_msg=str(label))
        np.testing.assert_allclose(r.read_accumulators()[0], ref.acc1[0], rtol=RTOL, atol=ATOL, err_msg=str(label))
        # the reproducible switch: every accumulator has the bytes of the oracle with the stable light sort
        settings(r, reproducible=True)
        start(r, ref.seeds0)
        r.make_light_rays(); r.make_camera_rays(); r.trace_light_rays(); r.trace_camera_rays()
        r.join_paths(); r.finalize_samples(); r.gather_light_image(); r.process_images()
        for got, want, what in zip(r.read_accumulators(), ref.acc1, ("image", "weights", "counts", "unidirectional")):
            assert same(got, want) if got.dtype == F else np.array_equal(got, want), (label, what)
    finally:
        settings(r)
        start(r, ref.seeds0)


# ---------------------------------------------------------------- every organisation
ORGANISED = [(name, "numpy") for name in es.CASES] + [(name, "native") for name in es.SCENES + ("film_rolled",)] + [("lamps_streamed", "gpu")]


@pytest.mark.parametrize("name,builder", ORGANISED)
def test_every_organisation_renders_the_oracles_samples(name, builder, handles, refs):
    """run_samples(2) in traversal modes 0-5, serial and with pipelining 2, with the trees of the numpy, the native and the GPU
    builder (the oracle walks the same Box[])."""
    r, ref = handles(name, 12, builder), refs(name, 12, builder)
    try:
        for mode in range(6):
            for pipelining in (0, 2):
                settings(r, mode=mode, pipelining=pipelining)
                start(r, ref.seeds0)
                r.run_samples(2)
                assert_two_samples(r, ref, (name, builder, mode, pipelining))
        settings(r, reproducible=True)
        start(r, ref.seeds0)
        r.run_samples(2)
        for got, want, what in zip(r.read_accumulators(), ref.acc2, ("image", "weights", "counts", "unidirectional")):
            assert same(got, want) if got.dtype == F else np.array_equal(got, want), (name, builder, what)
    finally:
        settings(r)
        start(r, ref.seeds0)


@pytest.mark.parametrize("K", [1, 2])
def test_sample_streams_on_a_frame_that_is_no_multiple_of_a_wave(K, refs):
    """lamps_lds at 67 x 33 = 2,211 entries: with two streams the boundary between them falls inside a wave.  Stream k is the
    oracle seeded with make_seeds(B, rank=k)."""
    from clive2_amd.renderer import Renderer, stream_seeds
    sc = es.scene("lamps_lds", 12, "numpy", 67, 33)
    B = 67 * 33
    want = [refs("lamps_lds", w=67, h=33, rank=k) for k in range(K)]
    assert np.array_equal(want[0].seeds0, stream_seeds(B, 2)[0])
    r = Renderer(sc, seeds=stream_seeds(B, K), streams=K)
    try:
        for mode in (0, 5):
            settings(r, mode=mode)
            start(r, stream_seeds(B, K))
            r.run_samples(2)
            for k, ref in enumerate(want):
                r.set_export_stream(k)
                for which, paths in ((LIGHT, ref.light2), (CAMERA, ref.camera2)):
                    assert same_paths(r.export_paths(which), paths) is not None, (K, mode, k, which)
                agg = r.export_aggregators()
                for f in AGG:
                    assert same(agg[f], ref.agg2[f]), (K, mode, k, f)
            assert np.array_equal(r.get_random_buffer().reshape(K, B, 2), np.stack([ref.seeds2 for ref in want]))
            assert r.counters()["rays"] == sum(ref.rays2 for ref in want)
    finally:
        r.close()


# ---------------------------------------------------------------- resolve forms
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", ["lamps_lds", "three_lights"])
def test_slim_resolve_kernel_against_its_parent(name, det):
    """T12: the slim kernel (the packed {triangle << 8 | material byte} of light vertex 0, materials in LDS) and k_connect_resolve,
    which debug bit 27 launches in its place: the same bytes of everything the resolve stage writes, as
    tests/test_gpu_resolve_slim.py compares them.  (T40 against the oracle: test_stage_by_stage.)"""
    sc = es.scene(name)
    (a,), (b,) = _one_sample(sc, 1, det, 0), _one_sample(sc, 1, det, PARENT_BIT)
    assert a["cmask"].tobytes() == b["cmask"].tobytes() and a["cmask"].any()
    for f in AGG:
        assert _b(a["agg"][f]) == _b(b["agg"][f]), f
    assert _b(a["unidirectional"]) == _b(b["unidirectional"])
    assert _b(a["finalized"]) == _b(b["finalized"])
    assert (a["light"][:, :3] > 0).any()
    if det:
        assert _b(a["light"]) == _b(b["light"])
    else:
        np.testing.assert_allclose(a["light"], b["light"], rtol=2e-5, atol=1e-9)


# ---------------------------------------------------------------- strategies and layers
@pytest.mark.parametrize("draw", range(3))
@pytest.mark.parametrize("name", ["lamps_lds", "lamps_streamed"])
def test_drawn_masks_and_layer_tables(name, draw, oracle_mod):
    from clive2_amd.renderer import stream_seeds
    sc = es.scene(name)
    rng = np.random.RandomState(4100 + 10 * draw + (name == "lamps_streamed"))
    case = mo.draw_case(rng)
    problems, left_out = mo.device_check(sc, stream_seeds(es.W * es.H, case["K"], seed=draw), case, passes=2)
    print(name, draw, {k: (hex(v) if k == "mask" else v) for k, v in case.items() if k != "table"}, "left out", left_out)
    assert not problems, problems


@pytest.fixture(scope="module")
def lamp_pixels(oracle_mod):
    sc = es.scene("lamps_lds")
    return es.pixels_by_first_hit(sc, lambda rays: oracle_mod.traverse(rays, sc.boxes, sc.triangles))


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("name", ["lamps_lds", "lamps_streamed"])
def test_emission_direct_and_indirect_layers(name, det, handles, lamp_pixels, oracle_mod):
    """strategies.LAYERS in one render against the masked oracle: bytes under the reproducible switch, else at the light image's
    tolerance.  On lamps_lds the emission layer is non-zero on the pixels that see only diffuse emitting faces of the lamp and zero on
    those that, with their neighbours, see only black and specular ones (tests/emitter_scenes.py: pixels_by_first_hit)."""
    from clive2_amd import strategies as S
    sc = es.scene(name)
    seeds = es.seeds(es.W * es.H)
    ref = mo.Render(sc, seeds, 2)
    plain = ref.render(None)
    r = handles(name)
    try:
        settings(r, reproducible=det)
        r.set_layers(S.LAYERS)
        start(r, seeds)
        r.run_samples(2)
        lacc = r.layer_accumulators()
        for l, (lname, m) in enumerate(S.LAYERS.items()):
            want = ref.render(m)
            problem, _ = mo.compare(lacc[l], want.packed[:3], det, nonfinite=want.nonfinite | plain.nonfinite)
            assert problem is None, (name, det, lname, problem)
        problem, _ = mo.compare(r.packed_accumulators().reshape(8, -1), plain.packed, det, nonfinite=plain.nonfinite)
        assert problem is None, (name, det, problem)
        assert all(np.any(lacc[l] != 0) for l in range(3))
        if name == "lamps_lds":
            emitting, dark = lamp_pixels
            assert emitting.sum() >= 12 and dark.sum() >= 5
            assert (lacc[0][:, emitting] > 0).any(axis=0).all()
            assert not lacc[0][:, dark].any()
    finally:
        r.set_layers(None)
        settings(r)
        start(r, seeds)


# ---------------------------------------------------------------- seeded visibility
def test_connection_query_with_many_emitters(handles, refs):
    """cl2_set_connection_query(1) is active on lamps_streamed in mode 5 -- the s = 1 rays start on 1,281 emitters -- and the
    aggregators after two samples have mode 0's bytes, which are the oracle's."""
    r, ref = handles("lamps_streamed"), refs("lamps_streamed")
    agg = []
    try:
        for mode, query in ((0, 0), (5, 0), (5, 1)):
            settings(r, mode=mode, query=query, pipelining=0)
            assert r.connection_query_active() == query
            start(r, ref.seeds0)
            r.run_samples(2)
            agg.append(r.export_aggregators())
    finally:
        settings(r)
        start(r, ref.seeds0)
    for f in AGG:
        assert agg[0][f].tobytes() == agg[1][f].tobytes() == agg[2][f].tobytes(), f
        assert same(agg[2][f], ref.agg2[f]), f


# ---------------------------------------------------------------- the feature pass on the films
@pytest.mark.parametrize("samples", [1, 3])
@pytest.mark.parametrize("name", es.FILMS)
def test_feature_pass_on_the_films(name, samples, handles, oracle_mod):
    """render_features casts the camera kernel's rays: against denoise_reference.feature_pass with the oracle's closest hit, as
    tests/test_gpu_denoise.py compares -- depth, albedo and coverage byte for byte, normals to 1e-6."""
    from clive2_amd.renderer import make_seeds
    sc = es.scene(name)
    S = make_seeds(es.FILM_W * es.FILM_H, seed=77)

    def closest_hit(rays):
        with np.errstate(divide="ignore"):
            rays["inv_direction"][:, :3] = F(1.0) / rays["direction"][:, :3]
        return oracle_mod.traverse(rays, sc.boxes, sc.triangles)
    r = handles(name)
    r.render_features(samples, seeds=S)
    f = r.features()
    want = dr.feature_pass(sc, S, samples, closest_hit)
    assert all(np.isfinite(x).all() for x in f.values())
    for k in ("depth", "albedo", "coverage"):
        assert f[k].tobytes() == want[k].tobytes(), (name, samples, k)
    np.testing.assert_allclose(f["normal"], want["normal"], rtol=0, atol=1e-6)
    assert (f["coverage"] == 1).all() and len(np.unique(f["albedo"].reshape(-1, 3), axis=0)) >= 3
