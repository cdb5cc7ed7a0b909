"""Layer accumulators (cl2_set_layers, csrc/layers.hpp, csrc/connect_resolve.hpp LAYERS) on the device: the layers of
ONE render are the masked renders of the strategy mask (cl2_set_strategy_mask), byte for byte in reproducible mode, and the ordinary
accumulators do not notice.  Frames of 64 x 48 (Cornell box, glass scene) and one of 50 x 37 (1,850 entries: a last workgroup with
lanes past the batch, and with two sample streams a stream boundary inside a wave).  Every render is 3 passes from
stream_seeds(seed=20240928).  Floats are compared as bytes with every NaN canonicalised to one pattern."""
import ctypes as C
import glob

import numpy as np
import pytest

from clive2_amd import strategies as S

pytestmark = pytest.mark.gpu

F = np.float32
RTOL, ATOL = 5e-5, 1e-8                        # the light-image tolerance of tests/test_gpu_strategies.py (float atomics)
DECOMP = 32.0 * 2.0 ** -24                     # |sum of parts - full| <= DECOMP * sum: test_masked_renders_decompose_the_picture
PASSES, SEED = 3, 20240928

T1_ODD = S.mask((s, 1) for s in (1, 3, 5))
T1_EVEN = S.mask((s, 1) for s in (2, 4, 6))
TABLES = {
    "layers": dict(S.LAYERS),
    # 1 .. 7 edges, then 8 and more: fills CL2_MAX_LAYERS
    "lengths": dict([(f"k{k}", S.path_length(k, k)) for k in range(1, 8)] + [("k8+", S.path_length(8))]),
    # the six t = 1 pairs over two layers: light-image routing
    "light_split": {"odd": T1_ODD, "even": T1_EVEN, "camera": S.CAMERA_IMAGE},
    # pairs left out, an empty layer
    "partial": {"direct": S.path_length(2, 2), "nothing": 0, "two": S.bit(3, 1) | S.bit(2, 3)},
}
PARTITIONS = ["layers", "lengths", "light_split"]
SCENE_NAMES = ["cornell", "glass"]


def _b(a):
    """bytes of a float array, every NaN made the same NaN"""
    a = np.array(a, dtype=F, copy=True)
    a[np.isnan(a)] = np.nan
    return a.tobytes()


def _handle(scene, det=True, K=1, mode=None, flags=0, pipe=None, variant=None):
    from clive2_amd.renderer import Renderer, stream_seeds
    r = Renderer(scene, streams=K, variant=variant)
    seeds = stream_seeds(r.batch_size, K, seed=SEED)
    r.set_seeds(seeds)
    r.set_reproducible(det)
    if mode is not None:
        r.set_traversal_mode(mode)
    if flags:
        r.set_debug_flags(flags)
    if pipe is not None:
        r.set_pipelining(pipe)
    return r, seeds


def _render(r, seeds, passes=PASSES, extras=False):
    """reset, seeds, `passes` passes: the eight rows, seeds, rays (and moments / buckets where they are on)"""
    r.reset_accumulators()
    r.set_seeds(seeds)
    r.reset_counters()
    r.run_samples(passes)
    out = dict(acc=r.packed_accumulators().reshape(8, -1), seeds=r.get_random_buffer(), rays=r.counters()["rays"],
               radiance=r.radiance)
    if extras:
        out.update(moments=r.moments(), buckets=r.buckets())
    return out


class Masked:
    """The comparison renders of one scene: the render without layers and, per mask, the masked render -- made once each on one
    handle and kept (never written)."""

    def __init__(self, scene, det=True, K=1, passes=PASSES):
        self.r, self.seeds = _handle(scene, det=det, K=K)
        self.passes = passes
        self.plain = _render(self.r, self.seeds, passes)
        self.cache = {}

    def __call__(self, mask):
        if mask not in self.cache:
            self.r.set_strategy_mask(mask)
            self.cache[mask] = _render(self.r, self.seeds, self.passes)
            self.r.set_strategy_mask(None)
        return self.cache[mask]

    def close(self):
        self.r.close()


def _layered(r, seeds, table, passes=PASSES, extras=False):
    r.set_layers(table)
    out = _render(r, seeds, passes, extras)
    out["lacc"] = r.layer_accumulators()
    return out


def _same_main(got, want):
    """all eight rows, seeds and ray counters"""
    assert _b(got["acc"]) == _b(want["acc"])
    assert np.array_equal(got["seeds"], want["seeds"]) and got["rays"] == want["rays"]


def _assert_layers_are_masked_renders(got, table, masked):
    assert got["lacc"].shape == (len(table), 3, got["acc"].shape[1]) and got["lacc"].dtype == F
    for l, (name, m) in enumerate(table.items()):
        want = masked(S.to_mask(m))
        assert _b(got["lacc"][l]) == _b(want["acc"][:3]), name
        if S.to_mask(m) == 0:
            assert got["lacc"][l].tobytes() == bytes(got["lacc"][l].nbytes), name          # +0 bytes
    _same_main(got, masked.plain)


@pytest.fixture(scope="module")
def scenes(cornell_small, glass_scene):
    return {"cornell": cornell_small, "glass": glass_scene}


@pytest.fixture(scope="module")
def masked(scenes):
    """Per scene the reproducible comparison renders (module scope: each mask is rendered once)."""
    out = {name: Masked(scene) for name, scene in scenes.items()}
    yield out
    for m in out.values():
        m.close()


# ---- 1: reproducible mode, every table, both scenes ----
@pytest.mark.parametrize("name", SCENE_NAMES)
@pytest.mark.parametrize("table", list(TABLES))
def test_layers_are_the_masked_renders_byte_for_byte(name, table, scenes, masked):
    r, seeds = _handle(scenes[name])
    got = _layered(r, seeds, TABLES[table])
    r.close()
    _assert_layers_are_masked_renders(got, TABLES[table], masked[name])
    assert np.any(got["lacc"] != 0)
    if table == "light_split":
        assert np.any(got["lacc"][0] != 0) and np.any(got["lacc"][1] != 0)        # both t = 1 layers received light


# ---- 2: with error tracking and robust buckets ----
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_layers_beside_moments_and_buckets(name, scenes, masked):
    r, seeds = _handle(scenes[name])
    r.set_error_tracking(True)
    r.set_robust_buckets(4)
    want = _render(r, seeds, extras=True)                               # layers off
    got = _layered(r, seeds, TABLES["lengths"], extras=True)
    r.close()
    _assert_layers_are_masked_renders(got, TABLES["lengths"], masked[name])
    assert _b(got["moments"]) == _b(want["moments"]) and _b(got["buckets"]) == _b(want["buckets"])
    _same_main(got, want)


# ---- 3: the stage calls ----
def test_one_sample_through_the_stage_calls(cornell_small):
    r, seeds = _handle(cornell_small)
    want = _layered(r, seeds, TABLES["light_split"], passes=1)
    r.reset_accumulators(); r.set_seeds(seeds)
    r.make_light_rays(); r.make_camera_rays(); r.trace_light_rays(); r.trace_camera_rays()
    r.join_paths(); r.finalize_samples(); r.gather_light_image(); r.process_images()
    assert _b(r.layer_accumulators()) == _b(want["lacc"])
    assert _b(r.packed_accumulators().reshape(8, -1)) == _b(want["acc"])
    assert np.any(want["lacc"][0] != 0) and np.any(want["lacc"][2] != 0)
    r.close()


# ---- 4: sample streams, traversal organisations, pipelining ----
def test_layers_do_not_depend_on_streams_organisation_or_pipelining():
    import clive2_amd as c2
    scene = c2.create_scene_from_preset("empty", 50, 37)
    table = TABLES["light_split"]
    ref = Masked(scene, K=2)
    want = None
    for mode, flags in ((None, 0), (1, 0), (2, 0), (5, 0), (None, 1 << 25)):
        for pipe in (0, 2):
            r, seeds = _handle(scene, K=2, mode=mode, flags=flags, pipe=pipe)
            got = _layered(r, seeds, table)
            r.close()
            if want is None:
                want = got
                _assert_layers_are_masked_renders(got, table, ref)      # K = 2 on 1,850 pixels against the masked renders
                assert np.any(got["lacc"][0] != 0) and np.any(got["lacc"][2] != 0)
            assert _b(got["lacc"]) == _b(want["lacc"]), (mode, flags, pipe)
            assert _b(got["acc"]) == _b(want["acc"]), (mode, flags, pipe)
    ref.close()


# ---- 5: the material table in global memory (MATS_LDS = false) ----
@pytest.mark.parametrize("det", [True, False])
def test_layers_with_a_material_table_beyond_the_lds_cap(det, cornell_small):
    import copy
    from clive2_amd import struct_types as st
    scene = copy.copy(cornell_small)
    mats = np.zeros(40, dtype=st.Material)                             # LDS_MAT_CAP = 32 (csrc/scene_layout.hpp)
    n = len(np.asarray(cornell_small.materials).reshape(-1))
    mats[:n] = np.asarray(cornell_small.materials).reshape(-1)
    mats[n:] = mats[n - 1]
    scene.materials = mats
    ref = Masked(scene, det=det)
    r, seeds = _handle(scene, det=det)
    got = _layered(r, seeds, TABLES["layers"])
    r.close()
    if det:
        _assert_layers_are_masked_renders(got, TABLES["layers"], ref)
    else:
        for l, m in enumerate(TABLES["layers"].values()):
            np.testing.assert_allclose(got["lacc"][l], ref(m)["acc"][:3], rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(got["acc"], ref.plain["acc"], rtol=RTOL, atol=ATOL)
    assert np.any(got["lacc"] != 0)
    ref.close()


# ---- 6: float atomics ----
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_layers_with_float_atomics(name, scenes):
    ref = Masked(scenes[name], det=False)
    for tname in ("light_split", "partial", "layers"):
        table = TABLES[tname]
        r, seeds = _handle(scenes[name], det=False)
        got = _layered(r, seeds, table)
        r.close()
        for l, (lname, m) in enumerate(table.items()):
            want = ref(S.to_mask(m))["acc"][:3]
            np.testing.assert_allclose(got["lacc"][l], want, rtol=RTOL, atol=ATOL, err_msg=f"{tname}/{lname}")
            if not S.to_mask(m) & S.LIGHT_IMAGE:
                assert _b(got["lacc"][l]) == _b(want), (tname, lname)   # no t = 1 pair: no atomics in this layer
        np.testing.assert_allclose(got["acc"], ref.plain["acc"], rtol=RTOL, atol=ATOL)
        assert np.array_equal(got["seeds"], ref.plain["seeds"]) and got["rays"] == ref.plain["rays"]
    ref.close()


# ---- 7: partitions add up ----
@pytest.mark.parametrize("table", PARTITIONS)
def test_the_layers_of_a_partition_add_up(table, cornell_small):
    """The bound, the pixel selection (every value finite, every pixel checked) and the render (two streams, four passes) of
    test_masked_renders_decompose_the_picture."""
    assert sum(S.layer_masks(TABLES[table])) == S.ALL
    r, seeds = _handle(cornell_small, K=2)
    got = _layered(r, seeds, TABLES[table], passes=4)
    r.close()
    total = sum(p.astype(np.float64) for p in got["lacc"])
    full = got["acc"][:3].astype(np.float64)
    assert np.all(np.isfinite(total)) and np.all(np.isfinite(full)) and np.all(total >= 0)
    err = np.abs(total - full)
    print("layers add up: max |sum - full| / sum =", float(np.max(err / np.maximum(total, 1e-300))), "bound", DECOMP)
    assert np.all(err <= DECOMP * total)
    assert np.any(total > 0)


# ---- 8: round trip and pictures ----
def test_round_trip_and_layer_radiance(cornell_small, masked):
    table = TABLES["layers"]
    r, seeds = _handle(cornell_small)
    got = _layered(r, seeds, table)
    pics = r.layer_radiance()
    assert list(pics) == list(table) == list(r.layers())
    for name, m in table.items():
        assert pics[name].shape == (48, 64, 3) and pics[name].dtype == F
        assert _b(pics[name]) == _b(masked["cornell"](m)["radiance"]), name
    rng = np.random.RandomState(11)
    a = rng.standard_normal(got["lacc"].shape).astype(F)
    a[0, 0, :4] = [np.inf, -np.inf, -0.0, np.nan]
    r.load_layer_accumulators(a)
    assert r.layer_accumulators().tobytes() == a.tobytes()
    r.close()
    # render_layers_once: the dictionary of render_layers, from one render
    r, seeds = _handle(cornell_small)
    r.set_layers({"keep": S.bit(0, 2)})
    once = r.render_layers_once(PASSES, seeds=seeds)
    assert r.layers() == {"keep": S.bit(0, 2)}                         # the table found on entry is restored
    assert list(once) == ["emission", "direct", "indirect"]
    for name, m in table.items():
        assert _b(once[name]) == _b(masked["cornell"](m)["radiance"]), name
    r.close()


# ---- 9: lifetime and refusals ----
def test_the_table_survives_and_lacc_follows_the_validity_rule(cornell_small):
    from clive2_amd.renderer import RendererError, stream_seeds
    r, seeds = _handle(cornell_small)
    assert r.layers() == {}                                             # off by default
    with pytest.raises(RendererError):
        r.layer_accumulators()                                          # no table: CL2_E_STATE
    table = TABLES["partial"]
    r.set_layers(table)
    masks = {k: S.to_mask(v) for k, v in table.items()}
    r.upload_scene(cornell_small)
    assert r.layers() == masks
    r.set_sample_streams(2)
    assert r.layers() == masks
    r.set_seeds(stream_seeds(r.batch_size, 2, seed=SEED))
    r.run_samples(2)                                                    # the re-allocated per-entry buffers
    assert np.any(r.layer_accumulators() != 0)
    r.set_sample_streams(1)
    assert np.any(r.layer_accumulators() != 0)                          # per pixel: kept, as the accumulators are
    r.reset_accumulators()
    assert r.layers() == masks
    z = r.layer_accumulators()
    assert z.tobytes() == bytes(z.nbytes)                               # a reset zeroes lacc
    # bits outside the 41 are dropped
    r.set_layers({"a": S.bit(0, 2) | 1 | 1 << 63})
    assert r.layers() == {"a": S.bit(0, 2)}
    # a different table on a handle with samples: invalid until a reset; the same table: nothing changes
    r.set_seeds(seeds)
    r.run_samples(1)
    kept = r.layer_accumulators()
    r.set_layers({"a": S.bit(0, 2)})
    assert r.layer_accumulators().tobytes() == kept.tobytes()
    r.set_layers({"b": S.bit(1, 2)})
    with pytest.raises(RendererError):
        r.layer_accumulators()
    r.run_samples(1)
    with pytest.raises(RendererError):
        r.layer_accumulators()
    r.load_layer_accumulators(np.ones((1, 3, r.batch_size), F))         # a write makes them valid
    assert np.all(r.layer_accumulators() == 1)
    r.load_packed_accumulators(r.packed_accumulators())                 # ... and a write of the accumulators invalid again
    with pytest.raises(RendererError):
        r.layer_accumulators()
    r.reset_accumulators()
    assert not r.layer_accumulators().any()
    # sizes and NULLs
    L, h = r._L, r._h
    buf = np.zeros(3 * r.batch_size + 1, F)
    assert L.cl2_read_layers_packed(h, buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.size)) == -1
    assert L.cl2_write_layers_packed(h, buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.size)) == -1
    assert L.cl2_read_layers_packed(h, None, C.c_size_t(3 * r.batch_size)) == -1
    assert L.cl2_set_layers(None, None, 0) == -1 and L.cl2_get_layers(None, None, 0) == -1
    one = (C.c_uint64 * 1)(S.bit(0, 2))
    assert L.cl2_set_layers(h, one, -1) == -1
    nine = (C.c_uint64 * 9)(*[S.bit(s, 2) for s in range(7)], S.bit(1, 3), S.bit(2, 3))
    assert L.cl2_set_layers(h, nine, 9) == -1                           # more than CL2_MAX_LAYERS
    two = (C.c_uint64 * 2)(S.bit(0, 2) | S.bit(1, 2), S.bit(1, 2))
    assert L.cl2_set_layers(h, two, 2) == -1                            # overlap
    assert r.layers() == {"b": S.bit(1, 2)}                             # the refused calls changed nothing
    r.set_layers(None)
    assert r.layers() == {}
    r.close()


def test_layers_refuse_masks_densities_and_the_cross_check_kernel(cornell_small):
    from clive2_amd.renderer import RendererError
    table = TABLES["layers"]
    r, seeds = _handle(cornell_small, det=False, variant="test")
    # a partial strategy mask
    r.set_strategy_mask(S.path_length(3))
    with pytest.raises(RendererError, match="cl2_set_strategy_mask"):
        r.set_layers(table)
    assert r.layers() == {}
    r.set_strategy_mask(None)
    r.set_layers(table)
    with pytest.raises(RendererError, match="cl2_set_layers"):
        r.set_strategy_mask(S.path_length(3))
    assert r.strategy_mask() == S.ALL
    r.set_strategy_mask(S.ALL)                                          # the full mask may be set again
    # a sample density, adaptive sampling
    with pytest.raises(RendererError, match="cl2_set_layers"):
        r.set_sample_density(np.ones((48, 64), F))
    with pytest.raises(RendererError, match="cl2_set_layers"):
        r._check(r._L.cl2_set_adaptive_sampling(r._h, 1, C.c_double(0.25)), "cl2_set_adaptive_sampling")
    r.set_layers(None)
    r.set_sample_density(np.ones((48, 64), F))
    with pytest.raises(RendererError, match="cl2_set_sample_density"):
        r.set_layers(table)
    r.set_sample_density(None)
    # debug bits 4-6 = 7
    WIDE = 7 << 4
    r.set_debug_flags(WIDE)
    with pytest.raises(RendererError, match="debug bits"):
        r.set_layers(table)
    r.set_debug_flags(0)
    r.set_layers(table)
    with pytest.raises(RendererError, match="cl2_set_layers"):
        r.set_debug_flags(WIDE)
    # more than eight, overlaps: refused before the library is called
    with pytest.raises(ValueError):
        r.set_layers({f"l{i}": S.bit(i % 7, 2 + i // 7) for i in range(9)})
    with pytest.raises(ValueError):
        r.set_layers({"a": [(0, 2), (1, 2)], "b": [(1, 2)]})
    assert r.layers() == {k: S.to_mask(v) for k, v in table.items()}
    out = _layered(r, seeds, table)                                      # and the handle still renders its layers
    assert np.any(out["lacc"] != 0)
    r.close()


# ---- 10: the command line ----
def test_render_single_pass_writes_the_layers(tmp_path):
    from clive2_amd import render
    common = ["--scene", "empty", "--width", "64", "--height", "48", "--samples", "2", "--reproducible"]
    one, three = str(tmp_path / "one"), str(tmp_path / "three")
    assert render.main(common + ["--layers", one, "--single-pass"]) == 0
    assert render.main(common + ["--layers", three]) == 0
    for name in ("emission", "direct", "indirect"):
        assert glob.glob(f"{one}_{name}.png*"), name                     # .png, or .png.npy without PIL
    a, b = np.load(one + "_layers.npz"), np.load(three + "_layers.npz")
    assert sorted(a.files) == sorted(b.files) == ["direct", "emission", "indirect"]
    for k in a.files:
        np.testing.assert_allclose(a[k], b[k], rtol=RTOL, atol=ATOL, err_msg=k)
        assert np.any(a[k] != 0)
