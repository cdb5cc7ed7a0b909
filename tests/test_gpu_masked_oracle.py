"""The strategy mask (STRAT), the layer accumulators (LAYERS) and the other forms of the resolve stage against the MASKED ORACLE
(tests/masked_oracle.py, pinned to the oracle by tests/test_masked_oracle_cpu.py): the colour the device files under bit
(t - 1) * 7 + s must be the colour the reference computes for pair (s, t).  In every test the oracle side is the reference, never a
second device run.

Floats are compared as bytes with every NaN canonicalised to one pattern; the light image's bytes are compared under the
reproducible switch (a fixed summation order).  With float atomics the comparison is at RTOL, ATOL of tests/test_gpu_strategies.py;
a pixel with a non-finite per-sample addend in the reference may be left out, at most one pixel in 1000, and the number left out is
printed.  Frames: 64 x 48 (Cornell box, glass scene), 67 x 33 (the open scene of tests/test_gpu_resolve_slim.py: a last workgroup
with lanes that own no pixel), 50 x 37 with two sample streams (a stream boundary inside a wave), and the random scenes of
tools/fuzz_parity.py (at most 120 x 80)."""
import importlib.util
import os
import time

import numpy as np
import pytest

from clive2_amd import strategies as S

import masked_oracle as mo
from test_gpu_layers import TABLES, T1_EVEN, T1_ODD
from test_gpu_strategies import ATOL, RTOL

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES, SEED = 3, 20240928
AGG = ("total_contribution", "weights", "contrib_weight_sum")
assert (RTOL, ATOL) == (mo.RTOL, mo.ATOL)

_rng = np.random.RandomState(1)
RANDOM_MASKS = [mo.draw_mask(_rng), mo.draw_mask(_rng)]
MASKS = {"1-2 edges": S.path_length(1, 2), "3+ edges": S.path_length(3), "t1 odd": T1_ODD, "t1 even": T1_EVEN,
         "random a": RANDOM_MASKS[0], "random b": RANDOM_MASKS[1]}
_rng = np.random.RandomState(2)
ALL_TABLES = dict(TABLES, random_a=mo.draw_table(_rng), random_b=mo.draw_table(_rng))
FORM_MASK = RANDOM_MASKS[0]                      # t = 1 and t >= 2 pairs, some kept and some dropped of either kind
assert FORM_MASK & S.LIGHT_IMAGE and ~FORM_MASK & S.LIGHT_IMAGE and FORM_MASK & S.CAMERA_IMAGE and ~FORM_MASK & S.CAMERA_IMAGE


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.time()
    yield
    print(f"\ntests/test_gpu_masked_oracle.py: module wall time {time.time() - t0:.1f} s")


def _box_50x37():
    import clive2_amd as c2
    return c2.create_scene_from_preset("empty", 50, 37)


@pytest.fixture(scope="module")
def scenes(cornell_small, glass_scene):
    return {"cornell": cornell_small, "glass": glass_scene, "open": mo.open_scene(67, 33), "box50x37": _box_50x37()}


@pytest.fixture(scope="module")
def references(scenes, oracle_mod):
    """(scene name, K) -> the masked oracle's render of PASSES passes from stream_seeds(seed=SEED): traced on first use, every mask
    rendered once, never written"""
    from clive2_amd.renderer import stream_seeds
    cache = {}

    def get(name, K=1):
        if (name, K) not in cache:
            scene = scenes[name]
            cache[name, K] = mo.Render(scene, stream_seeds(scene.pixel_width * scene.pixel_height, K, seed=SEED), PASSES, K)
        return cache[name, K]
    return get


def _handle(scene, det=True, K=1, mode=None, flags=0):
    from clive2_amd.renderer import Renderer, stream_seeds
    r = Renderer(scene, streams=K)
    seeds = stream_seeds(r.batch_size, K, seed=SEED)
    r.set_seeds(seeds)
    r.set_reproducible(det)
    if mode is not None:
        r.set_traversal_mode(mode)
    if flags:
        r.set_debug_flags(flags)
    return r, seeds


def _render(r, seeds, passes=PASSES):
    r.reset_accumulators()
    r.set_seeds(seeds)
    r.reset_counters()
    r.run_samples(passes)
    return dict(acc=r.packed_accumulators().reshape(8, -1), seeds=r.get_random_buffer(), rays=r.counters()["rays"])


def _check(what, got, want, exact=True, nonfinite=None):
    problem, left_out = mo.compare(got, want, exact, nonfinite)
    if not exact:
        print(f"{what}: pixels left out of the tolerance comparison: {left_out} of {np.asarray(want).shape[-1]}")
    assert problem is None, f"{what}: {problem}"


# ---- 1: stage level, reproducible switch on: every singleton, the empty mask, the two images ----
STAGE_SCENES = ["cornell", "glass", "open"]
STAGE_MASKS = dict([("empty", 0), ("light image", S.LIGHT_IMAGE), ("camera image", S.CAMERA_IMAGE)] +
                   [(f"s{s}t{t}", S.bit(s, t)) for s, t in S.PAIRS])


def _stages(r, seeds, mask):
    """One sample through the stage calls, run to the end (process_images clears the light image), from `seeds`."""
    r.set_seeds(seeds)
    r.set_strategy_mask(mask)
    r.make_light_rays(); r.make_camera_rays(); r.trace_light_rays(); r.trace_camera_rays()
    r.join_paths()
    out = dict(agg=r.export_aggregators())
    r.finalize_samples(); r.gather_light_image()
    out.update(r.export_sample_images())
    r.process_images()
    return out


@pytest.fixture(scope="module")
def stage_runs(scenes, oracle_mod):
    """Per scene, from one seed buffer: the device's samples on ONE handle and the masked oracle's from ONE trace, per mask of
    STAGE_MASKS and unmasked (None).  Computed once, never written."""
    out = {}
    for name in STAGE_SCENES:
        scene = scenes[name]
        r, seeds = _handle(scene)
        dev = {None: _stages(r, seeds, None)}
        dev.update({k: _stages(r, seeds, m) for k, m in STAGE_MASKS.items()})
        r.close()
        o = oracle_mod.OracleRenderer(scene, seeds=seeds)
        trace = mo.Trace(o)
        ref = {None: mo.resolve(o, trace, None)}
        ref.update({k: mo.resolve(o, trace, m) for k, m in STAGE_MASKS.items()})
        out[name] = (dev, ref, mo.pair_pixels(trace.log))
    return out


@pytest.mark.parametrize("name", STAGE_SCENES)
def test_every_singleton_sample_equals_the_masked_oracle(name, stage_runs):
    dev, ref, counts = stage_runs[name]
    coloured = 0
    for key in dev:
        got, want = dev[key], ref[key]
        for f in AGG:
            _check(f"{name} mask {key}: aggregator {f}", got["agg"][f], want["agg"][f])
        _check(f"{name} mask {key}: finalized sample", got["finalized"][:, :3], want["finalized"][:, :3])
        _check(f"{name} mask {key}: light image (b, g, r, weight)", got["light"], want["light"])
        _check(f"{name} mask {key}: sample weights", got["sample_weights"], want["sample_weights"])
        _check(f"{name} mask {key}: unidirectional image", got["unidirectional"], want["unidirectional"])
        coloured += bool(np.any(want["finalized"][:, :3] != 0) or np.any(want["light"][:, :3] != 0))
    # not vacuous: every pair that occurs in the scene has a coloured singleton, plus the two images and the unmasked sample
    assert coloured == sum(1 for n in counts.values() if n > 0) + 3
    if name == "cornell":
        assert all(n >= 20 for n in counts.values())


# ---- 2: pipeline level ----
PIPELINES = {"cornell-K1": ("cornell", 1), "box50x37-K2": ("box50x37", 2)}


@pytest.mark.parametrize("switch", ["reproducible", "atomics"])
@pytest.mark.parametrize("case", list(PIPELINES))
def test_masked_renders_equal_the_masked_oracle(case, switch, scenes, references):
    name, K = PIPELINES[case]
    ref, exact = references(name, K), switch == "reproducible"
    plain = ref.render(None)
    r, seeds = _handle(scenes[name], det=exact, K=K)
    for key, mask in MASKS.items():
        r.set_strategy_mask(mask)
        got, want = _render(r, seeds), ref.render(mask)
        assert np.any(want.packed[:3] != 0), key
        _check(f"{case} {switch} mask {key}: the eight rows", got["acc"], want.packed, exact, want.nonfinite | plain.nonfinite)
        _check(f"{case} {switch} mask {key}: unidirectional rows and counts", got["acc"][4:], plain.packed[4:])
        assert np.array_equal(got["seeds"], ref.seeds) and got["rays"] == ref.rays, key
    r.close()


# ---- 3: layers ----
def _assert_layers(what, got, lacc, table, ref, exact=True):
    plain = ref.render(None)
    assert lacc.shape == (len(table), 3, plain.packed.shape[1]) and lacc.dtype == F
    for l, (lname, m) in enumerate(table.items()):
        m = S.to_mask(m)
        want = ref.render(m)
        # a layer without a t = 1 pair receives no atomics: bytes in either mode
        _check(f"{what} layer {lname} ({m:#x})", lacc[l], want.packed[:3], exact or not m & S.LIGHT_IMAGE,
               want.nonfinite | plain.nonfinite)
    _check(f"{what}: the eight main rows", got["acc"], plain.packed, exact, plain.nonfinite)
    assert np.array_equal(got["seeds"], ref.seeds) and got["rays"] == ref.rays, what


@pytest.mark.parametrize("name,K", [("cornell", 1), ("glass", 1), ("box50x37", 2)])
@pytest.mark.parametrize("table", list(ALL_TABLES))
def test_layers_equal_the_masked_oracle(table, name, K, scenes, references):
    r, seeds = _handle(scenes[name], K=K)
    r.set_layers(ALL_TABLES[table])
    got = _render(r, seeds)
    lacc = r.layer_accumulators()
    r.close()
    _assert_layers(f"{name} K={K} table {table}:", got, lacc, ALL_TABLES[table], references(name, K))
    assert np.any(lacc != 0)


@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_layers_with_float_atomics_equal_the_masked_oracle(name, scenes, references):
    """the lay_light atomics: every t = 1 pair in a layer of its own (random_a / random_b spread them over eight layers)"""
    for table in ("light_split", "random_a", "random_b"):
        r, seeds = _handle(scenes[name], det=False)
        r.set_layers(ALL_TABLES[table])
        got = _render(r, seeds)
        lacc = r.layer_accumulators()
        r.close()
        _assert_layers(f"{name} atomics table {table}:", got, lacc, ALL_TABLES[table], references(name), exact=False)


# ---- 4: the other forms of the resolve stage ----
FORMS = {"mode 1": dict(mode=1), "mode 2": dict(mode=2), "mode 5": dict(mode=5), "debug bit 25": dict(flags=1 << 25),
         "flat density": dict(density=True)}


@pytest.mark.parametrize("name", ["cornell", "glass"])
@pytest.mark.parametrize("form", list(FORMS))
def test_the_other_resolve_forms_equal_the_masked_oracle(form, name, scenes, references):
    """One mask through the other launch organisations and through the MAPPED + STRAT kernels (an explicitly set flat sample density
    runs them through run_samples): the accumulators are the masked oracle's bytes."""
    cfg = FORMS[form]
    scene, ref = scenes[name], references(name)
    r, seeds = _handle(scene, mode=cfg.get("mode"), flags=cfg.get("flags", 0))
    if cfg.get("density"):
        r.set_sample_density(np.ones((scene.pixel_height, scene.pixel_width), F))
    r.set_strategy_mask(FORM_MASK)
    got, want = _render(r, seeds), ref.render(FORM_MASK)
    r.close()
    assert np.any(want.packed[:3] != 0)
    _check(f"{name} {form}: the eight rows", got["acc"], want.packed)
    assert np.array_equal(got["seeds"], ref.seeds) and got["rays"] == ref.rays


def test_the_parent_kernel_with_a_full_mask_equals_the_oracle(scenes, references):
    """debug bit 27 launches k_connect_resolve in the slim kernel's place; an explicitly set full mask keeps it"""
    ref = references("open")
    r, seeds = _handle(scenes["open"], flags=1 << 27)
    r.set_strategy_mask(S.ALL)
    got = _render(r, seeds)
    r.close()
    assert np.any(ref.render(None).packed[:3] != 0)
    _check("open scene, debug bit 27, full mask: the eight rows", got["acc"], ref.render(None).packed)
    assert np.array_equal(got["seeds"], ref.seeds) and got["rays"] == ref.rays


# ---- 5: random scenes, each with a drawn mask, layer table, stream count, traversal mode and switch ----
def _load_tool():
    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(ROOT, "tools", "fuzz_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("seed", list(range(600, 612)))          # tests/test_gpu_fuzz.py takes 500..511
def test_random_scene_masked_and_layered(seed, oracle_mod):
    from clive2_amd.renderer import stream_seeds
    fz = _load_tool()
    rng = np.random.RandomState(1000 + seed)
    scene, desc = fz.random_scene(rng)
    case = mo.draw_case(rng)
    B = scene.pixel_width * scene.pixel_height
    problems, left_out = mo.device_check(scene, stream_seeds(B, case["K"], seed=seed), case, passes=2)
    what = f"scene {seed} {desc} tris={len(scene.triangles)} mask={case['mask']:#x} table={[hex(m) for m in case['table'].values()]} " \
           f"K={case['K']} mode={case['mode']} reproducible={case['reproducible']}"
    print(f"{what}: pixels left out of the tolerance comparisons: {left_out}")
    assert not problems, f"{what}: {problems}"
