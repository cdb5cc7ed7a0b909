"""The strategy mask (cl2_set_strategy_mask, csrc/connect_resolve.hpp STRAT) on the device: a masked pair keeps its
MIS weight and loses its colour, nothing else changes.  Frames of 64 x 48 plus one of 50 x 37 (1,850 pixels: a last workgroup with
lanes past the batch).  Floats are compared as bytes with every NaN canonicalised to one pattern; light-image bytes are compared
under the reproducible switch (a fixed summation order)."""
import ctypes as C

import numpy as np
import pytest

from clive2_amd import strategies as S

pytestmark = pytest.mark.gpu

F = np.float32
T2_PAIRS = [(s, t) for t in range(2, 7) for s in range(7)]          # the kernel's order of the t >= 2 pairs: t outer, s inner
T1_PAIRS = [(s, 1) for s in range(1, 7)]
RTOL, ATOL = 5e-5, 1e-8                                              # the parity tests' light-image tolerance (float atomics)
DECOMP = 32.0 * 2.0 ** -24                                           # |P + Q - full| <= DECOMP * (P + Q): nine filter taps and eight
#                                                                      non-negative addends of float32 rounding, with margin


def _b(a):
    """bytes of a float array, every NaN made the same NaN"""
    a = np.array(a, dtype=F, copy=True)
    a[np.isnan(a)] = np.nan
    return a.tobytes()


def _handle(scene, det=True, mode=None, flags=0, variant=None, K=1, seed=20240928):
    from clive2_amd.renderer import Renderer, stream_seeds
    r = Renderer(scene, streams=K, variant=variant)
    seeds = stream_seeds(r.batch_size, K, seed=seed)
    r.set_seeds(seeds)
    r.set_reproducible(det)
    if mode is not None:
        r.set_traversal_mode(mode)
    if flags:
        r.set_debug_flags(flags)
    return r, seeds


def _stages(r, seeds, mask=None, paths=False):
    """One sample through the stage calls, run to the END (the light image is cleared by process_images only), from `seeds`."""
    from clive2_amd.renderer import LIGHT, CAMERA
    r.set_seeds(seeds)
    if mask is not None:
        r.set_strategy_mask(mask)
    r.reset_counters()
    r.make_light_rays(); r.make_camera_rays(); r.trace_light_rays(); r.trace_camera_rays()
    r.join_paths()
    out = dict(agg=r.export_aggregators())
    if paths:
        out.update(conn=r.export_connections(), light_paths=r.export_paths(LIGHT), camera_paths=r.export_paths(CAMERA))
    r.finalize_samples(); r.gather_light_image()
    out.update(r.export_sample_images())
    r.process_images()
    out.update(seeds=r.get_random_buffer(), rays=r.counters()["rays"])
    return out


def _total(o):
    return o["agg"]["total_contribution"][:, :3]


def _same_weights(a, b):
    """aggregator rows 0..8 and 12: the filter weights and contrib_weight_sum"""
    assert _b(a["agg"]["weights"]) == _b(b["agg"]["weights"])
    assert _b(a["agg"]["contrib_weight_sum"]) == _b(b["agg"]["contrib_weight_sum"])


def _same_colourless(a, b):
    """everything that carries no colour: aggregator rows 0..8 and 12, the light weight, the unidirectional image, seeds, rays"""
    _same_weights(a, b)
    assert _b(a["light"][:, 3]) == _b(b["light"][:, 3])
    assert _b(a["unidirectional"]) == _b(b["unidirectional"])
    assert _b(a["sample_weights"]) == _b(b["sample_weights"])
    assert np.array_equal(a["seeds"], b["seeds"]) and a["rays"] == b["rays"]


SCENE_NAMES = ["cornell", "glass"]


@pytest.fixture(scope="module")
def scenes(cornell_small, glass_scene):
    return {"cornell": cornell_small, "glass": glass_scene}


@pytest.fixture(scope="module")
def runs(scenes):
    """Per scene, from one seed buffer and on ONE handle (every run goes through process_images): the unmasked sample, the empty
    mask, the 41 singletons, the light image alone and the camera image alone -- reproducible mode.  Computed once, never written."""
    out = {}
    for name, scene in scenes.items():
        r, seeds = _handle(scene)
        d = dict(full=_stages(r, seeds, None, paths=True), empty=_stages(r, seeds, 0),
                 light_only=_stages(r, seeds, S.LIGHT_IMAGE), camera_only=_stages(r, seeds, S.CAMERA_IMAGE))
        d["single"] = {p: _stages(r, seeds, S.bit(*p)) for p in S.PAIRS}
        r.close()
        out[name] = d
    return out


# ---- 1: a full mask is the default ----
def test_a_full_mask_is_the_default(cornell_small, runs):
    r, seeds = _handle(cornell_small)
    assert r.strategy_mask() == S.ALL                                  # the default
    r.set_strategy_mask(S.ALL)
    assert r.strategy_mask() == S.ALL
    r.set_strategy_mask(2 ** 64 - 1)
    assert r.strategy_mask() == S.ALL                                  # the other 23 bits are dropped
    r.set_strategy_mask(S.bit(0, 2) | 1 | 1 << 63)
    assert r.strategy_mask() == S.bit(0, 2)
    r.set_strategy_mask(None)
    assert r.strategy_mask() == S.ALL
    got, want = _stages(r, seeds), runs["cornell"]["full"]             # the fixture's handle never set a mask before this run
    assert _b(got["agg"]["total_contribution"]) == _b(want["agg"]["total_contribution"])
    _same_colourless(got, want)
    for k in ("finalized", "light"):
        assert _b(got[k]) == _b(want[k]), k
    r.close()
    a, _ = _handle(cornell_small)
    a.set_strategy_mask(S.ALL)                                          # set explicitly: the default kernels
    u, _ = _handle(cornell_small)                                       # untouched
    a.run_samples(3); u.run_samples(3)
    assert _b(a.packed_accumulators()) == _b(u.packed_accumulators())  # all eight rows
    assert np.array_equal(a.get_random_buffer(), u.get_random_buffer())
    a.close(); u.close()


# ---- 2: an empty mask ----
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_an_empty_mask_keeps_every_weight_and_no_colour(name, runs):
    full, empty = runs[name]["full"], runs[name]["empty"]
    assert np.any(_total(full) != 0) and np.any(full["light"][:, :3] != 0)
    assert empty["agg"]["total_contribution"].tobytes() == bytes(empty["agg"]["total_contribution"].nbytes)     # rows 9..11: +0
    assert np.ascontiguousarray(empty["light"][:, :3]).tobytes() == bytes(3 * 4 * len(empty["light"]))
    _same_colourless(empty, full)                                       # rows 0..8, 12, light .w, unidirectional, seeds, rays


# ---- 3: the singletons fold to the whole, exactly ----
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_the_singletons_fold_to_the_whole(name, runs):
    full, single = runs[name]["full"], runs[name]["single"]
    acc = np.zeros_like(_total(full))                                   # +0
    for p in T2_PAIRS:                                                  # the kernel's order
        acc = acc + _total(single[p])                                   # float32 adds, one rounding each
        _same_weights(single[p], full)
    assert acc.dtype == F and _b(acc) == _b(_total(full))
    if name == "cornell":
        # not vacuous: at 64 x 48 and one sample of the default seed every t >= 2 strategy reaches some pixel of the closed box
        empty = [p for p in T2_PAIRS if not np.any(_total(single[p]) != 0)]
        assert empty == []


# ---- 4: attribution ----
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_a_singleton_is_nonzero_only_where_its_pair_exists(name, runs):
    full, single = runs[name]["full"], runs[name]["single"]
    cmask = full["conn"][0]
    Lc, Ll = full["camera_paths"]["length"], full["light_paths"]["length"]
    seen = 0
    for s, t in T2_PAIRS:
        nz = np.any(_total(single[(s, t)]) != 0, axis=1)               # a NaN counts as non-zero
        allowed = (Lc >= t) & (Ll >= s)
        if s >= 1:
            allowed &= ((cmask >> np.uint64((t - 1) * 6 + (s - 1))) & np.uint64(1)).astype(bool)
        else:
            allowed &= full["camera_paths"]["rays"]["hit_light"][:, t - 1] >= 0
        assert not np.any(nz & ~allowed), (s, t)
        seen += int(nz.sum())
    assert seen > 0
    # t = 1: a light-image contribution of (s, 1) exists only where some source pixel has the pair's connection
    for s, _ in T1_PAIRS:
        lit = np.any(single[(s, 1)]["light"][:, :3] != 0)
        has = np.any((Ll >= s) & (Lc >= 1) & ((cmask >> np.uint64(s - 1)) & np.uint64(1)).astype(bool))
        assert has or not lit, s


# ---- 5: light image ----
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_light_image_and_camera_image_split(name, runs):
    full, lo, co, single = (runs[name][k] for k in ("full", "light_only", "camera_only", "single"))
    # t = 1 only: the light image is the unmasked one, the totals are +0
    assert _b(lo["light"]) == _b(full["light"])
    assert lo["agg"]["total_contribution"].tobytes() == bytes(lo["agg"]["total_contribution"].nbytes)
    _same_colourless(lo, full)
    # t >= 2 only: no light colour, every light weight, the totals
    assert np.ascontiguousarray(co["light"][:, :3]).tobytes() == bytes(3 * 4 * len(co["light"]))
    assert _b(co["agg"]["total_contribution"]) == _b(full["agg"]["total_contribution"])
    _same_colourless(co, full)
    # the six t = 1 singletons
    rgb = sum(single[p]["light"][:, :3].astype(np.float64) for p in T1_PAIRS)
    np.testing.assert_allclose(rgb, full["light"][:, :3], rtol=RTOL, atol=ATOL)
    for p in T1_PAIRS:
        assert _b(single[p]["light"][:, 3]) == _b(full["light"][:, 3]), p
        assert single[p]["agg"]["total_contribution"].tobytes() == bytes(single[p]["agg"]["total_contribution"].nbytes)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_light_image_split_with_float_atomics(name, scenes):
    """Without the reproducible switch the splat's order is the hardware's: everything at the light image's tolerance."""
    r, seeds = _handle(scenes[name], det=False)
    full = _stages(r, seeds, None)
    lo, co = _stages(r, seeds, S.LIGHT_IMAGE), _stages(r, seeds, S.CAMERA_IMAGE)
    single = {p: _stages(r, seeds, S.bit(*p)) for p in T1_PAIRS}
    r.close()
    assert np.any(full["light"][:, :3] != 0)
    np.testing.assert_allclose(lo["light"], full["light"], rtol=RTOL, atol=ATOL)
    assert not np.any(_total(lo) != 0)
    assert not np.any(co["light"][:, :3] != 0)
    np.testing.assert_allclose(co["light"][:, 3], full["light"][:, 3], rtol=RTOL, atol=ATOL)
    assert _b(co["agg"]["total_contribution"]) == _b(full["agg"]["total_contribution"])      # no atomics in the totals
    rgb = sum(single[p]["light"][:, :3].astype(np.float64) for p in T1_PAIRS)
    np.testing.assert_allclose(rgb, full["light"][:, :3], rtol=RTOL, atol=ATOL)
    for p in T1_PAIRS:
        np.testing.assert_allclose(single[p]["light"][:, 3], full["light"][:, 3], rtol=RTOL, atol=ATOL)
        _same_weights(single[p], full)


# ---- 6: decomposition through the pipeline ----
def _pipeline(scene, mask, K=2, passes=4, density=None, seed=20240928):
    r, _ = _handle(scene, K=K, seed=seed)
    if density is not None:
        r.set_sample_density(density)
    r.set_strategy_mask(mask)
    r.run_samples(passes)
    out = r.packed_accumulators().reshape(8, -1), r.get_random_buffer()
    r.close()
    return out


def _assert_decomposition(parts, full, addends=None):
    """The parts add up to the whole within DECOMP.  Every value must be finite and is checked, unless `addends` is given: (n, 3)
    per-sample addends BEFORE the scrub, and a pixel is left out where one of them is not finite -- at most 0.1 % of the pixels."""
    total = sum(p.astype(np.float64) for p in parts)
    full = full.astype(np.float64)
    if addends is not None:
        bad = ~np.all(np.isfinite(np.stack(addends).astype(np.float64)), axis=(0, 2))
        print("decomposition: pixels left out for a non-finite addend:", int(bad.sum()), "of", bad.size)
        assert bad.sum() <= bad.size // 1000
        total, full = total[~bad], full[~bad]
    assert np.all(np.isfinite(total)) and np.all(np.isfinite(full)) and np.all(total >= 0)
    err = np.abs(total - full)
    print("decomposition: max |sum - full| / sum =", float(np.max(err / np.maximum(total, 1e-300))), "bound", DECOMP)
    assert np.all(err <= DECOMP * total)
    assert np.any(total > 0)


def test_masked_renders_decompose_the_picture(cornell_small):
    from clive2_amd.renderer import stream_seeds
    P, Q = S.path_length(1, 2), S.path_length(3)
    (accP, sP), (accQ, sQ), (acc, s) = (_pipeline(cornell_small, m) for m in (P, Q, None))
    for a, sd in ((accP, sP), (accQ, sQ)):
        assert _b(a[3:8]) == _b(acc[3:8])                              # weights, unidirectional rows, sample counts
        assert np.array_equal(sd, s)
    assert np.any(accP[:3] != 0) and np.any(accQ[:3] != 0)
    _assert_decomposition([accP[:3], accQ[:3]], acc[:3])
    # the same through render_layers
    r, seeds = _handle(cornell_small, K=2)
    r.set_strategy_mask(S.bit(1, 2))
    layers = r.render_layers(4, seeds=seeds)
    assert r.strategy_mask() == S.bit(1, 2)                            # left as found
    assert list(layers) == ["emission", "direct", "indirect"]
    assert all(v.shape == (48, 64, 3) and v.dtype == F for v in layers.values())
    r.set_strategy_mask(None)
    r.reset_accumulators(); r.set_seeds(stream_seeds(r.batch_size, 2))
    r.run_samples(4)
    assert _b(r.packed_accumulators()) == _b(acc)                      # the unmasked render of the same seeds
    _assert_decomposition(list(layers.values()), r.radiance)
    assert all(np.any(v != 0) for v in layers.values())
    r.close()


# ---- 7: independence of the launch organisation ----
def _masked_sample(scene, mode=None, flags=0):
    r, seeds = _handle(scene, mode=mode, flags=flags)
    o = _stages(r, seeds, S.path_length(3))
    r.close()
    return o


@pytest.mark.parametrize("name,size", [("cornell", (64, 48)), ("glass", (64, 48)), ("cornell", (50, 37))])
def test_masked_results_do_not_depend_on_the_launch_organisation(name, size, scenes):
    import clive2_amd as c2
    scene = scenes[name] if size == (64, 48) else c2.create_scene_from_preset("empty", *size)
    want = _masked_sample(scene)
    assert np.any(_total(want) != 0)
    for mode, flags in ((1, 0), (2, 0), (5, 0), (None, 1 << 25)):
        got = _masked_sample(scene, mode, flags)
        assert _b(got["agg"]["total_contribution"]) == _b(want["agg"]["total_contribution"]), (mode, flags)
        _same_colourless(got, want)
        assert _b(got["light"]) == _b(want["light"]), (mode, flags)
    if size != (64, 48):
        # the ragged frame against its own unmasked sample: every w, and the fold of the two halves
        r, seeds = _handle(scene)
        full, rest = _stages(r, seeds, None), _stages(r, seeds, S.path_length(1, 2))
        r.close()
        _same_colourless(want, full); _same_colourless(rest, full)
        _assert_decomposition([_total(rest), _total(want)], _total(full), addends=[_total(rest), _total(want), _total(full)])


def test_masked_mapped_kernels_decompose_the_picture(cornell_small):
    """An explicitly set flat sample density runs the MAPPED kernels through run_samples."""
    flat = np.ones((48, 64), F)
    (accP, sP), (accQ, sQ) = (_pipeline(cornell_small, m, density=flat) for m in (S.path_length(1, 2), S.path_length(3)))
    acc, s = _pipeline(cornell_small, None)
    for a, sd in ((accP, sP), (accQ, sQ)):
        assert _b(a[3:8]) == _b(acc[3:8]) and np.array_equal(sd, s)
    _assert_decomposition([accP[:3], accQ[:3]], acc[:3])


# ---- 8: state and refusals ----
def test_the_mask_survives_uploads_stream_changes_and_resets(cornell_small):
    r, seeds = _handle(cornell_small)
    m = S.path_length(2, 4)
    r.set_strategy_mask(m)
    r.upload_scene(cornell_small)
    assert r.strategy_mask() == m
    r.set_sample_streams(2)
    assert r.strategy_mask() == m
    r.set_sample_streams(1)
    r.reset_accumulators()
    assert r.strategy_mask() == m
    r.set_strategy_mask([(0, 2), (1, 1)])
    assert r.strategy_mask() == S.bit(0, 2) | S.bit(1, 1)
    with pytest.raises(ValueError):
        r.set_strategy_mask([(0, 1)])
    assert r.strategy_mask() == S.bit(0, 2) | S.bit(1, 1)
    # NULL handle, NULL out pointer: CL2_E_INVALID
    out = C.c_uint64(0)
    assert r._L.cl2_set_strategy_mask(None, C.c_uint64(m)) == -1
    assert r._L.cl2_get_strategy_mask(None, C.byref(out)) == -1
    assert r._L.cl2_get_strategy_mask(r._h, None) == -1
    # render_layers leaves the mask as it found it, also when a layer is refused
    r.render_layers(1, {"a": S.bit(0, 2), "b": [(1, 2)]}, seeds=seeds)
    assert r.strategy_mask() == S.bit(0, 2) | S.bit(1, 1)
    with pytest.raises(ValueError):
        r.render_layers(1, {"a": S.bit(0, 2), "bad": [(0, 1)]})
    assert r.strategy_mask() == S.bit(0, 2) | S.bit(1, 1)
    r.close()


def test_the_cross_check_resolve_kernel_has_no_masked_form(cornell_small):
    from clive2_amd.renderer import RendererError
    WIDE = 7 << 4
    r, seeds = _handle(cornell_small, det=False, variant="test")
    r.set_strategy_mask(S.path_length(3))
    with pytest.raises(RendererError):
        r.set_debug_flags(WIDE)
    assert r.strategy_mask() == S.path_length(3)
    masked = _stages(r, seeds)                                           # the flags were not taken: the masked kernel runs
    assert np.any(_total(masked) != 0)
    r.set_strategy_mask(None)
    r.set_debug_flags(WIDE)                                             # a full mask goes with the cross-check kernel
    with pytest.raises(RendererError):
        r.set_strategy_mask(S.path_length(3))
    assert r.strategy_mask() == S.ALL
    r.set_strategy_mask(S.ALL)                                          # ... and may be set again
    full = _stages(r, seeds)                                             # the cross-check kernel runs
    r.set_debug_flags(0)
    again = _stages(r, seeds, S.path_length(3))
    assert _b(_total(again)) == _b(_total(masked))
    _same_weights(again, full)
    r.close()


# ---- the command line ----
def test_render_writes_the_layers_and_a_masked_picture(tmp_path):
    """render.py in this process: --layers writes three pictures mapped with ONE log-average and the float layers, which add up to
    the plain render of the same seeds; --path-length renders one masked picture."""
    import glob
    import os
    from clive2_amd import render
    from clive2_amd.renderer import Renderer, stream_seeds
    import clive2_amd as c2
    prefix = str(tmp_path / "box")
    common = ["--scene", "empty", "--width", "64", "--height", "48", "--samples", "2", "--reproducible"]
    assert render.main(common + ["--layers", prefix]) == 0
    for name in ("emission", "direct", "indirect"):
        assert glob.glob(f"{prefix}_{name}.png*"), name                    # .png, or .png.npy without PIL
    layers = np.load(prefix + "_layers.npz")
    assert sorted(layers.files) == ["direct", "emission", "indirect"]
    r = Renderer(c2.create_scene_from_preset("empty", 64, 48), seeds=stream_seeds(64 * 48, 1))
    r.set_reproducible(True)
    r.run_samples(2)
    _assert_decomposition([layers[k] for k in layers.files], r.radiance)
    r.close()
    out = str(tmp_path / "indirect.png")
    assert render.main(common + ["--path-length", "3:", "--out", out]) == 0
    assert glob.glob(out + "*")
    assert render.main(common + ["--strategies", "0,2;1,2", "--out", out]) == 0
