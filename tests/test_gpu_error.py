"""Error tracking on the device: the moment sums against their float32 restatement (tests/error_reference.py) on the stage,
fused and import paths, the derived standard errors and frame metric, that tracking changes nothing else, render_until's
stopping rule, the validity rules of the moments, and the estimate's calibration on real renders."""
import numpy as np
import pytest

import error_reference as er
from test_gpu_denoise import _cornell, _glass, _open_scene

pytestmark = pytest.mark.gpu

SCENES = {"cornell": lambda: _cornell(64, 48), "glass": lambda: _glass(64, 48), "open": lambda: _open_scene(72, 40)}
INT_COUNTERS = ("rays", "conn_rays", "box_tests", "tri_tests", "counted_rays", "samples", "launches_traverse_paths",
                "launches_traverse_conn", "rays_traverse_paths", "rays_traverse_conn")


def _renderer(scene, K, seed=20240928, tracking=True, mode=None):
    from clive2_amd.renderer import Renderer, stream_seeds
    r = Renderer(scene, streams=K)
    r.set_seeds(stream_seeds(r.batch_size, K, seed=seed))
    r.set_reproducible(True)
    if mode is not None:
        r.set_traversal_mode(mode)
    if tracking:
        r.set_error_tracking(True)
    return r


@pytest.mark.parametrize("name,K", [("cornell", 1), ("cornell", 2), ("glass", 1), ("glass", 2), ("open", 4)])
def test_moments_are_exact_on_the_stage_and_fused_paths(name, K):
    """Six passes as stage calls, each stream's per-sample images exported before process_images and its addends restated in
    numpy: the device moments equal the float32 sums bit for bit.  A fresh handle with the same seeds through run_samples(6)
    (k_finalize_accumulate<true>) gives the same moment and accumulator bytes.  The open scene is a mesh scene on the 4-wide walk."""
    scene = SCENES[name]()
    mode = 5 if name == "open" else None
    r = _renderer(scene, K, mode=mode)
    if name == "open":
        assert r.organisation()["wide_nodes"] > 0
    mom = np.zeros((8, r.batch_size), np.float32)
    for _ in range(6):
        r.make_light_rays(); r.make_camera_rays(); r.trace_light_rays(); r.trace_camera_rays()
        r.join_paths(); r.finalize_samples(); r.gather_light_image()
        for k in range(K):
            r.set_export_stream(k)
            im = r.export_sample_images()
            x, w = er.addends(im["finalized"], im["light"], im["sample_weights"])
            er.add_moments(mom, x, w)
        r.process_images()
    got = r.moments().reshape(8, -1)
    assert got.tobytes() == mom.tobytes()
    acc_stage = r.packed_accumulators()
    assert (acc_stage.reshape(8, -1)[7] == 6 * K).all()

    f = _renderer(scene, K, mode=mode)
    f.run_samples(6)
    assert f.moments().tobytes() == got.tobytes()
    assert f.packed_accumulators().tobytes() == acc_stage.tobytes()


def test_moments_of_imported_samples_scrub_non_finite_colour():
    """Synthetic per-sample images through import_sample_images + process_images, NaN and +-inf in the finalized colour: the
    moments are those of the scrubbed addends, bit for bit."""
    r = _renderer(_cornell(64, 48), 1)
    B = r.batch_size
    rs = np.random.RandomState(5)
    mom = np.zeros((8, B), np.float32)
    for p in range(3):
        fin = rs.gamma(1.0, 0.5, size=(B, 4)).astype(np.float32)
        fin[:, 3] = 1.0
        light = rs.gamma(1.0, 0.1, size=(B, 4)).astype(np.float32)
        sw = rs.uniform(0.5, 2.0, size=B).astype(np.float32)
        uni = rs.gamma(1.0, 0.5, size=(B, 4)).astype(np.float32)
        bad = rs.choice(B, size=60, replace=False)
        fin[bad[:20], 0] = np.nan
        fin[bad[20:40], 1] = np.inf
        fin[bad[40:], 2] = -np.inf
        r.import_sample_images(finalized=fin, light=light, sample_weights=sw, unidirectional=uni)
        r.process_images()
        x, w = er.addends(fin, light, sw)
        er.add_moments(mom, x, w)
    got = r.moments().reshape(8, -1)
    assert np.isfinite(got).all()
    assert got.tobytes() == mom.tobytes()


def test_standard_error_and_frame_metric_match_numpy():
    r = _renderer(_cornell(64, 48), 1)
    r.run_samples(1)
    assert r.relative_error(0.05) == np.inf                       # one sample: no variance yet
    se1 = r.standard_error()
    assert np.isinf(se1[r.read_accumulators()[1][..., 0] > 0]).all()
    r.run_samples(7)
    acc, mom = r.packed_accumulators(), r.moments()
    se = r.standard_error()
    want = er.standard_error(acc, mom, r.pixel_height, r.pixel_width)
    assert se.shape == (48, 64, 4) and se.dtype == np.float32
    assert np.isfinite(se).all() and (se > 0).any()
    np.testing.assert_allclose(se, want, rtol=1e-6, atol=0)
    for floor in (0.0, 0.01, 0.05, 0.5):
        e = r.relative_error(floor)
        assert np.isfinite(e)
        assert e == pytest.approx(er.relative_error(acc, mom, floor), rel=1e-12)
    assert r.standard_error().tobytes() == se.tobytes()
    a, b = np.float64(r.relative_error(0.05)), np.float64(r.relative_error(0.05))
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name,K", [("cornell", 1), ("open", 4)])
def test_tracking_changes_nothing_else(name, K):
    scene = SCENES[name]()
    a = _renderer(scene, K, tracking=False)
    b = _renderer(scene, K, tracking=True)
    a.run_samples(8)
    b.run_samples(8)
    assert a.packed_accumulators().tobytes() == b.packed_accumulators().tobytes()
    assert a.get_random_buffer().tobytes() == b.get_random_buffer().tobytes()
    ca, cb = a.counters(), b.counters()
    assert {k: ca[k] for k in INT_COUNTERS} == {k: cb[k] for k in INT_COUNTERS}
    assert not a.error_tracking and b.error_tracking


def test_render_until_stops_at_the_first_boundary_below_target():
    scene = _cornell(64, 48)
    probe = _renderer(scene, 1)
    e = []
    for _ in range(4):
        probe.run_samples(8)
        e.append(probe.relative_error())
    assert e[1] > e[2], e
    target = 0.5 * (e[1] + e[2])                               # e(16) > target >= e(24)
    r = _renderer(scene, 1)
    done, reached = r.render_until(target, 32, min_samples=0, check_every=8)
    assert done == 24 and r.samples == 24
    assert reached == e[2]
    ref = _renderer(scene, 1)
    ref.run_samples(24)
    assert r.packed_accumulators().tobytes() == ref.packed_accumulators().tobytes()
    assert r.moments().tobytes() == ref.moments().tobytes()
    # unreachable: stops at the cap, chunks 2, 2, 1 after min_samples = 2
    u = _renderer(scene, 1)
    done, reached = u.render_until(1e-9, 7, min_samples=2, check_every=2)
    assert done == 7 and u.samples == 7 and reached > 1e-9
    assert (u.read_accumulators()[2] == 7).all()


def test_state_rules():
    from clive2_amd.renderer import RendererError
    r = _renderer(_cornell(64, 48), 1, tracking=False)
    assert not r.error_tracking
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.relative_error()
    r.run_samples(2)
    r.set_error_tracking(True)                                  # the accumulators already hold samples: invalid
    assert r.error_tracking
    for call in (r.relative_error, r.standard_error, r.moments):
        with pytest.raises(RendererError, match=r"\(-3\)"):
            call()
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.render_until(0.1, 4)
    r.reset_accumulators()
    assert not r.moments().any()                                 # reset zeroes them and makes them valid
    r.run_samples(3)
    acc, mom, e = r.packed_accumulators(), r.moments(), r.relative_error()
    r.load_packed_accumulators(acc)
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.relative_error()
    r.load_moments(mom)
    assert r.moments().tobytes() == mom.tobytes()
    assert r.relative_error() == e
    with pytest.raises(RendererError, match=r"\(-1\)"):
        r.render_until(0.1, 4, check_every=0)
    with pytest.raises(RendererError, match=r"\(-1\)"):
        r.render_until(0.1, 4, min_samples=5)
    with pytest.raises(RendererError, match=r"\(-1\)"):
        r.relative_error(-1.0)
    r.set_error_tracking(False)
    assert not r.error_tracking
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.moments()


def test_estimate_is_calibrated_on_real_renders():
    """24 renders of the 64 x 48 Cornell box with different seeds, 32 samples each: over the covered pixels, the median of
    (variance of the luma radiance across the renders) / (mean predicted variance) lies in [0.6, 1.6]; quadrupling the samples
    scales e by 0.4-0.6.  Measured on the MI355X: median ratio 0.97 (quartiles 0.79 / 1.19) over 3,072 pixels;
    e(128) / e(32) = 0.50.  The Cornell box is diffuse-only, so the heavy tails that bias a 32-sample variance low are mild here."""
    from clive2_amd.renderer import Renderer, make_seeds
    scene = _cornell(64, 48)
    lumas, pred = [], []
    for i in range(24):
        r = Renderer(scene, seeds=make_seeds(64 * 48, seed=1000 + i))
        r.set_error_tracking(True)
        r.run_samples(32)
        rad = r.radiance.astype(np.float64)
        lumas.append((rad[..., 0] * np.float64(np.float32(0.0722)) + rad[..., 1] * np.float64(np.float32(0.7152)))
                     + rad[..., 2] * np.float64(np.float32(0.2126)))
        pred.append(r.standard_error()[..., 3].astype(np.float64) ** 2)
        if i == 0:
            e32 = r.relative_error()
            r.run_samples(96)
            e128 = r.relative_error()
        r.close()
    emp = np.var(np.stack(lumas), axis=0, ddof=1)
    mp = np.mean(np.stack(pred), axis=0)
    ok = mp > 0
    ratio = emp[ok] / mp[ok]
    q1, med, q3 = np.percentile(ratio, [25, 50, 75])
    print(f"calibration: {ok.sum()} pixels, ratio quartiles {q1:.3f} {med:.3f} {q3:.3f}; e32 {e32:.4f} e128 {e128:.4f} "
          f"-> {e128 / e32:.3f}")
    assert 0.6 <= med <= 1.6
    assert 0.4 <= e128 / e32 <= 0.6
