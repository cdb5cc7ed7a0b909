"""Error tracking on the device: the moment sums against their float32 restatement (tests/error_reference.py) on the stage,
fused and import paths, the derived standard errors and frame metric, that tracking changes nothing else, render_until's
stopping rule, the validity rules of the moments, and the estimate's calibration on real renders.

The standard errors and the frame metric are also computed from injected states (tests/error_states.py: every branch of
err_pixel in every wave of some workgroups, frames from less than a wave to the 8 grid-stride trips of 1920 x 1080) and
compared with the restatement bit for bit -- the frame metric's sum in the device's reduction order (error_reference.grid_sum)
-- and the device's S is held against the residual sum of squares of the addends that made its moments."""
import numpy as np
import pytest

import error_reference as er
import error_states as es
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
    assert se.view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    for floor in (0.0, 0.01, 0.05, 0.5):
        e = r.relative_error(floor)
        assert np.isfinite(e)
        assert np.float64(e).tobytes() == np.float64(er.relative_error(acc, mom, floor)).tobytes()
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


# ---------------------------------------------------------------- injected states
FLOORS = (0.0, 0.001, 0.05, 0.5)


@pytest.fixture(scope="module")
def pool():
    return es.pool()


@pytest.fixture(scope="module")
def handles():
    """one handle per frame for the whole module (the 1920 x 1080 one is made once)"""
    made = {}

    def get(W, H):
        if (W, H) not in made:
            made[W, H] = _renderer(_cornell(W, H), 1)
        return made[W, H]
    yield get
    for r in made.values():
        r.close()


def _load(r, acc, mom):
    r.load_packed_accumulators(acc)
    r.load_moments(mom)


def _bits64(x):
    return np.float64(x).tobytes()


def _assert_metric(r, acc, mom, floors=FLOORS):
    """relative_error at every floor equals the grid_sum restatement bit for bit; returns the values"""
    out = []
    for floor in floors:
        got, want = r.relative_error(floor), er.relative_error(acc, mom, floor)
        assert _bits64(got) == _bits64(want), (floor, got, want)
        out.append(got)
    return out


@pytest.mark.parametrize("W,H", es.FRAMES)
def test_injected_states_standard_error_and_metric_bitwise(W, H, pool, handles):
    """Per frame: (1) every class (error_states.ALL): standard_error() bit for bit, no NaN, the frame metric +inf (covered pixels
    with n < 2); (2) without the n < 2 and overflowed pixels: +inf at floor 0 from the L + floor = 0 pixels, finite from floor
    0.001 on, bit for bit; (3) the well-scaled classes: finite and bit for bit at every floor, the same bytes on a second call."""
    r = handles(W, H)
    FB = W * H
    cls, acc, mom = es.state(pool, FB, es.ALL)
    if FB >= 576:
        assert set(np.unique(cls)) == set(es.ALL)
    _load(r, acc, mom)
    se = r.standard_error()
    want = er.standard_error(acc, mom, H, W)
    assert not np.isnan(se).any()
    bad = np.argwhere(se.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (len(bad), [(cls[y * W + x], se[y, x, c], want[y, x, c]) for y, x, c in bad[:5]])
    assert (se.reshape(-1, 4)[cls == es.UNCOVERED] == 0).all() and np.isinf(se.reshape(-1, 4)[cls == es.FEW]).all()
    if (cls == es.TINY).any():
        assert (se.reshape(-1, 4)[cls == es.TINY] > 0).any()          # subnormal sums read as their values, not flushed
    assert r.standard_error().tobytes() == se.tobytes()
    if (cls == es.FEW).any():
        assert _assert_metric(r, acc, mom) == [np.inf] * 4

    cls, acc, mom = es.state(pool, FB, es.NO_FEW)
    _load(r, acc, mom)
    e = _assert_metric(r, acc, mom)
    if (cls == es.SIGNED).any():
        assert e[0] == np.inf and np.isfinite(e[1:]).all(), e

    cls, acc, mom = es.state(pool, FB, es.BASE)
    _load(r, acc, mom)
    e = _assert_metric(r, acc, mom)
    assert np.isfinite(e).all() and all(x > 0 for x in e), e
    assert _bits64(r.relative_error(0.05)) == _bits64(e[2])
    se = r.standard_error()
    assert se.view(np.uint32).tobytes() == er.standard_error(acc, mom, H, W).view(np.uint32).tobytes()


@pytest.mark.parametrize("W,H", es.FRAMES)
def test_injected_states_frame_outcomes(W, H, pool, handles):
    """The frame-level branches on the well-scaled state: one covered pixel with n < 2 (n = 1, exactly noiseless: S * scale would be
    0 * inf) in the frame's last wave, in the last wave of the grid's last workgroup and, from 262,145 pixels on, in a second-trip
    position makes the metric
    +inf; nothing covered: +inf; covered pixels in one workgroup only, and only pixel FB - 1 covered: finite, bit for bit."""
    r = handles(W, H)
    FB = W * H
    cls, acc, mom = es.state(pool, FB, es.BASE)
    fa, fm = es.few_pixel(pool)
    spots = [FB - 1 - (FB - 1) % 64 + min(3, (FB - 1) % 64)]            # in the frame's last wave
    if FB >= 1024 * 256:
        spots.append(1023 * 256 + 192 + 3)                               # workgroup 1,023 of 1,024, its last wave
    if FB > 1024 * 256:
        spots.append(1024 * 256 + 256 + 70)                              # workgroup 1's second trip, its second wave
    for p in spots:
        a, m = acc.copy(), mom.copy()
        a[:, p], m[:, p] = fa, fm
        _load(r, a, m)
        assert _assert_metric(r, a, m, (0.0, 0.05)) == [np.inf, np.inf]
        se = r.standard_error().reshape(-1, 4)
        assert np.isinf(se[p]).all() and se.view(np.uint32).tobytes() == er.standard_error(a, m).view(np.uint32).tobytes()
    # nothing covered
    a = acc.copy()
    a[3] = np.where(np.arange(FB) % 2 == 0, np.float32(0.0), np.float32(np.nan))
    _load(r, a, mom)
    assert _assert_metric(r, a, mom, (0.0, 0.05)) == [np.inf, np.inf]
    assert not r.standard_error().any()
    # covered pixels in one workgroup only (its first-trip pixels); every other partial is (0, 0, 0)
    b = min(3, (FB - 1) // 256)
    inside = (np.arange(FB) >= 256 * b) & (np.arange(FB) < 256 * b + 256)
    a = acc.copy()
    a[3] = np.where(inside, acc[3], np.float32(0.0))
    _load(r, a, mom)
    e = _assert_metric(r, a, mom)
    assert np.isfinite(e).all() and e[1] > 0
    # only the last pixel covered
    a, m = acc.copy(), mom.copy()
    a[3] = 0.0
    a[:, FB - 1], m[:, FB - 1] = pool[1][:, 0], pool[2][:, 0]            # the pool's first state: ordinary, n = 2
    _load(r, a, m)
    e = _assert_metric(r, a, m)
    assert np.isfinite(e).all() and e[1] > 0
    _, var, L = er.variances(a[:, FB - 1:], m[:, FB - 1:])
    assert e[2] == np.sqrt(var[0, 3] / ((L[0] + 0.05) * (L[0] + 0.05)))


@pytest.mark.parametrize("W,H", [(41, 25), (512, 513)])
@pytest.mark.parametrize("n", [2, 8, 64])
def test_device_estimate_against_the_residual_sum_of_squares(W, H, n, handles):
    """The addends of every regime of test_error_estimate_cpu.test_float32_restatement_is_inside_the_derived_bound through
    import_sample_images + process_images, so that the moments are k_accumulate<true>'s own: they equal add_moments' bit for
    bit, and standard_error() stays inside |S - S*| <= 8 n u T against the float64 residual sums of the same addends (the bound
    and its two consequences: see that test's docstring).  The regimes share the frame: pixel p is of regime p mod 5."""
    r = handles(W, H)
    FB = W * H
    seqs = [es.addend_sequence(regime, FB, n, seed=2000 + n) for regime in es.REGIMES]
    which = np.arange(FB) % len(es.REGIMES)
    xs = [np.choose(which[:, None], [s[0][i] for s in seqs]).astype(np.float32) for i in range(n)]
    ws = [np.choose(which, [s[1][i] for s in seqs]).astype(np.float32) for i in range(n)]
    r.reset_accumulators()
    zero4 = np.zeros((FB, 4), np.float32)
    for x, w in zip(xs, ws):
        fin = np.concatenate([x, np.ones((FB, 1), np.float32)], axis=1)
        r.import_sample_images(finalized=fin, light=zero4, sample_weights=w, unidirectional=zero4)
        r.process_images()
    acc_ref, mom_ref = es.accumulate(xs, ws)
    acc = r.packed_accumulators().reshape(8, -1)
    assert r.moments().reshape(8, -1).tobytes() == mom_ref.tobytes()
    assert acc[:4].tobytes() == acc_ref[:4].tobytes() and (acc[7] == n).all()
    se = r.standard_error()
    assert se.view(np.uint32).tobytes() == er.standard_error(acc, mom_ref, H, W).view(np.uint32).tobytes()
    Sstar, T = er.residual_sums(xs, ws)
    for k, regime in enumerate(es.REGIMES):
        at = which == k
        er.check_against_residual_sums(se.reshape(-1, 4)[at], acc[:, at], Sstar[at], T[at], n, f"device {W}x{H} {regime} n={n}")
    r.reset_accumulators()
