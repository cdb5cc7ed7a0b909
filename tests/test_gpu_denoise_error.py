"""The error estimate of the filtered picture on the device (csrc/denoise_error.hpp, cl2_denoise_error) against its numpy statement
(tests/denoise_error_reference.py), on injected accumulator / moment / feature states: the filter's bytes, the perturbed picture
bit for bit, the map and the totals bit for bit, the states, that nothing else moves; then render_until on the new metric and the
calibration of the estimate on real renders of the Cornell box."""
import ctypes as C

import numpy as np
import pytest

import denoise_error_reference as de
import denoise_scenes as ds
import error_reference as er
import error_states as es
import feature_states as fs

pytestmark = pytest.mark.gpu

F = np.float32
FRAMES = [(7, 5), (41, 25)]          # one ragged tile; 3 x 2 tiles with a ragged edge, 3 passes reach the global-load form
KINDS = ("denoised", "guided")
SIGMA = {"denoised": "sigma_color", "guided": "sigma_luma"}
EPS = 1 / 16


@pytest.fixture(scope="module")
def pool():
    return es.pool()


class Case:
    """a handle with injected accumulators, moments and features, and what k_de_input makes of them"""

    def __init__(self, W, H, acc, mom):
        from clive2_amd.renderer import Renderer
        self.W, self.H = W, H
        self.scene = ds.cornell(W, H)
        self.r = r = Renderer(self.scene)
        r.set_error_tracking(True)
        _, n, z, a, cov = fs.features(W, H)
        self.acc, self.mom = acc, mom
        r.load_packed_accumulators(acc)
        r.load_moments(mom)
        r.load_features(n, z, a, cov)
        self.f = dict(normal=n, depth=z, albedo=a, coverage=cov)
        self.y, self.state, self.v, self.a, self.w = de.inputs(acc, mom, W, H)
        self.K = de.camera_kernel(self.scene)

    def call(self, kind, **kw):
        return self.r.denoised_error(kind, epsilon=EPS, return_map=True, return_totals=True, return_probe=True, **kw)

    def restated(self, kind, probes, floor, correlated):
        """(map, out) of the restatement on the device's own y', F(y), F(y') of `probes` single-probe calls"""
        yps, Fyps = zip(*[(p[0], p[2]) for p in probes])
        return de.terms(self.y, yps, probes[0][1], Fyps, self.state, self.v, EPS, floor)


@pytest.fixture(scope="module")
def cases(pool):
    """per frame: 'all' = the calm colours of feature_states under the moments of every class of error_states (variances beyond
    float32, overflowed sums, n < 2, subnormals: the bitwise tests), 'base' = the well-scaled classes alone (where a comparison
    with a tolerance means something)"""
    made = {}

    def get(W, H, which):
        if (W, H, which) not in made:
            if which == "all":
                cls = fs.features(W, H)[0]
                acc = fs.colours(cls, pool, wild=False)[1]
                mom = es.state(pool, W * H, es.ALL)[2]
            else:
                _, acc, mom = es.state(pool, W * H, es.BASE)
            made[(W, H, which)] = Case(W, H, acc, mom)
        return made[(W, H, which)]
    yield get
    for c in made.values():
        c.r.close()


@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_filtered_picture_is_the_filters_own(W, H, kind, cases):
    """F(y) of the probe output is denoised_radiance / guided_radiance of the same parameters byte for byte, at 0, 1 and 3 passes"""
    c = cases(W, H, "all")
    for it in (0, 1, 3):
        for sig in ((2.0, 0.1, 0.1), (0.7, 0.02, 0.3)):
            _, _, _, (yp, Fy, Fyp) = c.call(kind, iterations=it, sigma=sig[0], sigma_depth=sig[1], sigma_albedo=sig[2])
            kw = {SIGMA[kind]: sig[0], "sigma_depth": sig[1], "sigma_albedo": sig[2]}
            want = c.r.denoised_radiance(iterations=it, **kw) if kind == "denoised" else c.r.guided_radiance(iterations=it, **kw)
            assert Fy.tobytes() == want.tobytes(), (kind, it, sig)
            if it == 0:
                assert Fy.tobytes() == c.y.tobytes() and Fyp.tobytes() == yp.tobytes()


@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("correlated", [0, 1])
def test_perturbed_picture_bit_for_bit(W, H, correlated, cases):
    """y' equals the restatement bit for bit: border pixels, and states 0 and 1 (unperturbed) included"""
    c = cases(W, H, "all")
    assert (c.state == 0).any() and (c.state == 1).any() and (c.state == 2).any()
    for kind in KINDS:
        for seed in (0, 7, 0xFFFFFFFF):
            yp = c.call(kind, iterations=1, correlated=correlated, seed=seed)[3][0]
            z = de.field(W, H, seed, correlated, c.K)
            want = de.perturb(c.y, c.a, z, EPS)
            assert np.isfinite(want).all()
            assert yp.tobytes() == want.tobytes(), (kind, seed)
            assert yp[c.state != 2].tobytes() == c.y[c.state != 2].tobytes()
            assert (yp != c.y).any(axis=-1)[c.state == 2].mean() > 0.5
    # probe k of seed S is probe 0 of seed S + k: the LAST probe's y' of a 3-probe call
    yp3 = c.call("denoised", iterations=0, correlated=correlated, seed=5, probes=3)[3][0]
    assert yp3.tobytes() == de.perturb(c.y, c.a, de.field(W, H, 7, correlated, c.K), EPS).tobytes()


@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("correlated", [0, 1])
def test_filter_of_the_perturbed_picture_equals_numpy(W, H, kind, correlated, cases):
    """F(y') against the numpy filter of the device's y', rtol 1e-4 and atol 1e-6, on the well-scaled states"""
    c = cases(W, H, "base")
    for it in (1, 3):
        _, _, _, (yp, Fy, Fyp) = c.call(kind, iterations=it, correlated=correlated, seed=3)
        p = dict(de.DEFAULTS[de.KINDS[kind]], iterations=it)
        want = de.run_filter(de.KINDS[kind], yp, c.w, c.f, **p)
        assert np.isfinite(Fyp).all()
        np.testing.assert_allclose(Fyp, want, rtol=1e-4, atol=1e-6, err_msg=f"{kind} {it} passes")
        assert (Fyp != Fy).any()


@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("correlated", [0, 1])
@pytest.mark.parametrize("which", ["all", "base"])
def test_map_and_totals_bit_for_bit(W, H, kind, correlated, which, cases):
    """probes = 1: the map and all eight totals equal the restatement evaluated on the device's own y', F(y), F(y') and the
    injected acc / mom; probes = 4: the restatement built from four single-probe calls with seeds S .. S+3; two calls give the
    same bytes.  (A NaN -- inf - inf among the overflowed classes -- counts as equal to a NaN.)"""
    c = cases(W, H, which)
    S, floor = 0xFFFFFFFE, 0.001                    # S + 2 wraps
    singles = []
    for k in range(4):
        e, m, out, probe = c.call(kind, iterations=3, correlated=correlated, seed=S + k, floor=floor)
        wm, wout = c.restated(kind, [probe], floor, correlated)
        assert de.same(m, wm), (kind, k)
        assert de.same(out, wout), (kind, k, out, wout)
        assert de.same(np.float64(e), np.float64(wout[0]))
        singles.append(probe)
    e, m, out, probe = c.call(kind, iterations=3, correlated=correlated, seed=S, floor=floor, probes=4)
    wm, wout = c.restated(kind, singles, floor, correlated)
    assert de.same(m, wm) and de.same(out, wout), (out, wout)
    assert all(de.same(x, y) for x, y in zip(probe, singles[3]))
    e2, m2, out2, _ = c.call(kind, iterations=3, correlated=correlated, seed=S, floor=floor, probes=4)
    assert de.same(m, m2) and de.same(out, out2)
    if which == "base":
        assert np.isfinite(out).all() and out[3] == 0 and out[2] == (c.state > 0).sum()
        assert out[6] == er.grid_sum(np.where(c.state == 2, c.v.astype(np.float64), 0.0))


def test_states(pool):
    """one n < 2 pixel: e_dn = +inf, out[3] = 1, the map +inf there; an all-uncovered frame: +inf with N = 0"""
    W, H = 41, 25
    _, acc, mom = es.state(pool, W * H, es.BASE)
    fa, fm = es.few_pixel(pool)
    at = 13 * W + 17
    acc[:, at], mom[:, at] = fa, fm
    c = Case(W, H, acc, mom)
    for kind in KINDS:
        e, m, out, _ = c.call(kind)
        assert e == np.inf and out[0] == np.inf and out[3] == 1
        assert m.reshape(-1)[at] == np.inf and np.isfinite(np.delete(m.reshape(-1), at)).all()
        assert (m[c.state == 0] == 0).all() and (c.state == 0).any()
        assert np.isfinite(out[4:]).all()
    # a black, noiseless pixel at floor 0 without passes: its estimate is exactly 0 and adds 0 although luma + floor = 0
    black = 3 * W + 5
    acc[:3, black], acc[3, black], acc[7, black], mom[:, black] = 0.0, 2.0, 2.0, 0.0
    acc[:, at], mom[:, at] = acc[:, at + 1], mom[:, at + 1]
    c.r.load_packed_accumulators(acc)
    c.r.load_moments(mom)
    e, m, out, _ = c.call("denoised", iterations=0, floor=0.0)
    assert np.isfinite(e) and np.isfinite(out).all() and m.reshape(-1)[black] == 0
    c.r.load_packed_accumulators(np.zeros_like(acc))
    c.r.load_moments(mom)
    for kind in KINDS:
        e, m, out, _ = c.call(kind)
        assert e == np.inf and out[2] == 0 and not m.any()
    c.r.close()


@pytest.mark.parametrize("W,H", FRAMES)
def test_floors_behave_as_the_raw_metrics_do(W, H, cases):
    """Floors 0, 0.001 and 0.5: bit for bit the restatement; with no passes and independent signs e_dn(floor) is
    relative_error(floor) up to the rounding of y + delta (de.delta_rounding: per pixel |sure - v| <= v (2 r + r^2), summed with
    the metric's own weights, plus 2^-21 for luma of the float32 colour against the float64 L and for v against var_L)."""
    c = cases(W, H, "base")
    ok = c.state == 2
    for floor in (0.0, 0.001, 0.5):
        for kind in KINDS:
            e, m, out, probe = c.call(kind, iterations=3, floor=floor, seed=11)
            wm, wout = c.restated(kind, [probe], floor, 0)
            assert de.same(out, wout) and de.same(m, wm)
            assert np.isfinite(e)
        e, m, out, (yp, Fy, _) = c.call("denoised", iterations=0, correlated=0, floor=floor, seed=11)
        raw = c.r.relative_error(floor)
        r = de.delta_rounding(yp, c.v, EPS)
        d = de.luma64(Fy) + floor
        with np.errstate(divide="ignore", invalid="ignore"):
            slack = np.where(ok & (c.v > 0), c.v.astype(np.float64) * (2 * r + r * r) / (d * d), 0.0)
        tol = slack.sum() / out[2] + raw * raw * 2.0 ** -21
        print(f"{W} x {H} floor {floor}: e_dn {e:.9g} relative_error {raw:.9g}; |e_dn^2 - e^2| {abs(e * e - raw * raw):.3g} <= {tol:.3g}")
        assert abs(e * e - raw * raw) <= tol
        assert (m[ok & (c.v == 0)] == 0).all() and (ok & (c.v == 0)).any()


@pytest.mark.parametrize("kind", KINDS)
def test_nothing_else_moves(kind, cases):
    c = cases(41, 25, "all")
    r = c.r
    r.keep_picture("denoised", iterations=2)

    def snapshot():
        g, gv = r.guided_radiance(return_variance=True)
        f = r.features()
        return [r.packed_accumulators(), r.moments(), r.get_random_buffer(), f["normal"], f["depth"], f["albedo"], f["coverage"],
                r.kept_picture(), g, gv, r.denoised_radiance()]
    before = snapshot()
    kept = r.kept_kind
    for correlated in (0, 1):
        r.denoised_error(kind, correlated=correlated, probes=2, return_map=True, return_probe=True)
    assert r.kept_kind == kept
    for x, y in zip(before, snapshot()):
        assert x.tobytes() == y.tobytes()
    r.keep_picture(None)


def test_refusals(pool):
    from clive2_amd.renderer import Renderer, RendererError
    from clive2_amd._native import ptr
    W, H = 32, 24
    r = Renderer(ds.cornell(W, H))
    r.run_samples(2)
    with pytest.raises(RendererError, match=r"\(-3\)"):          # no features
        r.denoised_error()
    r.render_features(1)
    with pytest.raises(RendererError, match=r"\(-3\)"):          # tracking off
        r.denoised_error()
    r.set_error_tracking(True)
    with pytest.raises(RendererError, match=r"\(-3\)"):          # moments invalid
        r.denoised_error()
    r.reset_accumulators()
    r.run_samples(2)
    assert np.isfinite(r.denoised_error()) and np.isfinite(r.denoised_error("guided"))
    out, m, pr = (C.c_double * 8)(), np.empty(W * H, F), np.empty(9 * W * H, F)
    good = dict(kind=0, iterations=3, sigma=2.0, sigma_depth=0.1, sigma_albedo=0.1, probes=1, epsilon=EPS, correlated=0, seed=0,
                floor=0.001, n_map=m.size, n_probe=pr.size)

    def rc(**kw):
        a = dict(good, **kw)
        return r._L.cl2_denoise_error(r._h, a["kind"], a["iterations"], a["sigma"], a["sigma_depth"], a["sigma_albedo"], a["probes"],
                                      a["epsilon"], a["correlated"], C.c_uint32(a["seed"]), a["floor"], out, ptr(m),
                                      C.c_size_t(a["n_map"]), ptr(pr), C.c_size_t(a["n_probe"]))
    assert rc() == 0
    for bad in (dict(kind=2), dict(kind=-1), dict(probes=0), dict(probes=17), dict(epsilon=0.0), dict(epsilon=float("inf")),
                dict(epsilon=float("nan")), dict(floor=-1.0), dict(floor=float("nan")), dict(iterations=13), dict(iterations=-1),
                dict(sigma=0.0), dict(sigma_depth=float("nan")), dict(sigma_albedo=1e-23), dict(n_map=m.size - 1),
                dict(n_probe=pr.size - 1), dict(correlated=2)):
        assert rc(**bad) == -1, bad
    with pytest.raises(ValueError):
        r.denoised_error("robust")
    best, errs = r.best_iterations("denoised", candidates=range(0, 4), seed=3)
    assert set(errs) == {0, 1, 2, 3} and errs[best] == min(errs.values())
    assert errs[2] == r.denoised_error(iterations=2, seed=3)
    with pytest.raises(ValueError):
        r.render_until(0.1, 8, adaptive=True, metric="denoised")
    r.close()


def test_render_until_on_the_filtered_metric():
    """64 x 48 Cornell box, reproducible light image.  The pass count and e_dn of render_until(metric="denoised") equal those of a
    hand-written loop on a second handle with the same seeds; for the same target metric="picture" needs at least as many
    passes.  The target is the smallest e_dn of the hand loop's first three checks, so that the loop stops at one of them."""
    from clive2_amd.renderer import Renderer, make_seeds
    scene = ds.cornell(64, 48)
    S = make_seeds(64 * 48, seed=77)

    def handle():
        r = Renderer(scene, seeds=S)
        r.set_reproducible(True)
        r.set_error_tracking(True)
        return r
    a = handle()
    a.render_features()
    a.run_samples(2)
    hand = []
    for check in range(3):
        a.run_samples(8)
        hand.append(a.denoised_error("denoised", seed=check))
    a.close()
    target = min(hand)
    stop = hand.index(target)
    b = handle()
    done, e = b.render_until(target, 4096, metric="denoised")
    assert (done, e) == (2 + 8 * (stop + 1), hand[stop]) and b.samples == done
    b.close()
    c = handle()
    done_raw, e_raw = c.render_until(target, 4096, metric="picture")
    c.close()
    print(f"target {target:.4g}: {done} passes on the filtered metric (e_dn {e:.4g}), {done_raw} on the raw one (e {e_raw:.4g})")
    assert done <= done_raw < 4096 and e_raw <= target
    d = handle()
    done_g, e_g = d.render_until(target, 64, metric="guided", filter_params=dict(iterations=3))
    assert 10 <= done_g <= 64 and np.isfinite(e_g)
    d.close()


@pytest.mark.parametrize("guided", [False, True])
def test_cli_renders_until_the_filtered_error(guided, tmp_path, capsys):
    from clive2_amd import render
    out = tmp_path / "d.png"
    args = ["--scene", "empty", "--width", "64", "--height", "48", "--samples", "40", "--target-error", "0.5", "--denoise",
            "--error-of", "denoised", "--out", str(out)] + (["--variance-guided"] if guided else [])
    assert render.main(args) == 0
    assert out.exists() or (tmp_path / "d.png.npy").exists()
    text = capsys.readouterr().out
    assert "e_dn of the denoised picture" in text and "10 samples" in text


def _calibration(scene, kinds=KINDS, renders=24, truth_samples=16384):
    """{(kind, correlated): R} -- R = mean of out[4] / mean over the renders of sum over state 2 of (luma F(y) - luma mu)^2"""
    from clive2_amd.renderer import Renderer, make_seeds
    W, H = scene.pixel_width, scene.pixel_height
    t = Renderer(scene, seeds=make_seeds(W * H, seed=4321))
    t.run_samples(truth_samples)
    mu = de.luma64(t.radiance)
    t.close()
    est = {(k, c): [] for k in kinds for c in (0, 1)}
    true = {k: [] for k in kinds}
    for i in range(renders):
        r = Renderer(scene, seeds=make_seeds(W * H, seed=1000 + i))
        r.set_error_tracking(True)
        r.run_samples(32)
        r.render_features(4)
        state = er.variances(r.packed_accumulators(), r.moments())[0].reshape(H, W)
        for k in kinds:
            for c in (0, 1):
                _, out, (_, Fy, _) = r.denoised_error(k, correlated=c, seed=i, return_totals=True, return_probe=True)
                est[(k, c)].append(out[4])
            true[k].append(float(((de.luma64(Fy) - mu) ** 2)[state == 2].sum()))
        r.close()
    return {kc: float(np.mean(v) / np.mean(true[kc[0]])) for kc, v in est.items()}


def test_estimate_is_calibrated_on_real_renders():
    """In the manner of test_gpu_error.test_estimate_is_calibrated_on_real_renders: the 64 x 48 Cornell box, one render of 16,384
    samples as the truth mu (its own variance is the raw one / 512: negligible beside the filtered error), 24 renders of 32 samples
    with different seeds, features from render_features(4), both filters at their defaults.  R = mean of out[4] / mean of the sum
    over state 2 of (luma F(y) - luma mu)^2, for both perturbation modes.  R of the default mode lies in [0.6, 1.6] -- the bracket
    of the variance calibration; the truth comes from the renderer, not from the new code -- and the default mode is the one whose
    R is nearer 1: there is one default for both filters, so |R - 1| is summed over them (three passes of the fixed filter hardly
    tell the modes apart, 0.006 against 0.008 -- the guided filter does).  Measured on the MI355X, independent / reconstruction-correlated signs: fixed filter 0.994 / 1.008, guided
    filter 0.883 / 1.943; on the glass scene (tests/denoise_scenes.glass, not asserted) 1.043 / 0.576 and 1.197 / 0.438."""
    from clive2_amd import renderer as rmod
    R = _calibration(ds.cornell(64, 48))
    for k in KINDS:
        print(f"calibration, Cornell box, {k}: R independent {R[(k, 0)]:.3f}, reconstruction-correlated {R[(k, 1)]:.3f}")
    dflt = int(bool(rmod.DENOISED_ERROR_CORRELATED))
    for k in KINDS:
        assert 0.6 <= R[(k, dflt)] <= 1.6, (k, R)

    def off(c):
        return sum(abs(R[(k, c)] - 1.0) for k in KINDS)
    assert off(dflt) <= off(1 - dflt), R
