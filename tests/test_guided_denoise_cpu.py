"""The variance-guided denoiser's specification (tests/guided_denoise_reference.py, the numpy statement csrc/denoise_guided.hpp is
checked against on the GPU): properties that follow from it, on synthetic guide buffers, and the binding.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import denoise_reference as dr
import guided_denoise_reference as gr

F = np.float32


def _flat_features(H, W, depth=3.0):
    n = np.zeros((H, W, 3), F)
    n[..., 1] = 1
    return n, np.full((H, W), depth, F), np.full((H, W, 3), 0.5, F), np.ones((H, W), F)


def _noisy(H, W, seed=0):
    return np.random.RandomState(seed).gamma(1.0, 0.3, size=(H, W, 3)).astype(F)


def test_zero_iterations_is_identity():
    c = _noisy(20, 24)
    v = np.random.RandomState(1).gamma(1.0, 0.1, size=(20, 24)).astype(F)
    out, vout = gr.denoise(c, v, *_flat_features(20, 24), iterations=0)
    assert out.dtype == F and out.tobytes() == c.tobytes()
    assert vout.dtype == F and vout.tobytes() == v.tobytes()


@pytest.mark.parametrize("kind", ["zero", "small", "random", "huge"])
def test_constant_image_is_a_fixed_point(kind):
    H, W = 37, 45                                   # not a multiple of any step: taps fall off every edge
    c = np.empty((H, W, 3), F)
    c[...] = np.array([0.25, 0.5, 0.125], F)        # exact binary fractions: sum(w c) / sum(w) returns c to the last bit or so
    n, z, a, cov = _flat_features(H, W)
    z = z + np.linspace(0, 1, W, dtype=F)[None, :]  # guides that vary do not matter for a constant colour
    v = dict(zero=np.zeros((H, W), F), small=np.full((H, W), 1e-6, F),
             random=np.random.RandomState(3).gamma(1.0, 10.0, size=(H, W)).astype(F), huge=np.full((H, W), gr.CAP, F))[kind]
    out, vout = gr.denoise(c, v, n, z, a, cov, iterations=5)
    np.testing.assert_allclose(out, c, rtol=2e-6, atol=0)
    assert np.isfinite(vout).all() and (vout >= 0).all()


def test_it_smooths_where_the_variance_says_noise():
    H, W = 32, 32
    c = _noisy(H, W)
    v = np.full((H, W), 0.09, F)                    # gamma(1, 0.3): variance 0.09 per channel
    out, vout = gr.denoise(c, v, *_flat_features(H, W), iterations=3)
    assert out.std() < 0.5 * c.std()
    assert abs(out.mean() - c.mean()) < 0.05 * c.mean()
    assert (vout < v).all()


def test_uncovered_pixels_pass_through_and_are_not_taps():
    H, W = 24, 24
    c = _noisy(H, W, 1)
    n, z, a, cov = _flat_features(H, W)
    cov[:, :8] = 0                                  # a band of background
    c[:, :8] = 1000.0                               # ... far brighter than the rest: would leak if it were tapped
    v = np.full((H, W), 0.09, F)
    v[:, :8] = 1e12                                 # ... and with a variance that would open every neighbour's filter
    out, vout = gr.denoise(c, v, n, z, a, cov, iterations=4, sigma_luma=1e3)
    assert out[:, :8].tobytes() == c[:, :8].tobytes()
    assert vout[:, :8].tobytes() == v[:, :8].tobytes()
    assert out[:, 8:].max() < 10.0
    # the 3 x 3 of v leaves uncovered pixels out as well: column 8's vbar is that of the covered pixels alone
    vbar = gr.smoothed_variance(v, cov)
    np.testing.assert_allclose(vbar[:, 8:], 0.09, rtol=1e-6)
    assert vout[:, 8:].max() < 0.09


def test_colour_does_not_cross_a_crease():
    """Two regions whose normals are perpendicular: w_n = 0 between them, so every output pixel is a weighted mean of its own
    region's colours only (here: a constant per region), whatever the sigmas and the variance."""
    H, W = 30, 40
    n = np.zeros((H, W, 3), F)
    n[:, :17, 0] = 1                                # left wall faces +x
    n[:, 17:, 1] = 1                                # floor faces +y
    z = np.full((H, W), 2.0, F)
    a = np.full((H, W, 3), 0.7, F)
    cov = np.ones((H, W), F)
    c = np.zeros((H, W, 3), F)
    c[:, :17] = (1.0, 0.0, 0.0)
    c[:, 17:] = (0.0, 0.0, 4.0)
    v = np.full((H, W), 100.0, F)
    out, _ = gr.denoise(c, v, n, z, a, cov, iterations=5, sigma_luma=1e6, sigma_depth=1e6, sigma_albedo=1e6)
    assert np.all(out[:, :17, 2] == 0) and np.all(out[:, :17, 1] == 0)
    assert np.all(out[:, 17:, 0] == 0) and np.all(out[:, 17:, 1] == 0)
    np.testing.assert_allclose(out[:, :17, 0], 1.0, rtol=1e-6)
    np.testing.assert_allclose(out[:, 17:, 2], 4.0, rtol=1e-6)


def test_weights_follow_the_formula_for_one_tap():
    """A 1 x 2 frame at step 1: each output is the two-tap mean with the weights of the specification, written out by hand,
    and v' = sum w^2 v / (sum w)^2."""
    c = np.array([[[1.0, 2.0, 3.0], [0.5, 0.25, 4.0]]], F)
    v = np.array([[0.04, 0.25]], F)
    n = np.array([[[0.0, 1.0, 0.0], [0.0, 0.8, 0.6]]], F)
    z = np.array([[2.0, 2.5]], F)
    a = np.array([[[0.5, 0.5, 0.5], [0.4, 0.5, 0.6]]], F)
    cov = np.ones((1, 2), F)
    sl, sd, sa = 3.0, 0.1, 0.1
    out, vout = gr.denoise(c, v, n, z, a, cov, iterations=1, sigma_luma=sl, sigma_depth=sd, sigma_albedo=sa)

    def lum(x):
        return x[0] * 0.0722 + x[1] * 0.7152 + x[2] * 0.2126

    for p, q in ((0, 1), (1, 0)):
        vbar = (float(v[0, p]) / 4 + float(v[0, q]) / 8) / (1 / 4 + 1 / 8)        # g(0) g(0) = 1/4, g(0) g(+-1) = 1/8
        den_l = sl * np.sqrt(vbar) + 1e-8
        wn = max(0.0, float(n[0, p] @ n[0, q])) ** 32
        wz = np.exp(-abs(z[0, p] - z[0, q]) / (sd * z[0, p]))
        wa = np.exp(-np.sum((a[0, p] - a[0, q]) ** 2) / sa ** 2)
        wl = np.exp(-abs(lum(c[0, p]) - lum(c[0, q])) / den_l)
        wself = (3 / 8) ** 2
        wq = (3 / 8) * (1 / 4) * wn * wz * wa * wl
        want = (wself * c[0, p] + wq * c[0, q]) / (wself + wq)
        np.testing.assert_allclose(out[0, p], want, rtol=1e-5)
        want_v = (wself ** 2 * v[0, p] + wq ** 2 * v[0, q]) / (wself + wq) ** 2
        np.testing.assert_allclose(vout[0, p], want_v, rtol=1e-5)


def test_zero_variance_returns_the_input():
    """Consistency: where the estimate says "converged" the filter closes.  v = 0 makes den_l = 1e-8; a tap at luma distance d
    weighs at most exp(-d / 1e-8) and moves the pixel by at most d exp(-d / 1e-8) <= 1e-8 / e = 3.7e-9 (and by nothing at all once
    d exceeds 1e-6: the weight underflows).  What remains is the float32 rounding of (w c) / w with the centre tap alone: up to
    one ulp(c) per pass.  The picture is scaled like a rendered radiance (values below 0.25, ulp <= 1.5e-8), so five passes stay
    below 1e-7 absolute; a picture of values above 1 would show 2^-23 = 1.19e-7 from that rounding alone."""
    H, W = 40, 52
    c = (_noisy(H, W, 5) * F(0.05)).astype(F)
    assert c.max() < 0.25
    out, vout = gr.denoise(c, np.zeros((H, W), F), *_flat_features(H, W), iterations=5)
    worst = float(np.abs(out - c).max())
    print(f"v = 0: largest change {worst:.3g}")
    assert worst <= 1e-7
    assert not vout.any()


def test_variance_propagation_of_one_pass():
    """Flat guides, a constant v and every edge-stop open: an interior pixel is the plain B3-spline mean of 25 independent taps,
    v' = v (sum h^2)^2 = v (70 / 256)^2."""
    H, W = 16, 18
    c = np.full((H, W, 3), 0.5, F)
    for v0 in (0.25, 3e-5, 7.0):
        out, vout = gr.denoise(c, np.full((H, W), v0, F), *_flat_features(H, W), iterations=1, sigma_luma=1e6, sigma_depth=1e6,
                               sigma_albedo=1e6)
        np.testing.assert_allclose(vout[2:-2, 2:-2], F(v0) * 0.07476806640625, rtol=1e-6)
        assert (vout[0, 0] > vout[2, 2]) and np.isfinite(vout).all()          # fewer taps at the corner


@pytest.mark.parametrize("fy,fx,region", [(40, 32, 0.004), (48, 100, 0.008)])
def test_a_firefly_is_averaged_away(fy, fx, region):
    """A flat 128 x 96 picture of two regions (0.004 and 0.008) under gamma(1) noise, 16 samples per pixel; one sample of one pixel
    is 1e4 times the pixel's value, so the pixel's mean is 625 times too bright.  v = the sample variance of the mean.  The
    firefly's own variance is huge: it accepts every neighbour and ends within a factor 2 of its region's value, and its four
    neighbours, which reject it, within 25 %.  Five passes, the widest setting the filter was designed with: each pass spreads
    what is left of the firefly over a footprint twice as wide.  Measured on this statement: 1.30 x the region's value after 5
    passes (neighbours at most 1.07 x), 2.2 x after 4 (1.21 x), 6.8 x after 3 (2.3 x); the fixed filter leaves 6.4 x (0.0256) at
    its defaults."""
    H, W, n = 96, 128, 16
    rs = np.random.RandomState(11)
    level = np.where(np.arange(W) < W // 2, 0.004, 0.008)[None, :, None] * np.ones((H, W, 1))
    s = level[None] * rs.gamma(1.0, 1.0, size=(n, H, W, 1)) * np.ones((1, 1, 1, 3))     # grey samples: luma = the value
    assert level[fy, fx, 0] == region
    s[3, fy, fx] = 1e4 * region
    c = s.mean(0).astype(F)
    lum = gr.luma(s.astype(F)).astype(np.float64)
    v = (lum.var(0, ddof=1) / n).astype(F)
    out, _ = gr.denoise(c, v, *_flat_features(H, W), iterations=5, sigma_luma=4.0)
    fixed = dr.denoise(c, *_flat_features(H, W), **dr.DEFAULTS)
    got = float(out[fy, fx, 1])
    nb = [float(out[fy + dy, fx + dx, 1]) for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1))]
    print(f"firefly: input {float(c[fy, fx, 1]):.4g}, guided {got:.4g} (region {region}), fixed filter {float(fixed[fy, fx, 1]):.4g}; "
          f"neighbours {[f'{x:.4g}' for x in nb]}")
    assert region / 2 <= got <= region * 2
    assert all(abs(x - region) <= 0.25 * region for x in nb)
    assert float(fixed[fy, fx, 1]) > 2 * region                       # what the fixed filter leaves in place


@pytest.mark.parametrize("block", [1, 4])
def test_the_cap_keeps_everything_finite(block):
    """A pixel (or a block of them) with fewer than two samples carries v = 2^100: every product and sum stays finite."""
    H, W = 40, 44
    c = _noisy(H, W, 7)
    v = np.full((H, W), 0.01, F)
    v[17:17 + block, 21:21 + block] = gr.CAP
    c[17:17 + block, 21:21 + block] = 50.0
    for it in (1, 5):
        out, vout = gr.denoise(c, v, *_flat_features(H, W), iterations=it)
        assert np.isfinite(out).all() and np.isfinite(vout).all()
        assert (vout >= 0).all()
    v[...] = gr.CAP
    out, vout = gr.denoise(c, v, *_flat_features(H, W), iterations=5)
    assert np.isfinite(out).all() and np.isfinite(vout).all()


def test_input_variance_states():
    """v of the input kernel: the luma variance of the error estimate; 2^100 with n < 2 and for values beyond the cap; 0 uncovered."""
    import error_reference as er
    import error_states as es
    pl = es.pool()
    cls, acc, mom = es.state(pl, 64 * 30, es.ALL)
    v = gr.input_variance(acc, mom)
    state, var, _ = er.variances(acc, mom)
    assert v.dtype == F and np.isfinite(v).all() and (v >= 0).all() and (v <= gr.CAP).all()
    assert not v[state == 0].any() and (v[state == 1] == gr.CAP).all()
    ok = (state == 2) & (var[:, 3] < 2.0 ** 100)
    assert v[ok].tobytes() == var[ok, 3].astype(F).tobytes()
    big = (state == 2) & ~(var[:, 3] < 2.0 ** 100)
    assert big.any() and (v[big] == gr.CAP).all()
    se = er.standard_error(acc, mom)[:, 3].astype(np.float64)
    fin = ok & np.isfinite(se) & (se > 1e-18)
    np.testing.assert_allclose(np.sqrt(v[fin].astype(np.float64)), se[fin], rtol=3e-7)


# ---- the binding ----
@pytest.fixture(scope="module")
def native_lib():
    from clive2_amd import _native
    _native.build()
    return _native.lib()


def test_library_exports_the_guided_filter(native_lib):
    from clive2_amd import _native
    assert hasattr(native_lib, "cl2_denoise_guided") and "cl2_denoise_guided" in _native.EXPORTS
    assert native_lib.cl2_abi_version() == 6


def test_guided_filter_refuses_a_null_handle(native_lib):
    out, var = np.zeros(3 * 64, F), np.zeros(64, F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert native_lib.cl2_denoise_guided(None, 1, 4.0, 0.1, 0.1, p(out), out.size, p(var), var.size) == -1
    assert native_lib.cl2_denoise_guided(None, 1, 4.0, 0.1, 0.1, p(out), out.size, None, 0) == -1


def test_python_defaults_and_reference_defaults_agree():
    from clive2_amd.renderer import Renderer
    assert Renderer.GUIDED_DEFAULTS == gr.DEFAULTS
    assert Renderer.DENOISE_DEFAULTS == dr.DEFAULTS               # the fixed filter's defaults are untouched


@pytest.mark.parametrize("mod", ["render", "movie"])
def test_cli_refuses_variance_guided_without_denoise(mod):
    import importlib
    m = importlib.import_module(f"clive2_amd.{mod}")
    with pytest.raises(SystemExit):
        m.main(["--variance-guided"])
