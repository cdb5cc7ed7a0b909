"""The split of the luma variance into its camera and its light part and the mixed perturbation built on it (csrc/error_split.hpp,
noise model 2 of csrc/denoise_error.hpp) without a device: the numpy restatement (tests/error_split_reference.py)
against the two pure modes it must degenerate to, E z^2 = 1, the calibration of SURE under the split model's own noise, the
arithmetic of the share, and the plumbing of the new entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_error_reference as de
import error_reference as er
import error_split_reference as sp
from test_denoise_error_cpu import _scene, _unit_field

F = np.float32
D = np.float64
EPS = 1 / 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the bracket tests/test_denoise_error_cpu.py::test_unbiased_under_its_own_model holds each pure mode to under its own noise
BRACKET = (0.9, 1.1)


# ---------------------------------------------------------------- the two pure modes as degenerate shares
@pytest.mark.parametrize("W,H", [(7, 5), (41, 25)])
def test_degenerate_shares_are_the_pure_modes(W, H):
    """rho = 1 everywhere: y' of the independent mode with the signs of t ^ 0xA5A5A5A5 (cs = 0: 0 zK + b').  rho = 0 everywhere:
    y' of the correlated mode of t (cl = 0: zK + (+-0)).  Bit for bit, borders included.  A -0 in zK would turn into +0 under
    `+ (+0)` and could show in y' where y_c = -0: zK is a float32 sum that starts from +0 and a float64 quotient of it, and an
    exact cancellation rounds to +0, so none occurs -- the comparison below would show one."""
    rs = np.random.RandomState(W)
    y = rs.gamma(1.0, 0.5, (H, W, 3)).astype(F)
    y[0, 0] = (-0.0, 0.0, -0.0)
    a = (0.1 * rs.gamma(1.0, 0.5, (H, W, 3))).astype(F)
    for t in (0, 5, 0x5A5A5A5A, 0xFFFFFFFF):
        one = sp.perturb_split(y, a, np.ones((H, W), F), t, EPS)
        assert de.same(one, de.perturb(y, a, de.field(W, H, t ^ sp.SIGN_XOR, 0), EPS))
        zK = de.field(W, H, t, 1)
        assert not (np.signbit(zK) & (zK == 0)).any()
        zero = sp.perturb_split(y, a, np.zeros((H, W), F), t, EPS)
        assert de.same(zero, de.perturb(y, a, zK, EPS))
        assert de.same(sp.field_split(W, H, t, np.zeros((H, W), F)), zK)


def test_unit_variance():
    """E z^2 = 1 at a corner, an edge and an interior pixel for rho in {0, 0.3, 1}, over 4,096 seeds.

    Bound.  zK = sum k_i b_i / sqrt(sum k^2) over the in-frame sources, so zK^2 - 1 = sum_{i != j} k_i k_j b_i b_j / sum k^2 has
    variance V_K = 2 (1 - sum k^4 / (sum k^2)^2) (test_denoise_error_cpu.test_pass_through).  With cs^2 + cl^2 = 1,
    z^2 - 1 = cs^2 (zK^2 - 1) + 2 cs cl zK b'; b' is independent of zK with mean 0, so the two terms are uncorrelated and
    Var z^2 = cs^4 V_K + 4 cs^2 cl^2.  The mean of 4,096 draws is held to 4 standard deviations, plus 2^-20 for the float32
    rounding of cs, cl and z (cs^2 + cl^2 = 1 to 2^-23 each).  rho = 1 has variance 0: z = +-1 exactly."""
    W, H, N = 41, 25, 4096
    kx, ky = de.kernel()
    for rho in (0.0, 0.3, 1.0):
        r = np.full((H, W), rho, F)
        z = np.stack([sp.field_split(W, H, t, r) for t in range(N)]).astype(D)
        cl2 = float(F(rho))
        cs2 = 1.0 - cl2
        for (py, px), ii, jj in (((0, 0), (-1, 0), (-1, 0)), ((0, 20), (-1, 0, 1), (-1, 0)), ((12, 20), (-1, 0, 1), (-1, 0, 1))):
            k = np.array([D(ky[j + 1]) * D(kx[i + 1]) for j in jj for i in ii])
            VK = 2 * (1 - (k ** 4).sum() / (k ** 2).sum() ** 2)
            sd = np.sqrt((cs2 * cs2 * VK + 4 * cs2 * cl2) / N)
            mean = (z[:, py, px] ** 2).mean()
            print(f"rho {rho} at ({px}, {py}): mean z^2 - 1 = {mean - 1:+.4f}, 4 sigma {4 * sd:.4f}")
            assert abs(mean - 1) <= 4 * sd + 2.0 ** -20
    assert (np.abs(z) == 1).all()                         # the last one: rho = 1


# ---------------------------------------------------------------- calibration under its own model
def _rho_pattern(W, H):
    """not constant: the halves at 0.2 / 0.8 plus a vertical ramp of -0.1 .. +0.1"""
    yy, xx = np.mgrid[0:H, 0:W].astype(D)
    return (np.where(xx < W // 2, 0.2, 0.8) + 0.2 * (yy / (H - 1) - 0.5)).astype(F)


def _ratio(model, iterations, trials=12):
    """test_denoise_error_cpu._ratio with the split model's noise D_a (cs o (K * g) + cl o h): mean estimate / mean true squared
    luma error of the filtered picture, and the scatter of the per-trial estimates / mean truth.  model 0, 1: the pure probes,
    2: the split probe."""
    f, mu, sigma, d = _scene()
    H, W = sigma.shape
    rho = _rho_pattern(W, H)
    cs, cl = sp.coefficients(rho)
    state = np.full((H, W), 2)
    v = (sigma * sigma).astype(F)
    a = (np.sqrt(v.astype(D)).astype(F)[..., None] * d).astype(F)
    est, true = [], []
    for t in range(trials):
        rs = np.random.RandomState(9000 + t)
        g = _unit_field(rs, W, H, 1)
        h = rs.standard_normal((H, W))
        eta = sigma.astype(D) * (cs.astype(D) * g + cl.astype(D) * h)
        y = (mu.astype(D) + eta[..., None] * d.astype(D)).astype(F)
        if model == 2:
            _, out, pr = sp.estimate_split(y, state, v, a, None, f, rho, kind=0, probes=1, eps=EPS, seed=100 + t, iterations=iterations)
        else:
            _, out, pr = de.estimate(y, state, v, a, None, f, kind=0, probes=1, eps=EPS, correlated=model, seed=100 + t,
                                     iterations=iterations)
        est.append(out[4])
        true.append(float(((de.luma64(pr["Fy"]) - de.luma64(mu)) ** 2).sum()))
    return float(np.mean(est) / np.mean(true)), float(np.std(est, ddof=1) / np.mean(true))


def test_unbiased_under_its_own_model():
    """64 x 48, 12 trials with fixed seeds, 3 passes of the fixed filter, one probe, eps = 1/16, noise with the covariance the
    split probe assumes (rho: halves at 0.2 / 0.8 plus a ramp): the mean estimate / mean true squared luma error lies in the
    bracket the pure modes are held to under their own noise."""
    assert 0.05 < _rho_pattern(64, 48).min() < 0.35 and 0.65 < _rho_pattern(64, 48).max() < 0.95
    R, scatter = _ratio(2, 3)
    print(f"split noise, split probe, 3 passes: ratio {R:.3f}, per-trial scatter {scatter:.3f}")
    assert BRACKET[0] <= R <= BRACKET[1]


@pytest.mark.parametrize("model", [0, 1])
def test_pure_modes_miss_the_split_noise(model):
    """the same noise, a pure probe, one pass: the ratio lies outside the bracket (the split probe's, printed beside it, does not
    enter the assertion: at one pass its per-trial scatter is a quarter of the truth)"""
    R, scatter = _ratio(model, 1)
    R2, scatter2 = _ratio(2, 1)
    print(f"split noise, {'correlated' if model else 'independent'} probe, 1 pass: ratio {R:.3f}, per-trial scatter {scatter:.3f}; "
          f"split probe {R2:.3f}, scatter {scatter2:.3f}")
    assert not (BRACKET[0] <= R <= BRACKET[1])


# ---------------------------------------------------------------- the share
def _parts(rs, P, n, frac, mu=1.5, total_sd=0.2):
    """n addends of P pixels whose light part carries `frac` (P,) of the variance: each part is its weight times mu plus its own
    noise, so S_c and S_l are the parts' residual sums about L w"""
    parts = []
    sl, sc = total_sd * np.sqrt(frac), total_sd * np.sqrt(1 - frac)
    for _ in range(n):
        wc, wl = np.full(P, 0.75, F), np.full(P, 0.25, F)
        yc = 0.75 * mu + sc * rs.standard_normal(P)
        yl = 0.25 * mu + sl * rs.standard_normal(P)
        t = np.repeat(yc[:, None], 3, 1).astype(F)               # grey: luma(t) = yc up to rounding
        l = np.concatenate([np.repeat(yl[:, None], 3, 1), wl[:, None]], 1).astype(F)
        parts.append((t, wc, l))
    return parts


def _state_of(parts):
    """accumulators, moments and split rows of a sequence of parts, as the kernels add them"""
    P = len(parts[0][1])
    acc, mom = np.zeros((8, P), F), np.zeros((8, P), F)
    for t, wc, l in parts:
        fin = np.concatenate([t, np.ones((P, 1), F)], 1)
        x, w = er.addends(fin, l, wc)
        acc[:3] = (acc[:3] + x.T).astype(F)
        acc[3] = (acc[3] + w).astype(F)
        acc[7] = (acc[7] + F(1)).astype(F)
        er.add_moments(mom, x, w)
    return acc, mom, sp.split_moments_of(parts)


def test_share_recovers_a_known_fraction():
    """n = 4096 Gaussian addends per pixel, light fractions 0, 0.1, 0.5, 0.9, 1 of the variance.

    Tolerance.  S_c / sigma_c^2 and S_l / sigma_l^2 are chi-square with about n degrees of freedom (L is estimated from the same
    addends: a 1/n effect), relative standard deviation sqrt(2 / n) each and independent, so log(S_l / S_c) has standard deviation
    2 / sqrt(n) and rho = 1 / (1 + S_c / S_l) has f (1 - f) 2 / sqrt(n) by the delta method: held to 5 of those.  The estimate of L:
    L - mu has standard deviation sigma / sqrt(n) (sigma^2 the total variance) and adds n w^2 (L - mu)^2 to the S of the part with
    weight w, at most wc^2 = 0.5625 of sigma^2 chi-square_1 -- against S_c + S_l = n sigma^2 a shift of rho of 0.5625 chi-square_1 / n,
    at the same 5 standard deviations 0.5625 * 25 / n.  And 2^-12 for the float32 sums (4096 adds of relative 2^-24 each)."""
    n, P = 4096, 256
    rs = np.random.RandomState(11)
    for f in (0.0, 0.1, 0.5, 0.9, 1.0):
        acc, mom, smom = _state_of(_parts(rs, P, n, np.full(P, f)))
        rho, out = sp.light_share(acc, mom, smom)
        tol = 5 * f * (1 - f) * 2 / np.sqrt(n) + 0.5625 * 25 / n + 2.0 ** -12
        print(f"fraction {f}: rho in [{rho.min():.4f}, {rho.max():.4f}], frame share {out[0]:.4f}, tolerance {tol:.4f}")
        assert np.abs(rho.astype(D) - f).max() <= tol
        assert abs(out[0] - f) <= tol and out[3] == P


def test_share_falls_to_one():
    """S_c = S_l = 0, NaN / inf rows and n < 2 give rho = 1; negative remainders are clamped; the totals leave out what has no
    finite var_L"""
    rs = np.random.RandomState(3)
    acc, mom, smom = _state_of(_parts(rs, 16, 8, np.full(16, 0.5)))
    smom[:, 0] = 0                                   # both parts noiseless
    smom[:, 1] = np.nan
    smom[0, 2] = np.inf                              # inf - ... = inf or NaN
    smom[3, 3] = np.inf
    smom[:, 4] = (-1, 0, 0, -1, 0, 0)                # both negative: clamped to 0, 0
    smom[:, 5] = (1, 0, 0, -1, 0, 0)                 # only the light part clamped: rho = 0
    smom[:, 6] = (-1, 0, 0, 1, 0, 0)                 # only the camera part clamped: rho = 1 by the formula
    acc[7, 7] = 1                                    # n < 2
    acc[7, 8] = 0
    acc[3, 9] = 0                                    # uncovered
    mom[7, 10] = np.inf                              # var_L = +inf: rho from the rows, left out of the totals
    rho, state, vL = sp.rho64(acc, mom, smom)
    assert rho[[0, 1, 2, 3, 4, 6, 7, 8, 9]].tolist() == [1.0] * 9 and rho[5] == 0.0
    assert 0 < rho[10] < 1 and np.isinf(vL[10])
    assert ((rho >= 0) & (rho <= 1)).all()
    m, out = sp.light_share(acc, mom, smom)
    assert m.dtype == F and out[3] == 16 - 4 and np.isfinite(out).all() and 0 <= out[0] <= 1
    # nothing to sum: 0, not NaN
    acc[7] = 1
    assert sp.light_share(acc, mom, smom)[1].tolist() == [0.0, 0.0, 0.0, 0.0]


def test_split_rows_of_scrubbed_parts():
    """the scrub is per part and per channel, before the luma: a NaN or inf channel counts as 0 in its own part only"""
    t = np.array([[np.nan, 1.0, 2.0], [np.inf, -np.inf, 3.0], [-0.0, 0.0, 0.0]], F)
    l = np.array([[1.0, np.nan, 0.0, 0.5], [0.0, 0.0, 0.0, np.inf], [1.0, 1.0, 1.0, -0.0]], F)
    wc = np.array([1.0, 2.0, np.nan], F)
    smom = sp.split_moments_of([(t, wc, l)])
    yc = np.array([(F(0) * er.LUMA[0] + F(1) * er.LUMA[1]) + F(2) * er.LUMA[2], (F(0) + F(0)) + F(3) * er.LUMA[2], 0.0], F)
    assert smom[0].tolist() == (yc * yc).tolist()
    assert np.isnan(smom[1, 2]) and np.isnan(smom[2, 2]) and smom[5, 1] == np.inf and np.isnan(smom[4, 1])
    assert smom[3, 0] == F(er.LUMA[0]) * F(er.LUMA[0])


# ---------------------------------------------------------------- plumbing
def _names(header):
    with open(os.path.join(ROOT, "include", header)) as fh:
        return sorted(set(re.findall(r"\b(cl2_[a-z_0-9]+)\s*\(", fh.read())))


NEW_CALLS = ("cl2_ext_features", "cl2_set_split_tracking", "cl2_get_split_tracking", "cl2_read_split_moments_packed",
             "cl2_write_split_moments_packed", "cl2_light_share", "cl2_denoise_error_model", "cl2_denoise_select_model",
             "cl2_keep_selected_picture_model")


def test_plumbing(capsys, tmp_path):
    from clive2_amd import _native, render, movie
    from clive2_amd.renderer import Renderer
    assert _names("clive2_amd_ext.h") == sorted(_native.EXT_EXPORTS)
    assert set(NEW_CALLS) <= set(_native.EXT_EXPORTS) and not set(NEW_CALLS) & set(_native.EXPORTS)
    assert len(_native.EXPORTS) == 108
    raw = C.CDLL(_native.LIB_PATH)
    for name in NEW_CALLS:
        assert hasattr(raw, name), name
    L = _native.lib()
    assert L.cl2_ext_features() & 1 and L.cl2_ext_version() == 1 and L.cl2_abi_version() == 6
    # NULL handles
    buf = np.zeros(64, F)
    out4, out8 = (C.c_double * 4)(), (C.c_double * 8)()
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.cl2_set_split_tracking(None, 1) == -1 and L.cl2_get_split_tracking(None) == -1
    assert L.cl2_read_split_moments_packed(None, p, 64) == -1 and L.cl2_write_split_moments_packed(None, p, 64) == -1
    assert L.cl2_light_share(None, None, 0, out4) == -1
    assert L.cl2_denoise_error_model(None, 0, 3, 2.0, 0.1, 0.1, 1, EPS, 2, 0, 0.001, out8, None, 0, None, 0) == -1
    assert L.cl2_denoise_select_model(None, 3, 2.0, 0.1, 0.1, 1, EPS, 2, 0, 2, 0.001, None, 0, None, 0, out8, None, 0, None, 0) == -1
    assert L.cl2_keep_selected_picture_model(None, 3, 2.0, 0.1, 0.1, 1, EPS, 2, 0, 2) == -1
    # the ext header is still plain C
    src = tmp_path / "ext.c"
    src.write_text('#include "clive2_amd_ext.h"\nint main(void) { return cl2_ext_features() + cl2_light_share(0, 0, 0, 0); }\n')
    res = subprocess.run(["gcc", "-Wall", "-Werror", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert Renderer.NOISE_MODELS == {"independent": 0, "correlated": 1, "split": 2}
    # refused before any renderer exists
    base = ["--scene", "empty", "--width", "32", "--height", "24", "--samples", "8"]
    for main in (render.main, movie.main):
        for extra in (["--noise-model", "split"], ["--noise-model", "split", "--denoise"],
                      ["--noise-model", "correlated", "--select-scale"],
                      ["--noise-model", "independent", "--target-error", "0.1", "--error-of", "denoised"],
                      ["--noise-model", "split", "--denoise", "--select-scale", "--target-error", "0.1", "--adaptive"]):
            with pytest.raises(SystemExit) as ex:
                main(base + extra)
            assert ex.value.code == 2, extra
        with pytest.raises(SystemExit):
            main(base + ["--noise-model", "mixed"])
    for extra in (["--light-share-out", "x.npy"], ["--light-share-out", "x.npy", "--denoise", "--select-scale"],
                  ["--light-share-out", "x.npy", "--denoise", "--select-scale", "--noise-model", "correlated"]):
        with pytest.raises(SystemExit) as ex:
            render.main(base + extra)
        assert ex.value.code == 2, extra
    capsys.readouterr()


def test_noise_argument_without_a_device():
    """noise= goes through the *_model entry points with the model's number where `correlated` stood; noise=None keeps the old
    entry points; both together are a ValueError"""
    from clive2_amd.renderer import Renderer

    class Lib:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def call(h, *a):
                self.calls.append((name, a))
                return 0
            return call

    class Fake(Renderer):
        def __init__(self):
            self._L, self._h, self.pixel_width, self.pixel_height = Lib(), None, 6, 4

        def __del__(self):
            pass
    r = Fake()
    r.denoised_error()
    r.denoised_error(noise="split", seed=7)
    r.denoised_error("guided", noise="correlated")
    r.denoised_error(correlated=True)
    names = [c[0] for c in r._L.calls]
    assert names == ["cl2_denoise_error", "cl2_denoise_error_model", "cl2_denoise_error_model", "cl2_denoise_error"]
    assert [c[1][7] for c in r._L.calls] == [0, 2, 1, 1] and r._L.calls[1][1][8].value == 7
    r._L.calls.clear()
    r.selected_radiance()
    r.selected_radiance(noise="split")
    r.keep_selected_picture()
    r.keep_selected_picture(noise="independent", iterations=2)
    assert [c[0] for c in r._L.calls] == ["cl2_denoise_select", "cl2_denoise_select_model", "cl2_keep_selected_picture",
                                          "cl2_keep_selected_picture_model"]
    assert [c[1][6] for c in r._L.calls] == [0, 2, 0, 0] and r._L.calls[3][1][0] == 2
    for call in (lambda: r.denoised_error(noise="split", correlated=False), lambda: r.selected_radiance(noise="split", correlated=True),
                 lambda: r.keep_selected_picture(noise="correlated", correlated=True), lambda: r.denoised_error(noise="mixed"),
                 lambda: r.best_iterations(candidates=(1,), noise="split", correlated=True)):
        with pytest.raises(ValueError):
            call()
    best, errs = r.best_iterations(candidates=(1, 2), noise="split")
    assert sorted(errs) == [1, 2] and r._L.calls[-1][0] == "cl2_denoise_error_model"
