"""The numpy statement of the error estimate of the filtered picture (tests/denoise_error_reference.py, csrc/denoise_error.hpp) on
its own, without a device: what a linear filter must give, the pass-through, that the estimate is unbiased under its own noise
model and badly off under the other one, the signs and the reconstruction kernel, and the plumbing."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_error_reference as de
import denoise_reference as dr
import error_reference as er
import error_states as es
import feature_states as fs

F = np.float32
D = np.float64
EPS = 1 / 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pool():
    return es.pool()


def _ordinary(pool, W, H):
    """ordinary states (2 .. 4096 addends of gamma colours), those whose s_p is at least 2^-8 of the luma"""
    _, acc, mom = es.state(pool, 2 * W * H, (es.ORDINARY,))
    y, state, v, a, w = de.inputs(acc, mom, 2 * W, H)
    keep = np.flatnonzero((np.sqrt(v.astype(D)) >= 2.0 ** -8 * de.luma64(y)).reshape(-1))[:W * H]
    assert keep.size == W * H
    acc, mom = np.ascontiguousarray(acc[:, keep]), np.ascontiguousarray(mom[:, keep])
    y, state, v, a, w = de.inputs(acc, mom, W, H)
    assert (state == 2).all() and (np.sqrt(v.astype(D)) >= 2.0 ** -8 * de.luma64(y)).all()
    return acc, mom, y, state, v, a, w


def test_linear_filter(pool):
    """sigma_color so large that the colour weight is 1 to float32: F is linear in the colours, with weights from the features
    alone.  One pass, one probe, independent signs, and the perturbed pixels on a 3-lattice, so that no 5 x 5 window holds two of
    them: div_p = u_p g_p / eps^2 then is v_p w_pp / sum w, the centre tap's share (1 where the pixel passes through).

    Tolerance.  With the float64 companion of the filter g_p = (w_pp / sum w) u_p exactly, and u_p^2 / eps^2 misses v_p by the
    rounding of y + delta alone, at most v (2 r + r^2) (de.delta_rounding).  The float32 filter adds its own rounding to both
    pictures of g: the yardstick Y is the largest deviation of the float32 restatement's luma from its companion's on the
    unperturbed picture, allowed K = 8 times (feature_states.check) on each of the two: |u_p| 2 K Y / eps^2."""
    W, H = 41, 25
    _, _, y, state, v, a, w = _ordinary(pool, W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    lattice = (yy % 3 == 1) & (xx % 3 == 1)
    a = np.where(lattice[..., None], a, F(0)).astype(F)
    _, n, z, al, cov = fs.features(W, H)
    f = dict(normal=n, depth=z, albedo=al, coverage=cov)
    sig = dict(iterations=1, sigma=1e18, sigma_depth=0.1, sigma_albedo=0.1)
    _, _, pr = de.estimate(y, state, v, a, w, f, kind=0, probes=1, eps=EPS, correlated=0, seed=5, **sig)
    u = de.luma64(pr["yp"]) - de.luma64(y)
    g = de.luma64(pr["Fyp"]) - de.luma64(pr["Fy"])
    div = u * g / (EPS * EPS)
    assert (u[~lattice] == 0).all() and (u[lattice] != 0).all()
    # the centre tap's share, from the float64 companion
    F64, sw = dr.atrous_pass(y, n, z, al, cov, 0, 1e18, 0.1, 0.1, dtype=D, return_sw=True)
    n64 = n.astype(D)
    wn = np.maximum(0.0, dr._dot(n64, n64))
    for _ in range(5):
        wn = wn * wn
    wpp = (D(dr.H5[2]) * D(dr.H5[2])) * wn
    passes = (cov == 0) | ~(sw > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(passes, 1.0, wpp / sw)
    assert passes[lattice].any() and (~passes[lattice]).sum() > 20 and (share[lattice & ~passes] < 0.5).sum() > 20
    want = v.astype(D) * share
    Y = np.abs(de.luma64(pr["Fy"]) - er._luma64(F64[..., 0], F64[..., 1], F64[..., 2])).max()
    r = de.delta_rounding(pr["yp"], v, EPS)
    tol = want * (2 * r + r * r) + np.abs(u) * 2 * fs.K * Y / (EPS * EPS)
    err = np.abs(div - want)
    print(f"linear filter: worst |div - v share| / tolerance {(err[lattice] / tol[lattice]).max():.3f}; yardstick Y {Y:.3g}; "
          f"worst relative error {(err[lattice] / want[lattice]).max():.3g}")
    assert (err[lattice] <= tol[lattice]).all()
    assert np.median(tol[lattice] / want[lattice]) < 0.05      # the tolerance itself is tight: s_p is 2^-8 .. 1 of the luma
    assert (div[~lattice] == 0).all()


def test_pass_through(pool):
    """No passes, independent signs: sure_p = u_p^2 / eps^2 (+ 0 - v + 2 v), so out[4] is the sum of v_p and e_dn is
    error_reference.relative_error, to the rounding of y + delta (|sure - v| <= v (2 r + r^2) per pixel, de.delta_rounding; 2^-21
    more for luma of the float32 colour against the float64 L and v against var_L).  Reconstruction-correlated signs: z_p^2 has
    mean 1 over 64 seeds at a corner, an edge and an interior pixel -- E z^2 = 1 exactly by the normalisation, and the mean of 64
    draws of z^2 = 1 + sum_{i != j} k_i k_j b_i b_j / sum k^2 has variance 2 (1 - sum k^4 / (sum k^2)^2) / 64: 4 sigma."""
    W, H = 41, 25
    acc, mom, y, state, v, a, w = _ordinary(pool, W, H)
    for floor in (0.0, 0.001, 0.5):
        m, out, pr = de.estimate(y, state, v, a, w, None, kind=0, iterations=0, probes=1, eps=EPS, correlated=0, seed=2, floor=floor)
        r = de.delta_rounding(pr["yp"], v, EPS)
        slack = v.astype(D) * (2 * r + r * r)
        total_v = er.grid_sum(v.astype(D))
        assert out[6] == total_v and out[5] == 0
        assert abs(out[4] - total_v) <= slack.sum()
        assert slack.sum() < 1e-2 * total_v
        e = er.relative_error(acc, mom, floor)
        d = de.luma64(y) + floor
        tol = (slack / (d * d)).sum() / out[2] + e * e * 2.0 ** -21
        print(f"pass-through floor {floor}: e_dn {out[0]:.9g} e {e:.9g}, |e_dn^2 - e^2| {abs(out[0] ** 2 - e * e):.3g} <= {tol:.3g}")
        assert abs(out[0] ** 2 - e * e) <= tol
    kx, ky = de.kernel()
    z = np.stack([de.field(W, H, t, 1) for t in range(64)]).astype(D)
    for (py, px), ii, jj in (((0, 0), (-1, 0), (-1, 0)), ((0, 20), (-1, 0, 1), (-1, 0)), ((12, 20), (-1, 0, 1), (-1, 0, 1)),
                             ((H - 1, W - 1), (0, 1), (0, 1))):
        k = np.array([D(ky[j + 1]) * D(kx[i + 1]) for j in jj for i in ii])       # sources (x - i, y - j) inside the frame
        sd = np.sqrt(2 * (1 - (k ** 4).sum() / (k ** 2).sum() ** 2) / 64)
        mean = (z[:, py, px] ** 2).mean()
        print(f"z^2 at ({px}, {py}): mean {mean:.3f} over 64 seeds, sigma of the mean {sd:.3f}")
        assert abs(mean - 1) <= 4 * sd
        assert np.abs(z[:, py, px]).max() <= np.abs(k).sum() / np.sqrt((k ** 2).sum()) * (1 + 1e-6)
    assert np.abs(np.abs(z[:, 12, 20]).max() - np.abs(z[:, 0, 0]).max()) > 1e-3     # the corner has a normalisation of its own


# ---------------------------------------------------------------- unbiased under its own model
def _scene(W=64, H=48):
    """a crease, an albedo step, a smooth picture and a heteroscedastic sigma"""
    yy, xx = np.mgrid[0:H, 0:W].astype(D)
    left = xx < W // 2
    n = np.where(left[..., None], np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]))          # the crease
    n = n + 0.05 * np.stack([np.sin(xx / 9.0), np.zeros_like(xx), np.cos(yy / 7.0)], -1)
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F)
    depth = (3.0 + 0.01 * xx + 0.02 * yy).astype(F)
    top = yy < H // 2
    albedo = np.where(top[..., None], np.array([0.7, 0.6, 0.5]), np.array([0.3, 0.5, 0.7])).astype(F)     # the albedo step
    cov = np.ones((H, W), F)
    f = dict(normal=n, depth=depth, albedo=albedo, coverage=cov)
    shade = 0.6 + 0.3 * np.sin(xx / 11.0) * np.cos(yy / 13.0) + np.where(left, 0.0, 0.25)
    mu = (albedo.astype(D) * shade[..., None]).astype(F)
    sigma = (0.005 + 0.025 * (0.5 + 0.5 * np.sin(xx / 5.0 + yy / 8.0)) ** 2).astype(F)                 # luma standard deviation
    d = np.stack([0.8 + 0.4 * np.sin(xx / 3.0), 1.0 + 0.2 * np.cos(yy / 4.0), 1.2 + 0.3 * np.sin((xx + yy) / 6.0)], -1)
    d = (d / er._luma64(d[..., 0], d[..., 1], d[..., 2])[..., None]).astype(F)                          # luma(d) = 1
    return f, mu, sigma, d


def _unit_field(rs, W, H, correlated):
    """unit-variance Gaussian noise per pixel: independent, or independent noise passed through the reconstruction weights"""
    xi = rs.standard_normal((H, W))
    if not correlated:
        return xi
    kx, ky = de.kernel()
    inside = np.ones((H, W))
    num, den = np.zeros((H, W)), np.zeros((H, W))
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            k = D(ky[j + 1]) * D(kx[i + 1])
            num += k * dr._shifted(xi, -j, -i)
            den += k * k * dr._shifted(inside, -j, -i)
    return num / np.sqrt(den)


def _ratio(noise_correlated, probe_correlated, iterations, trials=12):
    """(mean estimate / mean true squared luma error of the filtered picture, scatter of the per-trial estimates / mean truth)"""
    f, mu, sigma, d = _scene()
    H, W = sigma.shape
    state = np.full((H, W), 2)
    v = (sigma * sigma).astype(F)
    a = (np.sqrt(v.astype(D)).astype(F)[..., None] * d).astype(F)
    est, true = [], []
    for t in range(trials):
        rs = np.random.RandomState(9000 + t)
        eta = sigma.astype(D) * _unit_field(rs, W, H, noise_correlated)
        y = (mu.astype(D) + eta[..., None] * d.astype(D)).astype(F)
        _, out, pr = de.estimate(y, state, v, a, None, f, kind=0, probes=1, eps=EPS, correlated=probe_correlated, seed=100 + t,
                                 iterations=iterations)
        est.append(out[4])
        true.append(float(((de.luma64(pr["Fy"]) - de.luma64(mu)) ** 2).sum()))
    return float(np.mean(est) / np.mean(true)), float(np.std(est, ddof=1) / np.mean(true))


@pytest.mark.parametrize("correlated", [0, 1])
def test_unbiased_under_its_own_model(correlated):
    """64 x 48, rank-1 colour noise of known luma variance, 12 trials with fixed seeds, 3 passes of the fixed filter, one probe,
    eps = 1/16: with the matching perturbation the mean estimate / mean true squared luma error lies in [0.9, 1.1]."""
    R, scatter = _ratio(correlated, correlated, 3)
    print(f"noise {'reconstruction-correlated' if correlated else 'independent'}, matched probe, 3 passes: ratio {R:.3f}, "
          f"per-trial scatter {scatter:.3f}")
    assert 0.9 <= R <= 1.1


@pytest.mark.parametrize("correlated", [0, 1])
def test_badly_off_under_the_other_model(correlated):
    """the mismatched perturbation at one pass: the ratio lies outside [0.5, 2]"""
    R, scatter = _ratio(correlated, 1 - correlated, 1)
    print(f"noise {'reconstruction-correlated' if correlated else 'independent'}, MISMATCHED probe, 1 pass: ratio {R:.3f}, "
          f"per-trial scatter {scatter:.3f}")
    assert not (0.5 <= R <= 2.0)


# ---------------------------------------------------------------- signs and kernel
def test_signs_and_kernel():
    """the hash against hand-computed values (python integers); K for square pixels; probe k of seed S is probe 0 of seed S + k"""
    def h(q, t):
        M = 0xFFFFFFFF
        x = (q * 0x9E3779B9 + t * 0x85EBCA6B) & M
        x ^= x >> 16
        x = (x * 0x7FEB352D) & M
        x ^= x >> 15
        x = (x * 0x846CA68B) & M
        return x ^ (x >> 16)
    for q, t, want in ((1, 0, 0x01FCE552), (7, 0, 0x9173A5E2), (4, 7, 0x80B65581), (3071, 0xFFFFFFFF, 0x4AF3993A)):
        assert h(q, t) == want
        assert de.sign(np.array([q]), t)[0] == (-1.0 if want >> 31 else 1.0)
    q = np.arange(64 * 48)
    for t in (0, 9, 0xFFFFFFFF):
        b = de.sign(q, t)
        assert b.dtype == F and b.tolist() == [-1.0 if h(int(k), t) >> 31 else 1.0 for k in q]
        assert 0.45 < (b < 0).mean() < 0.55
    kx, ky = de.kernel()
    np.testing.assert_allclose(kx, [0.135257, 0.746824, 0.746824], atol=1e-6, rtol=0)
    np.testing.assert_allclose(ky, kx, atol=0, rtol=0)
    kx2, ky2 = de.kernel(2.0, 1.0)                     # wide pixels: the spread is narrower in x (in pixels) than in y
    assert kx2[0] < kx[0] < ky2[0] and kx2[1] == kx2[2] and ky2[1] == ky2[2]
    W, H = 13, 9
    rs = np.random.RandomState(3)
    y = rs.gamma(1.0, 0.5, (H, W, 3)).astype(F)
    a = (0.1 * rs.gamma(1.0, 0.5, (H, W, 3))).astype(F)
    for corr in (0, 1):
        for S, k in ((5, 3), (0xFFFFFFFE, 3)):
            assert de.field(W, H, (S + k) & 0xFFFFFFFF, corr).tobytes() == de.field(W, H, S + k, corr).tobytes()
        state = np.full((H, W), 2)
        v = np.full((H, W), 0.01, F)
        _, _, p4 = de.estimate(y, state, v, a, None, None, kind=0, iterations=0, probes=4, correlated=corr, seed=0xFFFFFFFE)
        _, _, p1 = de.estimate(y, state, v, a, None, None, kind=0, iterations=0, probes=1, correlated=corr, seed=1)
        assert p4["yp"].tobytes() == p1["yp"].tobytes()


# ---------------------------------------------------------------- the loop of render_until on the filtered metric
def test_render_until_loop_without_a_device():
    """cl2_run_until's chunks (min_samples, then check_every, the last one clipped), the check index as the seed, the first
    e_dn <= target stops -- but not a check whose weighted total is not positive (e_dn = 0 by definition, not by convergence)"""
    from clive2_amd.renderer import Renderer

    class Fake(Renderer):
        def __init__(self, answers):
            self.answers, self.runs, self.seeds, self.samples, self.streams = list(answers), [], [], 0, 1
        error_tracking = True

        def features(self):
            return {}

        def run_samples(self, n):
            self.runs.append(n)
            self.samples += n

        def denoised_error(self, kind, floor=None, seed=0, return_totals=False, **kw):
            self.seeds.append(seed)
            e, t1 = self.answers.pop(0)
            return e, np.array([e, t1, 1, 0, 0, 0, 0, 0], D)

        def __del__(self):
            pass
    r = Fake([(0.5, 1.0), (0.0, -3.0), (0.2, 0.4), (0.1, 0.1)])
    assert r.render_until(0.25, 100, min_samples=2, check_every=8, metric="denoised") == (26, 0.2)
    assert r.runs == [2, 8, 8, 8] and r.seeds == [0, 1, 2]
    r = Fake([(0.5, 1.0), (0.4, 1.0)])
    assert r.render_until(0.25, 13, min_samples=2, check_every=8, metric="guided") == (13, 0.4)
    assert r.runs == [2, 8, 3]
    with pytest.raises(ValueError):
        r.render_until(0.25, 13, metric="denoised", adaptive=True)
    with pytest.raises(ValueError):
        r.render_until(0.25, 13, metric="median")
    with pytest.raises(ValueError):
        r.render_until(0.25, 13, filter_params=dict(iterations=2))


# ---------------------------------------------------------------- plumbing
def test_plumbing(capsys):
    from clive2_amd import _native, render, movie
    assert "cl2_denoise_error" in _native.EXPORTS
    L = C.CDLL(_native.LIB_PATH)
    assert hasattr(L, "cl2_denoise_error")
    assert L.cl2_abi_version() == 6
    with open(os.path.join(ROOT, "include", "clive2_amd.h")) as fh:
        assert "int cl2_denoise_error(" in fh.read()
    out = (C.c_double * 8)()
    assert _native.lib().cl2_denoise_error(None, 0, 3, 2.0, 0.1, 0.1, 1, EPS, 0, 0, 0.001, out, None, 0, None, 0) == -1
    # refused before any renderer exists
    base = ["--scene", "empty", "--width", "32", "--height", "24", "--samples", "8", "--error-of", "denoised"]
    for main in (render.main, movie.main):
        for extra in ([], ["--target-error", "0.1"], ["--denoise"], ["--target-error", "0.1", "--denoise", "--adaptive"],
                      ["--target-error", "0.1", "--denoise", "--robust"], ["--target-error", "0.1", "--robust-denoise"],
                      ["--target-error", "0.1", "--denoise", "--robust-denoise"]):
            with pytest.raises(SystemExit) as ex:
                main(base + extra)
            assert ex.value.code == 2, extra
        with pytest.raises(SystemExit):
            main(["--error-of", "guided"])
    capsys.readouterr()
    from clive2_amd import renderer as rmod
    assert rmod.DENOISED_ERROR_CORRELATED is False
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert f"the C ABI ({len(_native.EXPORTS)} entry points" in fh.read()
    assert len(_native.EXPORTS) == 108
