"""numpy statement of the error estimates (csrc/error_estimate.hpp and the MOMENTS form of the accumulate kernels in
csrc/kernels.hpp): the addends of one sample, the moment sums in float32, the per-pixel standard errors and the frame metric in
float64, every operation in the order the kernels perform it.  Arrays are packed [8][W*H] as Renderer.packed_accumulators()
and Renderer.moments() return them."""
import numpy as np

F = np.float32
LUMA = (F(0.0722), F(0.7152), F(0.2126))           # dn_compress's luma weights (csrc/denoise.hpp)


def scrub(x):
    x = np.asarray(x, F)
    return np.where(np.isfinite(x), x, F(0)).astype(F)


def addends(finalized, light, sample_weights):
    """One sample's addends from the per-sample images of export_sample_images(): x (n, 3) b, g, r and w (n,), float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = scrub(light[:, :3].astype(F) + finalized[:, :3].astype(F))
        w = (sample_weights.astype(F) + light[:, 3].astype(F)).astype(F)
    return x, w


def add_moments(mom, x, w):
    """mom [8][n] float32 += the second moments of one addend per pixel, one float32 add per row (in place)."""
    x0, x1, x2 = (x[:, c].astype(F) for c in range(3))
    w = w.astype(F)
    y = (x0 * LUMA[0] + x1 * LUMA[1]) + x2 * LUMA[2]
    for row, v in enumerate((x0 * x0, x1 * x1, x2 * x2, w * w, x0 * w, x1 * w, x2 * w, y * y)):
        mom[row] = (mom[row] + v).astype(F)
    return mom


def moments_of(xs, ws):
    """Moment buffer of a sequence of addends [(x (n,3), w (n,)), ...] added in order, from zero."""
    mom = np.zeros((8, len(ws[0])), F)
    for x, w in zip(xs, ws):
        add_moments(mom, x, w)
    return mom


def _luma64(b, g, r):
    return (b * np.float64(LUMA[0]) + g * np.float64(LUMA[1])) + r * np.float64(LUMA[2])


def variances(acc, mom):
    """(state, var (n, 4) b, g, r, luma, L): state 0 uncovered, 1 n < 2, 2 estimate; float64 as err_pixel computes it."""
    acc = np.asarray(acc, F).reshape(8, -1).astype(np.float64)
    m = np.asarray(mom, F).reshape(8, -1).astype(np.float64)
    Wt, n = acc[3], acc[7]
    covered = (Wt > 0) & np.isfinite(Wt)
    state = np.where(covered, np.where(n < 2, 1, 2), 0)
    ok = state == 2
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Wd = np.where(ok, Wt, 1.0)
        nd = np.where(ok, n, 2.0)
        I = acc[:3] / Wd
        L = _luma64(I[0], I[1], I[2])
        scale = nd / ((nd - 1.0) * (Wd * Wd))
        var = np.zeros((4, m.shape[1]))
        for c in range(3):
            S = (m[c] - 2.0 * I[c] * m[4 + c]) + I[c] * I[c] * m[3]
            var[c] = np.where(S > 0, S, 0.0) * scale
        myw = _luma64(m[4], m[5], m[6])
        S = (m[7] - 2.0 * L * myw) + L * L * m[3]
        var[3] = np.where(S > 0, S, 0.0) * scale
    var[:, ~ok] = 0.0
    return state, var.T, np.where(ok, L, 0.0)


def standard_error(acc, mom, H=None, W=None):
    """Per-pixel standard errors, float32 (n, 4) or (H, W, 4): 0 uncovered, inf with n < 2."""
    state, var, _ = variances(acc, mom)
    se = np.sqrt(var).astype(F)
    se[state == 1] = np.inf
    return se if H is None else se.reshape(H, W, 4)


def relative_error(acc, mom, floor):
    """e(floor) = sqrt(mean over covered pixels of var_L / (L + floor)^2); inf without covered pixels or with n < 2."""
    state, var, L = variances(acc, mom)
    covered = state > 0
    if not covered.any() or (state == 1).any():
        return np.inf
    ok = state == 2
    vL, d = var[ok, 3], L[ok] + floor
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(vL > 0, vL / (d * d), 0.0)
    return float(np.sqrt(terms.sum() / covered.sum()))
