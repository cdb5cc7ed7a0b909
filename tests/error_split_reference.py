"""numpy restatement of the split of the luma variance into its camera and its light part (csrc/error_split.hpp) and of the mixed
perturbation of noise model 2 (k_de_perturb_split, csrc/denoise_error.hpp), the same operations in the same order.  A helper
module: no tests live here.

    add_split_moments(smom, t, wc, l)    one addend per pixel into the rows [6][n], float32 (in place)
    split_moments_of(parts)              the rows of a sequence of addends, from zero
    rho64(acc, mom, smom)                (rho float64 (n,), state, var_L): split_rho of every pixel
    light_share(acc, mom, smom)          (map float32 (n,), out float64 (4,)): cl2_light_share, the totals in the device's order
    perturb_split(y, a, rho, W, H, t, eps, K)   y' of probe t
    estimate_split(...)                  denoise_error_reference.estimate with the split field
"""
import numpy as np

import denoise_error_reference as de
import error_reference as er

F = np.float32
D = np.float64
LUMA = er.LUMA
SIGN_XOR = 0xA5A5A5A5


def split_luma(c):
    """(scrub(b) 0.0722f + scrub(g) 0.7152f) + scrub(r) 0.2126f of colours (n, >= 3), float32"""
    c = er.scrub(np.asarray(c, F)[:, :3])
    return ((c[:, 0] * LUMA[0] + c[:, 1] * LUMA[1]) + c[:, 2] * LUMA[2]).astype(F)


def add_split_moments(smom, t, wc, l):
    """smom [6][n] += one addend: camera part t (n, >= 3) with weight wc (n,), light part l (n, 4) with wl = l[:, 3]"""
    with np.errstate(invalid="ignore", over="ignore"):
        yc, yl = split_luma(t), split_luma(l)
        wc, wl = np.asarray(wc, F), np.asarray(l, F)[:, 3]
        for row, v in enumerate((yc * yc, yc * wc, wc * wc, yl * yl, yl * wl, wl * wl)):
            smom[row] = (smom[row] + v.astype(F)).astype(F)
    return smom


def split_moments_of(parts):
    """rows of a sequence [(t, wc, l), ...] added in order, from zero"""
    smom = np.zeros((6, len(parts[0][1])), F)
    for t, wc, l in parts:
        add_split_moments(smom, t, wc, l)
    return smom


def rho64(acc, mom, smom):
    """split_rho: (rho (n,) float64, state (n,), var_L (n,) float64)"""
    state, var, L = er.variances(acc, mom)
    m = np.asarray(smom, F).reshape(6, -1).astype(D)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        Sc = (m[0] - 2.0 * L * m[1]) + L * L * m[2]
        Sl = (m[3] - 2.0 * L * m[4]) + L * L * m[5]
        sc, sl = np.where(Sc < 0, 0.0, Sc), np.where(Sl < 0, 0.0, Sl)         # a NaN stays a NaN: rho = 1
        s = sc + sl
        ok = (s > 0) & (s < np.inf)
        rho = np.where(ok & (state == 2), sl / np.where(ok, s, 1.0), 1.0)
    return rho, state, var[:, 3]


def light_share(acc, mom, smom):
    """cl2_light_share: (map float32 (n,), out (4,) float64)"""
    rho, state, vL = rho64(acc, mom, smom)
    use = (state == 2) & np.isfinite(vL)
    out = np.zeros(4, D)
    with np.errstate(invalid="ignore", over="ignore"):
        out[1] = er.grid_sum(np.where(use, rho * vL, 0.0))
        out[2] = er.grid_sum(np.where(use, vL, 0.0))
        out[3] = float(use.sum())
        out[0] = out[1] / out[2] if out[2] > 0 else 0.0
    return rho.astype(F), out


BOTH, QUIET, CAMERA_ONLY, LIGHT_ONLY, CANCEL, OVERFLOW, NANS = range(7)
SPLIT_CLASSES = (BOTH, QUIET, CAMERA_ONLY, LIGHT_ONLY, CANCEL, OVERFLOW, NANS)


def split_rows_for(acc, mom, seed=1, allowed=SPLIT_CLASSES):
    """(cls (n,), smom [6][n]) to go with an injected state acc, mom of error_states: split rows of seven classes, cycling through
    the lanes (pixel p is of class (p + p // 64) % 7, so every class meets every lane), a class outside `allowed` replaced by BOTH:
        BOTH         both parts noisy: residual sums S_c, S_l drawn log-uniformly over six decades about L w
        QUIET        both parts noiseless: every row exactly 0
        CAMERA_ONLY  the light rows exactly 0 (rho = 0)          LIGHT_ONLY  the camera rows exactly 0 (rho = 1)
        CANCEL       rows of exactly proportional parts, y = L w: S cancels to rounding size, either sign (the clamp)
        OVERFLOW     row sums that overflowed to +inf, in the camera part, the light part or both
        NANS         NaN in one row or in all
    Uncovered pixels and n = 0, 1 come with acc; the rows there are whatever the class gives (they must not matter)."""
    acc = np.asarray(acc, F).reshape(8, -1)
    n = acc.shape[1]
    rs = np.random.RandomState(seed)
    p = np.arange(n)
    cls = (p + p // 64) % len(SPLIT_CLASSES)
    cls = np.where(np.isin(cls, allowed), cls, BOTH)
    _, _, L = er.variances(acc, mom)
    L = np.where(np.isfinite(L), L, 1.0)
    cnt = np.maximum(acc[7].astype(D), 2.0)
    smom = np.zeros((6, n), D)
    for part in (0, 1):
        w2 = cnt * rs.uniform(0.25, 4.0, n)                       # sum w^2
        S = 10.0 ** rs.uniform(-6, 0, n) * (1.0 + L * L) * w2
        S = np.where(cls == CANCEL, 0.0, S)
        smom[3 * part + 2] = w2
        smom[3 * part + 1] = L * w2
        smom[3 * part + 0] = L * L * w2 + S
    smom = smom.astype(F)
    smom[:, cls == QUIET] = 0
    smom[3:, cls == CAMERA_ONLY] = 0
    smom[:3, cls == LIGHT_ONLY] = 0
    at = np.flatnonzero(cls == OVERFLOW)
    for k, rows in enumerate(((0,), (3,), (0, 3), (2,), (5,), (0, 1, 2, 3, 4, 5))):
        for row in rows:
            smom[row, at[k::6]] = np.inf
    at = np.flatnonzero(cls == NANS)
    for k, rows in enumerate(((0,), (4,), (0, 1, 2, 3, 4, 5))):
        for row in rows:
            smom[row, at[k::3]] = np.nan
    return cls, np.ascontiguousarray(smom)


def coefficients(rho):
    """(cs, cl) float32 of the float32 rho"""
    r = np.asarray(rho, F).astype(D)
    with np.errstate(invalid="ignore"):
        return np.sqrt(1.0 - r).astype(F), np.sqrt(r).astype(F)


def field_split(W, H, t, rho, K=None):
    """z (H, W) float32 of probe t: cs zK + cl b'"""
    cs, cl = coefficients(np.asarray(rho, F).reshape(H, W))
    zK = de.field(W, H, t, 1, K)
    b = de.sign(np.arange(W * H), (int(t) & 0xFFFFFFFF) ^ SIGN_XOR).reshape(H, W)
    with np.errstate(invalid="ignore"):
        return ((cs * zK).astype(F) + (cl * b).astype(F)).astype(F)


def perturb_split(y, a, rho, t, eps, K=None):
    H, W = np.asarray(y).shape[:2]
    return de.perturb(y, a, field_split(W, H, t, rho, K), eps)


def estimate_split(y, state, v, a, w, f, rho, kind=0, probes=1, eps=1 / 16, seed=0, floor=0.001, K=None, **params):
    """denoise_error_reference.estimate under noise model 2: (map, out, dict(yp=, Fy=, Fyp=) of the last probe)"""
    p = dict(de.DEFAULTS[kind], **params)
    Fy = de.run_filter(kind, y, w, f, **p)
    yps, Fyps = [], []
    for k in range(probes):
        yps.append(perturb_split(y, a, rho, (seed + k) & 0xFFFFFFFF, eps, K))
        Fyps.append(de.run_filter(kind, yps[-1], w, f, **p))
    m, out = de.terms(y, yps, Fy, Fyps, state, v, eps, floor)
    return m, out, dict(yp=yps[-1], Fy=Fy, Fyp=Fyps[-1])
