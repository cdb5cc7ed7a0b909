"""numpy restatement of the error estimate of the filtered picture (csrc/denoise_error.hpp, cl2_denoise_error): Monte-Carlo SURE
over the passes of the fixed filter (denoise_reference) or the guided one (guided_denoise_reference), the same operations in the
same order, the totals in the order of the device's reductions (error_reference.grid_sum).  A helper module: no tests live here.

    inputs(acc, mom, W, H)            y (H,W,3), state (H,W), v (H,W), a (H,W,3), w (H,W): what k_de_input forms
    sign / field                      the hashed signs b and the perturbation field z of one probe
    perturb(y, a, z, eps)             y' = y + (eps z) a
    run_filter(kind, y, w, f, ...)    F
    terms(...)                        (map, out[8]) from y, the probes' y' and F(y'), F(y), state and v
    estimate(...)                     all of it on the CPU
"""
import math

import numpy as np

import denoise_reference as dr
import error_reference as er
import guided_denoise_reference as gr

F = np.float32
D = np.float64
CAP = gr.CAP
KINDS = {"denoised": 0, "guided": 1}
DEFAULTS = {0: dict(iterations=3, sigma=2.0, sigma_depth=0.1, sigma_albedo=0.1),
            1: dict(iterations=4, sigma=4.0, sigma_depth=0.1, sigma_albedo=0.1)}


def luma64(c):
    """err_luma of float32 colours (..., 3), in float64"""
    c = np.asarray(c, F).astype(D)
    return er._luma64(c[..., 0], c[..., 1], c[..., 2])


def inputs(acc, mom, W, H):
    """k_de_input: the colour y, err_pixel's state, v (state 2 only, else 0), a = s d, and the .w the guided filter carries"""
    acc = np.asarray(acc, F).reshape(8, -1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c = (acc[:3] / acc[3]).astype(F)
        y = np.where(np.isfinite(c), c, F(0)).T.reshape(H, W, 3).copy()
        state, var, _ = er.variances(acc, mom)
        w = gr.input_variance(acc, mom)
        ok = state == 2
        v = np.where(ok, w, F(0)).astype(F)
        s = np.sqrt(v.astype(D)).astype(F)
        se = np.sqrt(var[:, :3])
        l = er._luma64(se[:, 0], se[:, 1], se[:, 2])
        fine = (l > 0) & np.isfinite(l)
        d = np.where(fine[:, None], (se / np.where(fine, l, 1.0)[:, None]).astype(F), F(1)).astype(F)
        a = (s[:, None] * d).astype(F)
    a[~ok] = 0
    return y, state.reshape(H, W), v.reshape(H, W), a.reshape(H, W, 3), w.reshape(H, W)


def sign(q, t):
    """b_q of probe t: +-1.0 float32"""
    M = np.uint64(0xFFFFFFFF)
    q = np.asarray(q).astype(np.uint64)
    h = (q * np.uint64(0x9E3779B9) + np.uint64(int(t) & 0xFFFFFFFF) * np.uint64(0x85EBCA6B)) & M
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & M
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & M
    h ^= h >> np.uint64(16)
    return np.where(h >> np.uint64(31), F(-1), F(1)).astype(F)


def kernel(ppw=1.0, pph=1.0):
    """(K_x, K_y), float32 (3,) each, index i + 1: the mean reconstruction weight of a camera sample for the pixel i to its right.
    ppw, pph: the camera's physical pixel sizes, float32 as the resolve kernel forms them."""
    ppw, pph = float(F(ppw)), float(F(pph))
    s2 = ppw * ppw + pph * pph
    out = []
    for c in (s2 / (2.0 * ppw * ppw), s2 / (2.0 * pph * pph)):
        q = math.sqrt(c)
        out.append(np.array([0.5 * math.sqrt(c * math.pi) * (math.erf((1.0 - i) / q) - math.erf(-i / q)) for i in (-1, 0, 1)], F))
    return tuple(out)


def camera_kernel(scene):
    cam = np.asarray(scene.camera).reshape(-1)[0]
    ppw = F(cam["phys_width"]) / F(cam["pixel_width"])
    pph = F(cam["phys_height"]) / F(cam["pixel_height"])
    return kernel(ppw, pph)


def field(W, H, t, correlated=0, K=None):
    """z (H, W) float32 of probe t"""
    b = sign(np.arange(W * H), t).reshape(H, W)
    if not correlated:
        return b
    kx, ky = kernel() if K is None else K
    inside = np.ones((H, W), bool)
    num, den = np.zeros((H, W), F), np.zeros((H, W), F)
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            k = F(ky[j + 1]) * F(kx[i + 1])
            src = dr._shifted(b, -j, -i)                   # b[y - j, x - i]
            m = dr._shifted(inside, -j, -i, fill=False)
            num = (num + np.where(m, k * src, F(0))).astype(F)
            den = (den + np.where(m, k * k, F(0))).astype(F)
    return (num.astype(D) / np.sqrt(den.astype(D))).astype(F)


def perturb(y, a, z, eps):
    ez = (F(eps) * np.asarray(z, F)).astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(y, F) + ez[..., None] * np.asarray(a, F)).astype(F)


def run_filter(kind, y, w, f, iterations, sigma, sigma_depth, sigma_albedo):
    """F: `iterations` passes of filter `kind` on the colours y; w: the guided filter's .w; f: dict of Renderer.features()"""
    if iterations == 0:
        return np.asarray(y, F)
    g = (f["normal"], f["depth"], f["albedo"], f["coverage"])
    if kind == 0:
        return dr.denoise(y, *g, iterations=iterations, sigma_color=sigma, sigma_depth=sigma_depth, sigma_albedo=sigma_albedo)
    return gr.denoise(y, w, *g, iterations=iterations, sigma_luma=sigma, sigma_depth=sigma_depth, sigma_albedo=sigma_albedo)[0]


def terms(y, yps, Fy, Fyps, state, v, eps, floor):
    """(map (H, W) float32, out (8,) float64) from the probes' y' and F(y') (lists, in probe order)"""
    state = np.asarray(state)
    ly, lf = luma64(y), luma64(Fy)
    s = np.zeros(ly.shape, D)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for yp, Fyp in zip(yps, Fyps):
            s = s + (luma64(yp) - ly) * (luma64(Fyp) - lf)
        scale = (D(F(eps)) * D(F(eps))) * D(len(yps))
        d2 = 2.0 * (s / scale)
        fid = (lf - ly) * (lf - ly)
        sure = (fid - np.asarray(v, F).astype(D)) + d2
        ok = state == 2
        m = np.where(ok, sure, 0.0).astype(F)
        m[state == 1] = np.inf
        den = lf + D(floor)
        t1 = np.where(ok & (sure != 0), sure / (den * den), 0.0)
        out = np.zeros(8, D)
        out[1] = er.grid_sum(t1)
        out[2] = float((state > 0).sum())
        out[3] = float((state == 1).sum())
        for k, x in ((4, sure), (5, fid), (6, np.asarray(v, F).astype(D)), (7, d2)):
            out[k] = er.grid_sum(np.where(ok, x, 0.0))
        if out[2] == 0 or out[3] != 0:
            out[0] = np.inf
        else:
            t = out[1] / out[2]
            out[0] = 0.0 if t < 0 else np.sqrt(t)
    return m, out


def estimate(y, state, v, a, w, f, kind=0, probes=1, eps=1 / 16, correlated=0, seed=0, floor=0.001, K=None, **params):
    """The whole estimate on the CPU: (map, out, dict(yp=, Fy=, Fyp=) of the last probe)"""
    H, W = y.shape[:2]
    p = dict(DEFAULTS[kind], **params)
    Fy = run_filter(kind, y, w, f, **p)
    yps, Fyps = [], []
    for k in range(probes):
        yps.append(perturb(y, a, field(W, H, (seed + k) & 0xFFFFFFFF, correlated, K), eps))
        Fyps.append(run_filter(kind, yps[-1], w, f, **p))
    m, out = terms(y, yps, Fy, Fyps, state, v, eps, floor)
    return m, out, dict(yp=yps[-1], Fy=Fy, Fyp=Fyps[-1])


def delta_rounding(yp, v, eps):
    """r (H, W): a bound on the relative error of the realised perturbation u = luma(y') - luma(y) against eps b s, s^2 = v.
    y'_c = fl(y_c + (eps z) a_c) with eps z a power of two times +-1, so the product is exact and the sum rounds once: an error of
    at most 2^-24 |y'_c| per channel, 2^-24 luma(|y'|) in luma.  a_c = fl(s d_c) and d_c = fl(se_c / luma(se)) add 2^-24 each and
    s = fl(sqrt(v)) another: 2^-22 covers them.  Hence |u^2 / eps^2 - v| <= v (2 r + r^2).  inf where v = 0 (there u = 0 = v)."""
    s = np.sqrt(np.asarray(v, F).astype(D))
    with np.errstate(divide="ignore", invalid="ignore"):
        return 2.0 ** -22 + 2.0 ** -24 * luma64(np.abs(yp)) / (float(F(eps)) * s)


def same(a, b):
    """bit for bit, a NaN equal to any NaN (the device's default NaN and numpy's differ in their sign bit)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool((na == nb).all() and (a.view(u)[~na] == b.view(u)[~nb]).all())
