"""numpy restatement of the per-pixel choice among the fixed filter's scales (csrc/denoise_select.hpp, cl2_denoise_select): the
same operations in the same order, built on denoise_reference (the passes), denoise_error_reference (inputs, probes, luma) and
error_reference (the order of the totals' sums).  A helper module: no tests live here.

    levels(y, f, K, ...)                       [K+1] pictures L_0 = y .. L_K
    raw_maps(Ly, Lyps, state, v, eps)          (m [K+1][H][W] float32, sure float64) from the levels of y and of every probe's y'
    smooth_pass / smooth(m, state, f, S, ...)  M; dtype=np.float64 is the companion, with_abs=True also smooths |m|
    select(M, state)                           k* int32
    gather(Ly, scale)                          the picture
    totals(M, scale, picture, state, floor)    out[8]
    estimate(...)                              all of it on the CPU

e_sel = out[0] IS BIASED LOW: a minimum over noisy estimates always is, on top of the calibration limits of the estimate itself
(DESIGN 6.15).  It is a diagnostic."""
import numpy as np

import denoise_error_reference as de
import denoise_reference as dr
import error_reference as er

F = np.float32
D = np.float64
DEFAULTS = dict(iterations=3, sigma_color=2.0, sigma_depth=0.1, sigma_albedo=0.1)


def _g(f):
    return f["normal"], f["depth"], f["albedo"], f["coverage"]


def levels(y, f, iterations, sigma_color=2.0, sigma_depth=0.1, sigma_albedo=0.1):
    """L_0 = y, L_(i+1) = pass i of the fixed filter on L_i: float32 (K+1, H, W, 3)"""
    out = [np.asarray(y, F)]
    for i in range(iterations):
        out.append(dr.atrous_pass(out[-1], *_g(f), i, sigma_color, sigma_depth, sigma_albedo))
    return np.stack(out)


def raw_maps(Ly, Lyps, state, v, eps):
    """(m, sure): Ly (K+1, H, W, 3) the levels of y, Lyps a list, in probe order, of the levels of each probe's y' (level 0 is
    y' itself).  sure is the float64 term behind m, whatever the state."""
    state = np.asarray(state)
    ly = de.luma64(Ly[0])
    lf = np.stack([de.luma64(x) for x in Ly])
    s = np.zeros(lf.shape, D)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for Lp in Lyps:
            u = de.luma64(Lp[0]) - ly
            for j in range(len(Ly)):
                s[j] = s[j] + u * (de.luma64(Lp[j]) - lf[j])
        scale = (D(F(eps)) * D(F(eps))) * D(len(Lyps))
        d2 = 2.0 * (s / scale)
        fid = (lf - ly[None]) * (lf - ly[None])
        sure = (fid - np.asarray(v, F).astype(D)[None]) + d2
        m = np.where((state == 2)[None], sure, 0.0).astype(F)
    m[:, state == 1] = np.inf
    return m, sure


def smooth_pass(m, state, f, i, sigma_depth, sigma_albedo, dtype=F, absm=None):
    """Pass i (step 2^i) of the maps' smoothing: m (J, H, W).  dtype=np.float64 is the companion (the same formula on the same
    float32 inputs, every operation in float64).  absm: a second stack smoothed with the same weights (the absolute-value
    companion: sum w |m| / sum w); then (M, Abs) is returned."""
    T = dtype
    normal, depth, albedo, coverage = (np.asarray(a, F) for a in _g(f))
    nT, zT, aT = normal.astype(T), depth.astype(T), albedo.astype(T)
    h5 = dr.H5.astype(T)
    ok = np.asarray(state) == 2
    stacks = [np.moveaxis(np.asarray(m, T), 0, -1)] + ([] if absm is None else [np.moveaxis(np.asarray(absm, T), 0, -1)])
    s = 1 << i
    den_a = T(T(F(sigma_albedo)) * T(F(sigma_albedo)))
    sw = np.zeros(ok.shape, T)
    sums = [np.zeros(x.shape, T) for x in stacks]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den_z = (T(F(sigma_depth)) * zT) * T(s)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                nq = dr._shifted(nT, dy * s, dx * s)
                zq = dr._shifted(zT, dy * s, dx * s)
                aq = dr._shifted(aT, dy * s, dx * s)
                valid = (dr._shifted(coverage, dy * s, dx * s) != 0) & dr._shifted(ok, dy * s, dx * s, fill=False)
                wn = np.maximum(T(0), dr._dot(nT, nq))
                for _ in range(5):
                    wn = wn * wn
                wz = np.exp(-np.abs(zT - zq) / den_z)
                da = aT - aq
                wa = np.exp(-dr._dot(da, da) / den_a)
                w = (((h5[dx + 2] * h5[dy + 2]) * wn) * wz) * wa
                sw = (sw + np.where(valid, w, T(0))).astype(T)
                for k, x in enumerate(stacks):
                    xq = dr._shifted(x, dy * s, dx * s)
                    sums[k] = (sums[k] + np.where(valid[..., None], w[..., None] * xq, T(0))).astype(T)
        keep = ~ok | (coverage == 0) | ~(sw > 0)
        outs = [np.moveaxis(np.where(keep[..., None], x, acc / sw[..., None]).astype(T), -1, 0) for x, acc in zip(stacks, sums)]
    return outs[0] if absm is None else tuple(outs)


def smooth(m, state, f, smooth_passes, sigma_depth=0.1, sigma_albedo=0.1, dtype=F, with_abs=False):
    """M after `smooth_passes` passes (0: m itself); with_abs=True: (M, Abs), Abs = |m| carried through the same weights"""
    M = np.asarray(m, dtype)
    A = np.abs(M) if with_abs else None
    for i in range(smooth_passes):
        if with_abs:
            M, A = smooth_pass(M, state, f, i, sigma_depth, sigma_albedo, dtype, absm=A)
        else:
            M = smooth_pass(M, state, f, i, sigma_depth, sigma_albedo, dtype)
    return (M, A) if with_abs else M


def select(M, state):
    """k*: state 0 takes 0, state 1 takes K; state 2: best = 0, then j = 1 .. K takes over if M_j < M_best or if M_best is NaN and
    M_j is not (ties to the smaller j, a NaN never wins over a number)"""
    M = np.asarray(M)
    state = np.asarray(state)
    best = np.zeros(M.shape[1:], np.int32)
    mb = M[0].copy()
    with np.errstate(invalid="ignore"):
        for j in range(1, len(M)):
            take = (M[j] < mb) | (np.isnan(mb) & ~np.isnan(M[j]))
            best[take] = j
            mb = np.where(take, M[j], mb)
    best[state == 0] = 0
    best[state == 1] = len(M) - 1
    return best


def gather(Ly, scale):
    """out_p = L_(k*_p)(y)_p"""
    return np.take_along_axis(np.asarray(Ly), np.asarray(scale)[None, ..., None].astype(np.int64), 0)[0]


def totals(M, scale, picture, state, floor):
    """out (8,) float64, the sums in the device's order"""
    M = np.asarray(M, F)
    state = np.asarray(state)
    ok = state == 2
    mb = np.take_along_axis(M, np.asarray(scale)[None].astype(np.int64), 0)[0].astype(D)
    out = np.zeros(8, D)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d = de.luma64(picture) + D(floor)
        out[1] = er.grid_sum(np.where(ok & (mb != 0), mb / (d * d), 0.0))
        out[2] = float((state > 0).sum())
        out[3] = float((state == 1).sum())
        out[4] = er.grid_sum(np.where(ok, mb, 0.0))
        out[5] = er.grid_sum(np.where(ok, M[-1].astype(D), 0.0))
        out[6] = er.grid_sum(np.where(ok, M[0].astype(D), 0.0))
        out[7] = er.grid_sum(np.where(state > 0, np.asarray(scale).astype(D), 0.0))
        if out[2] == 0 or out[3] != 0:
            out[0] = np.inf
        else:
            t = out[1] / out[2]
            out[0] = 0.0 if t < 0 else np.sqrt(t)
    return out


def estimate(y, state, v, a, f, probes=1, eps=1 / 16, correlated=0, seed=0, smooth_passes=0, floor=0.001, K=None, **params):
    """The whole call on the CPU: dict(picture, scale, out, m, M, Ly, Lyp (the last probe's levels))"""
    H, W = np.asarray(y).shape[:2]
    p = dict(DEFAULTS, **params)
    Ly = levels(y, f, **p)
    Lyps = []
    for k in range(probes):
        yp = de.perturb(y, a, de.field(W, H, (seed + k) & 0xFFFFFFFF, correlated, K), eps)
        Lyps.append(levels(yp, f, **p))
    m, _ = raw_maps(Ly, Lyps, state, v, eps)
    M = smooth(m, state, f, smooth_passes, p["sigma_depth"], p["sigma_albedo"])
    scale = select(M, state)
    picture = gather(Ly, scale)
    return dict(picture=picture, scale=scale, out=totals(M, scale, picture, state, floor), m=m, M=M, Ly=Ly, Lyp=Lyps[-1])
