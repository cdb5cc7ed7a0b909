"""numpy restatement of the variance-guided denoiser of csrc/denoise_guided.hpp (cl2_denoise_guided), float32 throughout, the
same operations in the same order, taps visited dy outer, dx inner.  A helper module: no tests live here.

    radiance   (H, W, 3) float32 b, g, r: the filter's input c (Renderer.radiance)
    v          (H, W) float32: the guide variance (input_variance: the luma variance of the error estimate, capped at 2^100)
    normal     (H, W, 3), depth (H, W), albedo (H, W, 3), coverage (H, W): Renderer.features()

The variance that comes back is the filter's guide, not an error estimate of the filtered picture.
"""
import numpy as np

import denoise_reference as dr
import error_reference as er

F = np.float32
H5 = dr.H5
G3 = np.array([1 / 4, 1 / 2, 1 / 4], dtype=F)
CAP = F(2.0 ** 100)
DEFAULTS = dict(iterations=4, sigma_luma=4.0, sigma_depth=0.1, sigma_albedo=0.1)


def input_variance(acc, mom, H=None, W=None):
    """v of k_denoise_guided_input from packed accumulators and moments: (float32) min(var_L, 2^100); 2^100 with n < 2;
    0 where the render left the pixel uncovered."""
    state, var, _ = er.variances(acc, mom)
    vl = var[:, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where(vl < np.float64(CAP), vl, np.float64(CAP)).astype(F)      # a NaN takes the cap too
    v[state == 1] = CAP
    v[state == 0] = 0
    return v if H is None else v.reshape(H, W)


def luma(c):
    return (c[..., 0] * F(0.0722) + c[..., 1] * F(0.7152)) + c[..., 2] * F(0.2126)


def smoothed_variance(v, coverage):
    """vbar: the 3 x 3 of v with g = (1/4, 1/2, 1/4), over taps in the frame with coverage, offsets never scaled by the step."""
    sg = np.zeros(v.shape, F)
    sv = np.zeros(v.shape, F)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            vq = dr._shifted(v, dy, dx)
            covq = dr._shifted(coverage, dy, dx)
            gg = G3[dy + 1] * G3[dx + 1]
            sg = sg + np.where(covq != 0, gg, F(0)).astype(F)
            sv = sv + np.where(covq != 0, gg * vq, F(0)).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sg > 0, sv / sg, F(0)).astype(F)


def guided_pass(c, v, normal, depth, albedo, coverage, i, sigma_luma, sigma_depth, sigma_albedo):
    """Pass i (step 2^i): (c', v')."""
    c, v = np.asarray(c, F), np.asarray(v, F)
    s = 1 << i
    den_a = F(F(sigma_albedo) * F(sigma_albedo))
    den_z = (F(sigma_depth) * depth) * F(s)
    den_l = (F(sigma_luma) * np.sqrt(smoothed_variance(v, coverage)) + F(1e-8)).astype(F)
    lp = luma(c)
    sw = np.zeros(c.shape[:2], F)
    sc = np.zeros(c.shape, F)
    sv = np.zeros(c.shape[:2], F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq = dr._shifted(c, dy * s, dx * s)
                vq = dr._shifted(v, dy * s, dx * s)
                nq = dr._shifted(normal, dy * s, dx * s)
                zq = dr._shifted(depth, dy * s, dx * s)
                aq = dr._shifted(albedo, dy * s, dx * s)
                covq = dr._shifted(coverage, dy * s, dx * s)        # 0 outside the frame: skipped like an uncovered tap
                wn = np.maximum(F(0), dr._dot(normal, nq))
                for _ in range(5):
                    wn = wn * wn
                wz = np.exp(-np.abs(depth - zq) / den_z)
                da = albedo - aq
                wa = np.exp(-dr._dot(da, da) / den_a)
                wl = np.exp(-np.abs(lp - luma(cq)) / den_l)
                w = ((((H5[dx + 2] * H5[dy + 2]) * wn) * wz) * wa) * wl
                w = np.where(covq != 0, w, F(0)).astype(F)
                sw = sw + w
                sc = sc + w[..., None] * cq
                sv = sv + (w * w) * vq
        out = sc / sw[..., None]
        vout = sv / (sw * sw)
    keep = (coverage == 0) | ~(sw > 0)
    return np.where(keep[..., None], c, out).astype(F), np.where(keep, v, vout).astype(F)


def denoise(radiance, v, normal, depth, albedo, coverage, iterations=4, sigma_luma=4.0, sigma_depth=0.1, sigma_albedo=0.1):
    """(picture, v') after `iterations` passes."""
    c, v = np.asarray(radiance, F), np.asarray(v, F)
    args = [np.asarray(a, F) for a in (normal, depth, albedo, coverage)]
    for i in range(iterations):
        c, v = guided_pass(c, v, *args, i, sigma_luma, sigma_depth, sigma_albedo)
    return c, v
