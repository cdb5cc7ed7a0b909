"""numpy restatement of the denoiser of csrc/denoise.hpp (cl2_denoise), float32 throughout, the same operations in the same
order, taps visited dy outer, dx inner.  A helper module: no tests live here.

    radiance   (H, W, 3) float32 b, g, r: the filter's input c (Renderer.radiance)
    normal     (H, W, 3), depth (H, W), albedo (H, W, 3), coverage (H, W): Renderer.features()
"""
import numpy as np

F = np.float32
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], dtype=F)
DEFAULTS = dict(iterations=3, sigma_color=2.0, sigma_depth=0.1, sigma_albedo=0.1)


def compress(c):
    """x = c / (1 + luma(c)), luma with the b, g, r weights of camera.py."""
    lum = (c[..., 0] * F(0.0722) + c[..., 1] * F(0.7152)) + c[..., 2] * F(0.2126)
    return c / (F(1) + lum)[..., None]


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _shifted(a, oy, ox, fill=0):
    """a[y + oy, x + ox] for every (y, x), `fill` where that lies outside the frame."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = (slice(oy, H), slice(0, H - oy)) if oy >= 0 else (slice(0, H + oy), slice(-oy, H))
    xs, xd = (slice(ox, W), slice(0, W - ox)) if ox >= 0 else (slice(0, W + ox), slice(-ox, W))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[yd, xd] = a[ys, xs]
    return out


def atrous_pass(c, normal, depth, albedo, coverage, i, sigma_color, sigma_depth, sigma_albedo):
    """Pass i (step 2^i) of the filter."""
    c = np.asarray(c, F)
    s = 1 << i
    den_c = F(np.ldexp(F(F(sigma_color) * F(sigma_color)), -2 * i))
    den_a = F(F(sigma_albedo) * F(sigma_albedo))
    den_z = (F(sigma_depth) * depth) * F(s)
    x = compress(c)
    sw = np.zeros(c.shape[:2], F)
    sc = np.zeros(c.shape, F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq = _shifted(c, dy * s, dx * s)
                nq = _shifted(normal, dy * s, dx * s)
                zq = _shifted(depth, dy * s, dx * s)
                aq = _shifted(albedo, dy * s, dx * s)
                covq = _shifted(coverage, dy * s, dx * s)          # 0 outside the frame: skipped like an uncovered tap
                wn = np.maximum(F(0), _dot(normal, nq))
                for _ in range(5):
                    wn = wn * wn
                wz = np.exp(-np.abs(depth - zq) / den_z)
                da = albedo - aq
                wa = np.exp(-_dot(da, da) / den_a)
                dxc = x - compress(cq)
                wc = np.exp(-_dot(dxc, dxc) / den_c)
                w = ((((H5[dx + 2] * H5[dy + 2]) * wn) * wz) * wa) * wc
                w = np.where(covq != 0, w, F(0)).astype(F)
                sw = sw + w
                sc = sc + w[..., None] * cq
        out = sc / sw[..., None]
    keep = (coverage == 0) | (sw <= 0)
    return np.where(keep[..., None], c, out).astype(F)


def denoise(radiance, normal, depth, albedo, coverage, iterations=3, sigma_color=2.0, sigma_depth=0.1, sigma_albedo=0.1):
    c = np.asarray(radiance, F)
    args = [np.asarray(a, F) for a in (normal, depth, albedo, coverage)]
    for i in range(iterations):
        c = atrous_pass(c, *args, i, sigma_color, sigma_depth, sigma_albedo)
    return c
