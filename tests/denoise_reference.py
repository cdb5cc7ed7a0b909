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
    """x = c / (1 + luma(c)), luma with the b, g, r weights of camera.py (in c's own precision)."""
    T = c.dtype.type
    lum = (c[..., 0] * T(F(0.0722)) + c[..., 1] * T(F(0.7152))) + c[..., 2] * T(F(0.2126))
    return c / (T(1) + lum)[..., None]


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


def atrous_pass(c, normal, depth, albedo, coverage, i, sigma_color, sigma_depth, sigma_albedo, dtype=F, return_sw=False):
    """Pass i (step 2^i) of the filter.  A covered pixel whose weight sum is not greater than 0 -- 0 for a zero normal, NaN
    where a denominator is 0 -- keeps its colour, as an uncovered one does.  dtype=np.float64 is the COMPANION: the same
    formula on the same float32 inputs (the sigmas, the constants and the kernel weights H5 are float32 values) with every
    operation in float64 -- the squares den_c and den_a included, which the host forms in float32 -- the yardstick for what
    float32 rounding alone does to the result.  return_sw=True also returns the weight sum."""
    T = dtype                                   # the working precision
    c, normal, depth, albedo = (np.asarray(a, T) for a in (c, normal, depth, albedo))
    h5 = H5.astype(T)
    sigma_color, sigma_depth, sigma_albedo = (F(x) for x in (sigma_color, sigma_depth, sigma_albedo))
    s = 1 << i
    den_c = T(np.ldexp(T(T(sigma_color) * T(sigma_color)), -2 * i))
    den_a = T(T(sigma_albedo) * T(sigma_albedo))
    den_z = (T(sigma_depth) * depth) * T(s)
    x = compress(c)
    sw = np.zeros(c.shape[:2], T)
    sc = np.zeros(c.shape, T)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq = _shifted(c, dy * s, dx * s)
                nq = _shifted(normal, dy * s, dx * s)
                zq = _shifted(depth, dy * s, dx * s)
                aq = _shifted(albedo, dy * s, dx * s)
                covq = _shifted(coverage, dy * s, dx * s)          # 0 outside the frame: skipped like an uncovered tap
                wn = np.maximum(T(0), _dot(normal, nq))
                for _ in range(5):
                    wn = wn * wn
                wz = np.exp(-np.abs(depth - zq) / den_z)
                da = albedo - aq
                wa = np.exp(-_dot(da, da) / den_a)
                dxc = x - compress(cq)
                wc = np.exp(-_dot(dxc, dxc) / den_c)
                w = ((((h5[dx + 2] * h5[dy + 2]) * wn) * wz) * wa) * wc
                w = np.where(covq != 0, w, T(0)).astype(T)
                sw = sw + w
                sc = sc + w[..., None] * cq
        out = sc / sw[..., None]
    keep = (coverage == 0) | ~(sw > 0)
    out = np.where(keep[..., None], c, out).astype(T)
    return (out, sw) if return_sw else out


def denoise(radiance, normal, depth, albedo, coverage, iterations=3, sigma_color=2.0, sigma_depth=0.1, sigma_albedo=0.1, dtype=F,
            return_sw=False):
    """`iterations` passes.  return_sw=True: (picture, smallest weight sum any pass gave each pixel; +inf where no pass formed one)."""
    c = np.asarray(radiance, dtype)
    args = [np.asarray(a, F) for a in (normal, depth, albedo, coverage)]
    sw_min = np.full(c.shape[:2], np.inf)
    for i in range(iterations):
        c, sw = atrous_pass(c, *args, i, sigma_color, sigma_depth, sigma_albedo, dtype=dtype, return_sw=True)
        with np.errstate(invalid="ignore"):
            sw_min = np.where(sw > 0, np.minimum(sw_min, sw), sw_min)
    return (c, sw_min) if return_sw else c


# ---- the feature pass (cl2_render_features: k_feat_rays, k_feat_shade, k_feat_finish) ----
def feature_pass(scene, seeds, samples, closest_hit):
    """The feature buffers of `samples` samples: dict normal (H,W,3), depth (H,W), albedo (H,W,3), coverage (H,W), float32.
    Sample k's rays are oracle.np_kernels.generate_camera_rays from the seed state sample k-1 left (k_feat_rays);
    closest_hit(rays) -> (triangle, t, u, v) for struct_types.Ray records is the walk under test or the oracle's; the sums of
    k_feat_shade are float32 adds in sample order and the divisions of k_feat_finish are numpy's."""
    from clive2_amd import struct_types as st
    from oracle import np_kernels as npk
    W, H = scene.pixel_width, scene.pixel_height
    FB = W * H
    T = scene.triangles
    n0, n1, n2, tn = (np.asarray(T[k][:, :3], F) for k in ("n0", "n1", "n2", "normal"))
    colour = np.asarray(scene.materials["color"][:, :3], F)[T["material"]]
    state = np.ascontiguousarray(seeds, np.uint32).reshape(FB, 2)
    g0, g1 = np.zeros((FB, 4), F), np.zeros((FB, 4), F)
    for _ in range(samples):
        o, d, _, state = npk.generate_camera_rays(scene.camera, state)
        rays = np.zeros(FB, st.Ray)
        rays["origin"][:, :3], rays["direction"][:, :3] = o, d
        tri, t, u, v = closest_hit(rays)[:4]
        at = np.flatnonzero(tri >= 0)
        k, uu, vv = tri[at], u[at, None].astype(F), v[at, None].astype(F)
        s = (n0[k] * ((F(1) - uu) - vv) + n1[k] * uu) + n2[k] * vv
        s = s * (F(1) / np.sqrt(_dot(s, s)))[:, None]
        s = np.where((_dot(d[at], tn[k]) > 0)[:, None], -s, s)
        g0[at, :3] = g0[at, :3] + s
        g0[at, 3] = g0[at, 3] + t[at].astype(F)
        g1[at, :3] = g1[at, :3] + colour[k]
        g1[at, 3] = g1[at, 3] + F(1)
    hit = g1[:, 3] > 0
    hits = g1[hit, 3]
    s = g0[hit, :3]
    ss = _dot(s, s)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.where((ss > 0)[:, None], s * (F(1) / np.sqrt(ss))[:, None], F(0))
    g0[hit, :3], g0[hit, 3] = n, g0[hit, 3] / hits
    g1[hit, :3], g1[hit, 3] = g1[hit, :3] / hits[:, None], hits / F(samples)
    return dict(normal=g0[:, :3].reshape(H, W, 3), depth=g0[:, 3].reshape(H, W), albedo=g1[:, :3].reshape(H, W, 3),
                coverage=g1[:, 3].reshape(H, W))
