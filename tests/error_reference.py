"""numpy statement of the error estimates (csrc/error_estimate.hpp and the MOMENTS form of the accumulate kernels in
csrc/kernels.hpp): the addends of one sample, the moment sums in float32, the per-pixel standard errors and the frame metric in
float64, every operation in the order the kernels perform it -- the frame metric's sum included (grid_sum: the fixed grid, the
wave tree, the four-wave sum and the final launch restated).  Arrays are packed [8][W*H] as Renderer.packed_accumulators() and
Renderer.moments() return them.

What the GPU suite pins with it (tests/test_gpu_error.py): standard_error() and relative_error(floor) bit for bit
on renders and on injected states (tests/error_states.py: uncovered pixels with Wt = 0, -0.0, < 0, NaN, +inf; n < 2 beside covered
pixels; S exactly 0, cancelled to either sign, inf - inf; L + floor = 0; sqrt(var) beyond float32; subnormal sums) at 7 x 5,
41 x 25, 512 x 512, 512 x 513 and 1920 x 1080.  residual_sums is the plain float64 statement of what S estimates; the float32
restatement (CPU) and the device's moments (GPU) are held to |S - S*| <= 8 n u T against it (derivation:
test_error_estimate_cpu.test_float32_restatement_is_inside_the_derived_bound; worst ratio observed 0.94 on the CPU, 1.18 on the
device, both signed colours at n = 2)."""
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
    with np.errstate(over="ignore"):
        se = np.sqrt(var).astype(F)                   # +inf where sqrt(var) exceeds float32, as the kernel's (float) does
    se[state == 1] = np.inf
    return se if H is None else se.reshape(H, W, 4)


def _wave_tree(v):
    """lane 0 of `for off in 32, 16, ... 1: v += __shfl_down(v, off)` over the last axis (64 lanes)"""
    h = 32
    while h:
        v = v[..., :h] + v[..., h:2 * h]
        h >>= 1
    return v[..., 0]


def _block_sum(v):
    """err_block_sum3 for one value: v (..., 256) per-thread sums -> the workgroup's sum, (s0 + s1) + (s2 + s3) over the waves"""
    s = _wave_tree(v.reshape(v.shape[:-1] + (4, 64)))
    return (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])


def _strided(v, threads):
    """per-thread sums of v taken in strides of `threads`, each from 0.0 in ascending order"""
    trips = -(-v.size // threads)
    if trips * threads != v.size:
        v = np.concatenate([v, np.zeros(trips * threads - v.size)])          # x + 0.0 = x: the missing trips add nothing
    t = np.zeros(threads)
    for row in v.reshape(trips, threads):
        t = t + row
    return t


def grid_sum(values, blocks=1024):
    """The float64 sum of a per-pixel array in the order of the device's reductions (k_rel_error_partial, k_dens_terms, k_dens_sum
    + err_block_sum3 + k_rel_error_final / k_dens_final): grid = min(ceil(FB / 256), blocks) workgroups of 256; each thread adds
    its pixels in grid-stride order from 0.0; per wave the __shfl_down tree 32, 16, ... 1 as lane 0 sees it; the four waves as
    (s0 + s1) + (s2 + s3); the final launch's 256 threads stride over the partials, then the same tree and the same four-wave sum.
    A pixel the kernel skips is a 0.0 here (the sums are never -0.0, so adding 0.0 changes no bit)."""
    v = np.asarray(values, np.float64).reshape(-1)
    grid = min(-(-v.size // 256), blocks)
    with np.errstate(invalid="ignore", over="ignore"):
        partial = _block_sum(_strided(v, grid * 256).reshape(grid, 256))
        return float(_block_sum(_strided(partial, 256)))


def relative_error(acc, mom, floor, order="grid"):
    """e(floor) = sqrt(mean over covered pixels of var_L / (L + floor)^2); inf without covered pixels or with n < 2.  The sum of
    the terms in the device's order (grid_sum: the same bytes as cl2_relative_error) or, order="pairwise", numpy's own."""
    state, var, L = variances(acc, mom)
    covered = state > 0
    if not covered.any() or (state == 1).any():
        return np.inf
    ok = state == 2
    d = L + floor
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        terms = np.where(ok & (var[:, 3] > 0), var[:, 3] / (d * d), 0.0)
        total = grid_sum(terms) if order == "grid" else terms[ok].sum()
        return float(np.sqrt(total / covered.sum()))


U = 2.0 ** -24                                      # float32 unit roundoff


def residual_sums(xs, ws):
    """The quantity S estimates, in float64 from the float32 addends xs [(P, 3)], ws [(P,)]: (S* (P, 4), T (P, 4)) for b, g, r, luma.
    I_c = sum x_c / sum w, S*_c = sum (x_c - I_c w)^2; luma with the float32 y of each addend (as add_moments computes it) and
    L = luma(I).  T is the magnitude the rounding of the float32 moments scales with:
    T_c = sum x_c^2 + 2 Ibar_c sum |x_c| w + Ibar_c^2 sum w^2, Ibar_c = sum |x_c| / sum w, and for luma the same with
    ybar = luma(|x|), Lbar = luma(Ibar)."""
    x32 = np.stack([np.asarray(x, F) for x in xs])                       # (n, P, 3)
    y32 = (x32[..., 0] * LUMA[0] + x32[..., 1] * LUMA[1]) + x32[..., 2] * LUMA[2]
    x, w, y = x32.astype(np.float64), np.stack([np.asarray(v, F) for v in ws]).astype(np.float64), y32.astype(np.float64)
    Wt = w.sum(0)
    I = x.sum(0) / Wt[:, None]
    L = _luma64(I[:, 0], I[:, 1], I[:, 2])
    S = np.empty((x.shape[1], 4))
    S[:, :3] = ((x - I[None] * w[..., None]) ** 2).sum(0)
    S[:, 3] = ((y - L[None] * w) ** 2).sum(0)
    ax = np.abs(x)
    Ibar = ax.sum(0) / Wt[:, None]
    ybar = _luma64(ax[..., 0], ax[..., 1], ax[..., 2])
    Lbar = _luma64(Ibar[:, 0], Ibar[:, 1], Ibar[:, 2])
    w2 = (w * w).sum(0)
    T = np.empty_like(S)
    T[:, :3] = (x * x).sum(0) + 2.0 * Ibar * (ax * w[..., None]).sum(0) + Ibar * Ibar * w2[:, None]
    T[:, 3] = (ybar * ybar).sum(0) + 2.0 * Lbar * (ybar * w).sum(0) + Lbar * Lbar * w2
    return S, T


def s_from_standard_error(se, acc):
    """S (P, 4) float64 recovered from standard errors (P, 4) and the accumulators: se^2 / scale, scale = n / ((n - 1) Wt^2)"""
    acc = np.asarray(acc, F).reshape(8, -1).astype(np.float64)
    scale = acc[7] / ((acc[7] - 1.0) * (acc[3] * acc[3]))
    return np.asarray(se, F).reshape(-1, 4).astype(np.float64) ** 2 / scale[:, None]


def check_against_residual_sums(se, acc, Sstar, T, n, label):
    """The three assertions of the bound |S - S*| <= 8 n u T (see test_error_estimate_cpu.test_float32_restatement_is_inside_the_derived_bound); returns
    the worst |S - S*| / (n u T)."""
    S = s_from_standard_error(se, acc)
    nuT = n * U * T
    pos = nuT > 0
    ratio = np.abs(S - Sstar)[pos] / nuT[pos]
    well = Sstar > 1000 * 8 * nuT
    se_star = np.sqrt(Sstar * (acc[7].astype(np.float64) / ((acc[7].astype(np.float64) - 1.0) * acc[3].astype(np.float64) ** 2))[:, None])
    rel = np.abs(se.reshape(-1, 4).astype(np.float64)[well] - se_star[well]) / se_star[well]
    zero = se.reshape(-1, 4) == 0
    zr = (Sstar[zero & pos] / nuT[zero & pos]).max() if (zero & pos).any() else 0.0
    print(f"bound {label}: worst |S - S*| / (n u T) {ratio.max():.3f}; well-conditioned {well.mean():.2f} of the values, worst "
          f"relative error of se {rel.max() if rel.size else 0:.2e}; returned as 0: {zero.mean():.2f}, worst S* / (n u T) among them {zr:.3f}")
    assert np.isfinite(S).all()
    assert (np.abs(S - Sstar) <= 8 * nuT).all()
    assert (rel < 5e-4).all()
    assert (Sstar[zero] <= 8 * nuT[zero]).all()
    return ratio.max()
