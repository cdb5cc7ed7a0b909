"""numpy statement of adaptive sampling (csrc/adaptive.hpp): the density from the error estimate, its
quantisation to units of 2^-16, the per-pass slot offsets and slot ranges, the weights 1/m and the mapped finalize + accumulate
in float32, every operation in the order the kernels perform it.

The two double sums (the finite error terms in `density_from_terms`, the density in `quantise`) are taken in the device's
reduction order (error_reference.grid_sum), so M of a density and of an error state equals the device's as integers; GPU tests
assert that on injected accumulator / moment states at 7 x 5 ... 1920 x 1080 (tests/test_gpu_adaptive.py).  order="pairwise"
gives numpy's own sum instead: the scale of the floors can then differ in its last bits, and an M_q by a unit."""
import numpy as np

from error_reference import scrub, add_moments, variances, grid_sum

F = np.float32
SHIFT = 16
UNIT = 1 << SHIFT
KAPPA = 16.0
M32 = 0xFFFFFFFF


def fmix32(h):
    """murmur3's 32-bit finaliser on Python ints"""
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def offset(pass_index, s):
    """u in [0, 2^16) of pass `pass_index` (the handle's count of passes rendered with a density), plane s"""
    return fmix32((0x9E3779B9 * pass_index + s) & M32) >> 16


def quantise(m, order="grid"):
    """M (uint64) of a density m (positive finite weights): M_q = 1 + F_q + extra_q (one unit reserved per pixel: M_q >= 1),
    F_q = floor(m_q scale),
    scale = FB (2^16 - 1) / sum m (1 - 2^-30), the deficit D = FB (2^16 - 1) - sum F spread as
    extra_q = floor((q+1) D / FB) - floor(q D / FB).  sum M = FB 2^16 exactly."""
    m = np.asarray(m, F).reshape(-1).astype(np.float64)
    FB = m.size
    scale = (FB * 65535.0 / (grid_sum(m) if order == "grid" else np.sum(m))) * (1.0 - 2.0 ** -30)
    Fq = np.floor(m * scale).astype(np.uint64)
    D = FB * 65535 - int(Fq.sum(dtype=np.uint64))
    assert D >= 0
    q = np.arange(FB, dtype=np.uint64)
    extra = ((q + np.uint64(1)) * np.uint64(D)) // np.uint64(FB) - (q * np.uint64(D)) // np.uint64(FB)
    return np.uint64(1) + Fq + extra


def from_density(d):
    """M of a density read back with Renderer.sample_density() (M / 2^16 in float32: exact while the density is below 256)"""
    d = np.asarray(d, F).reshape(-1).astype(np.float64)
    M = np.rint(d * UNIT).astype(np.uint64)
    assert np.array_equal(M.astype(np.float64) / UNIT, d), "density not exactly representable (>= 256?)"
    return M


def prefix(M):
    return np.cumsum(np.asarray(M, np.uint64), dtype=np.uint64)


def ranges(C, u):
    """slots [lo, hi) of every pixel in a plane drawn with offset u (C in 64 bits: it passes 2^32 from 65,536 pixels on)"""
    C = np.asarray(C, np.uint64)
    prev = np.concatenate([np.zeros(1, np.uint64), C[:-1]])
    lo = ((prev + np.uint64(u)) >> np.uint64(SHIFT)).astype(np.int64)
    hi = ((C + np.uint64(u)) >> np.uint64(SHIFT)).astype(np.int64)
    return lo, hi


def slot_map(C, u):
    """slot -> pixel of one plane"""
    lo, hi = ranges(C, u)
    return np.repeat(np.arange(len(C)), hi - lo)


def inv_density(M):
    """1/m_q = (float)(2^16 / M_q)"""
    return (65536.0 / np.asarray(M, np.uint64).astype(np.float64)).astype(F)


def camera_samples(C, first_pass, passes, streams):
    """camera samples per pixel after `passes` mapped passes numbered first_pass, first_pass + 1, ..."""
    n = np.zeros(len(C), np.int64)
    for p in range(first_pass, first_pass + passes):
        for s in range(streams):
            lo, hi = ranges(C, offset(p, s))
            n += hi - lo
    return n


def terms(acc, mom, floor):
    """r_q = sqrt(var_L) / (L + floor) as float32 (k_dens_terms): 0 uncovered or var_L = 0, +inf for a term to be clipped"""
    state, var, L = variances(acc, mom)
    vl = var[:, 3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = np.sqrt(vl) / (L + floor)
    t = np.where(state == 2, np.where(vl > 0, t, 0.0), 0.0)
    t = np.where((state == 2) & (vl > 0) & ~((t >= 0) & (t < np.inf)), np.inf, t)
    t = np.where(state == 1, np.inf, t)
    with np.errstate(over="ignore"):
        return t.astype(F)                            # +inf where the term exceeds float32: clipped like the others


def density_from_terms(r, beta, order="grid"):
    """m = beta + (1 - beta) min(r, KAPPA mean) / mean in float32, mean over the finite terms (their float32 values widened, summed
    in the device's order or, order="pairwise", numpy's); None when none is finite"""
    r = np.asarray(r, F).reshape(-1)
    fin = np.isfinite(r)
    if not fin.any():
        return None
    total = grid_sum(np.where(fin, r, F(0))) if order == "grid" else np.sum(r[fin].astype(np.float64))
    mean = total / fin.sum()
    if not mean > 0:
        return np.ones(r.shape, F)
    t = np.minimum(np.where(fin, r.astype(np.float64), np.inf), KAPPA * mean)
    return (beta + (1.0 - beta) * (t / mean)).astype(F)


def finalize_accumulate(agg, light, uni, acc, mom, C, invm, pass_index, W, H, streams=1, pixels=None):
    """k_finalize_accumulate_mapped on host arrays: agg [13][B] (rows of export_aggregators' layout: 9 filter weights,
    contribution b, g, r, weight), light / uni (B, 4), acc / mom [8][FB] (updated in place, mom may be None).  Returns the
    camera samples each pixel received.  pixels = an index array: only those pixels are restated (the per-pixel loops are
    Python); the columns of acc / mom of every other pixel then hold no restatement and must not be compared."""
    FB = W * H
    B = FB * streams
    received = np.zeros(FB, np.int64)
    todo = range(FB) if pixels is None else [int(p) for p in pixels]
    for s in range(streams):
        base = s * FB
        lo, hi = ranges(C, offset(pass_index, s))
        tot = np.zeros((FB, 3), F)
        wsum = np.zeros(FB, F)
        for p in todo:
            t0 = t1 = t2 = F(0)
            ws = F(0)
            px, py = p % W, p // W
            for i in (-1, 0, 1):
                for j in (-1, 0, 1):
                    sx, sy = px + i, py + j
                    if sx < 0 or sx >= W or sy < 0 or sy >= H:
                        continue
                    q = sy * W + sx
                    row = (1 - i) * 3 + (1 - j)
                    for slot in range(lo[q], hi[q]):
                        k = base + slot
                        wt = F(agg[row, k]) * invm[q]
                        t0 = F(t0 + F(wt * F(agg[9, k])))
                        t1 = F(t1 + F(wt * F(agg[10, k])))
                        t2 = F(t2 + F(wt * F(agg[11, k])))
                        ws = F(ws + F(wt * F(agg[12, k])))
            tot[p] = (t0, t1, t2)
            wsum[p] = ws
        l = light[base:base + FB].astype(F)
        with np.errstate(invalid="ignore", over="ignore"):
            x = scrub(l[:, :3] + tot)
            w = (wsum + l[:, 3]).astype(F)
        for c in range(3):
            acc[c] = (acc[c] + x[:, c]).astype(F)
        acc[3] = (acc[3] + w).astype(F)
        for p in todo:
            for slot in range(lo[p], hi[p]):
                u4 = scrub(uni[base + slot, :3])
                for c in range(3):
                    acc[4 + c, p] = F(acc[4 + c, p] + F(invm[p] * u4[c]))
        acc[7] = (acc[7] + F(1)).astype(F)
        if mom is not None:
            add_moments(mom, x, w)
        received += hi - lo
    return received
