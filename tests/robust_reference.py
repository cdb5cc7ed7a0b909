"""numpy statement of the robust picture (csrc/robust.hpp): the bucket hook of the accumulate kernels in float32 and the
Gini-trimmed median of means per pixel in float64, every operation in the order the kernels perform it.

Buckets are held as (M, 4, n): bucket k, rows b, g, r, w, n pixels -- Renderer.buckets().reshape(M, 4, -1).  The ranking is done
here with a stable sort and a running count of the valid buckets, the kernel counts pairs: two routes to the one order that the
rule fixes (key ascending, equal keys by bucket index, NaN keys as +inf)."""
import numpy as np

F = np.float32
LUMA = (F(0.0722), F(0.7152), F(0.2126))           # err_luma's weights (csrc/error_estimate.hpp)


def bucket_index(a7, M):
    """(int)a7 % M as the device computes it for a count (a negative remainder is moved up by M; NaN converts to 0)"""
    a = np.nan_to_num(np.asarray(a7, F).astype(np.float64), nan=0.0, posinf=2.0 ** 31 - 1, neginf=-2.0 ** 31)
    return np.trunc(np.clip(a, -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64) % M   # Python's %: already in 0 .. M-1


def add_bucket(bkt, a7, x, w):
    """bkt (M, 4, n) float32 += one addend per pixel (x (n, 3), w (n,)) in bucket (int)a7 % M, a7 (n,) = acc row 7 BEFORE the
    addend: one float32 add per row (in place)."""
    k = bucket_index(a7, bkt.shape[0])
    p = np.arange(bkt.shape[2])
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            bkt[k, c, p] = (bkt[k, c, p] + x[:, c].astype(F)).astype(F)
        bkt[k, 3, p] = (bkt[k, 3, p] + w.astype(F)).astype(F)
    return bkt


def accumulate(xs, ws, M, a7=None, n=None):
    """(acc row 7 (n,), bkt (M, 4, n)) of a sequence of addends added in order from zero (or from the counts a7); n = pixels, needed
    only for an empty sequence"""
    n = len(ws[0]) if n is None else n
    a7 = np.zeros(n, F) if a7 is None else np.asarray(a7, F).copy()
    bkt = np.zeros((M, 4, n), F)
    for x, w in zip(xs, ws):
        add_bucket(bkt, a7, x, w)
        a7 = (a7 + F(1)).astype(F)
    return a7, bkt


def keys(bkt):
    """(valid (M, n), key (M, n) float64, +inf for a NaN key; 0 where the bucket is not valid)"""
    b = np.asarray(bkt, F).astype(np.float64)
    W = b[:, 3]
    valid = (W > 0) & (W < np.inf)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Wd = np.where(valid, W, 1.0)
        I = b[:, :3] / Wd[:, None]
        key = (I[:, 0] * np.float64(LUMA[0]) + I[:, 1] * np.float64(LUMA[1])) + I[:, 2] * np.float64(LUMA[2])
    key = np.where(np.isnan(key), np.inf, key)
    return valid, np.where(valid, key, 0.0)


def gini_trim(bkt):
    """(valid, rank (M, n) 0-based, -1 for a bucket that is not valid; m, G float64, c int (n,))"""
    valid, key = keys(bkt)
    M, n = key.shape
    m = valid.sum(0)
    order = np.argsort(np.where(valid, key, np.inf), axis=0, kind="stable")      # ties in bucket order; invalid ones counted out below
    v_sorted = np.take_along_axis(valid, order, 0)
    k_sorted = np.take_along_axis(key, order, 0)
    pos = np.cumsum(v_sorted, 0) - 1                                             # rank of a valid bucket among the valid ones
    rank = np.full((M, n), -1, np.int64)
    np.put_along_axis(rank, order, np.where(v_sorted, pos, -1), 0)
    S, N = np.zeros(n), np.zeros(n)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for i in range(M):
            v = np.where(k_sorted[i] > 0, k_sorted[i], 0.0)
            coef = (2 * (pos[i] + 1) - m - 1).astype(np.float64)
            S = np.where(v_sorted[i], S + v, S)
            N = np.where(v_sorted[i], N + coef * v, N)
        G = N / (m.astype(np.float64) * S)
        G = np.where(~(G > 0), 0.0, np.where(G > 1, 1.0, G))
        G = np.where(np.isnan(S) | (S == np.inf), 1.0, np.where(~(S > 0), 0.0, G))
        c = np.minimum(np.floor(G * m.astype(np.float64) / 2.0).astype(np.int64), np.where(m > 0, (m - 1) // 2, 0))
    return valid, rank, m, G, c


def robust_picture(bkt, H=None, W=None):
    """(picture (n, 3) float32 BGR, stats (n, 2) float32 = G, c); reshaped to (H, W, .) when H and W are given"""
    bkt = np.asarray(bkt, F)
    valid, rank, m, G, c = gini_trim(bkt)
    kept = valid & (rank >= c[None]) & (rank < (m - c)[None])
    sums = np.zeros((4, bkt.shape[2]), F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(bkt.shape[0]):
            sums = np.where(kept[k][None], (sums + bkt[k]).astype(F), sums)
        pic = (sums[:3] / sums[3][None]).astype(F)
    pic = np.where(np.isfinite(pic) & (m > 0)[None], pic, F(0)).astype(F).T
    stats = np.stack([G.astype(F), c.astype(F)], 1)
    if H is not None:
        return np.ascontiguousarray(pic).reshape(H, W, 3), stats.reshape(H, W, 2)
    return np.ascontiguousarray(pic), stats


def plain_picture(bkt):
    """the ratio estimator over every addend, from the buckets in float64: (n, 3)"""
    b = np.asarray(bkt, F).astype(np.float64).sum(0)
    return (b[:3] / b[3][None]).T
