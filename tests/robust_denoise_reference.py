"""numpy restatement of the input of cl2_denoise_robust (csrc/denoise_robust.hpp): the robust picture and, as the guided filter's
guide, the variance of the mean of the buckets the Gini trim kept -- float64, every operation in the order the kernel performs it.
A helper module: no tests live here.

The trim and the colour are robust_reference's (gini_trim, keys, robust_picture); the passes that follow are
guided_denoise_reference.denoise, unchanged.  Buckets are held as (M, 4, n), as in robust_reference."""
import numpy as np

import guided_denoise_reference as gr
import robust_reference as rr

F = np.float32
CAP = gr.CAP
DEFAULTS = dict(iterations=4, sigma_luma=4.0, sigma_depth=0.1, sigma_albedo=0.1)


def kept_buckets(bkt):
    """(kept (M, n) bool, key (M, n) float64, m (n,), c (n,)): the buckets with ranks c + 1 .. m - c"""
    valid, rank, m, G, c = rr.gini_trim(bkt)
    _, key = rr.keys(bkt)
    return valid & (rank >= c[None]) & (rank < (m - c)[None]), key, m, c


def input_variance(bkt):
    """v (n,) float32: 0 at m = 0, 2^100 with fewer than two kept buckets, else (float32) min(var, 2^100) with
    ybar = (sum key) / n, Q = sum (key - ybar)^2, var = (Q / (n - 1)) / n over the kept buckets in ascending bucket index."""
    bkt = np.asarray(bkt, F)
    kept, key, m, c = kept_buckets(bkt)
    n = m - 2 * c
    assert (kept.sum(0) == n).all()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = np.zeros(bkt.shape[2])
        for k in range(bkt.shape[0]):
            s = np.where(kept[k], s + key[k], s)
        ybar = s / n.astype(np.float64)
        Q = np.zeros(bkt.shape[2])
        for k in range(bkt.shape[0]):
            d = key[k] - ybar
            Q = np.where(kept[k], Q + d * d, Q)
        var = (Q / (n - 1).astype(np.float64)) / n.astype(np.float64)
        v = np.where(var < np.float64(CAP), var, np.float64(CAP)).astype(F)          # a NaN takes the cap too
    v[n < 2] = CAP
    v[m == 0] = 0
    return v


def input_state(bkt, H=None, W=None):
    """(c (n, 3) float32 BGR, v (n,) float32) as k_denoise_robust_input writes them; reshaped to (H, W, 3) and (H, W) when H and W
    are given"""
    c = rr.robust_picture(bkt)[0]
    v = input_variance(bkt)
    if H is not None:
        return c.reshape(H, W, 3), v.reshape(H, W)
    return c, v


def denoise(bkt, H, W, normal, depth, albedo, coverage, **kw):
    """(picture, v') of cl2_denoise_robust: input_state, then the guided filter's passes"""
    c, v = input_state(bkt, H, W)
    return gr.denoise(c, v, normal, depth, albedo, coverage, **kw)
