"""Synthetic (acc row 7, bucket) states for the tests of the robust picture (csrc/robust.hpp), on the CPU and on the device.

A STATE is a pair a7 (FB,), bkt (M, 4, FB) float32 as Renderer.load_buckets() takes the latter.  Its pixels are drawn from a pool
of pixel states, one class per pixel:

    ORDINARY   n in {M, 3M+1, 64, 4096} addends (gamma colours, uniform weights) through the hook (robust_reference.add_bucket)
    FIREFLY    an ordinary n = 64 state with one bucket's colour at 1e3 .. 1e6 times the others
    PARTIAL    n = 0, 1, 2 or 3 addends: m = 0, 1, 2, 3 valid buckets, the others empty
    UNCOVERED  every W_k one of 0, -0.0, negative, NaN, +inf; the colour rows arbitrary, NaN and inf included
    TIES       equal keys in t = 2 .. M buckets (t = M: all equal), exactly: X = I w with I a power of two and w in {1/2, 1, 2, 4}
    ZERO       all keys 0 (colour sums 0, weights positive)
    NEGATIVE   an ordinary state with the colour sums of some or of all buckets negated
    NONFINITE  an ordinary state with +inf, -inf or NaN in a colour sum of one to three valid buckets
    BOUNDARY   M // 2 buckets with key exactly 0, the others with one equal key (green = a power of two): G is exactly 0.5 for even
               M, and at m = 8 the trim c is exactly 2.  Its neighbours either side: one of the equal colour sums one float32 ulp up
               (G just above 0.5; an ulp DOWN also raises G, equal keys being the least unequal) and one zero key raised to 2^-50
               of the others (G a few float64 ulps below 0.5, c = 1 at m = 8)

Class by position, as tests/error_states.py lays its states out: in every third wave-sized run of pixels the classes cycle through
the lanes (every class in the wave), the next run is ORDINARY only, the third is a seeded draw."""
import numpy as np

import robust_reference as rr

F = np.float32
ORDINARY, FIREFLY, PARTIAL, UNCOVERED, TIES, ZERO, NEGATIVE, NONFINITE, BOUNDARY = range(9)
ALL = tuple(range(9))
NAMES = ("ordinary", "firefly", "partial", "uncovered", "ties", "zero", "negative", "nonfinite", "boundary")
POOL = 16384


def _ordinary(rs, M, m, n):
    xs = (rs.gamma(1.0, 0.5, (m, 3)).astype(F) for _ in range(n))
    ws = [rs.uniform(0.5, 2.0, m).astype(F) for _ in range(n)]
    return rr.accumulate(xs, ws, M, n=m)


def pool(M, seed=20241017):
    """(cls (POOL,), a7 (POOL,), bkt (M, 4, POOL)): the pixel states the frames are filled from"""
    rs = np.random.RandomState(seed + M)
    parts = []

    def add(c, a7, bkt):
        parts.append((np.full(bkt.shape[2], c), np.asarray(a7, F), bkt))
    for n, m in ((M, 2048), (3 * M + 1, 2048), (64, 1024), (4096, 256)):
        add(ORDINARY, *_ordinary(rs, M, m, n))
    a7, bkt = _ordinary(rs, M, 1024, 64)
    k = rs.randint(0, M, 1024)
    bkt[k, :3, np.arange(1024)] *= (10.0 ** rs.uniform(3, 6, (1024, 1))).astype(F)
    add(FIREFLY, a7, bkt)
    for n in (0, 1, 2, 3):
        add(PARTIAL, *_ordinary(rs, M, 256, n))
    a7, bkt = _ordinary(rs, M, 1024, 2 * M)
    bkt[:, 3] = rs.choice(np.array([0.0, -0.0, -1.5, np.nan, np.inf], F), (M, 1024))
    bkt[:, :3, ::2] = rs.choice(np.array([np.nan, np.inf, -np.inf, 0.0, 7.0], F), (M, 3, 512))
    add(UNCOVERED, a7, bkt)
    # ties: t buckets share I exactly, the others hold ordinary sums
    a7, bkt = _ordinary(rs, M, 1024, 2 * M)
    t = 2 + np.arange(1024) % (M - 1)                                            # 2 .. M
    I = (2.0 ** rs.randint(-2, 3, (1024, 3))).astype(F)
    for p in range(1024):
        ks = rs.choice(M, t[p], replace=False)
        w = rs.choice(np.array([0.5, 1.0, 2.0, 4.0], F), t[p])
        bkt[ks, 3, p] = w
        bkt[ks, :3, p] = w[:, None] * I[p][None]
    add(TIES, a7, bkt)
    a7, bkt = _ordinary(rs, M, 512, 2 * M)
    bkt[:, :3] = 0.0
    add(ZERO, a7, bkt)
    a7, bkt = _ordinary(rs, M, 1024, 2 * M)
    neg = rs.uniform(size=(M, 1024)) < 0.4
    neg[rs.randint(0, M, 1024), np.arange(1024)] = True                          # at least one
    neg[:, ::4] = True                                                           # every fourth: all buckets
    bkt[:, :3] = np.where(neg[:, None], -bkt[:, :3], bkt[:, :3])
    add(NEGATIVE, a7, bkt)
    a7, bkt = _ordinary(rs, M, 1024, 2 * M)
    for p in range(1024):
        for k in rs.choice(M, 1 + p % 3, replace=False):
            bkt[k, rs.randint(0, 3), p] = rs.choice(np.array([np.inf, -np.inf, np.nan], F))
    add(NONFINITE, a7, bkt)
    # boundary: M // 2 zero keys, the others green = 2^e w; thirds: exact, one sum an ulp up, one zero key at 2^-50 of the others
    bkt = np.zeros((M, 4, 768), F)
    bkt[:, 3] = rs.choice(np.array([0.5, 1.0, 2.0, 4.0], F), (M, 768))
    e = (2.0 ** rs.randint(-3, 4, 768)).astype(F)
    for p in range(768):
        hi = rs.choice(M, M - M // 2, replace=False)
        bkt[hi, 1, p] = bkt[hi, 3, p] * e[p]
        if p % 3 == 1:
            bkt[hi[0], 1, p] = np.nextafter(bkt[hi[0], 1, p], F(np.inf))
        elif p % 3 == 2:
            lo = np.setdiff1d(np.arange(M), hi)[0]
            bkt[lo, 1, p] = bkt[lo, 3, p] * e[p] * F(2.0 ** -50)
    add(BOUNDARY, np.full(768, 2 * M, F), bkt)
    rest = POOL - sum(p[0].size for p in parts)
    assert rest > 0
    add(ORDINARY, *_ordinary(rs, M, rest, 2 * M))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts], 2)


def classes(FB, seed):
    """class of each pixel by position (see the module docstring)"""
    rs = np.random.RandomState(seed)
    p = np.arange(FB)
    wave, lane = p // 64, p % 64
    c = np.where(wave % 3 == 0, lane % len(ALL), np.where(wave % 3 == 1, ORDINARY, rs.randint(0, len(ALL), FB)))
    return c.astype(np.int64)


def picks(pl, FB, seed=1):
    """(cls (FB,), pick (FB,)): classes(FB, seed) and, per pixel, a seeded draw from the pool's states of its class"""
    pcls = pl[0]
    cls = classes(FB, seed)
    rs = np.random.RandomState(seed + 77)
    pick = np.empty(FB, np.int64)
    for c in np.unique(cls):
        at = np.flatnonzero(cls == c)
        pick[at] = rs.choice(np.flatnonzero(pcls == c), at.size)
    return cls, pick


def state(pl, FB, seed=1):
    """(cls, a7 (FB,), bkt (M, 4, FB)) of FB pixels"""
    cls, pick = picks(pl, FB, seed)
    return cls, np.ascontiguousarray(pl[1][pick]), np.ascontiguousarray(pl[2][:, :, pick])
