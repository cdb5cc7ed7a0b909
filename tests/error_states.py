"""Synthetic accumulator / moment states and addend sequences for the tests of the error estimate (csrc/error_estimate.hpp) and of
the density derived from it (csrc/adaptive.hpp), on the CPU and on the device.

A STATE is a pair acc, mom [8][FB] float32 as Renderer.load_packed_accumulators() / load_moments() take them.  Its pixels are
drawn from a pool of pixel states, one class per pixel:

    ORDINARY   n in {2, 3, 8, 64, 4096} addends (gamma colours, uniform weights) through add_moments
    UNCOVERED  Wt = 0, -0.0, negative, NaN or +inf; n >= 2; moments arbitrary, NaN and inf included (they must not be read)
    EXACT      exactly noiseless: x = I w with I a power of two and w a multiple of 1/8, so every colour's S is exactly 0
    NEAR       nearly noiseless: relative spread 1e-6 around I = 0.3, 1.7, 40; S cancels to rounding size, either sign
    TINY       Wt, the colour sums and the moments float32 subnormals
    SIGNED     addends in pairs (x, w), (-x, w): the colour sums are exactly 0, y^2 > 0, so L = 0 and var_L > 0
    LARGE      moments near 1e37 with Wt near 1e-21: sqrt(var) exceeds float32
    OVERFLOW   moment sums that overflowed to +inf: S = inf - inf (NaN, clamped to 0), S = +inf, I^2 m_3 = 0 * inf
    FEW        n = 0 or n = 1 with Wt > 0 (the n = 1 ones exactly noiseless: with the n < 2 test gone their S * scale is 0 * inf)

BASE = the well-scaled classes (the frame metric is finite at every floor and no single term swamps the sum, so a bitwise
comparison of the sum sees every pixel); NO_FEW adds the classes whose terms are huge or infinite but not n < 2; ALL adds the
rest.  Class by position: in every third wave-sized run of pixels the classes cycle through the lanes (every class in the wave),
the next run is ORDINARY only, the third is a seeded draw."""
import numpy as np

import error_reference as er

F = np.float32
ORDINARY, UNCOVERED, EXACT, NEAR, TINY, SIGNED, LARGE, OVERFLOW, FEW = range(9)
BASE = (ORDINARY, UNCOVERED, EXACT, NEAR)
NO_FEW = BASE + (TINY, SIGNED, LARGE)
ALL = NO_FEW + (OVERFLOW, FEW)
FRAMES = [(7, 5), (41, 25), (512, 512), (512, 513), (1920, 1080)]
POOL = 65536


def _accumulate(xs_ws, m):
    acc, mom = np.zeros((8, m), F), np.zeros((8, m), F)
    for x, w in xs_ws:
        acc[:3] = (acc[:3] + x.T).astype(F)
        acc[3] = (acc[3] + w).astype(F)
        acc[7] = (acc[7] + F(1)).astype(F)
        er.add_moments(mom, x, w)
    return acc, mom


def _ordinary(rs, m, n):
    return _accumulate(((rs.gamma(1.0, 0.5, (m, 3)).astype(F), rs.uniform(0.5, 2.0, m).astype(F)) for _ in range(n)), m)


def _exact(rs, m, n):
    I = (2.0 ** rs.randint(-2, 3, (m, 3))).astype(F)

    def one():
        w = (rs.randint(4, 17, m) / 8.0).astype(F)
        return (I * w[:, None]).astype(F), w
    return _accumulate((one() for _ in range(n)), m)


def _near(rs, m, n):
    I = rs.choice([0.3, 1.7, 40.0], (m, 1))

    def one():
        w = rs.uniform(0.5, 2.0, m)
        return (w[:, None] * I * (1.0 + 1e-6 * rs.standard_normal((m, 3)))).astype(F), w.astype(F)
    return _accumulate((one() for _ in range(n)), m)


def _signed(rs, m, pairs):
    seq = []
    for _ in range(pairs):
        x, w = rs.gamma(1.0, 0.5, (m, 3)).astype(F), rs.uniform(0.5, 2.0, m).astype(F)
        seq += [(x, w), (-x, w)]
    return _accumulate(seq, m)


def pool(seed=20241016):
    """(cls (POOL,), acc [8][POOL], mom [8][POOL]): the pixel states the frames are filled from"""
    rs = np.random.RandomState(seed)
    parts = []

    def add(c, acc, mom):
        parts.append((np.full(acc.shape[1], c), acc, mom))
    for n, m in ((2, 10240), (3, 10240), (8, 10240), (64, 8192), (4096, 2048)):
        add(ORDINARY, *_ordinary(rs, m, n))
    # uncovered: real states whose weight sum is overwritten; every fourth with arbitrary moments
    acc, mom = _ordinary(rs, 4000, 8)
    acc[3] = np.tile(np.array([0.0, -0.0, -1.5, np.nan, np.inf], F), 800)
    mom[:, ::4] = rs.choice(np.array([np.nan, np.inf, -np.inf, 1e30, -3.0], F), (8, 1000))
    acc[:3, 1::4] = rs.choice(np.array([np.nan, np.inf, 0.0, 7.0], F), (3, 1000))
    add(UNCOVERED, acc, mom)
    for n in (2, 8, 64):
        add(EXACT, *_exact(rs, 1000, n))
    for n in (8, 64):
        add(NEAR, *_near(rs, 2000, n))
    # tiny: subnormal sums (bit patterns 1 .. 2^20 as float32), n = 8
    acc, mom = np.zeros((8, 2000), F), np.zeros((8, 2000), F)
    acc[:4] = rs.randint(1, 1 << 20, (4, 2000)).astype(np.uint32).view(F)
    mom[:] = rs.randint(1, 1 << 20, (8, 2000)).astype(np.uint32).view(F)
    acc[7] = 8
    add(TINY, acc, mom)
    for pairs in (1, 2):
        add(SIGNED, *_signed(rs, 1000, pairs))
    acc, mom = np.zeros((8, 2000), F), np.zeros((8, 2000), F)
    acc[:4] = (rs.uniform(0.5, 2.0, (4, 2000)) * 1e-21).astype(F)
    mom[:] = (rs.uniform(0.5, 2.0, (8, 2000)) * 1e37).astype(F)
    mom[4:7] = (rs.uniform(0.5, 2.0, (3, 2000)) * 1e10).astype(F)
    acc[7] = 8
    add(LARGE, acc, mom)
    acc, mom = _ordinary(rs, 1500, 8)
    mom[0] = np.inf; mom[4] = np.inf                 # b: inf - inf
    mom[1] = np.inf                                  # g: +inf
    mom[7, ::2] = np.inf                             # luma: +inf in every second one
    mom[3, ::3] = np.inf; acc[2, ::3] = 0.0          # r of every third: I = 0, I^2 m_3 = 0 * inf
    add(OVERFLOW, acc, mom)
    acc, mom = _exact(rs, 1000, 1)
    acc[7, ::2] = 0.0
    add(FEW, acc, mom)
    # fill the pool up with ordinary states
    rest = POOL - sum(p[1].shape[1] for p in parts)
    assert rest > 0
    add(ORDINARY, *_ordinary(rs, rest, 8))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts], 1), np.concatenate([p[2] for p in parts], 1)


def classes(FB, seed):
    """class of each pixel by position (see the module docstring), all nine classes"""
    rs = np.random.RandomState(seed)
    p = np.arange(FB)
    wave, lane = p // 64, p % 64
    c = np.where(wave % 3 == 0, lane % len(ALL), np.where(wave % 3 == 1, ORDINARY, rs.randint(0, len(ALL), FB)))
    return c.astype(np.int64)


def state(pl, FB, allowed, seed=1):
    """(cls, acc, mom) of FB pixels: classes(FB, seed) with every class outside `allowed` replaced by ORDINARY, each pixel a
    seeded draw from the pool's states of its class"""
    pcls, pacc, pmom = pl
    cls = classes(FB, seed)
    cls = np.where(np.isin(cls, allowed), cls, ORDINARY)
    rs = np.random.RandomState(seed + 77)
    pick = np.empty(FB, np.int64)
    for c in np.unique(cls):
        at = np.flatnonzero(cls == c)
        pick[at] = rs.choice(np.flatnonzero(pcls == c), at.size)
    return cls, np.ascontiguousarray(pacc[:, pick]), np.ascontiguousarray(pmom[:, pick])


def few_pixel(pl):
    """one FEW pixel state (acc (8,), mom (8,)): n = 1, exactly noiseless"""
    pcls, pacc, pmom = pl
    k = np.flatnonzero((pcls == FEW) & (pacc[7] == 1))[0]
    return pacc[:, k].copy(), pmom[:, k].copy()


# ---- addend sequences for the estimator against the residual sum of squares ----
REGIMES = ("gamma", "near", "exact", "signed", "fireflies")


def addend_sequence(regime, P, n, seed):
    """n addends of P pixels: lists xs [(P, 3)], ws [(P,)] float32"""
    rs = np.random.RandomState(seed)
    xs, ws = [], []
    I = rs.choice([0.3, 1.7, 40.0], (P, 1))
    Ip = (2.0 ** rs.randint(-2, 3, (P, 3)))
    for _ in range(n):
        w = rs.uniform(0.5, 2.0, P)
        if regime == "gamma":
            x = rs.gamma(1.0, 0.5, (P, 3))
        elif regime == "near":
            x = w[:, None] * I * (1.0 + 1e-6 * rs.standard_normal((P, 3)))
        elif regime == "exact":
            w = rs.randint(4, 17, P) / 8.0
            x = Ip * w[:, None]
        elif regime == "signed":
            x = rs.standard_normal((P, 3)) * rs.gamma(1.0, 0.5, (P, 1))
        elif regime == "fireflies":
            x = rs.gamma(1.0, 0.5, (P, 3)) * np.where(rs.uniform(size=(P, 1)) < 0.01, 1e4, 1.0)
        else:
            raise ValueError(regime)
        xs.append(x.astype(F))
        ws.append(w.astype(F))
    return xs, ws


def accumulate(xs, ws):
    """acc, mom [8][P] float32 of the sequence, one float32 add per addend and row"""
    return _accumulate(zip(xs, ws), len(ws[0]))
