"""Synthetic accumulator states for the tests of the device tone map (csrc/tonemap.hpp), on the CPU and on the device.

A STATE is acc [8][FB] float32 as Renderer.load_packed_accumulators() takes it: planes b, g, r, w, ub, ug, ur, cnt.  Its pixels are
drawn from a pool of pixel states, one class per pixel (f is the picture's value: v / w, v, or u / cnt):

    ORDINARY   gamma colour sums times positive weights, counts 1 .. 300; independent draws for the three pictures
    BLACK      all colour sums 0 (the log term is log(0.1))
    UNCOVERED  w in {0, -0.0} and cnt = 0, colour sums zero (0 / 0) or not (x / 0)
    NONFINITE  NaN, +inf or -inf in one to three colour sums; or w in {NaN, +inf} over ordinary colour sums
    TINY       colour sums float32 subnormals over w = cnt = 1 (f and f * exposure subnormal), or over a subnormal w
    OVERFLOW   f in 1.8e38 .. 3.3e38: the float32 product f * exposure is +inf at exposure 2 and 4, so the two float32 pictures give
               inf / inf = NaN, byte 0; the float64 third picture stays finite
    SATURATED  colour sums in 1e24 .. 1e30 over w and cnt in {1, 3, 7}: result > 2^53, result + w^2 == result, so the byte is 254 or
               255 by the last bits of the quotient -- of a float32 division in the first picture, a float64 one in the third
    NEGATIVE   one channel, or all three, in -0.09 .. -0.001 (w = cnt = 1, so all three pictures see them): luma >= -0.09, the log
               argument stays >= 0.01; v is negative and wraps through int32
    POLE       f = -0.25 exactly in all channels: with exposure 4, Lw = 1, white point 1 result + w^2 is exactly 0 and v is -inf.
               Its luma is -0.25, so its log term is NaN: a state that holds one has a NaN log sum

ORDINARY_ONLY = (ORDINARY, BLACK); FINITE = every class but POLE (the log sum is finite, every term counts); ALL = every class.
Class by position, as tests/error_states.py lays its states out: in every third wave-sized run of pixels the classes cycle through
the lanes (every class in the wave), the next run is ORDINARY only, the third is a seeded draw.

The picture is a function of the pixel alone (given Lw), so a frame's reference is the pool's, gathered by `pick`."""
import numpy as np

F = np.float32
ORDINARY, BLACK, UNCOVERED, NONFINITE, TINY, OVERFLOW, SATURATED, NEGATIVE, POLE = range(9)
NAMES = ("ordinary", "black", "uncovered", "nonfinite", "tiny", "overflow", "saturated", "negative", "pole")
ORDINARY_ONLY = (ORDINARY, BLACK)
FINITE = tuple(range(8))
ALL = tuple(range(9))
SIZES = [(1, 1), (7, 1), (257, 1), (91, 60), (512, 512), (513, 512), (1920, 1080)]
DROP_POSITIONS = (0, 63, 64, 255, 256, 262143, 262144, -1)
POOL = 1 << 18


def _ordinary(rs, m):
    acc = np.empty((8, m), F)
    cnt = rs.randint(1, 301, m)
    acc[3] = cnt * rs.uniform(0.5, 2.0, m)
    acc[:3] = rs.gamma(1.0, 0.5, (3, m)) * acc[3]
    acc[4:7] = rs.gamma(1.0, 0.5, (3, m)) * cnt
    acc[7] = cnt
    return acc


def _unit(m):
    """w = cnt = 1: every picture's value is the colour sum itself"""
    acc = np.zeros((8, m), F)
    acc[3] = acc[7] = 1.0
    return acc


def pool(seed=20241018):
    """(cls (POOL,), acc [8][POOL]): the pixel states the frames are filled from"""
    rs = np.random.RandomState(seed)
    parts = []

    def add(c, acc):
        parts.append((np.full(acc.shape[1], c), acc))
    acc = _ordinary(rs, 4096)
    acc[:3] = 0.0; acc[4:7] = 0.0
    add(BLACK, acc)
    acc = _ordinary(rs, 4096)
    acc[3] = np.tile(np.array([0.0, -0.0], F), 2048)
    acc[7] = 0.0
    acc[:3, ::4] = 0.0; acc[4:7, ::4] = 0.0          # 0 / 0 in every fourth, x / 0 in the others
    add(UNCOVERED, acc)
    acc = _ordinary(rs, 4096)
    for p in range(3072):                             # one to three colour sums of both colour triples
        for c in rs.choice(3, 1 + p % 3, replace=False):
            acc[c, p] = rs.choice(np.array([np.nan, np.inf, -np.inf], F))
            acc[4 + c, p] = rs.choice(np.array([np.nan, np.inf, -np.inf], F))
    acc[3, 3072:] = np.tile(np.array([np.nan, np.inf], F), 512)
    add(NONFINITE, acc)
    acc = _unit(4096)
    acc[:3] = rs.randint(1, 1 << 20, (3, 4096)).astype(np.uint32).view(F)
    acc[4:7] = rs.randint(1, 1 << 20, (3, 4096)).astype(np.uint32).view(F)
    acc[3, ::2] = rs.randint(1, 1 << 20, 2048).astype(np.uint32).view(F)
    add(TINY, acc)
    acc = _unit(4096)
    acc[:3] = rs.uniform(1.8e38, 3.3e38, (3, 4096))
    acc[4:7] = rs.uniform(1.8e38, 3.3e38, (3, 4096))
    add(OVERFLOW, acc)
    acc = _unit(4096)
    acc[:3] = 10.0 ** rs.uniform(24, 30, (3, 4096))
    acc[4:7] = 10.0 ** rs.uniform(24, 30, (3, 4096))
    acc[3] = rs.choice(np.array([1, 3, 7], F), 4096)
    acc[7] = rs.choice(np.array([1, 3, 7], F), 4096)
    add(SATURATED, acc)
    acc = _unit(4096)
    for rows in (slice(0, 3), slice(4, 7)):
        x = rs.gamma(1.0, 0.5, (3, 4096))
        neg = -rs.uniform(0.001, 0.09, (3, 4096))
        one = rs.randint(0, 3, 4096)[None] == np.arange(3)[:, None]
        one[:, ::2] = True                           # every second: all channels
        acc[rows] = np.where(one, neg, x)
    add(NEGATIVE, acc)
    acc = _unit(256)
    acc[:3] = -0.25; acc[4:7] = -0.25
    add(POLE, acc)
    rest = POOL - sum(p[0].size for p in parts)
    assert rest > 0
    add(ORDINARY, _ordinary(rs, rest))
    return np.concatenate([p[0] for p in parts]), np.ascontiguousarray(np.concatenate([p[1] for p in parts], 1))


def classes(FB, seed):
    """class of each pixel by position (see the module docstring), all nine classes"""
    rs = np.random.RandomState(seed)
    p = np.arange(FB)
    wave, lane = p // 64, p % 64
    c = np.where(wave % 3 == 0, lane % len(ALL), np.where(wave % 3 == 1, ORDINARY, rs.randint(0, len(ALL), FB)))
    return c.astype(np.int64)


def state(pl, FB, allowed, seed=1):
    """(cls, pick, acc) of FB pixels: classes(FB, seed) with every class outside `allowed` replaced by ORDINARY, each pixel a seeded
    draw `pick` from the pool's states of its class"""
    pcls, pacc = pl
    cls = classes(FB, seed)
    cls = np.where(np.isin(cls, allowed), cls, ORDINARY)
    rs = np.random.RandomState(seed + 77)
    pick = np.empty(FB, np.int64)
    for c in np.unique(cls):
        at = np.flatnonzero(cls == c)
        pick[at] = rs.choice(np.flatnonzero(pcls == c), at.size)
    return cls, pick, np.ascontiguousarray(pacc[:, pick])


def poison_positions(FB):
    """where the poisoned pixel goes: first, last, and the first pixel of the second grid-stride iteration where there is one"""
    return sorted({0, FB - 1} | ({262144} if FB > 262144 else set()))


def poisoned(acc, p):
    """a copy of acc with pixel p at luma -1 in all three pictures: log(0.1 + luma) is NaN, and so is the sum if p is counted"""
    acc = acc.copy()
    acc[:, p] = np.array([-1, -1, -1, 1, -1, -1, -1, 1], F)
    return acc


def drop_positions(FB):
    return sorted({p % FB for p in DROP_POSITIONS if -FB <= p < FB})
