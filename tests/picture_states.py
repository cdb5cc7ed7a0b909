"""Synthetic kept pictures for the tests of the device tone map of a kept picture (csrc/tonemap_picture.hpp), on the CPU and on the
device.

A STATE is a picture (FB, 3) float32 b, g, r as Renderer.load_picture() takes it.  Its pixels are drawn from a pool of pixel states,
one class per pixel.  tests/tone_states.py defines its classes for the picture's value f = v / w; here the pixel itself is f, and
there is no scrub between it and the tone map:

    ORDINARY   gamma colours
    BLACK      0, 0, 0 (the log term is log(0.1))
    NONFINITE  NaN, +inf or -inf in one to three channels: the log term is NaN (or +inf), the bytes 0
    TINY       float32 subnormals (f and f * exposure subnormal)
    OVERFLOW   f in 1.8e38 .. 3.3e38: the float32 product f * exposure is +inf at exposure 2 and 4, inf / inf = NaN, byte 0
    SATURATED  f in 1e24 .. 1e30: result > 2^53, result + w^2 == result, so the byte is 254 or 255 by the last bits of the quotient
    NEGATIVE   one channel, or all three, in -0.09 .. -0.001: luma >= -0.09, the log argument stays >= 0.01; v is negative and wraps
    POLE       f = -0.25 exactly in all channels: with exposure 4, Lw = 1, white point 1 result + w^2 is exactly 0 and v is -inf.
               Its luma is -0.25, so its log term is NaN

ORDINARY_ONLY = (ORDINARY, BLACK); FINITE = every class but NONFINITE and POLE (the log sum is finite, every term counts); ALL =
every class.  Class by position, as tests/tone_states.py lays its states out: in every third wave-sized run of pixels the classes
cycle through the lanes (every class in the wave), the next run is ORDINARY only, the third is a seeded draw.

The picture's bytes are a function of the pixel alone (given Lw), so a frame's reference is the pool's, gathered by `pick`."""
import numpy as np

F = np.float32
ORDINARY, BLACK, NONFINITE, TINY, OVERFLOW, SATURATED, NEGATIVE, POLE = range(8)
NAMES = ("ordinary", "black", "nonfinite", "tiny", "overflow", "saturated", "negative", "pole")
ORDINARY_ONLY = (ORDINARY, BLACK)
FINITE = (ORDINARY, BLACK, TINY, OVERFLOW, SATURATED, NEGATIVE)
ALL = tuple(range(8))
KINDS = {"ordinary": ORDINARY_ONLY, "finite": FINITE, "all": ALL}
SIZES = [(1, 1), (7, 1), (257, 1), (91, 60), (512, 512), (513, 512)]
POOL = 1 << 16


def _ordinary(rs, m):
    return rs.gamma(1.0, 0.5, (m, 3)).astype(F)


def pool(seed=20241018):
    """(cls (POOL,), pic (POOL, 3) float32): the pixel states the frames are filled from"""
    rs = np.random.RandomState(seed)
    parts = []

    def add(c, pic):
        parts.append((np.full(len(pic), c), np.asarray(pic, F)))
    add(BLACK, np.zeros((64, 3), F))
    pic = _ordinary(rs, 4096)
    for p in range(4096):                              # one to three channels
        for c in rs.choice(3, 1 + p % 3, replace=False):
            pic[p, c] = rs.choice(np.array([np.nan, np.inf, -np.inf], F))
    add(NONFINITE, pic)
    add(TINY, rs.randint(1, 1 << 20, (4096, 3)).astype(np.uint32).view(F))
    add(OVERFLOW, rs.uniform(1.8e38, 3.3e38, (4096, 3)))
    add(SATURATED, 10.0 ** rs.uniform(24, 30, (4096, 3)))
    x = rs.gamma(1.0, 0.5, (4096, 3))
    neg = -rs.uniform(0.001, 0.09, (4096, 3))
    one = rs.randint(0, 3, 4096)[:, None] == np.arange(3)[None]
    one[::2] = True                                    # every second: all channels
    add(NEGATIVE, np.where(one, neg, x))
    add(POLE, np.full((64, 3), -0.25, F))
    rest = POOL - sum(len(p[0]) for p in parts)
    assert rest > 0
    add(ORDINARY, _ordinary(rs, rest))
    return np.concatenate([p[0] for p in parts]), np.ascontiguousarray(np.concatenate([p[1] for p in parts]))


def classes(FB, seed):
    """class of each pixel by position (see the module docstring), all eight classes"""
    rs = np.random.RandomState(seed)
    p = np.arange(FB)
    wave, lane = p // 64, p % 64
    c = np.where(wave % 3 == 0, lane % len(ALL), np.where(wave % 3 == 1, ORDINARY, rs.randint(0, len(ALL), FB)))
    return c.astype(np.int64)


def state(pl, FB, allowed, seed=1):
    """(cls, pick, pic) of FB pixels: classes(FB, seed) with every class outside `allowed` replaced by ORDINARY, each pixel a seeded
    draw `pick` from the pool's states of its class"""
    pcls, ppic = pl
    cls = classes(FB, seed)
    cls = np.where(np.isin(cls, allowed), cls, ORDINARY)
    rs = np.random.RandomState(seed + 77)
    pick = np.empty(FB, np.int64)
    for c in np.unique(cls):
        at = np.flatnonzero(cls == c)
        pick[at] = rs.choice(np.flatnonzero(pcls == c), at.size)
    return cls, pick, np.ascontiguousarray(ppic[pick])


def poison_positions(FB):
    """where the poisoned pixel goes: first, last, and the first pixel of the second grid-stride iteration where there is one"""
    return sorted({0, FB - 1} | ({262144} if FB > 262144 else set()))


def poisoned(pic, p):
    """a copy of pic with pixel p at luma -1: log(0.1 + luma) is NaN, and so is the sum if p is counted"""
    pic = pic.copy()
    pic[p] = -1.0
    return pic
