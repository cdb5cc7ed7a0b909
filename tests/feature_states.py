"""Synthetic feature buffers and colour states for the tests of the fixed denoiser (csrc/denoise.hpp, cl2_denoise), on the CPU and
on the device, in the style of error_states.py: seeded, every class named and listed in ALL / COLOURS.

features(W, H, seed) -> (cls, normal, depth, albedo, coverage) as Renderer.load_features() takes them, every value finite (the
feature pass never emits another).  cls (H, W) is a BIT MASK: bit k set = the pixel belongs to class k of ALL.

The frame is cut into REGIONS by borders at 48 k + (0, -1, +1)[k % 3] in x and in y -- 47, 97, 144, 191, 241, 288, ...: multiples of the
filter's 16-pixel tile and one pixel to either side of them, the seams of its tiles and of the halo it stages -- and, from 3
pixels up, behind the first and before the last row and column.  Region (i, j) takes kind (3 i + j) % 6:

    SMOOTH        unit normals that turn slowly, depth 3 + a ramp, albedo around 0.5
    CREASE_PERP   the normal of the region is perpendicular to its neighbours'      (w_n = 0 across the border)
    CREASE_OPP    ... opposite to the SMOOTH regions'                               (n_p . n_q < 0)
    DEPTH_STEP    depth 7 times the ramp
    ALBEDO_STEP   albedo (0.9, 0.1, 0.3)
    COV0_BLOCK    the whole region without coverage and all 0, as the feature pass leaves a miss: 47 x 47 pixels and more wherever
                  the frame holds an inner region (at 7 x 5 a region is a few pixels)
    BORDER        (a second bit, on every kind) the region is the first or last row or column

on top of which single pixels are stamped, pixel index p with p % STRIDE == k (STRIDE 11 below 2,000 pixels, else 97):

    ZERO_NORMAL   normal 0 on a covered pixel: every tap's w_n is 0, the weight sum is 0 and the pixel keeps its colour
    COV0_SINGLE   one uncovered pixel (all 0)
    FRACTIONAL    coverage 1/4, 1/2, 3/4 or 1/8
    DEPTH_ZERO    depth 0 on a covered pixel: den_z = 0, the centre tap's 0 / 0 makes the weight sum NaN, the pixel keeps its colour
    DEPTH_HUGE    depth (1 .. 2) x 1e30
    COV0_CHECKER  every second pixel of a patch in the middle of the frame uncovered

A pixel is PASS_THROUGH if the filter must return its input colour byte for byte: coverage 0, a zero normal or depth 0.

colours(cls, pool, seed) -> (ccls, acc): packed accumulators [8][W*H] (Renderer.load_packed_accumulators) whose radiance
scrub(acc[:3] / acc[3]) is the filter's input, one class of COLOURS per pixel:

    C_STATES      a pixel state of error_states (all nine of its classes: weights 0, -0, NaN and inf, NaN / inf sums, subnormal
                  sums, sums that cancel to 0); a negative weight is made positive
    C_WEIGHT0     weight 0 under finite sums: x / 0, scrubbed to 0
    C_NONFINITE   NaN, +inf or -inf in the image rows over weight 1: scrubbed to 0
    C_NEGWEIGHT   a state of error_states with a negative weight: a noisy negative colour, 1 + luma around -1
    C_NEGATIVE    a grey -k with k in 0.5 .. 0.999 and 1.001 .. 3: 1 + luma on either side of 0, x = c / (1 + luma) up to 1e3 either
                  sign; every pixel a k of its own
    C_RANGE       colours 10^u, u uniform in -30 .. 30 per channel: the 25-term sums stay far below float32's largest

The last three are the WILD ones: a huge colour reaches its neighbours through weights like exp(-60), whose relative error is 60 times
that of the exponent, and mixed signs cancel in sum(w c), so around them float32 itself is far from the exact result.  They live in
the right third of the frame only (x >= wild_from(W)); wild_reach() is the part of the frame they can influence in a given number of
passes, and the tests hold the plain tolerance outside it.  No class overflows: sum(w c) <= 25 x 1e30."""
import numpy as np

import error_states as es

F = np.float32
NAMES = ("SMOOTH", "CREASE_PERP", "CREASE_OPP", "DEPTH_STEP", "ALBEDO_STEP", "COV0_BLOCK", "BORDER",
         "ZERO_NORMAL", "COV0_SINGLE", "FRACTIONAL", "DEPTH_ZERO", "DEPTH_HUGE", "COV0_CHECKER")
(SMOOTH, CREASE_PERP, CREASE_OPP, DEPTH_STEP, ALBEDO_STEP, COV0_BLOCK, BORDER,
 ZERO_NORMAL, COV0_SINGLE, FRACTIONAL, DEPTH_ZERO, DEPTH_HUGE, COV0_CHECKER) = ALL = tuple(range(len(NAMES)))
KINDS = (SMOOTH, CREASE_PERP, CREASE_OPP, DEPTH_STEP, ALBEDO_STEP, COV0_BLOCK)
STAMPS = (ZERO_NORMAL, COV0_SINGLE, FRACTIONAL, DEPTH_ZERO, DEPTH_HUGE)
FRAMES = [(7, 5), (41, 25), (512, 513), (1920, 1080)]

C_NAMES = ("C_STATES", "C_WEIGHT0", "C_NONFINITE", "C_NEGWEIGHT", "C_NEGATIVE", "C_RANGE")
C_STATES, C_WEIGHT0, C_NONFINITE, C_NEGWEIGHT, C_NEGATIVE, C_RANGE = COLOURS = tuple(range(len(C_NAMES)))
WILD = (C_NEGWEIGHT, C_NEGATIVE, C_RANGE)


def has(cls, k):
    return (cls >> k) & 1 == 1


def borders(n):
    """region borders along an axis of n pixels: a region starts at each"""
    b = {48 * k + (0, -1, 1)[k % 3] for k in range(1, n // 48 + 2)}
    if n >= 3:
        b |= {1, n - 1}
    return sorted(x for x in b if 0 < x < n)


def _region_index(n):
    idx = np.zeros(n, np.int64)
    for b in borders(n):
        idx[b:] += 1
    return idx


def stride(FB):
    return 11 if FB < 2000 else 97


def features(W, H, seed=1):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    ri, rj = _region_index(H)[:, None], _region_index(W)[None, :]
    kind = ((3 * ri + rj) % 6) + 0 * x
    cls = (1 << kind).astype(np.int64)
    edge = (y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)
    cls |= np.where(edge, 1 << BORDER, 0)

    # SMOOTH base: a unit normal near +y that turns over ~60 pixels, in float32 as normalize() leaves it
    n = np.stack([0.2 * np.sin(x / 60.0), np.ones((H, W)), 0.2 * np.cos(y / 45.0)], -1)
    perp = np.stack([np.ones((H, W)), np.zeros((H, W)), np.zeros((H, W))], -1)
    n = np.where((kind == CREASE_PERP)[..., None], perp, n)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    n = np.where((kind == CREASE_OPP)[..., None], -n, n).astype(F)
    depth = (3.0 + 0.01 * x + 0.02 * y) * np.where(kind == DEPTH_STEP, 7.0, 1.0)
    albedo = 0.5 + 0.1 * np.stack([np.sin(x / 30.0), np.cos(y / 30.0), np.sin((x + y) / 50.0)], -1)
    albedo = np.where((kind == ALBEDO_STEP)[..., None], np.array([0.9, 0.1, 0.3]), albedo)
    cov = np.ones((H, W))

    p = y * W + x
    st = p % stride(W * H)
    for k, c in enumerate(STAMPS):
        cls |= np.where(st == k, 1 << c, 0)
    n = np.where(has(cls, ZERO_NORMAL)[..., None], 0.0, n).astype(F)
    frac = np.array([0.25, 0.5, 0.75, 0.125])[rs.randint(0, 4, (H, W))]
    cov = np.where(has(cls, FRACTIONAL), frac, cov)
    depth = np.where(has(cls, DEPTH_ZERO), 0.0, depth)
    depth = np.where(has(cls, DEPTH_HUGE), 1e30 * (1.0 + rs.uniform(size=(H, W))), depth)
    cx, cy, hw, hh = W // 2, H // 2, max(1, min(10, W // 4)), max(1, min(10, H // 4))
    checker = (abs(x - cx) <= hw) & (abs(y - cy) <= hh) & ((x + y) % 2 == 0)
    cls |= np.where(checker, 1 << COV0_CHECKER, 0)

    uncovered = (kind == COV0_BLOCK) | has(cls, COV0_SINGLE) | checker
    cov = np.where(uncovered, 0.0, cov)
    n = np.where(uncovered[..., None], 0.0, n)
    depth = np.where(uncovered, 0.0, depth)
    albedo = np.where(uncovered[..., None], 0.0, albedo)
    return cls, n.astype(F), depth.astype(F), albedo.astype(F), cov.astype(F)


def twin_outer_columns(normal, depth, albedo, coverage):
    """the same features with those of the first column copied onto the last: the only two columns of a 2049-wide frame that a
    step-2048 tap connects then weigh each other"""
    out = [x.copy() for x in (normal, depth, albedo, coverage)]
    for x in out:
        x[:, -1] = x[:, 0]
    return out


def pass_through(normal, depth, coverage):
    return (coverage == 0) | ~normal.any(axis=-1) | (depth == 0)


def wild_from(W, wild=True):
    return W - max(1, W // 3) if wild else W


def wild_reach(W, H, iterations, wild=True):
    """(H, W) bool: the pixels a WILD colour can have influenced after `iterations` passes (taps reach 2 steps per pass)"""
    x = np.arange(W)[None, :] + np.zeros((H, 1), np.int64)
    return x >= wild_from(W, wild) - 2 * ((1 << iterations) - 1) if wild else x < 0


def colours(cls, pool, seed=1, wild=True):
    """wild=False: no wild zone, the calm classes everywhere"""
    H, W = cls.shape
    FB = W * H
    _, acc, _ = es.state(pool, FB, es.ALL, seed=seed)
    acc = acc.copy()
    rs = np.random.RandomState(seed + 1234)
    p = np.arange(FB)
    yy, xx = p // W, p % W
    x0 = wild_from(W, wild)
    wild = xx >= x0
    ccls = np.full(FB, C_STATES, np.int64)
    neg = acc[3] < 0
    ccls[neg & wild] = C_NEGWEIGHT
    acc[3, neg & ~wild] = -acc[3, neg & ~wild]
    st = (p + 5) % stride(FB)                    # next to the feature stamps, not on them
    for k, c in enumerate((C_WEIGHT0, C_NONFINITE)):
        ccls[(st == k) & ~wild] = c
    st = (np.cumsum(wild) - 1) % (7 if FB < 2000 else 97)        # the wild zone has stamps of every class, however small it is
    for k, c in enumerate((C_WEIGHT0, C_NONFINITE, C_NEGATIVE, C_RANGE, C_NEGWEIGHT)):
        ccls[(st == k) & wild] = c
    ccls[(yy % 9 == 2) & (xx > x0 + W // 6)] = C_RANGE     # whole runs too, so that taps of one class meet
    at = ccls == C_WEIGHT0
    acc[:3, at] = rs.gamma(1.0, 0.5, (3, at.sum())).astype(F)
    acc[3, at] = 0.0
    at = np.flatnonzero(ccls == C_NONFINITE)
    acc[:3, at] = rs.choice(np.array([np.nan, np.inf, -np.inf, 0.5], F), (3, at.size))
    acc[rs.randint(0, 3, at.size), at] = rs.choice(np.array([np.nan, np.inf, -np.inf], F), at.size)
    acc[3, at] = 1.0
    at = np.flatnonzero((ccls == C_NEGWEIGHT) & ~(acc[3] < 0))
    acc[:3, at] = rs.gamma(1.0, 0.5, (3, at.size)).astype(F)
    acc[3, at] = -1.5
    at = np.flatnonzero(ccls == C_NEGATIVE)
    k = np.where(rs.uniform(size=at.size) < 0.5, rs.uniform(0.5, 0.999, at.size), rs.uniform(1.001, 3.0, at.size))
    acc[:3, at] = -k.astype(F)
    acc[3, at] = 1.0
    at = np.flatnonzero(ccls == C_RANGE)
    acc[:3, at] = (10.0 ** rs.uniform(-30, 30, (3, at.size))).astype(F)
    acc[3, at] = 1.0
    return ccls.reshape(H, W), acc


def radiance(acc, W, H):
    """Renderer.radiance / k_denoise_input on the packed accumulators: float32 (H, W, 3)"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c = (acc[:3] / acc[3]).astype(F)
    return np.where(np.isfinite(c), c, F(0)).T.reshape(H, W, 3).copy()


# ---- the tolerance of a comparison with the restatement ----
K = 8       # the allowed multiple of the float32 restatement's own deviation from its float64 companion, see check()


def nerr(a, b):
    """max over the channels of |a - b| / (1e-6 + 1e-4 |b|): <= 1 is assert_allclose(a, b, rtol=1e-4, atol=1e-6)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.abs(a - b) / (1e-6 + 1e-4 * np.abs(b))).max(axis=-1)


def restatements(c, normal, depth, albedo, coverage, sig, passes, wild=True):
    """{k: (want, reach, y, n_ref)} for every pass count k of `passes`: the float32 restatement after k passes, the wild colours'
    reach, and the yardstick of that reach: y = the largest nerr of the float32 restatement against its float64 companion in it,
    n_ref = how many of its pixels have nerr > 1.  The companion is evaluated on the columns from 2 reaches left of the wild zone
    only (what lies further left cannot influence the reach)."""
    import denoise_reference as dr
    H, W = c.shape[:2]
    last = max(passes)
    x0 = max(0, wild_from(W, wild) - 4 * ((1 << last) - 1)) if wild else W
    crop = (slice(None), slice(x0, W))
    c32, c64 = np.asarray(c, F), np.asarray(c, np.float64)[crop]
    g = (normal, depth, albedo, coverage)
    out = {}
    for i in range(last):
        c32 = dr.atrous_pass(c32, *g, i, **sig)
        if x0 < W:
            c64 = dr.atrous_pass(c64, *(a[crop] for a in g), i, dtype=np.float64, **sig)
        if i + 1 in passes:
            reach = wild_reach(W, H, i + 1, wild)
            y, n_ref = 0.0, 0
            if reach.any():
                e = nerr(c32[crop].astype(np.float64), c64)[reach[crop]]
                y, n_ref = float(e.max()), int((e > 1).sum())
            out[i + 1] = (c32, reach, y, n_ref)
    return out


def check(got, want, reach, y, n_ref, label=""):
    """The device's picture `got` against the float32 restatement `want`.  Outside the wild colours' reach: rtol 1e-4, atol 1e-6
    (nerr <= 1), the tolerance of every other comparison of the filter.  Inside it float32 itself is unreliable, and the yardstick
    is what float32 rounding alone does: nerr <= max(1, K y), and at most K n_ref + K pixels with nerr > 1.  K = 8: the device's
    expf and numpy's are each within an ulp of the exact value, so a weight differs by up to 2 ulp where the rounding that
    separates the restatement from its companion is half an ulp per operation (x 4), and the maximum over a zone of a heavy-tailed
    quantity differs between two draws of the rounding errors (x 2).  Returns the figures (calm max, wild max, wild count)."""
    assert np.isfinite(got).all(), label
    e = nerr(got.astype(np.float64), want.astype(np.float64))
    calm = float(e[~reach].max()) if (~reach).any() else 0.0
    wmax = float(e[reach].max()) if reach.any() else 0.0
    n = int((e[reach] > 1).sum())
    print(f"{label}: calm nerr {calm:.3g}; reach {int(reach.sum())} px nerr {wmax:.3g} (yardstick {y:.3g}), over 1: {n} (restatement {n_ref})")
    assert calm <= 1, f"{label}: outside the wild reach nerr {calm}"
    assert wmax <= max(1.0, K * y), f"{label}: in the wild reach nerr {wmax}, yardstick {y}"
    assert n <= K * n_ref + K, f"{label}: {n} pixels of the wild reach over the plain tolerance, the restatement has {n_ref}"
    return calm, wmax, n
