"""numpy statement of the device tone map (csrc/tonemap.hpp: tone_pixel, k_tone_logsum, k_tone_logsum_final, k_tone_apply), every
operation in the order and the type the kernels perform it.  `acc` is the packed accumulator state [8][W*H] float32 of
Renderer.packed_accumulators(): planes b, g, r, w, ub, ug, ur, cnt.  `which`: 0 image, 1 unweighted_image, 2 unidirectional_image.

Given Lw, a byte of the picture is a chain of IEEE float32 / float64 operations and one cast: apply() is held to the device with
no tolerance (tests/test_gpu_tone.py) and to clive2_amd.camera.tone_map byte for byte (tests/test_tone_cpu.py).  The one thing
that is not restated bit for bit is the sum of the log terms: sum_bound() is its derived tolerance, device_sum() the device's
order of additions for the CPU check of that bound, and fragile() the bytes that can move when Lw moves by that much."""
import math

import numpy as np

F = np.float32
D = np.float64
TONE_BLOCKS = 1024                                   # csrc/tonemap.hpp
PICTURES = ("image", "unweighted_image", "unidirectional_image")
U = 2.0 ** -53                                       # unit roundoff of float64


def scrub(x):
    """np.nan_to_num(x, neginf=0, posinf=0) in x's own type: tone_scrub"""
    return np.where(np.isfinite(x), x, x.dtype.type(0))


def pixel(acc, which, exposure):
    """(base, pre), float64 (FB, 3) b, g, r: the picture's value as `image * tone_vector` sees it, and `image * exposure` widened
    (a float32 product for the two float32 pictures, a float64 one for the third): tone_pixel"""
    acc = np.asarray(acc, F).reshape(8, -1)
    with np.errstate(all="ignore"):
        if which == 2:
            cnt = acc[7].astype(D)
            base = scrub(acc[4:7].astype(D) / cnt)
            pre = base * D(exposure)
        else:
            f = scrub((acc[:3] / acc[3]).astype(F) if which == 0 else acc[:3])
            base = f.astype(D)
            pre = (f * F(exposure)).astype(F).astype(D)
    return np.ascontiguousarray(base.T), np.ascontiguousarray(pre.T)


def log_terms(acc, which):
    """log(0.1 + luma) per pixel, float64 (FB,): the addends of k_tone_logsum (NaN where luma < -0.1)"""
    b = pixel(acc, which, 1.0)[0]
    with np.errstate(all="ignore"):
        return np.log(0.1 + ((b[:, 0] * 0.0722 + b[:, 1] * 0.7152) + b[:, 2] * 0.2126))


def to_byte(v):
    """k_tone_apply's cast, written out: truncation toward zero of the values strictly inside (-2^31, 2^31), its low 8 bits (so a
    negative value wraps through the two's complement int32); 0 for everything else, NaN and +-inf included"""
    v = np.asarray(v, D)
    with np.errstate(invalid="ignore"):
        ok = (v > -2147483648.0) & (v < 2147483648.0)
    iv = np.trunc(np.where(ok, v, 0.0)).astype(np.int64)
    return (iv & 0xFF).astype(np.uint8)


def value(acc, which, exposure, white_point, Lw):
    """255 * result / (result + white_point^2), result = pre / Lw: float64 (FB, 3), before the cast"""
    pre = pixel(acc, which, exposure)[1]
    wp2 = D(white_point) * D(white_point)
    with np.errstate(all="ignore"):
        res = pre / D(Lw)
        return 255.0 * res / (res + wp2)


def apply(acc, which, exposure, white_point, Lw):
    """the picture k_tone_apply writes: uint8 (FB, 3)"""
    return to_byte(value(acc, which, exposure, white_point, Lw))


def log_average(log_sum, FB):
    """Lw as Renderer.tone_mapped() forms it from the device's sum (numpy's exp)"""
    with np.errstate(all="ignore"):
        return np.exp(D(log_sum) / FB)


# ---------------------------------------------------------------- the sum
def _grid(FB):
    return min((FB + 255) // 256, TONE_BLOCKS)


def sum_depth(FB):
    """The largest number of float64 additions a term goes through on the device, read off the kernels: k_tone_logsum adds
    ceil(FB / (grid * 256)) terms per thread one after another, then 6 shuffle levels (64 lanes) and 2 levels over the four
    waves of the workgroup; k_tone_logsum_final does the same with ceil(grid / 256) partials per thread."""
    grid = _grid(FB)
    return -(-FB // (grid * 256)) + 6 + 2 + -(-grid // 256) + 6 + 2


def sum_bound(terms, FB):
    """|device sum - exact sum of the reference's terms| <= (sum_depth + 4) * 2^-53 * sum|terms|, to first order.

    A sum of float64 numbers in which no addend passes through more than d additions is within d u sum|t| of the exact one
    (u = 2^-53; Higham, Accuracy and Stability of Numerical Algorithms, 4.2).  The device's terms are not the reference's: each
    is the device's `log` of the same float64 argument (the argument itself is restated bit for bit; the library is built with
    -ffp-contract=off).  HIP's table of device math functions gives 1 ulp for the double precision `log` (HIP programming guide,
    "HIP math API", double precision mathematical functions; the ROCm installation this was written against carries no copy of
    that table, so the figure is the published one), and 1 ulp is what glibc states for the `log` numpy calls: the two differ by
    at most 2 ulp = 4 u relative, the `+ 4`.  Derived, not measured; test_tone_cpu.py checks that numpy's own sum and the
    restated device order (device_sum) stay inside it."""
    t = np.asarray(terms, D)
    return (sum_depth(FB) + 4) * U * float(np.abs(t).sum())


def exact_sum(terms):
    """math.fsum, NaN and inf propagated as a float64 sum would (fsum raises on inf - inf and on intermediate overflow)"""
    t = np.asarray(terms, D)
    if not np.isfinite(t).all():
        with np.errstate(all="ignore"):
            return float(t.sum())
    return math.fsum(t.tolist())


def _workgroup_sums(per_thread):
    """(n, 256) per-thread sums -> (n,): the __shfl_down tree of each wave of 64 (lane 0's value), then (w0 + w1) + (w2 + w3)"""
    s = per_thread.reshape(-1, 4, 64)
    off = 32
    while off:
        s = s[:, :, :off] + s[:, :, off:2 * off]
        off >>= 1
    s = s[:, :, 0]
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


def _strided(x, threads):
    """per-thread sums of x (n,) over `threads` threads, thread t adding x[t], x[t + threads], ... in that order from 0.0"""
    rows = -(-x.size // threads)
    pad = np.zeros(rows * threads, D)                # x + 0.0 is x: the padding adds nothing
    pad[:x.size] = x
    s = np.zeros(threads, D)
    for row in pad.reshape(rows, threads):
        s = s + row
    return s


def device_sum(terms):
    """the sum in the device's order: k_tone_logsum over _grid(FB) workgroups, then k_tone_logsum_final over the partials"""
    t = np.asarray(terms, D)
    grid = _grid(t.size)
    with np.errstate(all="ignore"):
        partial = _workgroup_sums(_strided(t, grid * 256).reshape(grid, 256))
        return float(_workgroup_sums(_strided(partial, 256).reshape(1, 256))[0])


# ---------------------------------------------------------------- which bytes may move with Lw
def fragile(acc, which, exposure, white_point, Lw, eps):
    """bool (FB, 3): the bytes whose cast changes when v = 255 x / (x + w^2) is scaled by 1 +- (2 eps + 2^-50), eps the relative
    uncertainty of Lw (sum_bound / FB: Lw = exp(sum / FB)).  For x >= 0 the relative change of v is at most that of x, which is
    that of Lw and of one more rounded division; 2 eps + 2^-50 covers them and numpy's exp of the two nearby arguments.  These
    are the only bytes on which the device's picture and the host's may disagree.  A saturated pixel (x > 2^53: x + w^2 == x,
    v = fl(255 x) / x, which is 255 or the double below it) is fragile."""
    v = value(acc, which, exposure, white_point, Lw)
    d = 2.0 * eps + 2.0 ** -50
    with np.errstate(all="ignore"):
        lo, hi = v * (1.0 - d), v * (1.0 + d)
    b = to_byte(v)
    return (to_byte(lo) != b) | (to_byte(hi) != b)


# ---------------------------------------------------------------- the host path on a packed state
def host_picture(acc, which, W, H):
    """the picture the Renderer property hands camera.tone_map, built from a packed state as clive2_amd/renderer.py builds it from
    read_accumulators(): float32 (H, W, 3) for `image` and `unweighted_image`, float64 for `unidirectional_image` (float32 / int32)"""
    acc = np.asarray(acc, F).reshape(8, -1)
    img = np.ascontiguousarray(acc[:3].T).reshape(H, W, 3)
    wts = acc[3].reshape(H, W, 1)
    uni = np.ascontiguousarray(acc[4:7].T).reshape(H, W, 3)
    cnt = np.rint(acc[7]).astype(np.int32).reshape(H, W, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        pic = (img / wts, img, uni / cnt)[which]
        return np.nan_to_num(pic, neginf=0, posinf=0)


def host_log_average(picture):
    """Lw as camera.tone_map computes it"""
    with np.errstate(all="ignore"):
        luma = (picture * np.array([0.0722, 0.7152, 0.2126])).sum(axis=2)
        return np.exp(np.log(0.1 + luma).sum() / (picture.shape[0] * picture.shape[1]))
