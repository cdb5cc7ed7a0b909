"""numpy statement of the device tone map of a kept picture (csrc/tonemap_picture.hpp: k_picture_logsum, k_picture_apply), every
operation in the order and the type the kernels perform it.  `pic` is the kept picture, float32 (FB, 3) b, g, r (any shape that
reshapes to it): what Renderer.load_picture() takes and Renderer.kept_picture() returns.

It is tests/tone_reference.py's statement for picture 0 with the pixel itself in the place of v / w and WITHOUT the scrub: the host
path of these pictures, camera.tone_map(picture), has none.  The cast, the sum's order, its derived tolerance and Lw are that
module's, imported."""
import numpy as np

from tone_reference import to_byte, exact_sum, device_sum, sum_bound, log_average      # noqa: F401  (re-exported for the tests)

F = np.float32
D = np.float64


def pixel(pic, exposure):
    """(base, pre), float64 (FB, 3): the picture's value widened, and the float32 product `picture * exposure` widened"""
    f = np.asarray(pic, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return f.astype(D), (f * F(exposure)).astype(F).astype(D)


def terms(pic):
    """log(0.1 + luma) per pixel, float64 (FB,): the addends of k_picture_logsum (NaN for a NaN pixel and where luma < -0.1)"""
    b = pixel(pic, 1.0)[0]
    with np.errstate(all="ignore"):
        return np.log(0.1 + ((b[:, 0] * 0.0722 + b[:, 1] * 0.7152) + b[:, 2] * 0.2126))


def value(pic, exposure, white_point, Lw):
    """255 * result / (result + white_point^2), result = pre / Lw: float64 (FB, 3), before the cast"""
    pre = pixel(pic, exposure)[1]
    wp2 = D(white_point) * D(white_point)
    with np.errstate(all="ignore"):
        res = pre / D(Lw)
        return 255.0 * res / (res + wp2)


def apply(pic, exposure, white_point, Lw):
    """the picture k_picture_apply writes: uint8 (FB, 3)"""
    return to_byte(value(pic, exposure, white_point, Lw))


def fragile(pic, exposure, white_point, Lw, eps):
    """bool (FB, 3): the bytes whose cast changes when v is scaled by 1 +- (2 eps + 2^-50), eps the relative uncertainty of Lw
    (sum_bound / FB): tone_reference.fragile for a kept picture, the only bytes on which the device and the host may disagree"""
    v = value(pic, exposure, white_point, Lw)
    d = 2.0 * eps + 2.0 ** -50
    with np.errstate(all="ignore"):
        lo, hi = v * (1.0 - d), v * (1.0 + d)
    b = to_byte(v)
    return (to_byte(lo) != b) | (to_byte(hi) != b)


def host_log_average(pic, W, H):
    """Lw as camera.tone_map computes it from the (H, W, 3) float32 picture"""
    p = np.asarray(pic, F).reshape(H, W, 3)
    with np.errstate(all="ignore"):
        luma = (p * np.array([0.0722, 0.7152, 0.2126])).sum(axis=2)
        return np.exp(np.log(0.1 + luma).sum() / (H * W))
