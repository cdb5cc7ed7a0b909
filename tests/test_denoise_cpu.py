"""The denoiser's specification (tests/denoise_reference.py, the numpy statement csrc/denoise.hpp is checked against on the
GPU): properties that follow from it, on synthetic guide buffers.  No GPU."""
import numpy as np

import denoise_reference as dr

F = np.float32


def _flat_features(H, W, depth=3.0):
    n = np.zeros((H, W, 3), F)
    n[..., 1] = 1
    return n, np.full((H, W), depth, F), np.full((H, W, 3), 0.5, F), np.ones((H, W), F)


def _noisy(H, W, seed=0):
    return np.random.RandomState(seed).gamma(1.0, 0.3, size=(H, W, 3)).astype(F)


def test_zero_iterations_is_identity():
    c = _noisy(20, 24)
    out = dr.denoise(c, *_flat_features(20, 24), iterations=0)
    assert out.dtype == F and out.tobytes() == c.tobytes()


def test_constant_image_is_a_fixed_point():
    H, W = 37, 45                                   # not a multiple of any step: taps fall off every edge
    c = np.empty((H, W, 3), F)
    c[...] = np.array([0.25, 0.5, 0.125], F)        # exact binary fractions: sum(w c) / sum(w) returns c to the last bit or so
    n, z, a, cov = _flat_features(H, W)
    z = z + np.linspace(0, 1, W, dtype=F)[None, :]  # guides that vary do not matter for a constant colour
    out = dr.denoise(c, n, z, a, cov, iterations=5)
    np.testing.assert_allclose(out, c, rtol=2e-6, atol=0)


def test_it_smooths():
    H, W = 32, 32
    c = _noisy(H, W)
    out = dr.denoise(c, *_flat_features(H, W), iterations=3, sigma_color=100.0)
    assert out.std() < 0.5 * c.std()
    assert abs(out.mean() - c.mean()) < 0.05 * c.mean()


def test_uncovered_pixels_pass_through_and_are_not_taps():
    H, W = 24, 24
    c = _noisy(H, W, 1)
    n, z, a, cov = _flat_features(H, W)
    cov[:, :8] = 0                                  # a band of background
    c[:, :8] = 1000.0                               # ... far brighter than the rest: would leak if it were tapped
    out = dr.denoise(c, n, z, a, cov, iterations=4, sigma_color=1e3)
    assert out[:, :8].tobytes() == c[:, :8].tobytes()
    assert out[:, 8:].max() < 10.0


def test_colour_does_not_cross_a_crease():
    """Two regions whose normals are perpendicular: w_n = 0 between them, so every output pixel is a weighted mean of its own
    region's colours only (here: a constant per region), whatever the other sigmas."""
    H, W = 30, 40
    n = np.zeros((H, W, 3), F)
    n[:, :17, 0] = 1                                # left wall faces +x
    n[:, 17:, 1] = 1                                # floor faces +y
    z = np.full((H, W), 2.0, F)
    a = np.full((H, W, 3), 0.7, F)
    cov = np.ones((H, W), F)
    c = np.zeros((H, W, 3), F)
    c[:, :17] = (1.0, 0.0, 0.0)
    c[:, 17:] = (0.0, 0.0, 4.0)
    out = dr.denoise(c, n, z, a, cov, iterations=5, sigma_color=1e6, sigma_depth=1e6, sigma_albedo=1e6)
    assert np.all(out[:, :17, 2] == 0) and np.all(out[:, :17, 1] == 0)
    assert np.all(out[:, 17:, 0] == 0) and np.all(out[:, 17:, 1] == 0)
    np.testing.assert_allclose(out[:, :17, 0], 1.0, rtol=1e-6)
    np.testing.assert_allclose(out[:, 17:, 2], 4.0, rtol=1e-6)


def test_weights_follow_the_formula_for_one_tap():
    """A 1 x 2 frame at step 1: each output is the two-tap mean with the weights of the specification, written out by hand."""
    c = np.array([[[1.0, 2.0, 3.0], [0.5, 0.25, 4.0]]], F)
    n = np.array([[[0.0, 1.0, 0.0], [0.0, 0.8, 0.6]]], F)
    z = np.array([[2.0, 2.5]], F)
    a = np.array([[[0.5, 0.5, 0.5], [0.4, 0.5, 0.6]]], F)
    cov = np.ones((1, 2), F)
    sc, sd, sa = 0.6, 0.1, 0.1
    out = dr.denoise(c, n, z, a, cov, iterations=1, sigma_color=sc, sigma_depth=sd, sigma_albedo=sa)

    def lum(v):
        return v[0] * 0.0722 + v[1] * 0.7152 + v[2] * 0.2126

    x = [c[0, k] / (1 + lum(c[0, k])) for k in range(2)]
    for p, q in ((0, 1), (1, 0)):
        wn = max(0.0, float(n[0, p] @ n[0, q])) ** 32
        wz = np.exp(-abs(z[0, p] - z[0, q]) / (sd * z[0, p]))
        wa = np.exp(-np.sum((a[0, p] - a[0, q]) ** 2) / sa ** 2)
        wc = np.exp(-np.sum((x[p] - x[q]) ** 2) / sc ** 2)
        wself = (3 / 8) ** 2
        wq = (3 / 8) * (1 / 4) * wn * wz * wa * wc
        want = (wself * c[0, p] + wq * c[0, q]) / (wself + wq)
        np.testing.assert_allclose(out[0, p], want, rtol=1e-5)
