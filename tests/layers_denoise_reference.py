"""numpy restatement of the filter over the layers (csrc/denoise_layers.hpp, cl2_denoise_layers): per layer
denoise_reference.denoise on scrub(lacc_l / w) with the layer's own sigma_color, then the float32 sum in layer order.  A helper
module: no tests live here, and nothing here needs the device.

    lacc   (L, 3, W*H) float32: Renderer.layer_accumulators()
    acc    (8, W*H) float32: Renderer.packed_accumulators(); row 3 is the shared weight
"""
import numpy as np

import denoise_reference as dr

F = np.float32


def layer_radiance(lacc, acc, W, H):
    """(L, H, W, 3) float32: k_layers_input, i.e. k_denoise_input on accumulators whose rows 0..2 are lacc[l]"""
    lacc, w = np.asarray(lacc, F), np.asarray(acc, F)[3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c = (lacc / w).astype(F)
    c = np.where(np.isfinite(c), c, F(0))
    return np.ascontiguousarray(c.reshape(len(lacc), 3, H, W).transpose(0, 2, 3, 1))


def layer_sum(pictures):
    """S = F_0, then S = S + F_l: one float32 add per component, in layer order"""
    pictures = np.asarray(pictures, F)
    s = pictures[0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for p in pictures[1:]:
            s = (s + p).astype(F)
    return s


def denoise_layers(lacc, acc, normal, depth, albedo, coverage, iterations, sigma_color, sigma_depth, sigma_albedo):
    """-> ((L, H, W, 3) filtered layers, (H, W, 3) their sum); sigma_color: one value per layer"""
    H, W = np.shape(coverage)
    c = layer_radiance(lacc, acc, W, H)
    assert len(sigma_color) == len(c)
    out = np.stack([dr.denoise(c[l], normal, depth, albedo, coverage, iterations=iterations, sigma_color=sigma_color[l],
                               sigma_depth=sigma_depth, sigma_albedo=sigma_albedo) for l in range(len(c))])
    return out, layer_sum(out)


def same_bytes_or_both_nan(got, want):
    """the comparison rule of the device tests: equal as bytes, except that where `want` holds a NaN `got` must hold a NaN
    (payload and sign are free)"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))
