"""The filter over the layers without a GPU: the two declarations of the header against _native.EXPORTS, the exports of the
built library at ABI 6, NULL handles, render.py's refusals before any renderer exists, and the numpy restatement
(tests/layers_denoise_reference.py) against denoise_reference on a small injected state."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_reference as dr
import error_states as es
import feature_states as fs
import layers_denoise_reference as ldr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cl2_denoise_layers", "cl2_keep_layer_picture")
DECLARATIONS = """
int cl2_denoise_layers(cl2_renderer* r, int iterations, const float* sigma_color /* [n_layers] */, float sigma_depth,
                       float sigma_albedo, float* out_layers /* [L][H][W][3] b, g, r, or NULL */, size_t n_layer_floats,
                       float* out_sum /* (H, W, 3), or NULL */, size_t n_sum_floats);
int cl2_keep_layer_picture(cl2_renderer* r, int layer /* 0..L-1, or -1 = the sum */, int iterations,
                           const float* sigma_color /* [n_layers] */, float sigma_depth, float sigma_albedo);
"""


def _header():
    return open(os.path.join(ROOT, "include", "clive2_amd.h")).read()


def test_header_declares_both_entry_points():
    from clive2_amd import _native
    header = _header()
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()
    flat = squeeze(header)
    for decl in DECLARATIONS.strip().split(";\n"):
        assert squeeze(decl.rstrip(";")) + ";" in flat, decl
    declared = set(re.findall(r"^(?:int|void|const char\*|size_t)\s+(cl2_\w+)\(", header, re.M))
    assert set(NAMES) <= declared
    assert declared == set(_native.EXPORTS)
    assert len(_native.EXPORTS) == len(set(_native.EXPORTS))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"the C ABI ({len(_native.EXPORTS)} entry points" in readme
    # the kinds of the kept picture and the working memory are stated where the functions are declared
    assert re.search(r"6 one filtered layer, 7 the sum of the filtered layers", header)
    assert "531 MB" in header
    assert "cl2_reduce_accumulators neither reduces nor refuses the layer accumulators" in header
    assert "no device tone map of layer pictures" not in flat


def test_library_exports_both_at_abi_6():
    from clive2_amd import _native
    _native.build()
    L = C.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.cl2_abi_version() == 6                                     # additions only
    # NULL handles are refused, not dereferenced (CL2_E_INVALID = -1)
    L.cl2_denoise_layers.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_size_t]
    L.cl2_keep_layer_picture.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float]
    sig, buf = (C.c_float * 1)(2.0), (C.c_float * 3)()
    assert L.cl2_denoise_layers(None, 1, sig, 0.1, 0.1, buf, 3, buf, 3) == -1
    assert L.cl2_denoise_layers(None, 1, None, 0.1, 0.1, None, 0, None, 0) == -1
    assert L.cl2_keep_layer_picture(None, -1, 1, sig, 0.1, 0.1) == -1
    assert L.cl2_keep_layer_picture(None, 0, 1, None, 0.1, 0.1) == -1


@pytest.mark.parametrize("argv", [
    ["--denoise-layers"],
    ["--denoise-layers", "--layers", "out"],                            # without --single-pass
    ["--denoise-layers", "--single-pass"],                              # without --layers
    ["--denoise-layers", "--denoise"],
    ["--denoise-layers", "--layers", "out", "--single-pass", "--denoise"],          # the refusals --layers has stay
    ["--denoise-layers", "--layers", "out", "--single-pass", "--device-tonemap"],
    ["--denoise-layers", "--layers", "out", "--single-pass", "--target-error", "0.05"],
    ["--denoise-layers", "--layers", "", "--single-pass"],
])
def test_render_refuses_before_any_renderer(argv, monkeypatch):
    from clive2_amd import render

    def no_renderer(*a, **k):
        raise AssertionError("a renderer was created")
    monkeypatch.setattr(render, "Renderer", no_renderer)
    monkeypatch.setattr(render, "create_scene_from_preset", no_renderer)
    with pytest.raises(SystemExit) as e:
        render.main(["--width", "16", "--height", "12"] + argv)
    assert e.value.code == 2                                            # ap.error


def test_python_names_the_new_kinds_and_defaults():
    from clive2_amd.renderer import Renderer
    assert Renderer._KEPT_NAMES[6] == "layer" and Renderer._KEPT_NAMES[7] == "layer_sum"
    assert set(Renderer._KEPT_KINDS.values()) == {1, 2, 3, 4}          # keep_picture makes neither
    d = Renderer.LAYER_DENOISE_DEFAULTS
    assert {k: d[k] for k in ("iterations", "sigma_depth", "sigma_albedo")} == \
        {k: Renderer.DENOISE_DEFAULTS[k] for k in ("iterations", "sigma_depth", "sigma_albedo")}
    assert isinstance(d["sigma_color"], dict)


# ---------------------------------------------------------------- the restatement
def _state(W, H, L, seed=3):
    """features and accumulators of feature_states (calm colours), and L layer accumulators that split rows 0..2"""
    pool = es.pool()
    cls, n, z, a, cov = fs.features(W, H)
    _, acc = fs.colours(cls, pool, wild=False)
    rs = np.random.RandomState(seed)
    share = rs.dirichlet(np.ones(L), size=(3, W * H)).astype(np.float32)          # (3, FB, L)
    with np.errstate(invalid="ignore", over="ignore"):
        lacc = np.ascontiguousarray((acc[:3, :, None] * share).transpose(2, 0, 1)).astype(np.float32)
    return acc, lacc, (n, z, a, cov)


def test_the_sum_of_one_layer_is_that_layer():
    W, H = 41, 25
    acc, lacc, g = _state(W, H, 1)
    layers, total = ldr.denoise_layers(lacc, acc, *g, 3, [1.5], 0.1, 0.1)
    assert layers.shape == (1, H, W, 3)
    assert total.tobytes() == layers[0].tobytes()
    assert ldr.same_bytes_or_both_nan(total, layers[0])


def test_one_layer_with_the_full_picture_is_the_plain_filter():
    W, H = 41, 25
    acc, _, g = _state(W, H, 1)
    lacc = acc[None, :3].copy()                                         # the one layer holds every pair
    c = fs.radiance(acc, W, H)
    assert ldr.layer_radiance(lacc, acc, W, H)[0].tobytes() == c.tobytes()
    for it in (0, 1, 3):
        layers, total = ldr.denoise_layers(lacc, acc, *g, it, [2.0], 0.1, 0.1)
        want = dr.denoise(c, *g, iterations=it, sigma_color=2.0, sigma_depth=0.1, sigma_albedo=0.1)
        assert layers[0].tobytes() == want.tobytes() == total.tobytes(), it


def test_layers_take_their_own_sigma_and_add_in_order():
    W, H = 7, 5
    acc, lacc, g = _state(W, H, 3)
    sig = [0.5, 2.0, 8.0]
    layers, total = ldr.denoise_layers(lacc, acc, *g, 2, sig, 0.1, 0.1)
    c = ldr.layer_radiance(lacc, acc, W, H)
    for l in range(3):
        want = dr.denoise(c[l], *g, iterations=2, sigma_color=sig[l], sigma_depth=0.1, sigma_albedo=0.1)
        assert layers[l].tobytes() == want.tobytes()
    assert total.tobytes() == ((layers[0] + layers[1]) + layers[2]).astype(np.float32).tobytes()
    other, _ = ldr.denoise_layers(lacc, acc, *g, 2, [2.0, 2.0, 2.0], 0.1, 0.1)
    assert other[1].tobytes() == layers[1].tobytes() and other[0].tobytes() != layers[0].tobytes()


def test_comparison_rule():
    a = np.array([1.0, np.nan, 3.0], np.float32)
    b = a.copy()
    b.view(np.uint32)[1] ^= 0x80000001                                  # another NaN: sign and payload are free
    assert np.isnan(b[1]) and ldr.same_bytes_or_both_nan(b, a)
    assert not ldr.same_bytes_or_both_nan(np.array([1.0, 2.0, 3.0], np.float32), a)
    assert not ldr.same_bytes_or_both_nan(np.array([1.0, np.nan, np.nan], np.float32), a)
    assert not ldr.same_bytes_or_both_nan(np.array([-0.0], np.float32), np.array([0.0], np.float32))
