"""Layer accumulators without a GPU: the header's macro and declarations against clive2_amd/strategies.py and _native.EXPORTS,
the ABI version, strategies.layer_masks, and render.py's refusals before any renderer exists."""
import ctypes as C
import os
import re

import pytest

from clive2_amd import strategies as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cl2_set_layers", "cl2_get_layers", "cl2_read_layers_packed", "cl2_write_layers_packed")


def _header():
    return open(os.path.join(ROOT, "include", "clive2_amd.h")).read()


def test_header_macro_and_declarations():
    from clive2_amd import _native
    header = _header()
    m = re.search(r"^#define CL2_MAX_LAYERS\s+(\d+)\s*$", header, re.M)
    assert m and int(m.group(1)) == S.MAX_LAYERS == 8
    want = {
        "cl2_set_layers": r"int cl2_set_layers\(cl2_renderer\* r, const uint64_t\* masks, int n_layers\);",
        "cl2_get_layers": r"int cl2_get_layers\(const cl2_renderer\* r, uint64_t\* masks_out, int capacity\);",
        "cl2_read_layers_packed": r"int cl2_read_layers_packed\(cl2_renderer\* r, float\* host_dst, size_t n_floats\);",
        "cl2_write_layers_packed": r"int cl2_write_layers_packed\(cl2_renderer\* r, const float\* host_src, size_t n_floats\);",
    }
    for name in NAMES:
        assert re.search("^" + want[name], header, re.M), name
        assert name in _native.EXPORTS, name
    # EXPORTS keeps matching the header: every declared entry point, and nothing else
    declared = set(re.findall(r"^(?:int|void|const char\*|size_t)\s+(cl2_\w+)\(", header, re.M))
    assert set(NAMES) <= declared
    assert declared == set(_native.EXPORTS)
    # what is out of scope is stated where the functions are declared
    assert "cl2_reduce_accumulators neither reduces nor refuses the layer accumulators" in header


def test_library_exports_the_four_functions_at_abi_6():
    from clive2_amd import _native
    _native.build()
    L = C.CDLL(_native.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.cl2_abi_version() == 6                                     # additions only
    # NULL handles are refused, not dereferenced (CL2_E_INVALID = -1)
    L.cl2_set_layers.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
    L.cl2_get_layers.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int]
    L.cl2_read_layers_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.cl2_write_layers_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    one = (C.c_uint64 * 1)(S.bit(0, 2))
    buf = (C.c_float * 3)()
    assert L.cl2_set_layers(None, one, 1) == -1
    assert L.cl2_get_layers(None, one, 1) == -1
    assert L.cl2_read_layers_packed(None, buf, 3) == -1
    assert L.cl2_write_layers_packed(None, buf, 3) == -1


def test_layer_masks_order_and_dropped_bits():
    assert S.layer_masks(S.LAYERS) == [S.path_length(1, 1), S.path_length(2, 2), S.path_length(3)]
    assert S.layer_masks({}) == []
    table = {"z": [(1, 2), (0, 2)], "a": S.bit(3, 1) | 1 | 1 << 63 | 1 << 42, "empty": 0, "m": S.bit(6, 6)}
    assert S.layer_masks(table) == [S.bit(0, 2) | S.bit(1, 2), S.bit(3, 1), 0, S.bit(6, 6)]      # the dictionary's order
    assert S.layer_masks(list(table.items())) == S.layer_masks(table)
    # a partition of all 41 pairs into eight layers by path length
    lengths = {k: S.path_length(k, k) for k in range(1, 8)}
    lengths[8] = S.path_length(8)
    masks = S.layer_masks(lengths)
    assert len(masks) == S.MAX_LAYERS and sum(masks) == S.ALL and all(masks)
    assert S.layer_masks(dict(list(S.SINGLETONS.items())[:8])) == [S.bit(s, t) for s, t in S.PAIRS[:8]]


def test_layer_masks_refusals():
    with pytest.raises(ValueError, match="share the pair \\(1, 2\\)"):
        S.layer_masks({"a": [(0, 2), (1, 2)], "b": S.bit(1, 2) | S.bit(2, 2)})
    with pytest.raises(ValueError, match="at most 8"):
        S.layer_masks({i: S.bit(*S.PAIRS[i]) for i in range(9)})
    with pytest.raises(ValueError):
        S.layer_masks(S.SINGLETONS)                                     # the pyramid has 41 layers: render_layers' job
    with pytest.raises(ValueError):
        S.layer_masks({"bad": [(0, 1)]})                                # not a pair
    with pytest.raises(ValueError):
        S.layer_masks({"bad": -1})
    # bits outside the 41 overlap nothing
    assert S.layer_masks({"a": 1 | 1 << 50, "b": 1 | 1 << 50 | S.bit(0, 2)}) == [0, S.bit(0, 2)]


@pytest.mark.parametrize("argv", [
    ["--single-pass"],                                                   # without --layers
    ["--single-pass", "--path-length", "3:"],
    ["--layers", "out", "--single-pass", "--strategies", "0,2"],       # the refusals --layers has
    ["--layers", "out", "--single-pass", "--path-length", "3:"],
    ["--layers", "out", "--single-pass", "--target-error", "0.05"],
    ["--layers", "out", "--single-pass", "--denoise"],
    ["--layers", "out", "--single-pass", "--robust"],
    ["--layers", "out", "--single-pass", "--robust-denoise"],
    ["--layers", "out", "--single-pass", "--device-tonemap"],
    ["--layers", "", "--single-pass"],
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


def test_render_refuses_single_pass_layers_on_several_ranks(monkeypatch):
    from clive2_amd import render

    def no_renderer(*a, **k):
        raise AssertionError("a renderer was created")
    monkeypatch.setattr(render, "Renderer", no_renderer)
    monkeypatch.setattr(render, "create_scene_from_preset", no_renderer)
    monkeypatch.setattr(render, "rank_info", lambda: (0, 0, 2))
    with pytest.raises(SystemExit) as e:
        render.main(["--layers", "out", "--single-pass"])
    assert e.value.code == 2
