"""Strategy masks without a GPU: the bit layout of clive2_amd/strategies.py against include/clive2_amd.h, the named masks, the
command-line parsers, render.py's refusals (before any renderer exists) and the library's two new exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from clive2_amd import strategies as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bit_layout_and_all():
    assert S.bit(0, 2) == 1 << 7 and S.bit(1, 1) == 1 << 1 and S.bit(6, 6) == 1 << 41 and S.bit(3, 4) == 1 << (3 * 7 + 3)
    assert bin(S.ALL).count("1") == 41 and len(S.PAIRS) == 41
    assert S.ALL == sum(1 << ((t - 1) * 7 + s) for t in range(1, 7) for s in range(7) if s + t >= 2)
    assert not S.ALL & 1                                   # (0, 1) is not a pair
    assert S.ALL >> 42 == 0
    for bad in [(0, 1), (0, 0), (1, 0), (7, 1), (1, 7), (-1, 3), (2, -1), (1.0, 2), ("1", 2), (True, 2)]:
        with pytest.raises(ValueError):
            S.bit(*bad)
    # the header's macros say the same
    header = open(os.path.join(ROOT, "include", "clive2_amd.h")).read()
    assert "#define CL2_STRATEGY_BIT(s, t)  ((uint64_t)1 << (((t) - 1) * 7 + (s)))" in header
    m = re.search(r"#define CL2_STRATEGY_ALL\s+\(\(uint64_t\)(0x[0-9A-Fa-f]+)\)", header)
    assert m and int(m.group(1), 16) == S.ALL
    assert "no reference counterpart (src/trace.metal:649-825 sums all pairs)" in header.lower()


def test_mask_and_pairs_round_trip():
    assert S.pairs(S.ALL) == list(S.PAIRS) and S.mask(S.PAIRS) == S.ALL
    assert S.mask([]) == 0 and S.pairs(0) == []
    rng = np.random.RandomState(3)
    for _ in range(50):
        chosen = [S.PAIRS[i] for i in np.flatnonzero(rng.rand(41) < 0.4)]
        assert S.pairs(S.mask(chosen)) == chosen           # bit order: t outer, s inner
    assert S.pairs(2 ** 64 - 1) == list(S.PAIRS)           # bits outside the 41 are dropped
    assert S.mask([(1, 2), (1, 2), (0, 2)]) == S.bit(0, 2) | S.bit(1, 2)
    for bad in ([(0, 1)], [(1, 2, 3)], [5], [(9, 9)]):
        with pytest.raises(ValueError):
            S.mask(bad)
    assert S.to_mask(None) == S.ALL and S.to_mask(5) == 5 and S.to_mask(np.uint64(6)) == 6 and S.to_mask([(2, 2)]) == S.bit(2, 2)
    for bad in (-1, 2 ** 64, True):
        with pytest.raises(ValueError):
            S.to_mask(bad)


def test_path_length_masks_partition_all():
    one, two, rest = S.path_length(1, 1), S.path_length(2, 2), S.path_length(3, None)
    assert S.pairs(one) == [(1, 1), (0, 2)] and S.pairs(two) == [(2, 1), (1, 2), (0, 3)]
    assert one | two | rest == S.ALL and not (one & two or one & rest or two & rest)
    assert S.path_length(3) == rest and S.path_length(1) == S.ALL and S.path_length(1, 2) == one | two
    assert S.path_length(1, 2) | S.path_length(3) == S.ALL and not S.path_length(1, 2) & S.path_length(3)
    for k in range(1, 12):
        assert all(s + t - 1 == k for s, t in S.pairs(S.path_length(k, k))) and S.path_length(k, k)
    assert S.path_length(12) == 0
    assert sum(bin(S.path_length(k, k)).count("1") for k in range(1, 12)) == 41
    for bad in [(0,), (2, 1), (1.5,), (1, 2.0), (True,)]:
        with pytest.raises(ValueError):
            S.path_length(*bad)


def test_light_and_camera_image_and_layers():
    assert S.LIGHT_IMAGE | S.CAMERA_IMAGE == S.ALL and not S.LIGHT_IMAGE & S.CAMERA_IMAGE
    assert S.pairs(S.LIGHT_IMAGE) == [(s, 1) for s in range(1, 7)]
    assert all(t >= 2 for _, t in S.pairs(S.CAMERA_IMAGE)) and bin(S.CAMERA_IMAGE).count("1") == 35
    assert list(S.LAYERS) == ["emission", "direct", "indirect"]
    assert S.LAYERS == {"emission": S.path_length(1, 1), "direct": S.path_length(2, 2), "indirect": S.path_length(3)}
    assert sum(S.LAYERS.values()) == S.ALL
    assert len(S.SINGLETONS) == 41 and sum(S.SINGLETONS.values()) == S.ALL and S.SINGLETONS["s0t2"] == S.bit(0, 2)


def test_parsers():
    assert S.parse_strategies("0,2") == S.bit(0, 2)
    assert S.parse_strategies("0,2;1,2") == S.bit(0, 2) | S.bit(1, 2)
    assert S.parse_strategies(" 6 , 6 ; 1,1 ") == S.bit(6, 6) | S.bit(1, 1)
    for bad in ["", " ", "0,1", "1", "1,2,3", "1;2", "a,b", "1,2;", ";1,2", "-1,2", "7,1", "1,7", "1.0,2", "1,2;;2,2", None, 3]:
        with pytest.raises(ValueError):
            S.parse_strategies(bad)
    assert S.parse_path_length("2") == S.path_length(2, 2)
    assert S.parse_path_length("1:2") == S.path_length(1, 2)
    assert S.parse_path_length("3:") == S.path_length(3) and S.parse_path_length(" 3 : ") == S.path_length(3)
    assert S.parse_path_length("1:") == S.ALL
    for bad in ["", "0", "0:2", "2:1", ":2", "a", "1:b", "1:2:3", "-1", "1.5", None, 2]:
        with pytest.raises(ValueError):
            S.parse_path_length(bad)


@pytest.mark.parametrize("argv", [
    ["--strategies", "0,1"],                                   # not a pair
    ["--strategies", "1;2"],
    ["--path-length", "0"],
    ["--path-length", "2:1"],
    ["--strategies", "0,2", "--path-length", "2"],            # mutually exclusive
    ["--layers", "out", "--strategies", "0,2"],
    ["--layers", "out", "--path-length", "3:"],
    ["--layers", "out", "--target-error", "0.05"],
    ["--layers", "out", "--denoise"],
    ["--layers", "out", "--robust"],
    ["--layers", "out", "--robust-denoise"],
    ["--layers", ""],
])
def test_render_refuses_bad_specs_before_any_renderer(argv, monkeypatch):
    from clive2_amd import render

    def no_renderer(*a, **k):
        raise AssertionError("a renderer was created")
    monkeypatch.setattr(render, "Renderer", no_renderer)
    monkeypatch.setattr(render, "create_scene_from_preset", no_renderer)
    with pytest.raises(SystemExit) as e:
        render.main(["--width", "16", "--height", "12"] + argv)
    assert e.value.code == 2                                   # ap.error


def test_render_refuses_layers_on_several_ranks(monkeypatch):
    from clive2_amd import render

    def no_renderer(*a, **k):
        raise AssertionError("a renderer was created")
    monkeypatch.setattr(render, "Renderer", no_renderer)
    monkeypatch.setattr(render, "create_scene_from_preset", no_renderer)
    monkeypatch.setattr(render, "rank_info", lambda: (0, 0, 2))
    with pytest.raises(SystemExit) as e:
        render.main(["--layers", "out"])
    assert e.value.code == 2


def test_host_tone_map_keeps_its_bytes_and_takes_a_log_average():
    from clive2_amd.camera import log_average, tone_map
    rng = np.random.RandomState(5)
    pic = (rng.rand(12, 16, 3) ** 4).astype(np.float32)
    luma = (pic * np.array([0.0722, 0.7152, 0.2126])).sum(axis=2)
    Lw = np.exp(np.log(0.1 + luma).sum() / (12 * 16))
    scaled = pic * 4.0 / Lw
    want = (255 * scaled / (scaled + 1.0)).astype(np.uint8)      # camera.py:73-82 as it was
    assert tone_map(pic, exposure=4.0).tobytes() == want.tobytes()
    assert log_average(pic) == Lw and tone_map(pic, exposure=4.0, Lw=Lw).tobytes() == want.tobytes()
    half = tone_map(pic * np.float32(0.5), exposure=4.0, Lw=Lw)
    scaled = (pic * np.float32(0.5)) * 4.0 / Lw
    assert half.tobytes() == (255 * scaled / (scaled + 1.0)).astype(np.uint8).tobytes()


def test_library_exports_both_functions():
    from clive2_amd import _native
    from clive2_amd.renderer import Renderer
    _native.build()
    L = C.CDLL(_native.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "clive2_amd.h")).read()
    for name in ("cl2_set_strategy_mask", "cl2_get_strategy_mask"):
        assert hasattr(L, name) and name in _native.EXPORTS, name
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert L.cl2_abi_version() == 6                               # additions only
    # NULL handles and a NULL out pointer are refused, not dereferenced (CL2_E_INVALID = -1)
    L.cl2_set_strategy_mask.argtypes = [C.c_void_p, C.c_uint64]
    L.cl2_get_strategy_mask.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    out = C.c_uint64(7)
    assert L.cl2_set_strategy_mask(None, S.ALL) == -1
    assert L.cl2_get_strategy_mask(None, C.byref(out)) == -1 and out.value == 7
    for name in ("set_strategy_mask", "strategy_mask", "render_layers"):
        assert callable(getattr(Renderer, name))
