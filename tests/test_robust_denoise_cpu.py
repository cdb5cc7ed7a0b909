"""The guided filter on the robust picture without a GPU: the input contract of csrc/denoise_robust.hpp through its numpy restatement
(tests/robust_denoise_reference.py) on the injected states of the GPU tests and on one pixel worked by hand, the gain the
combination was built for on synthetic addends with fireflies, the export, and the refusals of both CLIs."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import guided_denoise_reference as gr
import robust_denoise_reference as rd
import robust_reference as rr
import robust_states as rst

F = np.float32
CAP = F(2.0 ** 100)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- input states
@pytest.mark.parametrize("M", [3, 8, 16])
def test_input_variance_on_the_injected_states(M):
    cls, a7, bkt = rst.state(rst.pool(M), 41 * 25)
    assert set(np.unique(cls)) == set(rst.ALL)
    c, v = rd.input_state(bkt)
    assert v.dtype == np.float32 and c.dtype == np.float32 and v.shape == (41 * 25,) and c.shape == (41 * 25, 3)
    assert np.isfinite(v).all() and (v >= 0).all() and (v <= CAP).all()
    assert c.tobytes() == rr.robust_picture(bkt)[0].tobytes()
    kept, key, m, trim = rd.kept_buckets(bkt)
    n = m - 2 * trim
    assert (m == 0).any() and ((v == 0) >= (m == 0)).all()                    # 0 wherever m = 0 ...
    assert (m[v == 0] == 0).sum() == (m == 0).sum()
    few = (n < 2) & (m > 0)
    assert few.any() and (v[few] == CAP).all()
    nonfinite = (kept & ~np.isfinite(key)).any(0)
    assert (v[nonfinite] == CAP).all()
    assert nonfinite.any() or M == 16          # at m = 16 an infinite key gives G = 1, c = 7: the two buckets kept are finite ones
    assert (v[cls == rst.ZERO] == 0).all()
    k_lo = np.where(kept, key, np.inf).min(0)
    k_hi = np.where(kept, key, -np.inf).max(0)
    tied = (cls == rst.TIES) & (k_lo == k_hi) & (n >= 2)
    assert tied.any() and (v[tied] == 0).all()
    # ... and 0 nowhere else but where the kept keys are all equal
    assert ((v == 0) == ((m == 0) | ((n >= 2) & (k_lo == k_hi) & np.isfinite(k_lo)))).all()
    ordinary = cls == rst.ORDINARY
    assert (v[ordinary] > 0).all() and (v[ordinary] < 1).all()


def test_one_pixel_by_hand():
    """Grey buckets with keys 1 .. 7 and 1000, W = 1, M = 8.  S = 1028, N = -7 - 10 - 9 - 4 + 5 + 18 + 35 + 7000 = 7028,
    G = 7028 / (8 * 1028) = 0.8546, c = min(floor(3.418), 7 / 2) = 3: ranks 4 and 5 are kept, the keys 4 and 5 (buckets 3 and 4).
    n = 2, ybar = 4.5, Q = 0.25 + 0.25, var = (0.5 / 1) / 2 = 0.25; the colour is (4 + 5) / (1 + 1) = 4.5.  The luma weights are
    float32 and add up to 1 + 2e-8, hence the relative tolerance on ybar and v."""
    order = [5, 1000, 2, 4, 7, 1, 6, 3]
    b = np.array([(k, k, k, 1.0) for k in order], F).reshape(8, 4, 1)
    valid, rank, m, G, c = rr.gini_trim(b)
    assert m[0] == 8 and c[0] == 3
    assert G[0] == pytest.approx(7028.0 / 8224.0, rel=1e-12)
    kept, key, _, _ = rd.kept_buckets(b)
    assert np.flatnonzero(kept[:, 0]).tolist() == [0, 3]                      # the buckets that hold 5 and 4
    s = float(np.float64(rr.LUMA[0]) + np.float64(rr.LUMA[1]) + np.float64(rr.LUMA[2]))
    assert key[kept[:, 0], 0].mean() == pytest.approx(4.5 * s, rel=1e-12)
    pic, v = rd.input_state(b)
    assert pic[0].tolist() == [4.5, 4.5, 4.5]
    assert v.dtype == np.float32 and float(v[0]) == pytest.approx(0.25, rel=1e-6)
    # the firefly moved the guide not at all: without it (key 8 in its place) nothing is trimmed and v is the variance of the mean of 1 .. 8
    b[1, :3] = 8.0
    _, v8 = rd.input_state(b)
    assert rr.gini_trim(b)[4][0] == 1                                         # G = 0.29: one bucket either end
    assert float(v8[0]) == pytest.approx(3.5 / 6.0, rel=1e-6)                 # keys 2 .. 7: Q = 17.5, / 5 / 6


def test_few_kept_buckets_take_the_cap_and_no_bucket_gives_zero():
    empty = np.zeros((4, 4, 1), F)
    assert rd.input_state(empty)[1][0] == 0
    one = empty.copy(); one[2, :, 0] = (1.0, 2.0, 3.0, 2.0)
    pic, v = rd.input_state(one)
    assert pic[0].tolist() == [0.5, 1.0, 1.5] and v[0] == CAP
    inf = np.array([(1, 1, 1, 1), (np.inf, 1, 1, 1), (2, 2, 2, 1)], F).reshape(3, 4, 1)   # G = 1, c = 1: one bucket kept
    assert rr.gini_trim(inf)[4][0] == 1 and rd.input_state(inf)[1][0] == CAP
    huge = np.array([(1e30, 1e30, 1e30, 1e-8), (0, 0, 0, 1)], F).reshape(2, 4, 1)          # var = 5e75 > 2^100
    assert rd.input_state(huge)[1][0] == CAP


# ---------------------------------------------------------------- quality, on the restatement alone
def _synthetic(n, p, M=8, H=64, W=96):
    rs = np.random.RandomState(3)
    level = np.where(np.arange(W) < W // 2, 0.5, 1.0)[None, :] * np.ones((H, 1))
    xs, ws, lum = [], [], []
    for _ in range(n):
        x = level * rs.gamma(8.0, 0.125, (H, W))
        fly = rs.rand(H, W) < p                                               # drawn also when p = 0
        x = np.where(fly, 500 * level, x).astype(F).reshape(-1)
        xs.append(np.repeat(x[:, None], 3, 1)); ws.append(np.ones(H * W, F)); lum.append(x.astype(np.float64))
    _, bkt = rr.accumulate(xs, ws, M)
    lum = np.array(lum)
    nrm = np.zeros((H, W, 3), F); nrm[..., 1] = 1
    feats = (nrm, np.full((H, W), 3.0, F), np.full((H, W, 3), 0.5, F), np.ones((H, W), F))
    kw = dict(iterations=4, sigma_luma=4.0)
    plain = rr.plain_picture(bkt).astype(F).reshape(H, W, 3)
    vplain = (lum.var(0, ddof=1) / n).astype(F).reshape(H, W)
    mse = lambda a: float((((a[..., 1].astype(np.float64) - level) / level) ** 2).mean())
    return dict(raw=mse(plain), robust=mse(rr.robust_picture(bkt, H, W)[0]), guided=mse(gr.denoise(plain, vplain, *feats, **kw)[0]),
                new=mse(rd.denoise(bkt, H, W, *feats, **kw)[0]))


def test_the_combination_costs_little_on_clean_noise():
    """64 x 96, levels 0.5 | 1.0, 64 addends level * gamma(8, 0.125), M = 8, 4 passes, sigma_luma 4, flat features; the mean over
    pixels of ((green - level) / level)^2.  The guide from eight bucket means is noisier than the one from 64 addends: measured
    1.04 of the guided filter's error, bound 1.25 (the margin is for another numpy's gamma stream)."""
    e = _synthetic(64, 0.0)
    print({k: f"{x:.3g}" for k, x in e.items()}, f"new / guided {e['new'] / e['guided']:.3f}")
    assert e["new"] <= 1.25 * e["guided"]
    assert e["new"] <= 0.05 * e["raw"]                                        # and it does denoise (measured 0.0044)


@pytest.mark.parametrize("n", [64, 256])
def test_with_fireflies_the_combination_beats_both_parts(n):
    """The same with one addend in 1000 replaced by 500 * level: the new picture's error is at most 0.05 of the better of the robust
    picture's (full noise everywhere else) and the guided one's (the firefly spread over its neighbourhood).  Measured 0.0064 at
    64 addends and 0.0012 at 256."""
    e = _synthetic(n, 1e-3)
    print(n, {k: f"{x:.3g}" for k, x in e.items()}, f"new / min(robust, guided) {e['new'] / min(e['robust'], e['guided']):.4f}")
    assert e["new"] <= 0.05 * min(e["robust"], e["guided"])


# ---------------------------------------------------------------- binding
@pytest.fixture(scope="module")
def native_lib():
    from clive2_amd import _native
    _native.build()
    return _native.lib()


def test_library_exports_and_header_declares_the_call(native_lib):
    from clive2_amd import _native
    header = open(os.path.join(ROOT, "include", "clive2_amd.h")).read()
    assert "cl2_denoise_robust" in _native.EXPORTS
    assert hasattr(native_lib, "cl2_denoise_robust")
    assert re.search(r"^int cl2_denoise_robust\(", header, re.M)
    assert native_lib.cl2_abi_version() == 6


def test_the_call_refuses_a_null_handle(native_lib):
    buf = np.zeros(64, F)
    p = buf.ctypes.data_as(C.c_void_p)
    assert native_lib.cl2_denoise_robust(None, 1, 4.0, 0.1, 0.1, p, C.c_size_t(48), None, C.c_size_t(0)) == -1


def test_python_defaults_equal_the_restatements():
    from clive2_amd.renderer import Renderer
    assert Renderer.ROBUST_GUIDED_DEFAULTS == rd.DEFAULTS
    assert callable(Renderer.robust_guided_radiance) and isinstance(Renderer.robust_guided_image, property)


# ---------------------------------------------------------------- CLI
class _Reached(Exception):
    pass


def _guarded(cli, monkeypatch, reached):
    mod = importlib.import_module("clive2_amd." + cli)

    def no_renderer(*a, **k):
        if reached:
            raise _Reached()
        raise AssertionError("a renderer was made before the arguments were checked")
    monkeypatch.setattr(mod, "Renderer", no_renderer)
    monkeypatch.setattr(mod, "rank_info", no_renderer)
    return mod


WITH_ANOTHER = "does not go with --robust, --denoise or --variance-guided"
BAD_COUNT = "--robust-denoise takes 3..16 buckets"


@pytest.mark.parametrize("argv,why", [(["--robust-denoise", "--robust"], WITH_ANOTHER), (["--robust-denoise", "4", "--robust", "4"], WITH_ANOTHER),
                                      (["--robust-denoise", "--denoise"], WITH_ANOTHER),
                                      (["--robust-denoise", "--denoise", "--variance-guided"], WITH_ANOTHER),
                                      (["--robust-denoise", "--variance-guided"], "--variance-guided needs --denoise"),
                                      (["--robust-denoise", "2"], BAD_COUNT), (["--robust-denoise", "17"], BAD_COUNT),
                                      (["--robust-denoise", "-1"], BAD_COUNT)])
@pytest.mark.parametrize("cli", ["render", "movie"])
def test_cli_refuses_robust_denoise_with_another_picture(cli, argv, why, monkeypatch, capsys):
    """exit code 2 before any renderer is made, and by the check meant for it: the message names the reason (an unknown flag would
    exit with 2 as well)"""
    mod = _guarded(cli, monkeypatch, False)
    with pytest.raises(SystemExit) as e:
        mod.main(argv + ["--width", "16", "--height", "16"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert why in err and "unrecognized arguments" not in err


@pytest.mark.parametrize("argv", [["--robust-denoise"], ["--robust-denoise", "3"], ["--robust-denoise", "16"],
                                  ["--robust-denoise", "--target-error", "0.05", "--adaptive"]])
@pytest.mark.parametrize("cli", ["render", "movie"])
def test_cli_accepts_robust_denoise(cli, argv, monkeypatch):
    mod = _guarded(cli, monkeypatch, True)
    with pytest.raises(_Reached):                                             # past every check of the arguments
        mod.main(argv + ["--width", "16", "--height", "16"])
