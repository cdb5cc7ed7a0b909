"""The per-pixel choice among the fixed filter's scales (csrc/denoise_select.hpp, cl2_denoise_select) without a device: the
plumbing of the second public header, the numpy restatement (tests/denoise_select_reference.py) against the modules it is built
on, that the smoothing tolerance of the device test means something on the inputs it uses, the behaviour of the choice on a
picture with structure the features cannot see, and Renderer.selected_radiance's argument plumbing against a stand-in library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_error_reference as de
import denoise_reference as dr
import denoise_select_reference as sel
import error_states as es
import feature_states as fs

F = np.float32
D = np.float64
EPS = 1 / 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pool():
    return es.pool()


def _calm(pool, W, H):
    """the well-scaled pixel states of error_states under the features of feature_states: what k_de_input makes of them, and f"""
    _, acc, mom = es.state(pool, W * H, es.BASE)
    _, n, z, a, cov = fs.features(W, H)
    y, state, v, a_, _ = de.inputs(acc, mom, W, H)
    return y, state, v, a_, dict(normal=n, depth=z, albedo=a, coverage=cov)


@pytest.fixture(scope="module")
def calm(pool):
    made = {}

    def get(W, H):
        if (W, H) not in made:
            y, state, v, a, f = _calm(pool, W, H)
            made[(W, H)] = (y, state, v, a, f, sel.estimate(y, state, v, a, f, probes=2, eps=EPS, seed=5, smooth_passes=2, iterations=3))
        return made[(W, H)]
    return get


# ---------------------------------------------------------------- plumbing
def _names(header):
    with open(os.path.join(ROOT, "include", header)) as fh:
        return sorted(set(re.findall(r"\b(cl2_[a-z_0-9]+)\s*\(", fh.read())))


def test_plumbing(capsys, tmp_path):
    from clive2_amd import _native, render, movie
    from clive2_amd.renderer import Renderer
    assert _names("clive2_amd_ext.h") == sorted(_native.EXT_EXPORTS)
    assert _names("clive2_amd.h") == sorted(_native.EXPORTS)
    assert not set(_native.EXT_EXPORTS) & set(_native.EXPORTS)
    raw = C.CDLL(_native.LIB_PATH)
    for name in _native.EXT_EXPORTS:
        assert hasattr(raw, name), name
    L = _native.lib()
    assert L.cl2_ext_version() == 1 and L.cl2_abi_version() == 6
    out = (C.c_double * 8)()
    assert L.cl2_denoise_select(None, 3, 2.0, 0.1, 0.1, 1, EPS, 0, 0, 2, 0.001, None, 0, None, 0, out, None, 0, None, 0) == -1
    assert L.cl2_keep_selected_picture(None, 3, 2.0, 0.1, 0.1, 1, EPS, 0, 0, 2) == -1
    assert os.path.join(ROOT, "include", "clive2_amd_ext.h") in _native._sources()
    # the ext header is plain C
    src = tmp_path / "ext.c"
    src.write_text('#include "clive2_amd_ext.h"\nint main(void) { return cl2_ext_version(); }\n')
    res = subprocess.run(["gcc", "-Wall", "-Werror", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    with open(os.path.join(ROOT, "include", "clive2_amd_ext.h")) as fh:
        text = fh.read()
    assert "CLOSED" in text.split("#ifndef")[0] and "BIASED LOW" in text
    assert Renderer._KEPT_NAMES[8] == "selected" and "selected" not in Renderer._KEPT_KINDS
    # refused before any renderer exists
    base = ["--scene", "empty", "--width", "32", "--height", "24", "--samples", "8", "--select-scale"]
    for main in (render.main, movie.main):
        for extra in ([], ["--denoise", "--variance-guided"], ["--denoise", "--robust"], ["--robust-denoise"],
                      ["--denoise", "--robust-denoise"], ["--denoise", "--denoise-layers"],
                      ["--denoise", "--target-error", "0.1", "--error-of", "denoised"]):
            with pytest.raises(SystemExit) as ex:
                main(base + extra)
            assert ex.value.code == 2, extra
    with pytest.raises(SystemExit) as ex:
        render.main(base[:-1] + ["--denoise", "--scale-out", str(tmp_path / "k.npy")])
    assert ex.value.code == 2
    capsys.readouterr()


def test_new_kernels_use_no_scratch(tmp_path):
    """the compiler's resource report of every kernel of denoise_select.hpp, cross-compiled for gfx950: no scratch memory"""
    from clive2_amd import _native
    src = tmp_path / "ds.hip"
    csrc = os.path.join(ROOT, "clive2_amd", "csrc")
    src.write_text(f'#include "{csrc}/denoise.hpp"\n#include "{csrc}/denoise_select.hpp"\n')
    flags = [f for f in _native.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    res = subprocess.run(["hipcc"] + flags + ["--cuda-device-only", "-c", str(src), "-o", str(tmp_path / "ds.o"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    report = {}
    name = None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for key in ("VGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                report.setdefault(name, {})[key] = int(m.group(1))
    new = {k: v for k, v in report.items() if "k_ds_" in k}
    for k, v in new.items():
        print(k, v)
    assert sorted(re.search(r"k_ds_[a-z]+", k).group(0) for k in new) == ["k_ds_map", "k_ds_select", "k_ds_smooth", "k_ds_terms"]
    for k, v in new.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["LDS Size [bytes/block]"] < 65536 // 2


# ---------------------------------------------------------------- the restatement against the modules it is built on
@pytest.mark.parametrize("W,H", [(7, 5), (41, 25)])
def test_restatement_against_itself(W, H, calm):
    y, state, v, a, f, got = calm(W, H)
    g = (f["normal"], f["depth"], f["albedo"], f["coverage"])
    assert (state == 0).any() and (state == 2).any()
    # level j is the filter with j passes
    for j in range(4):
        assert got["Ly"][j].tobytes() == dr.denoise(y, *g, iterations=j).tobytes(), j
    # m_K is the error estimate's map, m_j that of j passes, the totals' N among them
    for j in (0, 1, 3):
        m, out, _ = de.estimate(y, state, v, a, None, f, kind=0, probes=2, eps=EPS, seed=5, iterations=j)
        assert de.same(got["m"][j], m), j
    assert got["out"][2] == out[2] and got["out"][3] == out[3]
    # S = 0: M is m
    assert sel.smooth(got["m"], state, f, 0) is not None and de.same(sel.smooth(got["m"], state, f, 0), got["m"])
    s0 = sel.estimate(y, state, v, a, f, probes=2, eps=EPS, seed=5, smooth_passes=0, iterations=3)
    assert de.same(s0["M"], s0["m"]) and de.same(s0["m"], got["m"])
    # smoothing moves the maps, leaves uncovered pixels alone, and the picture is a gather of the levels
    assert (got["M"] != got["m"]).any()
    assert (got["M"][:, state != 2] == got["m"][:, state != 2]).all()
    assert (got["scale"][state == 0] == 0).all()
    for j in range(4):
        at = got["scale"] == j
        assert got["picture"][at].tobytes() == got["Ly"][j][at].tobytes()
    assert got["out"][7] == got["scale"][state > 0].sum()


def test_argmin_rule():
    """ties go to the smaller j, a NaN never wins over a number, all NaN stays at 0; state 0 takes 0 and state 1 takes K"""
    nan, inf = np.nan, np.inf
    table = np.array([[[1.0, 2.0, nan]],            # M_0 of three pixels
                      [[1.0, 1.0, 5.0]],            # M_1
                      [[0.5, 1.0, 5.0]]], F)        # M_2
    assert sel.select(table, np.full((1, 3), 2)).tolist() == [[2, 1, 1]]
    table = np.array([[[nan, -inf, 3.0]], [[nan, nan, nan]], [[nan, -inf, 3.0]]], F)
    assert sel.select(table, np.full((1, 3), 2)).tolist() == [[0, 0, 0]]
    table = np.array([[[nan, inf, -1.0]], [[inf, 7.0, nan]], [[2.0, nan, -1.0]]], F)
    assert sel.select(table, np.full((1, 3), 2)).tolist() == [[2, 1, 0]]
    assert sel.select(table, np.array([[0, 1, 2]])).tolist() == [[0, 2, 0]]


# ---------------------------------------------------------------- the smoothing tolerance means something on these inputs
@pytest.mark.parametrize("W,H", [(7, 5), (41, 25)])
def test_smoothing_tolerance_is_meaningful(W, H, calm):
    """The device test holds |dev - ref| <= 1e-4 Abs_jp, Abs = sum w |m_j| / sum w carried through the passes.  That asks something
    only if float32 rounding alone stays well inside it: on the calm states, K = 3 and S = 2, the float32 restatement lies within
    0.25 of that bound of the same formula in float64.  A condition on the inputs, not on the code under test."""
    y, state, v, a, f, got = calm(W, H)
    m = got["m"]
    assert np.isfinite(m[:, state == 2]).all()
    M32 = sel.smooth(m, state, f, 2)
    M64, A64 = sel.smooth(m, state, f, 2, dtype=D, with_abs=True)
    assert de.same(M32, got["M"])
    assert (np.isfinite(M32) == np.isfinite(M64)).all()
    ok = np.broadcast_to(state == 2, m.shape)
    err = np.abs(M32.astype(D) - M64)[ok]
    bound = 1e-4 * A64[ok]
    worst = (err / np.where(bound > 0, bound, 1.0))[bound > 0].max()
    print(f"{W} x {H}: float32 against float64 smoothing, worst |d| / (1e-4 Abs) {worst:.4f}")
    assert (err <= 0.25 * bound).all()


# ---------------------------------------------------------------- behaviour
def test_flat_regions_choose_coarser_levels_than_hidden_structure():
    """64 x 48, constant features, 12 noise seeds, noise of known variance with consistent moments (v is exact).  Left half: a flat
    colour.  Right half: a one-pixel luma checkerboard the features cannot see, its contrast far above the noise: every pass
    destroys it.  The mean chosen level on the flat half is greater than on the checkerboard half."""
    W, H, K = 64, 48, 3
    yy, xx = np.mgrid[0:H, 0:W]
    f = dict(normal=np.tile(np.array([0, 1, 0], F), (H, W, 1)), depth=np.full((H, W), 3.0, F),
             albedo=np.full((H, W, 3), 0.5, F), coverage=np.ones((H, W), F))
    right = xx >= W // 2
    mu = np.where(right & ((xx + yy) % 2 == 0), 0.8, 0.5)
    mu = np.where(right & ((xx + yy) % 2 == 1), 0.2, mu)
    sigma = 0.05
    state = np.full((H, W), 2)
    v = np.full((H, W), sigma * sigma, F)
    a = np.repeat(np.sqrt(v.astype(D)).astype(F)[..., None], 3, -1)          # grey noise: d = (1, 1, 1), luma(d) = 1
    flat, checker = [], []
    for t in range(12):
        rs = np.random.RandomState(500 + t)
        eta = sigma * rs.standard_normal((H, W))
        y = np.repeat((mu + eta)[..., None], 3, -1).astype(F)
        got = sel.estimate(y, state, v, a, f, probes=1, eps=EPS, seed=t, smooth_passes=2, iterations=K)
        flat.append(got["scale"][:, : W // 2 - 4].mean())
        checker.append(got["scale"][:, W // 2 + 4:].mean())
    print(f"mean chosen level: flat half {np.mean(flat):.3f}, checkerboard half {np.mean(checker):.3f}")
    assert np.mean(flat) > np.mean(checker)


# ---------------------------------------------------------------- Renderer's argument plumbing, against a stand-in library
def test_selected_radiance_plumbing():
    from clive2_amd import renderer as rmod
    from clive2_amd.renderer import Renderer

    class Lib:
        def __init__(self):
            self.calls = []
            self.kind = 0

        def cl2_denoise_select(self, h, *a):
            self.calls.append(("select", a))
            out = a[14]
            for k in range(8):
                out[k] = float(k)
            return 0

        def cl2_keep_selected_picture(self, h, *a):
            self.calls.append(("keep", a))
            self.kind = 8
            return 0

        def cl2_kept_picture(self, h):
            return self.kind

    class Fake(Renderer):
        def __init__(self):
            self._L, self._h, self.pixel_width, self.pixel_height = Lib(), None, 6, 4

        def tone_mapped_picture(self, *a):
            return ("tone", a)

        def __del__(self):
            pass
    r = Fake()
    pic = r.selected_radiance()
    assert pic.shape == (4, 6, 3) and pic.dtype == F
    a = r._L.calls[-1][1]
    assert a[:4] == (3, 2.0, 0.1, 0.1) and a[4:7] == (1, 1 / 16, int(rmod.DENOISED_ERROR_CORRELATED))
    assert a[7].value == 0 and a[8] == rmod.SELECT_SMOOTH_PASSES and a[9] == Renderer.ERROR_FLOOR
    assert a[11].value == 72 and a[12] is None and a[13].value == 0 and a[15] is None and a[16].value == 0
    assert a[17] is None and a[18].value == 0 and len(a) == 19
    pic, scale, stats, (m, M) = r.selected_radiance(iterations=5, sigma_color=0.7, sigma_depth=0.2, sigma_albedo=0.3, probes=4,
                                                    epsilon=0.25, correlated=True, seed=-1, smooth_passes=0, floor=0.5,
                                                    return_scale=True, return_stats=True, return_maps=True)
    a = r._L.calls[-1][1]
    assert a[:4] == (5, 0.7, 0.2, 0.3) and a[4:7] == (4, 0.25, 1) and a[7].value == 0xFFFFFFFF and a[8] == 0 and a[9] == 0.5
    assert scale.shape == (4, 6) and scale.dtype == np.int32 and a[13].value == 24
    assert m.shape == M.shape == (6, 4, 6) and a[16].value == 2 * 6 * 24
    assert stats.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    assert r.selected_radiance(return_stats=True)[1].dtype == D
    assert r.kept_kind is None
    r.keep_selected_picture(iterations=2, seed=9)
    kind, a = r._L.calls[-1]
    assert kind == "keep" and a[:4] == (2, 2.0, 0.1, 0.1) and a[4:7] == (1, 1 / 16, 0) and a[7].value == 9 and a[8] == rmod.SELECT_SMOOTH_PASSES
    assert len(a) == 9 and r.kept_kind == "selected"
    with pytest.raises(TypeError):
        r.keep_selected_picture(floor=0.1)
    n = len(r._L.calls)
    assert r.tone_mapped("selected", 2.0, 0.5)[0] == "tone" and r._L.calls[n][0] == "keep" and len(r._L.calls) == n + 1
    assert 0 <= rmod.SELECT_SMOOTH_PASSES <= 4
