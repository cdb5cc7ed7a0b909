"""The numpy statement of the device tone map of a kept picture (tests/picture_tone_reference.py) against the host path it
restates (clive2_amd.camera.tone_map on a float32 picture), the derived tolerance of its log sum, the conditions on the injected
states (tests/picture_states.py) that the device tests (tests/test_gpu_picture_tone.py) rely on, and what of the new entry points
can be checked without a GPU: the NULL-handle returns, the symbols, the CLI refusals.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import picture_states as ps
import picture_tone_reference as pr
from clive2_amd.camera import tone_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [(4.0, 1.0), (2.0, 1.5), (4.0, 0.25), (3.3, 1.0)]          # tests/test_gpu_tone.py
NEW = ["cl2_keep_picture", "cl2_kept_picture", "cl2_write_picture", "cl2_read_picture", "cl2_picture_log_sum", "cl2_picture_tone_map"]


@pytest.fixture(scope="module")
def pl():
    return ps.pool()


def _host(pic, exposure, white_point):
    with np.errstate(all="ignore"):
        return tone_map(pic, exposure=exposure, white_point=white_point)


def _mismatch(got, want, cls):
    got, want = got.reshape(-1, 3), want.reshape(-1, 3)
    bad = np.flatnonzero((got != want).any(1))
    return f"{bad.size} pixels differ: " + str([(int(p), ps.NAMES[cls[p]], got[p].tolist(), want[p].tolist()) for p in bad[:5]])


@pytest.mark.parametrize("kind", ["ordinary", "finite"])
@pytest.mark.parametrize("W,H", [(7, 1), (91, 60), (513, 512)])
def test_apply_given_the_hosts_log_average_is_the_host_tone_map(W, H, kind, pl):
    """apply() with the Lw camera.tone_map itself computes equals camera.tone_map byte for byte, and the log terms are the host's
    bit for bit"""
    cls, pick, pic = ps.state(pl, W * H, ps.KINDS[kind], seed=W + H)
    if W * H >= 64:
        assert set(np.unique(cls[:64])) == set(ps.KINDS[kind])
    Lw = pr.host_log_average(pic, W, H)
    assert np.isfinite(Lw)
    for exposure, wp in SETTINGS:
        got = pr.apply(pic, exposure, wp, Lw).reshape(H, W, 3)
        want = _host(pic.reshape(H, W, 3), exposure, wp)
        assert got.tobytes() == want.tobytes(), (exposure, wp, _mismatch(got, want, cls))
    with np.errstate(all="ignore"):
        host_terms = np.log(0.1 + (pic.reshape(H, W, 3) * np.array([0.0722, 0.7152, 0.2126])).sum(axis=2)).reshape(-1)
    assert pr.terms(pic).tobytes() == host_terms.tobytes()


def test_all_states_give_a_nan_sum_and_a_black_picture_on_the_host(pl):
    """no scrub: one NaN term makes Lw NaN and every byte 0, in the restatement as on the host"""
    W, H = 91, 60
    cls, pick, pic = ps.state(pl, W * H, ps.ALL, seed=W + H)
    assert set(np.unique(cls[:64])) == set(ps.ALL)
    t = pr.terms(pic)
    assert np.isnan(t[cls == ps.POLE]).all() and not np.isfinite(t[cls == ps.NONFINITE]).any()
    assert np.isfinite(t[(cls != ps.POLE) & (cls != ps.NONFINITE)]).all()
    Lw = pr.host_log_average(pic, W, H)
    assert np.isnan(Lw) and np.isnan(pr.exact_sum(t)) and np.isnan(pr.device_sum(t))
    assert not _host(pic.reshape(H, W, 3), 4.0, 1.0).any() and not pr.apply(pic, 4.0, 1.0, Lw).any()
    # the pole: v is -inf, the byte 0
    assert np.isneginf(pr.value(pic, 4.0, 1.0, 1.0)[cls == ps.POLE]).all()


@pytest.mark.parametrize("W,H", ps.SIZES)
def test_sum_bound_holds_for_numpys_sum_and_for_the_device_order(W, H, pl):
    FB = W * H
    for kind in ("ordinary", "finite"):
        cls, pick, pic = ps.state(pl, FB, ps.KINDS[kind], seed=W + H)
        t = pr.terms(pic)
        exact, bound = pr.exact_sum(t), pr.sum_bound(t, FB)
        assert np.isfinite(exact) and bound > 0
        for s in (float(t.sum()), pr.device_sum(t)):
            assert abs(s - exact) <= bound, (kind, s, exact, bound)
        for p in sorted({0, FB - 1, min(FB - 1, 262144)}):            # a dropped term shows
            assert abs(t[p]) > 2 * bound


@pytest.mark.parametrize("W,H", ps.SIZES)
def test_log_average_disagreement_moves_only_fragile_bytes(W, H, pl):
    """The host's Lw (numpy's pairwise sum) and the Lw of the device's order of additions differ by at most the sum's tolerance;
    the two pictures then differ only at fragile bytes, by one count.  On ordinary states at most 16 bytes per frame are fragile
    (the device test fails beyond that), on finite states the SATURATED pixels are."""
    FB = W * H
    for kind in ("ordinary", "finite"):
        cls, pick, pic = ps.state(pl, FB, ps.KINDS[kind], seed=W + H)
        t = pr.terms(pic)
        exact, bound = pr.exact_sum(t), pr.sum_bound(t, FB)
        frag = pr.fragile(pic, 4.0, 1.0, pr.log_average(exact, FB), bound / FB)
        print(f"{W}x{H} {kind}: {int(frag.sum())} fragile bytes of {frag.size}")
        if kind == "ordinary":
            assert frag.sum() <= 16
        else:
            sat = cls == ps.SATURATED
            assert frag[sat].all() and frag[~sat].sum() <= 16
        host = pr.apply(pic, 4.0, 1.0, pr.host_log_average(pic, W, H))
        dev = pr.apply(pic, 4.0, 1.0, pr.log_average(pr.device_sum(t), FB))
        d = np.abs(host.astype(np.int16) - dev.astype(np.int16))
        assert not d[~frag].any() and (not frag.any() or d[frag].max() <= 1)
        # ... and a bound's worth of disagreement, both ways
        for s in (exact - bound, exact + bound):
            far = pr.apply(pic, 4.0, 1.0, pr.log_average(s, FB))
            assert not (far != host)[~frag].any()


def test_the_pools_picture_gathered_is_the_frames(pl):
    cls, pick, pic = ps.state(pl, 91 * 60, ps.ALL, seed=5)
    assert np.array_equal(pr.apply(pl[1], 4.0, 0.25, 1.0)[pick], pr.apply(pic, 4.0, 0.25, 1.0))
    assert pr.terms(pl[1])[pick].tobytes() == pr.terms(pic).tobytes()


def test_poisoned_states(pl):
    for FB in (1, 7, 513 * 512):
        cls, pick, pic = ps.state(pl, FB, ps.ORDINARY_ONLY, seed=3)
        for p in ps.poison_positions(FB):
            t = pr.terms(ps.poisoned(pic, p))
            assert np.isnan(t[p]) and np.isnan(t).sum() == 1


# ---------------------------------------------------------------- the entry points without a GPU
def test_null_handle():
    from clive2_amd import _native
    _native.build()
    L = _native.lib()
    buf = np.zeros(16, np.float32)
    s = C.c_double(0.0)
    for kind in range(-1, 7):
        assert L.cl2_keep_picture(None, kind, 3, 2.0, 0.1, 0.1) == -1
    assert L.cl2_kept_picture(None) == 0
    assert L.cl2_write_picture(None, _native.ptr(buf), C.c_size_t(buf.size)) == -1
    assert L.cl2_read_picture(None, _native.ptr(buf), C.c_size_t(buf.size)) == -1
    assert L.cl2_picture_log_sum(None, C.byref(s)) == -1
    assert L.cl2_picture_tone_map(None, 4.0, 1.0, 1.0, _native.ptr(buf), C.c_size_t(buf.size)) == -1


def test_header_binding_and_library_agree_on_the_new_symbols():
    from clive2_amd import _native
    _native.build()
    text = open(os.path.join(ROOT, "include", "clive2_amd.h")).read()
    declared = set(re.findall(r"^int (cl2_[a-z_0-9]+)\(", text, flags=re.M))
    lib = C.CDLL(_native.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _native.EXPORTS and hasattr(lib, name), name
    assert lib.cl2_abi_version() == 6
    assert "const cl2_renderer* r" in text[text.index("int cl2_kept_picture("):].split(";")[0]


def test_python_surface():
    from clive2_amd.renderer import Renderer
    for name in ("keep_picture", "kept_picture", "load_picture", "picture_log_sum", "tone_mapped_picture"):
        assert callable(getattr(Renderer, name))
    assert isinstance(Renderer.kept_kind, property)
    assert Renderer._KEPT_KINDS == {"denoised": 1, "guided": 2, "robust": 3, "robust_guided": 4}
    r = Renderer.__new__(Renderer)                    # no handle: the argument checks come first
    r._h = None
    with pytest.raises(ValueError):
        r.keep_picture("image")
    with pytest.raises(TypeError):
        r.keep_picture("robust", iterations=2)
    with pytest.raises(TypeError):
        r.keep_picture("denoised", sigma_luma=2.0)


def test_cli_refusals(capsys):
    from clive2_amd import movie, render
    with pytest.raises(SystemExit) as e:
        movie.main(["--denoise", "--device-tonemap", "--host-tonemap"])
    assert e.value.code == 2 and "--device-tonemap does not go with --host-tonemap" in capsys.readouterr().err
    # the refusals that were there still come before any renderer is made, with the new flag present
    for mod in (movie, render):
        for argv in (["--device-tonemap", "--variance-guided"], ["--device-tonemap", "--robust", "--denoise"],
                     ["--device-tonemap", "--robust-denoise", "--robust"], ["--device-tonemap", "--robust", "2"]):
            with pytest.raises(SystemExit) as e:
                mod.main(argv)
            assert e.value.code == 2
    capsys.readouterr()
    for mod in (movie, render):
        with pytest.raises(SystemExit):
            mod.main(["--help"])
        text = "".join(capsys.readouterr().out.split())           # argparse wraps, also at hyphens
        assert "--device-tonemap" in text and "tone-mappedonthehostunless--device-tonemap" in text
        assert "tone-mappedonthehost)" not in text and "tone-mappedonthehost." not in text
