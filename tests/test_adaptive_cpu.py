"""CPU tests of adaptive sampling (csrc/adaptive.hpp): the numpy statement of its policy (quantisation,
systematic slot expansion, density from the error estimate), the new exports and the Python-level refusals."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_reference as ar  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["cl2_set_sample_density", "cl2_read_sample_density", "cl2_update_sample_density", "cl2_set_adaptive_sampling",
               "cl2_get_adaptive_sampling", "cl2_read_camera_samples"]


def _densities():
    rng = np.random.RandomState(7)
    yield np.ones(64 * 48, np.float32)
    yield rng.uniform(0.01, 10.0, 64 * 48).astype(np.float32)
    yield rng.lognormal(0.0, 2.0, 333).astype(np.float32)
    d = np.full(1000, 0.25, np.float32)
    d[:500] = 1.75
    yield d
    d = np.full(97, 1e-6, np.float32)
    d[3] = 1e6
    yield d


@pytest.mark.parametrize("k", range(5))
def test_quantisation_sums_exactly(k):
    m = list(_densities())[k]
    M = ar.quantise(m)
    assert M.dtype == np.uint64 and (M >= 1).all()
    assert int(M.sum(dtype=np.uint64)) == m.size << ar.SHIFT
    # the normalised density m' in units, less the unit reserved per pixel: M = 1 + m' (2^16 - 1) + (0 .. 2)
    mn = m.astype(np.float64) / m.astype(np.float64).mean()
    dev = M.astype(np.float64) - (1.0 + mn * (ar.UNIT - 1))
    assert dev.min() >= -1.0 - 1e-6 * mn.max() * ar.UNIT and dev.max() <= 2.0


def test_flat_density_is_the_identity_map():
    for FB in (1, 7, 64 * 48, 1920 * 1080):
        M = ar.quantise(np.ones(FB, np.float32))
        assert (M == ar.UNIT).all()
        C = ar.prefix(M)
        for p in (0, 1, 12345):
            for s in (0, 3):
                assert np.array_equal(ar.slot_map(C, ar.offset(p, s)), np.arange(FB))
        assert (ar.inv_density(M) == np.float32(1.0)).all()
    # a constant other than one quantises to the same
    assert (ar.quantise(np.full(300, 2.0, np.float32)) == ar.UNIT).all()


@pytest.mark.parametrize("k", range(1, 5))
def test_expansion_is_systematic_sampling(k):
    m = list(_densities())[k]
    M = ar.quantise(m)
    C = ar.prefix(M)
    FB = m.size
    lo_m, hi_m = M // np.uint64(ar.UNIT), (M + np.uint64(ar.UNIT - 1)) // np.uint64(ar.UNIT)
    for u in (0, 1, 777, 32768, ar.UNIT - 1):
        lo, hi = ar.ranges(C, u)
        n = hi - lo
        assert n.sum() == FB
        assert ((n >= lo_m.astype(np.int64)) & (n <= hi_m.astype(np.int64))).all()
        mp = ar.slot_map(C, u)
        assert len(mp) == FB and (np.diff(mp) >= 0).all()          # contiguous, raster order
        assert lo[0] == 0 and hi[-1] == FB


def test_expansion_mean_over_all_offsets_is_exact():
    for m in list(_densities())[1:4]:
        M = ar.quantise(m)
        C = ar.prefix(M)
        total = np.zeros(m.size, np.int64)
        prev = np.concatenate([np.zeros(1, np.uint64), C[:-1]])
        # sum over all 2^16 offsets of floor((C + u) / 2^16), per pixel, by whole units and the remainder
        def floor_sum(c):
            q, r = (c >> np.uint64(ar.SHIFT)).astype(np.int64), (c & np.uint64(ar.UNIT - 1)).astype(np.int64)
            return q * ar.UNIT + r                                     # #{u : r + u >= 2^16} = r
        total = floor_sum(C) - floor_sum(prev)
        assert np.array_equal(total, M.astype(np.int64))               # E_u[n_q] = M_q / 2^16 exactly
        # and a brute-force check on a few offsets agrees with the ranges
        u = np.arange(0, ar.UNIT, 4099)
        brute = sum((ar.ranges(C, int(x))[1] - ar.ranges(C, int(x))[0]) for x in u)
        assert brute.sum() == len(u) * m.size


def test_offsets_are_spread():
    us = np.array([ar.offset(p, s) for p in range(4096) for s in range(2)])
    assert us.min() >= 0 and us.max() < ar.UNIT
    hist = np.bincount(us >> 12, minlength=16)
    assert hist.min() > 0.7 * hist.mean() and hist.max() < 1.3 * hist.mean()
    assert ar.offset(0, 0) != ar.offset(0, 1) != ar.offset(1, 0)


def _synthetic(FB=12):
    rng = np.random.RandomState(3)
    acc = np.zeros((8, FB), np.float32)
    mom = np.zeros((8, FB), np.float32)
    for _ in range(6):
        x = rng.uniform(0.0, 2.0, (FB, 3)).astype(np.float32)
        w = rng.uniform(0.5, 1.5, FB).astype(np.float32)
        for c in range(3):
            acc[c] += x[:, c]
        acc[3] += w
        acc[7] += 1
        ar.add_moments(mom, x, w)
    return acc, mom


def test_density_formula_on_synthetic_moments():
    acc, mom = _synthetic()
    acc[3, 0] = 0.0                        # uncovered
    acc[7, 1] = 1.0                        # fewer than two addends: +inf, clipped
    mom[:, 2] = 0.0                        # a noiseless pixel: var 0
    for c in range(3):                     # ... exactly: x = I w
        mom[c, 2] = 0.0
    r = ar.terms(acc, mom, 0.001)
    assert r[0] == 0.0 and np.isinf(r[1]) and r[2] == 0.0
    fin = np.isfinite(r)
    mean = r[fin].astype(np.float64).mean()
    m = ar.density_from_terms(r, 0.25)
    assert m[0] == np.float32(0.25) and m[2] == np.float32(0.25)
    assert m[1] == np.float32(0.25 + 0.75 * ar.KAPPA)
    k = 5
    assert m[k] == np.float32(0.25 + 0.75 * (np.float64(r[k]) / mean))
    assert (m > 0).all()
    # a term above KAPPA mean is clipped
    r2 = np.ones(40, np.float32)
    r2[0] = 1e6
    m2 = ar.density_from_terms(r2, 0.5)
    mean2 = r2.astype(np.float64).sum() / 40
    assert m2[0] == np.float32(0.5 + 0.5 * ar.KAPPA)
    assert m2[1] == np.float32(0.5 + 0.5 / mean2)
    # beta = 1: uniform
    assert (ar.density_from_terms(r, 1.0) == 1.0).all()
    # no finite term
    assert ar.density_from_terms(np.full(4, np.inf, np.float32), 0.25) is None
    # all terms zero: flat
    assert (ar.density_from_terms(np.zeros(4, np.float32), 0.25) == 1.0).all()


def test_mapped_finalize_with_flat_density_is_the_uniform_finalize():
    """the restatement with one slot per pixel and 1/m = 1 performs the uniform finalize's float operations"""
    rng = np.random.RandomState(11)
    W, H = 5, 4
    FB = W * H
    agg = rng.uniform(0, 1, (13, FB)).astype(np.float32)
    uni = rng.uniform(0, 1, (FB, 4)).astype(np.float32)
    light = rng.uniform(0, 1, (FB, 4)).astype(np.float32)
    M = ar.quantise(np.ones(FB, np.float32))
    acc = np.zeros((8, FB), np.float32)
    n = ar.finalize_accumulate(agg, light, uni, acc, None, ar.prefix(M), ar.inv_density(M), 5, W, H)
    assert (n == 1).all()
    for p in range(FB):
        t = np.zeros(3, np.float32)
        ws = np.float32(0)
        for i in (-1, 0, 1):
            for j in (-1, 0, 1):
                sx, sy = p % W + i, p // W + j
                if 0 <= sx < W and 0 <= sy < H:
                    k = sy * W + sx
                    wt = agg[(1 - i) * 3 + (1 - j), k]
                    t = (t + wt * agg[9:12, k]).astype(np.float32)
                    ws = np.float32(ws + wt * agg[12, k])
        assert np.array_equal(acc[:3, p], t + light[p, :3])
        assert acc[3, p] == np.float32(ws + light[p, 3])
        assert np.array_equal(acc[4:7, p], uni[p, :3]) and acc[7, p] == 1.0


def test_new_exports_are_listed_and_declared():
    from clive2_amd import _native
    for name in NEW_EXPORTS:
        assert name in _native.EXPORTS
    header = open(os.path.join(ROOT, "include", "clive2_amd.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\(" % name, header), name


def test_new_exports_are_in_the_library():
    from clive2_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built")
    import ctypes
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW_EXPORTS:
        assert hasattr(L, name), name


class _Stub:
    """just enough of a Renderer for the argument checks that run before any library call"""
    batch_size = 12
    streams = 1
    pixel_width, pixel_height = 4, 3


def test_python_refusals():
    from clive2_amd.renderer import Renderer
    r = _Stub()
    r._uniform_share = Renderer._uniform_share.__get__(r)
    r.UNIFORM_SHARE = Renderer.UNIFORM_SHARE
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            Renderer.update_sample_density(r, uniform_share=bad)
        with pytest.raises(ValueError):
            Renderer.render_until(r, 0.05, 10, adaptive=True, uniform_share=bad)
    with pytest.raises(ValueError):
        Renderer.update_sample_density(r, floor=-1.0)
    with pytest.raises(ValueError):
        Renderer.render_until(r, 0.05, 10, min_samples=1, adaptive=True)
    for bad in (np.ones(11), np.zeros(12), np.full(12, np.nan), np.full(12, np.inf), -np.ones(12)):
        with pytest.raises(ValueError):
            Renderer.set_sample_density(r, bad)


@pytest.mark.parametrize("module", ["clive2_amd.render", "clive2_amd.movie"])
def test_cli_refuses_adaptive_without_target(module, capsys):
    import importlib
    mod = importlib.import_module(module)
    with pytest.raises(SystemExit):
        mod.main(["--scene", "empty", "--adaptive"])
    assert "--adaptive needs --target-error" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mod.main(["--scene", "empty", "--target-error", "0.05", "--adaptive", "--uniform-share", "0"])
    assert "--uniform-share" in capsys.readouterr().err
