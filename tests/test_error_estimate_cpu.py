"""The error estimate's statement (tests/error_reference.py, what csrc/error_estimate.hpp is checked against on the GPU) on
synthetic samples with a known answer, the library's new C surface without a GPU, and the render CLI's refusals.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import error_reference as er

F = np.float32
NEW_CALLS = ("cl2_set_error_tracking", "cl2_get_error_tracking", "cl2_read_moments_packed", "cl2_write_moments_packed",
             "cl2_read_standard_error", "cl2_relative_error", "cl2_run_until")


def _trials(T, n, seed, rho=0.6, mu=(0.3, 0.5, 0.8), sigma=0.4):
    """T independent pixels of n iid addends each: w > 0 (gamma), x_c = w (mu_c + sigma z_c) with z_c correlated with w."""
    rs = np.random.RandomState(seed)
    w = rs.gamma(4.0, 0.25, size=(n, T))
    wz = (w - 1.0) / 0.5
    xs, ws = [], []
    for i in range(n):
        z = rho * wz[i][:, None] + np.sqrt(1 - rho * rho) * rs.standard_normal((T, 3))
        x = w[i][:, None] * (np.asarray(mu)[None, :] + sigma * z)
        xs.append(x.astype(F))
        ws.append(w[i].astype(F))
    acc = np.zeros((8, T), F)
    for x, wi in zip(xs, ws):
        acc[:3] = (acc[:3] + x.T).astype(F)
        acc[3] = (acc[3] + wi).astype(F)
        acc[7] = (acc[7] + F(1)).astype(F)
    return acc, er.moments_of(xs, ws)


def test_predicted_variance_matches_the_spread_of_the_ratio():
    """Mean delta-method variance over 20,000 trials of 64 addends vs the empirical variance of sum(x) / sum(w) across them:
    within 5 % for b, g, r and luma (the sampling error of an empirical variance over 20,000 trials is about 1 %)."""
    acc, mom = _trials(20000, 64, seed=3)
    state, var, L = er.variances(acc, mom)
    assert (state == 2).all()
    I = acc[:3].astype(np.float64) / acc[3].astype(np.float64)
    emp = [I[c].var(ddof=1) for c in range(3)] + [L.var(ddof=1)]
    pred = var.mean(axis=0)
    np.testing.assert_allclose(pred, emp, rtol=0.05)


def test_uncorrelated_weights_and_a_second_seed():
    acc, mom = _trials(20000, 64, seed=11, rho=0.0, mu=(1.0, 0.2, 0.05), sigma=0.8)
    _, var, L = er.variances(acc, mom)
    I = acc[:3].astype(np.float64) / acc[3].astype(np.float64)
    emp = [I[c].var(ddof=1) for c in range(3)] + [L.var(ddof=1)]
    np.testing.assert_allclose(var.mean(axis=0), emp, rtol=0.05)


def _pixels(addends):
    """acc, mom of pixels given as lists of (x (3,), w) addends each."""
    n = len(addends)
    acc, mom = np.zeros((8, n), F), np.zeros((8, n), F)
    for p, seq in enumerate(addends):
        for x, w in seq:
            x = np.asarray(x, F).reshape(1, 3)
            w = np.asarray([w], F)
            acc[:3, p] = (acc[:3, p] + x[0]).astype(F)
            acc[3, p] = (acc[3, p] + w[0]).astype(F)
            acc[7, p] = (acc[7, p] + F(1)).astype(F)
            m = mom[:, p:p + 1].copy()
            er.add_moments(m, x, w)
            mom[:, p] = m[:, 0]
    return acc, mom


def test_edge_cases():
    acc, mom = _pixels([
        [((1.0, 2.0, 3.0), 1.0)],                                   # one addend: inf
        [((0.0, 0.0, 0.0), 0.0)] * 3,                               # no weight: uncovered, 0
        [((0.5, 0.25, 0.125), 2.0)] * 4,                            # a constant pixel: 0
        [((0.5, 0.25, 0.125), 2.0), ((1.5, 0.75, 0.375), 2.0)],     # a noisy one
    ])
    se = er.standard_error(acc, mom)
    assert np.isinf(se[0]).all()
    assert (se[1] == 0).all()
    assert (se[2, :3] == 0).all()
    # luma: y is the float32 luma of each addend, L the float64 luma of the mean -- they differ in the last bits, which leaves
    # a rounding-sized remainder, not a noise estimate
    assert se[2, 3] < 1e-4 * er.variances(acc[:, 2:3], mom[:, 2:3])[2][0]
    assert (se[3] > 0).all() and np.isfinite(se[3]).all()
    assert er.relative_error(acc, mom, 0.05) == np.inf               # a covered pixel with n < 2
    e = er.relative_error(acc[:, 1:], mom[:, 1:], 0.05)             # uncovered pixel left out: N = 2
    state, var, L = er.variances(acc[:, 2:], mom[:, 2:])
    assert e == pytest.approx(np.sqrt((var[:, 3] / (L + 0.05) ** 2).sum() / 2), rel=1e-12)
    assert er.relative_error(acc[:, 1:2], mom[:, 1:2], 0.05) == np.inf    # nothing covered
    # non-finite weight sums are uncovered too
    acc2 = acc.copy()
    acc2[3, 3] = np.inf
    assert (er.standard_error(acc2, mom)[3] == 0).all()


def test_the_clamp_absorbs_cancellation():
    """A bright, nearly noiseless pixel: the raw-moment form of S cancels to a rounding remainder, which the clamp keeps >= 0."""
    seq = [((1000.0 + 1e-4 * k, 1000.0, 1000.0), 1.0) for k in range(64)]
    acc, mom = _pixels([seq])
    state, var, _ = er.variances(acc, mom)
    assert state[0] == 2 and (var >= 0).all() and np.isfinite(var).all()


@pytest.fixture(scope="module")
def native_lib():
    from clive2_amd import _native
    _native.build()
    return _native.lib()


def test_library_exports_the_error_calls(native_lib):
    from clive2_amd import _native
    for name in NEW_CALLS:
        assert hasattr(native_lib, name) and name in _native.EXPORTS


def test_error_calls_refuse_a_null_handle(native_lib):
    L = native_lib
    INVALID = -1
    buf = np.zeros(64, F)
    d, i = C.c_double(0), C.c_int(0)
    assert L.cl2_set_error_tracking(None, 1) == INVALID
    assert L.cl2_get_error_tracking(None) == INVALID
    assert L.cl2_read_moments_packed(None, buf.ctypes.data_as(C.c_void_p), 64) == INVALID
    assert L.cl2_write_moments_packed(None, buf.ctypes.data_as(C.c_void_p), 64) == INVALID
    assert L.cl2_read_standard_error(None, buf.ctypes.data_as(C.c_void_p), 64) == INVALID
    assert L.cl2_relative_error(None, 0.05, C.byref(d)) == INVALID
    assert L.cl2_run_until(None, 0.05, 0.05, 0, 8, 8, C.byref(i), C.byref(d)) == INVALID


@pytest.mark.parametrize("argv", [
    ["--target-error", "0"],
    ["--target-error", "-0.1"],
    ["--target-error", "nan"],
    ["--target-error", "0.05", "--check-every", "0"],
    ["--target-error", "0.05", "--error-floor", "-1"],
])
def test_render_cli_refuses_bad_error_arguments(argv, monkeypatch):
    from clive2_amd import render

    def no_renderer(*a, **k):
        raise AssertionError("a renderer was made before the arguments were checked")
    monkeypatch.setattr(render, "Renderer", no_renderer)
    monkeypatch.setattr(render, "create_scene_from_preset", no_renderer)
    with pytest.raises(SystemExit) as e:
        render.main(argv + ["--width", "16", "--height", "16"])
    assert e.value.code == 2


def test_render_cli_refuses_target_error_with_ranks(monkeypatch, capsys):
    from clive2_amd import render

    def no_renderer(*a, **k):
        raise AssertionError("a renderer was made before the arguments were checked")
    monkeypatch.setattr(render, "Renderer", no_renderer)
    monkeypatch.setattr(render, "create_scene_from_preset", no_renderer)
    monkeypatch.setattr(render, "rank_info", lambda: (0, 0, 2))
    with pytest.raises(SystemExit):
        render.main(["--target-error", "0.05"])
    assert "single rank" in capsys.readouterr().err
