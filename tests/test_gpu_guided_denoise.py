"""The variance-guided denoiser on the device (csrc/denoise_guided.hpp, cl2_denoise_guided): the kernels against their numpy
statement (tests/guided_denoise_reference.py) on renders and on injected accumulator / moment states, that the call leaves the
render alone, its refusals, sample streams and a sample density, and the gain in picture quality at 4 and at 256 passes."""
import ctypes as C

import numpy as np
import pytest

import error_reference as er
import error_states as es
import guided_denoise_reference as gr
from test_gpu_denoise import _cornell, _glass, _open_scene

pytestmark = pytest.mark.gpu

F = np.float32
SIGMAS = [dict(sigma_luma=4.0, sigma_depth=0.1, sigma_albedo=0.1), dict(sigma_luma=0.7, sigma_depth=0.02, sigma_albedo=0.3),
          dict(sigma_luma=30.0, sigma_depth=1.0, sigma_albedo=0.05)]


def _renderer(scene, K=1, seed=20240928, mode=None, tracking=True):
    from clive2_amd.renderer import Renderer, stream_seeds
    r = Renderer(scene, streams=K)
    r.set_seeds(stream_seeds(r.batch_size, K, seed=seed))
    if mode is not None:
        r.set_traversal_mode(mode)
    if tracking:
        r.set_error_tracking(True)
    return r


def _compare(r, c, v, f, label, **kw):
    """guided_radiance(return_variance=True) against the restatement fed with c, v and the features f"""
    got, gv = r.guided_radiance(return_variance=True, **kw)
    want, wv = gr.denoise(c, v, f["normal"], f["depth"], f["albedo"], f["coverage"], **kw)
    assert np.isfinite(got).all() and np.isfinite(gv).all(), label
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6, err_msg=label)
    np.testing.assert_allclose(gv, wv, rtol=1e-4, atol=1e-6 * float(v.max()), err_msg=label + " (variance)")
    assert r.guided_radiance(**kw).tobytes() == got.tobytes()               # the same picture without the variance
    return got, gv


@pytest.mark.parametrize("name,mode", [("cornell", None), ("open", 5)])
def test_kernel_equals_the_specification(name, mode):
    W, H = 70, 45                               # partial 16 x 16 tiles on both edges
    scene = {"cornell": _cornell, "open": _open_scene}[name](W, H)
    r = _renderer(scene, mode=mode)
    if mode == 5:
        assert r.organisation()["wide_nodes"] > 0
    r.run_samples(3)
    r.render_features(2)
    f = r.features()
    c = r.radiance
    acc, mom = r.packed_accumulators(), r.moments()
    v = gr.input_variance(acc, mom, H, W)
    assert (v > 0).any()
    if name == "open":
        assert (f["coverage"] == 0).any()
    for sig in SIGMAS:
        for it in (1, 5):
            _compare(r, c, v, f, f"{sig} iterations {it}", iterations=it, **sig)
    got, gv = r.guided_radiance(iterations=0, return_variance=True)
    assert got.tobytes() == c.tobytes()
    state, var, _ = er.variances(acc, mom)
    assert (state == 2).all() or name == "open"
    ok = state == 2
    assert gv.reshape(-1)[ok].tobytes() == var[ok, 3].astype(F).tobytes()
    assert gv.tobytes() == v.tobytes()
    r.close()


# ---------------------------------------------------------------- injected states
@pytest.fixture(scope="module")
def pool():
    return es.pool()


@pytest.mark.parametrize("W,H,iterations", [(41, 25, 3), (512, 513, 3), (1920, 1080, 5)])
def test_injected_states_equal_the_restatement(W, H, iterations, pool):
    """Every class of error_states (uncovered pixels with NaN / inf moments, n = 0 and 1, overflowed sums, subnormals, variances
    beyond float32) under the features of the Cornell box at the same frame: finite everywhere and equal to the restatement.  At
    1920 x 1080 five passes, so that the global-load pass runs at steps 4, 8 and 16 across tile and frame edges."""
    r = _renderer(_cornell(W, H))
    FB = W * H
    cls, acc, mom = es.state(pool, FB, es.ALL)
    assert set(np.unique(cls)) == set(es.ALL)
    r.load_packed_accumulators(acc)
    r.load_moments(mom)
    r.render_features(1)
    f = r.features()
    c = r.radiance
    assert np.isfinite(c).all()
    v = gr.input_variance(acc, mom, H, W)
    assert (v == gr.CAP).any() and (v == 0).any()
    got0, gv0 = r.guided_radiance(iterations=0, return_variance=True)
    np.testing.assert_allclose(got0, c, rtol=1e-4, atol=1e-6)
    assert gv0.tobytes() == v.tobytes()
    _compare(r, c, v, f, f"{W} x {H}", iterations=iterations)
    r.close()


@pytest.mark.parametrize("name,mode", [("cornell", 0), ("open", 5)])
def test_render_state_is_untouched(name, mode):
    from clive2_amd.renderer import Renderer, make_seeds
    W, H = 64, 48
    scene = {"cornell": _cornell, "open": _open_scene}[name](W, H)
    S = make_seeds(W * H, seed=5)
    a, b = Renderer(scene, seeds=S), Renderer(scene, seeds=S)
    for x in (a, b):
        x.set_reproducible(True)
        x.set_traversal_mode(mode)
        x.set_error_tracking(True)
        if mode == 5:
            x.set_counting(2)
    a.run_samples(2)
    b.run_samples(1)
    b.render_features(4)
    b.guided_radiance(return_variance=True)
    b.guided_image
    b.run_samples(1)
    assert a.packed_accumulators().tobytes() == b.packed_accumulators().tobytes()
    assert a.moments().tobytes() == b.moments().tobytes()
    assert a.get_random_buffer().tobytes() == b.get_random_buffer().tobytes()
    assert a.counters() == b.counters()
    assert a.walk_tallies() == b.walk_tallies()
    a.close(); b.close()


def test_state_errors():
    from clive2_amd.renderer import RendererError
    from clive2_amd._native import ptr
    scene = _cornell(32, 24)
    r = _renderer(scene, tracking=False)
    r.run_samples(2)
    r.render_features(1)
    with pytest.raises(RendererError, match=r"\(-3\)"):          # tracking off
        r.guided_radiance()
    r.set_error_tracking(True)
    with pytest.raises(RendererError, match=r"\(-3\)"):          # switched on after samples: moments invalid
        r.guided_radiance()
    r.reset_accumulators()
    r.run_samples(2)
    img = r.guided_radiance()
    assert img.shape == (24, 32, 3) and img.dtype == F
    assert r.guided_image.dtype == np.uint8 and r.guided_image.shape == (24, 32, 3)
    acc, mom = r.packed_accumulators(), r.moments()
    r.load_packed_accumulators(acc)                              # accumulators without their moments
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.guided_radiance()
    r.load_moments(mom)
    assert r.guided_radiance().tobytes() == img.tobytes()
    r.upload_scene(scene)                                        # the features describe the scene they were rendered from
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.guided_radiance()
    r.render_features(1)
    r.guided_radiance()
    out, var = np.empty(3 * 32 * 24, F), np.empty(32 * 24, F)
    L, h = r._L, r._h
    for args in ((1, -1.0, 0.1, 0.1, ptr(out), out.size, None, 0),                  # a negative sigma
                 (1, 4.0, 0.0, 0.1, ptr(out), out.size, None, 0),
                 (1, 4.0, 0.1, float("nan"), ptr(out), out.size, None, 0),
                 (1, float("inf"), 0.1, 0.1, ptr(out), out.size, None, 0),
                 (1, 4.0, 0.1, 1e-23, ptr(out), out.size, None, 0),                 # sigma_albedo^2 underflows to 0
                 (0, 4.0, 0.1, 1e-23, ptr(out), out.size, None, 0),
                 (1, 4.0, 0.1, 1e-19, ptr(out), out.size, None, 0),                 # ... to a subnormal (FLT_MIN = 1.1755e-38)
                 (1, 4.0, 0.1, 0.1, ptr(out), out.size, ptr(var), var.size - 1),    # a wrong n_var
                 (1, 4.0, 0.1, 0.1, ptr(out), out.size, None, var.size),
                 (1, 4.0, 0.1, 0.1, ptr(out), out.size - 1, None, 0),
                 (1, 4.0, 0.1, 0.1, None, 0, None, 0),
                 (-1, 4.0, 0.1, 0.1, ptr(out), out.size, None, 0),
                 (13, 4.0, 0.1, 0.1, ptr(out), out.size, None, 0)):
        with pytest.raises(RendererError, match=r"\(-1\)"):
            r._check(L.cl2_denoise_guided(h, *args[:5], C.c_size_t(args[5]), args[6], C.c_size_t(args[7])), "cl2_denoise_guided")
    assert L.cl2_denoise_guided(h, 12, 4.0, 0.1, 0.1, ptr(out), C.c_size_t(out.size), ptr(var), C.c_size_t(var.size)) == 0
    assert L.cl2_denoise_guided(h, 12, 1e-23, 0.1, 1.1e-19, ptr(out), C.c_size_t(out.size), None, C.c_size_t(0)) == 0   # 1.21e-38
    r.close()


def test_streams_and_density():
    """K = 4 sample streams on the mesh scene, then one run with a fixed 1.75 / 0.25 density: the moments are valid in both, the
    call succeeds and equals the restatement fed with packed_accumulators() / moments()."""
    W, H = 72, 40
    r = _renderer(_open_scene(W, H), K=4, mode=5)
    r.run_samples(2)
    r.render_features(2)
    f = r.features()
    acc, mom = r.packed_accumulators(), r.moments()
    assert acc.reshape(8, -1)[7].max() == 8                       # 2 passes x 4 streams
    _compare(r, r.radiance, gr.input_variance(acc, mom, H, W), f, "K = 4")
    r.close()
    r = _renderer(_cornell(W, H))
    d = np.full((H, W), 0.25, F)
    d[:, : W // 2] = 1.75
    r.set_sample_density(d)
    r.run_samples(4)
    r.render_features(2)
    acc, mom = r.packed_accumulators(), r.moments()
    _compare(r, r.radiance, gr.input_variance(acc, mom, H, W), r.features(), "density")
    r.close()


def _rmse(x, ref):
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2)))


@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_it_denoises_and_is_consistent(name):
    """256 x 192, defaults, against 1024 samples of seed 4321.  At 4 passes the guided picture's relative MSE is at most half the
    raw picture's and at most the fixed filter's; at 256 passes it is at most the raw picture's (the fixed filter's, printed, is
    not: it blurs a converged picture as much as a noisy one).  Measured on the MI355X, raw / fixed / guided: Cornell box 2.13e-4 /
    6.17e-5 / 1.99e-5 at 4 passes and 4.22e-6 / 5.91e-5 / 1.62e-6 at 256; glass scene 8.60e-3 / 2.25e-3 / 1.77e-3 and 1.65e-3 /
    4.96e-4 / 2.20e-4."""
    from clive2_amd.renderer import Renderer, make_seeds
    W, H = 256, 192
    scene = {"cornell": _cornell, "glass": _glass}[name](W, H)
    ref_r = Renderer(scene, seeds=make_seeds(W * H, seed=4321))
    ref_r.run_samples(1024)
    ref = ref_r.radiance
    ref_r.close()
    r = Renderer(scene)
    r.set_error_tracking(True)
    r.render_features(4)
    figures = {}
    for n in (4, 256):
        r.run_samples(n - r.samples)
        raw, fixed, guided = r.radiance, r.denoised_radiance(), r.guided_radiance()
        figures[n] = e = (_rmse(raw, ref), _rmse(fixed, ref), _rmse(guided, ref))
        print(f"{name} {n} passes: rMSE raw {e[0]:.4g} fixed {e[1]:.4g} guided {e[2]:.4g} (guided / raw {e[2] / e[0]:.3f}, "
              f"guided / fixed {e[2] / e[1]:.3f})")
    raw, fixed, guided = figures[4]
    assert guided <= 0.5 * raw
    assert guided <= fixed
    raw, fixed, guided = figures[256]
    assert guided <= raw
    img = r.guided_image
    assert img.dtype == np.uint8 and img.shape == (H, W, 3)
    r.close()


def test_cli_variance_guided_writes_a_png(tmp_path):
    from clive2_amd import render
    out = tmp_path / "g.png"
    assert render.main(["--scene", "empty", "--width", "64", "--height", "48", "--samples", "4", "--denoise", "--variance-guided",
                        "--out", str(out)]) == 0
    assert out.exists() or (tmp_path / "g.png.npy").exists()
