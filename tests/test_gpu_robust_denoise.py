"""The guided filter on the robust picture on the device (csrc/denoise_robust.hpp, cl2_denoise_robust): the input kernel against its
numpy restatement (tests/robust_denoise_reference.py) bit for bit on injected bucket states, the passes that follow on the same
states under injected features, a real render, the state rules, that the call leaves the render alone, the gain in picture quality
and the CLI."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import feature_states as fs
import guided_denoise_reference as gr
import robust_denoise_reference as rd
import robust_states as rst
from denoise_scenes import cornell as _cornell, glass as _glass

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _renderer(scene, K=1, M=8, seed=20240928, tracking=False):
    from clive2_amd.renderer import Renderer, stream_seeds
    r = Renderer(scene, streams=K)
    r.set_seeds(stream_seeds(r.batch_size, K, seed=seed))
    r.set_reproducible(True)
    if tracking:
        r.set_error_tracking(True)
    if M:
        r.set_robust_buckets(M)
    return r


# ---------------------------------------------------------------- injected states
@pytest.fixture(scope="module")
def pools():
    """per M: the pool of pixel states and the restatement's input (c, v) of every one of them, computed once (the input is a
    function of the pixel's buckets alone, so a frame's reference is the pool's, gathered)"""
    made = {}

    def get(M):
        if M not in made:
            pl = rst.pool(M)
            made[M] = (pl,) + rd.input_state(pl[2])
        return made[M]
    return get


@pytest.fixture(scope="module")
def handles():
    made = {}

    def get(W, H):
        if (W, H) not in made:
            made[W, H] = _renderer(_cornell(W, H), 1, 0)
        return made[W, H]
    yield get
    for r in made.values():
        r.close()


def _inject(r, pl, W, H, M):
    """the state robust_states.state(pl, W * H) on the handle: packed accumulators whose row 7 is a7 (which invalidates the
    buckets), then the buckets (which makes them valid), under the features of feature_states"""
    FB = W * H
    cls, pick = rst.picks(pl, FB)
    a7, bkt = np.ascontiguousarray(pl[1][pick]), np.ascontiguousarray(pl[2][:, :, pick])
    acc = np.zeros((8, FB), F)
    acc[7] = a7
    r.set_robust_buckets(M)
    r.load_packed_accumulators(acc)
    r.load_buckets(bkt)
    f = fs.features(W, H)[1:]
    r.load_features(*f)
    return cls, pick, f


@pytest.mark.parametrize("W,H,M", [(7, 5, 3), (7, 5, 8), (7, 5, 16), (41, 25, 3), (41, 25, 8), (41, 25, 16), (1920, 1080, 16)])
def test_input_kernel_bitwise(W, H, M, pools, handles):
    """Every class of tests/robust_states.py: with iterations = 0 the picture's bytes are robust_radiance()'s and the restatement's,
    and v's bytes are the restatement's, no pixel excluded.  At 1920 x 1080 with M = 16 the bucket byte offsets pass 2^31 (531 MB);
    7 x 5 is below a workgroup, 41 x 25 has a partial last one."""
    pl, ref_c, ref_v = pools(M)
    FB = W * H
    r = handles(W, H)
    cls, pick, _ = _inject(r, pl, W, H, M)
    if FB >= 64:
        assert set(np.unique(cls)) == set(rst.ALL)
    pic, v = r.robust_guided_radiance(iterations=0, return_variance=True)
    assert pic.shape == (H, W, 3) and v.shape == (H, W) and pic.dtype == v.dtype == np.float32
    want_c, want_v = ref_c[pick], ref_v[pick]
    same = (pic.reshape(FB, 3).view(np.uint32) == want_c.view(np.uint32)).all(1) & (v.reshape(FB).view(np.uint32) == want_v.view(np.uint32))
    bad = np.flatnonzero(~same)
    assert bad.size == 0, [(int(p), rst.NAMES[cls[p]], pic.reshape(FB, 3)[p], want_c[p], v.reshape(FB)[p], want_v[p]) for p in bad[:5]]
    assert pic.tobytes() == r.robust_radiance().tobytes()
    assert np.isfinite(pic).all() and np.isfinite(v).all()
    assert r.robust_guided_radiance(iterations=0).tobytes() == pic.tobytes()  # without the variance: the same picture
    r.set_robust_buckets(0)


def _compare(r, c, v, f, label, **kw):
    """robust_guided_radiance(return_variance=True) against the restatement's passes fed with c, v and the features f: the
    convention of tests/test_gpu_guided_denoise.py"""
    got, gv = r.robust_guided_radiance(return_variance=True, **kw)
    want, wv = gr.denoise(c, v, *f, **kw)
    assert np.isfinite(got).all() and np.isfinite(gv).all(), label
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6, err_msg=label)
    # The convention's atol scales with the largest input variance.  On the injected states that is the cap, 2^100, so there this line
    # checks only the v' near the cap; v' after the passes is checked in earnest on the real render, where v.max() is small, and
    # the input v bit for bit in test_input_kernel_bitwise.
    np.testing.assert_allclose(gv, wv, rtol=1e-4, atol=1e-6 * float(v.max()), err_msg=label + " (variance)")
    assert r.robust_guided_radiance(**kw).tobytes() == got.tobytes()          # the same picture without the variance
    return got, gv


@pytest.mark.parametrize("W,H,iterations", [(41, 25, 1), (41, 25, 3), (512, 513, 5)])
def test_passes_on_injected_states(W, H, iterations, pools, handles):
    """The same states (M = 8) under the features of tests/feature_states.py: finite everywhere and equal to the restatement at
    rtol 1e-4, atol 1e-6, no pixel and no class excluded.  512 x 513 with five passes runs the global-load pass at steps 4, 8 and 16
    across tile and frame edges.  On the CPU the float32 restatement stays within 0.19 of this tolerance of its float64 companion
    at 512 x 513 (0.10 and 0.07 at 41 x 25 with 1 and 3 passes), no pixel of any class beyond it."""
    pl, ref_c, ref_v = pools(8)
    r = handles(W, H)
    cls, pick, f = _inject(r, pl, W, H, 8)
    assert set(np.unique(cls)) == set(rst.ALL)
    c, v = ref_c[pick].reshape(H, W, 3), ref_v[pick].reshape(H, W)
    assert (v == gr.CAP).any() and (v == 0).any()
    _compare(r, c, v, f, f"{W} x {H}, {iterations} passes", iterations=iterations)
    r.set_robust_buckets(0)


# ---------------------------------------------------------------- a real render
@pytest.mark.parametrize("K", [1, 2])
def test_a_real_render_equals_the_restatement(K):
    W, H, M = 70, 45, 8                         # partial 16 x 16 tiles on both edges
    r = _renderer(_cornell(W, H), K, M)
    r.run_samples(3)
    r.render_features(2)
    ft = r.features()
    f = (ft["normal"], ft["depth"], ft["albedo"], ft["coverage"])
    bkt = r.buckets().reshape(M, 4, -1)
    c, v = rd.input_state(bkt, H, W)
    assert (v > 0).any() and np.isfinite(v).all()
    got0, v0 = r.robust_guided_radiance(iterations=0, return_variance=True)
    assert got0.tobytes() == r.robust_radiance().tobytes() == c.tobytes()
    assert v0.tobytes() == v.tobytes()
    for it in (1, 5):
        _compare(r, c, v, f, f"K = {K}, {it} passes", iterations=it)
    img = r.robust_guided_image
    assert img.dtype == np.uint8 and img.shape == (H, W, 3)
    r.close()


# ---------------------------------------------------------------- state rules
def test_state_rules():
    from clive2_amd.renderer import RendererError
    from clive2_amd._native import ptr
    scene = _cornell(32, 24)
    r = _renderer(scene, M=0)                                    # error tracking is off throughout
    assert not r.error_tracking
    r.run_samples(2)
    r.render_features(1)
    with pytest.raises(RendererError, match=r"\(-3\).*buckets are off"):
        r.robust_guided_radiance()
    r.set_robust_buckets(8)                                      # switched on over accumulators that hold sums
    with pytest.raises(RendererError, match=r"\(-3\).*cl2_reset_accumulators or cl2_write_buckets_packed"):
        r.robust_guided_radiance()
    r.reset_accumulators()
    r.run_samples(2)
    img = r.robust_guided_radiance()
    assert img.shape == (24, 32, 3) and img.dtype == F and np.isfinite(img).all() and img.any()
    acc, bkt = r.packed_accumulators(), r.buckets()
    r.load_packed_accumulators(acc)                              # accumulators without their buckets
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.robust_guided_radiance()
    r.load_buckets(bkt)
    assert r.robust_guided_radiance().tobytes() == img.tobytes()
    r.upload_scene(scene)                                        # the features describe the scene they were rendered from
    with pytest.raises(RendererError, match=r"\(-3\).*features"):
        r.robust_guided_radiance()
    r.render_features(1)
    assert r.robust_guided_radiance().tobytes() == img.tobytes()
    out, var = np.empty(3 * 32 * 24, F), np.empty(32 * 24, F)
    L, h = r._L, r._h
    for args in ((1, -1.0, 0.1, 0.1, ptr(out), out.size, None, 0),                  # a negative sigma
                 (1, 4.0, 0.0, 0.1, ptr(out), out.size, None, 0),
                 (1, 4.0, 0.1, float("nan"), ptr(out), out.size, None, 0),
                 (1, float("inf"), 0.1, 0.1, ptr(out), out.size, None, 0),
                 (1, 4.0, 0.1, 1e-23, ptr(out), out.size, None, 0),                 # sigma_albedo^2 underflows to 0
                 (0, 4.0, 0.1, 1e-23, ptr(out), out.size, None, 0),
                 (1, 4.0, 0.1, 1e-19, ptr(out), out.size, None, 0),                 # ... to a subnormal
                 (1, 4.0, 0.1, 0.1, ptr(out), out.size, ptr(var), var.size - 1),    # a wrong n_var
                 (1, 4.0, 0.1, 0.1, ptr(out), out.size, None, var.size),
                 (1, 4.0, 0.1, 0.1, ptr(out), out.size - 1, None, 0),
                 (1, 4.0, 0.1, 0.1, None, 0, None, 0),
                 (-1, 4.0, 0.1, 0.1, ptr(out), out.size, None, 0),
                 (13, 4.0, 0.1, 0.1, ptr(out), out.size, None, 0)):
        with pytest.raises(RendererError, match=r"\(-1\)"):
            r._check(L.cl2_denoise_robust(h, *args[:5], C.c_size_t(args[5]), args[6], C.c_size_t(args[7])), "cl2_denoise_robust")
    assert L.cl2_denoise_robust(h, 12, 4.0, 0.1, 0.1, ptr(out), C.c_size_t(out.size), ptr(var), C.c_size_t(var.size)) == 0
    assert np.isfinite(out).all() and np.isfinite(var).all()
    assert r.robust_guided_radiance().tobytes() == img.tobytes()                    # the refused calls changed nothing
    r.close()


def test_render_state_is_untouched():
    """Two handles with the same seeds, two passes each; one of them renders features and calls the filter between the passes:
    accumulators, buckets, seeds and counters come out byte for byte the same, and the features are what they were before the call."""
    scene = _cornell(64, 48)
    a, b = _renderer(scene, 2), _renderer(scene, 2)
    a.run_samples(2)
    b.run_samples(1)
    b.render_features(4)
    acc, bkt, feat = b.packed_accumulators(), b.buckets(), b.features()
    b.robust_guided_radiance(return_variance=True)
    b.robust_guided_radiance(iterations=0)
    b.robust_guided_image
    assert b.packed_accumulators().tobytes() == acc.tobytes() and b.buckets().tobytes() == bkt.tobytes()
    after = b.features()
    assert all(after[k].tobytes() == feat[k].tobytes() for k in feat)
    b.run_samples(1)
    assert a.packed_accumulators().tobytes() == b.packed_accumulators().tobytes()
    assert a.buckets().tobytes() == b.buckets().tobytes()
    assert a.get_random_buffer().tobytes() == b.get_random_buffer().tobytes()
    assert a.counters() == b.counters()
    assert a.robust_radiance().tobytes() == b.robust_radiance().tobytes()
    a.close(); b.close()


# ---------------------------------------------------------------- quality
def _rmse(x, ref):                                   # tests/test_gpu_denoise.py
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2)))


def _measured(scene, passes):
    """the row of profiles/robust_denoise_quality_mi355x.json (tools/robust_denoise_quality.py on the MI355X)"""
    with open(os.path.join(ROOT, "profiles", "robust_denoise_quality_mi355x.json")) as f:
        runs = json.load(f)["runs"]
    return next(r for r in runs if r["scene"] == scene and r["passes"] == passes)


@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_quality_on_real_renders(name):
    """256 x 192, M = 8, defaults, relative MSE (_rmse) against 1024 passes of seed 4321.  Both scenes at 4 and 256 passes: new <=
    raw.  Cornell box at 64 and 256 passes: new <= 1.25 x the ratio to guided that tools/robust_denoise_quality.py measured on the
    MI355X x guided (one seed's figure of a noisy quantity, hence the quarter).

    The feature's claim -- glass scene at 256 passes: new <= min(robust, guided) -- did NOT hold on the MI355X and is therefore not
    asserted: measured there raw 1.65e-3, robust 2.11e-4, guided 2.20e-4, new 2.18e-4.  The combination is between its parts on
    this scene (0.5 % of the pixels are trimmed, and the robust picture's remaining error is not noise a filter removes).  Where
    it does beat both is the few-sample glass scene: 4 passes raw 8.60e-3, robust 2.73e-3, guided 1.77e-3, new 9.68e-4.  Cornell
    box, guided / new: 1.99e-5 / 2.06e-5 at 4 passes, 2.47e-6 / 2.49e-6 at 64, 1.62e-6 / 1.63e-6 at 256 (nothing trimmed: the
    price of a guide from eight bucket means, 1 to 4 %).  The whole table is in DESIGN 6.8 and profiles/robust_denoise_quality_mi355x.json."""
    from clive2_amd.renderer import Renderer, make_seeds
    W, H = 256, 192
    scene = {"cornell": _cornell, "glass": _glass}[name](W, H)
    ref_r = Renderer(scene, seeds=make_seeds(W * H, seed=4321))
    ref_r.run_samples(1024)
    ref = ref_r.radiance
    ref_r.close()
    r = Renderer(scene)
    r.set_error_tracking(True)                                   # for the guided column only
    r.set_robust_buckets(8)
    r.render_features(4)
    e = {}
    for n in (4, 64, 256):
        r.run_samples(n - r.samples)
        e[n] = dict(raw=_rmse(r.radiance, ref), robust=_rmse(r.robust_radiance(), ref), guided=_rmse(r.guided_radiance(), ref),
                    new=_rmse(r.robust_guided_radiance(), ref))
        print(f"{name} {n} passes: rMSE " + " ".join(f"{k} {x:.4g}" for k, x in e[n].items()) +
              f" (new / guided {e[n]['new'] / e[n]['guided']:.3f})")
    r.close()
    for n in (4, 256):
        assert e[n]["new"] <= e[n]["raw"]
    if name == "cornell":
        for n in (64, 256):
            assert e[n]["new"] <= 1.25 * _measured("cornell", n)["new_over_guided"] * e[n]["guided"]


# ---------------------------------------------------------------- CLI
@pytest.mark.parametrize("extra", [[], ["--target-error", "0.5"]])
def test_cli_robust_denoise_writes_a_picture(extra, tmp_path):
    from clive2_amd import render
    out = tmp_path / "rd.png"
    assert render.main(["--scene", "empty", "--width", "64", "--height", "48", "--samples", "8", "--robust-denoise", "--out", str(out)]
                       + extra) == 0
    assert out.exists() or (tmp_path / "rd.png.npy").exists()
