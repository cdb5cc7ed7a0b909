"""Adaptive sampling on the device (csrc/adaptive.hpp): a flat density through the mapped kernels gives the
default path's bytes; a non-uniform density's camera sample counts and one pass's accumulators equal their numpy restatement
(tests/adaptive_reference.py); an uneven density leaves the picture's expectation unchanged; render_until(adaptive=True)
against the uniform render; the refusals and the command line.

The density from the error estimate (k_dens_terms, k_dens_final, k_dens_from_terms and the quantisation) is compared with the
restatement as integers on injected states (tests/error_states.py) at frames up to 1920 x 1080, and mapped passes run at
320 x 240 and 1920 x 1080, where the prefix sum C of the quantised density no longer fits 32 bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_reference as ar
import error_reference as er
import error_states as es
from test_gpu_denoise import _cornell, _glass, _open_scene

pytestmark = pytest.mark.gpu

SCENES = {"cornell": lambda: _cornell(64, 48), "glass": lambda: _glass(64, 48), "open": lambda: _open_scene(72, 40)}


def _renderer(scene, K=1, seed=20240928, mode=None, pipelining=None, variant=None, tracking=True):
    from clive2_amd.renderer import Renderer, stream_seeds
    r = Renderer(scene, streams=K, variant=variant)
    r.set_seeds(stream_seeds(r.batch_size, K, seed=seed))
    r.set_reproducible(True)
    if mode is not None:
        r.set_traversal_mode(mode)
    if pipelining is not None:
        r.set_pipelining(pipelining)
    if tracking:
        r.set_error_tracking(True)
    return r


def _halves(W, H, left=1.75, right=0.25):
    d = np.full((H, W), right, np.float32)
    d[:, : W // 2] = left
    return d


def _luma(img):
    img = img.astype(np.float64)
    return (img[..., 0] * np.float64(np.float32(0.0722)) + img[..., 1] * np.float64(np.float32(0.7152))) \
        + img[..., 2] * np.float64(np.float32(0.2126))


@pytest.mark.parametrize("name,K", [("cornell", 1), ("cornell", 4), ("glass", 1), ("open", 2)])
@pytest.mark.parametrize("pipelining", [0, 2])
def test_flat_density_gives_the_default_bytes(name, K, pipelining):
    """An explicitly set flat density runs the mapped kernels (slot maps, mapped camera rays and resolve, the mapped finalize)
    and must give the default path's accumulators and moments byte for byte, serial and pipelined.  The open scene is a mesh
    scene on the 4-wide walk."""
    scene = SCENES[name]()
    mode = 5 if name == "open" else None
    a = _renderer(scene, K, mode=mode, pipelining=pipelining)
    a.run_samples(6)
    b = _renderer(scene, K, mode=mode, pipelining=pipelining)
    if name == "open":
        assert b.organisation()["wide_nodes"] > 0
    b.set_sample_density(np.ones((scene.pixel_height, scene.pixel_width), np.float32))
    assert (b.sample_density() == 1.0).all()
    b.run_samples(6)
    assert b.packed_accumulators().tobytes() == a.packed_accumulators().tobytes()
    assert b.moments().tobytes() == a.moments().tobytes()
    assert (b.camera_samples() == 6 * K).all() and (a.camera_samples() == 6 * K).all()


def _fixed_density(W, H):
    d = _halves(W, H)
    d[H // 3: H // 2, :] *= 3.0                    # a band of denser rows, pixels of up to five slots
    return d


def test_camera_samples_equal_the_numpy_expansion():
    scene = _cornell(64, 48)
    K = 2
    r = _renderer(scene, K, pipelining=2)
    r.set_sample_density(_fixed_density(64, 48))
    M = ar.from_density(r.sample_density())
    assert int(M.sum()) == 64 * 48 * ar.UNIT
    # the device's quantisation of the same weights, restated with the double sum in the device's order
    assert np.array_equal(M, ar.quantise(_fixed_density(64, 48)))
    r.run_samples(7)                               # pass numbers 0..6 of this handle, the level probe's pass included
    want = ar.camera_samples(ar.prefix(M), 0, 7, K)
    assert np.array_equal(r.camera_samples().reshape(-1), want.astype(np.float32))
    assert (r.packed_accumulators().reshape(8, -1)[7] == 7 * K).all()
    r.reset_accumulators()
    assert (r.camera_samples() == 0).all()


def test_one_pass_matches_the_float32_restatement():
    """Test variant with debug flag 4 (the t = 1 pairs skipped, so the light image stays empty): one mapped pass of a fixed
    non-uniform density, restated from the exported aggregators and unidirectional image with the device's M -- accumulators
    and moments bit for bit."""
    scene = _cornell(64, 48)
    W, H = 64, 48
    r = _renderer(scene, 1, variant="test")
    r.set_debug_flags(4)
    r.set_sample_density(_fixed_density(W, H))
    M = ar.from_density(r.sample_density())
    r.run_samples(1)
    agg_rec = r.export_aggregators().view(np.float32).reshape(W * H, 32)
    agg = np.zeros((13, W * H), np.float32)
    agg[:9] = agg_rec[:, :9].T
    agg[9:12] = agg_rec[:, 12:15].T
    agg[12] = agg_rec[:, 16]
    im = r.export_sample_images()
    uni = im["unidirectional"].reshape(-1, 4).astype(np.float32)
    light = np.zeros((W * H, 4), np.float32)
    acc = np.zeros((8, W * H), np.float32)
    mom = np.zeros((8, W * H), np.float32)
    n = ar.finalize_accumulate(agg, light, uni, acc, mom, ar.prefix(M), ar.inv_density(M), 0, W, H)
    got = r.packed_accumulators().reshape(8, -1)
    assert np.array_equal(r.camera_samples().reshape(-1), n.astype(np.float32))
    assert got.tobytes() == acc.tobytes(), np.argwhere(got != acc)[:5]
    assert r.moments().reshape(8, -1).tobytes() == mom.tobytes()


def test_reproducible_with_a_density():
    scene = _glass(64, 48)
    out = []
    for _ in range(2):
        r = _renderer(scene, 2, pipelining=2)
        r.set_sample_density(_fixed_density(64, 48))
        r.run_samples(5)
        out.append((r.packed_accumulators().tobytes(), r.moments().tobytes()))
        r.close()
    assert out[0] == out[1]


@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_uneven_density_is_unbiased(name):
    """N passes with 1.75 on the left half and 0.25 on the right against a uniform render with other seeds: per-pixel luma z
    scores from both standard errors.  Bounds set from the recorded runs, with margin.  The glass scene's
    caustics are carried by light-traced paths: the case that catches a wrong weighting of the light image."""
    scene = SCENES[name]()
    W, H = scene.pixel_width, scene.pixel_height
    N = 256
    a = _renderer(scene, 1, seed=11, pipelining=2)
    a.set_sample_density(_halves(W, H))
    a.run_samples(N)
    u = _renderer(scene, 1, seed=23, pipelining=2)
    u.run_samples(N)
    La, Lu = _luma(a.radiance), _luma(u.radiance)
    sa, su = a.standard_error()[..., 3].astype(np.float64), u.standard_error()[..., 3].astype(np.float64)
    ok = np.isfinite(sa) & np.isfinite(su) & ((sa > 0) | (su > 0))
    z = (La[ok] - Lu[ok]) / np.sqrt(sa[ok] ** 2 + su[ok] ** 2)
    rel = (La[ok].mean() - Lu[ok].mean()) / Lu[ok].mean()
    cnt = a.camera_samples()
    frac4 = np.mean(np.abs(z) > 4)
    print(f"unbiased {name}: {ok.sum()} pixels, frame-mean rel diff {rel:+.4f}, mean z {z.mean():+.4f}, sd z {z.std():.3f}, "
          f"|z|>4 {frac4:.4f}; camera samples left {cnt[:, : W // 2].mean():.1f} right {cnt[:, W // 2:].mean():.1f}")
    assert abs(cnt[:, : W // 2].mean() / N - 1.75) < 0.05 and abs(cnt[:, W // 2:].mean() / N - 0.25) < 0.05
    assert ok.sum() > 0.9 * W * H
    assert abs(rel) < 0.02
    assert abs(z.mean()) < 0.15
    assert frac4 < 0.01


@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_render_until_adaptive_against_uniform(name):
    """128 x 96: passes to reach the target, and the true relative MSE of the luma against a long uniform reference at equal
    passes.  What DESIGN 6.5 records; the assertions are only what the recorded runs support."""
    import clive2_amd as c2
    W, H = 128, 96
    scene = _cornell(W, H) if name == "cornell" else _glass(W, H)
    target = 0.05 if name == "cornell" else 0.1
    ref = _renderer(scene, 1, seed=99, pipelining=2, tracking=False)
    ref.run_samples(2048)
    Lref = _luma(ref.radiance)
    res = {}
    for adaptive in (False, True):
        r = _renderer(scene, 1, seed=5, pipelining=2)
        passes, e = r.render_until(target, 4096, min_samples=8, check_every=8, adaptive=adaptive)
        L = _luma(r.radiance)
        covered = Lref > 0
        mse = np.mean(((L[covered] - Lref[covered]) / (Lref[covered] + 0.01)) ** 2)
        res[adaptive] = (passes, e, mse)
        if adaptive:
            assert r.sample_density().std() > 0
    # the same number of passes with the density of the adaptive run's end, against uniform
    print(f"gain {name}: uniform {res[False][0]} passes (e {res[False][1]:.4f}, rel MSE {res[False][2]:.3e}); adaptive "
          f"{res[True][0]} passes (e {res[True][1]:.4f}, rel MSE {res[True][2]:.3e})")
    assert res[True][1] <= target
    assert res[True][0] <= 1.5 * res[False][0]


def test_refusals():
    from clive2_amd.renderer import RendererError
    scene = _cornell(32, 24)
    r = _renderer(scene, 1, tracking=False)
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.update_sample_density()                       # no moments
    for bad in (np.ones(5, np.float32),):
        with pytest.raises(ValueError):
            r.set_sample_density(bad)
    # the C entry points' own checks
    L, h = r._L, r._h
    from clive2_amd._native import ptr
    import ctypes as C
    for bad in (np.full(32 * 24, np.nan, np.float32), np.zeros(32 * 24, np.float32), np.full(32 * 24, np.inf, np.float32),
                -np.ones(32 * 24, np.float32)):
        assert L.cl2_set_sample_density(h, ptr(bad), C.c_size_t(bad.size)) == -1
    ones = np.ones(32 * 24, np.float32)
    assert L.cl2_set_sample_density(h, ptr(ones), C.c_size_t(ones.size - 1)) == -1
    r.set_sample_density(ones.reshape(24, 32))
    for stage in (r.make_light_rays, r.make_camera_rays, r.trace_light_rays, r.trace_camera_rays, r.join_paths,
                  r.finalize_samples, r.gather_light_image, r.process_images):
        with pytest.raises(RendererError, match=r"\(-3\)"):
            stage()
    r.set_sample_density(None)
    r.make_light_rays()                                  # uniform again: the stage calls work
    # adaptive render_until needs two addends before its first update
    r.set_error_tracking(True)
    r.reset_accumulators()
    assert L.cl2_set_adaptive_sampling(h, 1, C.c_double(0.25)) == 0
    assert L.cl2_get_adaptive_sampling(h) == 1
    done, e = C.c_int(0), C.c_double(0)
    assert L.cl2_run_until(h, 0.05, 0.001, 1, 4, 1, C.byref(done), C.byref(e)) == -1
    assert L.cl2_set_adaptive_sampling(h, 1, C.c_double(0.0)) == -1
    assert L.cl2_set_adaptive_sampling(h, 0, C.c_double(0.0)) == 0
    # the cross-check resolve of the test variant
    t = _renderer(scene, 1, variant="test", tracking=False)
    t.set_reproducible(False)                            # (the cross-check kernel has no reproducible form either)
    t.set_debug_flags(0x70)
    t.set_sample_density(ones)
    with pytest.raises(RendererError, match=r"\(-3\)"):
        t.run_samples(1)


def test_density_calls_refused_with_a_communicator(tmp_path):
    child = os.path.join(os.path.dirname(__file__), "adaptive_comm_child.py")
    env = dict(os.environ, CLIVE2_RENDEZVOUS_FILE=str(tmp_path / "rccl_id"), HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300, env=env)
    steps = [l.split()[1] for l in p.stdout.splitlines() if l.startswith("STEP ")]
    assert p.returncode == 0, (steps, p.stdout[-2000:], p.stderr[-3000:])
    assert steps == ["comm-up", "refused", "closed"], steps


def test_cli_adaptive_writes_a_png(tmp_path):
    from clive2_amd import render
    out = tmp_path / "a.png"
    render.main(["--scene", "empty", "--width", "48", "--height", "32", "--samples", "256", "--adaptive", "--target-error", "0.05",
                 "--out", str(out)])
    assert out.exists() and out.stat().st_size > 0


# ---------------------------------------------------------------- the density from injected error states
SHARES = (0.1, 0.25, 1.0)


@pytest.fixture(scope="module")
def pool():
    return es.pool()


@pytest.fixture(scope="module")
def handles():
    """one handle per frame for the whole module (the 1920 x 1080 one is made once)"""
    made = {}

    def get(W, H, K=1, pipelining=None):
        key = (W, H, K, pipelining)
        if key not in made:
            made[key] = _renderer(_cornell(W, H), K, pipelining=pipelining)
        return made[key]
    yield get
    for r in made.values():
        r.close()


def _load(r, acc, mom):
    r.load_packed_accumulators(acc)
    r.load_moments(mom)


def _device_M(r, FB):
    """M of the density in force, with the two invariants asserted on the device's own values"""
    M = ar.from_density(r.sample_density())
    assert int(M.sum(dtype=np.uint64)) == FB * ar.UNIT and int(M.min()) >= 1
    return M


def _assert_update(r, acc, mom, floor, share, terms=None):
    FB = acc.shape[1]
    t = ar.terms(acc, mom, floor) if terms is None else terms
    m = ar.density_from_terms(t, share)
    r.update_sample_density(floor, share)
    M = _device_M(r, FB)
    want = ar.quantise(m)
    bad = np.flatnonzero(M != want)
    assert bad.size == 0, (floor, share, len(bad), bad[:5], M[bad[:5]], want[bad[:5]])
    return t, m, M


@pytest.mark.parametrize("W,H", es.FRAMES)
def test_density_from_injected_states_equals_the_restatement(W, H, pool, handles):
    """update_sample_density() on the injected states that have a finite term -- the well-scaled classes; with the subnormal,
    L = 0 and float32-overflowing ones; with the overflowed moments and n < 2 pixels as well -- for uniform_share 0.1, 0.25, 1 and
    floor 0, 0.001: M equals quantise(density_from_terms(terms(acc, mom, floor), share)) as integers."""
    r = handles(W, H)
    FB = W * H
    for allowed in (es.BASE, es.NO_FEW, es.ALL):
        cls, acc, mom = es.state(pool, FB, allowed)
        _load(r, acc, mom)
        for floor in (0.0, 0.001):
            t = ar.terms(acc, mom, floor)
            if allowed is not es.BASE and FB >= 576:
                assert np.isinf(t).any() and np.isfinite(t).any()      # terms to be clipped beside finite ones
            for share in SHARES:
                _, m, M = _assert_update(r, acc, mom, floor, share, terms=t)
                if share == 1.0:
                    assert (M == ar.UNIT).all()
                elif allowed is es.BASE:
                    assert M.min() < ar.UNIT < M.max()
    r.set_sample_density(None)


@pytest.mark.parametrize("W,H", es.FRAMES)
def test_density_clip_flat_and_no_finite_term(W, H, pool, handles):
    """A pixel whose finite term lies above 16 x the mean is clipped to it; every finite term 0 gives the flat density; no finite
    term is refused with CL2_E_STATE and leaves the density that was in force."""
    from clive2_amd.renderer import RendererError
    r = handles(W, H)
    FB = W * H
    cls, acc, mom = es.state(pool, FB, es.BASE)
    k = int(np.flatnonzero(cls == es.ORDINARY)[len(np.flatnonzero(cls == es.ORDINARY)) // 2])
    mom = mom.copy()
    mom[:, k] = pool[2][:, 0] * np.float32(1e6)                          # the pool's first state (n = 2) with a million-fold spread
    acc = acc.copy()
    acc[:, k] = pool[1][:, 0]
    _load(r, acc, mom)
    t, m, M = _assert_update(r, acc, mom, 0.001, 0.25)
    mean = er.grid_sum(np.where(np.isfinite(t), t, 0)) / np.isfinite(t).sum()
    assert np.isfinite(t[k]) and t[k] > ar.KAPPA * mean
    assert m[k] == np.float32(0.25 + 0.75 * ar.KAPPA) and M[k] == M.max()
    clipped = M.copy()
    # every finite term 0: moments all zero (S = 0), uncovered pixels beside them
    zero = np.zeros_like(mom)
    _load(r, acc, zero)
    t, m, M = _assert_update(r, acc, zero, 0.001, 0.25)
    assert not t.any() and (M == ar.UNIT).all()
    # no finite term: every pixel covered with n = 1
    m_fixed = (1.0 + 0.5 * np.cos(np.arange(FB))).astype(np.float32)
    r.set_sample_density(m_fixed)
    before = r.sample_density().copy()
    assert np.array_equal(ar.from_density(before), ar.quantise(m_fixed))
    fa, fm = es.few_pixel(pool)
    a1, m1 = np.repeat(fa[:, None], FB, 1), np.repeat(fm[:, None], FB, 1)
    _load(r, a1, m1)
    assert np.isinf(ar.terms(a1, m1, 0.001)).all() and ar.density_from_terms(ar.terms(a1, m1, 0.001), 0.25) is None
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.update_sample_density(0.001, 0.25)
    assert r.sample_density().tobytes() == before.tobytes()
    # and the clipped state again, after the refusal: the same integers
    _load(r, acc, mom)
    r.update_sample_density(0.001, 0.25)
    assert np.array_equal(_device_M(r, FB), clipped)
    r.set_sample_density(None)


# ---------------------------------------------------------------- mapped passes where C leaves 32 bits
def _far_density(W, H):
    """_fixed_density scaled to the frame, plus a block of weight-8 pixels in the last rows: the slots of the last pixels lie far
    from their own index"""
    d = _fixed_density(W, H)
    d[H - H // 8:, W // 4: W // 2] = 8.0
    return d


@pytest.mark.parametrize("W,H", [(320, 240), (1920, 1080)])
def test_camera_samples_where_the_prefix_sum_passes_32_bits(W, H, handles):
    """K = 2, pipelined, three passes of a fixed non-uniform density at 76,800 and 2,073,600 pixels (C ends at 5.03e9 and
    1.36e11): every pixel's camera samples equal the numpy expansion, and acc row 7 is 3 K everywhere."""
    K = 2
    FB = W * H
    r = handles(W, H, K, 2)
    r.reset_accumulators()
    r.set_sample_density(_far_density(W, H))
    M = _device_M(r, FB)
    assert np.array_equal(M, ar.quantise(_far_density(W, H)))
    C = ar.prefix(M)
    assert int(C[-1]) == FB * ar.UNIT > 1 << 32
    lo, hi = ar.ranges(C, 0)
    assert np.abs(lo - np.arange(FB)).max() > FB // 64                    # slots far from their pixels
    r.run_samples(3)                               # the handle's first passes with a density: numbers 0, 1, 2
    want = ar.camera_samples(C, 0, 3, K)
    got = r.camera_samples().reshape(-1)
    bad = np.flatnonzero(got != want.astype(np.float32))
    assert bad.size == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    assert (r.packed_accumulators().reshape(8, -1)[7] == 3 * K).all()
    r.set_sample_density(None)
    r.reset_accumulators()


def test_one_pass_at_320x240_matches_the_float32_restatement():
    """test_one_pass_matches_the_float32_restatement at 320 x 240, where slot indices pass 65,536 and C passes 2^32: one mapped pass
    (test variant, debug flag 4) against adaptive_reference.finalize_accumulate, accumulators and moments bit for bit at the
    pixels restated -- the first and last rows and columns, the border of the weight-8 block (inside and outside), and a seeded
    draw of 1,500 of the pixels whose slots lie above 65,536; at least 2,000 pixels, at least 500 of them with slots above
    65,536.  The camera sample counts are compared at every pixel."""
    W, H = 320, 240
    FB = W * H
    r = _renderer(_cornell(W, H), 1, variant="test")
    r.set_debug_flags(4)
    r.set_sample_density(_far_density(W, H))
    M = ar.from_density(r.sample_density())
    C = ar.prefix(M)
    r.run_samples(1)
    agg_rec = r.export_aggregators().view(np.float32).reshape(FB, 32)
    agg = np.zeros((13, FB), np.float32)
    agg[:9] = agg_rec[:, :9].T
    agg[9:12] = agg_rec[:, 12:15].T
    agg[12] = agg_rec[:, 16]
    uni = r.export_sample_images()["unidirectional"].reshape(-1, 4).astype(np.float32)
    lo, hi = ar.ranges(C, ar.offset(0, 0))
    y, x = np.divmod(np.arange(FB), W)
    edge = (y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)
    y0, x0, x1 = H - H // 8, W // 4, W // 2
    near_block = (y >= y0 - 2) & (x >= x0 - 2) & (x < x1 + 2)
    deep = (y >= y0 + 1) & (x >= x0 + 1) & (x < x1 - 1)
    border = near_block & ~deep
    high = np.flatnonzero((lo >= 65536) & (hi > lo))
    draw = np.random.RandomState(4).choice(high, 1500, replace=False)
    pixels = np.unique(np.concatenate([np.flatnonzero(edge | border), draw]))
    assert len(pixels) >= 2000 and np.isin(pixels, high).sum() >= 500
    acc = np.zeros((8, FB), np.float32)
    mom = np.zeros((8, FB), np.float32)
    n = ar.finalize_accumulate(agg, np.zeros((FB, 4), np.float32), uni, acc, mom, C, ar.inv_density(M), 0, W, H, pixels=pixels)
    assert np.array_equal(r.camera_samples().reshape(-1), n.astype(np.float32))
    got, gmom = r.packed_accumulators().reshape(8, -1), r.moments().reshape(8, -1)
    assert got[:, pixels].tobytes() == acc[:, pixels].tobytes(), pixels[np.argwhere(got[:, pixels] != acc[:, pixels])[:5, 1]]
    assert gmom[:, pixels].tobytes() == mom[:, pixels].tobytes()
    assert (got[3, pixels] > 0).sum() > 1000
    r.close()
