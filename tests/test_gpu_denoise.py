"""The denoiser on the device (csrc/denoise.hpp): the feature pass against the render's own first hits, the filter against
its numpy statement (tests/denoise_reference.py) on renders and on injected features and colours (tests/feature_states.py), the
gain in picture quality, and that neither touches the render."""
import ctypes as C

import numpy as np
import pytest

import denoise_reference as dr
from denoise_scenes import cornell as _cornell, glass as _glass, open_scene as _open_scene      # (other test modules take them from here too)
import error_states as es
import feature_states as fs

pytestmark = pytest.mark.gpu


def _shading_normals(scene, tri, u, v, d):
    """sn of shade_and_bounce (csrc/kernels.hpp) in float32, turned to face the ray."""
    T = scene.triangles[tri]
    f = np.float32
    n0, n1, n2, tn = (np.asarray(T[k][:, :3], f) for k in ("n0", "n1", "n2", "normal"))
    u, v = u[:, None].astype(f), v[:, None].astype(f)
    s = (n0 * ((f(1) - u) - v) + n1 * u) + n2 * v
    length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    s = s * (f(1) / length)[:, None]
    facing = (d[:, 0] * tn[:, 0] + d[:, 1] * tn[:, 1]) + d[:, 2] * tn[:, 2]
    return np.where((facing > 0)[:, None], -s, s)


@pytest.mark.parametrize("name,mode", [("cornell", 0), ("glass", 0), ("open", 0), ("open", 5)])
def test_features_are_the_first_hits_of_the_camera_rays(name, mode):
    from clive2_amd.renderer import Renderer, make_seeds, CAMERA
    W, H = 72, 40
    scene = {"cornell": _cornell, "glass": _glass, "open": _open_scene}[name](W, H)
    S = make_seeds(W * H, seed=77)
    r = Renderer(scene, seeds=S)
    r.set_traversal_mode(mode)
    if mode == 5:
        assert r.organisation()["wide_nodes"] > 0
    r.make_camera_rays()
    rays = r.export_rays(CAMERA)
    bi, bt, u, v = r.probe_traverse(rays)
    r.render_features(1, seeds=S)
    f = r.features()
    assert all(np.isfinite(x).all() for x in f.values())
    hit = bi >= 0
    if name == "open":
        assert hit.any() and (~hit).any()
    else:
        assert hit.all()
    depth, cov = f["depth"].reshape(-1), f["coverage"].reshape(-1)
    normal, albedo = f["normal"].reshape(-1, 3), f["albedo"].reshape(-1, 3)
    assert np.array_equal(cov, hit.astype(np.float32))
    assert depth[hit].tobytes() == bt[hit].tobytes()
    mat_colour = np.asarray(scene.materials["color"][:, :3], np.float32)
    assert albedo[hit].tobytes() == mat_colour[scene.triangles["material"][bi[hit]]].tobytes()
    d = np.asarray(rays["direction"][:, :3], np.float32)
    want = _shading_normals(scene, bi[hit], u[hit], v[hit], d[hit])
    np.testing.assert_allclose(normal[hit], want, rtol=0, atol=1e-6)
    assert not normal[~hit].any() and not depth[~hit].any() and not albedo[~hit].any()
    # more samples: the coverage counts the hits, the normals stay unit length
    r.render_features(4, seeds=S)
    f4 = r.features()
    c4 = f4["coverage"]
    assert set(np.unique(c4)) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    n4 = f4["normal"][c4 > 0]
    np.testing.assert_allclose(np.linalg.norm(n4, axis=-1), 1.0, atol=1e-5)


SIGMAS = [dict(sigma_color=0.6, sigma_depth=0.1, sigma_albedo=0.1), dict(sigma_color=0.2, sigma_depth=0.02, sigma_albedo=0.3),
          dict(sigma_color=4.0, sigma_depth=1.0, sigma_albedo=0.05)]


@pytest.mark.parametrize("name,W,H", [pytest.param("cornell", 70, 45, id="cornell"), pytest.param("open", 70, 45, id="open"),
                                      pytest.param("open", 640, 360, id="open-640x360")])
def test_kernel_equals_the_specification(name, W, H):
    """70 x 45: partial 16 x 16 tiles on both edges.  640 x 360 on the open mesh scene: coverage fractions along every silhouette."""
    from clive2_amd.renderer import Renderer
    scene = {"cornell": _cornell, "open": _open_scene}[name](W, H)
    r = Renderer(scene)
    r.run_samples(3)
    r.render_features(2)
    f = r.features()
    c = r.radiance
    assert all(np.isfinite(x).all() for x in f.values())
    if name == "open":
        assert (f["coverage"] == 0).any()
    if W == 640:
        assert ((f["coverage"] > 0) & (f["coverage"] < 1)).sum() > 100
    for sig in SIGMAS:
        for it in (1, 5):
            got = r.denoised_radiance(iterations=it, **sig)
            want = dr.denoise(c, f["normal"], f["depth"], f["albedo"], f["coverage"], iterations=it, **sig)
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6, err_msg=f"{sig} iterations {it}")
    assert r.denoised_radiance(iterations=0).tobytes() == c.tobytes()


def _rmse(x, ref):
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2)))


@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_it_denoises(name):
    from clive2_amd.renderer import Renderer, make_seeds
    W, H = 256, 192
    scene = {"cornell": _cornell, "glass": _glass}[name](W, H)
    ref_r = Renderer(scene, seeds=make_seeds(W * H, seed=4321))
    ref_r.run_samples(1024)
    ref = ref_r.radiance
    ref_r.close()
    r = Renderer(scene)
    r.run_samples(4)
    r.render_features(4)
    raw, den = r.radiance, r.denoised_radiance()
    ratio = _rmse(den, ref) / _rmse(raw, ref)
    print(f"{name}: rMSE raw {_rmse(raw, ref):.4g} denoised {_rmse(den, ref):.4g} ratio {ratio:.3f}")
    assert ratio <= 0.5
    img = r.denoised_image
    assert img.dtype == np.uint8 and img.shape == (H, W, 3)


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
        if mode == 5:
            x.set_counting(2)
    a.run_samples(2)
    b.run_samples(1)
    b.render_features(4)
    b.denoised_radiance()
    _, n, z, al, cov = fs.features(W, H)
    b.load_features(n, z, al, cov)
    b.denoised_radiance(iterations=5)
    b.run_samples(1)
    assert a.packed_accumulators().tobytes() == b.packed_accumulators().tobytes()
    assert a.get_random_buffer().tobytes() == b.get_random_buffer().tobytes()
    assert a.counters() == b.counters()
    assert a.walk_tallies() == b.walk_tallies()


def test_denoise_needs_current_features():
    from clive2_amd.renderer import Renderer, RendererError
    from clive2_amd._native import ptr
    scene = _cornell(32, 24)
    r = Renderer(scene)
    r.run_samples(1)
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.denoised_radiance()
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.features()
    r.render_features(1)
    r.denoised_radiance()
    r.upload_scene(scene)
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.denoised_radiance()
    with pytest.raises(RendererError, match=r"\(-1\)"):
        r.render_features(0)
    with pytest.raises(RendererError, match=r"\(-1\)"):
        r._check(r._L.cl2_denoise(r._h, 1, -1.0, 0.1, 0.1, None, 0), "cl2_denoise")
    r.render_features(1)
    out = np.empty(3 * 32 * 24, np.float32)
    call = lambda it, sc, sd, sa: r._L.cl2_denoise(r._h, it, sc, sd, sa, ptr(out), C.c_size_t(out.size))
    for args in ((1, -1.0, 0.1, 0.1), (1, 2.0, 0.0, 0.1), (1, 2.0, 0.1, float("nan")), (1, float("inf"), 0.1, 0.1),
                 (-1, 2.0, 0.1, 0.1), (13, 2.0, 0.1, 0.1),
                 (1, 2.0, 0.1, 1e-23),              # sigma_albedo^2 underflows to 0
                 (0, 2.0, 0.1, 1e-23),              # ... whatever the number of passes
                 (1, 2.0, 0.1, 1e-19),              # ... or to a subnormal: 1e-38 < FLT_MIN = 1.1755e-38
                 (1, 1e-23, 0.1, 0.1),              # sigma_color^2 underflows
                 (1, 1e-19, 0.1, 0.1),
                 (12, 2e-16, 0.1, 0.1)):            # 4e-32 x 4^-11 = 9.5e-39: the last pass's denominator is subnormal
        assert call(*args) == -1, args
        with pytest.raises(RendererError, match=r"\(-1\)"):
            r._check(call(*args), "cl2_denoise")
    for args in ((1, 2.0, 0.1, 1.1e-19),            # 1.21e-38 >= FLT_MIN
                 (1, 1.1e-19, 0.1, 0.1),
                 (0, 1e-23, 0.1, 0.1),              # no pass divides by den_c
                 (11, 2e-16, 0.1, 0.1),             # 4e-32 x 4^-10 = 3.8e-38
                 (12, 2.5e-16, 0.1, 0.1),           # 6.25e-32 x 4^-11 = 1.49e-38
                 (12, 2.0, 1e-30, 0.1)):            # sigma_depth has no frame-wide denominator: its rule is per pixel
        assert call(*args) == 0, args
        assert np.isfinite(out).all()


# ---------------------------------------------------------------- the feature pass against its full restatement
def _feature_case(name, mode, K, W, H, samples):
    from clive2_amd.renderer import Renderer, make_seeds, stream_seeds
    scene = {"cornell": _cornell, "glass": _glass, "open": _open_scene}[name](W, H)
    S = make_seeds(W * H, seed=77)
    r = Renderer(scene, streams=K)
    if K > 1:
        r.set_seeds(stream_seeds(r.batch_size, K, seed=3))
    r.set_traversal_mode(mode)
    if mode == 5:
        assert r.organisation()["wide_nodes"] > 0
    r.render_features(samples, seeds=S)
    f = r.features()
    want = dr.feature_pass(scene, S, samples, r.probe_traverse)
    label = f"{name} mode {mode} K {K} {W} x {H} samples {samples}"
    assert all(np.isfinite(x).all() for x in f.values()), label
    for k in ("depth", "albedo", "coverage"):
        assert f[k].tobytes() == want[k].tobytes(), f"{label}: {k}"
    np.testing.assert_allclose(f["normal"], want["normal"], rtol=0, atol=1e-6, err_msg=label)
    cov = f["coverage"]
    if name == "open":
        assert (cov == 0).any() and (cov == 1).any()
        if samples > 1:
            assert ((cov > 0) & (cov < 1)).any()          # where dividing by the samples and by the hits differ
    else:
        assert (cov == 1).all()
    r.close()
    return f


WALKS = [("cornell", 0, 1), ("glass", 0, 1), ("open", 0, 1), ("open", 2, 1), ("open", 5, 1), ("open", 5, 4)]


@pytest.mark.parametrize("W,H", [(72, 40), (333, 251)])
@pytest.mark.parametrize("samples", [1, 3, 8])
def test_feature_pass_equals_the_restatement(W, H, samples):
    """Rays and seed states chained through oracle.np_kernels.generate_camera_rays, hits from probe_traverse on those rays, the
    float32 sums of k_feat_shade in sample order and the divisions of k_feat_finish in numpy: depth, albedo and coverage byte for
    byte, normals to 1e-6 (the reciprocal square roots of the two normalisations).  The walks and the stream count change no byte."""
    got = {w: _feature_case(*w, W, H, samples) for w in WALKS}
    for w in WALKS[3:]:
        for k in ("normal", "depth", "albedo", "coverage"):
            assert got[w][k].tobytes() == got[WALKS[2]][k].tobytes(), (w, k)


@pytest.mark.parametrize("samples", [1, 3, 8])
def test_feature_pass_equals_the_restatement_at_1080p(samples):
    """2,073,600 rays per launch: more than the device holds lanes (256 CUs x 2,048), so every walk's grid runs in several rounds.
    Every scene and walk of WALKS at every sample count, and the walks and the stream count change no byte, as at the small sizes
    (six handles per case: 5, 7 and 15 s on the MI355X, most of it the restatement's numpy)."""
    got = {w: _feature_case(*w, 1920, 1080, samples) for w in WALKS}
    for w in WALKS[3:]:
        for k in ("normal", "depth", "albedo", "coverage"):
            assert got[w][k].tobytes() == got[WALKS[2]][k].tobytes(), (w, k)


# ---------------------------------------------------------------- injected features x injected colours
@pytest.fixture(scope="module")
def pool():
    return es.pool()


def _injected(W, H, pool, wild=True, tracking=False, twin=False):
    """a handle whose features and accumulators are the states of feature_states; returns it, the feature arrays and the input"""
    from clive2_amd.renderer import Renderer
    r = Renderer(_cornell(W, H))
    cls, n, z, a, cov = fs.features(W, H)
    if twin:
        n, z, a, cov = fs.twin_outer_columns(n, z, a, cov)
    ccls, acc = fs.colours(cls, pool, wild=wild)
    if tracking:
        r.set_error_tracking(True)
    r.load_packed_accumulators(acc)
    if tracking:
        r.load_moments(es.state(pool, W * H, es.ALL)[2])
    r.load_features(n, z, a, cov)
    c = fs.radiance(acc, W, H)
    assert r.radiance.tobytes() == c.tobytes()
    return r, (cls, ccls), (n, z, a, cov), c


PASSES = (1, 2, 3, 5)


@pytest.mark.parametrize("W,H,sigmas", [(7, 5, (0, 1, 2)), (41, 25, (0, 1, 2)), (512, 513, (0, 1, 2)), (1920, 1080, (0,))],
                         ids=["7x5", "41x25", "512x513", "1920x1080"])
def test_injected_states_equal_the_restatement(W, H, sigmas, pool):
    """Every feature class and every colour class of feature_states at 1, 2, 3 and 5 passes.  Pixels that must pass through
    (coverage 0, a zero normal, depth 0) come back byte for byte; outside the reach of the wild colours rtol 1e-4, atol 1e-6, inside
    it the yardstick of feature_states.check().  (1920 x 1080: the first of the SIGMAS only, 20 s of numpy per chain.)"""
    r, (cls, ccls), g, c = _injected(W, H, pool)
    for k in fs.ALL:
        assert fs.has(cls, k).any(), fs.NAMES[k]
    for k in fs.COLOURS:
        assert (ccls == k).any(), fs.C_NAMES[k]
    f = r.features()
    for key, x in zip(("normal", "depth", "albedo", "coverage"), g):
        assert f[key].tobytes() == x.tobytes()
    keep = fs.pass_through(g[0], g[1], g[3])
    got0 = r.denoised_radiance(iterations=0)
    assert got0.tobytes() == c.tobytes()          # one IEEE division and the scrub: nothing to round differently
    acc = fs.colours(cls, pool)[1]                # the accumulators that _injected loaded (seeded)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        bad = ~np.isfinite(acc[:3] / acc[3]).T.reshape(H, W, 3)
    assert (got0[bad] == 0).all()                 # the scrub is per channel: a finite channel beside a NaN keeps its value
    assert bad[ccls == fs.C_WEIGHT0].all() and bad[ccls == fs.C_NONFINITE].any(axis=-1).all()
    for k in sigmas:
        res = fs.restatements(c, *g, SIGMAS[k], PASSES)
        for it in PASSES:
            got = r.denoised_radiance(iterations=it, **SIGMAS[k])
            assert got[keep].tobytes() == got0[keep].tobytes(), f"{W} x {H} sigmas {k} passes {it}: pass-through pixels"
            fs.check(got, *res[it], label=f"{W} x {H} sigmas {k} passes {it}")
    r.close()


@pytest.mark.parametrize("W,H", [(7, 5), (41, 25)])
def test_small_frames_with_calm_colours(W, H, pool):
    """On the two small frames the wild colours reach every pixel from 2 passes (7 x 5) and at 5 passes (41 x 25), so the test
    above holds none of their pixels to the plain tolerance there.  The same features under calm colours only: rtol 1e-4,
    atol 1e-6 over the whole frame at every pass count (the float32 restatement stays within an eighth of it of its float64
    companion, test_denoise_cpu.py)."""
    r, _, g, c = _injected(W, H, pool, wild=False)
    for k, sig in enumerate(SIGMAS):
        res = fs.restatements(c, *g, sig, PASSES, wild=False)
        for it in PASSES:
            assert not res[it][1].any()
            fs.check(r.denoised_radiance(iterations=it, **sig), *res[it], label=f"calm {W} x {H} sigmas {k} passes {it}")
    r.close()


WIDE = dict(sigma_color=1024.0, sigma_depth=1.0, sigma_albedo=0.3)      # den_c = 4^(10 - i): the colour edge-stop is still open at step 2048


@pytest.mark.parametrize("W,H", [(300, 200), (2049, 3)])
def test_twelve_passes(W, H, pool):
    """Passes 6 to 12, steps 32 to 2048: at 300 x 200 every tap but the centre leaves the frame from step 512 on (from 256 on in
    y), at 2049 x 3 a step-2048 tap connects the outermost columns only (their features are twins, so that they weigh each other).
    Calm colours: the float32 restatement stays within an eighth of the tolerance of its float64 companion (test_denoise_cpu.py),
    so rtol 1e-4, atol 1e-6 holds over the whole frame."""
    r, _, g, c = _injected(W, H, pool, wild=False, twin=W == 2049)
    for sig in SIGMAS + [WIDE]:
        res = fs.restatements(c, *g, sig, (6, 9, 11, 12), wild=False)
        for it in (6, 9, 11, 12):
            got = r.denoised_radiance(iterations=it, **sig)
            fs.check(got, *res[it], label=f"{W} x {H} {sig['sigma_color']} passes {it}")
    if W == 2049:
        b11, b12 = r.denoised_radiance(iterations=11, **WIDE), r.denoised_radiance(iterations=12, **WIDE)
        moved = np.abs(b12 - b11).max(axis=-1) / np.abs(b11).max(axis=-1).clip(1e-30)
        assert moved[:, 0].max() > 1e-3 and moved[:, -1].max() > 1e-3 and moved[:, 1:-1].max() < 1e-6
    r.close()


def test_no_state_leaks_from_call_to_call(pool):
    """iterations 0 .. 12 on one handle, then 12 .. 0, guided_radiance() calls in between (both filters share d_dn[0 / 1] and
    d_dn_out): every call returns the bytes a fresh handle returns for it."""
    W, H = 70, 45
    sig = SIGMAS[2]
    fresh = {}
    for it in range(13):
        r, _, _, _ = _injected(W, H, pool)
        fresh[it] = r.denoised_radiance(iterations=it, **sig)
        r.close()
    for a, b in ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5)):
        assert fresh[a].tobytes() != fresh[b].tobytes()                    # even and odd pass counts are different pictures
    r, _, _, _ = _injected(W, H, pool, tracking=True)
    guided = r.guided_radiance(iterations=3)
    for n, it in enumerate(list(range(13)) + list(range(12, -1, -1))):
        assert r.denoised_radiance(iterations=it, **sig).tobytes() == fresh[it].tobytes(), f"call {n}: iterations {it}"
        if n % 3 == 1:
            assert r.guided_radiance(iterations=2 + n % 2).shape == (H, W, 3)
    assert r.guided_radiance(iterations=3).tobytes() == guided.tobytes()
    r.close()


def test_degenerate_denominators_keep_the_input(pool):
    """Depth 0 on every covered pixel: den_z = 0, every weight sum is NaN and the picture comes back as it went in; so it does
    with a sigma_depth whose product with the depth underflows to 0 (1e-42 x 3 x 2^-149 is no float32), pixel by pixel."""
    W, H = 41, 25
    r, _, (n, z, a, cov), c = _injected(W, H, pool)
    got0 = r.denoised_radiance(iterations=0)
    r.load_features(n, np.zeros_like(z), a, cov)
    for it in (1, 4):
        assert r.denoised_radiance(iterations=it).tobytes() == got0.tobytes()
    r.load_features(n, np.where(cov > 0, np.float32(1e-4), 0).astype(np.float32), a, cov)
    got = r.denoised_radiance(iterations=1, sigma_depth=1e-42)
    assert got.tobytes() == got0.tobytes()
    assert got.tobytes() == dr.denoise(got0, n, np.where(cov > 0, np.float32(1e-4), 0), a, cov, iterations=1, sigma_depth=1e-42).tobytes()
    r.close()


# ---------------------------------------------------------------- cl2_write_features
def test_load_features_round_trip_and_refusals(pool):
    from clive2_amd.renderer import Renderer, RendererError
    from clive2_amd._native import ptr
    W, H = 41, 25
    scene = _cornell(W, H)
    r = Renderer(scene)
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.features()
    rs = np.random.RandomState(5)
    g0 = rs.randint(0, 2 ** 32, (H, W, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)      # any bytes, NaN patterns too
    g1 = rs.randint(0, 2 ** 32, (H, W, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)
    L, h = r._L, r._h
    for args in ((None, ptr(g1), W * H), (ptr(g0), None, W * H), (ptr(g0), ptr(g1), W * H - 1), (ptr(g0), ptr(g1), W * H + 1),
                 (ptr(g0), ptr(g1), 0), (ptr(g0), ptr(g1), 4 * W * H)):
        assert L.cl2_write_features(h, args[0], args[1], C.c_size_t(args[2])) == -1
    assert L.cl2_write_features(None, ptr(g0), ptr(g1), C.c_size_t(W * H)) == -1
    with pytest.raises(RendererError, match=r"\(-3\)"):                    # a refused write leaves no features behind
        r.features()
    assert L.cl2_write_features(h, ptr(g0), ptr(g1), C.c_size_t(W * H)) == 0   # allocates the feature set: none was rendered
    b0, b1 = np.empty_like(g0), np.empty_like(g1)
    assert L.cl2_read_features(h, ptr(b0), ptr(b1), C.c_size_t(W * H)) == 0
    assert b0.tobytes() == g0.tobytes() and b1.tobytes() == g1.tobytes()
    _, n, z, a, cov = fs.features(W, H)
    r.load_features(n, z, a, cov)
    f = r.features()
    assert all(f[k].tobytes() == x.tobytes() for k, x in zip(("normal", "depth", "albedo", "coverage"), (n, z, a, cov)))
    r.run_samples(1)
    r.denoised_radiance()
    r.upload_scene(scene)                                                   # written features go with the scene, as rendered ones do
    for call in (r.features, r.denoised_radiance):
        with pytest.raises(RendererError, match=r"\(-3\)"):
            call()
    r.load_features(n, z, a, cov)
    r.denoised_radiance()
    r.render_features(2)                                                    # rendering over written ones, and writing over rendered ones
    rendered = r.features()
    assert rendered["coverage"].min() == 1
    r.load_features(n, z, a, cov)
    assert r.features()["coverage"].tobytes() == cov.tobytes()
    r.load_features(**rendered)
    assert all(r.features()[k].tobytes() == rendered[k].tobytes() for k in rendered)
    r.close()
