"""The denoiser's specification (tests/denoise_reference.py, the numpy statement csrc/denoise.hpp is checked against on the
GPU): properties that follow from it, on synthetic guide buffers.  No GPU."""
import numpy as np

import denoise_reference as dr

F = np.float32


def _flat_features(H, W, depth=3.0):
    n = np.zeros((H, W, 3), F)
    n[..., 1] = 1
    return n, np.full((H, W), depth, F), np.full((H, W, 3), 0.5, F), np.ones((H, W), F)


def _noisy(H, W, seed=0):
    return np.random.RandomState(seed).gamma(1.0, 0.3, size=(H, W, 3)).astype(F)


def test_zero_iterations_is_identity():
    c = _noisy(20, 24)
    out = dr.denoise(c, *_flat_features(20, 24), iterations=0)
    assert out.dtype == F and out.tobytes() == c.tobytes()


def test_constant_image_is_a_fixed_point():
    H, W = 37, 45                                   # not a multiple of any step: taps fall off every edge
    c = np.empty((H, W, 3), F)
    c[...] = np.array([0.25, 0.5, 0.125], F)        # exact binary fractions: sum(w c) / sum(w) returns c to the last bit or so
    n, z, a, cov = _flat_features(H, W)
    z = z + np.linspace(0, 1, W, dtype=F)[None, :]  # guides that vary do not matter for a constant colour
    out = dr.denoise(c, n, z, a, cov, iterations=5)
    np.testing.assert_allclose(out, c, rtol=2e-6, atol=0)


def test_it_smooths():
    H, W = 32, 32
    c = _noisy(H, W)
    out = dr.denoise(c, *_flat_features(H, W), iterations=3, sigma_color=100.0)
    assert out.std() < 0.5 * c.std()
    assert abs(out.mean() - c.mean()) < 0.05 * c.mean()


def test_uncovered_pixels_pass_through_and_are_not_taps():
    H, W = 24, 24
    c = _noisy(H, W, 1)
    n, z, a, cov = _flat_features(H, W)
    cov[:, :8] = 0                                  # a band of background
    c[:, :8] = 1000.0                               # ... far brighter than the rest: would leak if it were tapped
    out = dr.denoise(c, n, z, a, cov, iterations=4, sigma_color=1e3)
    assert out[:, :8].tobytes() == c[:, :8].tobytes()
    assert out[:, 8:].max() < 10.0


def test_colour_does_not_cross_a_crease():
    """Two regions whose normals are perpendicular: w_n = 0 between them, so every output pixel is a weighted mean of its own
    region's colours only (here: a constant per region), whatever the other sigmas."""
    H, W = 30, 40
    n = np.zeros((H, W, 3), F)
    n[:, :17, 0] = 1                                # left wall faces +x
    n[:, 17:, 1] = 1                                # floor faces +y
    z = np.full((H, W), 2.0, F)
    a = np.full((H, W, 3), 0.7, F)
    cov = np.ones((H, W), F)
    c = np.zeros((H, W, 3), F)
    c[:, :17] = (1.0, 0.0, 0.0)
    c[:, 17:] = (0.0, 0.0, 4.0)
    out = dr.denoise(c, n, z, a, cov, iterations=5, sigma_color=1e6, sigma_depth=1e6, sigma_albedo=1e6)
    assert np.all(out[:, :17, 2] == 0) and np.all(out[:, :17, 1] == 0)
    assert np.all(out[:, 17:, 0] == 0) and np.all(out[:, 17:, 1] == 0)
    np.testing.assert_allclose(out[:, :17, 0], 1.0, rtol=1e-6)
    np.testing.assert_allclose(out[:, 17:, 2], 4.0, rtol=1e-6)


def test_weights_follow_the_formula_for_one_tap():
    """A 1 x 2 frame at step 1: each output is the two-tap mean with the weights of the specification, written out by hand."""
    c = np.array([[[1.0, 2.0, 3.0], [0.5, 0.25, 4.0]]], F)
    n = np.array([[[0.0, 1.0, 0.0], [0.0, 0.8, 0.6]]], F)
    z = np.array([[2.0, 2.5]], F)
    a = np.array([[[0.5, 0.5, 0.5], [0.4, 0.5, 0.6]]], F)
    cov = np.ones((1, 2), F)
    sc, sd, sa = 0.6, 0.1, 0.1
    out = dr.denoise(c, n, z, a, cov, iterations=1, sigma_color=sc, sigma_depth=sd, sigma_albedo=sa)

    def lum(v):
        return v[0] * 0.0722 + v[1] * 0.7152 + v[2] * 0.2126

    x = [c[0, k] / (1 + lum(c[0, k])) for k in range(2)]
    for p, q in ((0, 1), (1, 0)):
        wn = max(0.0, float(n[0, p] @ n[0, q])) ** 32
        wz = np.exp(-abs(z[0, p] - z[0, q]) / (sd * z[0, p]))
        wa = np.exp(-np.sum((a[0, p] - a[0, q]) ** 2) / sa ** 2)
        wc = np.exp(-np.sum((x[p] - x[q]) ** 2) / sc ** 2)
        wself = (3 / 8) ** 2
        wq = (3 / 8) * (1 / 4) * wn * wz * wa * wc
        want = (wself * c[0, p] + wq * c[0, q]) / (wself + wq)
        np.testing.assert_allclose(out[0, p], want, rtol=1e-5)


# ---- the keep rule: a weight sum that is not greater than 0 keeps the colour ----
def test_a_nan_weight_sum_keeps_the_colour():
    """sigma_albedo = 1e-23 is positive and finite, but its square underflows to 0 in float32: the centre tap's -0 / 0 makes every
    weight sum NaN.  (cl2_denoise refuses such a sigma; the restatement states what the kernel's `sw > 0` does with it.)"""
    c = _noisy(20, 24)
    f = _flat_features(20, 24)
    for kw in (dict(sigma_albedo=1e-23), dict(sigma_color=1e-23)):
        out, sw = dr.atrous_pass(c, *f, 0, **{**dict(sigma_color=2.0, sigma_depth=0.1, sigma_albedo=0.1), **kw}, return_sw=True)
        assert np.isnan(sw).all()
        assert out.tobytes() == c.tobytes()
        assert dr.denoise(c, *f, iterations=3, **kw).tobytes() == c.tobytes()


def test_zero_depth_and_zero_normal_keep_the_colour():
    H, W = 12, 14
    c = _noisy(H, W, 3)
    n, z, a, cov = _flat_features(H, W)
    z[3, 4] = 0                                     # den_z = 0: the centre tap is 0 / 0
    n[7, 9] = 0                                     # every w_n is 0: the weight sum is exactly 0
    out, sw = dr.atrous_pass(c, n, z, a, cov, 0, 2.0, 0.1, 0.1, return_sw=True)
    assert np.isnan(sw[3, 4]) and sw[7, 9] == 0
    keep = np.zeros((H, W), bool)
    keep[3, 4] = keep[7, 9] = True
    assert out[keep].tobytes() == c[keep].tobytes()
    assert np.isfinite(out).all() and (out[~keep] != c[~keep]).any(axis=-1).all()
    assert (sw[~keep] > 0.14).all()                 # everywhere else the centre tap alone weighs (3/8)^2


# ---- the state builders (tests/feature_states.py) ----
import feature_states as fs  # noqa: E402
import error_states as es    # noqa: E402
import pytest                # noqa: E402

SIGMAS = [dict(sigma_color=0.6, sigma_depth=0.1, sigma_albedo=0.1), dict(sigma_color=0.2, sigma_depth=0.02, sigma_albedo=0.3),
          dict(sigma_color=4.0, sigma_depth=1.0, sigma_albedo=0.05)]


@pytest.fixture(scope="module")
def pool():
    return es.pool()


@pytest.mark.parametrize("W,H", fs.FRAMES + [(300, 200), (2049, 3)])
def test_state_builders_have_every_class_and_only_finite_features(W, H, pool):
    cls, n, z, a, cov = fs.features(W, H)
    for k in fs.ALL:
        assert fs.has(cls, k).any(), fs.NAMES[k]
    for x in (n, z, a, cov):
        assert x.dtype == F and np.isfinite(x).all()
    # what the classes promise
    assert not n[fs.has(cls, fs.ZERO_NORMAL)].any() and (cov[fs.has(cls, fs.ZERO_NORMAL) & ~fs.has(cls, fs.COV0_CHECKER)
                                                             & ~fs.has(cls, fs.COV0_BLOCK) & ~fs.has(cls, fs.COV0_SINGLE)] > 0).all()
    for k in (fs.COV0_BLOCK, fs.COV0_SINGLE, fs.COV0_CHECKER):
        assert (cov[fs.has(cls, k)] == 0).all()
    covered = cov > 0
    assert (z[fs.has(cls, fs.DEPTH_ZERO)] == 0).all() and (z[fs.has(cls, fs.DEPTH_HUGE) & covered] >= 1e30).all()
    assert set(np.unique(cov)) >= {0.0, 1.0} and ((cov > 0) & (cov < 1)).any()
    length = np.linalg.norm(n.astype(np.float64), axis=-1)
    assert np.all((length == 0) | (np.abs(length - 1) < 1e-6))           # unit or zero, as k_feat_finish leaves them
    nothing = cov == 0
    assert not n[nothing].any() and not z[nothing].any() and not a[nothing].any()
    if W >= 48 and H >= 48:                                              # uncovered blocks larger than a 16 x 16 tile
        ys, xs = np.nonzero(fs.has(cls, fs.COV0_BLOCK) & ~fs.has(cls, fs.BORDER))
        assert ys.size and np.ptp(ys) >= 17 and np.ptp(xs) >= 17
        bx = fs.borders(W)
        assert {47, 97, 144} <= set(bx) or W < 146                       # seams on a tile multiple and one to either side
    assert {1, W - 1} <= set(fs.borders(W)) and {1, H - 1} <= set(fs.borders(H))
    ccls, acc = fs.colours(cls, pool)
    for k in fs.COLOURS:
        assert (ccls == k).any(), fs.C_NAMES[k]
    c = fs.radiance(acc, W, H)
    assert np.isfinite(c).all()
    w = acc[3].reshape(H, W)
    assert not c[(ccls == fs.C_WEIGHT0) | (ccls == fs.C_NONFINITE)].all(axis=-1).any()      # scrubbed to 0
    assert (w[ccls == fs.C_WEIGHT0] == 0).all() and not np.isfinite(acc[:3].T.reshape(H, W, 3)[ccls == fs.C_NONFINITE]).all(axis=-1).any()
    lum1 = 1 + c[ccls == fs.C_NEGATIVE].astype(np.float64) @ np.array([0.0722, 0.7152, 0.2126])
    assert (lum1 > 0).any() and (lum1 < 0).any() or (ccls == fs.C_NEGATIVE).sum() < 2
    r = c[ccls == fs.C_RANGE]
    assert r.min() > 0 and r.max() <= 1e30 and (r.max() > 1e10 or r.size < 30) and (r.min() < 1e-10 or r.size < 30)
    assert np.abs(c).max() <= 1e30                                       # 25 taps of weight <= 1 cannot overflow
    wild = np.isin(ccls, fs.WILD)
    assert not wild[:, :fs.wild_from(W)].any() and not (c[:, :fs.wild_from(W)] < 0).any()
    ccalm, acalm = fs.colours(cls, pool, wild=False)
    assert not np.isin(ccalm, fs.WILD).any() and not (fs.radiance(acalm, W, H) < 0).any()


@pytest.mark.parametrize("W,H", [(7, 5), (41, 25), (160, 113)])
def test_companion_yardstick_and_pass_through(W, H, pool):
    """The float64 companion against the float32 restatement: outside the wild colours' reach they agree to an eighth of the
    tolerance of the device comparison, so that tolerance (rtol 1e-4, atol 1e-6) holds there; pass-through pixels come back byte
    for byte from both; no weight sum of a covered pixel with a unit normal and a depth is small, so no pixel is ill-conditioned
    in the sense of DESIGN 6.3 and none is left out of a comparison."""
    cls, n, z, a, cov = fs.features(W, H)
    ccls, acc = fs.colours(cls, pool)
    c = fs.radiance(acc, W, H)
    keep = fs.pass_through(n, z, cov)
    assert keep.any() and not keep.all()
    for sig in SIGMAS:
        res = fs.restatements(c, n, z, a, cov, sig, (1, 2, 3, 5))
        c64 = c.astype(np.float64)
        for i in range(5):
            c64 = dr.atrous_pass(c64, n, z, a, cov, i, dtype=np.float64, **sig)
            if i + 1 not in res:
                continue
            want, reach, y, n_ref = res[i + 1]
            assert want.dtype == F and np.isfinite(want).all() and np.isfinite(c64).all()
            assert want[keep].tobytes() == c[keep].tobytes() and np.array_equal(c64[keep], c[keep].astype(np.float64))
            e = fs.nerr(want.astype(np.float64), c64)
            if (~reach).any():
                assert e[~reach].max() <= 1 / fs.K
            if reach.any():
                assert y == e[reach].max() and n_ref == (e[reach] > 1).sum()     # the cropped companion is the full one there
            # the restatement against itself passes the check; pushed beyond the yardstick it does not
            fs.check(want, want, reach, y, n_ref)
            bad = want.copy()
            yy, xx = np.nonzero(~keep)
            bad[yy[0], xx[0]] *= F(1 + 1e-3 * max(1.0, fs.K * y))
            bad[yy[0], xx[0]] += F(1e-3 * max(1.0, fs.K * y))
            with pytest.raises(AssertionError):
                fs.check(bad, want, reach, y, n_ref)
        _, sw = dr.denoise(c, n, z, a, cov, iterations=5, return_sw=True, **sig)
        assert (sw[~keep] > 0.14).all() and np.isinf(sw[keep]).all()


@pytest.mark.parametrize("W,H", [(7, 5), (41, 25)])
def test_calm_small_frames_stay_within_the_tolerance_of_the_companion(W, H, pool):
    """The calm-colour twins of the two small frames (test_gpu_denoise.py::test_small_frames_with_calm_colours): at 1 to 5 passes
    the float32 restatement is within an eighth of rtol 1e-4 / atol 1e-6 of its companion over the whole frame."""
    cls, n, z, a, cov = fs.features(W, H)
    _, acc = fs.colours(cls, pool, wild=False)
    c = fs.radiance(acc, W, H)
    for sig in SIGMAS:
        c32, c64 = c, c.astype(np.float64)
        for i in range(5):
            c32 = dr.atrous_pass(c32, n, z, a, cov, i, **sig)
            c64 = dr.atrous_pass(c64, n, z, a, cov, i, dtype=np.float64, **sig)
            assert fs.nerr(c32.astype(np.float64), c64).max() <= 1 / fs.K, (W, H, sig, i + 1)


def test_twelve_passes_stay_within_the_tolerance_of_the_companion(pool):
    """300 x 200 and 2049 x 3, calm colours, the three SIGMAS and the wide one of the device test: after twelve passes the float32
    restatement is within an eighth of rtol 1e-4 / atol 1e-6 of its companion, so the device comparison keeps that tolerance."""
    wide = dict(sigma_color=1024.0, sigma_depth=1.0, sigma_albedo=0.3)
    for W, H in ((300, 200), (2049, 3)):
        cls, n, z, a, cov = fs.features(W, H)
        _, acc = fs.colours(cls, pool, wild=False)
        c = fs.radiance(acc, W, H)
        for sig in SIGMAS + [wide]:
            a32 = dr.denoise(c, n, z, a, cov, iterations=12, **sig)
            a64 = dr.denoise(c, n, z, a, cov, iterations=12, dtype=np.float64, **sig)
            assert fs.nerr(a32.astype(np.float64), a64).max() <= 1 / fs.K, (W, H, sig)
        # the wide sigma keeps the colour edge-stop open at step 2048, and with the first column's features copied onto the last
        # the two outermost columns of the 2049-wide frame do see each other there -- and no other pair of pixels does
        if W == 2049:
            n, z, a, cov = fs.twin_outer_columns(n, z, a, cov)
            b11 = dr.denoise(c, n, z, a, cov, iterations=11, **wide)
            b12 = dr.atrous_pass(b11, n, z, a, cov, 11, **wide)
            moved = np.abs(b12 - b11).max(axis=-1) / np.abs(b11).max(axis=-1).clip(1e-30)
            assert moved[:, 0].max() > 1e-3 and moved[:, -1].max() > 1e-3 and moved[:, 1:-1].max() < 1e-6


# ---- the feature pass ----
def test_multi_sample_feature_restatement(oracle_mod):
    """dr.feature_pass on a tiny open scene with the oracle's walk: one sample is the first hits; three samples are the float64
    means of the three samples' hits, coverage their count / 3, and the numpy walk of np_kernels gives the same bytes."""
    from clive2_amd import struct_types as st
    from clive2_amd.renderer import make_seeds
    from oracle import np_kernels as npk
    from denoise_scenes import open_scene as _open_scene
    W, H = 24, 16
    scene = _open_scene(W, H)
    S = make_seeds(W * H, seed=77)
    trace = lambda rays: oracle_mod.traverse(rays, scene.boxes, scene.triangles)
    one = dr.feature_pass(scene, S, 1, trace)
    o, d, _, S1 = npk.generate_camera_rays(scene.camera, S)
    rays = np.zeros(W * H, st.Ray)
    rays["origin"][:, :3], rays["direction"][:, :3] = o, d
    bi, bt, u, v, _ = trace(rays)
    hit = bi >= 0
    assert hit.any() and (~hit).any()
    assert np.array_equal(one["coverage"].reshape(-1), hit.astype(F))
    assert one["depth"].reshape(-1)[hit].tobytes() == bt[hit].tobytes()
    mat = np.asarray(scene.materials["color"][:, :3], F)[scene.triangles["material"]]
    assert one["albedo"].reshape(-1, 3)[hit].tobytes() == mat[bi[hit]].tobytes()
    for k in ("normal", "depth", "albedo"):
        assert not one[k].reshape(W * H, -1)[~hit].any()
    three = dr.feature_pass(scene, S, 3, trace)
    ts, hs, state = [], [], S
    for _ in range(3):
        o, d, _, state = npk.generate_camera_rays(scene.camera, state)
        rays["origin"][:, :3], rays["direction"][:, :3] = o, d
        bi, bt, _, _, _ = trace(rays)
        ts.append(np.where(bi >= 0, bt, 0).astype(np.float64)); hs.append(bi >= 0)
    hits = np.sum(hs, axis=0)
    assert set(np.unique(hits)) == {0, 1, 2, 3}                          # fractional coverage is real on this scene
    assert np.array_equal(three["coverage"].reshape(-1), (hits.astype(F) / F(3)))
    some = hits > 0
    np.testing.assert_allclose(three["depth"].reshape(-1)[some], np.sum(ts, axis=0)[some] / hits[some], rtol=3e-7)
    length = np.linalg.norm(three["normal"].reshape(-1, 3)[some].astype(np.float64), axis=-1)
    np.testing.assert_allclose(length, 1.0, atol=1e-6)
    assert not (three["depth"].reshape(-1)[some] == one["depth"].reshape(-1)[some]).all()      # the seed state was carried on
    again = dr.feature_pass(scene, S, 3, lambda r: npk.traverse(r["origin"][:, :3], r["direction"][:, :3], scene.boxes, scene.triangles))
    for k in three:
        assert three[k].tobytes() == again[k].tobytes()
