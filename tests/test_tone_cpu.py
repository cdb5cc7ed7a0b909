"""The numpy statement of the device tone map (tests/tone_reference.py) against the host path it restates
(clive2_amd.camera.tone_map on the pictures the Renderer properties build) and against the reference's own fixtures, the derived
tolerance of the log sum against math.fsum, and the conditions on the injected states (tests/tone_states.py) that the device tests
(tests/test_gpu_tone.py) rely on.  CPU only."""
import os

import numpy as np
import pytest

import tone_reference as tr
import tone_states as ts
from clive2_amd.camera import tone_map

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = {"ordinary": ts.ORDINARY_ONLY, "finite": ts.FINITE, "all": ts.ALL}
SETTINGS = [(4.0, 1.0), (2.0, 1.5), (3.3, 1.0)]          # (exposure, white point); 3.3: a float32 product that rounds
LWS = [1.0, 1e-300, 0.0, np.inf, np.nan, 5e-324, 0.37]


@pytest.fixture(scope="module")
def pl():
    return ts.pool()


@pytest.fixture(scope="module")
def pool_terms(pl):
    return [tr.log_terms(pl[1], which) for which in range(3)]


def _host(pic, exposure, white_point):
    with np.errstate(all="ignore"):
        return tone_map(pic, exposure=exposure, white_point=white_point)


def _mismatch(got, want, cls):
    """the failure message: how many bytes, and the first few with their class and both values (a disagreement here may be the
    test host's float64 -> uint8 cast differing from tone_reference.to_byte: it is reported, not absorbed)"""
    got, want = got.reshape(-1, 3), want.reshape(-1, 3)
    bad = np.flatnonzero((got != want).any(1))
    return f"{bad.size} pixels differ: " + str([(int(p), ts.NAMES[cls[p]], got[p].tolist(), want[p].tolist()) for p in bad[:5]])


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("W,H", [(91, 60), (513, 512)])
def test_apply_given_the_hosts_log_average_is_the_host_tone_map(W, H, kind, pl):
    """apply() with the Lw camera.tone_map itself computes equals camera.tone_map byte for byte, for the three pictures built as
    the Renderer properties build them, at (exposure, white point) (4, 1), (2, 1.5) and (3.3, 1).  `all` holds POLE pixels, whose log term
    is NaN: Lw is NaN and every byte 0 on both sides."""
    cls, pick, acc = ts.state(pl, W * H, KINDS[kind], seed=W + H)
    if W * H >= 64:
        assert set(np.unique(cls[:64])) == set(KINDS[kind])
    for which in range(3):
        pic = tr.host_picture(acc, which, W, H)
        Lw = tr.host_log_average(pic)
        assert np.isfinite(Lw) == (kind != "all")
        for exposure, wp in SETTINGS:
            got = tr.apply(acc, which, exposure, wp, Lw).reshape(H, W, 3)
            want = _host(pic, exposure, wp)
            assert got.tobytes() == want.tobytes(), (tr.PICTURES[which], exposure, wp, _mismatch(got, want, cls))
        # the log terms are the host's, bit for bit (NaN for NaN)
        with np.errstate(all="ignore"):
            host_terms = np.log(0.1 + (pic * np.array([0.0722, 0.7152, 0.2126])).sum(axis=2)).reshape(-1)
        terms = tr.log_terms(acc, which)
        assert ((terms == host_terms) | (np.isnan(terms) & np.isnan(host_terms))).all()


@pytest.mark.parametrize("Lw", LWS)
def test_apply_given_any_log_average_is_numpys_chain(Lw, pl):
    """The last two lines of camera.tone_map with Lw handed in (so that the pole, Lw = 0, inf, NaN and the subnormal are reached):
    numpy's own promotion and its float64 -> uint8 cast against the explicit statement, every class, (4, 1), (2, 1.5), (3.3, 1), (4, 0.25)."""
    W, H = 91, 60
    cls, pick, acc = ts.state(pl, W * H, ts.ALL, seed=W + H)
    for which in range(3):
        pic = tr.host_picture(acc, which, W, H)
        for exposure, wp in SETTINGS + [(4.0, 0.25)]:
            with np.errstate(all="ignore"):
                scaled = pic * exposure / np.float64(Lw)
                want = (255 * scaled / (scaled + wp ** 2)).astype(np.uint8)
            got = tr.apply(acc, which, exposure, wp, Lw).reshape(H, W, 3)
            assert got.tobytes() == want.tobytes(), (tr.PICTURES[which], exposure, wp, _mismatch(got, want, cls))


def test_every_class_does_what_its_description_says(pl):
    """the states reach the cases they are there for (from the reference alone)"""
    pcls, pacc = pl
    for which in range(3):
        v = tr.value(pacc, which, 4.0, 1.0, 1.0)
        b = tr.to_byte(v)
        pre = tr.pixel(pacc, which, 4.0)[1]
        assert np.isneginf(v[pcls == ts.POLE]).all() and not b[pcls == ts.POLE].any()
        assert (v[pcls == ts.NEGATIVE] < 0).any(1).all()
        assert (v[pcls == ts.NEGATIVE] <= -1).any()                                              # bytes that wrap through int32
        assert (pre[pcls == ts.SATURATED] > 2.0 ** 53).all() and (b[pcls == ts.SATURATED] >= 254).all()
        if which < 2:
            assert np.isposinf(pre[pcls == ts.OVERFLOW]).all() and not b[pcls == ts.OVERFLOW].any()
            assert np.isposinf(tr.pixel(pacc, which, 2.0)[1][pcls == ts.OVERFLOW]).all()
        else:
            assert np.isfinite(pre[pcls == ts.OVERFLOW]).all() and (b[pcls == ts.OVERFLOW] >= 254).all()
        tiny = pre[(pcls == ts.TINY) & (pacc[3] == 1)]
        assert ((tiny > 0) & (tiny < 2.0 ** -126)).all()
        assert which == 1 or not pre[pcls == ts.UNCOVERED].any()                                 # (unweighted_image does not divide)
        terms = tr.log_terms(pacc, which)
        assert np.isnan(terms[pcls == ts.POLE]).all() and np.isfinite(terms[pcls != ts.POLE]).all()
    # out of int32's range on either side, at white point 0.25 and an Lw that puts a negative result next to -w^2
    far = tr.value(pacc, 1, 4.0, 0.25, 1.0)
    assert (far[pcls == ts.NEGATIVE] < -255).any()
    assert np.array_equal(tr.to_byte(np.array([-1.0, -1.9, -256.0, -257.5, 2.0 ** 31, -2.0 ** 31, -2.0 ** 31 + 1, 2.0 ** 31 - 0.5, 1e300,
                                               np.nan, np.inf, -np.inf, 255.99, 256.0])),
                          np.array([255, 255, 0, 255, 0, 0, 1, 255, 0, 0, 0, 0, 255, 0], np.uint8))


def test_apply_reproduces_the_tone_map_fixture():
    """tests/golden/tone_map.npz (the reference's tone_map of a seeded float32 picture, exposure 4): the picture as the colour sums
    of `unweighted_image`"""
    g = np.load(os.path.join(GOLD, "tone_map.npz"))
    img = g["image"]
    H, W = img.shape[:2]
    acc = np.zeros((8, W * H), np.float32)
    acc[:3] = img.reshape(-1, 3).T
    acc[3] = acc[7] = 1.0
    assert img.dtype == np.float32
    got = tr.apply(acc, 1, 4.0, 1.0, tr.host_log_average(img)).reshape(H, W, 3)
    assert got.tobytes() == g["out"].tobytes()


def test_apply_reproduces_the_three_pictures_of_the_glue_fixture():
    """tests/golden/renderer_glue.npz: the reference's three pictures of its own accumulators, given their Lw"""
    g = np.load(os.path.join(GOLD, "renderer_glue.npz"))
    W, H = int(g["width"]), int(g["height"])
    B = W * H
    acc = np.zeros((8, B), np.float32)
    acc[0:3] = g["summed_image"].reshape(B, 3).T
    acc[3] = g["summed_sample_weights"].reshape(B)
    acc[4:7] = g["unidirectional_image_buffer"].reshape(B, 3).T
    acc[7] = g["summed_sample_counts"].reshape(B)
    for which, name in enumerate(tr.PICTURES):
        Lw = tr.host_log_average(tr.host_picture(acc, which, W, H))
        got = tr.apply(acc, which, 4.0, 1.0, Lw).reshape(H, W, 3)
        assert got.tobytes() == g[name].tobytes(), (name, int((got != g[name]).sum()))


def test_sum_depth():
    assert [tr.sum_depth(W * H) for W, H in ts.SIZES] == [1 + 8 + 1 + 8, 18, 18, 18, 1 + 8 + 4 + 8, 2 + 8 + 4 + 8, 8 + 8 + 4 + 8]
    assert tr._grid(512 * 512) == tr._grid(513 * 512) == tr.TONE_BLOCKS and tr._grid(257) == 2


@pytest.mark.parametrize("W,H", ts.SIZES)
def test_sum_bound_holds_for_numpys_sum_and_for_the_device_order(W, H, pl, pool_terms):
    """|sum - math.fsum(terms)| <= sum_bound for numpy's pairwise sum and for the restated device order (per-thread strided sums,
    the shuffle tree, the four waves, the final kernel), on ordinary and on edge states without POLE (with it the sums are NaN, all
    three).  Neither involves another `log`, so both should sit well inside."""
    FB = W * H
    for kind in ("ordinary", "finite", "all"):
        cls, pick, acc = ts.state(pl, FB, KINDS[kind], seed=W + H)
        for which in range(3):
            terms = pool_terms[which][pick]
            exact, bound = tr.exact_sum(terms), tr.sum_bound(terms, FB)
            sums = float(terms.sum()), tr.device_sum(terms)
            if kind == "all" and FB >= 64:
                assert np.isnan(exact) and np.isnan(bound) and all(np.isnan(s) for s in sums)
                continue
            assert np.isfinite(exact) and bound > 0
            print(f"{W}x{H} {kind} {tr.PICTURES[which]}: |numpy - fsum| / bound {abs(sums[0] - exact) / bound:.3f}, "
                  f"|device order - fsum| / bound {abs(sums[1] - exact) / bound:.3f}")
            assert abs(sums[0] - exact) <= bound and abs(sums[1] - exact) <= bound


def test_device_order_counts_every_term_once():
    """the restated order itself: integers add exactly in any order"""
    for n in (1, 7, 257, 5460, 262144, 262145, 262144 + 513):
        assert tr.device_sum(np.arange(1.0, n + 1)) == n * (n + 1) / 2


@pytest.mark.parametrize("W,H", ts.SIZES)
def test_conditions_on_the_states(W, H, pl, pool_terms):
    """From the reference alone, per size and for the seed the device tests use:
    - ordinary states: at most 1e-5 of the bytes are fragile at the picture's own Lw, so the comparison with the host path is a
      comparison of (nearly) every byte;
    - edge states: the SATURATED pixels are fragile (254 / 255 by the last bit of the result), which is why that comparison runs
      on ordinary states only;
    - dropping or double counting the pixel at 0, 63, 64, 255, 256, 262143, 262144 or FB - 1 moves the sum by more than twice the
      tolerance, so the sum test sees it."""
    FB = W * H
    cls, pick, acc = ts.state(pl, FB, ts.ORDINARY_ONLY, seed=W + H)
    for which in range(3):
        terms = pool_terms[which][pick]
        bound = tr.sum_bound(terms, FB)
        Lw = tr.log_average(tr.exact_sum(terms), FB)
        frag = tr.fragile(acc, which, 4.0, 1.0, Lw, bound / FB)
        print(f"{W}x{H} {tr.PICTURES[which]}: {int(frag.sum())} fragile bytes of {frag.size}")
        assert frag.sum() <= 1e-5 * frag.size
        for p in ts.drop_positions(FB):
            assert abs(terms[p]) > 2 * bound, (p, terms[p], bound)
    if FB >= 64:
        cls, pick, acc = ts.state(pl, FB, ts.FINITE, seed=W + H)
        for which in range(3):
            terms = pool_terms[which][pick]
            bound = tr.sum_bound(terms, FB)
            frag = tr.fragile(acc, which, 4.0, 1.0, tr.log_average(tr.exact_sum(terms), FB), bound / FB)
            sat = (cls == ts.SATURATED) | ((cls == ts.OVERFLOW) & (which == 2))                  # (finite in float64, and > 2^53)
            print(f"{W}x{H} edge {tr.PICTURES[which]}: {int(frag.sum())} fragile bytes of {frag.size}, {int(frag[sat].sum())} saturated")
            assert frag[sat].all() and frag[~sat].sum() <= 1e-5 * frag.size
            for p in ts.drop_positions(FB):
                assert abs(terms[p]) > 2 * bound, (p, ts.NAMES[cls[p]], terms[p], bound)


def test_the_pools_picture_gathered_is_the_frames(pl):
    """what the device tests use: the picture is a function of the pixel, so apply() on the pool, gathered, is apply() on the frame"""
    cls, pick, acc = ts.state(pl, 91 * 60, ts.ALL, seed=5)
    for which in range(3):
        assert np.array_equal(tr.apply(pl[1], which, 4.0, 0.25, 1.0)[pick], tr.apply(acc, which, 4.0, 0.25, 1.0))
        a, b = tr.log_terms(pl[1], which)[pick], tr.log_terms(acc, which)
        assert ((a == b) | (np.isnan(a) & np.isnan(b))).all()


def test_poisoned_states(pl):
    for FB in (1, 7, 513 * 512):
        cls, pick, acc = ts.state(pl, FB, ts.ORDINARY_ONLY, seed=3)
        assert ts.poison_positions(FB) == ([0] if FB == 1 else [0, FB - 1] if FB <= 262144 else [0, 262144, FB - 1])
        for p in ts.poison_positions(FB):
            bad = ts.poisoned(acc, p)
            for which in range(3):
                terms = tr.log_terms(bad, which)
                assert np.isnan(terms[p]) and np.isnan(terms).sum() == 1
                assert not tr.apply(bad, which, 4.0, 1.0, np.nan).any()
