"""The device tone map (csrc/tonemap.hpp: k_tone_logsum, k_tone_logsum_final, k_tone_apply) against its numpy statement
(tests/tone_reference.py) on injected states (tests/tone_states.py), 1 x 1 to 1920 x 1080:

    the log sum       within the derived sum_bound of math.fsum of the reference's terms; NaN where a term is
    the picture       given Lw, byte for byte -- no tolerance -- on every class, at eight Lw that reach the pole, 0, inf, NaN
    tone_mapped()     the restatement at the device's own Lw byte for byte; the host property outside the fragile bytes
    hygiene           same bytes twice, the shared partial-sum buffer across interleaved calls, the accumulators untouched
    a real render     the drain before the kernels

512 x 512 is exactly TONE_BLOCKS * 256 pixels (the last frame on which every thread adds one term), 513 x 512 the first with a
second grid-stride iteration, 1920 x 1080 has 8 of them and 1024 partials in the final kernel; 1 x 1, 7 x 1, 257 x 1 and 91 x 60
are below a wave, below a workgroup, one workgroup + 1 and a ragged last workgroup.  Nothing larger takes another path.

The picture is a function of the pixel alone once Lw is given, and a state's pixels are draws from a pool of 2^18 pixel states,
so a frame's reference is the pool's, gathered (tests/test_tone_cpu.py checks that this is the frame's)."""
import numpy as np
import pytest

import tone_reference as tr
import tone_states as ts
from denoise_scenes import cornell as _cornell

pytestmark = pytest.mark.gpu

KINDS = {"ordinary": ts.ORDINARY_ONLY, "finite": ts.FINITE, "all": ts.ALL}
# (exposure, white point).  An exposure of 2 or 4 scales a float32 exactly, so whether `f * exposure` is a float32 or a float64 product
# shows at these only where it overflows; 3.3 is there so that it shows in every ordinary pixel's last bits.
SETTINGS = [(4.0, 1.0), (2.0, 1.5), (4.0, 0.25), (3.3, 1.0)]
WORST = {}                                            # (W, H) -> the largest |device sum - fsum| / sum_bound seen (reported only)


@pytest.fixture(scope="module")
def pl():
    return ts.pool()


@pytest.fixture(scope="module")
def pool_terms(pl):
    return [tr.log_terms(pl[1], which) for which in range(3)]


@pytest.fixture(scope="module")
def handles():
    """one renderer per size, the scene preset "empty" """
    import clive2_amd as c2
    from clive2_amd.renderer import Renderer
    made = {}

    def get(W, H):
        if (W, H) not in made:
            made[W, H] = Renderer(c2.create_scene_from_preset("empty", W, H))
            assert made[W, H].batch_size == W * H
        return made[W, H]
    yield get
    for r in made.values():
        r.close()


@pytest.fixture(scope="module")
def frames(pl, pool_terms):
    """per (W, H, kind): the state and, per picture, (terms, math.fsum of them, sum_bound): computed once, never written to"""
    made = {}

    def get(W, H, kind):
        if (W, H, kind) not in made:
            FB = W * H
            cls, pick, acc = ts.state(pl, FB, KINDS[kind], seed=W + H)
            if FB >= 64:
                assert set(np.unique(cls[:64])) == set(KINDS[kind])
            sums = []
            for which in range(3):
                terms = pool_terms[which][pick]
                sums.append((terms, tr.exact_sum(terms), tr.sum_bound(terms, FB)))
            acc.setflags(write=False)
            made[W, H, kind] = (cls, pick, acc, sums)
        return made[W, H, kind]
    return get


_APPLIED = {}


def _pool_picture(pl, which, exposure, wp, Lw):
    """apply() on the pool, kept: the sizes share most of their (exposure, white point, Lw)"""
    key = (which, exposure, wp, np.float64(Lw).tobytes())
    if key not in _APPLIED:
        _APPLIED[key] = tr.apply(pl[1], which, exposure, wp, Lw)
    return _APPLIED[key]


def _differing(got, want, cls):
    got, want = got.reshape(-1, 3), want.reshape(-1, 3)
    bad = np.flatnonzero((got != want).any(1))
    return f"{bad.size} pixels differ: " + str([(int(p), ts.NAMES[cls[p]], got[p].tolist(), want[p].tolist()) for p in bad[:5]])


def _host(r, name):
    with np.errstate(all="ignore"):
        return getattr(r, name)


@pytest.mark.parametrize("W,H", ts.SIZES)
def test_log_sum_is_within_the_derived_bound(W, H, handles, frames):
    """tone_log_sum against math.fsum of the reference's terms, tolerance sum_bound (derived in tests/tone_reference.py, not
    measured), on ordinary states, on edge states without POLE -- every other class, the sum finite so that every term counts --
    and on the full edge states, whose POLE pixels have a NaN term: the sum must be NaN."""
    r = handles(W, H)
    for kind in KINDS:
        cls, pick, acc, sums = frames(W, H, kind)
        r.load_packed_accumulators(acc)
        for which, name in enumerate(tr.PICTURES):
            terms, exact, bound = sums[which]
            got = r.tone_log_sum(name)
            if np.isnan(exact):
                assert kind == "all" and np.isnan(got), (kind, name, got)
                continue
            ratio = abs(got - exact) / bound
            WORST[W, H] = max(WORST.get((W, H), 0.0), ratio)
            print(f"{W}x{H} {kind} {name}: device sum {got!r}, fsum {exact!r}, |difference| / sum_bound = {ratio:.4f}")
            assert abs(got - exact) <= bound, (kind, name, got, exact, bound)
    print(f"{W}x{H}: largest |device sum - fsum| / sum_bound = {WORST.get((W, H), 0.0):.4f}")


@pytest.mark.parametrize("W,H", ts.SIZES)
def test_one_poisoned_pixel_makes_the_sum_nan(W, H, handles, frames):
    """Ordinary states with one pixel of luma -1 (first pixel, last pixel, the first pixel of the second grid-stride iteration):
    a sum that skips it is finite.  The picture is then all zero bytes, as the host's."""
    r = handles(W, H)
    cls, pick, acc, sums = frames(W, H, "ordinary")
    for p in ts.poison_positions(W * H):
        r.load_packed_accumulators(ts.poisoned(acc, p))
        for name in tr.PICTURES:
            assert np.isnan(r.tone_log_sum(name)), (p, name)
            got = r.tone_mapped(name)
            assert got.shape == (H, W, 3) and got.dtype == np.uint8 and not got.any(), (p, name)
            assert got.tobytes() == _host(r, name).tobytes(), (p, name)


@pytest.mark.parametrize("W,H", ts.SIZES)
def test_picture_given_the_log_average_is_bitwise(W, H, handles, frames, pl):
    """tone_mapped(..., log_average=Lw) against apply(), no tolerance, every class, (exposure, white point) (4, 1), (2, 1.5),
    (4, 0.25), (3.3, 1), at Lw = the host's own (NaN when the state holds a POLE pixel, so also: the host's Lw of the same frame's state
    without POLE, a finite one of the size these states have), 1.0 (the pole: result + w^2 == 0), 1e-300, 0.0, +inf, NaN and
    5e-324."""
    r = handles(W, H)
    cls, pick, acc, sums = frames(W, H, "all")
    finite = frames(W, H, "finite")[2]
    r.load_packed_accumulators(acc)
    for which, name in enumerate(tr.PICTURES):
        own = tr.host_log_average(tr.host_picture(acc, which, W, H))
        twin = tr.host_log_average(tr.host_picture(finite, which, W, H))
        assert np.isfinite(twin) and (np.isnan(own) or W * H < 64)
        for Lw in (own, twin, 1.0, 1e-300, 0.0, np.inf, np.nan, 5e-324):
            for exposure, wp in SETTINGS:
                want = _pool_picture(pl, which, exposure, wp, Lw)[pick]
                got = r.tone_mapped(name, exposure, wp, log_average=Lw)
                assert got.shape == (H, W, 3) and got.dtype == np.uint8
                assert got.tobytes() == want.tobytes(), (name, exposure, wp, Lw, _differing(got, want, cls))


@pytest.mark.parametrize("W,H", ts.SIZES)
def test_tone_mapped_is_the_restatement_at_the_devices_log_average(W, H, handles, frames, pl):
    """tone_mapped(which) == apply(..., Lw = exp(tone_log_sum(which) / FB)) byte for byte, every kind of state"""
    r = handles(W, H)
    for kind in KINDS:
        cls, pick, acc, sums = frames(W, H, kind)
        r.load_packed_accumulators(acc)
        for which, name in enumerate(tr.PICTURES):
            Lw = tr.log_average(r.tone_log_sum(name), W * H)
            for exposure, wp in (SETTINGS[0], SETTINGS[1], SETTINGS[3]):
                want = tr.apply(pl[1], which, exposure, wp, Lw)[pick]
                got = r.tone_mapped(name, exposure, wp)
                assert got.tobytes() == want.tobytes(), (kind, name, exposure, wp, Lw, _differing(got, want, cls))


def _assert_host_outside_fragile(got, host, frag, what):
    d = np.abs(got.reshape(-1, 3).astype(np.int16) - host.reshape(-1, 3).astype(np.int16))
    assert not d[~frag].any(), (what, int((d[~frag] > 0).sum()), "bytes outside the fragile set differ")
    assert not frag.any() or d[frag].max() <= 1, (what, int(d[frag].max()))


@pytest.mark.parametrize("W,H", ts.SIZES)
def test_tone_mapped_is_the_host_property_outside_the_fragile_bytes(W, H, handles, frames, pl):
    """On ordinary states: the device's picture equals `image` / `unweighted_image` / `unidirectional_image` at every byte that
    cannot move when Lw moves by the sum's tolerance (fragile(): test_tone_cpu.py shows they are at most 1e-5 of the bytes here),
    and is within one count on those."""
    r = handles(W, H)
    cls, pick, acc, sums = frames(W, H, "ordinary")
    r.load_packed_accumulators(acc)
    for which, name in enumerate(tr.PICTURES):
        terms, exact, bound = sums[which]
        frag = tr.fragile(pl[1], which, 4.0, 1.0, tr.log_average(exact, W * H), bound / (W * H))[pick]
        got = r.tone_mapped(name)
        assert W * H < 64 or got.std() > 5                       # a picture, not a constant
        _assert_host_outside_fragile(got, _host(r, name), frag, name)


@pytest.mark.parametrize("W,H", ts.SIZES)
def test_calls_repeat_interleave_and_leave_the_accumulators(W, H, handles, frames):
    """The three pictures share d_tone_partial and d_tone_out: the same bytes on a second call and with the calls of the other
    pictures in between, and the accumulators are what was loaded, bit for bit (NaN payloads included)."""
    r = handles(W, H)
    cls, pick, acc, sums = frames(W, H, "finite")
    r.load_packed_accumulators(acc)
    first_sum = {n: r.tone_log_sum(n) for n in tr.PICTURES}
    first_pic = {n: r.tone_mapped(n).tobytes() for n in tr.PICTURES}
    for n in tr.PICTURES:
        assert r.tone_log_sum(n) == first_sum[n] and r.tone_mapped(n).tobytes() == first_pic[n]
    for n in reversed(tr.PICTURES):
        others = [m for m in tr.PICTURES if m != n]
        r.tone_mapped(others[0], 2.0, 1.5)
        assert r.tone_log_sum(n) == first_sum[n]
        r.tone_log_sum(others[1])
        r.tone_mapped(others[1], log_average=1.0)
        assert r.tone_mapped(n).tobytes() == first_pic[n]
    assert r.packed_accumulators().tobytes() == acc.tobytes()


def test_a_real_render(pl):
    """64 x 48 Cornell box, 3 sample streams, 4 passes; tone_mapped() is called straight after run_samples(), before anything
    reads the device (the drain before the kernels): the three pictures equal the restatement applied to packed_accumulators()
    byte for byte, the sums are within sum_bound, and the host properties agree outside the fragile bytes."""
    from clive2_amd.renderer import Renderer, stream_seeds
    W, H = 64, 48
    r = Renderer(_cornell(W, H), streams=3)
    r.set_seeds(stream_seeds(r.batch_size, 3))
    r.run_samples(4)
    pics = {n: r.tone_mapped(n) for n in tr.PICTURES}
    acc = r.packed_accumulators().reshape(8, -1)
    assert r.samples == 12 and acc[7].max() > 0
    for which, name in enumerate(tr.PICTURES):
        terms = tr.log_terms(acc, which)
        exact, bound = tr.exact_sum(terms), tr.sum_bound(terms, W * H)
        s = r.tone_log_sum(name)
        print(f"render {name}: |device sum - fsum| / sum_bound = {abs(s - exact) / bound:.4f}")
        assert abs(s - exact) <= bound
        want = tr.apply(acc, which, 4.0, 1.0, tr.log_average(s, W * H)).reshape(H, W, 3)
        assert pics[name].tobytes() == want.tobytes(), (name, int((pics[name] != want).sum()))
        assert pics[name].std() > 5
        frag = tr.fragile(acc, which, 4.0, 1.0, tr.log_average(exact, W * H), bound / (W * H))
        _assert_host_outside_fragile(pics[name], _host(r, name), frag, name)
    r.close()
