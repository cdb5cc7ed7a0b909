"""The kept picture and its tone map on the device (cl2_keep_picture ... cl2_picture_tone_map, csrc/tonemap_picture.hpp) against
their numpy statement (tests/picture_tone_reference.py) on injected pictures (tests/picture_states.py), 1 x 1 to 513 x 512:

    the log sum       within the derived sum_bound of math.fsum of the reference's terms; NaN where a term is (there is no scrub)
    the picture       given Lw, byte for byte -- no tolerance, no pixel excluded -- on every class, at Lw that reach the pole, 0, inf, NaN
    the host          at its own Lw, tone_map(kept_picture()) outside the fragile bytes, of which ordinary states have at most 16
    the producers     keep_picture(kind) leaves the bytes of the old call, on real renders and on injected states
    state rules, hygiene, the two CLIs

512 x 512 is exactly TONE_BLOCKS * 256 pixels (the last frame on which every thread adds one term), 513 x 512 the first with a
second grid-stride iteration and with all 1024 partials; 1 x 1, 7 x 1, 257 x 1 and 91 x 60 are below a wave, below a workgroup, one
workgroup + 1 and a ragged last workgroup (and 3 * W * H is 3, 21, 771 -- not multiples of the four values a thread of
k_picture_apply maps -- and 16380, a multiple).  Nothing larger takes another path and byte offsets stay far below 2^31."""
import ctypes as C
import os

import numpy as np
import pytest

import error_states as es
import feature_states as fs
import picture_states as ps
import picture_tone_reference as pr
import robust_states as rst
import tone_states as ts
from clive2_amd.camera import tone_map
from denoise_scenes import cornell as _cornell

pytestmark = pytest.mark.gpu

F = np.float32
SETTINGS = [(4.0, 1.0), (2.0, 1.5), (4.0, 0.25), (3.3, 1.0)]          # tests/test_gpu_tone.py
KINDS = ("denoised", "guided", "robust", "robust_guided")
OLD = {"denoised": "denoised_radiance", "guided": "guided_radiance", "robust": "robust_radiance", "robust_guided": "robust_guided_radiance"}


@pytest.fixture(scope="module")
def pl():
    return ps.pool()


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
def frames(pl):
    """per (W, H, kind): the picture and (terms, math.fsum of them, sum_bound): computed once, never written to"""
    made = {}

    def get(W, H, kind):
        if (W, H, kind) not in made:
            FB = W * H
            cls, pick, pic = ps.state(pl, FB, ps.KINDS[kind], seed=W + H)
            if FB >= 64:
                assert set(np.unique(cls[:64])) == set(ps.KINDS[kind])
            t = pr.terms(pic)
            pic.setflags(write=False)
            made[W, H, kind] = (cls, pick, pic, t, pr.exact_sum(t), pr.sum_bound(t, FB))
        return made[W, H, kind]
    return get


_APPLIED = {}


def _pool_picture(pl, exposure, wp, Lw):
    """apply() on the pool, kept: the sizes share most of their (exposure, white point, Lw)"""
    key = (exposure, wp, np.float64(Lw).tobytes())
    if key not in _APPLIED:
        _APPLIED[key] = pr.apply(pl[1], exposure, wp, Lw)
    return _APPLIED[key]


def _differing(got, want, cls):
    got, want = got.reshape(-1, 3), want.reshape(-1, 3)
    bad = np.flatnonzero((got != want).any(1))
    return f"{bad.size} pixels differ: " + str([(int(p), ps.NAMES[cls[p]], got[p].tolist(), want[p].tolist()) for p in bad[:5]])


def _host(pic):
    with np.errstate(all="ignore"):
        return tone_map(pic, exposure=4.0)


# ---------------------------------------------------------------- the log sum
@pytest.mark.parametrize("W,H", ps.SIZES)
def test_log_sum_is_within_the_derived_bound(W, H, handles, frames):
    r = handles(W, H)
    for kind in ps.KINDS:
        cls, pick, pic, t, exact, bound = frames(W, H, kind)
        r.load_picture(pic)
        assert r.kept_kind == "loaded"
        got = r.picture_log_sum()
        if W * H >= 64:
            assert np.isnan(exact) == (kind == "all")
        if not np.isfinite(exact):                    # a NONFINITE or POLE pixel: NaN for NaN (and inf for inf, below a wave)
            assert kind == "all" and (np.isnan(got) if np.isnan(exact) else got == exact), (kind, got, exact)
            continue
        print(f"{W}x{H} {kind}: device sum {got!r}, fsum {exact!r}, |difference| / sum_bound = {abs(got - exact) / bound:.4f}")
        assert abs(got - exact) <= bound, (kind, got, exact, bound)


@pytest.mark.parametrize("W,H", ps.SIZES)
def test_one_poisoned_pixel_makes_the_sum_nan(W, H, handles, frames):
    """Ordinary pictures with one pixel of luma -1 (first pixel, last pixel, the first pixel of the second grid-stride iteration):
    a sum that skips it is finite.  The picture is then all zero bytes, as the host's."""
    r = handles(W, H)
    pic = frames(W, H, "ordinary")[2]
    assert ps.poison_positions(W * H) == ts.poison_positions(W * H)
    for p in ps.poison_positions(W * H):
        bad = ps.poisoned(pic, p)
        r.load_picture(bad)
        assert np.isnan(r.picture_log_sum()), p
        got = r.tone_mapped_picture()
        assert got.shape == (H, W, 3) and got.dtype == np.uint8 and not got.any(), p
        assert got.tobytes() == _host(bad.reshape(H, W, 3)).tobytes(), p


# ---------------------------------------------------------------- the picture
@pytest.mark.parametrize("W,H", ps.SIZES)
def test_picture_given_the_log_average_is_bitwise(W, H, handles, frames, pl):
    """tone_mapped_picture(log_average=Lw) against apply(), no tolerance, every kind of state, the four (exposure, white point), at
    Lw = the host's own of the state, the host's of the frame's finite state, 1.0 (the pole), 1e-300, 0.0, +inf, NaN and 5e-324."""
    r = handles(W, H)
    twin = pr.host_log_average(frames(W, H, "finite")[2], W, H)
    assert np.isfinite(twin)
    for kind in ps.KINDS:
        cls, pick, pic = frames(W, H, kind)[:3]
        r.load_picture(pic)
        assert r.kept_picture().tobytes() == pic.tobytes()
        own = pr.host_log_average(pic, W, H)
        for Lw in (own, twin, 1.0, 1e-300, 0.0, np.inf, np.nan, 5e-324):
            for exposure, wp in SETTINGS:
                want = _pool_picture(pl, exposure, wp, Lw)[pick]
                got = r.tone_mapped_picture(exposure, wp, log_average=Lw)
                assert got.shape == (H, W, 3) and got.dtype == np.uint8
                assert got.tobytes() == want.tobytes(), (kind, exposure, wp, Lw, _differing(got, want, cls))


@pytest.mark.parametrize("W,H", ps.SIZES)
def test_tone_mapped_picture_is_the_restatement_at_the_devices_log_average(W, H, handles, frames, pl):
    r = handles(W, H)
    for kind in ps.KINDS:
        cls, pick, pic = frames(W, H, kind)[:3]
        r.load_picture(pic)
        Lw = pr.log_average(r.picture_log_sum(), W * H)
        for exposure, wp in (SETTINGS[0], SETTINGS[3]):
            want = pr.apply(pl[1], exposure, wp, Lw)[pick]
            got = r.tone_mapped_picture(exposure, wp)
            assert got.tobytes() == want.tobytes(), (kind, exposure, wp, Lw, _differing(got, want, cls))


@pytest.mark.parametrize("W,H", ps.SIZES)
def test_tone_mapped_picture_is_the_hosts_outside_the_fragile_bytes(W, H, handles, frames):
    """On ordinary states, at the picture's own Lw: the device's bytes equal tone_map(kept_picture()) wherever the byte cannot move
    when Lw moves by the sum's tolerance, and are within one count elsewhere.  More than 16 fragile bytes in a frame fail the test
    (the reference alone gives 0 at 7 x 1, 91 x 60, 512 x 512 and 513 x 512: tests/test_picture_tone_cpu.py)."""
    r = handles(W, H)
    cls, pick, pic, t, exact, bound = frames(W, H, "ordinary")
    r.load_picture(pic)
    frag = pr.fragile(pic, 4.0, 1.0, pr.log_average(exact, W * H), bound / (W * H))
    print(f"{W}x{H}: {int(frag.sum())} fragile bytes")
    assert frag.sum() <= 16
    got = r.tone_mapped_picture()
    host = _host(r.kept_picture())
    assert W * H < 64 or got.std() > 5                            # a picture, not a constant
    d = np.abs(got.reshape(-1, 3).astype(np.int16) - host.reshape(-1, 3).astype(np.int16))
    print(f"{W}x{H}: {int((d > 0).sum())} bytes differ from the host's")
    assert not d[~frag].any(), (int((d[~frag] > 0).sum()), "bytes outside the fragile set differ")
    assert not frag.any() or d[frag].max() <= 1


# ---------------------------------------------------------------- the producers
def _renderer(scene, K=1, seed=20240928):
    """error tracking and 8 buckets on, reproducible light image"""
    from clive2_amd.renderer import Renderer, stream_seeds
    r = Renderer(scene, streams=K)
    r.set_seeds(stream_seeds(r.batch_size, K, seed=seed))
    r.set_reproducible(True)
    r.set_error_tracking(True)
    r.set_robust_buckets(8)
    return r


def _check_producers(r, W, H, label):
    for kind in KINDS:
        old = getattr(r, OLD[kind])()
        r.keep_picture(kind)
        assert r.kept_kind == kind
        kept = r.kept_picture()
        assert kept.shape == (H, W, 3) and kept.dtype == F
        assert kept.tobytes() == old.tobytes(), (label, kind, int((kept.view(np.uint32) != old.view(np.uint32)).sum()))
        assert getattr(r, OLD[kind])().tobytes() == old.tobytes()      # the old call, after the new one: its own bytes still
        got = r.tone_mapped(kind)
        assert r.kept_kind == kind and r.kept_picture().tobytes() == old.tobytes()
        Lw = pr.log_average(r.picture_log_sum(), W * H)
        want = pr.apply(old, 4.0, 1.0, Lw).reshape(H, W, 3)
        assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), (label, kind, int((got != want).sum()))
        t = pr.terms(old)
        if np.isfinite(t).all():
            assert abs(r.picture_log_sum() - pr.exact_sum(t)) <= pr.sum_bound(t, W * H), (label, kind)
    # with arguments: the old call's with the same ones
    for kind, kw in (("denoised", dict(iterations=1, sigma_color=1.5)), ("guided", dict(iterations=0)),
                     ("robust_guided", dict(iterations=5, sigma_luma=2.0, sigma_depth=0.2, sigma_albedo=0.3))):
        r.keep_picture(kind, **kw)
        assert r.kept_picture().tobytes() == getattr(r, OLD[kind])(**kw).tobytes(), (label, kind, kw)


@pytest.mark.parametrize("K", [1, 2])
def test_producers_on_a_real_render(K):
    W, H = 70, 45                               # partial 16 x 16 tiles on both edges
    r = _renderer(_cornell(W, H), K)
    r.run_samples(4)
    r.render_features(2)
    _check_producers(r, W, H, f"K = {K}")
    assert r.tone_mapped("robust_guided").std() > 5
    r.close()


def test_producers_on_injected_states():
    """41 x 25: accumulators and moments of tests/error_states.py (every class), buckets of tests/robust_states.py (every class),
    features of tests/feature_states.py"""
    W, H, M = 41, 25, 8
    FB = W * H
    r = _renderer(_cornell(W, H))
    cls, acc, mom = es.state(es.pool(), FB, es.ALL)
    rpl = rst.pool(M)
    rcls, pick = rst.picks(rpl, FB)
    assert set(np.unique(cls)) == set(es.ALL) and set(np.unique(rcls)) == set(rst.ALL)
    r.load_packed_accumulators(acc)
    r.load_moments(mom)
    r.load_buckets(np.ascontiguousarray(rpl[2][:, :, pick]))
    r.load_features(*fs.features(W, H)[1:])
    _check_producers(r, W, H, "injected")
    r.close()


# ---------------------------------------------------------------- state rules
def test_state_rules():
    from clive2_amd.renderer import Renderer, RendererError
    from clive2_amd._native import ptr
    W, H = 32, 24
    scene = _cornell(W, H)
    r = Renderer(scene)
    L, h = r._L, r._h
    # CL2_E_STATE without a kept picture
    assert r.kept_kind is None
    for call in (r.kept_picture, r.picture_log_sum, r.tone_mapped_picture):
        with pytest.raises(RendererError, match=r"\(-3\).*no kept picture"):
            call()
    # the messages of the old calls are carried over
    r.run_samples(2)
    for kind in ("denoised", "guided", "robust_guided"):
        with pytest.raises(RendererError, match=r"\(-3\).*no features for the current scene"):
            r.keep_picture(kind)
    r.render_features(1)
    with pytest.raises(RendererError, match=r"\(-3\).*error tracking is off"):
        r.keep_picture("guided")
    for kind in ("robust", "robust_guided"):
        with pytest.raises(RendererError, match=r"\(-3\).*buckets are off"):
            r.keep_picture(kind)
    r.set_robust_buckets(8)
    r.set_error_tracking(True)
    with pytest.raises(RendererError, match=r"\(-3\).*cl2_reset_accumulators or cl2_write_buckets_packed"):
        r.keep_picture("robust")
    with pytest.raises(RendererError, match=r"\(-3\).*cl2_reset_accumulators or cl2_write_moments_packed"):
        r.keep_picture("guided")
    for kw, msg in ((dict(iterations=13), "iterations must be in 0..12"), (dict(sigma_depth=-1.0), "sigmas must be positive and finite"),
                    (dict(sigma_albedo=1e-23), "sigma_albedo\\^2 underflows"), (dict(iterations=12, sigma_color=1e-17), "sigma_color\\^2")):
        with pytest.raises(RendererError, match=r"\(-1\).*" + msg):
            r.keep_picture("denoised", **kw)
    for bad in (-1, 5, 6):
        assert L.cl2_keep_picture(h, bad, 3, 2.0, 0.1, 0.1) == -1
    assert r.kept_kind is None                                    # none of the refused calls made a picture
    # a refused keep preserves the previous picture
    x = np.random.RandomState(1).gamma(1.0, 0.5, (H, W, 3)).astype(F)
    r.load_picture(x)
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.keep_picture("robust")
    with pytest.raises(RendererError, match=r"\(-1\)"):
        r.keep_picture("denoised", iterations=-1)
    assert r.kept_kind == "loaded" and r.kept_picture().tobytes() == x.tobytes()
    # pointer and size errors
    out, byt = np.empty(3 * W * H, F), np.empty(3 * W * H, np.uint8)
    s = C.c_double(0.0)
    assert L.cl2_read_picture(h, None, C.c_size_t(out.size)) == -1 and L.cl2_read_picture(h, ptr(out), C.c_size_t(out.size - 1)) == -1
    assert L.cl2_write_picture(h, None, C.c_size_t(out.size)) == -1 and L.cl2_write_picture(h, ptr(out), C.c_size_t(out.size + 1)) == -1
    assert L.cl2_picture_log_sum(h, None) == -1
    assert L.cl2_picture_tone_map(h, 4.0, 1.0, 1.0, None, C.c_size_t(byt.size)) == -1
    assert L.cl2_picture_tone_map(h, 4.0, 1.0, 1.0, ptr(byt), C.c_size_t(byt.size - 1)) == -1
    assert r.kept_kind == "loaded" and r.kept_picture().tobytes() == x.tobytes()
    # kind 0 frees the picture
    r.keep_picture(None)
    assert r.kept_kind is None
    with pytest.raises(RendererError, match=r"\(-3\).*no kept picture"):
        r.kept_picture()
    r.keep_picture(None)                                          # twice: nothing to free
    # the snapshot survives run_samples, reset_accumulators and upload_scene
    r.keep_picture("denoised")
    kept, pic = r.kept_picture(), r.tone_mapped_picture()
    assert kept.tobytes() == r.denoised_radiance().tobytes() and pic.std() > 5
    r.run_samples(1)
    r.reset_accumulators()
    r.upload_scene(scene)
    assert r.kept_kind == "denoised" and r.kept_picture().tobytes() == kept.tobytes() and r.tone_mapped_picture().tobytes() == pic.tobytes()
    r.close()


# ---------------------------------------------------------------- hygiene
def test_the_two_tone_maps_share_their_buffers_without_mixing(handles, frames):
    W, H = 91, 60
    r = handles(W, H)
    acc = ts.state(ts.pool(), W * H, ts.ORDINARY_ONLY, seed=W + H)[2]
    r.load_packed_accumulators(acc)
    r.load_picture(frames(W, H, "finite")[2])
    img, img_sum = r.tone_mapped("image").tobytes(), r.tone_log_sum("image")
    pic, pic_sum = r.tone_mapped_picture().tobytes(), r.picture_log_sum()
    assert img != pic and img_sum != pic_sum
    for _ in range(2):
        assert r.picture_log_sum() == pic_sum
        assert r.tone_mapped("image").tobytes() == img
        assert r.tone_log_sum("image") == img_sum
        assert r.tone_mapped_picture().tobytes() == pic                # the same call twice: the same bytes
        assert r.tone_mapped_picture().tobytes() == pic
        r.tone_mapped_picture(2.0, 1.5, log_average=1.0)
        assert r.tone_mapped("image").tobytes() == img
    assert r.packed_accumulators().tobytes() == acc.tobytes()


def test_render_state_is_untouched():
    """seeds, packed accumulators, moments, buckets, features and counters byte for byte before and after every new call"""
    W, H = 64, 48
    r = _renderer(_cornell(W, H), 2)
    r.run_samples(2)
    r.render_features(2)

    def snapshot():
        f = r.features()
        return (r.get_random_buffer().tobytes(), r.packed_accumulators().tobytes(), r.moments().tobytes(), r.buckets().tobytes(),
                tuple(f[k].tobytes() for k in sorted(f)), r.counters(), r.walk_tallies())
    before = snapshot()
    first = {}
    for kind in KINDS:
        r.keep_picture(kind)
        first[kind] = (r.kept_picture().tobytes(), r.picture_log_sum(), r.tone_mapped_picture().tobytes(), r.tone_mapped(kind).tobytes())
        assert first[kind][2] == first[kind][3]
    r.load_picture(np.ones((H, W, 3), F))
    r.tone_mapped_picture(log_average=1.0)
    r.keep_picture(None)
    assert snapshot() == before
    for kind in KINDS:                                            # the same calls again: the same bytes
        r.keep_picture(kind)
        assert (r.kept_picture().tobytes(), r.picture_log_sum(), r.tone_mapped_picture().tobytes(), r.tone_mapped(kind).tobytes()) == first[kind]
    assert snapshot() == before
    r.close()


# ---------------------------------------------------------------- the CLIs
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1]


def test_cli_render_writes_the_device_picture(tmp_path):
    from clive2_amd import render
    from clive2_amd.renderer import Renderer, stream_seeds
    import clive2_amd as c2
    W, H = 64, 48
    out = tmp_path / "rd.png"
    assert render.main(["--scene", "empty", "--width", str(W), "--height", str(H), "--samples", "8", "--reproducible", "--robust-denoise",
                        "--device-tonemap", "--out", str(out)]) == 0
    r = Renderer(c2.create_scene_from_preset("empty", pixel_width=W, pixel_height=H))
    r.set_reproducible(True)
    r.set_robust_buckets(8)
    r.set_seeds(stream_seeds(W * H, 1))
    r.run_samples(8)
    r.render_features(4)
    want = r.tone_mapped("robust_guided")
    assert want.std() > 5 and _png(out).tobytes() == want.tobytes()
    r.close()


def test_cli_movie_writes_the_device_picture(tmp_path, monkeypatch):
    """movie.py has no --reproducible: the test's Renderer turns the fixed-order light image on, so that two renders give the
    same bytes"""
    from clive2_amd import movie
    from clive2_amd.renderer import Renderer
    from clive2_amd.scene import create_scene_from_preset_with_params

    class Reproducible(Renderer):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.set_reproducible(True)
    monkeypatch.setattr(movie, "Renderer", Reproducible)
    W, H = 64, 48
    assert movie.main(["--scene", "empty", "--width", str(W), "--height", str(H), "--samples", "4", "--movie-frames", "1", "--denoise",
                       "--device-tonemap", "--out-root", str(tmp_path), "--movie-name", "m"]) == 0
    r = Reproducible(create_scene_from_preset_with_params("empty", pixel_width=W, pixel_height=H, frame_idx=0, total_frames=1))
    r.run_samples(4)
    r.render_features(4)
    want = r.tone_mapped("denoised")
    assert want.std() > 5 and _png(os.path.join(str(tmp_path), "m", "frame_0000.png")).tobytes() == want.tobytes()
    r.close()
