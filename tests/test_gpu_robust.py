"""The robust picture on the device (csrc/robust.hpp): the bucket hook against its float32 restatement (tests/robust_reference.py)
on the import, stage, fused and mapped paths, that buckets change nothing else, the picture and its statistics on injected states
(tests/robust_states.py) bit for bit, the validity rules, the reduce on a one-rank communicator, and real renders."""
import os
import subprocess
import sys

import numpy as np
import pytest

import error_reference as er
import robust_reference as rr
import robust_states as rst
from test_gpu_denoise import _cornell, _glass, _open_scene, _rmse

pytestmark = pytest.mark.gpu

F = np.float32
SCENES = {"cornell": lambda: _cornell(64, 48), "glass": lambda: _glass(64, 48), "open": lambda: _open_scene(72, 40)}


def _renderer(scene, K, M=8, seed=20240928, tracking=False, mode=None):
    from clive2_amd.renderer import Renderer, stream_seeds
    r = Renderer(scene, streams=K)
    r.set_seeds(stream_seeds(r.batch_size, K, seed=seed))
    r.set_reproducible(True)
    if mode is not None:
        r.set_traversal_mode(mode)
    if tracking:
        r.set_error_tracking(True)
    if M:
        r.set_robust_buckets(M)
    return r


def _bkt(r):
    return r.buckets().reshape(r.robust_buckets, 4, -1)


# ---------------------------------------------------------------- the hook
@pytest.mark.parametrize("K,M", [(1, 3), (1, 8), (3, 3), (3, 8)])
def test_buckets_of_imported_samples_equal_the_restatement(K, M):
    """Synthetic per-sample images through import_sample_images + process_images (k_accumulate<., true>), 41 x 25, K streams,
    2M + 2 passes, NaN and +-inf in the finalized colour: the buckets are those of the scrubbed addends in bucket (addends so
    far) % M, byte for byte; with error tracking on in the K = 3 cases (the <true, true> form)."""
    r = _renderer(_cornell(41, 25), K, M, tracking=K == 3)
    FB = r.batch_size
    assert FB == 41 * 25
    rs = np.random.RandomState(100 * K + M)
    a7, bkt, acc3 = np.zeros(FB, F), np.zeros((M, 4, FB), F), np.zeros((4, FB), F)
    for p in range(2 * M + 2):
        for k in range(K):
            fin = rs.gamma(1.0, 0.5, size=(FB, 4)).astype(F)
            fin[:, 3] = 1.0
            light = rs.gamma(1.0, 0.1, size=(FB, 4)).astype(F)
            sw = rs.uniform(0.5, 2.0, size=FB).astype(F)
            uni = rs.gamma(1.0, 0.5, size=(FB, 4)).astype(F)
            bad = rs.choice(FB, size=60, replace=False)
            fin[bad[:20], 0] = np.nan
            fin[bad[20:40], 1] = np.inf
            fin[bad[40:], 2] = -np.inf
            r.set_export_stream(k)
            r.import_sample_images(finalized=fin, light=light, sample_weights=sw, unidirectional=uni)
            x, w = er.addends(fin, light, sw)
            rr.add_bucket(bkt, a7, x, w)
            a7 = (a7 + F(1)).astype(F)
            acc3[:3] = (acc3[:3] + x.T).astype(F)
            acc3[3] = (acc3[3] + w).astype(F)
        r.process_images()
    got = _bkt(r)
    assert np.isfinite(got).all()
    assert got.tobytes() == bkt.tobytes()
    acc = r.packed_accumulators().reshape(8, -1)
    assert acc[:4].tobytes() == acc3.tobytes() and (acc[7] == a7).all()
    r.close()


def _sum_bound(n):
    """|sum_k bkt[k] - acc row| <= 2 (n - 1) u sum|addends|, u = 2^-24: both are float32 sums of the same n addends in different
    orders (the accumulator row one running sum; the buckets M running sums of about n / M addends, added up here in float64), and
    each is within (n - 1) u sum|x| of the exact sum to first order.  The colour addends are >= 0 here and the weights > 0, so
    sum|x| is the row itself up to that same error; the factor 2.1 leaves room for the second-order terms."""
    return 2.1 * (n - 1) * 2.0 ** -24


@pytest.mark.parametrize("name,K", [("cornell", 1), ("cornell", 2), ("glass", 1), ("glass", 2)])
def test_buckets_are_exact_on_the_stage_and_fused_paths(name, K):
    """2M + 3 passes (M = 8) as stage calls, each stream's per-sample images exported before process_images and its addends
    restated in numpy: the device buckets equal the float32 restatement bit for bit.  A fresh handle with the same seeds through
    run_samples (k_finalize_accumulate<., true>) gives the same bucket and accumulator bytes.  Row by row the buckets add up to
    the accumulator row within _sum_bound(n), and min(n, M) buckets per pixel are non-empty."""
    M, passes = 8, 19
    scene = SCENES[name]()
    r = _renderer(scene, K, M)
    FB = r.pixel_width * r.pixel_height
    a7, bkt = np.zeros(FB, F), np.zeros((M, 4, FB), F)
    for _ in range(passes):
        r.make_light_rays(); r.make_camera_rays(); r.trace_light_rays(); r.trace_camera_rays()
        r.join_paths(); r.finalize_samples(); r.gather_light_image()
        for k in range(K):
            r.set_export_stream(k)
            im = r.export_sample_images()
            x, w = er.addends(im["finalized"], im["light"], im["sample_weights"])
            rr.add_bucket(bkt, a7, x, w)
            a7 = (a7 + F(1)).astype(F)
        r.process_images()
    got = _bkt(r)
    assert got.tobytes() == bkt.tobytes()
    acc = r.packed_accumulators().reshape(8, -1)
    n = passes * K
    assert (acc[7] == n).all()
    _assert_buckets_add_up(got, acc, n, M)

    f = _renderer(scene, K, M)
    f.run_samples(passes)
    assert f.buckets().tobytes() == got.tobytes()
    assert f.packed_accumulators().tobytes() == acc.tobytes()
    r.close(); f.close()


def _assert_buckets_add_up(bkt, acc, n, M):
    tot = bkt.astype(np.float64).sum(0)
    mag = np.abs(bkt.astype(np.float64)).sum(0)
    err = np.abs(tot - acc[:4].astype(np.float64))
    worst = (err / np.where(mag > 0, mag, 1.0)).max()
    print(f"buckets against accumulators, n = {n}: worst |sum_k bkt - acc| / sum|bkt| = {worst:.3e}, bound {_sum_bound(n):.3e}")
    assert (err <= _sum_bound(n) * mag).all()
    assert ((bkt[:, 3] != 0).sum(0) == min(n, M)).all()          # every addend has a weight > 0: bucket k is non-empty iff k < n


def test_buckets_of_a_mapped_pass_sequence():
    """Adaptive sampling (k_finalize_accumulate_mapped<true, true>): 4 uniform passes, a density from the error estimate, 9 mapped
    passes, M = 8, K = 2.  The buckets add up to the accumulator rows within the bound, 8 buckets are non-empty, the accumulators
    and moments equal those of the same sequence with buckets off byte for byte, and the picture comes out."""
    scene = _glass(64, 48)
    a, b = _renderer(scene, 2, 0, tracking=True), _renderer(scene, 2, 8, tracking=True)
    for r in (a, b):
        r.run_samples(4)
        r.update_sample_density()
        r.run_samples(9)
    acc = b.packed_accumulators()
    assert acc.tobytes() == a.packed_accumulators().tobytes()
    assert b.moments().tobytes() == a.moments().tobytes()
    assert b.camera_samples().tobytes() == a.camera_samples().tobytes()
    _assert_buckets_add_up(_bkt(b), acc.reshape(8, -1), 26, 8)
    pic = b.robust_radiance()
    assert np.isfinite(pic).all() and (pic > 0).any()
    a.close(); b.close()


@pytest.mark.parametrize("name,K", [("cornell", 4), ("open", 4)])
def test_buckets_change_nothing_else(name, K):
    """Buckets off and on, error tracking on in both: the RNG buffer, the accumulators and the moments are byte-identical (and the
    accumulators equal those of a handle with neither)."""
    scene = SCENES[name]()
    mode = 5 if name == "open" else None
    plain = _renderer(scene, K, 0, mode=mode)
    a = _renderer(scene, K, 0, tracking=True, mode=mode)
    b = _renderer(scene, K, 8, tracking=True, mode=mode)
    for r in (plain, a, b):
        r.run_samples(8)
    assert a.packed_accumulators().tobytes() == b.packed_accumulators().tobytes() == plain.packed_accumulators().tobytes()
    assert a.get_random_buffer().tobytes() == b.get_random_buffer().tobytes() == plain.get_random_buffer().tobytes()
    assert a.moments().tobytes() == b.moments().tobytes()
    assert a.robust_buckets == 0 and b.robust_buckets == 8
    for r in (plain, a, b):
        r.close()


# ---------------------------------------------------------------- the picture on injected states
@pytest.fixture(scope="module")
def pools():
    """per M: the pool of pixel states and the restatement's picture and statistics of every one of them, computed once (the
    picture is a function of the pixel's buckets alone, so a frame's reference is the pool's, gathered)"""
    made = {}

    def get(M):
        if M not in made:
            pl = rst.pool(M)
            made[M] = (pl,) + rr.robust_picture(pl[2])
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


@pytest.mark.parametrize("W,H,M", [(7, 5, 3), (7, 5, 8), (7, 5, 16), (41, 25, 3), (41, 25, 8), (41, 25, 16), (1920, 1080, 16)])
def test_injected_states_picture_and_stats_bitwise(W, H, M, pools, handles):
    """Every class of tests/robust_states.py in every third wave: picture and (G, c) equal the restatement bit for bit, no pixel
    excluded.  1920 x 1080 with M = 16 is the largest buffer the feature allocates per pixel count in the suite (531 MB, indices
    up to 1.3e8 floats); the frames below a workgroup and with a partial last workgroup are 7 x 5 and 41 x 25."""
    pl, ref_pic, ref_st = pools(M)
    FB = W * H
    cls, pick = rst.picks(pl, FB, seed=W + M)
    bkt = np.ascontiguousarray(pl[2][:, :, pick])
    r = handles(W, H)
    r.set_robust_buckets(M)
    r.load_buckets(bkt)
    pic, st = r.robust_radiance(return_stats=True)
    assert pic.shape == (H, W, 3) and st.shape == (H, W, 2) and pic.dtype == st.dtype == np.float32
    want_pic, want_st = ref_pic[pick], ref_st[pick]
    if FB >= 64:
        assert set(np.unique(cls[:64])) == set(rst.ALL)
    same = (pic.reshape(FB, 3).view(np.uint32) == want_pic.view(np.uint32)).all(1) & \
           (st.reshape(FB, 2).view(np.uint32) == want_st.view(np.uint32)).all(1)
    bad = np.flatnonzero(~same)
    assert bad.size == 0, [(int(p), rst.NAMES[cls[p]], pic.reshape(FB, 3)[p], want_pic[p], st.reshape(FB, 2)[p], want_st[p])
                           for p in bad[:5]]
    assert np.isfinite(pic).all()
    assert r.robust_radiance().tobytes() == pic.tobytes()        # without the statistics: the same picture
    r.set_robust_buckets(0)


# ---------------------------------------------------------------- state rules
def test_state_rules():
    from clive2_amd.renderer import RendererError
    r = _renderer(_cornell(64, 48), 1, 0)
    FB = r.batch_size
    assert r.robust_buckets == 0
    for call in (r.robust_radiance, r.buckets, lambda: r.load_buckets(np.zeros(4 * 8 * FB, F))):   # the feature is off
        with pytest.raises(RendererError, match=r"\(-3\)"):
            call()
    for M in (1, 2, 17, -3):                                     # the C call refuses too (the binding's check bypassed)
        assert r._L.cl2_set_robust_buckets(r._h, M) == -1
    assert r.robust_buckets == 0
    r.set_robust_buckets(8)                                      # on over clean accumulators: valid
    assert r.robust_buckets == 8
    assert not r.buckets().any() and not r.robust_radiance().any()
    r.run_samples(3)
    pic, b8, acc = r.robust_radiance(), r.buckets(), r.packed_accumulators()
    assert b8.size == 4 * 8 * FB and pic.any()
    # wrong sizes
    buf = np.zeros(4 * 8 * FB + 4, F)
    p = buf.ctypes.data
    for n in (4 * 8 * FB - 1, 4 * 8 * FB + 1, 8 * FB, 0):
        assert r._L.cl2_read_buckets_packed(r._h, p, n) == -1
        assert r._L.cl2_write_buckets_packed(r._h, p, n) == -1
    assert r._L.cl2_robust_picture(r._h, p, 3 * FB - 1, None, 0) == -1
    assert r._L.cl2_robust_picture(r._h, p, 3 * FB, p, 2 * FB + 1) == -1
    assert r._L.cl2_robust_picture(r._h, p, 3 * FB, None, 2 * FB) == -1
    assert r.robust_radiance().tobytes() == pic.tobytes()        # the refused calls changed nothing
    # writing the accumulators invalidates; writing the buckets makes them valid again
    r.load_packed_accumulators(acc)
    with pytest.raises(RendererError, match=r"\(-3\).*cl2_reset_accumulators or cl2_write_buckets_packed"):
        r.robust_radiance()
    assert r.buckets().tobytes() == b8.tobytes()                 # reading works on invalid buckets
    r.load_buckets(b8)
    assert r.robust_radiance().tobytes() == pic.tobytes()
    # another M over accumulators that hold sums: a new, zeroed buffer, invalid
    r.set_robust_buckets(4)
    assert r.robust_buckets == 4 and r.buckets().size == 4 * 4 * FB and not r.buckets().any()
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.robust_radiance()
    r.set_robust_buckets(4)                                      # the same M again: nothing happens
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.robust_radiance()
    # reset zeroes and makes valid
    r.run_samples(1)
    assert r.buckets().any()
    r.reset_accumulators()
    assert not r.buckets().any() and not r.robust_radiance().any()
    r.run_samples(2)
    assert r.robust_radiance().any()
    # off and on again over accumulators that hold sums: invalid until a reset
    r.set_robust_buckets(0)
    assert r.robust_buckets == 0
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.buckets()
    r.set_robust_buckets(8)
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.robust_radiance()
    r.reset_accumulators()
    r.set_robust_buckets(5)                                      # another M over clean accumulators: valid
    assert not r.robust_radiance().any()
    r.close()


# ---------------------------------------------------------------- reduce
def test_reduce_on_one_rank_keeps_the_buckets(tmp_path):
    """cl2_reduce_accumulators on a one-rank communicator, in a fresh child process (tests/robust_comm_child.py): the sum over one
    rank returns the same bucket bytes, and they stay valid."""
    child = os.path.join(os.path.dirname(__file__), "robust_comm_child.py")
    env = dict(os.environ, CLIVE2_RENDEZVOUS_FILE=str(tmp_path / "rccl_id"), HSA_ENABLE_IPC_MODE_LEGACY="0")
    try:
        p = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300, env=env)
        out, err, rc = p.stdout, p.stderr, p.returncode
    except subprocess.TimeoutExpired as e:
        dec = lambda b: b.decode(errors="replace") if isinstance(b, bytes) else (b or "")
        out, err, rc = dec(e.stdout), dec(e.stderr), None
    steps = [l.split()[1] for l in out.splitlines() if l.startswith("STEP ")]
    assert rc is not None, f"the RCCL child hung after steps {steps}"
    assert rc == 0, (rc, steps, out[-2000:], err[-3000:])
    assert steps == ["rendered", "comm-up", "reduced-same-bytes", "picture-same-bytes", "invalid-stays-invalid", "comm-down", "closed"], steps


# ---------------------------------------------------------------- real renders
# robust / raw relative MSE of the Cornell box measured on the MI355X (profiles/robust_quality_mi355x.json): nothing is trimmed there at
# 64 and 256 passes, so the two pictures differ by the order of their float32 sums only
CORNELL_RATIO = {64: 0.99999994, 256: 0.99999989}


@pytest.mark.parametrize("name", ["cornell", "glass"])
def test_real_renders(name):
    """256 x 192, M = 8, relative MSE (_rmse of tests/test_gpu_denoise.py) against 1024 passes of seed 4321.  Glass scene at 256
    passes: robust <= raw.  Cornell box at 64 and at 256 passes: robust <= 1.25 x the ratio measured on the MI355X
    (tools/robust_quality.py, profiles/robust_quality_mi355x.json) x raw -- one seed's figure of a noisy quantity, hence the
    quarter.  Measured there, raw / robust: glass scene 6.60e-4 / 3.58e-4 at 64 passes and 1.65e-3 / 2.11e-4 at 256 (0.5 % of the
    pixels trimmed); Cornell box 1.42e-5 and 4.22e-6 for both pictures (nothing trimmed, ratios 0.99999994 and 0.99999989)."""
    from clive2_amd.renderer import Renderer, make_seeds
    W, H = 256, 192
    scene = {"cornell": _cornell, "glass": _glass}[name](W, H)
    ref_r = Renderer(scene, seeds=make_seeds(W * H, seed=4321))
    ref_r.run_samples(1024)
    ref = ref_r.radiance
    ref_r.close()
    r = Renderer(scene)
    r.set_robust_buckets(8)
    ratios = {}
    for n in (64, 256):
        r.run_samples(n - r.samples)
        raw, rob = _rmse(r.radiance, ref), _rmse(r.robust_radiance(), ref)
        ratios[n] = rob / raw
        st = r.robust_radiance(return_stats=True)[1]
        print(f"{name} {n} passes: rMSE raw {raw:.4g} robust {rob:.4g} (robust / raw {rob / raw:.3f}); trimmed pixels "
              f"{(st[..., 1] > 0).mean():.3f}, mean G {st[..., 0].mean():.3f}")
    r.close()
    if name == "glass":
        assert ratios[256] <= 1.0
    else:
        for n in (64, 256):
            assert ratios[n] <= 1.25 * CORNELL_RATIO[n]
