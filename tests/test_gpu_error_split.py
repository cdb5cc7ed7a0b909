"""Split tracking and the split noise model on the device (csrc/error_split.hpp, noise model 2 of csrc/denoise_error.hpp, DESIGN.md
6.17) against their numpy statement (tests/error_split_reference.py): the split rows bit for bit on the stage, fused and import
paths, that nothing else moves, cl2_light_share and the mixed perturbation on injected states, the *_model calls against the old
calls, the state rules, and the ordering of the three models' divergence totals on a real render."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_error_reference as de
import denoise_scenes as ds
import error_reference as er
import error_split_reference as sp
import error_states as es
import feature_states as fs

pytestmark = pytest.mark.gpu

F = np.float32
D = np.float64
FRAMES = [(7, 5), (41, 25)]
KINDS = ("denoised", "guided")
EPS = 1 / 16
INT_COUNTERS = ("rays", "conn_rays", "box_tests", "tri_tests", "counted_rays", "samples", "launches_traverse_paths",
                "launches_traverse_conn", "rays_traverse_paths", "rays_traverse_conn")
SCENES = {"cornell": ds.cornell, "glass": ds.glass}


def _renderer(scene, K=1, seed=20240928, split=True):
    from clive2_amd.renderer import Renderer, stream_seeds
    r = Renderer(scene, streams=K)
    r.set_seeds(stream_seeds(r.batch_size, K, seed=seed))
    r.set_reproducible(True)
    r.set_error_tracking(True)
    if split:
        r.set_split_tracking(True)
    return r


# ---------------------------------------------------------------- the split rows
@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("name,K", [("cornell", 1), ("cornell", 2), ("glass", 1), ("glass", 2)])
def test_split_rows_on_the_stage_and_fused_paths(name, K, W, H):
    """Four passes as stage calls, each stream's per-sample images exported before process_images and its parts restated in numpy:
    the device's rows equal the float32 sums bit for bit (k_split_moments_staged).  A fresh handle with the same seeds through
    run_samples(4) (k_split_moments_fused: the nine-tap gather repeated) gives the same bytes."""
    scene = SCENES[name](W, H)
    r = _renderer(scene, K)
    assert r.split_tracking and r.error_tracking
    rows = np.zeros((6, r.batch_size), F)
    for _ in range(4):
        r.make_light_rays(); r.make_camera_rays(); r.trace_light_rays(); r.trace_camera_rays()
        r.join_paths(); r.finalize_samples(); r.gather_light_image()
        for k in range(K):
            r.set_export_stream(k)
            im = r.export_sample_images()
            sp.add_split_moments(rows, im["finalized"], im["sample_weights"], im["light"])
        r.process_images()
    got = r.split_moments().reshape(6, -1)
    assert de.same(got, rows)
    assert got[:3].any() and got[3:].any()                     # both parts carry something
    acc, mom = r.packed_accumulators(), r.moments()
    r.close()
    f = _renderer(scene, K)
    f.run_samples(4)
    assert de.same(f.split_moments().reshape(6, -1), got)
    assert f.packed_accumulators().tobytes() == acc.tobytes() and f.moments().tobytes() == mom.tobytes()
    f.close()


@pytest.mark.parametrize("W,H", FRAMES)
def test_split_rows_of_imported_samples(W, H):
    """Synthetic per-sample images through import_sample_images + process_images with NaN, +-inf and -0 in either part and a light
    weight l.w that is not 0: the rows are those of the parts scrubbed one by one, bit for bit, and the moments stay the sum's."""
    r = _renderer(ds.cornell(W, H))
    B = r.batch_size
    rs = np.random.RandomState(5)
    rows, mom = np.zeros((6, B), F), np.zeros((8, B), F)
    for p in range(3):
        fin = rs.gamma(1.0, 0.5, size=(B, 4)).astype(F)
        fin[:, 3] = 1.0
        light = rs.gamma(1.0, 0.1, size=(B, 4)).astype(F)
        light[:, 3] = np.where(rs.uniform(size=B) < 0.5, 0.0, rs.uniform(0.1, 0.5, size=B)).astype(F)
        sw = rs.uniform(0.5, 2.0, size=B).astype(F)
        uni = rs.gamma(1.0, 0.5, size=(B, 4)).astype(F)
        bad = rs.choice(B, size=min(B, 32), replace=False)
        for k, (arr, ch, val) in enumerate(((fin, 0, np.nan), (fin, 1, np.inf), (fin, 2, -np.inf), (fin, 0, -0.0),
                                            (light, 0, np.nan), (light, 1, np.inf), (light, 2, -np.inf), (light, 1, -0.0))):
            arr[bad[k::8], ch] = val
        r.import_sample_images(finalized=fin, light=light, sample_weights=sw, unidirectional=uni)
        r.process_images()
        sp.add_split_moments(rows, fin, sw, light)
        er.add_moments(mom, *er.addends(fin, light, sw))
    got = r.split_moments().reshape(6, -1)
    assert np.isfinite(got).all() and de.same(got, rows)
    assert r.moments().reshape(8, -1).tobytes() == mom.tobytes()
    r.close()


def test_nothing_else_moves():
    """Accumulators, moments, buckets (M = 8), layer accumulators, seeds and ray counts of a render with split tracking on equal
    those with it off, byte for byte (K = 2, the fused path; then one pass of stage calls)"""
    from clive2_amd import strategies
    scene = ds.cornell(41, 25)
    out = []
    for split in (False, True):
        r = _renderer(scene, 2, split=split)
        r.set_robust_buckets(8)
        r.set_layers(strategies.LAYERS)
        r.run_samples(6)
        r.make_light_rays(); r.make_camera_rays(); r.trace_light_rays(); r.trace_camera_rays()
        r.join_paths(); r.finalize_samples(); r.gather_light_image(); r.process_images()
        c = r.counters()
        out.append([r.packed_accumulators(), r.moments(), r.buckets(), r.layer_accumulators(), r.get_random_buffer(),
                    np.array([c[k] for k in INT_COUNTERS], np.uint64)])
        assert r.split_tracking == split
        r.close()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- injected states
@pytest.fixture(scope="module")
def pool():
    return es.pool()


class Case:
    """a handle with injected accumulators, moments, split rows and features, and what the kernels make of them"""

    def __init__(self, W, H, acc, mom, smom):
        from clive2_amd.renderer import Renderer
        self.W, self.H = W, H
        self.scene = ds.cornell(W, H)
        self.r = r = Renderer(self.scene)
        r.set_split_tracking(True)
        _, n, z, a, cov = fs.features(W, H)
        self.acc, self.mom, self.smom = acc, mom, smom
        r.load_packed_accumulators(acc)
        r.load_moments(mom)
        r.load_split_moments(smom)
        r.load_features(n, z, a, cov)
        self.f = dict(normal=n, depth=z, albedo=a, coverage=cov)
        self.y, self.state, self.v, self.a, self.w = de.inputs(acc, mom, W, H)
        self.K = de.camera_kernel(self.scene)
        self.rho = sp.light_share(acc, mom, smom)[0].reshape(H, W)

    def call(self, kind, **kw):
        return self.r.denoised_error(kind, epsilon=EPS, return_map=True, return_totals=True, return_probe=True, **kw)

    def restated(self, probes, floor):
        yps, Fyps = zip(*[(p[0], p[2]) for p in probes])
        return de.terms(self.y, yps, probes[0][1], Fyps, self.state, self.v, EPS, floor)

    def select(self, model, entry, K=3, S=2, probes=1, seed=0, floor=0.001, sigma=(2.0, 0.1, 0.1)):
        """every output of cl2_denoise_select (entry 'old') or cl2_denoise_select_model"""
        from clive2_amd._native import ptr
        H, W, n = self.H, self.W, K + 1
        o = dict(picture=np.empty((H, W, 3), F), scale=np.empty((H, W), np.int32), maps=np.empty((2, n, H, W), F),
                 out=(C.c_double * 8)())
        fn = self.r._L.cl2_denoise_select if entry == "old" else self.r._L.cl2_denoise_select_model
        rc = fn(self.r._h, K, sigma[0], sigma[1], sigma[2], probes, EPS, model, C.c_uint32(seed & 0xFFFFFFFF), S, floor,
                ptr(o["picture"]), C.c_size_t(o["picture"].size), ptr(o["scale"]), C.c_size_t(o["scale"].size), o["out"],
                ptr(o["maps"]), C.c_size_t(o["maps"].size), None, C.c_size_t(0))
        assert rc == 0, self.r._L.cl2_last_error(self.r._h)
        o["out"] = np.array(o["out"][:], D)
        return o


def _state(pool, W, H, which):
    if which == "all":
        cls = fs.features(W, H)[0]
        acc = fs.colours(cls, pool, wild=False)[1]
        mom = es.state(pool, W * H, es.ALL)[2]
    else:
        _, acc, mom = es.state(pool, W * H, es.BASE)
    return acc, mom


@pytest.fixture(scope="module")
def cases(pool):
    """per frame: 'all' = the calm colours of feature_states under the moments of every class of error_states and the split rows of
    every class of error_split_reference.split_rows_for; 'base' = the well-scaled classes of both; 'one' = 'base' with rho = 1
    everywhere (the camera rows 0, the light rows noisy)"""
    made = {}

    def get(W, H, which):
        if (W, H, which) not in made:
            acc, mom = _state(pool, W, H, "all" if which == "all" else "base")
            if which == "all":
                smom = sp.split_rows_for(acc, mom)[1]
            elif which == "base":
                smom = sp.split_rows_for(acc, mom, allowed=(sp.BOTH, sp.QUIET, sp.CAMERA_ONLY, sp.LIGHT_ONLY, sp.CANCEL))[1]
            else:
                smom = sp.split_rows_for(acc, mom, allowed=(sp.BOTH, sp.QUIET, sp.CAMERA_ONLY, sp.LIGHT_ONLY, sp.CANCEL))[1]
                smom[:3] = 0                                   # no camera part anywhere: S_c = 0
            made[(W, H, which)] = Case(W, H, acc, mom, smom)
        return made[(W, H, which)]
    yield get
    for c in made.values():
        c.r.close()


@pytest.mark.parametrize("W,H", FRAMES + [(512, 513)])
def test_light_share_on_injected_states(W, H, pool):
    """cl2_light_share on every class of accumulator / moment state (uncovered, n = 0 and 1, overflowed sums among them) under
    every class of split rows (both parts noiseless, only one part noisy, cancellation to either sign, overflowed sums, NaN
    rows): the map and the four totals equal the float64 restatement bit for bit, the totals in the device's reduction order
    (512 x 513: a partial second grid-stride trip); the same bytes on a second call; then the well-scaled classes alone, where
    the frame's share lies strictly inside (0, 1)."""
    from clive2_amd.renderer import Renderer
    r = Renderer(ds.cornell(W, H))
    r.set_split_tracking(True)
    for allowed in (es.ALL, es.BASE):
        cls, acc, mom = es.state(pool, W * H, allowed)
        scls, smom = sp.split_rows_for(acc, mom)
        if W * H >= 576:
            assert set(np.unique(scls)) == set(sp.SPLIT_CLASSES)
        r.load_packed_accumulators(acc)
        r.load_moments(mom)
        r.load_split_moments(smom)
        share, m = r.light_share(return_map=True)
        out = (C.c_double * 4)()
        assert r._L.cl2_light_share(r._h, None, 0, out) == 0
        want_m, want = sp.light_share(acc, mom, smom)
        assert m.dtype == F and not np.isnan(m).any() and ((m >= 0) & (m <= 1)).all()
        bad = np.flatnonzero(m.reshape(-1).view(np.uint32) != want_m.view(np.uint32))
        assert bad.size == 0, (len(bad), [(cls[p], scls[p], m.reshape(-1)[p], want_m[p]) for p in bad[:5]])
        assert de.same(np.array(out[:], D), want), (out[:], want)
        assert share == want[0] and np.isfinite(want).all()
        state = er.variances(acc, mom)[0]
        assert (m.reshape(-1)[state != 2] == 1).all()
        for c, v in ((sp.QUIET, 1.0), (sp.CAMERA_ONLY, 0.0), (sp.LIGHT_ONLY, 1.0), (sp.NANS, 1.0), (sp.OVERFLOW, 1.0)):
            at = (scls == c) & (state == 2)
            if c == sp.CAMERA_ONLY:                            # a camera part that cancels to <= 0 leaves nothing: 1
                at &= want_m != 1
            assert (m.reshape(-1)[at] == v).all(), c
        assert r.light_share(return_map=True)[1].tobytes() == m.tobytes()
    assert 0.0 < share < 1.0 and want[3] > 0
    r.close()


@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("which", ["all", "base"])
def test_perturbed_picture_of_the_split_model_bit_for_bit(W, H, which, cases):
    """y' of noise model 2 equals the restatement bit for bit under the mixed rho of the injected rows: border pixels, states 0
    and 1 (unperturbed) and every class of rows included"""
    c = cases(W, H, which)
    assert len(np.unique(c.rho)) > 3 and (c.rho == 0).any() and (c.rho == 1).any()
    for kind in KINDS:
        for seed in (0, 7, 0xFFFFFFFF):
            yp = c.call(kind, iterations=1, noise="split", seed=seed)[3][0]
            want = sp.perturb_split(c.y, c.a, c.rho, seed, EPS, c.K)
            assert np.isfinite(want).all()
            assert de.same(yp, want), (kind, seed)
            assert (yp[c.state != 2] == c.y[c.state != 2]).all()          # in value: y + 0 turns a -0 of y into +0
    yp3 = c.call("denoised", iterations=0, noise="split", seed=5, probes=3)[3][0]
    assert de.same(yp3, sp.perturb_split(c.y, c.a, c.rho, 7, EPS, c.K))


@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["all", "base"])
def test_map_and_totals_of_the_split_model_bit_for_bit(W, H, kind, which, cases):
    """cl2_denoise_error_model(.., 2) at 0, 1 and 3 passes.  probes = 1: the map and all eight totals equal the restatement
    evaluated on the device's own y', F(y), F(y'); probes = 4: the restatement built from four single-probe calls with seeds
    S .. S + 3 (S + 2 wraps); two calls give the same bytes."""
    c = cases(W, H, which)
    S, floor = 0xFFFFFFFE, 0.001
    for it in (0, 1, 3):
        singles = []
        for k in range(4):
            e, m, out, probe = c.call(kind, iterations=it, noise="split", seed=S + k, floor=floor)
            wm, wout = c.restated([probe], floor)
            assert de.same(m, wm) and de.same(out, wout), (kind, it, k, out, wout)
            assert de.same(np.float64(e), np.float64(wout[0]))
            singles.append(probe)
        e, m, out, probe = c.call(kind, iterations=it, noise="split", seed=S, floor=floor, probes=4)
        wm, wout = c.restated(singles, floor)
        assert de.same(m, wm) and de.same(out, wout), (kind, it, out, wout)
        assert all(de.same(x, y) for x, y in zip(probe, singles[3]))
        e2, m2, out2, _ = c.call(kind, iterations=it, noise="split", seed=S, floor=floor, probes=4)
        assert de.same(m, m2) and de.same(out, out2)
        if which == "base":
            assert np.isfinite(out).all() and out[6] == er.grid_sum(np.where(c.state == 2, c.v.astype(D), 0.0))


@pytest.mark.parametrize("W,H", FRAMES)
def test_model_calls_against_the_old_calls(W, H, cases):
    """noise model 0 and 1 through the *_model entry points return the old calls' bytes -- e_dn, map, totals and the three probe
    pictures; the scale selection's picture, scale map, maps and totals.  With rho = 1 everywhere model 2 is the independent
    mode with the signs of seed ^ 0xA5A5A5A5: one probe (probe k of the split model hashes (S + k) ^ 0xA5A5A5A5, which is
    (S ^ 0xA5A5A5A5) + k for k = 0 only)."""
    c = cases(W, H, "base")
    for kind in KINDS:
        for model, name in ((0, "independent"), (1, "correlated")):
            for probes in (1, 3):
                old = c.call(kind, correlated=model, seed=9, probes=probes)
                new = c.call(kind, noise=name, seed=9, probes=probes)
                assert old[0] == new[0] and de.same(old[1], new[1]) and de.same(old[2], new[2])
                assert all(de.same(x, y) for x, y in zip(old[3], new[3]))
    for model in (0, 1):
        old, new = c.select(model, "old", probes=2, seed=4), c.select(model, "model", probes=2, seed=4)
        for k in ("picture", "scale", "maps", "out"):
            assert de.same(old[k], new[k]), (model, k)
    one = cases(W, H, "one")
    assert (one.rho == 1).all()
    S = 0x12345678
    for kind in KINDS:
        old = one.call(kind, correlated=0, seed=S ^ sp.SIGN_XOR)
        new = one.call(kind, noise="split", seed=S)
        assert old[0] == new[0] and de.same(old[1], new[1]) and de.same(old[2], new[2])
        assert all(de.same(x, y) for x, y in zip(old[3], new[3]))
    old, new = one.select(0, "old", seed=S ^ sp.SIGN_XOR), one.select(2, "model", seed=S)
    for k in ("picture", "scale", "maps", "out"):
        assert de.same(old[k], new[k]), k
    # the kept picture of the model call is the selected picture of the same arguments
    one.r.keep_selected_picture(noise="split", seed=S, iterations=3, smooth_passes=2)
    assert one.r.kept_kind == "selected" and one.r.kept_picture().tobytes() == one.select(2, "model", seed=S)["picture"].tobytes()
    one.r.keep_picture(None)


# ---------------------------------------------------------------- state rules and refusals
def test_state_rules_and_refusals():
    from clive2_amd.renderer import Renderer, RendererError
    from clive2_amd._native import ptr
    W, H = 41, 25
    r = Renderer(ds.cornell(W, H))
    r.set_error_tracking(True)
    r.render_features(1)
    out4, out8 = (C.c_double * 4)(), (C.c_double * 8)()

    def model2(model=2):
        return r._L.cl2_denoise_error_model(r._h, 0, 3, 2.0, 0.1, 0.1, 1, EPS, model, C.c_uint32(0), 0.001, out8, None, C.c_size_t(0),
                                            None, C.c_size_t(0))

    def select2():
        return r._L.cl2_denoise_select_model(r._h, 3, 2.0, 0.1, 0.1, 1, EPS, 2, C.c_uint32(0), 2, 0.001, None, C.c_size_t(0), None,
                                             C.c_size_t(0), out8, None, C.c_size_t(0), None, C.c_size_t(0))

    def refused():
        """every call that needs valid rows returns CL2_E_STATE"""
        assert r._L.cl2_light_share(r._h, None, C.c_size_t(0), out4) == -3 and model2() == -3 and select2() == -3
        assert r._L.cl2_keep_selected_picture_model(r._h, 3, 2.0, 0.1, 0.1, 1, EPS, 2, C.c_uint32(0), 2) == -3
        with pytest.raises(RendererError, match=r"\(-3\)"):
            r.split_moments()
    r.run_samples(2)
    assert not r.split_tracking
    refused()                                                    # tracking off
    assert model2(0) == 0 and model2(1) == 0                     # the pure models do not need the rows
    r.set_split_tracking(True)                                   # over existing samples: invalid before a reset
    assert r.split_tracking
    refused()
    r.reset_accumulators()
    assert not r.split_moments().any()
    r.run_samples(3)
    acc, mom, rows = r.packed_accumulators(), r.moments(), r.split_moments()
    share, m = r.light_share(return_map=True)
    e = r.denoised_error(noise="split", seed=3)
    assert np.isfinite(e) and 0.0 <= share <= 1.0 and select2() == 0
    r.keep_picture("denoised")
    kept = r.kept_picture()
    r.load_packed_accumulators(acc)                              # accumulators written without their rows
    r.load_moments(mom)
    refused()
    assert r.kept_kind == "denoised" and r.kept_picture().tobytes() == kept.tobytes()      # a refused call changes nothing
    assert r.packed_accumulators().tobytes() == acc.tobytes() and r.moments().tobytes() == mom.tobytes()
    r.load_split_moments(rows)
    assert r.light_share() == share and r.denoised_error(noise="split", seed=3) == e
    assert r.split_moments().tobytes() == rows.tobytes()
    r.keep_picture(None)
    # argument checks
    assert model2(3) == -1 and model2(-1) == -1
    assert r._L.cl2_denoise_error(r._h, 0, 3, 2.0, 0.1, 0.1, 1, EPS, 2, C.c_uint32(0), 0.001, out8, None, C.c_size_t(0), None,
                                  C.c_size_t(0)) == -1          # the old call keeps its 0..1 check
    assert b"correlated must be 0 or 1" in r._L.cl2_last_error(r._h)
    assert r._L.cl2_set_split_tracking(r._h, 2) == -1
    buf = np.zeros(6 * W * H, F)
    assert r._L.cl2_read_split_moments_packed(r._h, ptr(buf), C.c_size_t(buf.size - 1)) == -1
    assert r._L.cl2_write_split_moments_packed(r._h, ptr(buf), C.c_size_t(buf.size + 1)) == -1
    assert r._L.cl2_light_share(r._h, ptr(buf), C.c_size_t(W * H - 1), out4) == -1
    assert r._L.cl2_light_share(r._h, None, C.c_size_t(0), None) == -1
    # a sample density has no split form, either way round
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.set_sample_density(np.ones((H, W), F))
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.update_sample_density()
    with pytest.raises(RendererError, match=r"\(-3\)"):
        r.render_until(0.01, 8, adaptive=True)
    assert r.sample_density().min() == 1 and r.packed_accumulators().tobytes() == acc.tobytes()
    r.set_split_tracking(False)
    assert not r.split_tracking and r.error_tracking
    r.set_sample_density(np.ones((H, W), F))
    assert r._L.cl2_set_split_tracking(r._h, 1) == -3 and not r.split_tracking
    r.set_sample_density(None)
    r.set_split_tracking(True)
    assert r.split_tracking
    # render_until on the split model turns the tracking on by itself
    r.close()
    u = Renderer(ds.cornell(W, H))
    done, e = u.render_until(1e-6, 10, metric="denoised", filter_params=dict(noise="split"))
    assert done == 10 and u.split_tracking and np.isfinite(e) and 0 < u.light_share() < 1
    u.close()


def test_reduce_leaves_the_split_rows_invalid(tmp_path):
    """cl2_reduce_accumulators on a one-rank communicator (a child process, the pattern of test_gpu_parity's RCCL test): the rows
    are not reduced, every call that needs them returns -3 afterwards; a hang is a failure and the STEP trace says where"""
    child = os.path.join(os.path.dirname(__file__), "split_reduce_child.py")
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
    assert steps == ["rendered", "comm-up", "reduced", "rows-invalid", "rows-valid-again", "closed"]


def test_cli_with_the_split_model(tmp_path, capsys):
    from clive2_amd import render
    out, rho = tmp_path / "s.png", tmp_path / "rho.npy"
    args = ["--scene", "empty", "--width", "64", "--height", "48", "--samples", "16", "--denoise", "--select-scale",
            "--noise-model", "split", "--light-share-out", str(rho), "--out", str(out)]
    assert render.main(args) == 0
    assert out.exists() or (tmp_path / "s.png.npy").exists()
    m = np.load(rho)
    assert m.shape == (48, 64) and m.dtype == F and ((m >= 0) & (m <= 1)).all() and len(np.unique(m)) > 100
    assert "light share of the frame's luma variance" in capsys.readouterr().out


# ---------------------------------------------------------------- ordering on a real render
ORDER_FRAME, ORDER_SAMPLES = (48, 36), 16


def test_divergence_total_of_the_split_model_lies_between_the_pure_ones():
    """The fixed filter at its defaults on the Cornell box, ORDER_FRAME with ORDER_SAMPLES samples, four probes, the same seed:
    out[7] (the sum of 2 div) of noise model 2 lies between model 0's and model 1's.  For a filter with non-negative weights this
    follows from the covariances: every off-diagonal entry of the split field's is cs_p cs_q <= 1 times the correlated one's.
    The frame is the smallest tried at which the pure modes' totals differ by more than four times the spread (max - min) of
    model 2's total over four seeds -- a condition on the frame, asserted below, not a tolerance.
    Measured on the MI355X (sum of 2 div x 1e-4: independent / split / correlated; model 2 over the four seeds; gap / spread):
        32 x 24    0.985 / 1.169 / 1.523    1.125 .. 1.386    2.06   (the condition fails)
        48 x 36    0.785 / 1.155 / 2.011    1.069 .. 1.239    7.19   <- the smallest frame that meets it
        64 x 48    1.270 / 2.155 / 3.469    1.667 .. 2.308    3.43   (fails: the spread is one seed's luck, not monotone in the frame)
        96 x 72    1.923 / 3.192 / 5.021    3.192 .. 3.469   11.18
        128 x 96   2.520 / 4.152 / 7.967    4.152 .. 4.958    6.76
    The split total lay between the pure ones at every size; the light share was 0.60 .. 0.61 at every size.
    The frame's light share lies strictly inside (0, 1)."""
    r = _renderer(ds.cornell(*ORDER_FRAME))
    r.run_samples(ORDER_SAMPLES)
    r.render_features(4)
    tot = {name: r.denoised_error("denoised", noise=name, probes=4, seed=40, return_totals=True)[1][7]
           for name in ("independent", "correlated", "split")}
    spread = [r.denoised_error("denoised", noise="split", probes=4, seed=40 + 4 * k, return_totals=True)[1][7] for k in range(4)]
    share = r.light_share()
    r.close()
    gap = abs(tot["correlated"] - tot["independent"])
    print(f"sum 2 div: independent {tot['independent']:.6g}, split {tot['split']:.6g}, correlated {tot['correlated']:.6g}; "
          f"split over four seeds {min(spread):.6g} .. {max(spread):.6g}: gap / spread {gap / (max(spread) - min(spread)):.2f}; "
          f"light share {share:.4f}")
    assert gap > 4 * (max(spread) - min(spread))
    lo, hi = sorted((tot["independent"], tot["correlated"]))
    assert lo < tot["split"] < hi
    assert 0.0 < share < 1.0
