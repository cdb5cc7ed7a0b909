"""The slim resolve kernel (csrc/connect_resolve.hpp: k_connect_resolve_slim) against k_connect_resolve,
which debug bit 27 launches in its place, and against the oracle.

The slim kernel changes where values live -- one word for a light vertex's triangle and material, no distance word in the hit
records of the t >= 2 pairs (t = 1 is peeled out of the t loop), two LDS rows fewer -- and nothing of what is computed: every
output of the resolve stage must have the same BYTES under both kernels.  Per case one sample goes through the stage calls on two
handles from the same seeds, and the strategy-pair mask, the aggregators, the unidirectional image and the light image are
compared as bytes (NaNs canonicalised); the slim form is then compared with the oracle as tests/test_gpu_parity.py does: aggregators
and unidirectional image bit for bit, light image to the tolerance of a sum whose order differs.

The light image and float atomics: without the reproducible switch the t = 1 contributions of a pixel are added in hardware order
(include/clive2_amd.h, cl2_set_reproducible: "two renders agree to a few ulp only"), so two runs of ONE kernel need not give the
same bytes -- measured for this file on the 64 x 48 Cornell box, four pairs of renders each: k_connect_resolve against itself 155 to
512 of the light image's 12,288 words differ, the slim kernel against itself 344 to 506, one against the other 444 to 470, while
aggregators, finalized samples and unidirectional image are identical.  The bytes of the light image are therefore compared
where they are defined, under the reproducible switch (every t = 1 contribution is a record {colour, weight} at a slot named by its
pair and pixel, summed in slot order): EVERY case is rendered with the switch as well, and its light image, which then holds every
contribution's colour and weight exactly, must be identical.  With atomics the two light images are held to the parity tests'
tolerance for that sum (rtol 2e-5, atol 1e-9), after printing how many words differ.

Frames: 64 x 48 = 12 full workgroups; 67 x 33 = 2,211 entries, a last workgroup with 93 lanes that own no pixel; 257 x 1.  The open
scene (emitter, floor, back wall and a glass ball: 328 triangles) has specular vertices on both subpaths, subpaths of every length and
connections culled for a specular endpoint.  Two sample streams at 67 x 33 put a stream boundary
inside a wave.  The reproducible switch runs the DET form of both kernels, on every case."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
PARENT_BIT = 1 << 27


def _b(a):
    """bytes of a float array, every NaN made the same NaN"""
    a = np.array(a, dtype=F, copy=True)
    a[np.isnan(a)] = np.nan
    return a.tobytes()


def _cornell(w, h):
    import clive2_amd as c2
    return c2.create_scene_from_preset("empty", w, h)


def _open_scene(w, h):
    import clive2_amd as c2
    from clive2_amd.load import triangles_for_box
    from clive2_amd.meshes import icosphere
    keep = [t for t in triangles_for_box() if t.emitter or t.n[1] > 0.5 or t.n[2] > 0.5]          # emitter, floor, back wall
    scene = c2.create_scene(w, h, np.array([0, 1.5, 6.0]), np.array([0, 0, -1.0]), room=keep,
                            file_specs=[dict(mesh=icosphere(2, radius=1.5), material=5, offset=np.array([0.5, 0.0, -1.0]))])
    assert len(scene.triangles) == 328
    return scene


# name: (scene maker, width, height, sample streams); every case runs with float atomics and with the reproducible switch
CASES = {
    "cornell-64x48": (_cornell, 64, 48, 1),
    "cornell-67x33": (_cornell, 67, 33, 1),
    "cornell-257x1": (_cornell, 257, 1, 1),
    "open-64x48": (_open_scene, 64, 48, 1),
    "cornell-67x33-two-streams": (_cornell, 67, 33, 2),
}
SWITCH = {"atomics": False, "reproducible": True}


def _one_sample(scene, K, det, flags):
    """One sample through the stage calls; per stream the outputs of the resolve stage."""
    from clive2_amd._native import ptr
    from clive2_amd.renderer import Renderer, stream_seeds
    r = Renderer(scene, streams=K)
    r.set_seeds(stream_seeds(r.batch_size, K))
    r.set_reproducible(det)
    if flags:
        r.set_debug_flags(flags)
    r.make_light_rays(); r.make_camera_rays(); r.trace_light_rays(); r.trace_camera_rays()
    r.join_paths()
    r.finalize_samples(); r.gather_light_image()
    # the strategy-pair masks of all K x W x H entries (Renderer.export_connections sizes its arrays for one stream)
    n = r.batch_size * K
    cmask = np.zeros(n, np.uint64)
    r._check(r._L.cl2_export_connections(r._h, ptr(cmask), None, None, C.c_size_t(n)), "export_connections")
    out = []
    for k in range(K):
        r.set_export_stream(k)
        d = dict(agg=r.export_aggregators(), cmask=cmask.reshape(K, -1)[k])
        d.update(r.export_sample_images())
        out.append(d)
    r.process_images()
    r.close()
    return out


@pytest.fixture(scope="module")
def runs():
    """(case, switch) -> (slim form, parent form, scene): rendered on first use, shared by the tests below and never written."""
    cache, scenes = {}, {}

    def get(name, switch):
        if (name, switch) not in cache:
            make, w, h, K = CASES[name]
            if name not in scenes:
                scenes[name] = make(w, h)
            scene, det = scenes[name], SWITCH[switch]
            cache[name, switch] = (_one_sample(scene, K, det, 0), _one_sample(scene, K, det, PARENT_BIT), scene)
        return cache[name, switch]
    return get


@pytest.mark.parametrize("switch", list(SWITCH))
@pytest.mark.parametrize("case", list(CASES))
def test_slim_kernel_writes_the_parent_kernels_bytes(case, switch, runs):
    slim, parent, _ = runs(case, switch)
    if case == "open-64x48":                                            # pixels with and without a contribution
        has = slim[0]["agg"]["contrib_weight_sum"] > 0
        assert has.any() and not has.all()
    for k, (a, b) in enumerate(zip(slim, parent)):
        assert a["cmask"].tobytes() == b["cmask"].tobytes(), f"stream {k}: cmask"
        assert a["cmask"].any()
        for f in ("weights", "total_contribution", "contrib_weight_sum"):
            assert _b(a["agg"][f]) == _b(b["agg"][f]), f"stream {k}: aggregator {f}"
        assert _b(a["unidirectional"]) == _b(b["unidirectional"]), f"stream {k}: unidirectional image"
        assert _b(a["finalized"]) == _b(b["finalized"]), f"stream {k}: finalized sample"
        assert case == "cornell-257x1" or (a["light"][:, :3] > 0).any()          # (no t = 1 ray meets a film one pixel high)
        differing = int((np.frombuffer(_b(a["light"]), np.uint32) != np.frombuffer(_b(b["light"]), np.uint32)).sum())
        print(f"{case} {switch} stream {k}: light-image words that differ: {differing} of {a['light'].size}")
        if SWITCH[switch]:
            assert _b(a["light"]) == _b(b["light"]), f"stream {k}: light image"
        else:
            np.testing.assert_allclose(a["light"], b["light"], rtol=2e-5, atol=1e-9)


@pytest.fixture(scope="module")
def oracles():
    """(case, stream) -> the oracle after one sample's stage calls: computed once, read only"""
    return {}


@pytest.mark.parametrize("switch", list(SWITCH))
@pytest.mark.parametrize("case", list(CASES))
def test_slim_kernel_against_the_oracle(case, switch, runs, oracle_mod, oracles):
    slim, _, scene = runs(case, switch)
    B = scene.pixel_width * scene.pixel_height
    for k, got in enumerate(slim):
        if (case, k) not in oracles:
            o = oracle_mod.OracleRenderer(scene, seeds=oracle_mod.make_seeds(B, rank=k))
            o.make_light_rays(); o.make_camera_rays(); o.trace_light_rays(); o.trace_camera_rays()
            o.join_paths(); o.finalize_samples(); o.gather_light_image()
            oracles[case, k] = o
        o = oracles[case, k]
        for f in ("weights", "total_contribution", "contrib_weight_sum"):
            assert got["agg"][f].tobytes() == o.weight_aggregators[f].tobytes(), f"stream {k}: aggregator {f}"
        assert got["finalized"][:, :3].tobytes() == o.finalized_samples[:, :3].tobytes(), f"stream {k}: finalized sample"
        assert got["unidirectional"].tobytes() == o.out_camera_image.tobytes(), f"stream {k}: unidirectional image"
        # the light image is a sum in a different order (atomics or records by slot vs the reference's sorted segments)
        np.testing.assert_allclose(got["light"][:, :3], o.out_light_image[:, :3], rtol=2e-5, atol=1e-9)
        assert case == "cornell-257x1" or (o.out_light_image[:, :3] > 0).any()
