"""The fused connection launch of LDS-resident trees (k_connect_walk_lds, csrc/kernels.hpp) against the two launches it
replaces (k_connect_setup + k_traverse_conn over the global tag queue; debug bit 25 selects them): the same cull mask, the
same closest hits of every live strategy pair, the same ray tallies; and the scenes it is not for keep the two launches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OLD_PATH = 1 << 25


def _connection_stage(scene, flags=0, counting=False):
    from clive2_amd.renderer import Renderer, make_seeds
    r = Renderer(scene, seeds=make_seeds(scene.pixel_width * scene.pixel_height))
    r.set_debug_flags(flags)
    r.set_profiling(2)
    if counting:
        r.set_counting(True)
    r.make_light_rays(); r.make_camera_rays(); r.trace_light_rays(); r.trace_camera_rays()
    r.join_paths()
    cmask, tri, t1 = r.export_connections()
    out = dict(cmask=cmask, tri=tri, t1=t1, counters=r.counters(), agg=r.export_aggregators())
    r.close()
    return out


def _assert_same_connections(a, b):
    assert a["cmask"].tobytes() == b["cmask"].tobytes()
    for slot in range(36):
        live = ((a["cmask"] >> np.uint64(slot)) & np.uint64(1)).astype(bool)
        assert a["tri"][slot][live].tobytes() == b["tri"][slot][live].tobytes(), slot
        if slot < 6:
            assert a["t1"][slot][live].tobytes() == b["t1"][slot][live].tobytes(), slot
    for k in ("rays", "conn_rays"):
        assert a["counters"][k] == b["counters"][k], k
    assert a["agg"].tobytes() == b["agg"].tobytes()


def _open_glass_scene(w, h):
    """Emitter, floor and back wall of the box with a subdivision-3 rough-glass ball: more than 512 triangles, so the tree
    is not LDS-resident (the scene of tests/test_gpu_parity.py::test_ragged_frames_with_short_subpaths)."""
    import clive2_amd as c2
    from clive2_amd.load import get_materials, triangles_for_box
    from clive2_amd.meshes import icosphere
    mats = get_materials()
    mats["alpha"][5] = 0.1
    keep = [t for t in triangles_for_box() if t.emitter or t.n[1] > 0.5 or t.n[2] > 0.5]
    return c2.create_scene(w, h, np.array([0, 1.5, 6]), np.array([0, 0, -1]), room=keep, materials=mats,
                           file_specs=[dict(mesh=icosphere(3, radius=1.5), material=5, offset=np.array([0.5, 0.0, -1.0]))])


@pytest.mark.parametrize("size", [(64, 48), (41, 25), (91, 60), (640, 360)])
def test_fused_connection_launch_matches_the_two_launches(size):
    """Cornell box, full and ragged frames (4 x 256 + 1 pixels; 21 x 256 + 84): cmask and the hit of every live pair are
    the same bytes, rays / conn_rays the same, and the fused launch is the one that ran (no set-up time)."""
    import clive2_amd as c2
    scene = c2.create_scene_from_preset("empty", *size)
    fused, old = _connection_stage(scene), _connection_stage(scene, OLD_PATH)
    assert fused["counters"]["ms_connect_setup"] == 0.0
    assert old["counters"]["ms_connect_setup"] > 0.0
    assert fused["counters"]["conn_rays"] > 0
    _assert_same_connections(fused, old)


def test_fused_connection_launch_through_the_sample_pipeline():
    """Several samples through run_samples (both {chit, cmask} sets, the connection stream): the same RNG state, sample
    counts and unidirectional image as the two-launch path, the light image within the splat's float-atomic tolerance."""
    import clive2_amd as c2
    from clive2_amd.renderer import Renderer, make_seeds
    scene = c2.create_scene_from_preset("empty", 91, 60)
    seeds = make_seeds(91 * 60)
    a, b = Renderer(scene, seeds=seeds), Renderer(scene, seeds=seeds)
    b.set_debug_flags(OLD_PATH)
    a.run_samples(4); b.run_samples(4)
    assert np.array_equal(a.get_random_buffer(), b.get_random_buffer())
    ua, ub = a.read_accumulators(), b.read_accumulators()
    assert np.array_equal(ua[2], ub[2]) and ua[3].tobytes() == ub[3].tobytes()
    assert np.allclose(ua[0], ub[0], rtol=2e-5, atol=1e-7)
    assert a.counters()["rays"] == b.counters()["rays"]
    a.close(); b.close()


def test_counting_mode_keeps_the_two_launches():
    """Counting mode tallies the reference's walk over the full table: the set-up launch runs, and cmask, hits and ray
    counts are those of the fused launch."""
    import clive2_amd as c2
    scene = c2.create_scene_from_preset("empty", 64, 48)
    counted, fused = _connection_stage(scene, counting=True), _connection_stage(scene)
    assert counted["counters"]["ms_connect_setup"] > 0.0
    assert fused["counters"]["ms_connect_setup"] == 0.0
    _assert_same_connections(counted, fused)


def test_non_flat_pruned_table_keeps_the_two_launches():
    """At 257 x 1 the camera's film quad keeps an inner record in the Cornell box's pruned table (4 records, not a flat list
    of 3 leaves: tests/test_scene_prep_cpu.py's driver shows it), so the set-up launch runs -- over one full workgroup and
    one of a single pixel -- with the same results as the forced two-launch path."""
    import clive2_amd as c2
    scene = c2.create_scene_from_preset("empty", 257, 1)
    a, b = _connection_stage(scene), _connection_stage(scene, OLD_PATH)
    assert a["counters"]["ms_connect_setup"] > 0.0 and b["counters"]["ms_connect_setup"] > 0.0
    _assert_same_connections(a, b)


def test_mesh_scene_keeps_the_two_launches():
    """A tree that is not LDS-resident takes the set-up launch and the persistent walk whatever debug bit 25 says."""
    scene = _open_glass_scene(91, 60)
    assert len(scene.triangles) > 512
    a, b = _connection_stage(scene), _connection_stage(scene, OLD_PATH)
    assert a["counters"]["ms_connect_setup"] > 0.0 and b["counters"]["ms_connect_setup"] > 0.0
    _assert_same_connections(a, b)
