"""The flat walk of LDS-resident trees (closest_hit_flat, csrc/bvh_traverse.hpp) with the record address in a vector register
and the unclamped fetch into the pad records behind the staged triangles, against the loop it replaces (debug bit 26:
closest_hit_flat_clamped) and against the oracle: the same cull mask, the same closest hit of every live strategy pair, the same
subpaths, ray tallies and accumulators; the pad records are counted where the staged tree is sized."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LIGHT, CAMERA = 0, 1
CLAMPED_LOOP = 1 << 26
TWO_LAUNCHES = 1 << 25
PADS = 2


def _stages(scene, flags, seeds):
    """Subpaths, connection stage and aggregators of one sample, stage by stage; and, in a second renderer, three samples
    through the pipeline with the reproducible light image (all four accumulators are then the same bytes for the same
    contributions)."""
    from clive2_amd.renderer import Renderer
    r = Renderer(scene, seeds=seeds)
    r.set_debug_flags(flags)
    r.set_profiling(2)
    org = r.organisation()
    r.make_light_rays(); r.make_camera_rays(); r.trace_light_rays(); r.trace_camera_rays()
    paths = [r.export_paths(LIGHT).tobytes(), r.export_paths(CAMERA).tobytes()]
    r.join_paths()
    cmask, tri, t1 = r.export_connections()
    out = dict(org=org, paths=paths, cmask=cmask, tri=tri, t1=t1, agg=r.export_aggregators(), counters=r.counters())
    r.close()
    r = Renderer(scene, seeds=seeds)
    r.set_debug_flags(flags)
    r.set_reproducible(True)
    r.run_samples(1); r.run_samples(2)
    out.update(acc=r.read_accumulators(), rand=r.get_random_buffer(), rays=r.counters()["rays"])
    r.close()
    return out


def _assert_same(a, b):
    assert a["paths"][LIGHT] == b["paths"][LIGHT] and a["paths"][CAMERA] == b["paths"][CAMERA]
    assert a["cmask"].tobytes() == b["cmask"].tobytes()
    for slot in range(36):
        live = ((a["cmask"] >> np.uint64(slot)) & np.uint64(1)).astype(bool)
        assert a["tri"][slot][live].tobytes() == b["tri"][slot][live].tobytes(), slot
        if slot < 6:
            assert a["t1"][slot][live].tobytes() == b["t1"][slot][live].tobytes(), slot
    for k in ("rays", "conn_rays"):
        assert a["counters"][k] == b["counters"][k], k
    assert a["rays"] == b["rays"]
    for k in a["agg"].dtype.names:
        assert a["agg"][k].tobytes() == b["agg"][k].tobytes(), k
    assert np.array_equal(a["rand"], b["rand"])
    for x, y in zip(a["acc"], b["acc"]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def _assert_oracle(scene, seeds, got, oracle_mod):
    o = oracle_mod.OracleRenderer(scene, seeds=seeds)
    o.make_light_rays(); o.make_camera_rays(); o.trace_light_rays(); o.trace_camera_rays()
    assert got["paths"][LIGHT] == o.out_light_paths.tobytes() and got["paths"][CAMERA] == o.out_camera_paths.tobytes()
    o.join_paths()
    for k in ("total_contribution", "weights", "contrib_weight_sum"):
        assert got["agg"][k].tobytes() == o.weight_aggregators[k].tobytes(), k
    o.finalize_samples(); o.gather_light_image(); o.process_images()
    for _ in range(2):
        o.run_sample()
    assert np.array_equal(got["rand"], o.rand_buffer)
    assert got["rays"] == o.rays_traced
    img, wts, cnt, uni = got["acc"]
    np.testing.assert_allclose(uni, o.unidirectional_image_buffer, rtol=1e-6, atol=0)
    # the oracle's first sample went through its stage calls, whose light image is not summed in slot order
    np.testing.assert_allclose(img, o.summed_image, rtol=5e-5, atol=1e-8)
    np.testing.assert_allclose(wts, o.summed_sample_weights, rtol=5e-5, atol=1e-8)


@pytest.mark.parametrize("size", [(64, 48), (67, 33)])
def test_flat_walk_matches_the_clamped_loop_and_the_oracle(size, oracle_mod):
    """Cornell box, a full frame and a ragged one (8 x 256 + 163 pixels: the last workgroup is partial).  The fused connection
    launch runs in both forms (no set-up time), so both launches that walk the flat table are compared."""
    import clive2_amd as c2
    from clive2_amd.renderer import make_seeds
    scene = c2.create_scene_from_preset("empty", *size)
    seeds = make_seeds(size[0] * size[1])
    new, old = _stages(scene, 0, seeds), _stages(scene, CLAMPED_LOOP, seeds)
    assert new["org"]["pruned_records"] == old["org"]["pruned_records"] == 3
    assert new["counters"]["ms_connect_setup"] == 0.0 and old["counters"]["ms_connect_setup"] == 0.0
    assert new["counters"]["conn_rays"] > 0
    _assert_same(new, old)
    _assert_oracle(scene, seeds, new, oracle_mod)


def test_non_flat_pruned_table_is_untouched(oracle_mod):
    """At 257 x 1 the Cornell box's pruned table keeps an inner record: the per-lane walk runs whatever bit 26 says (the set-up
    launch shows it), over staged triangles that now end in the pad records."""
    import clive2_amd as c2
    from clive2_amd.renderer import make_seeds
    scene = c2.create_scene_from_preset("empty", 257, 1)
    seeds = make_seeds(257)
    new, old = _stages(scene, 0, seeds), _stages(scene, CLAMPED_LOOP, seeds)
    assert new["org"]["pruned_records"] == 4
    assert new["counters"]["ms_connect_setup"] > 0.0 and old["counters"]["ms_connect_setup"] > 0.0
    _assert_same(new, old)
    _assert_oracle(scene, seeds, new, oracle_mod)


def _leaf_scene(w, h):
    """The Cornell box's 16 triangles under a hand-made tree: leaves of 1, 2, 3, 2 and 8 triangles below four inner boxes that
    all span the room, so that the pruned table drops every inner record (a test that cannot miss saves nothing) and is the flat
    list of the five leaves.  The 8-triangle leaf ends with the array's last triangle: the fetch behind it lands on a pad."""
    import clive2_amd as c2
    from clive2_amd import struct_types as st
    base = c2.create_scene_from_preset("empty", w, h)
    tris = base.triangles
    assert len(tris) == 16
    corners = np.stack([tris["v0"][:, :3], tris["v1"][:, :3], tris["v2"][:, :3]], axis=1)       # [tri, vertex, xyz]
    boxes = np.zeros(9, dtype=st.Box)
    room = corners.min(axis=(0, 1)), corners.max(axis=(0, 1))
    inner = {0: 1, 1: 3, 2: 5, 5: 7}                                       # box -> first child (children at left, left + 1)
    leaves = {3: (0, 1), 4: (1, 3), 6: (3, 6), 7: (6, 8), 8: (8, 16)}      # box -> triangles [left, right)
    for i, left in inner.items():
        boxes["min"][i, :3], boxes["max"][i, :3] = room
        boxes["left"][i], boxes["right"][i] = left, 0
    for i, (a, b) in leaves.items():
        boxes["min"][i, :3], boxes["max"][i, :3] = corners[a:b].min(axis=(0, 1)), corners[a:b].max(axis=(0, 1))
        boxes["left"][i], boxes["right"][i] = a, b
    scene = copy.copy(base)
    scene.boxes = boxes
    scene.validate()
    return scene, sorted(b - a for a, b in leaves.values())


def test_leaves_of_one_two_three_and_eight_triangles(oracle_mod):
    """Both exits of the two-at-a-time loop (odd and even leaves), a leaf that is a single trip and one of four trips, and the
    prefetch behind the array's last record."""
    from clive2_amd.renderer import make_seeds
    scene, sizes = _leaf_scene(67, 33)
    assert sizes == [1, 2, 2, 3, 8]
    seeds = make_seeds(67 * 33)
    new, old = _stages(scene, 0, seeds), _stages(scene, CLAMPED_LOOP, seeds)
    org = new["org"]
    # nine records of which the five leaves remain
    if (org["n_records"], org["pruned_records"]) != (9, 5):
        pytest.skip(f"upload did not make the table of five leaves out of this tree: {org}")
    # ... walked as a flat list: only then does the fused connection launch run, in both forms
    assert new["counters"]["ms_connect_setup"] == 0.0 and old["counters"]["ms_connect_setup"] == 0.0
    assert org["tree_in_lds"] == 1 and org["lds_triangles"] == 1
    assert org["staged_bytes"] == (2 * 9 + 3 * (16 + PADS) + 2 * 5) * 16
    _assert_same(new, old)
    _assert_oracle(scene, seeds, new, oracle_mod)
    # and the per-lane walk of the full table (no pruned table at all) sees the same scene
    full = _stages(scene, 1 << 7, seeds)
    assert full["org"]["pruned_records"] == 0
    _assert_same(new, full)


def test_scene_at_the_triangle_cap_keeps_its_residency(oracle_mod):
    """512 triangles, the most that are staged: the tree stays LDS-resident with the pad records behind its triangles, the
    pruned table is built or left out by the rule of cl2_upload_scene (three workgroups per CU with the subpath kernel's 9.7 KB
    of shading tables, pads counted), and subpaths and aggregators are the oracle's."""
    import clive2_amd as c2
    from clive2_amd.load import get_materials
    from clive2_amd.meshes import icosphere
    from clive2_amd.renderer import make_seeds
    mats = get_materials()
    mats["alpha"][5] = 0.1
    v0, f0 = icosphere(0, radius=0.7, center=(0.0, 3.2, -2.0))
    specs = [dict(mesh=icosphere(2, radius=1.6, center=(0.0, 0.5, 0.0)), material=5),
             dict(mesh=icosphere(1, radius=1.0, center=(-4.0, 0.0, -3.0)), material=3),
             dict(mesh=icosphere(1, radius=1.0, center=(4.0, 0.0, -3.0)), material=1),
             dict(mesh=(v0, f0[:16]), material=2)]
    scene = c2.create_scene(64, 48, np.array([0, 1.5, 6]), np.array([0, 0, -1]), file_specs=specs, materials=mats)
    assert len(scene.triangles) == 512
    seeds = make_seeds(64 * 48)
    new, old = _stages(scene, 0, seeds), _stages(scene, CLAMPED_LOOP, seeds)
    org = new["org"]
    assert org["tree_in_lds"] == 1 and org["lds_triangles"] == 1 and org["n_lds_records"] == org["n_records"]
    assert org["staged_bytes"] == (2 * org["n_records"] + 3 * (512 + PADS) + 2 * org["pruned_records"]) * 16
    with_table = (2 * org["n_records"] + 3 * (512 + PADS)) * 16 + 9728
    assert org["pruned_records"] == 0 or with_table + 2 * org["pruned_records"] * 16 <= 160 * 1024 // 3, org
    _assert_same(new, old)
    _assert_oracle(scene, seeds, new, oracle_mod)


def test_bit_26_is_a_known_debug_bit_and_changes_no_organisation():
    import clive2_amd as c2
    from clive2_amd.renderer import Renderer, make_seeds
    scene = c2.create_scene_from_preset("empty", 64, 48)
    r = Renderer(scene, seeds=make_seeds(64 * 48))
    before = r.organisation()
    r.set_debug_flags(CLAMPED_LOOP | TWO_LAUNCHES)
    assert r.organisation() == before
    assert before["staged_bytes"] == (2 * 5 + 3 * (16 + PADS) + 2 * 3) * 16
    r.close()
