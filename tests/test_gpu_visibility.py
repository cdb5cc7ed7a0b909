"""The opt-in seeded visibility walk of the t >= 2 connection rays (cl2_set_connection_query(1), cl2_probe_visibility;
csrc/bvh_wide.hpp VIS) on the GPU: the probe against the numpy restatement of the query for every ray (tests/visibility_reference.py;
tests/test_visibility_cpu.py checks the ray sets), the switch, the pipeline in both modes, and the work the mode removes.  The
default -- closest-hit queries, the reference's -- is what every other test of the suite runs."""
import numpy as np
import pytest

import visibility_reference as ref

pytestmark = pytest.mark.gpu
LIGHT, CAMERA = 0, 1
f32 = np.float32


def _rays(o, d):
    from clive2_amd import struct_types as st
    rays = np.zeros(len(o), dtype=st.Ray)
    rays["origin"][:, :3] = o
    rays["direction"][:, :3] = d
    return rays


@pytest.fixture(scope="module")
def probe(oracle_mod):
    from clive2_amd.renderer import Renderer
    scene, sets, exact = ref.probe_sets()
    r = Renderer(scene)
    r.set_traversal_mode(5)
    yield r, scene, sets, exact
    r.close()


@pytest.mark.parametrize("name", ["a_true_targets", "b_closest_hit", "c_random_other", "d_aimed_closest_hit", "d_aimed_neighbour"])
def test_probe_equals_the_restatement_for_every_ray(probe, name):
    """Glass icosphere, subdivision 3, 64 x 36, traversal mode 5.  The verdict `out_tri == T` of every ray equals the restatement's: no
    tolerance.  (a) the t >= 2 connection rays of two samples with their true targets; (b) T = the exact closest hit: all visible, the
    full walk; (c) T = a random other triangle: most miss T; (d) rays aimed at the mesh's vertices and edge midpoints, T = the exact
    closest hit and T = a neighbouring triangle that shares the point: exact-t ties settled both ways.  Beyond the verdict: a visible
    ray reports t_T to the bit, a ray that misses T reports (-1, inf), a blocked ray a blocker -- another triangle, hit no farther than
    T -- and a second run returns the same bytes."""
    r, scene, sets, _ = probe
    o, d, T = sets[name]
    want = ref.probe_verdicts()[name]
    rays = _rays(o, d)
    tri, t = r.probe_visibility(rays, T)
    got = tri == T
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (name, len(bad), len(T), bad[:8], tri[bad[:8]], T[bad[:8]])
    tris = scene.triangles
    v0 = tris["v0"][:, :3].astype(f32)
    ok_T, t_T = ref.tri_hit(o, d, v0[T], tris["v1"][T, :3].astype(f32) - v0[T], tris["v2"][T, :3].astype(f32) - v0[T])
    assert np.array_equal(tri == -1, ~ok_T)
    assert np.isinf(t[~ok_T]).all()
    assert t[got].tobytes() == t_T[got].tobytes()
    blocked = ok_T & ~got
    assert (tri[blocked] >= 0).all() and (t[blocked] <= t_T[blocked]).all()
    tri2, t2 = r.probe_visibility(rays, T)
    assert tri2.tobytes() == tri.tobytes() and t2.tobytes() == t.tobytes()


def test_unseeded_probe_rays_are_closest_hit_queries(probe):
    """(e) target = -1 returns what cl2_probe_traverse returns, and so does every ray with a zero direction component, whatever its
    target: such rays take the binary walk, unseeded.  Targets beyond the scene's triangles are refused."""
    from clive2_amd.renderer import RendererError
    r, scene, sets, _ = probe
    o, d, T = (x[:4096] for x in sets["a_true_targets"])
    rays = _rays(o, d)
    bi, bt, _, _ = r.probe_traverse(rays)
    tri, t = r.probe_visibility(rays, np.full(len(rays), -1, np.int32))
    assert tri.tobytes() == bi.tobytes() and t.tobytes() == bt.tobytes()
    # axis-parallel and plane-parallel rays through the sphere and the room, from two points
    dirs = np.array([[0, 0, -1], [0, -1, 0], [1, 0, 0], [0, 0.6, -0.8], [0.6, 0, -0.8], [-0.8, 0.6, 0], [0, -0.6, -0.8]], f32)
    oz = np.concatenate([np.tile(np.array([[0.1, 1.2, 5.5]], f32), (len(dirs), 1)), np.tile(np.array([[-0.3, 4.0, 2.0]], f32), (len(dirs), 1))])
    dz = np.concatenate([dirs, dirs])
    zrays = _rays(oz, dz)
    zi, zt, _, _ = r.probe_traverse(zrays)
    assert (zi >= 0).sum() >= 8
    held = np.where(zi >= 0, zi, 0)
    for target in (np.full(len(zrays), -1, np.int32), held.astype(np.int32), ((held + 1) % len(scene.triangles)).astype(np.int32)):
        tri, t = r.probe_visibility(zrays, target)
        assert tri.tobytes() == zi.tobytes() and t.tobytes() == zt.tobytes()
    with pytest.raises(RendererError):
        r.probe_visibility(rays[:4], np.array([0, 1, len(scene.triangles), 2], np.int32))
    with pytest.raises(RendererError):
        r.set_debug_flags(1 << 13); r.probe_visibility(rays[:4], T[:4])
    r.set_debug_flags(0)
    # the 48-byte triangle records (debug bit 14) give the same bytes as the packed ones
    want = r.probe_visibility(rays, T)
    r.set_debug_flags(1 << 14)
    got = r.probe_visibility(rays, T)
    r.set_debug_flags(0)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_connection_query_is_opt_in(cornell_small):
    """Default 0; other values than 0 and 1 are refused and leave the setting alone; mode 1 and the nearest-first order, or debug
    bit 13 or 14, refuse each other whichever comes second.  The Cornell box is resident in LDS: its connection launch is not the
    4-wide walk, the query is not active, and Path[] and the aggregators have the same bytes in either mode."""
    from clive2_amd.renderer import Renderer, RendererError, make_seeds
    seeds = make_seeds(cornell_small.pixel_width * cornell_small.pixel_height)
    a, b = Renderer(cornell_small, seeds=seeds), Renderer(cornell_small, seeds=seeds)
    assert a.connection_query() == 0 and a.connection_query_active() == 0
    b.set_connection_query(1)
    assert b.connection_query() == 1
    for bad in (2, -1, 7):
        with pytest.raises(RendererError):
            b.set_connection_query(bad)
        assert b.connection_query() == 1
    # refused both ways round
    with pytest.raises(RendererError):
        b.set_traversal_order(1)
    assert b.traversal_order() == 0
    for bit in (13, 14):
        with pytest.raises(RendererError):
            b.set_debug_flags(1 << bit)
    b.set_debug_flags(1 << 12)                               # other bits are not concerned
    b.set_debug_flags(0)
    a.set_traversal_order(1)
    with pytest.raises(RendererError):
        a.set_connection_query(1)
    assert a.connection_query() == 0
    a.set_traversal_order(0)
    for bit in (13, 14):
        a.set_debug_flags(1 << bit)
        with pytest.raises(RendererError):
            a.set_connection_query(1)
        assert a.connection_query() == 0
    a.set_debug_flags(0)
    assert b.connection_query_active() == 0                  # LDS-resident tree
    a.run_samples(3); b.run_samples(3)
    for which in (LIGHT, CAMERA):
        assert a.export_paths(which).tobytes() == b.export_paths(which).tobytes()
    agg_a, agg_b = a.export_aggregators(), b.export_aggregators()
    for f in ("weights", "total_contribution", "contrib_weight_sum"):
        assert agg_a[f].tobytes() == agg_b[f].tobytes(), f
    a.close(); b.close()


def _staged_sample(r):
    r.make_light_rays(); r.make_camera_rays(); r.trace_light_rays(); r.trace_camera_rays(); r.join_paths()
    out = (r.export_connections(), r.export_paths(CAMERA)["rays"]["triangle"][:, :6].astype(np.int32), r.export_aggregators()["total_contribution"].copy())
    r.finalize_samples(); r.gather_light_image(); r.process_images()
    return out


def test_pipeline_in_both_modes():
    """Same scene as the probe, traversal mode 5, two stage-by-stage samples on the same seeds with mode 0 and with mode 1: the t = 1
    slots of the connection results (triangle and distance) have the same bytes; for every masked t >= 2 slot `tri == the camera
    vertex's triangle` agrees (tests/test_visibility_cpu.py: no ray of these samples is one of the hits in front of its own leaf box on
    which the two queries may differ); so the aggregators' total_contribution has the same bytes.  While mode 1 is counting with the
    reference walk's tallies (set_counting(1): the binary walk) it is not active."""
    from clive2_amd.renderer import Renderer, make_seeds
    scene = ref.glass(3, 64, 36)
    B = 64 * 36
    seeds = make_seeds(B)
    r0, r1 = Renderer(scene, seeds=seeds), Renderer(scene, seeds=seeds)
    for r in (r0, r1):
        r.set_traversal_mode(5)
    r1.set_connection_query(1)
    assert r0.connection_query_active() == 0 and r1.connection_query_active() == 1
    r1.set_counting(1)
    assert r1.connection_query_active() == 0
    r1.set_counting(0)
    assert r1.connection_query_active() == 1
    differing_slots = 0
    for _ in range(2):
        (m0, tri0, t10), ctri0, agg0 = _staged_sample(r0)
        (m1, tri1, t11), ctri1, agg1 = _staged_sample(r1)
        assert m0.tobytes() == m1.tobytes() and ctri0.tobytes() == ctri1.tobytes()
        for slot in range(6):                                # (an unmasked slot holds whatever the buffer held)
            masked = ((m0 >> np.uint64(slot)) & np.uint64(1)).astype(bool)
            assert masked.any()
            assert tri0[slot][masked].tobytes() == tri1[slot][masked].tobytes() and t10[slot][masked].tobytes() == t11[slot][masked].tobytes()
        n_masked = 0
        for t in range(2, 7):
            for s in range(1, 7):
                slot = (t - 1) * 6 + (s - 1)
                masked = ((m0 >> np.uint64(slot)) & np.uint64(1)).astype(bool)
                n_masked += int(masked.sum())
                T = ctri0[:, t - 1]
                assert np.array_equal((tri0[slot] == T)[masked], (tri1[slot] == T)[masked]), (t, s)
                differing_slots += int((tri0[slot] != tri1[slot])[masked].sum())
        assert n_masked > 10 * B
        assert agg0.tobytes() == agg1.tobytes()
    assert differing_slots > 0                                # mode 1 did stop at blockers that are not the closest hit
    r0.close(); r1.close()


@pytest.mark.parametrize("streams,pipelining", [(1, 0), (1, 2), (2, 0), (2, 2)])
def test_reproducible_renders_are_identical_in_both_modes(streams, pipelining):
    """run_samples with the reproducible light image: all four accumulators have the same bytes in mode 0 and in mode 1, with one and
    with two sample streams, in the serial order and with three pipeline stages."""
    from clive2_amd.renderer import Renderer, stream_seeds
    scene = ref.glass(3, 64, 36)
    acc = []
    for mode in (0, 1):
        r = Renderer(scene, seeds=stream_seeds(64 * 36, streams), streams=streams)
        r.set_traversal_mode(5); r.set_reproducible(True); r.set_pipelining(pipelining)
        r.set_connection_query(mode)
        assert r.connection_query_active() == mode
        r.run_samples(3)
        acc.append([x.copy() for x in r.read_accumulators()])
        r.close()
    for x, y in zip(*acc):
        assert x.tobytes() == y.tobytes()
    assert np.isfinite(acc[0][0]).all() and acc[0][0].max() > 0


def test_the_seeded_walk_visits_less():
    """Config-3 geometry (subdivision 4) at 320 x 180, one sample, the walk's own tallies (set_counting(2)): a connection ray visits
    strictly fewer wide nodes and reads strictly fewer triangle records in mode 1 (the target's record included); the subpath launches
    are the same launches."""
    from clive2_amd.renderer import Renderer, make_seeds
    scene = ref.glass(4, 320, 180)
    seeds = make_seeds(320 * 180)
    tallies = []
    for mode in (0, 1):
        r = Renderer(scene, seeds=seeds)
        r.set_traversal_mode(5); r.set_connection_query(mode); r.set_counting(2)
        assert r.connection_query_active() == mode
        r.run_samples(1)
        tallies.append(r.walk_tallies())
        r.close()
    t0, t1 = tallies
    assert t0["subpath"] == t1["subpath"] and t0["subpath"]["rays"] > 0
    n = t0["connection"]["rays"]
    assert n == t1["connection"]["rays"] > 0
    print({k: (t0["connection"][k] / n, t1["connection"][k] / n) for k in ("wide_visits", "tri_records")})
    assert t1["connection"]["wide_visits"] < t0["connection"]["wide_visits"]
    assert t1["connection"]["tri_records"] < t0["connection"]["tri_records"]
