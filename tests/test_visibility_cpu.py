"""The seeded visibility query (cl2_set_connection_query(1), cl2_probe_visibility; csrc/bvh_wide.hpp VIS) without a GPU: its numpy
restatement (tests/visibility_reference.py) on hand-made cases, the new symbols of the library, and the input check of the ray sets
that tests/test_gpu_visibility.py sends through the probe."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import visibility_reference as ref

f32 = np.float32


def _scene(leaves):
    """A tree by hand, one triangle per leaf: leaves = [(box lo, box hi, (v0, v1, v2))]; a right-leaning chain of inner boxes whose
    bounds are the union of what lies below them.  Returns a stand-in for a scene (boxes, triangles)."""
    from clive2_amd import struct_types as st
    n = len(leaves)
    tris = np.zeros(n, dtype=st.Triangle)
    for k, (_, _, (a, b, c)) in enumerate(leaves):
        tris["v0"][k, :3], tris["v1"][k, :3], tris["v2"][k, :3] = a, b, c
    boxes = np.zeros(2 * n - 1, dtype=st.Box)
    # box 2k = inner (children 2k+1 = leaf k, 2k+2 = the rest) for k < n-1; the last leaf is box 2n-2
    for k in range(n):
        leaf = 2 * k + 1 if k < n - 1 else 2 * n - 2
        boxes["min"][leaf, :3], boxes["max"][leaf, :3] = leaves[k][0], leaves[k][1]
        boxes["left"][leaf], boxes["right"][leaf] = k, k + 1
    for k in range(n - 2, -1, -1):
        boxes["left"][2 * k], boxes["right"][2 * k] = 2 * k + 1, 0
        boxes["min"][2 * k, :3] = np.minimum(boxes["min"][2 * k + 1, :3], boxes["min"][2 * k + 2, :3])
        boxes["max"][2 * k, :3] = np.maximum(boxes["max"][2 * k + 1, :3], boxes["max"][2 * k + 2, :3])
    return SimpleNamespace(boxes=boxes, triangles=tris)


def _quad_tri(z, shift=0.0):
    """a big triangle in the plane z = const that the test ray crosses, and its tight box"""
    a, b, c = (-4.0 + shift, -4.0, z), (6.0 + shift, -4.0, z), (-4.0 + shift, 6.0, z)
    return (-4.0 + shift, -4.0, z), (6.0 + shift, 6.0, z), (a, b, c)


O = np.array([[0.0, 0.0, 0.0]], f32)
D = (np.array([[0.1, 0.07, 1.0]], f32) / np.sqrt(f32(0.1) ** 2 + f32(0.07) ** 2 + f32(1.0))).astype(f32)   # no zero component: finite 1/d


def _verdict(scene, target):
    return bool(ref.visible(scene, O, D, np.array([target]))[0])


def test_a_blocker_in_front_of_the_target_hides_it():
    s = _scene([_quad_tri(2.0), _quad_tri(1.0)])            # T = 0 at z = 2, X = 1 at z = 1
    assert not _verdict(s, 0)
    assert _verdict(s, 1)                                    # and from X's side: the triangle behind it is no blocker


def test_a_blocker_behind_the_target_does_not():
    s = _scene([_quad_tri(1.0), _quad_tri(2.0), _quad_tri(3.0)])
    assert _verdict(s, 0)
    assert not _verdict(s, 1) and not _verdict(s, 2)


def test_a_missed_target_is_not_visible():
    s = _scene([_quad_tri(1.0, shift=20.0), _quad_tri(2.0)])   # T = 0 lies beside the ray; nothing else is in front of anything
    ok, _ = ref.tri_hit(O, D, *[np.asarray(x, f32)[None] for x in (s.triangles["v0"][0, :3], s.triangles["v1"][0, :3] - s.triangles["v0"][0, :3],
                                                                    s.triangles["v2"][0, :3] - s.triangles["v0"][0, :3])])
    assert not ok[0]
    assert not _verdict(s, 0)
    assert _verdict(s, 1)


def test_an_exact_tie_goes_to_the_triangle_the_reference_meets_first():
    """Two copies of one triangle: the same t to the bit.  The reference pops the child at left + 1 first, so the copy in the second
    leaf (triangle 1) is met first and wins (`t < best_t`, trace.metal:170): it blocks triangle 0, and triangle 0 does not block it."""
    s = _scene([_quad_tri(1.5), _quad_tri(1.5)])
    rank = ref.visit_rank(s.boxes, 2)
    assert rank[1] < rank[0]
    t0 = ref.tri_hit(O, D, *[np.asarray(s.triangles[k][0, :3], f32)[None] - (0 if k == "v0" else np.asarray(s.triangles["v0"][0, :3], f32)[None]) for k in ("v0", "v1", "v2")])[1]
    t1 = ref.tri_hit(O, D, *[np.asarray(s.triangles[k][1, :3], f32)[None] - (0 if k == "v0" else np.asarray(s.triangles["v0"][1, :3], f32)[None]) for k in ("v0", "v1", "v2")])[1]
    assert t0.tobytes() == t1.tobytes()
    assert not _verdict(s, 0)
    assert _verdict(s, 1)
    # the other way round: with the copies swapped between the leaves the verdicts swap with them
    s.boxes["left"][[1, 2]], s.boxes["right"][[1, 2]] = [1, 0], [2, 1]
    rank = ref.visit_rank(s.boxes, 2)
    assert rank[0] < rank[1]
    assert _verdict(s, 0)
    assert not _verdict(s, 1)


def test_a_leaf_whose_box_lies_behind_the_target_is_not_entered():
    """The definition goes by the leaf's OWN box: a triangle in front of the target whose leaf box starts behind t_T (a box that does
    not bound its triangle -- by rounding in a real tree, by hand here) is no blocker.  With its true box it is one."""
    lo, hi, tri = _quad_tri(1.0)
    far = _scene([_quad_tri(2.0), ((lo[0], lo[1], 5.0), (hi[0], hi[1], 6.0), tri)])
    assert _verdict(far, 0)
    true = _scene([_quad_tri(2.0), (lo, hi, tri)])
    assert not _verdict(true, 0)


def test_the_restatement_refuses_rays_it_does_not_cover():
    s = _scene([_quad_tri(1.0), _quad_tri(2.0)])
    with pytest.raises(AssertionError):
        ref.visible(s, O, np.array([[0.0, 0.0, 1.0]], f32), np.array([0]))


def test_the_library_exports_the_connection_query():
    """cl2_set/get_connection_query, cl2_connection_query_active and cl2_probe_visibility: in the built library, in the header and in
    the binding's list (build() refuses a library that lacks an entry of that list)."""
    import os
    from clive2_amd import _native
    _native.build()
    L = C.CDLL(_native.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "clive2_amd.h")).read()
    for name in ("cl2_set_connection_query", "cl2_get_connection_query", "cl2_connection_query_active", "cl2_probe_visibility"):
        assert hasattr(L, name), name
        assert name in _native.EXPORTS, name
        assert name + "(" in header, name
    assert L.cl2_abi_version() == 6                          # additions only
    # NULL handles are refused, not dereferenced (CL2_E_INVALID = -1)
    L.cl2_get_connection_query.argtypes = L.cl2_connection_query_active.argtypes = [C.c_void_p]
    L.cl2_set_connection_query.argtypes = [C.c_void_p, C.c_int]
    assert L.cl2_get_connection_query(None) == -1 and L.cl2_connection_query_active(None) == -1
    assert L.cl2_set_connection_query(None, 1) == -1
    for method in ("set_connection_query", "connection_query", "connection_query_active", "probe_visibility"):
        from clive2_amd.renderer import Renderer
        assert callable(getattr(Renderer, method))


def test_the_probe_ray_sets_ask_what_the_reference_answers(oracle_mod):
    """Input check of the ray sets of tests/test_gpu_visibility.py (subdivision-3 glass scene, 64 x 36, the t >= 2 connection rays of
    two samples; rays aimed at the mesh's vertices and edge midpoints): the restated verdict against `closest_hit == T` of the C
    oracle.  The two differ only where a hit lies in front of its own leaf box's entry distance (csrc/bvh_wide.hpp), which must be
    rare on pipeline rays -- at most 1 ray in 10,000 -- or the probe test would be checking something else than visibility.

    Disagreements on this seed (SEED of visibility_reference.py), rays in brackets:
        a  true targets      0 [128,162]
        b  closest hit       0 [126,441]
        c  random other      0 [128,162]
        d  aimed, closest    21 [10,184]     (exempt: a vertex lies ON the faces of its leaf's box)
        d  aimed, neighbour  27 [10,184]     (exempt)
    Every set must also hold both verdicts in numbers, or it tests one branch only."""
    scene, sets, exact = ref.probe_sets()
    verdicts = ref.probe_verdicts()
    assert len(scene.triangles) > 1280 and scene.pixel_width == 64 and scene.pixel_height == 36
    report = {}
    for name, (o, d, t) in sets.items():
        v = verdicts[name]
        want = exact[name] == t
        report[name] = (int((v != want).sum()), len(t), int(v.sum()))
    print(report)
    for name in ("a_true_targets", "b_closest_hit", "c_random_other"):
        bad, n, _ = report[name]
        assert n > 50_000, report
        assert bad * 10_000 <= n, report
    assert report["d_aimed_closest_hit"][1] > 8_000 and report["d_aimed_neighbour"][1] > 8_000, report
    # what each set is for
    n_a, vis_a = report["a_true_targets"][1], report["a_true_targets"][2]
    assert 0.2 * n_a < vis_a < 0.98 * n_a, report                                   # a: both verdicts
    assert report["b_closest_hit"][2] >= 0.9999 * report["b_closest_hit"][1], report   # b: all visible, the full walk
    assert report["c_random_other"][2] < 0.05 * report["c_random_other"][1], report    # c: most miss or are blocked
    o, d, t = sets["c_random_other"]
    assert (t != sets["a_true_targets"][2]).all()
    o, d, t = sets["d_aimed_neighbour"]
    assert (exact["d_aimed_neighbour"] != t).sum() > 0.5 * len(t)                   # d: the neighbour is another triangle than the hit
    # ... and it is hit at exactly the closest hit's t on many rays: ties that the target loses here and wins in the set above
    tris = scene.triangles
    v0 = tris["v0"][:, :3].astype(f32)
    ok_T, t_T = ref.tri_hit(o, d, v0[t], tris["v1"][t, :3].astype(f32) - v0[t], tris["v2"][t, :3].astype(f32) - v0[t])
    _, t_hit = ref.exact_closest_hit(scene, o, d)
    ties = ok_T & (exact["d_aimed_neighbour"] != t) & (t_T.view(np.uint32) == t_hit.view(np.uint32))
    print("ties", int(ties.sum()))
    assert ties.sum() > 100, int(ties.sum())          # (209 on this scene: enough for the rule to go wrong on)
