"""GPU: the nearest-first child order of the 4-wide walk (cl2_set_traversal_order(1); csrc/bvh_wide.hpp ORDER) on the trees whose
stack it makes deep -- a left-leaning chain and the GPU builder's trees with one-triangle leaves (tests/wide_stack_cases.py).  The
kernel's pushes are not clamped: what keeps them inside the per-lane overflow array is the host's sizing from the tree's order_depth
(csrc/scene_prep.hpp: wide_overflow_entries; cl2_wide_stack_capacity), whose bound tests/test_wide_stack_cpu.py proves on the CPU
restatement of the walk.  These tests pin the behaviour that follows from it on the device: hits that equal the reference order's and
the oracle's, the spill count of the restatement, and the refusal of a tree that no array can serve."""
import importlib.util
import os

import numpy as np
import pytest

import wide_stack_cases as cases
import wide_walk_reference as model
from test_scene_prep_cpu import Input, lib                           # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = model.WIDE_STACK_LDS


def _order_tool():
    spec = importlib.util.spec_from_file_location("exp_order_ab", os.path.join(ROOT, "tools", "exp_order_ab.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rays(o, d):
    from clive2_amd import struct_types as st
    rays = np.zeros(len(o), dtype=st.Ray)
    rays["origin"][:, :3] = o; rays["direction"][:, :3] = d
    rays["inv_direction"][:, :3] = np.float32(1.0) / d
    return rays


def _same(got, want_i, want_t):
    return np.array_equal(got[0], want_i) and np.array_equal(got[1].view(np.uint32), want_t.view(np.uint32))


def test_rays_along_a_left_chain_spill_as_the_restatement_says(lib, oracle_mod):
    """A left chain of 40 inner boxes: max_pending 1, order_depth 40.  Every plate ray stacks 40 entries nearest first, 32 of them in
    the overflow array, which the pending depth alone sized at 6.  Both orders return the oracle's hits (no hit of these rays lies in
    front of its own leaf box: test_wide_stack_cpu.py), the device's spill tally EQUALS the restatement's with the speculative
    expansion on (what the nearest-first launch runs; the restatement follows a lane exactly) and is no less than the one with it
    off; back in the reference's order -- the overflow array is freed and allocated again at its old size -- the hits are the same."""
    from clive2_amd.renderer import Renderer
    scene = cases.plate_chain(cases.plate_scene(39))
    depth = model.order_depth(scene.boxes)
    assert depth == 40
    po, pd = cases.plate_rays(256)
    ro, rd = cases.random_rays(2000, 11)
    o, d = np.concatenate([po, ro]), np.concatenate([pd, rd])
    rays = _rays(o, d)
    want_i, want_t = oracle_mod.traverse(rays, scene.boxes, scene.triangles)[:2]
    err, out = Input(scene).prepare(lib)
    assert err is None and (out["max_pending"], out["order_depth"]) == (1, depth)
    b = scene.boxes
    walk = lambda spec: model.walk(np.frombuffer(out["wide"], np.float32), b["min"][0], b["max"][0], np.frombuffer(out["tris"], np.float32),
                                   np.frombuffer(out["tri_rank"], np.int32), o, d, 1, spec=spec)
    with_spec, without = walk(True), walk(False)
    assert (with_spec["peak"][:256] == depth).all() and _same((with_spec["tri"], with_spec["t"]), want_i, want_t)
    r = Renderer(scene)
    try:
        r.set_traversal_mode(5)
        assert r.wide_stack_capacity() == LDS + 6
        first = r.probe_traverse(rays)
        assert _same(first, want_i, want_t)
        r.set_traversal_order(1)
        assert r.traversal_order() == 1 and r.wide_stack_capacity() >= depth
        r.set_counting(2); r.reset_counters()
        assert _same(r.probe_traverse(rays), want_i, want_t)
        tally = r.walk_tallies()["subpath"]
        assert tally["rays"] == len(rays) and tally["binary_records"] == 0
        assert tally["stack_spills"] == int(with_spec["spills"].sum()) > 256 * (depth - LDS) - 1
        assert tally["stack_spills"] >= int(without["spills"].sum()) > 0
        r.set_counting(0)
        r.set_traversal_order(0)
        assert r.wide_stack_capacity() == LDS + 6
        again = r.probe_traverse(rays)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(first, again))
    finally:
        r.close()


@pytest.mark.parametrize("sub", [2, 3])
def test_gpu_built_trees_with_one_triangle_leaves(sub, oracle_mod):
    """The glass scene under the GPU builder's tree, one triangle per leaf: the smaller subtree goes to left + 1, so the pending
    depth stays near log2(n) while order_depth does not (27 against 8 + 18 entries of the old sizing at subdivision 2, 32 against 8 + 22
    at 3).  The stack has room for order_depth; the two orders agree except where a hit lies in front of its own leaf box, neither
    misses what the other hits, and the reference's order returns the oracle's hits."""
    from clive2_amd.renderer import Renderer
    tool = _order_tool()
    scene = cases.glass(sub, bvh_builder="gpu", max_members=1)
    leaves = scene.boxes[scene.boxes["right"] != 0]
    assert (leaves["right"] - leaves["left"]).max() == 1
    depth = model.order_depth(scene.boxes)
    o, d = cases.glass_rays(scene)
    rays = _rays(o, d)
    want_i, want_t = oracle_mod.traverse(rays, scene.boxes, scene.triangles)[:2]
    r = Renderer(scene)
    try:
        r.set_traversal_mode(5)
        assert _same(r.probe_traverse(rays), want_i, want_t)
        r.set_traversal_order(1)
        assert r.wide_stack_capacity() >= depth > 0
    finally:
        r.close()
    n_aimed = len(cases.aimed_rays(scene)[0])
    res = tool.compare_orders(scene, [("aimed", o[:n_aimed], d[:n_aimed]), ("random", o[n_aimed:], d[n_aimed:])])
    assert res["rays"] == len(o) and res["by_kind"]["aimed"]["rays"] == n_aimed > 2000
    assert res["missed_by_order0"] == 0 and res["missed_by_order1"] == 0, res
    assert res["in_front_of_own_leaf"] == res["differ"], res


def test_a_tree_too_deep_for_the_nearest_first_order_is_refused(oracle_mod):
    """A left chain of 200 inner boxes (order_depth 200 > 8 + 136): served in the reference's order, whose stack holds two entries
    there; cl2_set_traversal_order(1) is refused and leaves the setting alone; with order 1 set first the upload is refused and the
    renderer has no scene until one it can serve arrives.  Nothing is launched in order 1."""
    from clive2_amd.renderer import Renderer, RendererError
    small = cases.plate_scene(39)
    scene = cases.plate_chain(cases.plate_scene(199))
    assert model.order_depth(scene.boxes) == 200
    po, pd = cases.plate_rays(256)
    ro, rd = cases.random_rays(2000, 11)
    rays = _rays(np.concatenate([po, ro]), np.concatenate([pd, rd]))
    want_i, want_t = oracle_mod.traverse(rays, scene.boxes, scene.triangles)[:2]
    assert (want_i[:256] == 198).all()
    r = Renderer(scene)
    try:
        r.set_traversal_mode(5)
        assert r.wide_stack_capacity() == LDS + 6
        assert _same(r.probe_traverse(rays), want_i, want_t)
        with pytest.raises(RendererError, match="200 entries, the limit is 144"):
            r.set_traversal_order(1)
        assert r.traversal_order() == 0 and r.wide_stack_capacity() == LDS + 6
        assert _same(r.probe_traverse(rays), want_i, want_t)
    finally:
        r.close()
    r = Renderer(small)
    try:
        r.set_traversal_mode(5)
        r.set_traversal_order(1)
        assert r.wide_stack_capacity() >= model.order_depth(small.boxes)
        with pytest.raises(RendererError, match="200 entries, the limit is 144"):
            r.upload_scene(scene)
        assert r.traversal_order() == 1 and r.wide_stack_capacity() == 0
        with pytest.raises(RendererError, match="no scene uploaded"):
            r.probe_traverse(rays)
        r.set_traversal_order(0)
        r.upload_scene(scene)
        assert r.wide_stack_capacity() == LDS + 6
        assert _same(r.probe_traverse(rays), want_i, want_t)
    finally:
        r.close()
