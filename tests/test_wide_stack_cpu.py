"""CPU tests of the two bounds the per-lane stack of the 4-wide walk is sized from (csrc/scene_prep.hpp: build_wide's order_depth,
wide_overflow_entries; the kernel, csrc/bvh_wide.hpp, does not clamp its pushes), against a restatement of the walk's own push and
pop rules (tests/wide_walk_reference.py) -- no GPU, and nothing of the hipcc-built library.

    reference child order     peak sp <= WIDE_STACK_LDS + min(136, 2 x max_pending + 4)
    nearest child first       peak sp <= order_depth, and a ray along a left-leaning chain reaches exactly that

on the trees of tests/wide_stack_cases.py: a left chain of 40 inner boxes over a row of plates (max_pending 1: the stack sized from
the pending depth alone held 14 entries, the rays along the chain stack 40), the GPU builder's PLOC trees with one-triangle leaves over
the glass scenes (order_depth 27 and 32 against 26 and 30 entries of the old sizing; the deepest stack any ray of these tests
reaches there is 11 and 12), and random uneven trees.  The model's hits in both orders are the oracle's, bit for bit, except where
a hit lies in front of its own leaf box (tests/test_order_independence.py)."""
import numpy as np
import pytest

import wide_stack_cases as cases
import wide_walk_reference as model
from test_order_independence import predict, visit_rank
from test_scene_prep_cpu import Input, inputs, lib, scenes          # noqa: F401 (fixtures)

LDS, OVERFLOW = model.WIDE_STACK_LDS, model.WIDE_STACK_OVERFLOW
N_PLATE_RAYS = 256


def old_capacity(max_pending):
    """Entries per lane when the overflow array was sized from the reference's pending depth whatever the child order."""
    return LDS + min(OVERFLOW, 2 * max_pending + 4)


class Walked:
    """One tree: what prepare_scene made of it, the oracle's hits on its rays and the model's walks of them."""
    def __init__(self, L, orc, scene, o, d, n_plate_rays=0):
        from clive2_amd import struct_types as st
        self.scene, self.o, self.d, self.n_plate_rays = scene, o, d, n_plate_rays
        err, self.out = Input(scene).prepare(L)
        assert err is None, err
        rays = np.zeros(len(o), dtype=st.Ray)
        rays["origin"][:, :3] = o; rays["direction"][:, :3] = d
        rays["inv_direction"][:, :3] = np.float32(1.0) / d
        self.want_i, self.want_t = orc.traverse(rays, scene.boxes, scene.triangles)[:2]
        rank = visit_rank(scene.boxes, len(scene.triangles))
        self.explained = np.concatenate([predict(o[lo:lo + 1024], d[lo:lo + 1024], scene.boxes, scene.triangles, rank)[2]
                                         for lo in range(0, len(o), 1024)])
        self.walks = {(order, spec): self.walk(order, spec) for order in (0, 1) for spec in (True, False)}

    def walk(self, order, spec=True, rays=slice(None)):
        b = self.scene.boxes
        return model.walk(np.frombuffer(self.out["wide"], np.float32), b["min"][0], b["max"][0], np.frombuffer(self.out["tris"], np.float32),
                          np.frombuffer(self.out["tri_rank"], np.int32), self.o[rays], self.d[rays], order, spec=spec)


@pytest.fixture(scope="module")
def trees(lib, oracle_mod):
    chain = cases.plate_chain(cases.plate_scene(39))
    po, pd = cases.plate_rays(N_PLATE_RAYS)
    ro, rd = cases.random_rays(2000, 11)
    out = {"left_chain": Walked(lib, oracle_mod, chain, np.concatenate([po, ro]), np.concatenate([pd, rd]), N_PLATE_RAYS)}
    for sub in (2, 3):
        glass = cases.glass(sub)
        o, d = cases.glass_rays(glass)
        out[f"ploc{sub}"] = Walked(lib, oracle_mod, cases.ploc_tree(glass), o, d)
        if sub == 2:
            for seed in (1, 2, 3):
                out[f"random{seed}"] = Walked(lib, oracle_mod, cases.random_tree(glass, seed), o, d)
    return out


def test_the_trees_are_the_ones_the_bounds_differ_on(trees):
    """(max_pending, order_depth) of every tree: the chain and the PLOC trees are deeper, nearest first, than the stack sized from the
    pending depth; every tree has a 4-wide collapse."""
    got = {name: (w.out["max_pending"], w.out["order_depth"]) for name, w in trees.items()}
    assert got["left_chain"] == (1, 40) and got["ploc2"] == (7, 27) and got["ploc3"] == (9, 32), got
    for name in ("left_chain", "ploc2", "ploc3", "random1", "random2", "random3"):
        assert got[name][1] > old_capacity(got[name][0]), (name, got[name])
    assert all(w.out["n_wide"] > 0 for w in trees.values())


def test_order_depth_is_the_structural_bound(lib, inputs, trees):
    """PreparedScene.order_depth equals the Python statement on the reference Box[] wherever there is a 4-wide collapse, and is 0
    where there is none."""
    for name, inp in inputs.items():
        out = inp.prepare(lib)[1]
        assert out["order_depth"] == (model.order_depth(inp.boxes) if out["n_wide"] > 0 else 0), name
    for name, w in trees.items():
        assert w.out["order_depth"] == model.order_depth(w.scene.boxes) > 0, name


def test_the_reference_order_stays_within_its_bound(trees):
    for name, w in trees.items():
        for spec in (True, False):
            assert w.walks[0, spec]["peak"].max() <= old_capacity(w.out["max_pending"]), (name, spec)


def test_the_nearest_first_order_stays_within_order_depth(trees):
    """With and without the speculative expansion (which only ever works within the LDS part: no transient entry beyond the bound
    shows in the model)."""
    for name, w in trees.items():
        print(f"{name:8s} max_pending {w.out['max_pending']:2d}  old capacity {old_capacity(w.out['max_pending']):3d}  order_depth {w.out['order_depth']:3d}  "
              f"model peak: reference order {w.walks[0, True]['peak'].max()}, nearest first {w.walks[1, True]['peak'].max()}")
        for spec in (True, False):
            assert w.walks[1, spec]["peak"].max() <= w.out["order_depth"], (name, spec)


def test_rays_along_the_chain_reach_order_depth_exactly(trees):
    """The bound is tight, and the test bites: every plate ray stacks 40 entries where the old sizing gave a lane 14."""
    w = trees["left_chain"]
    assert old_capacity(w.out["max_pending"]) == 14
    for spec in (True, False):
        peak = w.walks[1, spec]["peak"][:N_PLATE_RAYS]
        assert (peak == w.out["order_depth"]).all(), (spec, peak.min(), peak.max())
        assert (peak > 14).sum() >= 64
        assert (w.walks[1, spec]["spills"][:N_PLATE_RAYS] == w.out["order_depth"] - LDS).all()


def test_hits_of_both_orders_are_the_oracles(trees):
    for name, w in trees.items():
        for (order, spec), got in w.walks.items():
            same = (got["tri"] == w.want_i) & (got["t"].view(np.uint32) == w.want_t.view(np.uint32))
            assert same[w.explained].all(), (name, order, spec, np.flatnonzero(w.explained & ~same)[:5])
            if order == 0:
                assert same.all(), (name, spec)                  # the reference's order is exact for every ray
        assert (~w.explained).sum() < len(w.explained) // 10, (name, int((~w.explained).sum()), len(w.explained))
        assert w.explained[:w.n_plate_rays].all(), name
    assert (trees["left_chain"].want_i[:N_PLATE_RAYS] == 38).all()    # the plate rays hit the nearest plate: the chain's deepest


def test_overflow_sizing(lib, inputs, trees):
    entries = lib.sp_wide_overflow_entries
    assert (lib.sp_wide_stack_lds(), lib.sp_wide_stack_overflow()) == (LDS, OVERFLOW)
    # order 0: what cl2_upload_scene has always allocated
    pinned = {"cornell": 6, "glass": 16, "mesh": 22, "big_leaf": 6, "not_nested": 6, "chain": 52}
    prepared = {name: inp.prepare(lib)[1] for name, inp in inputs.items()}
    prepared.update({name: w.out for name, w in trees.items()})
    for name, out in prepared.items():
        mp, depth = out["max_pending"], out["order_depth"]
        assert entries(mp, depth, 0) == min(OVERFLOW, 2 * mp + 4) == pinned.get(name, 2 * mp + 4), name
        assert entries(mp, depth, 1) >= max(depth - LDS, entries(mp, depth, 0)), name
        assert entries(mp, depth, 1) <= OVERFLOW
    assert entries(1, 40, 1) == 36 and entries(7, 27, 1) == 23 and entries(9, 32, 1) == 28      # depth - LDS + 4 entries of slack
    assert entries(24, 36, 1) == entries(24, 36, 0) == 52                                          # never below order 0's
    # the cap: a lane has LDS + OVERFLOW entries at the most
    assert entries(1, LDS + OVERFLOW, 1) == OVERFLOW and entries(1, LDS + OVERFLOW + 1, 1) == -1
    assert entries(62, 0, 0) == 128 and entries(70, 0, 0) == OVERFLOW
    # a left chain of 200 inner boxes: accepted, served in the reference's order, not nearest first
    long_chain = cases.plate_chain(cases.plate_scene(199))
    err, out = Input(long_chain).prepare(lib)
    assert err is None and (out["max_pending"], out["order_depth"]) == (1, 200) and model.order_depth(long_chain.boxes) == 200
    assert entries(1, 200, 0) == 6 and entries(1, 200, 1) == -1
