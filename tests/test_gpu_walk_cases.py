"""GPU: every closest-hit walk of the device on the adversarial scenes and ray classes of tests/walk_cases.py, against the C oracle bit
for bit (tests/test_walk_cases_cpu.py holds that oracle to a float64 brute force and counts what each class brings).  No tolerance
anywhere: best_i of every ray, and the bytes of best_t, u, v wherever the oracle reports a hit.

Routes, each asserted from Renderer.organisation() or the walk's tallies:

    tiny       tree and triangles in LDS, the pruned table a flat list of leaves: closest_hit_flat; bit 26 its clamped loop; bit 11 the
               per-lane walk of that table; bit 7 the full table
    lds        tree in LDS, pruned table with inner boxes: closest_hit_impl over the pruned table; bit 7 over the full one
    streamed   the tree through the caches; mode 5: the 4-wide walk (rays with a non-finite 1/d: the binary walk inside that launch),
               without the speculative expansion (bit 13), with 48-byte records (bit 14), with LDS windows of 32, 64, 96 and 0 nodes
    all        set_counting(1): the binary stackless walk that counts the reference's box and triangle tests

plus the nearest-first order and the seeded visibility walk on `streamed`, and -- the walks inside the pipeline's kernels cannot be
probed -- two samples of each scene rendered in every traversal mode against OracleRenderer."""
import importlib.util
import os

import numpy as np
import pytest

import visibility_reference as vis
import walk_cases as wc
from path_compare import nan_vertices, same_paths

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIGHT, CAMERA = 0, 1
f32 = np.float32
# scene, builder; `_open`: the room without its front and right wall -- rays from inside miss everything (27 % of the ordinary ones)
RIGS = [("tiny", "numpy"), ("tiny", "native"), ("lds", "numpy"), ("lds", "native"), ("streamed", "numpy"), ("streamed", "native"),
        ("tiny_open", "numpy"), ("lds_open", "numpy"), ("streamed_open", "numpy")]
ARRANGEMENTS = ("grouped", "reversed", "interleaved")


def _bits(*bits):
    return sum(1 << b for b in bits)


# (name, traversal mode, debug flags, counting) of the probe routes; `only`: the scenes a route exists on
ROUTES = [("mode 0", 0, 0, 0, None),
          ("mode 0, full table (bit 7)", 0, _bits(7), 0, ("tiny", "lds")),
          ("mode 0, per-lane walk of the flat table (bit 11)", 0, _bits(11), 0, ("tiny",)),
          ("mode 0, clamped flat loop (bit 26)", 0, _bits(26), 0, ("tiny",)),
          ("counting the reference's tests", 0, 0, 1, None),
          ("mode 5", 5, 0, 0, None),
          ("mode 5, no speculation (bit 13)", 5, _bits(13), 0, None),
          ("mode 5, 48-byte records (bit 14)", 5, _bits(14), 0, None),
          ("mode 5, bits 13 and 14", 5, _bits(13, 14), 0, None)] + \
         [("mode 5, LDS window %d" % w, 5, w << 20, 0, None) for w in (1, 2, 3, 15)]


class Rig:
    """One scene under one builder: its renderer, its ray classes and the oracle's answers (grouped arrangement), made once."""
    def __init__(self, name, builder, orc):
        from clive2_amd.renderer import Renderer, make_seeds
        self.name, self.base = name, name.replace("_open", "")
        self.scene = wc.scene(self.base, builder, True, name.endswith("_open"))
        self.sets = wc.ray_sets(self.scene)
        self.o, self.d, _, self.spans = wc.arranged(self.sets, "grouped")
        self.rays = wc.make_rays(self.o, self.d)
        self.tri, self.t, self.u, self.v, self.counters = orc.traverse(self.rays, self.scene.boxes, self.scene.triangles)
        self.seeds = make_seeds(wc.W * wc.H)
        self.r = Renderer(self.scene, seeds=self.seeds)

    def settings(self, mode=0, flags=0, counting=0, order=0, query=0, pipelining=-1, levels=0):
        r = self.r
        r.set_counting(0); r.set_connection_query(0); r.set_traversal_order(0); r.set_debug_flags(0)      # nothing refuses the next
        r.set_traversal_mode(mode); r.set_debug_flags(flags); r.set_traversal_order(order); r.set_connection_query(query)
        r.set_pipelining(pipelining); r.set_levels_per_launch(levels); r.set_counting(counting)

    def check(self, got, where, rows=None):
        """`got` = (tri, t, u, v) in the grouped order (of rays `rows`) equals the oracle."""
        rows = slice(None) if rows is None else rows
        tri, t, u, v = self.tri[rows], self.t[rows], self.u[rows], self.v[rows]
        bad = np.flatnonzero(got[0] != tri)
        assert len(bad) == 0, (where, "triangles differ", len(bad), bad[:8], got[0][bad[:8]], tri[bad[:8]])
        hit = tri >= 0
        for name, a, b in (("t", got[1], t), ("u", got[2], u), ("v", got[3], v)):
            bad = np.flatnonzero(hit & (a.view(np.uint32) != b.view(np.uint32)))
            assert len(bad) == 0, (where, name, len(bad), bad[:8], a[bad[:8]], b[bad[:8]])


@pytest.fixture(scope="module")
def rigs(oracle_mod):
    made = {}

    def get(name, builder):
        if (name, builder) not in made:
            made[(name, builder)] = Rig(name, builder, oracle_mod)
        return made[(name, builder)]
    yield get
    for rig in made.values():
        rig.r.close()


@pytest.mark.parametrize("name,builder", RIGS)
def test_each_scene_takes_its_storage_route(name, builder, rigs):
    rig = rigs(name, builder)
    name = rig.base
    rig.settings()
    org = rig.r.organisation()
    boxes = rig.scene.boxes
    n_leaves = int((boxes["right"] != 0).sum())
    assert org["n_records"] == len(boxes) and org["wide_nodes"] > 0, org
    if name == "tiny":      # a pruned table of the leaves alone: closest_hit_flat
        assert org["tree_in_lds"] == 1 and org["pruned_records"] == n_leaves < org["n_records"], org
    elif name == "lds":     # inner boxes survive in the pruned table: closest_hit_impl over it
        assert org["tree_in_lds"] == 1 and n_leaves < org["pruned_records"] < org["n_records"], org
    else:
        assert org["tree_in_lds"] == 0 and org["pruned_records"] == 0, org
    if name != "streamed":
        rig.settings(flags=_bits(7))
        assert rig.r.organisation()["pruned_records"] == 0
        rig.settings()


@pytest.mark.parametrize("how", ARRANGEMENTS)
@pytest.mark.parametrize("name,builder", RIGS)
def test_closest_hit_every_route(name, builder, how, rigs):
    """Every probe route returns the oracle's hit for every ray of every class, whatever the rays' order in the launch: class after
    class, reversed, or with single rays of non-finite 1/d among 63 ordinary ones.  Under set_counting(1) the device's box and
    triangle test tallies are the oracle's."""
    rig = rigs(name, builder)
    o, d, perm, _ = wc.arranged(rig.sets, how)
    rays = wc.make_rays(o, d)
    if name.endswith("_open"):
        assert (rig.tri[rig.spans["ordinary"]] < 0).sum() > 0.2 * len(rig.sets["ordinary"][0])
    try:
        for route, mode, flags, counting, only in ROUTES:
            if only is not None and rig.base not in only:
                continue
            rig.settings(mode=mode, flags=flags, counting=counting)
            rig.r.reset_counters()
            got = wc.back(perm, *rig.r.probe_traverse(rays))
            rig.check(got, (name, builder, how, route))
            if counting:
                c = rig.r.counters()
                assert (c["counted_rays"], c["box_tests"], c["tri_tests"]) == \
                       (len(rays), rig.counters["box_tests"], rig.counters["tri_tests"]), (route, c, rig.counters)
    finally:
        rig.settings()


@pytest.mark.parametrize("name,builder", [("lds", "numpy"), ("streamed", "numpy"), ("streamed", "native")])
def test_both_walks_of_the_wide_launch_run(name, builder, rigs):
    """set_counting(2), mode 5: the rays with a non-finite 1/d (all of axis and in_plane, a part of tiny_inverse and outside) read
    binary records and visit no wide node; the others visit wide nodes and read no binary record.  Same hits as uncounted."""
    rig = rigs(name, builder)
    with np.errstate(divide="ignore", over="ignore"):
        finite = np.isfinite(f32(1.0) / rig.d).all(axis=1)
    assert not finite[rig.spans["axis"]].any() and not finite[rig.spans["in_plane"]].any() and finite[rig.spans["ordinary"]].all()
    try:
        rig.settings(mode=5, counting=2)
        for rows, binary in ((np.flatnonzero(~finite), True), (np.flatnonzero(finite), False)):
            rig.r.reset_counters()
            got = rig.r.probe_traverse(rig.rays[rows])
            tally = rig.r.walk_tallies()["subpath"]
            rig.check(got, (name, builder, "counting 2", binary), rows)
            assert tally["rays"] == len(rows) > 1000, tally
            if binary:
                assert tally["binary_records"] > len(rows) and tally["wide_visits"] == 0, tally
            else:
                assert tally["wide_visits"] > len(rows) and tally["binary_records"] == 0 and tally["tri_records"] > 0, tally
    finally:
        rig.settings()


def _order_tool():
    spec = importlib.util.spec_from_file_location("exp_order_ab", os.path.join(ROOT, "tools", "exp_order_ab.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("builder", ["numpy", "native"])
def test_nearest_first_order_on_streamed(builder, rigs):
    """cl2_set_traversal_order(1) on the doubled mesh: neither order misses what the other hits, and every ray whose (triangle, t bits)
    differ is a hit in front of its own leaf box (tools/exp_order_ab.py: compare_orders) -- an exact-t tie, thousands of them here, is
    settled as the reference's order settles it (csrc/bvh_traverse.hpp: tri_test_tie_rule, the tri_rank table)."""
    rig = rigs("streamed", builder)
    chunks = [(k, rig.o[sp], rig.d[sp]) for k, sp in rig.spans.items()]
    res = _order_tool().compare_orders(rig.scene, chunks)
    print({k: res[k] for k in ("rays", "differ", "ties", "non_ties", "in_front_of_own_leaf")})
    assert res["rays"] == len(rig.o) and res["by_kind"]["aimed"]["rays"] > 7000
    assert res["missed_by_order0"] == 0 and res["missed_by_order1"] == 0, res
    assert res["in_front_of_own_leaf"] == res["differ"], res
    # and order 0 of that tool's renderer is this module's oracle: order 1 on the module's renderer, ties included
    try:
        rig.settings(mode=5, order=1)
        tri, t, _, _ = rig.r.probe_traverse(rig.rays)
        differ = (tri != rig.tri) | ((rig.tri >= 0) & (t.view(np.uint32) != rig.t.view(np.uint32)))
        assert differ.sum() == res["differ"], (int(differ.sum()), res["differ"])
    finally:
        rig.settings()


@pytest.fixture(scope="module")
def seeded(rigs):
    """The finite-1/d rays of `streamed` for the seeded walk (ordinary, every third aimed ray, delta), their targets and the
    restatement's verdicts (tests/visibility_reference.py: visible), made once."""
    rig = rigs("streamed", "numpy")
    rows = np.concatenate([np.arange(sp.start, sp.stop)[::step] for sp, step in
                           ((rig.spans["ordinary"], 2), (rig.spans["aimed"], 3), (rig.spans["delta"], 1))])
    o, d, hit = rig.o[rows], rig.d[rows], rig.tri[rows]
    assert (hit >= 0).all()
    twin = wc.twin(rig.scene)
    copy = np.where(twin[hit] >= 0, twin[hit], hit).astype(np.int32)
    rng = np.random.RandomState(7)
    n_tris = len(rig.scene.triangles)
    other = ((hit + 1 + rng.randint(0, n_tris - 1, len(hit))) % n_tris).astype(np.int32)
    targets = {"hit": hit.astype(np.int32), "copy": copy, "other": other}
    verdicts = dict(zip(targets, vis.visible(rig.scene, o, d, np.stack(list(targets.values())))))
    return rig, rows, o, d, targets, verdicts


@pytest.mark.parametrize("kind", ["hit", "copy", "other"])
def test_seeded_visibility_on_streamed(kind, seeded):
    """cl2_probe_visibility with the oracle's hit as the target (visible, t to the bit, wherever the restatement says so: all but a
    few ties), with its coincident copy (the tie rule: the
    copy is visible iff it is the one the reference's order meets first -- the restatement's verdict and t) and with a random other
    triangle (the restatement's verdict).  Bit 14 gives the same bytes."""
    rig, rows, o, d, targets, verdicts = seeded
    T, want = targets[kind], verdicts[kind]
    rays = wc.make_rays(o, d)
    tris = rig.scene.triangles
    v0 = tris["v0"][:, :3].astype(f32)
    ok_T, t_T = vis.tri_hit(o, d, v0[T], tris["v1"][T, :3].astype(f32) - v0[T], tris["v2"][T, :3].astype(f32) - v0[T])
    try:
        rig.settings(mode=5)
        tri, t = rig.r.probe_visibility(rays, T)
        got = tri == T
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (kind, len(bad), len(T), bad[:8], tri[bad[:8]], T[bad[:8]])
        assert np.array_equal(tri == -1, ~ok_T) and np.isinf(t[~ok_T]).all()
        assert t[got].tobytes() == t_T[got].tobytes()
        blocked = ok_T & ~got
        assert (tri[blocked] >= 0).all() and (t[blocked] <= t_T[blocked]).all()
        if kind == "hit":
            # the oracle's hit is visible, except where the restatement -- which tries every leaf whose own box the ray enters --
            # finds a blocker in a leaf the oracle's walk never tested, the order dependence cl2_set_connection_query documents
            # (tests/test_walk_cases_cpu.py: fewer than 0.5 % of the aimed rays; 6 of these 5,693)
            assert ok_T.all() and (~want).sum() < 0.005 * len(T)
            assert t[want].tobytes() == rig.t[rows][want].tobytes()
        if kind == "copy":                                    # both verdicts occur: the copy is met first (47 rays), or the original is
            moved = T != targets["hit"]
            assert moved.sum() > 2000 and 20 < want[moved].sum() < moved.sum() - 2000
            at_t = t[moved & ~want].view(np.uint32) == t_T[moved & ~want].view(np.uint32)               # blocked at exactly t_T,
            assert (~at_t).sum() < 0.005 * len(T)                                                        # but for that order dependence
        rig.settings(mode=5, flags=_bits(14))
        tri2, t2 = rig.r.probe_visibility(rays, T)
        assert tri2.tobytes() == tri.tobytes() and t2.tobytes() == t.tobytes()
    finally:
        rig.settings()


def test_unseeded_and_axis_rays_of_the_visibility_probe(rigs):
    """Target -1 is cl2_probe_traverse byte for byte, for every class; a ray with a non-finite 1/d returns the unseeded result whatever
    its target."""
    rig = rigs("streamed", "numpy")
    try:
        rig.settings(mode=5)
        tri, t = rig.r.probe_visibility(rig.rays, np.full(len(rig.rays), -1, np.int32))
        bi, bt, _, _ = rig.r.probe_traverse(rig.rays)
        assert tri.tobytes() == bi.tobytes() and t.tobytes() == bt.tobytes()
        rig.check((tri, t, rig.u, rig.v), "visibility probe, no target")
        rows = np.concatenate([np.arange(rig.spans[k].start, rig.spans[k].stop) for k in ("axis", "in_plane")])
        held = np.where(rig.tri[rows] >= 0, rig.tri[rows], 0).astype(np.int32)
        n_tris = len(rig.scene.triangles)
        for flags in (0, _bits(14)):
            rig.settings(mode=5, flags=flags)
            for target in (held, ((held + 1) % n_tris).astype(np.int32), np.full(len(rows), n_tris - 1, np.int32)):
                tri, t = rig.r.probe_visibility(rig.rays[rows], target)
                assert tri.tobytes() == bi[rows].tobytes() and t.tobytes() == bt[rows].tobytes()
    finally:
        rig.settings()


# ---- the walks inside the pipeline's kernels ----
def _combinations(name):
    out = [dict(mode=m, pipelining=p) for m in range(6) for p in (0, 2)]
    out += [dict(mode=m, pipelining=0, flags=_bits(12)) for m in (2, 4)]
    out += [dict(mode=1, pipelining=0, levels=1), dict(mode=1, pipelining=0, levels=6)]
    if name == "tiny":
        out += [dict(mode=0, pipelining=p, flags=_bits(25)) for p in (0, 2)]
    return out


@pytest.fixture(scope="module")
def rendered(oracle_mod):
    """Two samples of each scene (numpy builder) by OracleRenderer, made once: the last sample's Path[] of both kinds, the RNG buffer,
    the aggregators, the ray count -- and the connection rays' and vertices' statistics."""
    out = {}
    for name in ("tiny", "lds", "streamed"):
        sc = wc.scene(name)
        from clive2_amd.renderer import make_seeds
        o = oracle_mod.OracleRenderer(sc, seeds=make_seeds(wc.W * wc.H))
        zero_rays = on_copies = 0
        copies = np.bincount(wc.coincident(sc))[wc.coincident(sc)]
        for _ in range(2):
            o.run_sample()
            zero_rays += connection_rays_with_a_zero_component(o.out_light_paths, o.out_camera_paths)
            for p in (o.out_light_paths, o.out_camera_paths):
                live = np.arange(p["rays"].shape[1])[None, :] < p["length"][:, None]
                tri = p["rays"]["triangle"]
                on_copies += int((live & (tri >= 0) & (copies[np.maximum(tri, 0)] >= 2)).sum())
        out[name] = dict(light=o.out_light_paths.copy(), camera=o.out_camera_paths.copy(), seeds=o.rand_buffer.copy(),
                         agg={f: o.weight_aggregators[f].copy() for f in ("weights", "total_contribution", "contrib_weight_sum")},
                         rays=o.rays_traced, zero_rays=zero_rays, on_copies=on_copies)
    return out


def connection_rays_with_a_zero_component(lp, cp):
    """Connection rays (light vertex s - 1 toward camera vertex t - 1, every pair both subpaths are long enough for) whose float32
    direction has an exact zero component: both ends on one wall or plate."""
    from oracle.np_kernels import _normalize
    count = 0
    o_l, o_c = lp["rays"]["origin"][:, :6, :3].astype(f32), cp["rays"]["origin"][:, :6, :3].astype(f32)
    for s in range(1, 7):
        for t in range(1, 7):
            m = (lp["length"] >= s) & (cp["length"] >= t)
            v = o_c[m, t - 1] - o_l[m, s - 1]
            with np.errstate(divide="ignore", invalid="ignore"):
                dn = _normalize(v)
            count += int((np.isfinite(dn).all(axis=1) & (dn == 0).any(axis=1)).sum())
    return count


@pytest.mark.parametrize("name", ["tiny", "lds", "streamed"])
def test_the_pipeline_walks_render_the_adversarial_scenes(name, rigs, rendered):
    """k_trace_subpath, k_subpaths_persistent, k_traverse_persistent, k_traverse_conn and k_connect_walk_lds have no probe: two samples
    at 32 x 18 in traversal modes 0-5, serial and with three pipeline stages, bit 12 on modes 2 and 4, one and six levels per launch,
    and bit 25 on `tiny`, against OracleRenderer -- Path[] of both kinds, the RNG buffer, the three aggregator fields, the ray count.
    Vertices on the plates and the walls make connection rays with exact zero components whose origins lie on slab planes: hundreds
    a scene.  Bytes first; where they differ, with every NaN in one bit pattern (the device's and the host's default NaN differ in the
    sign bit: DESIGN 2.2) -- which cannot hide a failure while fewer than 1 % of the vertices hold a NaN.  (On the committed seeds no
    vertex does: a zero-area triangle's test yields NaN u, v, t and `t > DELTA` rejects it, so none is ever hit.)"""
    rig, want = rigs(name, "numpy"), rendered[name]
    # (2,333 / 2,094 / 2,108 such rays and 97 / 572 / 610 vertices on doubled faces in the two samples)
    assert want["zero_rays"] >= 1000 and want["on_copies"] >= (40 if name == "tiny" else 250), (want["zero_rays"], want["on_copies"])
    for p in (want["light"], want["camera"]):
        bad, live = nan_vertices(p)
        assert bad < 0.01 * live, (bad, live)
    r = rig.r
    how = {}
    try:
        for combo in _combinations(name):
            rig.settings(**combo)
            r.set_seeds(rig.seeds); r.reset_accumulators(); r.reset_counters()
            r.run_samples(2)
            for which, key in ((LIGHT, "light"), (CAMERA, "camera")):
                same = same_paths(r.export_paths(which), want[key])
                assert same is not None, (name, combo, key)
                how[same] = how.get(same, 0) + 1
            assert np.array_equal(r.get_random_buffer(), want["seeds"]), (name, combo)
            agg = r.export_aggregators()
            for f, ref in want["agg"].items():
                a, b = agg[f], ref
                same = a.tobytes() == b.tobytes() or (np.array_equal(np.isnan(a), np.isnan(b)) and
                                                      np.where(np.isnan(a), 0, a).tobytes() == np.where(np.isnan(b), 0, b).tobytes())
                assert same, (name, combo, f)
            assert r.counters()["rays"] == want["rays"], (name, combo)
    finally:
        rig.settings()
        r.set_seeds(rig.seeds); r.reset_accumulators()
    print(name, how)


def test_connection_query_on_streamed(rigs):
    """cl2_set_connection_query(1) is active on `streamed` in mode 5, and its aggregators after two samples have mode 0's bytes."""
    rig = rigs("streamed", "numpy")
    r = rig.r
    agg = []
    try:
        for query in (0, 1):
            rig.settings(mode=5, query=query, pipelining=0)
            assert r.connection_query_active() == query
            r.set_seeds(rig.seeds); r.reset_accumulators(); r.reset_counters()
            r.run_samples(2)
            agg.append(r.export_aggregators())
    finally:
        rig.settings()
        r.set_seeds(rig.seeds); r.reset_accumulators()
    for f in ("weights", "total_contribution", "contrib_weight_sum"):
        assert agg[0][f].tobytes() == agg[1][f].tobytes(), f
