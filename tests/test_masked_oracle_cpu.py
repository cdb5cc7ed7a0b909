"""tests/masked_oracle.py pinned to the oracle, on the CPU: the helper that tests/test_gpu_masked_oracle.py holds the strategy mask
and the layer accumulators to must itself be the oracle wherever the oracle has an answer (a full mask), must take exactly the
colour out (an empty mask), and must be able to tell the 41 pairs apart.  One sample of make_seeds(W * H) per scene: the Cornell
box and the glass scene at 64 x 48, the open scene of tests/test_gpu_resolve_slim.py at 67 x 33."""
import numpy as np
import pytest

from clive2_amd import strategies as S

import masked_oracle as mo

SCENE_NAMES = ["cornell", "glass", "open"]

# Pixels per pair in the one sample of each scene, (s, t) in bit order -- measured with this file, asserted below.  On the Cornell
# box every pair occurs in at least 20 pixels (the rarest, (0, 2), in 27); the open scene has 21 of the 41.
_ORDER = list(S.PAIRS)
PAIR_PIXELS = {
    "cornell": [362, 1537, 1423, 1461, 1442, 1431, 27, 2519, 2496, 2466, 2488, 2449, 2467, 78, 2135, 2559, 2412, 2435, 2455, 2457,
                40, 2344, 2498, 2444, 2502, 2460, 2396, 34, 2216, 2507, 2432, 2432, 2431, 2438, 44, 2271, 2472, 2470, 2448, 2421,
                2418],
    "glass": [358, 1132, 1115, 1149, 1079, 1159, 27, 1980, 2086, 1985, 1973, 1947, 1940, 51, 1879, 2101, 1921, 1948, 1898, 1894,
              30, 2119, 2120, 2039, 2003, 2007, 1919, 42, 1979, 2150, 2012, 2024, 1967, 1989, 40, 2064, 2082, 2041, 1994, 1980, 1930],
    "open": [0, 82, 24, 8, 3, 0, 0, 108, 10, 3, 1, 0, 0, 11, 27, 4, 3, 0, 0, 0, 1, 28, 2, 1, 0, 0, 0, 7, 7, 1, 0, 0, 0, 0, 0, 5, 0,
             0, 0, 0, 0],
}
NONFINITE_PIXELS = {"cornell": 0, "glass": 0, "open": 0}               # pixels with a pair whose term is not finite (measured)
STAGES = ("finalized", "light", "sample_weights", "unidirectional")
AGG = ("weights", "total_contribution", "contrib_weight_sum")


@pytest.fixture(scope="module")
def scenes(cornell_small, glass_scene):
    return {"cornell": cornell_small, "glass": glass_scene, "open": mo.open_scene(67, 33)}


@pytest.fixture(scope="module")
def traced(scenes, oracle_mod):
    """name -> (a work oracle, the Trace of one sample, the untouched oracle after run_sample(stable_light_sort=True))"""
    out = {}
    for name, scene in scenes.items():
        B = scene.pixel_width * scene.pixel_height
        o = oracle_mod.OracleRenderer(scene, seeds=oracle_mod.make_seeds(B))
        trace = mo.Trace(o)
        ref = oracle_mod.OracleRenderer(scene, seeds=oracle_mod.make_seeds(B))
        ref.run_sample(stable_light_sort=True)
        out[name] = (o, trace, ref)
    return out


@pytest.fixture(scope="module")
def singles(traced):
    """name -> {pair: resolve() of the pair's singleton mask}; computed once, never written"""
    return {name: {p: mo.resolve(o, trace, S.bit(*p)) for p in S.PAIRS} for name, (o, trace, _) in traced.items()}


def _packed_after(o, trace, mask, scene):
    acc = mo.Accumulators(scene)
    out = mo.resolve(o, trace, mask)
    acc.add(o)
    return out, acc


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_a_full_mask_gives_the_oracles_bytes_at_every_stage(name, scenes, traced):
    o, trace, ref = traced[name]
    plain, acc = _packed_after(o, trace, None, scenes[name])
    # the untouched path of the helper is the oracle's run_sample
    for f in AGG:
        assert plain["agg"][f].tobytes() == ref.weight_aggregators[f].tobytes(), f
    assert plain["finalized"].tobytes() == ref.finalized_samples.tobytes()
    assert plain["light"][:, :3].tobytes() == ref.out_light_image[:, :3].tobytes()
    assert (plain["sample_weights"] + plain["light"][:, 3]).tobytes() == ref.sample_weights.tobytes()
    assert plain["unidirectional"].tobytes() == ref.out_camera_image.tobytes()
    assert acc.image.tobytes() == ref.summed_image.tobytes() and acc.weights.tobytes() == ref.summed_sample_weights.tobytes()
    assert acc.unidirectional.tobytes() == ref.unidirectional_image_buffer.tobytes()
    assert acc.counts.tobytes() == ref.summed_sample_counts.tobytes()
    assert np.any(plain["agg"]["total_contribution"] != 0) and np.any(plain["light"][:, :3] != 0)
    # the fold and the shade slots under a full mask, and under all 64 bits, write the same bytes
    total, wsum = mo.fold(trace.log, S.ALL)
    assert total.tobytes() == ref.weight_aggregators["total_contribution"][:, :3].tobytes()
    assert wsum.tobytes() == ref.weight_aggregators["contrib_weight_sum"].tobytes()
    for mask in (S.ALL, 2 ** 64 - 1):
        got, gacc = _packed_after(o, trace, mask, scenes[name])
        for f in AGG:
            assert got["agg"][f].tobytes() == plain["agg"][f].tobytes(), (mask, f)
        for k in STAGES:
            assert got[k].tobytes() == plain[k].tobytes(), (mask, k)
        assert gacc.packed.tobytes() == acc.packed.tobytes()


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_an_empty_mask_gives_no_colour_and_every_weight(name, scenes, traced):
    o, trace, _ = traced[name]
    plain, acc = _packed_after(o, trace, None, scenes[name])
    empty, eacc = _packed_after(o, trace, 0, scenes[name])
    B = o.batch_size
    assert empty["agg"]["total_contribution"].tobytes() == bytes(16 * B)                     # +0
    for k in ("finalized", "light"):
        assert np.ascontiguousarray(empty[k][:, :3]).tobytes() == bytes(12 * B), k
    for f in ("weights", "contrib_weight_sum"):
        assert empty["agg"][f].tobytes() == plain["agg"][f].tobytes(), f
    assert empty["light"][:, 3].tobytes() == plain["light"][:, 3].tobytes()
    for k in ("sample_weights", "unidirectional"):
        assert empty[k].tobytes() == plain[k].tobytes(), k
    assert eacc.packed[:3].tobytes() == bytes(12 * B)
    assert eacc.packed[3:].tobytes() == acc.packed[3:].tobytes()                             # weights, unidirectional, counts
    assert np.any(acc.packed[3] > 0)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_pixels_per_pair(name, traced):
    counts = mo.pair_pixels(traced[name][1].log)
    print(name, "pixels per pair:", counts)
    assert [counts[p] for p in _ORDER] == PAIR_PIXELS[name]
    if name == "cornell":
        assert min(counts.values()) >= 20
    # a log record outside the 41 pairs never carries a flag
    log = traced[name][1].log
    for t in range(7):
        for s in range(7):
            if not S.is_pair(s, t):
                assert not np.any(log[:, t, s, 0])


def _picture(single):
    """the colour one sample adds to the image: light image + finalized sample"""
    return single["light"][:, :3] + single["finalized"][:, :3]


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_the_reference_tells_the_pairs_apart(name, singles, traced):
    """Where both pairs occur, the singleton pictures of (s, t) and (t, s) differ, and so do those of (s, t) and (s + 1, t - 1): a
    kernel that files a pair's colour under the transposed bit, or under a neighbour of the same path length, cannot match."""
    counts = mo.pair_pixels(traced[name][1].log)
    single = singles[name]
    compared = 0
    for s, t in S.PAIRS:
        assert np.any(_picture(single[s, t]) != 0) == (counts[s, t] > 0), (s, t)           # colour exactly where the pair occurs
        for other in ((t, s), (s + 1, t - 1)):
            if other == (s, t) or not S.is_pair(*other) or not counts[s, t] or not counts[other]:
                continue
            assert mo.canonical(_picture(single[s, t])) != mo.canonical(_picture(single[other])), ((s, t), other)
            compared += 1
    print(name, "pairs of pairs compared:", compared)
    assert compared >= (60 if name != "open" else 10)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_nonfinite_terms(name, traced):
    bad = mo.nonfinite_pixels(traced[name][1].log)
    print(name, "pixels with a non-finite term:", int(bad.sum()), "of", bad.size)
    assert int(bad.sum()) == NONFINITE_PIXELS[name]
    assert bad.sum() <= bad.size // 1000                                 # the cap of the tolerance comparisons on the device


def test_masked_sample_render_and_layers_are_one_computation(oracle_mod):
    """masked_sample on one oracle, sample after sample, is masked_render; layered_render's layers are the masked renders of its
    masks and its main rows the oracle's own run_sample; two streams are added pass by pass, stream by stream."""
    import clive2_amd as c2
    scene = c2.create_scene_from_preset("empty", 37, 23)
    B, mask = 37 * 23, S.path_length(2, 3) | S.bit(2, 1) | S.bit(5, 1)
    seeds = np.stack([oracle_mod.make_seeds(B, rank=k) for k in range(2)])
    o = oracle_mod.OracleRenderer(scene, seeds=seeds[0])
    first = mo.masked_sample(o, mask)
    mo.masked_sample(o, mask)
    assert o.samples == 2 and first["log"].shape == (B, 7, 7, 24)
    want = mo.Render(scene, seeds[0], 2).render(mask)
    assert o.summed_image.tobytes() == want.image.tobytes() and o.summed_sample_weights.tobytes() == want.weights.tobytes()
    assert mo.masked_render(scene, seeds[0], mask, 2).tobytes() == want.packed.tobytes()
    assert np.any(want.image != 0)
    # two streams against two untouched oracles that share one pair of accumulators (tests/test_gpu_round5.py)
    table = {"a": mask, "b": S.bit(2, 4), "none": 0}
    main, lacc, rand, rays = mo.layered_render(scene, seeds, table, 2, K=2)
    os_ = [oracle_mod.OracleRenderer(scene, seeds=seeds[k]) for k in range(2)]
    img, wts = np.zeros((23, 37, 3), np.float32), np.zeros((23, 37, 1), np.float32)
    for _ in range(2):
        for x in os_:
            x.summed_image[:] = img; x.summed_sample_weights[:] = wts
            x.run_sample(stable_light_sort=True)
            img, wts = x.summed_image.copy(), x.summed_sample_weights.copy()
    assert main[:3].tobytes() == np.ascontiguousarray(img.reshape(-1, 3).T).tobytes() and main[3].tobytes() == wts.tobytes()
    assert (main[7] == 4).all() and rays == sum(x.rays_traced for x in os_)
    assert np.array_equal(rand, np.stack([x.rand_buffer for x in os_]))
    assert lacc.shape == (3, 3, B) and lacc[2].tobytes() == bytes(12 * B)
    for l, m in enumerate((mask, S.bit(2, 4))):
        assert lacc[l].tobytes() == mo.masked_render(scene, seeds, m, 2, K=2)[:3].tobytes()
        assert np.any(lacc[l] != 0)


def test_the_singletons_fold_to_the_whole_and_halves_add_up(traced):
    """The fold's order is the aggregator's: adding the t >= 2 singleton totals in pair order gives the oracle's bytes; two
    complementary masks add up to the unmasked picture to float32 rounding."""
    o, trace, ref = traced["cornell"]
    acc = np.zeros((o.batch_size, 3), np.float32)
    for p in mo.T2_PAIRS:
        acc = acc + mo.fold(trace.log, S.bit(*p))[0]
    assert acc.tobytes() == ref.weight_aggregators["total_contribution"][:, :3].tobytes()
    P, Q = S.path_length(1, 2), S.path_length(3)
    parts = _picture(mo.resolve(o, trace, P)).astype(np.float64) + _picture(mo.resolve(o, trace, Q)).astype(np.float64)
    full = _picture(mo.resolve(o, trace, None)).astype(np.float64)
    err = np.abs(parts - full)
    print("halves: max |P + Q - full| / full =", float(np.max(err / np.maximum(full, 1e-300))))
    assert np.all(err <= 32.0 * 2.0 ** -24 * parts) and np.any(parts > 0)
