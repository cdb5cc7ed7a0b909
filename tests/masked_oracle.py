"""A masked oracle: the CPU reference of the strategy mask and the layer accumulators (TEST INFRASTRUCTURE, plain numpy over oracle/).

The oracle's connect stage can log, for every connected pair (s, t) of every pixel, the MIS weight w, the path density p_s, the
geometry term g and the colour (oracle.strategy_log).  Two facts make that log a reference for ANY mask:

  * t >= 2 and s = 0: the aggregator's colour is the float32 fold `total += (color * (w * g)) / p_s` over the logged pairs, t outer
    and s inner (bdpt_oracle.c: connect_paths_one).  Folding only the pairs whose mask bit is set gives the masked colour; the
    weight sum takes every pair, masked or not.
  * t = 1: pair (s, 1) of source pixel id owns slot s * B + id of the five light arrays.  Writing +0 into `out_light_shade` of the
    masked-out pairs leaves every weight in place and takes the colour out of K8's sum (w * 0 = +0).

Everything after the connect stage -- finalize_samples, the stable sort, K8, process_images -- is the oracle's own code.
tests/test_masked_oracle_cpu.py pins this file to the unmasked oracle.  Masks have the bit layout of clive2_amd/strategies.py.
"""
import numpy as np

from clive2_amd import strategies as S

F = np.float32
T2_PAIRS = [(s, t) for s, t in S.PAIRS if t >= 2]       # in the kernel's order: t outer, s inner
T1_PAIRS = [(s, t) for s, t in S.PAIRS if t == 1]


def open_scene(w, h):
    """The open scene of tests/test_gpu_resolve_slim.py: emitter, floor, back wall and a glass ball (328 triangles) -- specular
    vertices on both subpaths, subpaths of every length, pixels with and without a contribution."""
    import clive2_amd as c2
    from clive2_amd.load import triangles_for_box
    from clive2_amd.meshes import icosphere
    keep = [t for t in triangles_for_box() if t.emitter or t.n[1] > 0.5 or t.n[2] > 0.5]
    scene = c2.create_scene(w, h, np.array([0, 1.5, 6.0]), np.array([0, 0, -1.0]), room=keep,
                            file_specs=[dict(mesh=icosphere(2, radius=1.5), material=5, offset=np.array([0.5, 0.0, -1.0]))])
    assert len(scene.triangles) == 328
    return scene


def canonical(a):
    """bytes of a float array, every NaN made the same NaN"""
    a = np.array(a, dtype=F, copy=True)
    a[np.isnan(a)] = np.nan
    return a.tobytes()


def pair_terms(log):
    """{(s, t): (flag[B] bool, term[B, 3] float32, w[B] float32)} of the t >= 2 pairs (s = 0 included) of a strategy log: the
    addend of the aggregator's colour as the oracle rounds it, and the addend of its weight sum."""
    out = {}
    with np.errstate(all="ignore"):
        for s, t in T2_PAIRS:
            rec = log[:, t, s]
            w, p_s, g, color = rec[:, 1], rec[:, 2], rec[:, 4], rec[:, 5:8]
            term = (color * (w * g)[:, None]) / p_s[:, None]
            assert term.dtype == F
            out[s, t] = (rec[:, 0] == 1.0, term, w)
    return out


def fold(log, mask):
    """(total_contribution[B, 3], contrib_weight_sum[B]) of a strategy log under `mask`, float32, in the kernel's pair order."""
    mask = S.to_mask(mask)
    B = log.shape[0]
    total, wsum = np.zeros((B, 3), F), np.zeros(B, F)
    with np.errstate(all="ignore"):
        for (s, t), (flag, term, w) in pair_terms(log).items():
            if mask & S.bit(s, t):
                total = np.where(flag[:, None], total + term, total)
            wsum = np.where(flag, wsum + w, wsum)
    assert total.dtype == F and wsum.dtype == F
    return total, wsum


def pair_pixels(log):
    """{(s, t): the number of pixels whose log has the pair} for all 41 pairs"""
    return {(s, t): int((log[:, t, s, 0] == 1.0).sum()) for s, t in S.PAIRS}


def nonfinite_pixels(log):
    """bool[B]: the pixels with a logged pair, of any t, whose term (color * (w * g)) / p_s is not finite"""
    bad = np.zeros(log.shape[0], bool)
    with np.errstate(all="ignore"):
        for s, t in S.PAIRS:
            rec = log[:, t, s]
            term = (rec[:, 5:8] * (rec[:, 1] * rec[:, 4])[:, None]) / rec[:, 2][:, None]
            bad |= (rec[:, 0] == 1.0) & ~np.all(np.isfinite(term), axis=1)
    return bad


_LIGHT_ARRAYS = ("out_light_indices", "out_light_path_indices", "out_light_ray_indices", "out_light_weights", "out_light_shade")


class Trace:
    """One oracle sample after the connect stage, as copies: what the rest of the sample reads.  Tracing does not depend on the
    mask, so every mask of a render is derived from the same Trace."""

    def __init__(self, o):
        from oracle import oracle as orc
        o.make_light_rays(); o.make_camera_rays(); o.trace_light_rays(); o.trace_camera_rays()
        self.log = orc.strategy_log(o)                                  # runs join_paths
        self.agg = o.weight_aggregators.copy()
        self.light = {k: getattr(o, k).copy() for k in _LIGHT_ARRAYS}
        self.light_paths = o.out_light_paths.copy()
        self.unidirectional = o.out_camera_image.copy()
        self._fold = {}

    def fold(self, mask):
        if mask not in self._fold:
            self._fold[mask] = fold(self.log, mask)
        return self._fold[mask]


def resolve(work, trace, mask=None):
    """The rest of one sample under `mask` on the oracle `work` (any OracleRenderer of the scene; its per-sample arrays are
    replaced): finalize_samples, gather_light_image(stable=True).  mask=None is the oracle untouched; an integer goes through the
    fold and the shade slots, S.ALL included.  Returns the per-sample outputs as the device exports them: `agg`, `finalized`,
    `light` (b, g, r and K8's weight sum), `sample_weights` (of finalize_samples, before K8 adds to them), `unidirectional`;
    `work` is left ready for process_images()."""
    B = work.batch_size
    work.weight_aggregators = trace.agg.copy()
    for k in _LIGHT_ARRAYS:
        setattr(work, k, trace.light[k].copy())
    work.out_light_paths = trace.light_paths.copy()                      # copies: a later stage call of `work` writes into them
    work.out_camera_image = trace.unidirectional.copy()
    if mask is not None:
        mask = S.to_mask(mask)
        total, wsum = trace.fold(mask & S.CAMERA_IMAGE)
        assert canonical(wsum) == canonical(trace.agg["contrib_weight_sum"])                 # the weight sum ignores the mask
        work.weight_aggregators["total_contribution"][:, :3] = total
        for s, _ in T1_PAIRS:
            if not mask & S.bit(s, 1):
                work.out_light_shade[s * B:(s + 1) * B] = 0.0            # +0: the pair keeps its weight and loses its colour
    work.finalize_samples()
    sample_weights = work.sample_weights.copy()
    work.sample_weights[:] = 0.0
    work.gather_light_image(stable=True)                                 # K8: sum_weights[id] += weight_sum
    light_w = work.sample_weights.copy()
    work.sample_weights[:] = sample_weights + light_w
    light = work.out_light_image.copy()
    light[:, 3] = light_w
    return dict(agg=work.weight_aggregators.copy(), finalized=work.finalized_samples.copy(), light=light,
                sample_weights=sample_weights, unidirectional=work.out_camera_image.copy())


def masked_sample(o, mask=None):
    """One oracle sample of `o` under `mask`, through the stage calls with the log on, run to the end (process_images adds it to
    o's accumulators).  Returns resolve()'s dictionary plus `log`."""
    trace = Trace(o)
    out = resolve(o, trace, mask)
    o.process_images()
    o.samples += 1
    out["log"] = trace.log
    return out


class Accumulators:
    """The four host accumulators of one render, and their packed form [8][W*H] (include/clive2_amd.h)."""

    def __init__(self, scene):
        res = (scene.pixel_height, scene.pixel_width)
        self.image, self.weights = np.zeros((*res, 3), F), np.zeros((*res, 1), F)
        self.counts, self.unidirectional = np.zeros((*res, 1), np.int32), np.zeros((*res, 3), F)
        self.nonfinite = np.zeros(res, bool)                            # a per-sample addend of the image was not finite

    def add(self, work):
        """process_images of the sample that `work` holds"""
        work.summed_image, work.summed_sample_weights = self.image, self.weights
        work.summed_sample_counts, work.unidirectional_image_buffer = self.counts, self.unidirectional
        with np.errstate(all="ignore"):
            addend = work.out_light_image[:, :3] + work.finalized_samples[:, :3]
        self.nonfinite |= ~np.all(np.isfinite(addend), axis=1).reshape(self.nonfinite.shape)
        work.process_images()

    @property
    def packed(self):
        rows = [self.image[..., c] for c in range(3)] + [self.weights[..., 0]] + \
               [self.unidirectional[..., c] for c in range(3)] + [self.counts[..., 0].astype(F)]
        return np.stack([np.ascontiguousarray(r, dtype=F).reshape(-1) for r in rows])


class Render:
    """`passes` passes of K sample streams of one scene, traced once: one oracle per stream, seeded with seeds[k].  render(mask)
    adds the samples into one set of accumulators pass by pass and stream by stream, as the product does, and is kept per mask
    (never written).  `seeds`: (B, 2) for one stream, else (K, B, 2)."""

    def __init__(self, scene, seeds, passes, K=1):
        from oracle import oracle as orc
        seeds = np.asarray(seeds, dtype=np.uint32).reshape(K, -1, 2)
        self.scene, self.passes, self.K = scene, passes, K
        streams = [orc.OracleRenderer(scene, seeds=seeds[k]) for k in range(K)]
        self.traces = [Trace(o) for _ in range(passes) for o in streams]          # pass by pass, stream by stream
        self.seeds = np.stack([o.rand_buffer for o in streams]) if K > 1 else streams[0].rand_buffer.copy()
        self.rays = sum(o.rays_traced for o in streams)
        self.work = streams[0]
        self._cache = {}

    def render(self, mask=None):
        """Accumulators of the render under `mask` (None: the oracle untouched)"""
        mask = None if mask is None else S.to_mask(mask)
        if mask not in self._cache:
            acc = Accumulators(self.scene)
            for trace in self.traces:
                resolve(self.work, trace, mask)
                acc.add(self.work)
            self._cache[mask] = acc
        return self._cache[mask]

    def layers(self, table):
        """float32 (L, 3, W*H): what cl2_read_layers_packed holds after this render under the layer table `table`"""
        masks = S.layer_masks(table)
        return np.stack([self.render(m).packed[:3] for m in masks]) if masks else np.zeros((0, 3, self.work.batch_size), F)


def masked_render(scene, seeds, mask, passes, K=1):
    """The packed accumulators [8][W*H] of `passes` passes of K sample streams under `mask`"""
    return Render(scene, seeds, passes, K).render(mask).packed


def layered_render(scene, seeds, table, passes, K=1):
    """(the unmasked packed accumulators [8][W*H], the layer accumulators (L, 3, W*H), seeds after the render, rays traced) of one
    render under the layer table `table`: every layer is the masked render of its mask, from the same traces."""
    r = Render(scene, seeds, passes, K)
    return r.render(None).packed, r.layers(table), r.seeds, r.rays


# ---- one drawn case on the device against the masked oracle (tests/test_gpu_masked_oracle.py, tools/fuzz_parity.py --masked) ----
RTOL, ATOL = 5e-5, 1e-8              # float atomics: the light-image tolerance of tests/test_gpu_strategies.py
NONFINITE_CAP = 1000                 # at most one pixel in 1000 is left out of a tolerance comparison for a non-finite addend


def draw_mask(rng):
    """every pair with probability 1/2"""
    return sum(S.bit(*p) for p in S.PAIRS if rng.rand() < 0.5)


def draw_table(rng):
    """eight layers: every pair goes to a random layer or to none"""
    assign = rng.randint(-1, S.MAX_LAYERS, size=len(S.PAIRS))
    return {f"l{l}": sum(S.bit(*p) for p, a in zip(S.PAIRS, assign) if a == l) for l in range(S.MAX_LAYERS)}


def draw_case(rng):
    """a mask, a layer table, K in {1, 2}, a traversal mode in 0..2, the reproducible switch"""
    return dict(mask=draw_mask(rng), table=draw_table(rng), K=int(rng.choice([1, 2])), mode=int(rng.randint(0, 3)),
                reproducible=bool(rng.rand() < 0.5))


def compare(got, want, exact, nonfinite=None, rtol=RTOL, atol=ATOL):
    """(problem or None, pixels left out): `got` against the reference `want`, both (rows, W*H) float32.  exact: the same bytes,
    NaNs canonicalised, every pixel.  Else |got - want| <= atol + rtol |want| on every pixel but those of `nonfinite` (bool[W*H]:
    a per-sample addend of the reference was not finite), of which there may be at most one in NONFINITE_CAP."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    if got.shape != want.shape:
        return f"shape {got.shape} instead of {want.shape}", 0
    if exact:
        if canonical(got) == canonical(want):
            return None, 0
        diff = np.frombuffer(canonical(got), np.uint32) != np.frombuffer(canonical(want), np.uint32)
        i = int(np.flatnonzero(diff)[0])
        return f"{int(diff.sum())} of {diff.size} words differ, first at {np.unravel_index(i, got.shape)}: " \
               f"{got.reshape(-1)[i]!r} instead of {want.reshape(-1)[i]!r}", 0
    keep = np.ones(got.shape[-1], bool) if nonfinite is None else ~np.asarray(nonfinite, bool).reshape(-1)
    left_out = int((~keep).sum())
    if left_out > keep.size // NONFINITE_CAP:
        return f"{left_out} of {keep.size} pixels have a non-finite addend: more than one in {NONFINITE_CAP}", left_out
    g, w = got[..., keep].astype(np.float64), want[..., keep].astype(np.float64)
    with np.errstate(all="ignore"):
        ok = np.abs(g - w) <= atol + rtol * np.abs(w)
    if np.all(ok):
        return None, left_out
    worst = float(np.nanmax(np.where(ok, 0.0, np.abs(g - w) / np.maximum(np.abs(w), 1e-300))))
    return f"{int((~ok).sum())} of {ok.size} values outside rtol {rtol} atol {atol}, worst relative error {worst:.3g}", left_out


def device_check(scene, seeds, case, passes, flags=0):
    """Render `case` (draw_case) on the device -- the masked render, then the layered render on the same handle -- and compare both
    with the masked oracle of the same passes: bytes under the reproducible switch, else at RTOL / ATOL.  `seeds`: (K, B, 2).
    Returns (the list of problems, the pixels left out of the tolerance comparisons)."""
    from clive2_amd.renderer import Renderer
    K, exact = case["K"], case["reproducible"]
    seeds = np.asarray(seeds, dtype=np.uint32).reshape(K, -1, 2)
    ref = Render(scene, seeds, passes, K)
    r = Renderer(scene, seeds=seeds if K > 1 else seeds[0], streams=K)
    problems, left_out = [], 0

    def chk(what, got, want, exact=exact, nonfinite=None):
        nonlocal left_out
        problem, n = compare(got, want, exact, nonfinite)
        left_out += n
        if problem:
            problems.append(f"{what}: {problem}")

    try:
        r.set_traversal_mode(case["mode"])
        if flags:
            r.set_debug_flags(flags)
        r.set_reproducible(exact)
        plain = ref.render(None)
        # the masked render
        want = ref.render(case["mask"])
        r.set_strategy_mask(case["mask"])
        r.reset_counters()
        r.run_samples(passes)
        chk("masked render", r.packed_accumulators().reshape(8, -1), want.packed, nonfinite=want.nonfinite | plain.nonfinite)
        chk("masked render: unidirectional rows, counts", r.packed_accumulators().reshape(8, -1)[4:], plain.packed[4:], True)
        if not np.array_equal(r.get_random_buffer().reshape(K, -1, 2), ref.seeds.reshape(K, -1, 2)):
            problems.append("masked render: RNG state")
        if r.counters()["rays"] != ref.rays:
            problems.append(f"masked render: {r.counters()['rays']} rays instead of {ref.rays}")
        # the layered render
        r.set_strategy_mask(None)
        r.set_layers(case["table"])
        r.reset_accumulators()
        r.set_seeds(seeds if K > 1 else seeds[0])
        r.reset_counters()
        r.run_samples(passes)
        lacc = r.layer_accumulators()
        for l, (name, m) in enumerate(case["table"].items()):
            want = ref.render(m)
            chk(f"layer {name} ({m:#x})", lacc[l], want.packed[:3], exact or not m & S.LIGHT_IMAGE,
                nonfinite=want.nonfinite | plain.nonfinite)
        chk("layered render: main rows", r.packed_accumulators().reshape(8, -1), plain.packed, nonfinite=plain.nonfinite)
        if not np.array_equal(r.get_random_buffer().reshape(K, -1, 2), ref.seeds.reshape(K, -1, 2)):
            problems.append("layered render: RNG state")
        if r.counters()["rays"] != ref.rays:
            problems.append(f"layered render: {r.counters()['rays']} rays instead of {ref.rays}")
    finally:
        r.close()
    return problems, left_out
