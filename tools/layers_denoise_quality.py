"""Quality and cost of the filter over the layers of one render (csrc/denoise_layers.hpp).

Quality (the default): Cornell box and glass scene at 256 x 192, 4 passes under strategies.LAYERS, features of 4 samples; relative
MSE (`_rmse` of tests/test_gpu_denoise.py) against a 1024-pass picture of seed 4321 of `radiance`, of `denoised_radiance()` at its
defaults, of the layered sum with DENOISE_DEFAULTS' sigma_color on every layer, of the layered sum at LAYER_DENOISE_DEFAULTS, and a
sweep of the layered sum over sigma_color in SIGMAS for each of the three layers (343 combinations), beside the same sweep of `denoised_radiance()` -- the figures behind
Renderer.LAYER_DENOISE_DEFAULTS.

    python tools/layers_denoise_quality.py [--out profiles/r22_layers_denoise_quality.json]

Cost (--timing): the Cornell box at 1920 x 1080, 20 passes, features rendered, 3 iterations, for L = 3 (strategies.LAYERS) and
L = 8 (path lengths); host clocks around synchronised calls, the variants alternating, `--reps` rounds after one warm-up round:

    layered            cl2_denoise_layers, layer pictures copied out (out_sum NULL)
    layered_with_sum   ... and the sum
    layered_kept       cl2_keep_layer_picture(-1): the same launches and the sum, nothing copied out
    write_and_denoise  L x (cl2_write_accumulators_packed + cl2_denoise) on a second handle: the only way without the call
    bare               L x cl2_denoise on L prepared handles (one per layer)
    bare_kept          L x cl2_keep_picture(denoised) on those handles: nothing copied out

    python tools/layers_denoise_quality.py --timing [--out profiles/r22_layers_denoise_timing.json]
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIGMAS = (0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0)


def _rmse(x, ref):                                   # tests/test_gpu_denoise.py
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2)))


def quality():
    from clive2_amd import strategies
    from clive2_amd.renderer import Renderer, make_seeds
    from denoise_scenes import cornell, glass
    W, H = 256, 192
    names = list(strategies.LAYERS)
    out = {"what": "relative MSE against 1024 passes of seed 4321, 256 x 192, 4 passes from the default seeds; sweep: sigma_color of "
                   + " / ".join(names) + " -> relative MSE of the layered sum, the other arguments at their defaults",
           "denoise_defaults": dict(Renderer.DENOISE_DEFAULTS), "layer_denoise_defaults": dict(Renderer.LAYER_DENOISE_DEFAULTS),
           "runs": []}
    for name, make in (("cornell", cornell), ("glass", glass)):
        scene = make(W, H)
        ref_r = Renderer(scene, seeds=make_seeds(W * H, seed=4321))
        ref_r.run_samples(1024)
        ref = ref_r.radiance
        ref_r.close()
        r = Renderer(scene)
        r.set_layers(strategies.LAYERS)
        r.run_samples(4)
        r.render_features(4)
        same = Renderer.DENOISE_DEFAULTS["sigma_color"]
        raw_layers = r.denoised_layers(iterations=0)[0]
        run = {"scene": name, "rmse_raw": _rmse(r.radiance, ref), "rmse_denoised": _rmse(r.denoised_radiance(), ref),
               "rmse_layered_same_sigma": _rmse(r.denoised_layers(sigma_color=same)[1], ref),
               "rmse_layered_defaults": _rmse(r.denoised_layers()[1], ref),
               "rmse_sum_of_raw_layers": _rmse(r.denoised_layers(iterations=0)[1], ref),
               "mean_of_raw_layers": {n: float(raw_layers[n].mean()) for n in names}}
        run["sweep"] = {"/".join(f"{s:g}" for s in sig): _rmse(r.denoised_layers(sigma_color=dict(zip(names, sig)))[1], ref)
                        for sig in itertools.product(SIGMAS, repeat=len(names))}
        run["sweep_denoised"] = {f"{s:g}": _rmse(r.denoised_radiance(sigma_color=s), ref) for s in SIGMAS}
        best = min(run["sweep"], key=run["sweep"].get)
        run["best"] = {"sigma_color": best, "rmse": run["sweep"][best]}
        out["runs"].append(run)
        r.close()
    # the combination that is best for both scenes together: smallest product of the two ratios to the same-sigma sum
    a, b = out["runs"]
    score = {k: (a["sweep"][k] / a["rmse_layered_same_sigma"]) * (b["sweep"][k] / b["rmse_layered_same_sigma"]) for k in a["sweep"]}
    k = min(score, key=score.get)
    out["best_for_both"] = {"sigma_color": k, "ratio_cornell": a["sweep"][k] / a["rmse_layered_same_sigma"],
                            "ratio_glass": b["sweep"][k] / b["rmse_layered_same_sigma"]}
    return out


def timing(reps):
    import ctypes as C
    import clive2_amd as c2
    from clive2_amd import strategies as S
    from clive2_amd._native import ptr
    from clive2_amd.renderer import Renderer
    W, H, IT = 1920, 1080, 3
    FB = W * H
    tables = {3: dict(S.LAYERS), 8: dict([(f"k{k}", S.path_length(k, k)) for k in range(1, 8)] + [("k8+", S.path_length(8))])}
    scene = c2.create_scene_from_preset("empty", W, H)
    d = Renderer.DENOISE_DEFAULTS
    sc, sd, sa = d["sigma_color"], d["sigma_depth"], d["sigma_albedo"]
    out = {"what": "1080p Cornell box, 20 passes, 3 iterations, sigma_color 2 on every layer: wall ms of synchronised calls, the "
                   "variants alternating, one warm-up round, then `reps` rounds", "reps": reps, "runs": []}
    for L, table in tables.items():
        r = Renderer(scene)
        r.tune()
        r.set_layers(table)
        r.reset_accumulators()                                            # tune() rendered without the table
        r.run_samples(20)
        r.render_features(4)
        feats = r.features()
        acc, lacc = r.packed_accumulators().reshape(8, -1), r.layer_accumulators()
        twins = []
        for l in range(L):
            t = Renderer(scene)
            t.load_features(**feats)
            a = acc.copy()
            a[:3] = lacc[l]
            t.load_packed_accumulators(a)
            twins.append((t, a))
        w = twins[0][0]                                                   # the handle of write_and_denoise
        sig = np.full(L, sc, np.float32)
        lay, tot, one = np.empty((L, H, W, 3), np.float32), np.empty((H, W, 3), np.float32), np.empty((H, W, 3), np.float32)
        lib, n3 = r._L, C.c_size_t(3 * FB)

        def ok(rc):
            assert rc == 0, rc

        def write_and_denoise():
            for _, a in twins:
                ok(lib.cl2_write_accumulators_packed(w._h, ptr(a), C.c_size_t(a.size)))
                ok(lib.cl2_denoise(w._h, IT, sc, sd, sa, ptr(one), n3))

        def bare():
            for t, _ in twins:
                ok(lib.cl2_denoise(t._h, IT, sc, sd, sa, ptr(one), n3))

        def bare_kept():
            for t, _ in twins:
                ok(lib.cl2_keep_picture(t._h, 1, IT, sc, sd, sa))

        variants = {
            "layered": lambda: ok(lib.cl2_denoise_layers(r._h, IT, ptr(sig), sd, sa, ptr(lay), C.c_size_t(lay.size), None, C.c_size_t(0))),
            "layered_with_sum": lambda: ok(lib.cl2_denoise_layers(r._h, IT, ptr(sig), sd, sa, ptr(lay), C.c_size_t(lay.size), ptr(tot), n3)),
            "layered_kept": lambda: ok(lib.cl2_keep_layer_picture(r._h, -1, IT, ptr(sig), sd, sa)),
            "write_and_denoise": write_and_denoise, "bare": bare, "bare_kept": bare_kept}
        ms = {k: [] for k in variants}
        for rep in range(reps + 1):
            for k, fn in variants.items():
                t0 = time.perf_counter()
                fn()
                if rep:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
        # the bare calls were left with the last layer on handle `w`: the layered pictures must be the bare ones
        bare()
        same = all(np.array_equal(lay[l], t.denoised_radiance(iterations=IT), equal_nan=True) for l, (t, _) in enumerate(twins[1:], 1))
        run = {"layers": L, "layered_equals_bare": bool(same), "ms": {k: [round(x, 3) for x in v] for k, v in ms.items()},
               "median_ms": {k: round(float(np.median(v)), 3) for k, v in ms.items()}}
        m = run["median_ms"]
        run["bare_over_layered"] = round(m["bare"] / m["layered"], 3)
        run["bare_kept_over_layered_kept"] = round(m["bare_kept"] / m["layered_kept"], 3)
        run["write_and_denoise_over_layered"] = round(m["write_and_denoise"] / m["layered"], 3)
        out["runs"].append(run)
        for t, _ in twins:
            t.close()
        r.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--timing", action="store_true", help="time the calls at 1920 x 1080 instead of measuring the quality")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    out = timing(args.reps) if args.timing else quality()
    if not args.timing:
        # the stored form of the sweep: a 7 x 7 x 7 array in the order of SIGMAS, six digits
        S = [f"{s:g}" for s in SIGMAS]
        out["sweep_axes"] = "sweep[i][j][k]: sigma_color of emission / direct / indirect = SIGMAS[i], [j], [k]; SIGMAS = " + ", ".join(S)
        for run in out["runs"]:
            run["sweep"] = [[[float(f"{run['sweep'][f'{a}/{b}/{c}']:.6g}") for c in S] for b in S] for a in S]
    head = {k: v for k, v in out.items() if k != "runs"}
    text = "{" + json.dumps(head)[1:-1] + ', "runs": [\n' + ",\n".join(" " + json.dumps(r) for r in out["runs"]) + "\n]}"      # a run per line
    print(json.dumps(head | {"runs": [{k: v for k, v in run.items() if k != "sweep"} for run in out["runs"]]}, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
