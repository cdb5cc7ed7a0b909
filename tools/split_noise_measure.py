"""Measurements behind the split noise model (csrc/error_split.hpp).  Each part prints one JSON object.

    python tools/split_noise_measure.py full   [--out profiles/split_noise_full.json]   [--truth-samples 16384]
    python tools/split_noise_measure.py small  [--out profiles/split_noise_small.json]
    python tools/split_noise_measure.py cost   [--out profiles/split_noise_cost.json]   [--root OTHER_CHECKOUT]

full    6.15's table again with the split model beside the pure ones: the Cornell box at 1920 x 1080, one handle, 10 / 34 / 130
        passes, the fixed and the guided filter at their defaults, one probe; every term of the estimate in units of the true summed
        squared luma error of the filtered picture against a render of --truth-samples samples with other seeds; the frame's light
        share; one row of the glass scene (34 passes, fixed filter).
small   6.15's 64 x 48 calibration with a split column: 24 renders of 32 samples, truth 16,384 samples, both scenes and filters.
cost    Cornell box at 1920 x 1080, one stream: run_samples(64) after a warm-up, five runs, ms per pass with error tracking alone
        and with split tracking; denoised_error (3 passes, one probe) under the correlated and the split model on the same handle.
        --root: import the package of another checkout (the parent commit's build) and time error tracking alone there.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUMA = np.array([0.0722, 0.7152, 0.2126], np.float32).astype(np.float64)
MODELS = ("independent", "correlated", "split")
KINDS = ("denoised", "guided")


def luma64(c):
    c = np.asarray(c, np.float32).astype(np.float64)
    return (c[..., 0] * LUMA[0] + c[..., 1] * LUMA[1]) + c[..., 2] * LUMA[2]


def _scene(name, W, H):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import denoise_scenes as ds
    return ds.cornell(W, H) if name == "cornell" else ds.glass(W, H)


def _truth(scene, samples, streams=4):
    """luma of a render of `samples` samples with seeds of its own"""
    from clive2_amd.renderer import Renderer, stream_seeds
    t = Renderer(scene, streams=streams)
    t.set_seeds(stream_seeds(t.batch_size, streams, seed=4321))
    t.run_samples(samples // streams)
    mu = luma64(t.radiance)
    t.close()
    return mu


def _state2(r):
    H, W = r.pixel_height, r.pixel_width
    acc = r.packed_accumulators().reshape(8, H, W)
    return (acc[3] > 0) & np.isfinite(acc[3]) & (acc[7] >= 2)


def _rows(r, mu, passes, kinds, seed=0):
    """one row per filter: the totals of the three models in units of the truth"""
    rows = []
    ok = _state2(r)
    for kind in kinds:
        tot = {}
        for m in MODELS:
            _, out, (_, Fy, _) = r.denoised_error(kind, noise=m, seed=seed, return_totals=True, return_probe=True)
            tot[m] = out
        truth = float(((luma64(Fy) - mu) ** 2)[ok].sum())
        row = {"passes": passes, "filter": kind, "truth": truth, "fidelity": tot["split"][5] / truth, "sum_v": tot["split"][6] / truth,
               "two_div": {m: tot[m][7] / truth for m in MODELS}, "R": {m: tot[m][4] / truth for m in MODELS},
               "e_dn": {m: tot[m][0] for m in MODELS},
               "two_div_needed": (truth - tot["split"][5] + tot["split"][6]) / truth}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    return rows


def full(truth_samples=16384):
    from clive2_amd.renderer import Renderer
    W, H = 1920, 1080
    out = {"what": "1920 x 1080, default seeds, one probe; every term in units of the true summed squared luma error of the filtered "
                   "picture (pixels with an estimate) against a render of truth_samples samples", "truth_samples": truth_samples,
           "runs": []}
    for name, steps, kinds in (("cornell", (10, 34, 130), KINDS), ("glass", (34,), ("denoised",))):
        scene = _scene(name, W, H)
        mu = _truth(scene, truth_samples)
        r = Renderer(scene)
        r.set_split_tracking(True)
        r.render_features(4)
        run = {"scene": name, "rows": [], "light_share": {}}
        for n in steps:
            r.run_samples(n - r.samples)
            run["light_share"][str(n)] = r.light_share()
            run["rows"] += _rows(r, mu, n, kinds)
        share, rho = r.light_share(return_map=True)
        run["rho_quartiles"] = np.percentile(rho[_state2(r)], [5, 25, 50, 75, 95]).round(4).tolist()
        r.close()
        out["runs"].append(run)
    return out


def small(renders=24, truth_samples=16384):
    from clive2_amd.renderer import Renderer, make_seeds
    W, H = 64, 48
    out = {"what": "64 x 48, 24 renders of 32 samples, features from 4 rays, one probe: R = mean out[4] / mean true summed squared "
                   "luma error over the pixels with an estimate", "runs": []}
    for name in ("cornell", "glass"):
        scene = _scene(name, W, H)
        t = Renderer(scene, seeds=make_seeds(W * H, seed=4321))
        t.run_samples(truth_samples)
        mu = luma64(t.radiance)
        t.close()
        est = {(k, m): [] for k in KINDS for m in MODELS}
        true = {k: [] for k in KINDS}
        shares = []
        for i in range(renders):
            r = Renderer(scene, seeds=make_seeds(W * H, seed=1000 + i))
            r.set_split_tracking(True)
            r.run_samples(32)
            r.render_features(4)
            ok = _state2(r)
            shares.append(r.light_share())
            for k in KINDS:
                for m in MODELS:
                    _, o, (_, Fy, _) = r.denoised_error(k, noise=m, seed=i, return_totals=True, return_probe=True)
                    est[(k, m)].append(o[4])
                true[k].append(float(((luma64(Fy) - mu) ** 2)[ok].sum()))
            r.close()
        run = {"scene": name, "light_share": float(np.mean(shares)),
               "R": {k: {m: float(np.mean(est[(k, m)]) / np.mean(true[k])) for m in MODELS} for k in KINDS}}
        out["runs"].append(run)
        print(json.dumps(run), file=sys.stderr)
    return out


def _passes(r, n=64, runs=5):
    r.run_samples(n)                                  # warm-up: tuning, allocation
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        r.run_samples(n)                              # returns after the device work has drained
        ts.append((time.perf_counter() - t0) * 1e3 / n)
    return {"median_ms_per_pass": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts)), "runs": runs, "passes": n}


def _clock(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts)), "reps": reps}


def cost(other_root=None):
    out = {"what": "Cornell box 1920 x 1080, one stream, run_samples(64) after a warm-up, five runs, host clock"}
    if other_root:
        # the other checkout's package: nothing of this one is imported before it
        sys.path.insert(0, os.path.abspath(other_root))
        from clive2_amd.renderer import Renderer
        scene = _scene("cornell", 1920, 1080)
        r = Renderer(scene)
        r.set_error_tracking(True)
        out["other_checkout_error_tracking"] = _passes(r)
        out["other_checkout_error_tracking_again"] = _passes(r)
        r.close()
        return out
    from clive2_amd.renderer import Renderer
    scene = _scene("cornell", 1920, 1080)
    r = Renderer(scene)
    out["plain"] = _passes(r)
    r.close()
    r = Renderer(scene)
    r.set_error_tracking(True)
    out["error_tracking"] = _passes(r)
    out["error_tracking_again"] = _passes(r)          # the noise floor: the same state twice
    r.close()
    r = Renderer(scene)
    r.set_split_tracking(True)
    out["split_tracking"] = _passes(r)
    out["split_tracking_again"] = _passes(r)
    r.render_features(4)
    for m in MODELS:
        out["denoised_error_" + m] = _clock(lambda: r.denoised_error(iterations=3, probes=1, noise=m))
    out["light_share"] = _clock(r.light_share)
    r.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=("full", "small", "cost"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--truth-samples", type=int, default=16384)
    ap.add_argument("--root", default=None)
    args = ap.parse_args(argv)
    if args.root is None and ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    res = {"full": lambda: full(args.truth_samples), "small": small, "cost": lambda: cost(args.root)}[args.part]()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
