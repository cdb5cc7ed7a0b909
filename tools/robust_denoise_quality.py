"""Quality and cost of the guided filter on the robust picture (csrc/denoise_robust.hpp).

Quality (the default): Cornell box and glass scene at 256 x 192, M buckets, at 4, 16, 64 and 256 passes; relative MSE (`_rmse` of
tests/test_gpu_denoise.py) against a 1024-pass picture of seed 4321 of `radiance`, `robust_radiance()`, `guided_radiance()` at its
defaults and `robust_guided_radiance()` at its defaults, and a sweep of the latter over iterations 3..5 x sigma_luma 1, 2, 4, 8, 16
-- the figures behind Renderer.ROBUST_GUIDED_DEFAULTS and tests/test_gpu_robust_denoise.py::test_quality_on_real_renders.

    python tools/robust_denoise_quality.py [--buckets 8] [--out profiles/robust_denoise_quality_mi355x.json]

Cost (--timing): the Cornell box at 1920 x 1080, M = 8, 8 passes; host clocks around synchronised calls after a warm-up, beside
guided_radiance() and robust_radiance() on the same handle.  The profiler slows the host, so the host times come from a run
without it and the kernel times from one run under it:

    python tools/robust_denoise_quality.py --timing --out host.json
    rocprofv3 --kernel-trace --stats -f csv -d <dir> -o rd -- python tools/robust_denoise_quality.py --timing
    python tools/robust_denoise_quality.py --kernel-stats <dir>/.../rd_kernel_stats.csv --host host.json \
        --out profiles/robust_denoise_timing.json
"""
import argparse
import collections
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PASSES = (4, 16, 64, 256)
ITERATIONS = (3, 4, 5)
SIGMAS = (1.0, 2.0, 4.0, 8.0, 16.0)


def _rmse(x, ref):                                   # tests/test_gpu_denoise.py
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2)))


def _dump(out):
    """the result as JSON, one run per line"""
    head = {k: v for k, v in out.items() if k not in ("runs", "kernels")}
    lines = ["{" + json.dumps(head)[1:-1] + ("," if head else ""), ' "runs": [']
    lines += ["  " + json.dumps(r) + ("," if i + 1 < len(out["runs"]) else "") for i, r in enumerate(out.get("runs", []))]
    lines.append(" ]" + (', "kernels": ' + json.dumps(out["kernels"]) if "kernels" in out else "") + "}")
    return "\n".join(lines)


def quality(M):
    from clive2_amd.renderer import Renderer, make_seeds
    from denoise_scenes import cornell, glass
    W, H = 256, 192
    out = {"what": "relative MSE against 1024 passes of seed 4321, 256 x 192; default seeds for the render; sweep[iterations][sigma_luma] "
                   "of robust_guided_radiance, the other arguments at their defaults", "buckets": M,
           "guided_defaults": dict(Renderer.GUIDED_DEFAULTS), "robust_guided_defaults": dict(Renderer.ROBUST_GUIDED_DEFAULTS), "runs": []}
    for name, make in (("cornell", cornell), ("glass", glass)):
        scene = make(W, H)
        ref_r = Renderer(scene, seeds=make_seeds(W * H, seed=4321))
        ref_r.run_samples(1024)
        ref = ref_r.radiance
        ref_r.close()
        r = Renderer(scene)
        r.set_error_tracking(True)                    # for the guided column
        r.set_robust_buckets(M)
        r.render_features(4)
        for n in PASSES:
            r.run_samples(n - r.samples)
            pic, st = r.robust_radiance(return_stats=True)
            run = {"scene": name, "passes": n, "rmse_raw": _rmse(r.radiance, ref), "rmse_robust": _rmse(pic, ref),
                   "rmse_guided": _rmse(r.guided_radiance(), ref), "rmse_new": _rmse(r.robust_guided_radiance(), ref)}
            run["new_over_guided"] = run["rmse_new"] / run["rmse_guided"]
            run["new_over_robust"] = run["rmse_new"] / run["rmse_robust"]
            run["trimmed_pixel_share"] = float((st[..., 1] > 0).mean())
            run["sweep"] = {str(it): {f"{sl:g}": _rmse(r.robust_guided_radiance(iterations=it, sigma_luma=sl), ref) for sl in SIGMAS}
                            for it in ITERATIONS}
            out["runs"].append(run)
        r.close()
    return out


def _clock(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                  # every library call returns after its device work has drained
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "reps": reps}


def timing(M, reps):
    import clive2_amd as c2
    from clive2_amd.renderer import Renderer
    W, H = 1920, 1080
    r = Renderer(c2.create_scene_from_preset("empty", W, H))
    r.set_error_tracking(True)
    r.set_robust_buckets(M)
    r.run_samples(8)
    r.render_features(4)
    calls = collections.OrderedDict([
        ("robust_guided_defaults", lambda: r.robust_guided_radiance()),
        ("robust_guided_defaults_with_variance", lambda: r.robust_guided_radiance(return_variance=True)),
        ("robust_guided_3_passes", lambda: r.robust_guided_radiance(iterations=3)),
        ("robust_guided_input_and_copy", lambda: r.robust_guided_radiance(iterations=0)),
        ("guided_defaults", lambda: r.guided_radiance()),
        ("guided_input_and_copy", lambda: r.guided_radiance(iterations=0)),
        ("robust_radiance", lambda: r.robust_radiance())])
    run = {"scene": "cornell", "width": W, "height": H, "buckets": M, "output_mb": round(W * H * 12 / 1e6, 1)}
    for name, fn in calls.items():
        fn()
        run[name] = _clock(fn, reps)
    r.close()
    return {"what": "cl2_denoise_robust beside cl2_denoise_guided and cl2_robust_picture on one handle: host clock around synchronised "
                    "calls, median over reps after one warm-up call", "robust_guided_defaults": dict(Renderer.ROBUST_GUIDED_DEFAULTS),
            "runs": [run]}


def kernel_times(path):
    """{kernel: {calls, average_us, min_us}} of the filter's kernels and k_robust_picture in a rocprofv3 kernel_stats.csv"""
    out = collections.OrderedDict()
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            if "cl2::k_denoise" in name or "cl2::k_robust_picture" in name:
                short = name.split("cl2::", 1)[1].split("(", 1)[0].replace(" ", "")
                out[short] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                              "min_us": round(float(row["MinNs"]) / 1e3, 2)}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--buckets", type=int, default=8)
    ap.add_argument("--timing", action="store_true", help="time the calls at 1920 x 1080 instead of measuring the quality")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kernel-stats", default=None, metavar="CSV",
                    help="summarise this rocprofv3 kernel_stats.csv of a --timing run instead of running")
    ap.add_argument("--host", default=None, help="with --kernel-stats: the JSON of a --timing run without the profiler, merged in")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.kernel_stats:
        out = json.load(open(args.host)) if args.host else {"runs": []}
        out["kernels"] = {"what": "rocprofv3 --kernel-trace --stats of one --timing run, no counters; average over the run's launches",
                          **kernel_times(args.kernel_stats)}
    elif args.timing:
        out = timing(args.buckets, args.reps)
    else:
        out = quality(args.buckets)
    text = _dump(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
