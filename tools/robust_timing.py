"""Cost of the robust buckets (csrc/robust.hpp) on the Cornell box at 1920 x 1080: host clocks around synchronised
calls, after a warm-up, for run_samples(N) with buckets off and with M = 8 and 16, and for robust_radiance().  Prints one JSON
object.

    python tools/robust_timing.py [--reps 5] [--samples 32] [--out profiles/robust_timing.json]

robust_radiance() = k_robust_picture + the copy of the (H, W, 3) float32 picture to the host (25 MB at 1080p).  The kernels alone
(the accumulate kernel with and without the hook, k_robust_picture), one profiled run per M so that the rows do not mix:

    rocprofv3 --kernel-trace --stats -f csv -d <dir8> -o rb -- python tools/robust_timing.py --buckets 0 8
    rocprofv3 --kernel-trace --stats -f csv -d <dir16> -o rb -- python tools/robust_timing.py --buckets 16
    python tools/robust_timing.py --kernel-stats 8=<dir8>/.../rb_kernel_stats.csv 16=<dir16>/.../rb_kernel_stats.csv --host host.json \
        --out profiles/robust_timing.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _clock(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                  # every library call returns after its device work has drained
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "reps": reps}


def kernel_times(path):
    """{short kernel name: {calls, average_us}} of the accumulate kernels and k_robust_picture in a rocprofv3 kernel_stats.csv"""
    import csv
    out = {}
    for row in csv.DictReader(open(path)):
        name = row["Name"]
        for k in ("k_finalize_accumulate", "k_accumulate", "k_robust_picture"):
            if "cl2::" + k + "<" in name or "cl2::" + k + "(" in name:
                short = name.split("cl2::", 1)[1].split("(", 1)[0].replace(" ", "")
                out[short] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3}
    return out


def _dump(out):
    """the result as JSON, one run per line"""
    head = {k: v for k, v in out.items() if k not in ("runs", "kernels")}
    lines = ["{" + json.dumps(head)[1:-1] + ("," if head else ""), ' "runs": [']
    lines += ["  " + json.dumps(r) + ("," if i + 1 < len(out["runs"]) else "") for i, r in enumerate(out.get("runs", []))]
    lines.append(" ]" + (', "kernels": ' + json.dumps(out["kernels"]) if "kernels" in out else "") + "}")
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--buckets", type=int, nargs="+", default=[0, 8, 16], help="the bucket counts to time (0 = off)")
    ap.add_argument("--kernel-stats", nargs="+", default=None, metavar="M=CSV",
                    help="summarise these rocprofv3 kernel_stats.csv files (one per profiled run) instead of running")
    ap.add_argument("--host", default=None, help="with --kernel-stats: the JSON of a run without the profiler, merged in")
    args = ap.parse_args(argv)
    if args.kernel_stats:
        out = json.load(open(args.host)) if args.host else {}
        out["kernels"] = {"what": "rocprofv3 --kernel-trace --stats, one run of this tool per key (its --buckets); average over the run's launches",
                          **{m: kernel_times(path) for m, path in (a.split("=", 1) for a in args.kernel_stats)}}
        text = _dump(out)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return 0
    import clive2_amd as c2
    from clive2_amd.renderer import Renderer
    W, H = 1920, 1080
    scene = c2.create_scene_from_preset("empty", W, H)
    out = {"what": "robust buckets: host clock around synchronised calls, median over reps after one warm-up call", "width": W,
           "height": H, "samples_per_call": args.samples, "runs": []}
    for M in args.buckets:
        r = Renderer(scene)
        if M:
            r.set_robust_buckets(M)
        r.run_samples(args.samples)
        run = {"buckets": M, "run_samples": _clock(lambda: r.run_samples(args.samples), args.reps)}
        run["ms_per_sample"] = run["run_samples"]["median_ms"] / args.samples
        if M:
            r.robust_radiance()
            run["robust_radiance"] = _clock(r.robust_radiance, args.reps)
            run["robust_radiance_with_stats"] = _clock(lambda: r.robust_radiance(return_stats=True), args.reps)
        out["runs"].append(run)
        r.close()
    text = _dump(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
