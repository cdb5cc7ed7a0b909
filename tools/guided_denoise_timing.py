"""Cost of the variance-guided filter (csrc/denoise_guided.hpp) next to the fixed one (csrc/denoise.hpp), both on the same handle:
the Cornell box at 1920x1080 and 3840x2160, 4 samples, error tracking on.  Prints one JSON object.

    python tools/guided_denoise_timing.py [--reps 10] [--out host.json]
    rocprofv3 --kernel-trace --stats -f csv -d <dir> -o guided -- python tools/guided_denoise_timing.py --reps 10
    python tools/guided_denoise_timing.py --kernel-trace <dir>/.../guided_kernel_trace.csv --host host.json \
        --out profiles/guided_denoise_timing.json

Host times: clocks around synchronised calls after a warm-up (each call = its launches + the copy of the (H, W, 3) float32
picture to the host; `*_input_and_copy` is the same call with iterations=0, so the difference is what the passes cost).  The
profiler slows the host, so the host times come from a run without it.  Kernel times: per kernel instantiation and frame from
the profiler's kernel trace; the fixed filter's passes are the yardstick, re-measured in the same run, and `ratio_to_twin` is
guided pass / fixed pass of the same LDS_STEP.
"""
import argparse
import collections
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FRAMES = ((1920, 1080), (3840, 2160))


def _clock(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                  # every library call returns after its device work has drained
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "reps": reps}


def host_times(reps, samples):
    import clive2_amd as c2
    from clive2_amd.renderer import Renderer
    out = {"what": "fixed and variance-guided denoiser on one handle: host clock around synchronised calls, median over reps "
                   "after one warm-up call", "guided_defaults": dict(Renderer.GUIDED_DEFAULTS),
           "fixed_defaults": dict(Renderer.DENOISE_DEFAULTS), "runs": []}
    for W, H in FRAMES:
        r = Renderer(c2.create_scene_from_preset("empty", W, H))
        r.set_error_tracking(True)
        r.run_samples(samples)
        r.render_features(4)
        calls = collections.OrderedDict([
            ("fixed_3_passes", lambda: r.denoised_radiance(iterations=3)),
            ("fixed_5_passes", lambda: r.denoised_radiance(iterations=5)),
            ("fixed_input_and_copy", lambda: r.denoised_radiance(iterations=0)),
            ("guided_3_passes", lambda: r.guided_radiance(iterations=3)),
            ("guided_5_passes", lambda: r.guided_radiance(iterations=5)),
            ("guided_defaults", lambda: r.guided_radiance()),
            ("guided_defaults_with_variance", lambda: r.guided_radiance(return_variance=True)),
            ("guided_input_and_copy", lambda: r.guided_radiance(iterations=0))])
        run = {"scene": "cornell", "width": W, "height": H, "output_mb": round(W * H * 12 / 1e6, 1)}
        for name, fn in calls.items():
            fn()
            run[name] = _clock(fn, reps)
        out["runs"].append(run)
        r.close()
    return out


def _frame(name, gx, gy):
    if "_pass" in name:
        return {(1920, 1088): "1080p", (3840, 2160): "2160p"}.get((gx, gy), f"{gx}x{gy}")
    for lab, (W, H) in zip(("1080p", "2160p"), FRAMES):
        if abs(gx * gy - W * H) < 256:
            return lab
    return f"{gx}x{gy}"


def kernel_times(path):
    """{kernel: {frame: {calls, average_us, min_us, max_us}}} of the denoiser kernels in a rocprofv3 kernel trace"""
    agg = collections.OrderedDict()
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            m = re.search(r"(k_denoise\w*(?:<\d+>)?)", name)
            if not m:
                continue
            dur = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            fr = _frame(m.group(1), int(row["Grid_Size_X"]), int(row["Grid_Size_Y"]))
            a = agg.setdefault(m.group(1), collections.OrderedDict()).setdefault(
                fr, {"calls": 0, "total_us": 0.0, "min_us": 1e18, "max_us": 0.0})
            a["calls"] += 1
            a["total_us"] += dur
            a["min_us"] = min(a["min_us"], dur)
            a["max_us"] = max(a["max_us"], dur)
    for frames in agg.values():
        for a in frames.values():
            a["average_us"] = round(a.pop("total_us") / a["calls"], 2)
            a["min_us"], a["max_us"] = round(a["min_us"], 2), round(a["max_us"], 2)
    ratios = collections.OrderedDict()
    for k in ("<1>", "<2>", "<0>"):
        g, t = agg.get("k_denoise_guided_pass" + k), agg.get("k_denoise_pass" + k)
        if g and t:
            ratios["pass" + k] = {fr: round(g[fr]["average_us"] / t[fr]["average_us"], 3) for fr in g if fr in t}
    return {"kernels": agg, "ratio_to_twin": ratios}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=4, help="render samples before the filters (their input)")
    ap.add_argument("--kernel-trace", default=None, help="summarise this rocprofv3 kernel trace (csv) instead of running")
    ap.add_argument("--host", default=None, help="with --kernel-trace: the JSON of a run without the profiler, merged in")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.kernel_trace:
        out = json.load(open(args.host)) if args.host else {}
        out.update(kernel_times(args.kernel_trace))
    else:
        out = host_times(args.reps, args.samples)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
