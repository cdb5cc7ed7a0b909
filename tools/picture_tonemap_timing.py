"""What the host detour of the derived pictures costs, and what the device tone map of a kept picture costs instead.

On one handle per frame size (Cornell box, 8 buckets, error tracking on, 4 passes, features rendered), wall time of

    robust_guided_image            cl2_denoise_robust, 12*W*H bytes to the host, camera.tone_map in float64 numpy
    tone_mapped("robust_guided")   cl2_keep_picture, cl2_picture_log_sum, cl2_picture_tone_map, 3*W*H bytes to the host

and the same pair for "denoised": the median of 5 runs after one warm-up, and the bytes copied.  Reported, not asserted.

    python tools/picture_tonemap_timing.py [--out profiles/picture_tonemap_timing.json]
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

SIZES = ((1920, 1080), (3840, 2160))
PAIRS = (("robust_guided", "robust_guided_image"), ("denoised", "denoised_image"))
REPS = 5


def _median_ms(call):
    call()                                            # warm-up: first-use allocations
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 3), round(min(t), 3)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)
    import clive2_amd as c2
    from clive2_amd.renderer import Renderer
    out = {"what": "host clock around the call, median (and min) of 5 runs after one warm-up; Cornell box, 8 buckets, error tracking on, "
                   "4 passes, 4 feature rays per pixel; numpy " + np.__version__, "runs": []}
    for W, H in SIZES:
        r = Renderer(c2.create_scene_from_preset("empty", W, H))
        r.set_error_tracking(True)
        r.set_robust_buckets(8)
        r.run_samples(4)
        r.render_features(4)
        run = {"width": W, "height": H, "host_bytes_copied": 12 * W * H, "device_bytes_copied": 3 * W * H}
        for kind, prop in PAIRS:
            with np.errstate(all="ignore"):
                host = _median_ms(lambda: getattr(r, prop))
            dev = _median_ms(lambda: r.tone_mapped(kind))
            with np.errstate(all="ignore"):
                differing = int((getattr(r, prop) != r.tone_mapped(kind)).sum())
            run[kind] = {"host_median_ms": host[0], "host_min_ms": host[1], "device_median_ms": dev[0], "device_min_ms": dev[1],
                         "bytes_differing": differing}
            print(f"{W}x{H} {kind}: host {host[0]} ms, device {dev[0]} ms, {differing} bytes differ", flush=True)
        out["runs"].append(run)
        r.close()
    text = "{" + json.dumps({"what": out["what"]})[1:-1] + ',\n "runs": [\n' + ",\n".join("  " + json.dumps(x) for x in out["runs"]) + "\n ]}"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
