"""Cost of the denoiser (csrc/denoise.hpp): host clocks around synchronised calls, after a warm-up, for
render_features(4) and denoised_radiance() (default filter: 3 passes) on the Cornell box at 1920x1080 and 3840x2160 and
on the 1M-triangle interior at 1920x1080.  Prints one JSON object.

    python tools/denoise_timing.py [--reps 10] [--out profiles/denoise_timing.json]

denoised_radiance() = the filter's launches + the copy of the (H, W, 3) float32 picture to the host (25 MB at 1080p);
`input_and_copy_ms` times the same call with iterations=0 (the input kernel and the copy alone), so the difference is what
the passes cost.  The kernels alone: run this under `rocprofv3 --kernel-trace --stats`.
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


def _scene(name, W, H):
    import clive2_amd as c2
    if name == "cornell":
        return c2.create_scene_from_preset("empty", W, H)
    from clive2_amd import meshes
    from clive2_amd.load import get_materials
    mats = get_materials()
    mats["alpha"][5] = 0.1
    specs = [dict(mesh=(v, f), material=m) for v, f, m in meshes.interior_grid()]
    return c2.create_scene(W, H, np.array([0, 1.5, 6]), np.array([0, 0, -1]), file_specs=specs, materials=mats)


def _clock(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                  # every library call returns after its device work has drained
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "reps": reps}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=4, help="render samples before the filter (its input)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from clive2_amd.renderer import Renderer
    out = {"what": "denoiser cost: host clock around synchronised calls, median over reps after one warm-up call", "runs": []}
    for name, W, H in (("cornell", 1920, 1080), ("cornell", 3840, 2160), ("interior", 1920, 1080)):
        scene = _scene(name, W, H)
        r = Renderer(scene)
        r.run_samples(args.samples)
        r.render_features(4)
        r.denoised_radiance()
        r.denoised_radiance(iterations=0)
        run = {"scene": name, "width": W, "height": H, "triangles": int(len(scene.triangles)),
               "render_features_4": _clock(lambda: r.render_features(4), args.reps),
               "denoised_radiance": _clock(r.denoised_radiance, args.reps),
               "input_and_copy_ms": _clock(lambda: r.denoised_radiance(iterations=0), args.reps),
               "output_mb": round(W * H * 12 / 1e6, 1)}
        out["runs"].append(run)
        r.close()
        del scene
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
