"""The sweep behind Renderer.GUIDED_DEFAULTS: Cornell box and glass scene at 256 x 192, at 4 and at 256 passes,
relative MSE against 1024 samples of another seed, for the raw picture, the fixed filter at its defaults and the variance-guided
filter over iterations x sigma_luma (sigma_depth and sigma_albedo as the fixed filter's).  Prints one JSON object.

    python tools/guided_denoise_sweep.py [--out profiles/guided_denoise_sweep.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ITERATIONS = (2, 3, 4, 5, 6)
SIGMA_LUMA = (1.0, 2.0, 4.0, 8.0, 16.0)


def _scene(name, W, H):
    import clive2_amd as c2
    if name == "cornell":
        return c2.create_scene_from_preset("empty", W, H)
    from clive2_amd.load import get_materials
    from clive2_amd.meshes import icosphere
    mats = get_materials()
    mats["alpha"][5] = 0.1
    v, f = icosphere(2, radius=2.0, center=(0.0, 1.0, 0.0))
    return c2.create_scene(W, H, np.array([0, 1.5, 6]), np.array([0, 0, -1]), file_specs=[dict(mesh=(v, f), material=5)],
                           materials=mats)


def rmse(x, ref):
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from clive2_amd.renderer import Renderer, make_seeds
    W, H = 256, 192
    out = {"what": "relative MSE against 1024 samples of seed 4321, 256 x 192", "iterations": ITERATIONS, "sigma_luma": SIGMA_LUMA,
           "runs": []}
    for name in ("cornell", "glass"):
        scene = _scene(name, W, H)
        ref_r = Renderer(scene, seeds=make_seeds(W * H, seed=4321))
        ref_r.run_samples(1024)
        ref = ref_r.radiance
        ref_r.close()
        r = Renderer(scene)
        r.set_error_tracking(True)
        r.render_features(4)
        for n in (4, 16, 64, 256):
            r.run_samples(n - r.samples)
            run = {"scene": name, "passes": n, "raw": rmse(r.radiance, ref), "fixed": rmse(r.denoised_radiance(), ref),
                   "guided": [[rmse(r.guided_radiance(iterations=it, sigma_luma=sl), ref) for sl in SIGMA_LUMA] for it in ITERATIONS]}
            out["runs"].append(run)
            print(f"{name} {n}: raw {run['raw']:.3g} fixed {run['fixed']:.3g}", file=sys.stderr)
            for it, row in zip(ITERATIONS, run["guided"]):
                print(f"   it {it}: " + " ".join(f"{x:.3g}" for x in row), file=sys.stderr)
        r.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
