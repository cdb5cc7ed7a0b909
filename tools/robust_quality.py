"""Quality of the robust picture (csrc/robust.hpp) on real renders: relative MSE of `radiance` and of
`robust_radiance()` against a 1024-pass picture of another seed, 256 x 192, M buckets, on the Cornell box and the glass scene at
4, 16, 64 and 256 passes -- the figures behind tests/test_gpu_robust.py::test_real_renders.  Prints one JSON object.

    python tools/robust_quality.py [--buckets 8] [--out profiles/robust_quality_mi355x.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _rmse(x, ref):                                   # tests/test_gpu_denoise.py
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2)))


def _dump(out):
    """the result as JSON, one run per line"""
    head = {k: v for k, v in out.items() if k not in ("runs", "kernels")}
    lines = ["{" + json.dumps(head)[1:-1] + ("," if head else ""), ' "runs": [']
    lines += ["  " + json.dumps(r) + ("," if i + 1 < len(out["runs"]) else "") for i, r in enumerate(out.get("runs", []))]
    lines.append(" ]" + (', "kernels": ' + json.dumps(out["kernels"]) if "kernels" in out else "") + "}")
    return "\n".join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--buckets", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from clive2_amd.renderer import Renderer, make_seeds
    from denoise_scenes import cornell, glass
    W, H = 256, 192
    out = {"what": "relative MSE against 1024 passes of seed 4321, 256 x 192; default seeds for the render", "buckets": args.buckets,
           "runs": []}
    for name, make in (("cornell", cornell), ("glass", glass)):
        scene = make(W, H)
        ref_r = Renderer(scene, seeds=make_seeds(W * H, seed=4321))
        ref_r.run_samples(1024)
        ref = ref_r.radiance
        ref_r.close()
        r = Renderer(scene)
        r.set_robust_buckets(args.buckets)
        for n in (4, 16, 64, 256):
            r.run_samples(n - r.samples)
            pic, st = r.robust_radiance(return_stats=True)
            raw, rob = _rmse(r.radiance, ref), _rmse(pic, ref)
            out["runs"].append({"scene": name, "passes": n, "rmse_raw": raw, "rmse_robust": rob, "robust_over_raw": rob / raw,
                                "trimmed_pixel_share": float((st[..., 1] > 0).mean()), "mean_gini": float(st[..., 0].mean())})
        r.close()
    text = _dump(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
