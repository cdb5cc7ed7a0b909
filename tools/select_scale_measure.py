"""Measurements behind the per-pixel scale choice (csrc/denoise_select.hpp).  Each part prints one JSON object.

    python tools/select_scale_measure.py smooth   [--out profiles/select_scale_smooth.json]
    python tools/select_scale_measure.py quality  [--out profiles/select_scale_quality.json]
    python tools/select_scale_measure.py timing   [--out profiles/select_scale_timing.json]

smooth    what Renderer.SELECT_SMOOTH_PASSES is chosen from: Cornell box and glass scene at 64 x 48, 24 renders of 32 samples with
          different seeds, features from 4 rays, the truth a 16,384-sample render; the true summed squared luma error (pixels with an
          estimate) of the raw picture, of three passes of the fixed filter and of the selected picture for smooth_passes 0..4, the
          mean of out[4] over the truth of the selected picture (the selection bias) and the histogram of the chosen levels.
quality   the same scenes at 256 x 192 with 4 and 64 samples: relative MSE against 1024 samples of another seed (rmse of
          tools/guided_denoise_sweep.py) of the raw picture, the fixed filter at its defaults and the selected picture; mean k*.
timing    Cornell box at 1920 x 1080: host clock around synchronised calls, median of 5 after a warm-up, of
          cl2_denoise_error(kind 0, 3 passes, one probe) and of cl2_denoise_select(K = 3, one probe) without host outputs for
          smooth_passes 0..4 (the difference of two neighbours is one smoothing pass), and of keep_selected_picture().
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from guided_denoise_sweep import _scene, rmse          # noqa: E402

LUMA = np.array([0.0722, 0.7152, 0.2126], np.float32).astype(np.float64)


def luma64(c):
    c = np.asarray(c, np.float32).astype(np.float64)
    return (c[..., 0] * LUMA[0] + c[..., 1] * LUMA[1]) + c[..., 2] * LUMA[2]


def smooth(renders=24, truth_samples=16384, K=3):
    from clive2_amd.renderer import Renderer, make_seeds
    W, H = 64, 48
    out = {"what": "64 x 48, 32 samples, mean over the renders of the true summed squared luma error over the pixels with an "
                   "estimate; selected[S] for smooth_passes S; bias[S] = mean out[4] / that truth; levels[S] = share of k* = 0..K",
           "renders": renders, "truth_samples": truth_samples, "K": K, "runs": []}
    for name in ("cornell", "glass"):
        scene = _scene(name, W, H)
        t = Renderer(scene, seeds=make_seeds(W * H, seed=4321))
        t.run_samples(truth_samples)
        mu = luma64(t.radiance)
        t.close()
        raw, fixed = [], []
        picked, est = [[] for _ in range(5)], [[] for _ in range(5)]
        hist = np.zeros((5, K + 1))
        for i in range(renders):
            r = Renderer(scene, seeds=make_seeds(W * H, seed=1000 + i))
            r.set_error_tracking(True)
            r.run_samples(32)
            r.render_features(4)
            acc = r.packed_accumulators().reshape(8, H, W)
            ok = (acc[3] > 0) & np.isfinite(acc[3]) & (acc[7] >= 2)          # the pixels with an estimate (err_pixel's state 2)
            for S in range(5):
                pic, scale, o = r.selected_radiance(iterations=K, seed=i, smooth_passes=S, return_scale=True, return_stats=True)
                picked[S].append(float(((luma64(pic) - mu) ** 2)[ok].sum()))
                est[S].append(float(o[4]))
                hist[S] += np.bincount(scale[ok], minlength=K + 1)
            raw.append(float(((luma64(r.radiance) - mu) ** 2)[ok].sum()))
            fixed.append(float(((luma64(r.denoised_radiance(iterations=K)) - mu) ** 2)[ok].sum()))
            r.close()
        run = {"scene": name, "raw": float(np.mean(raw)), "fixed": float(np.mean(fixed)),
               "selected": [float(np.mean(x)) for x in picked],
               "bias": [float(np.mean(e) / np.mean(x)) for e, x in zip(est, picked)],
               "levels": [(h / h.sum()).round(4).tolist() for h in hist]}
        out["runs"].append(run)
        print(json.dumps(run), file=sys.stderr)
    return out


def quality():
    from clive2_amd.renderer import Renderer, make_seeds
    W, H = 256, 192
    out = {"what": "relative MSE against 1024 samples of seed 4321, 256 x 192; selected at the defaults", "runs": []}
    for name in ("cornell", "glass"):
        scene = _scene(name, W, H)
        ref_r = Renderer(scene, seeds=make_seeds(W * H, seed=4321))
        ref_r.run_samples(1024)
        ref = ref_r.radiance
        ref_r.close()
        r = Renderer(scene)
        r.set_error_tracking(True)
        r.render_features(4)
        for n in (4, 64):
            r.run_samples(n - r.samples)
            pic, scale, o = r.selected_radiance(return_scale=True, return_stats=True)
            run = {"scene": name, "passes": n, "raw": rmse(r.radiance, ref), "fixed": rmse(r.denoised_radiance(), ref),
                   "selected": rmse(pic, ref), "mean_scale": float(scale.mean()), "e_sel": float(o[0]),
                   "levels": (np.bincount(scale.reshape(-1), minlength=4) / scale.size).round(4).tolist()}
            out["runs"].append(run)
            print(json.dumps(run), file=sys.stderr)
        r.close()
    return out


def _clock(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                  # every library call returns after its device work has drained
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "reps": reps}


def timing():
    from clive2_amd.renderer import Renderer
    W, H = 1920, 1080
    r = Renderer(_scene("cornell", W, H))
    r.set_error_tracking(True)
    r.run_samples(4)
    r.render_features(4)
    res = (C.c_double * 8)()

    def select(S):
        rc = r._L.cl2_denoise_select(r._h, 3, 2.0, 0.1, 0.1, 1, 1 / 16, 0, C.c_uint32(0), S, 0.001, None, 0, None, 0, res, None, 0,
                                     None, 0)
        assert rc == 0
    out = {"what": "Cornell box 1920 x 1080, host clock around synchronised calls, median of 5 after a warm-up; no host outputs "
                   "but the eight totals",
           "denoise_error_3_passes_1_probe": _clock(lambda: r.denoised_error(iterations=3, probes=1)),
           "denoise_select_K3_1_probe": {str(S): _clock(lambda: select(S)) for S in range(5)},
           "keep_selected_picture": _clock(r.keep_selected_picture)}
    r.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=("smooth", "quality", "timing"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    line = json.dumps({"smooth": smooth, "quality": quality, "timing": timing}[args.part]())
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
