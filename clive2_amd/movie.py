"""Turntable movie: the flag surface of the reference's `src/movie.py:13-21`, one PNG per frame
instead of a cv2 window.  Every frame is its own scene (the camera quad is part of the geometry,
`load.py:261-271`) and its own Renderer, exactly as in the reference's frame loop (`movie.py:29-55`).

Frames are independent units: with one process per GPU (RANK / LOCAL_RANK / WORLD_SIZE in the
environment, e.g. under `python -m torch.distributed.run --nproc-per-node N -m clive2_amd.movie ...`)
rank r renders frames r, r+N, r+2N, ... on its own GPU with no collective.

    python -m clive2_amd.movie --scene empty --width 1280 --height 720 --samples 15 --movie-frames 120
"""
import argparse
import os
import shutil
import time

import numpy as np

from .distributed import rank_info
from .render import _selected_image
from .renderer import ERROR_FLOOR, UNIFORM_SHARE, Renderer, RendererError
from .scene import create_scene_from_preset_with_params


def frames_for_rank(start_frame, total_frames, rank, world):
    """Round-robin split of [start_frame, total_frames) -- neighbouring frames cost about the same."""
    return list(range(start_frame + rank, total_frames, world))


def save_frame(path, image):
    """`image` is the Renderer's tone-mapped uint8 BGR picture; row 0 is the TOP of the picture (the film
    sits behind the pinhole), exactly what the reference shows with cv2 (movie.py:45-47): BGR -> RGB only."""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(image[:, :, ::-1])).save(path)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--scene", type=str, default="teapots")
    ap.add_argument("--movie-name", type=str, default="test-movie")
    ap.add_argument("--movie-frames", type=int, default=120)
    ap.add_argument("--start-frame", type=int, default=0)
    ap.add_argument("--out-root", type=str, default="../output")
    ap.add_argument("--host-tonemap", action="store_true",
                    help="tone-map every frame on the host with numpy (the reference's path, Renderer.image) instead of on the device")
    ap.add_argument("--device-tonemap", action="store_true",
                    help="with --denoise, --variance-guided, --robust or --robust-denoise: keep the derived picture on the device and "
                         "tone-map it there (Renderer.tone_mapped, DESIGN.md 6.9) instead of copying it out as float32 and mapping it with "
                         "numpy; the plain picture is tone-mapped on the device already.  Not with --host-tonemap")
    ap.add_argument("--denoise", action="store_true",
                    help="after each frame's samples, render its first-hit features and save the denoised picture (Renderer.denoised_image)")
    ap.add_argument("--feature-samples", type=int, default=4, help="camera rays per pixel of the feature pass of --denoise")
    ap.add_argument("--variance-guided", action="store_true",
                    help="with --denoise: the filter whose edge-stop follows the per-pixel error estimate (Renderer.guided_image, "
                         "DESIGN.md 6.6).  Turns error tracking on before each frame's first sample")
    ap.add_argument("--select-scale", action="store_true",
                    help="with --denoise: choose the filter's number of passes per pixel by smoothed SURE maps "
                         "(Renderer.selected_image, DESIGN.md 6.16).  Turns error tracking on before each frame's first sample.  Goes "
                         "with --target-error on the raw metric, --feature-samples and --device-tonemap; not with --variance-guided, "
                         "--robust, --robust-denoise or --error-of denoised")
    ap.add_argument("--noise-model", choices=("independent", "correlated", "split"), default=None,
                    help="the noise model of the SURE estimates behind --error-of denoised and --select-scale (needs --denoise and one of "
                         "them; default independent): independent signs, signs spread like a camera sample over 3 x 3 pixels, or "
                         "split -- a mix of the two by each pixel's light share (DESIGN.md 6.17), which turns split tracking on "
                         "before the first sample and does not go with --adaptive")
    ap.add_argument("--target-error", type=float, default=None,
                    help="render each frame until its relative error (Renderer.relative_error) is at most this, --samples as the cap")
    ap.add_argument("--error-floor", type=float, default=None,
                    help=f"floor of the relative error's denominator L + floor (default {ERROR_FLOOR})")
    ap.add_argument("--check-every", type=int, default=8, help="passes between two checks of --target-error")
    ap.add_argument("--error-of", choices=("picture", "denoised"), default="picture",
                    help="what --target-error measures: the raw Monte Carlo picture (Renderer.relative_error, the default) or, with "
                         "--denoise, the filtered picture that is saved (Renderer.denoised_error, DESIGN.md 6.15; the guided filter's "
                         "with --variance-guided).  Not with --adaptive, --robust or --robust-denoise")
    ap.add_argument("--adaptive", action="store_true",
                    help="with --target-error: spread the camera samples by the per-pixel error estimate before every check "
                         "(adaptive sampling, DESIGN.md 6.5)")
    ap.add_argument("--uniform-share", type=float, default=None,
                    help=f"share of the density that stays uniform under --adaptive, in (0, 1] (default {UNIFORM_SHARE})")
    ap.add_argument("--robust", type=int, nargs="?", const=8, default=0, metavar="M",
                    help="save the firefly-robust picture: a Gini-trimmed median of means over M buckets per pixel, 3..16 "
                         "(Renderer.robust_image, DESIGN.md 6.7; default 8; tone-mapped on the host unless --device-tonemap).  Goes with --target-error and "
                         "--adaptive (the error metric stays on the plain estimates), not with --denoise")
    ap.add_argument("--robust-denoise", type=int, nargs="?", const=8, default=0, metavar="M",
                    help="save the robust picture after the variance-guided filter, guided by the variance of the buckets the trim "
                         "kept (Renderer.robust_guided_image, DESIGN.md 6.8): M buckets per pixel, 3..16, default 8; the feature pass "
                         "takes --feature-samples; tone-mapped on the host unless --device-tonemap.  Goes with --target-error and --adaptive (the error "
                         "metric stays on the plain estimates), not with --robust, --denoise or --variance-guided")
    args = ap.parse_args(argv)
    if args.target_error is not None and not (args.target_error > 0 and np.isfinite(args.target_error)):
        ap.error("--target-error must be positive and finite")
    if args.error_floor is not None and not (args.error_floor >= 0 and np.isfinite(args.error_floor)):
        ap.error("--error-floor must be >= 0 and finite")
    if args.check_every < 1:
        ap.error("--check-every must be >= 1")
    if args.adaptive and args.target_error is None:
        ap.error("--adaptive needs --target-error")
    if args.variance_guided and not args.denoise:
        ap.error("--variance-guided needs --denoise")
    if args.select_scale:
        if not args.denoise:
            ap.error("--select-scale needs --denoise")
        if args.variance_guided or args.robust or args.robust_denoise or args.error_of == "denoised":
            ap.error("--select-scale chooses among the passes of the fixed filter: it does not go with --variance-guided, --robust, "
                     "--robust-denoise or --error-of denoised")
    if args.noise_model is not None:
        if not (args.denoise and (args.error_of == "denoised" or args.select_scale)):
            ap.error("--noise-model sets the noise model of --error-of denoised or --select-scale: it needs --denoise and one of them")
        if args.noise_model == "split" and args.adaptive:
            ap.error("--noise-model split does not go with --adaptive: a sample density has no split form")
    if args.robust and not (3 <= args.robust <= 16):
        ap.error("--robust takes 3..16 buckets")
    if args.robust and args.denoise:
        ap.error("--robust does not go with --denoise: the denoisers take the plain picture")
    if args.robust_denoise and not (3 <= args.robust_denoise <= 16):
        ap.error("--robust-denoise takes 3..16 buckets")
    if args.robust_denoise and (args.robust or args.denoise or args.variance_guided):
        ap.error("--robust-denoise is a picture of its own: it does not go with --robust, --denoise or --variance-guided")
    if args.uniform_share is not None and not (0.0 < args.uniform_share <= 1.0):
        ap.error("--uniform-share must be in (0, 1]")
    if args.device_tonemap and args.host_tonemap:
        ap.error("--device-tonemap does not go with --host-tonemap")
    if args.error_of == "denoised":
        if args.target_error is None or not args.denoise:
            ap.error("--error-of denoised measures the picture --denoise saves: it needs --target-error and --denoise")
        if args.adaptive or args.robust or args.robust_denoise:
            ap.error("--error-of denoised does not go with --adaptive, --robust or --robust-denoise")

    rank, local_rank, world = rank_info()
    out_dir = os.path.join(args.out_root, args.movie_name)
    if world == 1 and args.start_frame == 0 and os.path.exists(out_dir):
        shutil.rmtree(out_dir)                       # movie.py:23-26: a fresh movie replaces the old one
                                                     # (with several ranks frames are only overwritten)
    os.makedirs(out_dir, exist_ok=True)

    for f in frames_for_rank(args.start_frame, args.movie_frames, rank, world):
        t0 = time.time()
        scene = create_scene_from_preset_with_params(args.scene, pixel_width=args.width, pixel_height=args.height,
                                                     frame_idx=f, total_frames=args.movie_frames)
        try:
            renderer = Renderer(scene, device=local_rank)
        except RendererError:
            if local_rank == 0:
                raise
            renderer = Renderer(scene, device=0)     # the launcher exposes one GPU per rank: it is device 0
        note = ""
        if args.variance_guided or args.select_scale:
            renderer.set_error_tracking(True)
        if args.noise_model == "split":
            renderer.set_split_tracking(True)
        if args.robust or args.robust_denoise:
            renderer.set_robust_buckets(args.robust or args.robust_denoise)
        filtered = args.error_of == "denoised"
        if filtered:
            renderer.render_features(args.feature_samples)
            _, reached = renderer.render_until(args.target_error, args.samples, floor=args.error_floor, check_every=args.check_every,
                                               metric="guided" if args.variance_guided else "denoised",
                                               filter_params=dict(noise=args.noise_model) if args.noise_model else None)
            note = f" ({renderer.samples} samples, e_dn of the denoised picture {reached:.4g})"
        elif args.target_error is not None:
            _, reached = renderer.render_until(args.target_error, args.samples, floor=args.error_floor, check_every=args.check_every,
                                               adaptive=args.adaptive, uniform_share=args.uniform_share)
            note = f" ({renderer.samples} samples, relative error {reached:.4g})"
        else:
            renderer.run_samples(args.samples)
        # a frame leaves the device tone-mapped (6 MB at 1080p; Renderer.image reads 66 MB of accumulators and maps them with numpy)
        dev = args.device_tonemap
        if args.robust:
            image = renderer.tone_mapped("robust") if dev else renderer.robust_image
        elif args.robust_denoise:
            renderer.render_features(args.feature_samples)
            image = renderer.tone_mapped("robust_guided") if dev else renderer.robust_guided_image
        elif args.denoise:
            if not filtered:
                renderer.render_features(args.feature_samples)
            if args.select_scale:
                image = _selected_image(renderer, dev, args.noise_model)
            elif dev:
                image = renderer.tone_mapped("guided" if args.variance_guided else "denoised")
            else:
                image = renderer.guided_image if args.variance_guided else renderer.denoised_image
        else:
            image = renderer.image if args.host_tonemap else renderer.tone_mapped("image")
        save_frame(os.path.join(out_dir, f"frame_{f:04d}.png"), image)
        del renderer, scene
        print(f"Frame {f} time: {time.time() - t0:.3f}{note}", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
