"""Command-line render: the flag surface of the reference's `src/render.py:13-19`, writing a PNG
instead of opening a cv2 window (display code is out of scope).

    python -m clive2_amd.render --scene empty --width 1280 --height 720 --samples 64 --out cornell.png
    python -m clive2_amd.render --scene empty --samples 4 --denoise --out cornell_denoised.png
    python -m clive2_amd.render --scene empty --target-error 0.05 --samples 1024 --error-out err.npy
    python -m clive2_amd.render --scene empty --target-error 0.05 --samples 1024 --denoise --variance-guided --out cornell_guided.png
    python -m clive2_amd.render --scene empty --target-error 0.05 --samples 1024 --denoise --error-of denoised --out cornell_until_denoised.png
    python -m clive2_amd.render --scene empty --samples 64 --denoise --select-scale --scale-out passes.npy --out cornell_selected.png
    python -m clive2_amd.render --scene empty --samples 256 --robust --out cornell_robust.png
    python -m clive2_amd.render --scene empty --samples 256 --robust-denoise --out cornell_robust_denoised.png
    python -m clive2_amd.render --scene empty --samples 64 --path-length 3: --out cornell_indirect_only.png
    python -m clive2_amd.render --scene empty --samples 64 --layers cornell
    python -m clive2_amd.render --scene empty --samples 4 --layers cornell --single-pass --denoise-layers

Several GPUs: start one process per GPU with RANK / LOCAL_RANK / WORLD_SIZE in the environment (e.g.
`python -m torch.distributed.run --nproc-per-node N -m clive2_amd.render ...`; any spawner will do, torch
itself is not used) -- every rank renders its share of the samples of the same frame with its own seeds,
ONE in-place RCCL all-reduce of the accumulators follows, rank 0 writes the picture.
"""
import argparse
import time

import numpy as np

from . import _native, strategies
from .camera import log_average, tone_map
from .distributed import rank_info, samples_for_rank, join_communicator
from .renderer import ERROR_FLOOR, UNIFORM_SHARE, Renderer, RendererError, stream_seeds
from .scene import create_scene_from_preset


def _save(path, image):
    try:
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(image[:, :, ::-1])).save(path)
    except ImportError:
        np.save(path + ".npy", image)


def _selected_image(renderer, dev, noise):
    """--select-scale's picture under the noise model `noise` (None: the default), tone-mapped on the device or on the host"""
    if noise is None:
        return renderer.tone_mapped("selected") if dev else renderer.selected_image
    if dev:
        renderer.keep_selected_picture(noise=noise)
        return renderer.tone_mapped_picture()
    return tone_map(renderer.selected_radiance(noise=noise), exposure=4.0)


def _write_layers(renderer, args, K):
    """--layers: the three layer pictures, tone-mapped with the log-average of their SUM so that their brightness is comparable."""
    t0 = time.time()
    try:
        if args.single_pass:
            layers = renderer.render_layers_once(-(-args.samples // K))
        else:
            layers = renderer.render_layers(-(-args.samples // K))
    finally:
        renderer.close()
    print(f"[rank 0] rendering {len(layers)} layers took {time.time() - t0:.2f} seconds")
    total = None
    for pic in layers.values():
        total = pic.copy() if total is None else total + pic
    Lw = log_average(total)
    for name, pic in layers.items():
        _save(f"{args.layers}_{name}.png", tone_map(pic, exposure=4.0, Lw=Lw))
    np.savez(f"{args.layers}_layers.npz", **layers)
    return 0


def _write_denoised_layers(renderer, args, K):
    """--layers --single-pass --denoise-layers: one render with per-layer accumulators, the features, then every layer through the
    filter on the device (Renderer.denoised_layers).  The pictures are tone-mapped ON THE DEVICE with the log-average of the
    filtered SUM: keep the sum, picture_log_sum, then each layer with that Lw."""
    t0 = time.time()
    try:
        renderer.reset_accumulators()
        renderer.set_layers(strategies.LAYERS)
        renderer.run_samples(-(-args.samples // K))
        renderer.render_features(args.feature_samples)
        layers, total = renderer.denoised_layers()
        renderer.keep_layer_picture(None)
        Lw = np.exp(np.float64(renderer.picture_log_sum()) / (args.width * args.height))
        images = {"denoised": renderer.tone_mapped_picture(exposure=4.0, log_average=Lw)}
        for name in layers:
            renderer.keep_layer_picture(name)
            images[name] = renderer.tone_mapped_picture(exposure=4.0, log_average=Lw)
    finally:
        renderer.close()
    print(f"[rank 0] rendering and filtering {len(layers)} layers took {time.time() - t0:.2f} seconds")
    for name, image in images.items():
        _save(f"{args.layers}_{name}.png", image)
    np.savez(f"{args.layers}_layers.npz", denoised=total, **layers)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--save-on-quit", action="store_true")
    ap.add_argument("--scene", type=str, default="empty")
    ap.add_argument("--out", type=str, default="render.png")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--device-tonemap", action="store_true",
                    help="tone-map on the device (Renderer.tone_mapped) instead of on the host with numpy (Renderer.image, the reference's "
                         "path); with --denoise, --variance-guided, --robust and --robust-denoise the derived picture stays on the device "
                         "and is tone-mapped there too (DESIGN.md 6.9)")
    ap.add_argument("--sample-streams", type=lambda v: v if v == "auto" else int(v), default=1,
                    help="K independent samples of the frame per pass (Renderer(streams=K): one seed buffer each, as K renderers "
                         "would hold; pays on mesh scenes, where it makes every launch K times larger); the samples are rounded up "
                         "to a multiple of K.  1 = the reference's single renderer; auto = by scene and frame size (Renderer.auto_streams)")
    ap.add_argument("--reproducible", action="store_true",
                    help="sum the light image in a fixed order (Renderer.set_reproducible) instead of with float atomics: two runs "
                         "then write the same bytes, as the reference's sort + gather chain does (renderer.py:212-250); slower")
    ap.add_argument("--visibility-query", action="store_true",
                    help="walk the t >= 2 connection rays as visibility queries seeded with their target triangle "
                         "(Renderer.set_connection_query(1), DESIGN.md 6.10): opt-in, not the parity path; no effect on scenes "
                         "whose tree is resident in LDS, such as the Cornell box")
    ap.add_argument("--denoise", action="store_true",
                    help="after the samples, render the first-hit features and write the denoised picture (Renderer.denoised_image)")
    ap.add_argument("--feature-samples", type=int, default=4, help="camera rays per pixel of the feature pass of --denoise")
    ap.add_argument("--variance-guided", action="store_true",
                    help="with --denoise: the filter whose edge-stop follows the per-pixel error estimate (Renderer.guided_image, "
                         "DESIGN.md 6.6): it closes where the picture has converged.  Turns error tracking on before the first sample")
    ap.add_argument("--select-scale", action="store_true",
                    help="with --denoise: choose the filter's number of passes per pixel by smoothed SURE maps "
                         "(Renderer.selected_image, DESIGN.md 6.16).  Turns error tracking on before the first sample.  Goes with "
                         "--target-error on the raw metric, --feature-samples and --device-tonemap; not with --variance-guided, "
                         "--robust, --robust-denoise, --denoise-layers or --error-of denoised")
    ap.add_argument("--scale-out", type=str, default=None, metavar="PATH.npy",
                    help="with --select-scale: save the chosen pass count per pixel ((H, W) int32) as .npy")
    ap.add_argument("--noise-model", choices=("independent", "correlated", "split"), default=None,
                    help="the noise model of the SURE estimates behind --error-of denoised and --select-scale (needs --denoise and one of "
                         "them; default independent): independent signs, signs spread like a camera sample over 3 x 3 pixels, or "
                         "split -- a mix of the two by each pixel's light share (DESIGN.md 6.17), which turns split tracking on "
                         "before the first sample and does not go with --adaptive")
    ap.add_argument("--light-share-out", type=str, default=None, metavar="PATH.npy",
                    help="with --noise-model split: save each pixel's light share of the luma variance (Renderer.light_share: (H, W) "
                         "float32, 1 where a pixel has no usable split) as .npy")
    ap.add_argument("--target-error", type=float, default=None,
                    help="render until the relative error e (Renderer.relative_error) is at most this, with --samples as the cap "
                         "(one rank only)")
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
    ap.add_argument("--error-out", type=str, default=None,
                    help="save the per-pixel standard error (Renderer.standard_error: (H, W, 4) float32 b, g, r, luma) as .npy")
    ap.add_argument("--robust", type=int, nargs="?", const=8, default=0, metavar="M",
                    help="save the firefly-robust picture: a Gini-trimmed median of means over M buckets per pixel, 3..16 "
                         "(Renderer.robust_image, DESIGN.md 6.7; default 8; tone-mapped on the host unless --device-tonemap).  Goes with --target-error and "
                         "--adaptive (the error metric stays on the plain estimates), not with --denoise")
    ap.add_argument("--robust-denoise", type=int, nargs="?", const=8, default=0, metavar="M",
                    help="save the robust picture after the variance-guided filter, guided by the variance of the buckets the trim "
                         "kept (Renderer.robust_guided_image, DESIGN.md 6.8): M buckets per pixel, 3..16, default 8; the feature pass "
                         "takes --feature-samples; tone-mapped on the host unless --device-tonemap.  Goes with --target-error and --adaptive (the error "
                         "metric stays on the plain estimates), not with --robust, --denoise or --variance-guided")
    ap.add_argument("--strategies", type=str, default=None, metavar="S,T;S,T;...",
                    help="keep the colour of these (s, t) connection strategies only (s light vertices 0..6, t camera vertices "
                         "1..6, s + t >= 2; Renderer.set_strategy_mask, DESIGN.md 6.11): every strategy keeps its MIS weight, so the "
                         "pictures of a partition add up to the full one")
    ap.add_argument("--path-length", type=str, default=None, metavar="A[:B]",
                    help="keep the strategies whose paths have exactly A edges (A), A to B edges (A:B) or A and more (A:); "
                         "1 = emitters seen directly, 2 = direct light.  Not with --strategies")
    ap.add_argument("--layers", type=str, default=None, metavar="PREFIX",
                    help="render the emission / direct / indirect layers (Renderer.render_layers, one render of --samples each from "
                         "the same seeds) and write PREFIX_emission.png, PREFIX_direct.png, PREFIX_indirect.png, tone-mapped with "
                         "the log-average of their sum, and PREFIX_layers.npz with the float pictures (one rank only)")
    ap.add_argument("--single-pass", action="store_true",
                    help="with --layers: write the same pictures from ONE render with per-layer accumulators "
                         "(Renderer.render_layers_once, DESIGN.md 6.12) instead of one render per layer")
    ap.add_argument("--denoise-layers", action="store_true",
                    help="with --layers PREFIX --single-pass: render the first-hit features (--feature-samples), filter every layer on "
                         "the device (Renderer.denoised_layers, DESIGN.md 6.14) and write the filtered PREFIX_<layer>.png, their sum "
                         "PREFIX_denoised.png, all tone-mapped on the device with the log-average of the sum, and PREFIX_layers.npz")
    args = ap.parse_args(argv)
    # refused before any renderer is made
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
        if args.variance_guided or args.robust or args.robust_denoise or args.denoise_layers or args.error_of == "denoised":
            ap.error("--select-scale chooses among the passes of the fixed filter: it does not go with --variance-guided, --robust, "
                     "--robust-denoise, --denoise-layers or --error-of denoised")
    if args.scale_out and not args.select_scale:
        ap.error("--scale-out saves the scale map of --select-scale")
    if args.noise_model is not None:
        if not (args.denoise and (args.error_of == "denoised" or args.select_scale)):
            ap.error("--noise-model sets the noise model of --error-of denoised or --select-scale: it needs --denoise and one of them")
        if args.noise_model == "split" and args.adaptive:
            ap.error("--noise-model split does not go with --adaptive: a sample density has no split form")
    if args.light_share_out and args.noise_model != "split":
        ap.error("--light-share-out saves the light share of --noise-model split")
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
    if args.error_of == "denoised":
        if args.target_error is None or not args.denoise:
            ap.error("--error-of denoised measures the picture --denoise saves: it needs --target-error and --denoise")
        if args.adaptive or args.robust or args.robust_denoise:
            ap.error("--error-of denoised does not go with --adaptive, --robust or --robust-denoise")

    if args.strategies is not None and args.path_length is not None:
        ap.error("--strategies and --path-length both set the strategy mask: give one")
    strategy_mask = None
    try:
        if args.strategies is not None:
            strategy_mask = strategies.parse_strategies(args.strategies)
        if args.path_length is not None:
            strategy_mask = strategies.parse_path_length(args.path_length)
    except ValueError as e:
        ap.error(str(e))
    if args.single_pass and args.layers is None:
        ap.error("--single-pass is a way to render --layers: give --layers PREFIX")
    if args.denoise_layers and not (args.layers is not None and args.single_pass):
        ap.error("--denoise-layers filters the layers of one render: give --layers PREFIX --single-pass")
    if args.layers is not None:
        if strategy_mask is not None:
            ap.error("--layers sets the strategy mask of each layer itself: it does not go with --strategies or --path-length")
        if args.target_error is not None:
            ap.error("--layers renders --samples per layer: it does not go with --target-error")
        if args.denoise or args.variance_guided or args.robust or args.robust_denoise:
            ap.error("--layers writes the plain layer pictures: it does not go with --denoise, --variance-guided, --robust or --robust-denoise")
        if args.device_tonemap:
            ap.error("--layers tone-maps its pictures on the host with one log-average: it does not go with --device-tonemap")
        if not args.layers:
            ap.error("--layers needs a file name prefix")

    rank, local_rank, world = rank_info()
    if args.layers is not None and world > 1:
        ap.error("--layers renders on one GPU: run it with a single rank (WORLD_SIZE=1)")
    if args.target_error is not None and world > 1:
        ap.error("--target-error renders one frame on one GPU: run it with a single rank (WORLD_SIZE=1)")
    scene = create_scene_from_preset(args.scene, pixel_width=args.width, pixel_height=args.height)
    if world > 1:
        # one GPU per rank; a launcher that exposes a single GPU to each rank makes it device 0
        device = local_rank % max(_native.lib().cl2_device_count(), 1)
    else:
        device = args.device
    renderer = Renderer(scene, device=device, streams=args.sample_streams if args.sample_streams == "auto" else max(1, args.sample_streams))
    K = renderer.streams
    if args.reproducible:
        renderer.set_reproducible(True)
    if args.visibility_query:
        renderer.set_connection_query(1)
    if args.target_error is not None or args.error_out or args.variance_guided or args.select_scale:
        renderer.set_error_tracking(True)
    if args.noise_model == "split":
        renderer.set_split_tracking(True)
    if args.robust or args.robust_denoise:
        renderer.set_robust_buckets(args.robust or args.robust_denoise)
    if strategy_mask is not None:
        renderer.set_strategy_mask(strategy_mask)      # before the first sample, the same on every rank
    # seed buffers of the job: stream k of rank r is buffer r * K + k
    renderer.set_seeds(stream_seeds(args.width * args.height, K, first_rank=rank * K))
    if args.denoise_layers:
        return _write_denoised_layers(renderer, args, K)
    if args.layers is not None:
        return _write_layers(renderer, args, K)
    if world > 1:
        join_communicator(renderer, rank, world)
    t0 = time.time()
    failure = None
    reached = None
    filtered = args.error_of == "denoised"
    try:
        if filtered:
            renderer.render_features(args.feature_samples)
            _, reached = renderer.render_until(args.target_error, max(1, -(-args.samples // K)), floor=args.error_floor,
                                               check_every=args.check_every,
                                               metric="guided" if args.variance_guided else "denoised",
                                               filter_params=dict(noise=args.noise_model) if args.noise_model else None)
        elif args.target_error is not None:
            _, reached = renderer.render_until(args.target_error, max(1, -(-args.samples // K)), floor=args.error_floor,
                                               check_every=args.check_every, adaptive=args.adaptive,
                                               uniform_share=args.uniform_share)
        else:
            renderer.run_samples(-(-samples_for_rank(args.samples, rank, world) // K))
    except (KeyboardInterrupt, RendererError) as e:
        failure = e
    if world > 1:
        # Agree on the outcome BEFORE the collective: a rank that failed must not leave its peers blocked in
        # the all-reduce, and a sum that lacks a rank's samples must not be mistaken for the picture.
        # (A rank that died outright cannot answer; its peers then fail in RCCL when the launcher kills the job.)
        try:
            bad = renderer.allreduce_host([1.0 if failure is not None else 0.0], op="max")[0] > 0.0
        except RendererError as e:
            bad, failure = True, failure or e
        if bad and not args.save_on_quit:
            renderer.close()
            if failure is not None:
                raise failure
            raise RendererError(f"[rank {rank}] another rank failed: the accumulators were not reduced")
        if bad:
            print(f"[rank {rank}] a rank stopped early: reducing what every rank has ({renderer.samples} samples here)")
        renderer.reduce_accumulators()
    elif failure is not None and not args.save_on_quit:
        raise failure
    dt = time.time() - t0
    rays = renderer.counters()["rays"]
    print(f"[rank {rank}] rendering took {dt:.2f} seconds ({renderer.samples} samples, {rays / max(dt, 1e-9) / 1e6:.0f} Mrays/s)")
    if reached is not None and filtered:
        print(f"[rank {rank}] target error {args.target_error}: {renderer.samples} samples, e_dn of the denoised picture {reached:.4g}")
    elif reached is not None:
        print(f"[rank {rank}] target error {args.target_error}: {renderer.samples} samples, relative error {reached:.4g}")
    if args.error_out and rank == 0:
        np.save(args.error_out, renderer.standard_error())
    if args.light_share_out and rank == 0:
        share, rho = renderer.light_share(return_map=True)
        print(f"[rank {rank}] light share of the frame's luma variance {share:.4g}")
        np.save(args.light_share_out, rho)
    if rank != 0:
        renderer.close()
        return 0
    # Tone-mapped uint8, BGR.  The film sits BEHIND the pinhole, so the picture on it is already upright
    # when read row 0 first (row 0 looks up at the ceiling light): the reference hands `renderer.image`
    # to cv2 unflipped (render.py:35-37).  Only the channel order changes for a PNG (BGR -> RGB).
    dev = args.device_tonemap
    if args.robust:
        image = renderer.tone_mapped("robust") if dev else renderer.robust_image
    elif args.robust_denoise:
        t1 = time.time()
        renderer.render_features(args.feature_samples)
        image = renderer.tone_mapped("robust_guided") if dev else renderer.robust_guided_image
        print(f"[rank {rank}] features ({args.feature_samples} rays per pixel) and denoising took {time.time() - t1:.2f} seconds")
    elif args.denoise:
        t1 = time.time()
        if not filtered:
            renderer.render_features(args.feature_samples)
        if args.select_scale:
            if args.scale_out:
                np.save(args.scale_out, renderer.selected_radiance(return_scale=True, noise=args.noise_model)[1])
            image = _selected_image(renderer, dev, args.noise_model)
        elif dev:
            image = renderer.tone_mapped("guided" if args.variance_guided else "denoised")
        else:
            image = renderer.guided_image if args.variance_guided else renderer.denoised_image
        print(f"[rank {rank}] features ({args.feature_samples} rays per pixel) and denoising took {time.time() - t1:.2f} seconds")
    else:
        image = renderer.tone_mapped("image") if dev else renderer.image
    renderer.close()
    try:
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(image[:, :, ::-1])).save(args.out)
    except ImportError:
        np.save(args.out + ".npy", image)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
