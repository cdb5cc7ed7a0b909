"""`Renderer`: the reference's render driver (src/renderer.py:16-352) on top of the HIP library.

Same constructor, stage-method names, `samples` counter, image properties and accumulator
attributes as the reference class, so callers written against it (`render.py:26-37`,
`movie.py:39-44`) work unchanged.  Differences, all deliberate:

* device state and accumulators live in the library (SoA in HBM); the accumulator attributes
  are read back on access instead of being updated on the host every sample;
* the RNG buffer is explicit: `Renderer(scene, seeds=...)` / `set_seeds()` (the reference seeds
  from unseeded `np.random.randint`, renderer.py:86-87, and is therefore not reproducible);
* `run_samples(n)` runs n iterations of the pipeline without returning to the host;
* `gather_light_image` is a no-op synchronisation point: the t=1 light-image splat happens in
  `join_paths` with float atomics (the reference's 300-launch bitonic sort + host bincount,
  renderer.py:212-250, has no counterpart);
* multi-GPU sample splitting: `comm_init(rank, world, id)` + `reduce_accumulators()` sum the
  accumulators of all ranks with one in-place RCCL all-reduce inside the library (no torch).
"""
import ctypes as C

import numpy as np

from . import _native
from ._native import RendererError, Counters, Organisation, ptr
from . import struct_types as st
from . import strategies
from .camera import tone_map
from .constants import timed, MAX_PATH_LENGTH  # noqa: F401

LIGHT, CAMERA = 0, 1

# Default floor of the relative error e(floor) = sqrt(mean var_L / (L + floor)^2) (Renderer.relative_error): half the darkest
# percentile of the Cornell box's and the glass scene's luma (0.0022), so it keeps truly near-black pixels from dominating e and
# leaves it a relative error everywhere else
ERROR_FLOOR = 0.001

# Default perturbation of Renderer.denoised_error: independent signs per pixel (False) or signs spread over 3 x 3 pixels like a
# camera sample's reconstruction weights (True).  Measured on 24 renders of 32 samples against a 16,384-sample picture, estimate /
# true squared luma error of the filtered picture, fixed / guided filter: Cornell box 0.99 / 0.88 independent and 1.01 / 1.94
# correlated; glass scene 1.04 / 1.20 independent and 0.58 / 0.44 correlated: the independent signs it is
DENOISED_ERROR_CORRELATED = False

# Default number of smoothing passes over the SURE maps of Renderer.selected_radiance: the smallest S in 0..4 for which, on 24 renders
# of 32 samples at 64 x 48 against a 16,384-sample picture, the true squared luma error of the selected picture is not above the
# larger of the raw picture's and the three-pass picture's, on the Cornell box and on the glass scene.  It holds for every S, so 0 it
# is.  selected / raw / three passes, S = 0, 1, 2, 3, 4: Cornell box (6.0, 3.0, 2.6, 2.7, 3.1) / 8.7 / 71 x 1e-4, glass scene
# (2.80, 3.08, 3.06, 3.06, 3.06) / 6.06 / 3.54 x 1e-2: two passes halve the Cornell box's error and cost the glass
# scene 9 %
SELECT_SMOOTH_PASSES = 0

# Default uniform share beta of adaptive sampling's density m = beta + (1 - beta) r / mean(r) (Renderer.update_sample_density,
# DESIGN.md 6.5)
UNIFORM_SHARE = 0.25


def make_seeds(batch_size, seed=20240928, rank=0):
    """Seed buffer of SURVEY.md §8(d): `RandomState(seed+rank).randint(0, 2**32, (B,2), uint32)`
    -- the call shape of renderer.py:86-87 -- with zeros (xorshift's fixed point) replaced by 1."""
    s = np.random.RandomState(seed + rank).randint(0, 2 ** 32, size=(batch_size, 2), dtype=np.uint32)
    s[s == 0] = 1
    return s


def stream_seeds(batch_size, streams, seed=20240928, first_rank=0):
    """Seed buffers of `streams` sample streams: stream k gets `make_seeds(batch, seed, first_rank + k)`, the buffer rank
    first_rank + k of a sample split would use.  Shape (batch, 2) for one stream, else (streams, batch, 2)."""
    if streams == 1:
        return make_seeds(batch_size, seed, first_rank)
    return np.stack([make_seeds(batch_size, seed, first_rank + k) for k in range(streams)])


def next_power_of_two(n):
    return 1 << (n - 1).bit_length() if n > 0 else 1


class Renderer:
    def __init__(self, scene, kernel_path=None, seeds=None, device=0, variant=None, streams=1):
        # kernel_path is accepted for signature compatibility (the reference JIT-compiles
        # trace.metal from it, renderer.py:27-29); the HIP kernels are precompiled.
        # variant="test" loads libclive2_amd_test.so (carries the cross-check resolve kernel).
        # streams=K: K independent samples of the frame per pass, one seed buffer each (what K reference Renderers --
        # the ranks of a sample split -- would render); seeds then has shape (K, batch, 2).  Default 1 = the reference;
        # "auto" = auto_streams() (with seeds=None: the default seed buffers of that many streams).
        self._h = C.c_void_p()
        self._L = _native.lib(variant)
        self.scene = scene
        self.device = device
        self.pixel_width, self.pixel_height = scene.pixel_width, scene.pixel_height
        self.batch_size = scene.pixel_width * scene.pixel_height
        rc = self._L.cl2_create(int(device), int(scene.pixel_width), int(scene.pixel_height), C.byref(self._h))
        if rc != 0:
            msg = self._L.cl2_last_error(None)
            self._h = C.c_void_p()
            raise RendererError(f"cl2_create failed ({rc}): {msg.decode() if msg else ''}")
        self.samples = 0
        self.streams = 1
        self.upload_scene(scene)
        if streams == "auto":
            streams = self.auto_streams()
        if int(streams) != 1:
            self.set_sample_streams(streams)
        self.set_seeds(stream_seeds(self.batch_size, self.streams) if seeds is None else seeds)

    # ---- plumbing ----
    _FATAL = (-2, -5)                    # CL2_E_HIP, CL2_E_COMM (include/clive2_amd.h): the device or the communicator is gone

    def _check(self, rc, what):
        if rc != 0:
            # close() aborts the communicator of a FAILED handle instead of waiting for peers.  A refused argument or a call out
            # of sequence (CL2_E_INVALID, CL2_E_STATE, CL2_E_NOMEM) leaves device and communicator healthy: a caller that catches
            # it and carries on must not tear the communicator down under peers that are fine.
            if rc in self._FATAL:
                self._failed = True
            msg = self._L.cl2_last_error(self._h)
            raise RendererError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def upload_scene(self, scene):
        if hasattr(scene, "validate"):
            scene.validate()
        def rec(a, dt):
            a = np.ascontiguousarray(a)
            if a.dtype.itemsize != dt.itemsize:
                raise RendererError(f"scene array has itemsize {a.dtype.itemsize}, expected {dt.itemsize}")
            return a.reshape(-1)
        boxes, tris = rec(scene.boxes, st.Box), rec(scene.triangles, st.Triangle)
        mats, cam = rec(scene.materials, st.Material), rec(scene.camera, st.Camera)
        ltris = rec(scene.light_triangles, st.Triangle)
        areas = np.ascontiguousarray(scene.light_surface_areas, dtype=np.float32).reshape(-1)
        lidx = np.ascontiguousarray(scene.light_triangle_indices, dtype=np.int32).reshape(-1)
        n_light = int(np.asarray(scene.light_counts).reshape(-1)[0])
        if not (len(ltris) == len(areas) == len(lidx) == n_light):
            raise RendererError("light arrays disagree in length")
        self._check(self._L.cl2_upload_scene(self._h, ptr(boxes), len(boxes), ptr(tris), len(tris), ptr(mats), len(mats),
                                             ptr(cam), ptr(ltris), ptr(areas), ptr(lidx), n_light), "cl2_upload_scene")

    def set_sample_streams(self, streams):
        """K independent samples of the frame per pass (cl2_set_sample_streams): frees and re-allocates the per-pixel device
        state, so the seeds must be set again -- `set_seeds` of shape (K, batch, 2), stream k = the buffer Renderer k of a
        sample split would own.  Accumulators, scene and counters are kept."""
        self._check(self._L.cl2_set_sample_streams(self._h, int(streams)), "cl2_set_sample_streams")
        self.streams = int(streams)

    def auto_streams(self):
        """The stream count `streams="auto"` takes: 1 for a scene whose tree is LDS-resident (one thread per pixel already fills
        the machine: the Cornell box gains nothing), else as many as bring a launch to about 2^24 entries, at most 8 (measured at
        1080p: config 3 9.7 / 11.2 / 11.4 Grays/s at 1 / 4 / 8 streams; at 3840 x 2160 two streams add 3 %)."""
        if self.organisation()["tree_in_lds"]:
            return 1
        return int(max(1, min(8, round((1 << 24) / self.batch_size))))

    def set_export_stream(self, stream):
        """The sample stream that export_rays / export_paths / export_aggregators / {ex,im}port_sample_images address."""
        self._check(self._L.cl2_set_export_stream(self._h, int(stream)), "cl2_set_export_stream")

    def set_seeds(self, seeds):
        s = np.ascontiguousarray(seeds, dtype=np.uint32)
        if s.size != 2 * self.batch_size * self.streams:
            raise RendererError(f"seed buffer needs {2 * self.batch_size * self.streams} uint32 words, got {s.size}")
        self._check(self._L.cl2_set_seeds(self._h, ptr(s), C.c_size_t(s.size)), "cl2_set_seeds")

    def get_random_buffer(self):
        """(batch, 2) uint32 as the reference's rand_buffer; (streams, batch, 2) with more than one sample stream."""
        shape = (self.batch_size, 2) if self.streams == 1 else (self.streams, self.batch_size, 2)
        s = np.empty(shape, dtype=np.uint32)
        self._check(self._L.cl2_get_seeds(self._h, ptr(s), C.c_size_t(s.size)), "cl2_get_seeds")
        return s

    # ---- the eight stages of run_sample (renderer.py:113-278) ----
    @timed
    def make_light_rays(self):
        self._check(self._L.cl2_make_light_rays(self._h), "make_light_rays")

    @timed
    def make_camera_rays(self):
        self._check(self._L.cl2_make_camera_rays(self._h), "make_camera_rays")

    @timed
    def trace_light_rays(self):
        self._check(self._L.cl2_trace_light_rays(self._h), "trace_light_rays")

    @timed
    def trace_camera_rays(self):
        self._check(self._L.cl2_trace_camera_rays(self._h), "trace_camera_rays")

    @timed
    def join_paths(self):
        self._check(self._L.cl2_join_paths(self._h), "join_paths")

    @timed
    def finalize_samples(self):
        self._check(self._L.cl2_finalize_samples(self._h), "finalize_samples")

    @timed
    def gather_light_image(self):
        self._check(self._L.cl2_gather_light_image(self._h), "gather_light_image")

    @timed
    def process_images(self):
        self._check(self._L.cl2_process_images(self._h), "process_images")

    @timed
    def run_sample(self):
        self.run_samples(1)

    def run_samples(self, n):
        """n passes of the pipeline = n x run_sample (n * streams samples of the frame with more than one sample stream)."""
        self._check(self._L.cl2_run_samples(self._h, int(n)), "run_samples")
        self.samples += int(n) * self.streams

    # ---- accumulators (renderer.py:41-45) ----
    def read_accumulators(self):
        H, W, B = self.pixel_height, self.pixel_width, self.batch_size
        img = np.empty((H, W, 3), np.float32)
        wts = np.empty((H, W, 1), np.float32)
        cnt = np.empty((H, W, 1), np.int32)
        uni = np.empty((H, W, 3), np.float32)
        self._check(self._L.cl2_read_accumulators(self._h, ptr(img), ptr(wts), ptr(cnt), ptr(uni), C.c_size_t(B)),
                    "cl2_read_accumulators")
        return img, wts, cnt, uni

    summed_image = property(lambda self: self.read_accumulators()[0])
    summed_sample_weights = property(lambda self: self.read_accumulators()[1])
    summed_sample_counts = property(lambda self: self.read_accumulators()[2])
    unidirectional_image_buffer = property(lambda self: self.read_accumulators()[3])

    def reset_accumulators(self):
        self._check(self._L.cl2_reset_accumulators(self._h), "cl2_reset_accumulators")
        self.samples = 0

    @property
    def radiance(self):
        """`summed_image / summed_sample_weights`, scrubbed -- the reference image before tone
        mapping (renderer.py:295-297); float32 (H,W,3), BGR."""
        img, wts, _, _ = self.read_accumulators()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.nan_to_num(img / wts, neginf=0, posinf=0)

    @property
    def unidirectional_radiance(self):
        _, _, cnt, uni = self.read_accumulators()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.nan_to_num(uni / cnt, neginf=0, posinf=0)

    @property
    def image(self):
        return tone_map(self.radiance, exposure=4.0)

    _PICTURES = {"image": 0, "unweighted_image": 1, "unidirectional_image": 2}

    def tone_log_sum(self, which="image"):
        """Sum over the pixels of log(0.1 + luma) of one of the three pictures, in float64, computed on the device
        (cl2_tone_log_sum): what `tone_mapped()` forms Lw = exp(sum / (W*H)) from.  NaN where a pixel's luma is below -0.1."""
        s = C.c_double(0.0)
        self._check(self._L.cl2_tone_log_sum(self._h, self._PICTURES[which], C.byref(s)), "cl2_tone_log_sum")
        return float(s.value)

    def tone_mapped(self, which="image", exposure=4.0, white_point=1.0, log_average=None):
        """`tone_map` (camera.py:73-82) of one of the three pictures of renderer.py:293-316, computed ON THE DEVICE from
        the accumulators (cl2_tone_log_sum + cl2_tone_map, csrc/tonemap.hpp): uint8 (H,W,3), BGR.  Only the 3*W*H bytes
        of the picture cross PCIe (the host path reads the 32*W*H bytes of the accumulators and maps them with numpy).
        Same arithmetic and dtypes as the host path: given the same Lw the bytes are the host's, every one (tests/test_gpu_tone.py).
        The float64 log-luminance sum is added in another order, so Lw can differ from the host's in its last bits, and a byte can
        then differ from `.image` by one count where 255*x/(x+w) lies within ~1e-13 (relative) of an integer.  Among ordinary
        pixels that is rare; a saturated pixel (x > 2^53, so x + w == x) always sits there: fl(255*x)/x is 255 or the double
        below it by the last bits of x, so many such bytes trade 254 for 255 at once (tests/tone_reference.py: fragile).
        `log_average`: use this Lw instead of the picture's own (no log-sum launch).

        `which` may also be "denoised", "guided", "robust" or "robust_guided": keep_picture(which) with the defaults, then
        tone_mapped_picture() -- the device counterpart of denoised_image, guided_image, robust_image and robust_guided_image.
        "selected": keep_selected_picture() with the defaults, the counterpart of selected_image.  This REPLACES the kept picture."""
        if which == "selected":                     # kept kind 8 has an entry point of its own (keep_selected_picture)
            self._numpy2("tone_mapped()")
            self.keep_selected_picture()
            return self.tone_mapped_picture(exposure, white_point, log_average)
        if which in self._KEPT_KINDS:
            self._numpy2("tone_mapped()")
            self.keep_picture(which)
            return self.tone_mapped_picture(exposure, white_point, log_average)
        w = self._PICTURES[which]
        # the device arithmetic restates what numpy >= 2 (NEP 50 promotion) makes of camera.py:73-82: the float32 picture times
        # the exposure stays float32 and is widened by the division by the float64 Lw.  numpy 1.x keeps `result` in float32
        # (value-based casting), and the host path then differs from this one by far more than one count.
        if int(np.__version__.split(".")[0]) < 2:
            raise RendererError("tone_mapped() reproduces the reference's tone map under numpy >= 2 (NEP 50) only; use .image")
        if log_average is None:
            log_avg = np.exp(np.float64(self.tone_log_sum(which)) / (self.pixel_height * self.pixel_width))   # Lw, with numpy's exp
        else:
            log_avg = log_average
        out = np.empty((self.pixel_height, self.pixel_width, 3), np.uint8)
        self._check(self._L.cl2_tone_map(self._h, w, float(exposure), float(white_point), float(log_avg), ptr(out),
                                         C.c_size_t(out.size)), "cl2_tone_map")
        return out

    # ---- a kept picture and its tone map on the device (cl2_keep_picture ... cl2_picture_tone_map, csrc/tonemap_picture.hpp) ----
    _KEPT_KINDS = {"denoised": 1, "guided": 2, "robust": 3, "robust_guided": 4}
    _KEPT_NAMES = {0: None, 1: "denoised", 2: "guided", 3: "robust", 4: "robust_guided", 5: "loaded", 6: "layer", 7: "layer_sum",
                   8: "selected"}

    @staticmethod
    def _numpy2(what):
        if int(np.__version__.split(".")[0]) < 2:
            raise RendererError(f"{what} reproduces the reference's tone map under numpy >= 2 (NEP 50) only; use the *_image properties")

    def keep_picture(self, kind, **params):
        """Compute one of the derived pictures and KEEP it in device memory instead of copying it to the host: `kind` is
        "denoised" (denoised_radiance), "guided" (guided_radiance), "robust" (robust_radiance), "robust_guided"
        (robust_guided_radiance) or None (drop the kept picture and free its 12*W*H bytes).  `params` are the filter arguments of
        the corresponding method (iterations, sigma_color or sigma_luma, sigma_depth, sigma_albedo); unset ones take
        DENOISE_DEFAULTS, GUIDED_DEFAULTS or ROBUST_GUIDED_DEFAULTS; "robust" takes none.  Same launches, same checks and same
        errors as that method.  The kept picture is a snapshot: later samples, resets and scene uploads do not change it; a
        refused call leaves the previous one in place."""
        if kind is None:
            if params:
                raise TypeError("keep_picture(None) takes no filter arguments")
            self._check(self._L.cl2_keep_picture(self._h, 0, 0, 0.0, 0.0, 0.0), "cl2_keep_picture")
            return
        if kind not in self._KEPT_KINDS:
            raise ValueError(f"kept picture: one of {sorted(self._KEPT_KINDS)} or None, not {kind!r}")
        d = {"denoised": self.DENOISE_DEFAULTS, "guided": self.GUIDED_DEFAULTS, "robust": {},
             "robust_guided": self.ROBUST_GUIDED_DEFAULTS}[kind]
        unknown = sorted(set(params) - set(d))
        if unknown:
            raise TypeError(f"keep_picture({kind!r}) takes {sorted(d)}, not {unknown}")
        a = {k: (v if params.get(k) is None else params[k]) for k, v in d.items()}
        sigma = a.get("sigma_color", a.get("sigma_luma", 0.0))
        self._check(self._L.cl2_keep_picture(self._h, self._KEPT_KINDS[kind], int(a.get("iterations", 0)), float(sigma),
                                             float(a.get("sigma_depth", 0.0)), float(a.get("sigma_albedo", 0.0))), "cl2_keep_picture")

    @property
    def kept_kind(self):
        """what the handle keeps: None, "denoised", "guided", "robust", "robust_guided", "loaded" (load_picture), "layer" or "layer_sum"
        (keep_layer_picture), "selected" (keep_selected_picture)"""
        return self._KEPT_NAMES[int(self._L.cl2_kept_picture(self._h))]

    def kept_picture(self):
        """The kept picture: float32 (H,W,3), BGR -- for kinds made by keep_picture, byte for byte what the corresponding
        *_radiance method returns."""
        out = np.empty((self.pixel_height, self.pixel_width, 3), np.float32)
        self._check(self._L.cl2_read_picture(self._h, ptr(out), C.c_size_t(out.size)), "cl2_read_picture")
        return out

    def load_picture(self, a):
        """Make `a` (3*W*H float32 values, (H,W,3) BGR) the kept picture (kind "loaded"): any float picture can take the device
        tone map, and tests inject states."""
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        self._check(self._L.cl2_write_picture(self._h, ptr(a), C.c_size_t(a.size)), "cl2_write_picture")

    def picture_log_sum(self):
        """Sum over the pixels of log(0.1 + luma) of the kept picture, in float64, on the device (cl2_picture_log_sum).  There is
        no scrub: NaN where a pixel is NaN or its luma is below -0.1, as numpy's sum on the host."""
        s = C.c_double(0.0)
        self._check(self._L.cl2_picture_log_sum(self._h, C.byref(s)), "cl2_picture_log_sum")
        return float(s.value)

    def tone_mapped_picture(self, exposure=4.0, white_point=1.0, log_average=None):
        """`tone_map` (camera.py:73-82) of the kept picture ON THE DEVICE: uint8 (H,W,3), BGR; 3*W*H bytes cross PCIe where the
        *_image properties copy 12*W*H and map them with numpy.  Given the same Lw the bytes are the host's tone_map(kept_picture()),
        every one; the float64 log sum is added in another order, so Lw can differ in its last bits and a byte can then differ by
        one count where 255*x/(x+w) lies within ~1e-13 (relative) of an integer (tone_mapped()'s docstring;
        tests/picture_tone_reference.py: fragile).  `log_average`: use this Lw instead of the picture's own."""
        self._numpy2("tone_mapped_picture()")
        if log_average is None:
            log_avg = np.exp(np.float64(self.picture_log_sum()) / (self.pixel_height * self.pixel_width))   # Lw, with numpy's exp
        else:
            log_avg = log_average
        out = np.empty((self.pixel_height, self.pixel_width, 3), np.uint8)
        self._check(self._L.cl2_picture_tone_map(self._h, float(exposure), float(white_point), float(log_avg), ptr(out),
                                                 C.c_size_t(out.size)), "cl2_picture_tone_map")
        return out

    @property
    def unweighted_image(self):
        return tone_map(np.nan_to_num(self.read_accumulators()[0], neginf=0, posinf=0), exposure=4.0)

    @property
    def unidirectional_image(self):
        return tone_map(self.unidirectional_radiance, exposure=4.0)

    # ---- multi-GPU sample split: one sum-reduce of the packed accumulators ----
    def packed_accumulators(self):
        a = np.empty(8 * self.batch_size, np.float32)
        self._check(self._L.cl2_read_accumulators_packed(self._h, ptr(a), C.c_size_t(a.size)), "read_packed")
        return a

    def load_packed_accumulators(self, a):
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        self._check(self._L.cl2_write_accumulators_packed(self._h, ptr(a), C.c_size_t(a.size)), "write_packed")

    def comm_init(self, rank, world_size, unique_id):
        """Join the RCCL communicator of the sample split (collective: returns when every rank has
        called it).  `unique_id`: the bytes rank 0 got from `comm_unique_id()` and handed to everybody
        (`clive2_amd.distributed.exchange_unique_id`)."""
        uid = bytes(unique_id)
        self._check(self._L.cl2_comm_init_rank(self._h, int(world_size), int(rank), uid, C.c_size_t(len(uid))), "cl2_comm_init_rank")
        self.rank, self.world_size = int(rank), int(world_size)

    def comm_unique_id(self):
        n = self._L.cl2_comm_unique_id_bytes()
        buf = C.create_string_buffer(n)
        rc = self._L.cl2_comm_get_unique_id(buf, C.c_size_t(n))
        if rc != 0:
            msg = self._L.cl2_last_error(None)
            raise RendererError(f"cl2_comm_get_unique_id failed ({rc}): {msg.decode() if msg else ''}")
        return buf.raw

    def reduce_accumulators(self):
        """ONE in-place all-reduce (sum) of the packed accumulators over the communicator's ranks
        (RCCL over xGMI); every rank then holds the sums.  Needs `comm_init`."""
        self._check(self._L.cl2_reduce_accumulators(self._h), "cl2_reduce_accumulators")

    def allreduce_host(self, values, op="sum"):
        """Up to 16 host floats summed / maximised over the ranks (also the barrier of the job)."""
        v = (C.c_double * len(values))(*[float(x) for x in values])
        self._check(self._L.cl2_comm_allreduce_f64(self._h, v, len(values), {"sum": 0, "max": 1}[op]), "cl2_comm_allreduce_f64")
        return list(v)

    def comm_info(self):
        """What the communicator says about itself (ncclCommCount / ncclCommUserRank / ncclCommCuDevice) and the PCI address
        of this handle's GPU; `nranks` is 0 without a communicator."""
        info = _native.CommInfo()
        self._check(self._L.cl2_comm_info(self._h, C.byref(info)), "cl2_comm_info")
        return {"nranks": info.nranks, "rank": info.rank, "comm_device": info.comm_device, "device_ordinal": info.device_ordinal,
                "pci_address": info.pci_address, "pci_bus_id": info.pci_bus_id.decode()}

    def comm_destroy(self):
        self._check(self._L.cl2_comm_destroy(self._h), "cl2_comm_destroy")

    def comm_abort(self):
        """This rank failed: tear the communicator down without waiting for the others (ncclCommAbort)."""
        self._L.cl2_comm_abort(self._h)

    def synchronize(self):
        self._check(self._L.cl2_synchronize(self._h), "cl2_synchronize")

    # ---- counters / profiling ----
    def set_profiling(self, level=2):
        """HIP-event stage timers: 0 off, 1 the connection-ray traversal launch only, 2 (or True) every stage."""
        level = 2 if level is True else int(level)
        self._check(self._L.cl2_set_profiling(self._h, level), "set_profiling")

    def set_counting(self, on=True):
        """True / 1: the node and triangle test tallies of the reference's walk (counters()); 2: what the 4-wide walk itself
        fetches (walk_tallies()); False / 0: off."""
        self._check(self._L.cl2_set_counting(self._h, int(on)), "set_counting")

    def walk_tallies(self):
        """{'subpath': {...}, 'connection': {...}} of set_counting(2): rays, wide nodes visited, triangle records read, stack
        entries spilled to global memory, binary records (rays with a non-finite 1/d) since the last reset_counters()."""
        t = _native.WalkTallies()
        self._check(self._L.cl2_read_walk_tallies(self._h, C.byref(t)), "read_walk_tallies")
        return {k: {n: getattr(getattr(t, k), n) for n, _ in _native.WalkTally._fields_} for k in ("subpath", "connection")}

    def set_levels_per_launch(self, levels):
        """Bounces traced per launch (1..6, 0 = chosen from the survival seen in the first sample); a pure
        performance knob, results are identical."""
        self._check(self._L.cl2_set_levels_per_launch(self._h, int(levels)), "set_levels_per_launch")

    def selftest_exact_math(self):
        """(rcp mismatches, x/pi mismatches) over all 2^32 float inputs; both must be 0."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.cl2_selftest_exact_math(self._h, C.byref(a), C.byref(b)), "selftest_exact_math")
        return a.value, b.value

    def set_pipelining(self, stages=-1):
        """Sample pipeline inside run_samples: 0 serial, 1 subpaths of sample i+1 beside the connection
        phase of sample i, 2 three stages, -1 (default) chosen by frame size.  A pure performance knob,
        results are identical."""
        self._check(self._L.cl2_set_pipelining(self._h, int(stages)), "set_pipelining")

    def set_traversal_mode(self, mode):
        """0 auto, 1 fused one-ray-per-lane kernels, 2 persistent traversal with ray replacement (one launch per
        level), 3 fused subpaths + persistent connection rays, 4 whole subpaths in one persistent launch, 5 exact 4-wide
        walk for the connection rays."""
        self._check(self._L.cl2_set_traversal_mode(self._h, int(mode)), "set_traversal_mode")

    def set_debug_flags(self, flags):
        """Launch-organisation switches (include/clive2_amd.h); none changes a result.  The shipped library
        refuses bits 0-2 (they skip parts of the resolve stage and exist only in the test variant)."""
        self._check(self._L.cl2_set_debug_flags(self._h, int(flags)), "set_debug_flags")

    def set_traversal_order(self, order=1):
        """Child order of the 4-wide walks (cl2_set_traversal_order): 0 = the reference's fixed order (trace.metal:157-160; the
        default, bit-exact), 1 = nearest child first -- fewer node visits and triangle tests per ray; exact-t ties go to the triangle
        the reference meets first, but NOT bit-exact by construction (a hit that rounding puts in front of its own leaf box is found
        or not depending on the visit order: a few rays in 1e8).  Opt-in; no reference counterpart."""
        self._check(self._L.cl2_set_traversal_order(self._h, int(order)), "set_traversal_order")

    def traversal_order(self):
        return int(self._L.cl2_get_traversal_order(self._h))

    def wide_stack_capacity(self):
        """Stack entries a lane of the 4-wide walk has for the uploaded scene in the current child order (LDS entries plus the
        per-lane overflow array, sized from the tree: cl2_wide_stack_capacity); 0 when the scene has no 4-wide collapse."""
        return int(self._L.cl2_wide_stack_capacity(self._h))

    def set_connection_query(self, mode=1):
        """What a connection ray asks of the tree (cl2_set_connection_query): 0 = its closest hit (the default, as the reference),
        1 = for a t >= 2 pair, whether the camera vertex's triangle is what the ray sees -- a walk seeded with that triangle, which
        prunes with its distance from the root on and stops at the first blocker.  Opt-in and NOT the parity path (the verdict
        differs where a hit lies in front of its own leaf box: a few rays in 1e8); refused together with set_traversal_order(1)
        and debug bits 13 / 14.  No reference counterpart."""
        self._check(self._L.cl2_set_connection_query(self._h, int(mode)), "set_connection_query")

    def connection_query(self):
        return int(self._L.cl2_get_connection_query(self._h))

    def connection_query_active(self):
        """1 iff the uploaded scene's connection launch really runs the seeded walk (0 for an LDS-resident tree such as the Cornell
        box, for a tree without a 4-wide collapse, and while set_counting(1) is on)."""
        return int(self._L.cl2_connection_query_active(self._h))

    def set_reproducible(self, on=True):
        """Reproducible light image (cl2_set_reproducible): the t = 1 contributions sorted and summed in a fixed order instead of
        float atomics -- two renders of the same scene and seeds then agree byte for byte, as the reference's sort + gather
        chain does (renderer.py:97-111, :213-250).  Off by default (costs a radix sort per pass)."""
        self._check(self._L.cl2_set_reproducible(self._h, int(bool(on))), "set_reproducible")

    # ---- strategy mask (cl2_set_strategy_mask, clive2_amd/strategies.py) ----
    def set_strategy_mask(self, mask_or_pairs=None):
        """Keep the colour of these (s, t) strategy pairs only: a 64-bit mask (strategies.bit / mask / path_length / LAYERS ...) or
        an iterable of (s, t) pairs; None = all 41 (the default).  A masked pair is still evaluated and keeps its MIS weight
        wherever that goes today, so the `radiance` of masks that partition strategies.ALL add up to the full picture; seeds,
        paths, filter weights, the unidirectional picture and the ray counters are those of the unmasked render.  Bits outside the 41
        are dropped.  The mask stays until it is set again (uploads, stream changes and resets keep it)."""
        m = strategies.to_mask(mask_or_pairs)
        self._check(self._L.cl2_set_strategy_mask(self._h, C.c_uint64(m)), "cl2_set_strategy_mask")

    def strategy_mask(self):
        m = C.c_uint64(0)
        self._check(self._L.cl2_get_strategy_mask(self._h, C.byref(m)), "cl2_get_strategy_mask")
        return int(m.value)

    def render_layers(self, passes, layers=strategies.LAYERS, seeds=None):
        """One render per layer of `layers` ({name: mask or pairs}; default emission / direct / indirect), all from the same seeds
        and therefore along the same paths: per layer reset_accumulators(), set_seeds(seeds), set_strategy_mask(layer),
        run_samples(passes), `radiance`.  Returns {name: (H, W, 3) float32, BGR}; layers that partition strategies.ALL add up to
        the unmasked `radiance` of the same seeds, to float rounding (use set_reproducible(True) for a light image summed in one
        order).  `seeds`: as set_seeds; None = the handle's current seeds.  The mask found on entry is restored; the accumulators
        are left holding the last layer.  With layers=strategies.SINGLETONS this is the per-strategy pyramid."""
        start = self.get_random_buffer() if seeds is None else np.array(seeds, dtype=np.uint32, copy=True)
        masks = {name: strategies.to_mask(m) for name, m in dict(layers).items()}     # refused before anything is rendered
        found = self.strategy_mask()
        out = {}
        try:
            for name, m in masks.items():
                self.reset_accumulators()
                self.set_seeds(start)
                self.set_strategy_mask(m)
                self.run_samples(passes)
                out[name] = self.radiance
        finally:
            self.set_strategy_mask(found)
        return out

    # ---- layer accumulators (cl2_set_layers, csrc/layers.hpp) ----
    def set_layers(self, layers=None):
        """Fill one colour accumulator per layer of `layers` ({name: mask or pairs}, at most 8, pairwise disjoint) in every pass,
        beside the ordinary accumulators, which get the bytes they get without layers.  Layer l receives what rows 0..2 of the
        accumulators receive in a render with set_strategy_mask(layer l): with set_reproducible(True) the same bytes.  None or an
        empty dictionary switches the layers off (the default).  The table stays until it is set again; setting another one on a
        handle that holds samples invalidates the layer accumulators until reset_accumulators().  Not together with a partial
        strategy mask, a sample density / adaptive sampling or the cross-check resolve kernel."""
        items = dict(layers or {})
        masks = strategies.layer_masks(items)                 # refused before the library sees anything
        arr = (C.c_uint64 * max(len(masks), 1))(*masks)
        self._check(self._L.cl2_set_layers(self._h, arr if masks else None, len(masks)), "cl2_set_layers")
        self._layer_names = list(items)

    def layers(self):
        """{name: mask} of the table that is set ({} = off); layers set through the C ABI alone are named layer0, layer1, ..."""
        m = (C.c_uint64 * strategies.MAX_LAYERS)()
        n = self._L.cl2_get_layers(self._h, m, strategies.MAX_LAYERS)
        if n < 0:
            self._check(n, "cl2_get_layers")
        names = getattr(self, "_layer_names", [])
        if len(names) != n:
            names = [f"layer{l}" for l in range(n)]
        return {names[l]: int(m[l]) for l in range(n)}

    def layer_accumulators(self):
        """The layer accumulators, float32 (L, 3, W*H): per layer the b, g, r planes, packed like rows 0..2 of
        packed_accumulators().  RendererError while they are invalid or no table is set."""
        n = len(self.layers())
        a = np.empty((n, 3, self.batch_size), np.float32)
        self._check(self._L.cl2_read_layers_packed(self._h, ptr(a), C.c_size_t(a.size)), "cl2_read_layers_packed")
        return a

    def load_layer_accumulators(self, a):
        """Write the layer accumulators (checkpoints: after load_packed_accumulators, which invalidates them)."""
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        self._check(self._L.cl2_write_layers_packed(self._h, ptr(a), C.c_size_t(a.size)), "cl2_write_layers_packed")

    def layer_radiance(self):
        """{name: (H, W, 3) float32, BGR}: layer accumulator / summed_sample_weights, scrubbed -- `radiance` of the render masked
        with the layer, from the one render that filled the accumulators."""
        names = list(self.layers())
        la = self.layer_accumulators()
        _, wts, _, _ = self.read_accumulators()
        H, W = self.pixel_height, self.pixel_width
        out = {}
        for l, name in enumerate(names):
            img = np.ascontiguousarray(la[l].reshape(3, H, W).transpose(1, 2, 0))
            with np.errstate(divide="ignore", invalid="ignore"):
                out[name] = np.nan_to_num(img / wts, neginf=0, posinf=0)
        return out

    # ---- the filter over the layers (cl2_denoise_layers, cl2_keep_layer_picture, csrc/denoise_layers.hpp) ----
    # DENOISE_DEFAULTS, and a colour sigma per layer name where one measured better (a name not listed takes DENOISE_DEFAULTS'):
    # on the 256 x 192, 4-pass set-up of DESIGN 6.3 the indirect layer of strategies.LAYERS wants a wide edge-stop (relative MSE of
    # the sum on the glass scene 0.78 of the same-sigma sum's, Cornell box unchanged); emission and direct moved neither scene by
    # more than 0.5 % anywhere between 0.5 and 32 (tools/layers_denoise_quality.py)
    LAYER_DENOISE_DEFAULTS = dict(iterations=3, sigma_color={"indirect": 8.0}, sigma_depth=0.1, sigma_albedo=0.1)

    def _layer_filter_args(self, iterations, sigma_color, sigma_depth, sigma_albedo):
        d = self.LAYER_DENOISE_DEFAULTS
        names = list(self.layers())
        default = self.DENOISE_DEFAULTS["sigma_color"]
        sc = {} if sigma_color is None else sigma_color
        if isinstance(sc, dict):
            unknown = sorted(set(sc) - set(names))
            if unknown:
                raise ValueError(f"sigma_color names layers that are not set: {unknown} (set: {names})")
            sig = [float(sc.get(n, d["sigma_color"].get(n, default))) for n in names]
        else:
            sig = [float(sc)] * len(names)
        arr = np.asarray(sig if sig else [default], dtype=np.float32)       # never NULL: without a table the library refuses
        it = d["iterations"] if iterations is None else int(iterations)
        sd = d["sigma_depth"] if sigma_depth is None else float(sigma_depth)
        sa = d["sigma_albedo"] if sigma_albedo is None else float(sigma_albedo)
        return names, it, arr, sd, sa

    def denoised_layers(self, iterations=None, sigma_color=None, sigma_depth=None, sigma_albedo=None):
        """The layers of the render in the accumulators (set_layers), each through the filter of denoised_radiance() with its
        own colour sigma, and their sum, in ONE device call: ({name: (H,W,3) float32, BGR}, sum).  `sigma_color` is a float for
        all layers or {name: float}; names not given take LAYER_DENOISE_DEFAULTS' value for that name, else
        DENOISE_DEFAULTS'; the other unset arguments take LAYER_DENOISE_DEFAULTS.  Layer `name` is, byte for byte, denoised_radiance() of a render masked with that layer; the sum is
        added in float32 in table order.  iterations=0 is layer_radiance() computed on the device.  render_features() first."""
        names, it, sig, sd, sa = self._layer_filter_args(iterations, sigma_color, sigma_depth, sigma_albedo)
        H, W = self.pixel_height, self.pixel_width
        lay, tot = np.empty((max(len(names), 1), H, W, 3), np.float32), np.empty((H, W, 3), np.float32)
        self._check(self._L.cl2_denoise_layers(self._h, it, ptr(sig), sd, sa, ptr(lay), C.c_size_t(len(names) * H * W * 3), ptr(tot),
                                               C.c_size_t(tot.size)), "cl2_denoise_layers")
        return {name: lay[l] for l, name in enumerate(names)}, tot

    def keep_layer_picture(self, name=None, **params):
        """Filter as denoised_layers(**params) does and KEEP one layer's picture (`name`) or the sum (None) in device memory, for
        kept_picture(), picture_log_sum() and tone_mapped_picture(): the bytes of denoised_layers, nothing copied to the host.  For
        a single layer only that layer is filtered.  keep_picture(None) drops it; a refused call leaves the previous kept picture."""
        unknown = sorted(set(params) - {"iterations", "sigma_color", "sigma_depth", "sigma_albedo"})
        if unknown:
            raise TypeError(f"keep_layer_picture takes iterations, sigma_color, sigma_depth, sigma_albedo, not {unknown}")
        names, it, sig, sd, sa = self._layer_filter_args(params.get("iterations"), params.get("sigma_color"),
                                                         params.get("sigma_depth"), params.get("sigma_albedo"))
        if name is not None and name not in names:
            raise ValueError(f"keep_layer_picture: {name!r} is not a layer of the table (set: {names})")
        layer = -1 if name is None else names.index(name)
        self._check(self._L.cl2_keep_layer_picture(self._h, layer, it, ptr(sig), sd, sa), "cl2_keep_layer_picture")

    def render_layers_once(self, passes, layers=strategies.LAYERS, seeds=None):
        """The dictionary render_layers returns, from ONE render: reset_accumulators(), set_seeds(seeds), set_layers(layers),
        run_samples(passes), layer_radiance().  `seeds`: as set_seeds; None = the handle's current seeds.  The layer table found on
        entry is restored; the accumulators are left holding the full picture of the render."""
        start = self.get_random_buffer() if seeds is None else np.array(seeds, dtype=np.uint32, copy=True)
        table = dict(layers)
        strategies.layer_masks(table)                          # refused before anything is rendered
        found = self.layers()
        try:
            self.reset_accumulators()
            self.set_seeds(start)
            self.set_layers(table)
            self.run_samples(passes)
            return self.layer_radiance()
        finally:
            self.set_layers(found)

    def set_subpath_gather(self, lanes=0, wait_steps=0):
        """Whole-subpath launch: lanes gathered / steps waited before a wave runs its bounce phase (0 = default)."""
        self._check(self._L.cl2_set_subpath_gather(self._h, int(lanes), int(wait_steps)), "set_subpath_gather")

    def tune(self):
        """Make the measured launch-organisation choices now (cl2_tune); returns the number of (real) samples it rendered."""
        n = C.c_int(0)
        self._check(self._L.cl2_tune(self._h, C.byref(n)), "cl2_tune")
        self.samples += n.value * self.streams
        return n.value

    def counters(self):
        c = Counters()
        self._check(self._L.cl2_read_counters(self._h, C.byref(c)), "read_counters")
        return c.as_dict()

    def organisation(self):
        """What the automatic launch-organisation choices came to for this scene (dict of cl2_organisation)."""
        o = Organisation()
        self._check(self._L.cl2_query_organisation(self._h, C.byref(o)), "query_organisation")
        return o.as_dict()

    def reset_counters(self):
        self._check(self._L.cl2_reset_counters(self._h), "reset_counters")

    # ---- debug exports in the reference's AoS layouts ----
    def export_rays(self, which):
        out = np.zeros(self.batch_size, dtype=st.Ray)
        self._check(self._L.cl2_export_rays(self._h, int(which), ptr(out), C.c_size_t(len(out))), "export_rays")
        return out

    def export_paths(self, which):
        out = np.zeros(self.batch_size, dtype=st.Path)
        self._check(self._L.cl2_export_paths(self._h, int(which), ptr(out), C.c_size_t(len(out))), "export_paths")
        return out

    def export_aggregators(self):
        out = np.zeros(self.batch_size, dtype=st.WeightAggregator)
        self._check(self._L.cl2_export_aggregators(self._h, ptr(out), C.c_size_t(len(out))), "export_aggregators")
        return out

    def export_connections(self):
        """Connection stage of the last join_paths: cmask (uint64 per pixel), hit triangle per strategy pair (int32 [36, B],
        meaningful where the pair's cmask bit is set) and hit distance of the t = 1 pairs (float32 [6, B])."""
        B = self.batch_size
        cmask = np.zeros(B, np.uint64)
        tri = np.zeros((36, B), np.int32)
        t1 = np.zeros((6, B), np.float32)
        self._check(self._L.cl2_export_connections(self._h, ptr(cmask), ptr(tri), ptr(t1), C.c_size_t(B)), "export_connections")
        return cmask, tri, t1

    def export_sample_images(self):
        B = self.batch_size
        fin, light, uni = (np.zeros((B, 4), np.float32) for _ in range(3))
        sw = np.zeros(B, np.float32)
        self._check(self._L.cl2_export_sample_images(self._h, ptr(fin), ptr(light), ptr(sw), ptr(uni), C.c_size_t(B)),
                    "export_sample_images")
        return dict(finalized=fin, light=light, sample_weights=sw, unidirectional=uni)

    def import_sample_images(self, finalized=None, light=None, sample_weights=None, unidirectional=None):
        """Per-sample images from host arrays ((B,4) float32 / (B,) float32): lets `process_images` be
        checked on its own against the reference's numpy code (tests/golden/renderer_glue.npz)."""
        def f4(a):
            return None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(self.batch_size, 4)
        fin, li, un = f4(finalized), f4(light), f4(unidirectional)
        sw = None if sample_weights is None else np.ascontiguousarray(sample_weights, dtype=np.float32).reshape(self.batch_size)
        self._check(self._L.cl2_import_sample_images(self._h, ptr(fin), ptr(li), ptr(sw), ptr(un), C.c_size_t(self.batch_size)),
                    "import_sample_images")

    def probe_traverse(self, rays):
        rays = np.ascontiguousarray(rays, dtype=st.Ray)
        n = len(rays)
        bi, bt = np.empty(n, np.int32), np.empty(n, np.float32)
        u, v = np.empty(n, np.float32), np.empty(n, np.float32)
        self._check(self._L.cl2_probe_traverse(self._h, ptr(rays), C.c_size_t(n), ptr(bi), ptr(bt), ptr(u), ptr(v)),
                    "probe_traverse")
        return bi, bt, u, v

    def probe_visibility(self, rays, targets):
        """Every ray through the seeded visibility walk with its target triangle (cl2_probe_visibility): per ray the stored triangle
        and its distance -- (T, t_T) where the target is visible, the first blocker met where it is not, (-1, inf) where the ray
        misses T; a target < 0 gives the plain closest hit."""
        rays = np.ascontiguousarray(rays, dtype=st.Ray)
        targets = np.ascontiguousarray(targets, dtype=np.int32)
        n = len(rays)
        if targets.shape != (n,):
            raise ValueError("probe_visibility: one target per ray")
        tri, t = np.empty(n, np.int32), np.empty(n, np.float32)
        self._check(self._L.cl2_probe_visibility(self._h, ptr(rays), C.c_size_t(n), ptr(targets), ptr(tri), ptr(t)),
                    "probe_visibility")
        return tri, t

    # ---- denoiser (cl2_render_features / cl2_read_features / cl2_denoise, csrc/denoise.hpp) ----
    # settled on the Cornell box and the glass scene at 256 x 192, 4 samples, against 1024-sample pictures (include/clive2_amd.h)
    DENOISE_DEFAULTS = dict(iterations=3, sigma_color=2.0, sigma_depth=0.1, sigma_albedo=0.1)

    def render_features(self, samples=4, seeds=None):
        """First-hit guide buffers of the frame: `samples` jittered camera rays per pixel, their closest hits averaged into
        normal, depth, albedo and coverage (features()).  `seeds`: (W*H, 2) uint32 in the layout of set_seeds with one stream;
        default make_seeds(W*H, seed=1), a buffer apart from the render's.  The render's seeds, accumulators and counters are
        not touched."""
        s = make_seeds(self.batch_size, seed=1) if seeds is None else seeds
        s = np.ascontiguousarray(s, dtype=np.uint32)
        if s.size != 2 * self.batch_size:
            raise RendererError(f"feature seeds need {2 * self.batch_size} uint32 words, got {s.size}")
        self._check(self._L.cl2_render_features(self._h, ptr(s), C.c_size_t(s.size), int(samples)), "cl2_render_features")

    def features(self):
        """The guide buffers the filter reads: normal (H,W,3), depth (H,W), albedo (H,W,3) b, g, r, coverage (H,W); float32."""
        H, W = self.pixel_height, self.pixel_width
        g0, g1 = np.empty((H, W, 4), np.float32), np.empty((H, W, 4), np.float32)
        self._check(self._L.cl2_read_features(self._h, ptr(g0), ptr(g1), C.c_size_t(H * W)), "cl2_read_features")
        return dict(normal=g0[..., :3], depth=g0[..., 3], albedo=g1[..., :3], coverage=g1[..., 3])

    def load_features(self, normal, depth, albedo, coverage):
        """Write the guide buffers (the counterpart of features(), same shapes): they become the current features of the
        uploaded scene, as if render_features() had made them.  The render state is not touched."""
        H, W = self.pixel_height, self.pixel_width
        g0, g1 = np.empty((H, W, 4), np.float32), np.empty((H, W, 4), np.float32)
        g0[..., :3], g0[..., 3] = np.reshape(normal, (H, W, 3)), np.reshape(depth, (H, W))
        g1[..., :3], g1[..., 3] = np.reshape(albedo, (H, W, 3)), np.reshape(coverage, (H, W))
        self._check(self._L.cl2_write_features(self._h, ptr(g0), ptr(g1), C.c_size_t(H * W)), "cl2_write_features")

    def denoised_radiance(self, iterations=None, sigma_color=None, sigma_depth=None, sigma_albedo=None):
        """`radiance` after the edge-avoiding a-trous filter guided by the features (render_features() first; a new scene
        needs new features): float32 (H,W,3), BGR.  Unset arguments take DENOISE_DEFAULTS."""
        d = self.DENOISE_DEFAULTS
        it = d["iterations"] if iterations is None else int(iterations)
        sc = d["sigma_color"] if sigma_color is None else float(sigma_color)
        sd = d["sigma_depth"] if sigma_depth is None else float(sigma_depth)
        sa = d["sigma_albedo"] if sigma_albedo is None else float(sigma_albedo)
        out = np.empty((self.pixel_height, self.pixel_width, 3), np.float32)
        self._check(self._L.cl2_denoise(self._h, it, sc, sd, sa, ptr(out), C.c_size_t(out.size)), "cl2_denoise")
        return out

    @property
    def denoised_image(self):
        """`image` of the denoised radiance: tone_map(denoised_radiance(), exposure=4.0) on the host, uint8 (H,W,3), BGR."""
        return tone_map(self.denoised_radiance(), exposure=4.0)

    # ---- variance-guided denoiser (cl2_denoise_guided, csrc/denoise_guided.hpp) ----
    # settled on the Cornell box and the glass scene at 256 x 192, at 4 and at 256 passes, against 1024-sample pictures
    GUIDED_DEFAULTS = dict(iterations=4, sigma_luma=4.0, sigma_depth=0.1, sigma_albedo=0.1)

    def guided_radiance(self, iterations=None, sigma_luma=None, sigma_depth=None, sigma_albedo=None, return_variance=False):
        """`radiance` after the a-trous filter whose edge-stop compares luma differences with the per-pixel standard error
        (render_features() first, error tracking on since the last reset): float32 (H,W,3), BGR.  Where the estimate says
        "converged" the filter closes, so more samples give a sharper picture.  Unset arguments take GUIDED_DEFAULTS.
        return_variance=True returns (picture, v'): v' (H,W) float32 is the luma variance the filter carried through its
        passes -- its GUIDE, not an error estimate of the filtered picture (it treats the taps of every pass as independent
        and comes out 10 to 100 times too small)."""
        d = self.GUIDED_DEFAULTS
        it = d["iterations"] if iterations is None else int(iterations)
        sl = d["sigma_luma"] if sigma_luma is None else float(sigma_luma)
        sd = d["sigma_depth"] if sigma_depth is None else float(sigma_depth)
        sa = d["sigma_albedo"] if sigma_albedo is None else float(sigma_albedo)
        out = np.empty((self.pixel_height, self.pixel_width, 3), np.float32)
        var = np.empty((self.pixel_height, self.pixel_width), np.float32) if return_variance else None
        self._check(self._L.cl2_denoise_guided(self._h, it, sl, sd, sa, ptr(out), C.c_size_t(out.size), ptr(var),
                                               C.c_size_t(0 if var is None else var.size)), "cl2_denoise_guided")
        return (out, var) if return_variance else out

    @property
    def guided_image(self):
        """`image` of the variance-guided radiance: tone_map(guided_radiance(), exposure=4.0) on the host, uint8 (H,W,3), BGR."""
        return tone_map(self.guided_radiance(), exposure=4.0)

    # ---- error estimates (cl2_set_error_tracking ... cl2_run_until, csrc/error_estimate.hpp) ----
    ERROR_FLOOR = ERROR_FLOOR

    def set_error_tracking(self, on=True):
        """Track the second moments of every sample's addends (off by default; 32*W*H bytes of device memory while on).  Turned
        on while the accumulators hold samples, the moments stay invalid -- and the error calls refuse -- until reset_accumulators()."""
        self._check(self._L.cl2_set_error_tracking(self._h, int(bool(on))), "cl2_set_error_tracking")

    @property
    def error_tracking(self):
        return bool(self._L.cl2_get_error_tracking(self._h) == 1)

    def moments(self):
        """The moment buffer [8][W*H] float32 (x_c^2 b, g, r | w^2 | x_c w b, g, r | y^2), packed like packed_accumulators()."""
        a = np.empty(8 * self.batch_size, np.float32)
        self._check(self._L.cl2_read_moments_packed(self._h, ptr(a), C.c_size_t(a.size)), "cl2_read_moments_packed")
        return a

    def load_moments(self, a):
        """Write the moment buffer (checkpoints: after load_packed_accumulators, which invalidates the moments)."""
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        self._check(self._L.cl2_write_moments_packed(self._h, ptr(a), C.c_size_t(a.size)), "cl2_write_moments_packed")

    def standard_error(self):
        """Per-pixel standard error of `radiance` by the delta method: float32 (H,W,4) b, g, r, luma; 0 where the pixel has no
        sample weight, inf with fewer than 2 samples."""
        out = np.empty((self.pixel_height, self.pixel_width, 4), np.float32)
        self._check(self._L.cl2_read_standard_error(self._h, ptr(out), C.c_size_t(out.size)), "cl2_read_standard_error")
        return out

    def relative_error(self, floor=None):
        """e(floor) = sqrt(mean over covered pixels of var_L / (L + floor)^2): the frame's relative noise level."""
        e = C.c_double(0.0)
        f = self.ERROR_FLOOR if floor is None else float(floor)
        self._check(self._L.cl2_relative_error(self._h, f, C.byref(e)), "cl2_relative_error")
        return e.value

    # ---- the luma variance split into its camera and its light part (cl2_set_split_tracking ... cl2_light_share,
    # csrc/error_split.hpp) ----
    def set_split_tracking(self, on=True):
        """Keep every sample's luma moments apart for its camera part and its light part (off by default; 24*W*H bytes of device
        memory while on), for noise="split" and light_share().  Turns error tracking on too if it is off.  The rules are those of
        set_error_tracking: turned on while the accumulators hold samples, the rows stay invalid until reset_accumulators().
        Not together with a sample density."""
        if on and not self.error_tracking:
            self.set_error_tracking(True)
        self._check(self._L.cl2_set_split_tracking(self._h, int(bool(on))), "cl2_set_split_tracking")

    @property
    def split_tracking(self):
        return bool(self._L.cl2_get_split_tracking(self._h) == 1)

    def split_moments(self):
        """The split rows [6][W*H] float32 (camera yc^2, yc wc, wc^2 | light yl^2, yl wl, wl^2), packed like moments()."""
        a = np.empty(6 * self.batch_size, np.float32)
        self._check(self._L.cl2_read_split_moments_packed(self._h, ptr(a), C.c_size_t(a.size)), "cl2_read_split_moments_packed")
        return a

    def load_split_moments(self, a):
        """Write the split rows (checkpoints: after load_packed_accumulators, which invalidates them)."""
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        self._check(self._L.cl2_write_split_moments_packed(self._h, ptr(a), C.c_size_t(a.size)), "cl2_write_split_moments_packed")

    def light_share(self, return_map=False):
        """The share of the frame's luma variance that comes from the light image (t = 1 splats, whose noise is independent between
        pixels; the rest is camera-image noise, correlated over 3 x 3 pixels): sum rho var_L / sum var_L over the pixels with an
        estimate.  return_map=True returns (share, rho): rho float32 (H,W), 1 where a pixel has no usable split."""
        out = (C.c_double * 4)()
        m = np.empty((self.pixel_height, self.pixel_width), np.float32) if return_map else None
        self._check(self._L.cl2_light_share(self._h, ptr(m), C.c_size_t(0 if m is None else m.size), out), "cl2_light_share")
        return (float(out[0]), m) if return_map else float(out[0])

    # ---- the error of the filtered picture (cl2_denoise_error, csrc/denoise_error.hpp) ----
    _ERROR_KINDS = {"denoised": 0, "guided": 1}
    NOISE_MODELS = {"independent": 0, "correlated": 1, "split": 2}

    def _noise_model(self, noise, correlated, who):
        """None (the old entry points, `correlated` as before) or the model's number for the *_model entry points"""
        if noise is None:
            return None
        if correlated is not None:
            raise ValueError(f"{who}: give noise= or correlated=, not both")
        if noise not in self.NOISE_MODELS:
            raise ValueError(f"{who}: noise is one of {sorted(self.NOISE_MODELS)}, not {noise!r}")
        return self.NOISE_MODELS[noise]

    def denoised_error(self, kind="denoised", floor=None, iterations=None, sigma=None, sigma_depth=None, sigma_albedo=None,
                       probes=1, epsilon=1 / 16, correlated=None, seed=0, return_map=False, return_totals=False,
                       return_probe=False, noise=None):
        """e_dn(floor): relative_error(floor)'s counterpart for the FILTERED picture -- denoised_radiance() (kind "denoised") or
        guided_radiance() ("guided") -- by Monte-Carlo SURE: the filter runs once on the picture and once per probe on a picture
        perturbed by epsilon times the estimated noise, and the response gives the filter's divergence.  render_features() first,
        error tracking on since the last reset.  `sigma` is the filter's sigma_color / sigma_luma; unset filter arguments take
        DENOISE_DEFAULTS / GUIDED_DEFAULTS.  `correlated`: perturb with independent signs (False) or with signs spread like a camera
        sample over 3 x 3 pixels (True); None takes DENOISED_ERROR_CORRELATED.  `noise` names the model instead: "independent",
        "correlated", or "split" -- a mix of the two by each pixel's light share (set_split_tracking() before the samples; DESIGN.md
        6.17); not together with `correlated`.  `seed` picks the signs: probe k of seed S is probe 0
        of seed S + k, and the same arguments give the same bytes.  The extras follow e_dn in this order: return_map the per-pixel
        estimate of the squared luma error, float32 (H,W) (0 uncovered, inf with n < 2; noisy, possibly negative); return_totals
        the eight float64 totals of cl2_denoise_error; return_probe (y', F(y), F(y')) of the last probe, float32 (H,W,3) each."""
        if kind not in self._ERROR_KINDS:
            raise ValueError(f"denoised_error: kind is one of {sorted(self._ERROR_KINDS)}, not {kind!r}")
        d = self.DENOISE_DEFAULTS if kind == "denoised" else self.GUIDED_DEFAULTS
        it = d["iterations"] if iterations is None else int(iterations)
        sg = d["sigma_color" if kind == "denoised" else "sigma_luma"] if sigma is None else float(sigma)
        sd = d["sigma_depth"] if sigma_depth is None else float(sigma_depth)
        sa = d["sigma_albedo"] if sigma_albedo is None else float(sigma_albedo)
        f = self.ERROR_FLOOR if floor is None else float(floor)
        model = self._noise_model(noise, correlated, "denoised_error")
        corr = DENOISED_ERROR_CORRELATED if correlated is None else bool(correlated)
        H, W = self.pixel_height, self.pixel_width
        out = (C.c_double * 8)()
        emap = np.empty((H, W), np.float32) if return_map else None
        probe = np.empty((3, H, W, 3), np.float32) if return_probe else None
        call, name = (self._L.cl2_denoise_error, "cl2_denoise_error") if model is None else \
                     (self._L.cl2_denoise_error_model, "cl2_denoise_error_model")
        self._check(call(self._h, self._ERROR_KINDS[kind], it, sg, sd, sa, int(probes), float(epsilon), int(corr) if model is None else model,
                         C.c_uint32(int(seed) & 0xFFFFFFFF), f, out, ptr(emap), C.c_size_t(0 if emap is None else emap.size), ptr(probe),
                         C.c_size_t(0 if probe is None else probe.size)), name)
        extras = []
        if return_map:
            extras.append(emap)
        if return_totals:
            extras.append(np.array(out[:], np.float64))
        if return_probe:
            extras.append((probe[0], probe[1], probe[2]))
        return (float(out[0]), *extras) if extras else float(out[0])

    # ---- the fixed filter's scale chosen per pixel (cl2_denoise_select, csrc/denoise_select.hpp) ----
    def _select_args(self, iterations, sigma_color, sigma_depth, sigma_albedo, probes, epsilon, correlated, seed, smooth_passes,
                     model=None):
        """the arguments the select calls share; `model`: the noise model's number in the place of `correlated`"""
        d = self.DENOISE_DEFAULTS
        return (d["iterations"] if iterations is None else int(iterations),
                d["sigma_color"] if sigma_color is None else float(sigma_color),
                d["sigma_depth"] if sigma_depth is None else float(sigma_depth),
                d["sigma_albedo"] if sigma_albedo is None else float(sigma_albedo),
                int(probes), float(epsilon),
                int(DENOISED_ERROR_CORRELATED if correlated is None else bool(correlated)) if model is None else model,
                C.c_uint32(int(seed) & 0xFFFFFFFF), SELECT_SMOOTH_PASSES if smooth_passes is None else int(smooth_passes))

    def selected_radiance(self, iterations=None, sigma_color=None, sigma_depth=None, sigma_albedo=None, probes=1, epsilon=1 / 16,
                          correlated=None, seed=0, smooth_passes=None, floor=None, return_scale=False, return_stats=False,
                          return_maps=False, noise=None):
        """`radiance` after the fixed filter with the number of passes chosen PER PIXEL: float32 (H,W,3), BGR.  One run of
        `iterations` = K passes gives the pictures of denoised_radiance(iterations=0 .. K); denoised_error's Monte-Carlo SURE
        (probes, epsilon, correlated, seed, noise as there) gives a map of the squared luma error of each; the maps are smoothed by
        `smooth_passes` passes of the filter's kernel under its normal, depth and albedo weights, and every pixel takes the level
        whose smoothed estimate is smallest.  render_features() first, error tracking on since the last reset.  Unset arguments
        take DENOISE_DEFAULTS, DENOISED_ERROR_CORRELATED and SELECT_SMOOTH_PASSES; `floor` (ERROR_FLOOR) enters the statistics only.
        The extras follow the picture in this order: return_scale the chosen pass count k*, int32 (H,W); return_stats the eight
        float64 totals of cl2_denoise_select -- [0] e_sel, [4] the summed estimate of the selected picture, [5] of the K-pass and
        [6] of the raw picture, [7] the sum of k*; return_maps (m, M), the raw and the smoothed maps, float32 (K+1,H,W) each.
        e_sel is BIASED LOW: it estimates the level that looked best, and a minimum over noisy estimates lies below the estimate
        of any fixed level, on top of the calibration limits of denoised_error.  It is a diagnostic."""
        model = self._noise_model(noise, correlated, "selected_radiance")
        a = self._select_args(iterations, sigma_color, sigma_depth, sigma_albedo, probes, epsilon, correlated, seed, smooth_passes, model)
        call, name = (self._L.cl2_denoise_select, "cl2_denoise_select") if model is None else \
                     (self._L.cl2_denoise_select_model, "cl2_denoise_select_model")
        f = self.ERROR_FLOOR if floor is None else float(floor)
        H, W = self.pixel_height, self.pixel_width
        pic = np.empty((H, W, 3), np.float32)
        scale = np.empty((H, W), np.int32) if return_scale else None
        maps = np.empty((2, max(a[0], 0) + 1, H, W), np.float32) if return_maps else None
        out = (C.c_double * 8)()
        self._check(call(self._h, *a, f, ptr(pic), C.c_size_t(pic.size), ptr(scale), C.c_size_t(0 if scale is None else scale.size), out,
                         ptr(maps), C.c_size_t(0 if maps is None else maps.size), None, C.c_size_t(0)), name)
        extras = []
        if return_scale:
            extras.append(scale)
        if return_stats:
            extras.append(np.array(out[:], np.float64))
        if return_maps:
            extras.append((maps[0], maps[1]))
        return (pic, *extras) if extras else pic

    @property
    def selected_image(self):
        """`image` of the selected radiance: tone_map(selected_radiance(), exposure=4.0) on the host, uint8 (H,W,3), BGR."""
        return tone_map(self.selected_radiance(), exposure=4.0)

    def keep_selected_picture(self, **params):
        """selected_radiance(**params) KEPT in device memory (kind "selected") under keep_picture's rules: a snapshot, nothing is
        copied to the host, a refused call leaves the previous kept picture.  `params`: iterations, sigma_color, sigma_depth,
        sigma_albedo, probes, epsilon, correlated, seed, smooth_passes, noise."""
        names = ("iterations", "sigma_color", "sigma_depth", "sigma_albedo", "probes", "epsilon", "correlated", "seed", "smooth_passes",
                 "noise")
        unknown = sorted(set(params) - set(names))
        if unknown:
            raise TypeError(f"keep_selected_picture takes {sorted(names)}, not {unknown}")
        d = dict(iterations=None, sigma_color=None, sigma_depth=None, sigma_albedo=None, probes=1, epsilon=1 / 16, correlated=None,
                 seed=0, smooth_passes=None)
        d.update(params)
        model = self._noise_model(d.pop("noise", None), d["correlated"], "keep_selected_picture")
        if model is None:
            self._check(self._L.cl2_keep_selected_picture(self._h, *self._select_args(**d)), "cl2_keep_selected_picture")
        else:
            self._check(self._L.cl2_keep_selected_picture_model(self._h, *self._select_args(**d, model=model)),
                        "cl2_keep_selected_picture_model")

    def best_iterations(self, kind="denoised", candidates=range(0, 6), **params):
        """The pass count among `candidates` whose filtered picture denoised_error(kind, iterations=..., **params) estimates to be
        the most accurate: (argmin, {iterations: e_dn}), every candidate with the same seed."""
        if "iterations" in params:
            raise TypeError("best_iterations chooses the iterations: give candidates instead")
        errs = {int(i): self.denoised_error(kind, iterations=int(i), **params) for i in candidates}
        if not errs:
            raise ValueError("best_iterations: no candidates")
        return min(errs, key=lambda i: (errs[i] if errs[i] == errs[i] else np.inf, i)), errs

    def _render_until_filtered(self, metric, target, max_samples, floor, min_samples, check_every, filter_params):
        """render_until's loop on denoised_error: cl2_run_until's chunks (first min_samples, then check_every, the last one clipped
        to max_samples), the estimate after each chunk of check_every with the check index as its seed, stop at the first
        e_dn <= target"""
        target, max_samples, min_samples, check_every = float(target), int(max_samples), int(min_samples), int(check_every)
        if not (target > 0.0 and np.isfinite(target)):
            raise ValueError("target must be positive and finite")
        if check_every < 1 or max_samples < 1 or not (0 <= min_samples <= max_samples):
            raise ValueError("check_every >= 1, 0 <= min_samples <= max_samples, max_samples >= 1")
        params = dict(filter_params or {})
        if "seed" in params:
            raise TypeError("render_until seeds every check with its index")
        if not self.error_tracking:
            self.set_error_tracking(True)
        if params.get("noise") == "split" and not self.split_tracking:
            self.set_split_tracking(True)
        try:
            self.features()
        except RendererError:
            self.render_features()
        done = 0
        if min_samples:
            self.run_samples(min_samples)
            done = min_samples
        check, e = 0, None
        while done < max_samples:
            n = min(check_every, max_samples - done)
            self.run_samples(n)
            done += n
            e, totals = self.denoised_error(metric, floor=floor, seed=check, return_totals=True, **params)
            check += 1
            # a total that is not positive is no estimate (the probe's noise or the estimator's bias exceeds it; e_dn is then 0
            # by its definition): it never stops the render
            if e <= target and totals[1] > 0.0:
                break
        if e is None:
            e = self.denoised_error(metric, floor=floor, seed=0, **params)
        return done, e

    def render_until(self, target, max_samples, floor=None, min_samples=2, check_every=8, adaptive=False, uniform_share=None,
                     metric="picture", filter_params=None):
        """Render until relative_error(floor) <= target, at most `max_samples` passes (units of run_samples: a pass renders
        one sample per stream): first `min_samples`, then chunks of `check_every`, checking after each.  Turns error tracking on
        if it is off.  adaptive=True: before every chunk the sample density is rebuilt from the error estimate
        (update_sample_density(floor, uniform_share)); the density stays set afterwards.  Returns (passes rendered, error reached).

        metric="denoised" / "guided": the error that is checked is denoised_error(metric, floor, seed=<check index>,
        **filter_params) -- the estimated error of the picture denoised_radiance() / guided_radiance() would return -- in a loop
        on the host; render_features() is called once if the handle has no current features.  A check whose weighted total is not
        positive (e_dn = 0 by definition, not by convergence) never stops the render.  Not with adaptive=True: the density update
        stays on the raw estimate.  Where the filter removes nearly all of the variance the estimate runs low (at
        10 passes of the 1080p Cornell box e_dn says 0.0086 where the filtered picture's true relative error is 0.0139, and the
        guided filter's total is negative, so that metric runs to the cap there): leave a margin in `target`.
        filter_params={"noise": "split"} checks with the split noise model (nearer the truth on that frame, and the
        guided filter's total turns positive) and turns split tracking on if it is off -- before the first sample, or the rows
        stay invalid until reset_accumulators()."""
        if metric not in ("picture", "denoised", "guided"):
            raise ValueError(f"render_until: metric is 'picture', 'denoised' or 'guided', not {metric!r}")
        if metric != "picture":
            if adaptive:
                raise ValueError("render_until: adaptive sampling follows the raw error estimate; use metric='picture' with it")
            return self._render_until_filtered(metric, target, max_samples, floor, min_samples, check_every, filter_params)
        if filter_params:
            raise ValueError("render_until: filter_params go with metric='denoised' or 'guided'")
        share = self._uniform_share(uniform_share)
        if adaptive and int(min_samples) * self.streams < 2:
            raise ValueError("adaptive sampling needs two samples per pixel before its first update: min_samples * streams >= 2")
        if not self.error_tracking:
            self.set_error_tracking(True)
        f = self.ERROR_FLOOR if floor is None else float(floor)
        done, e = C.c_int(0), C.c_double(0.0)
        self._check(self._L.cl2_set_adaptive_sampling(self._h, int(bool(adaptive)), share), "cl2_set_adaptive_sampling")
        try:
            self._check(self._L.cl2_run_until(self._h, float(target), f, int(min_samples), int(max_samples), int(check_every),
                                              C.byref(done), C.byref(e)), "cl2_run_until")
        finally:
            self.samples += done.value * self.streams
            if adaptive:
                self._L.cl2_set_adaptive_sampling(self._h, 0, share)
        return done.value, e.value

    # ---- adaptive sampling (cl2_set_sample_density ... cl2_read_camera_samples, csrc/adaptive.hpp) ----
    UNIFORM_SHARE = UNIFORM_SHARE

    def _uniform_share(self, uniform_share):
        share = self.UNIFORM_SHARE if uniform_share is None else float(uniform_share)
        if not (0.0 < share <= 1.0):
            raise ValueError("uniform_share must be in (0, 1]")
        return share

    def set_sample_density(self, density):
        """Spread each pass's camera samples over the pixels by `density` ((H, W) or W*H positive finite weights, normalised to
        mean 1): pixel q gets floor(m_q) or ceil(m_q) camera samples per pass and stream, each weighted 1/m_q, so the expected
        picture is the uniform one.  None = uniform (the default kernels).  Only run_samples / render_until render with a
        density; the stage methods refuse."""
        if density is None:
            self._check(self._L.cl2_set_sample_density(self._h, None, C.c_size_t(0)), "cl2_set_sample_density")
            return
        d = np.ascontiguousarray(density, dtype=np.float32).reshape(-1)
        if d.size != self.batch_size:
            raise ValueError(f"density must hold W*H = {self.batch_size} weights, got {d.size}")
        if not (np.all(np.isfinite(d)) and np.all(d > 0)):
            raise ValueError("density weights must be positive and finite")
        self._check(self._L.cl2_set_sample_density(self._h, ptr(d), C.c_size_t(d.size)), "cl2_set_sample_density")

    def sample_density(self):
        """The quantised density in use, float32 (H, W), mean 1 (units of 2^-16); all ones without one."""
        out = np.empty((self.pixel_height, self.pixel_width), np.float32)
        self._check(self._L.cl2_read_sample_density(self._h, ptr(out), C.c_size_t(out.size)), "cl2_read_sample_density")
        return out

    def update_sample_density(self, floor=None, uniform_share=None):
        """Set the density from the error estimate: m = beta + (1 - beta) r / mean(r), r = each pixel's term
        sqrt(var_L) / (L + floor) of relative_error(floor), clipped to 16 mean(r); beta = uniform_share (default UNIFORM_SHARE)."""
        share = self._uniform_share(uniform_share)
        f = self.ERROR_FLOOR if floor is None else float(floor)
        if not (f >= 0.0 and np.isfinite(f)):
            raise ValueError("floor must be >= 0 and finite")
        self._check(self._L.cl2_update_sample_density(self._h, f, share), "cl2_update_sample_density")

    def camera_samples(self):
        """Camera samples each pixel received since reset_accumulators(), float32 (H, W)."""
        out = np.empty((self.pixel_height, self.pixel_width), np.float32)
        self._check(self._L.cl2_read_camera_samples(self._h, ptr(out), C.c_size_t(out.size)), "cl2_read_camera_samples")
        return out

    # ---- robust picture (cl2_set_robust_buckets ... cl2_robust_picture, csrc/robust.hpp) ----
    ROBUST_BUCKETS = 8

    def set_robust_buckets(self, M=ROBUST_BUCKETS):
        """Keep M partial sums per pixel (3..16; 0 = off, the default; 16*M*W*H bytes of device memory while on): every addend of
        a pixel goes to bucket (addends so far) % M.  Switched on, or to another M, while the accumulators hold samples, the
        buckets stay invalid -- and robust_radiance() refuses -- until reset_accumulators()."""
        M = int(M)
        if M != 0 and not (3 <= M <= 16):
            raise ValueError("robust buckets: M must be 0 (off) or in 3..16")
        self._check(self._L.cl2_set_robust_buckets(self._h, M), "cl2_set_robust_buckets")

    @property
    def robust_buckets(self):
        """M, 0 while the buckets are off"""
        return int(self._L.cl2_get_robust_buckets(self._h))

    def buckets(self):
        """The bucket buffer [M][4][W*H] float32 (bucket k: rows b, g, r, w), flat."""
        a = np.empty(4 * max(self.robust_buckets, 1) * self.batch_size, np.float32)
        self._check(self._L.cl2_read_buckets_packed(self._h, ptr(a), C.c_size_t(a.size)), "cl2_read_buckets_packed")
        return a

    def load_buckets(self, a):
        """Write the bucket buffer (checkpoints: after load_packed_accumulators, which invalidates the buckets)."""
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        M = self.robust_buckets
        if M and a.size != 4 * M * self.batch_size:
            raise ValueError(f"the buckets hold 4*M*W*H = {4 * M * self.batch_size} floats, got {a.size}")
        self._check(self._L.cl2_write_buckets_packed(self._h, ptr(a), C.c_size_t(a.size)), "cl2_write_buckets_packed")

    def robust_radiance(self, return_stats=False):
        """`radiance` as a Gini-trimmed median of means over the buckets (set_robust_buckets() before the samples): float32
        (H,W,3), BGR.  Where a pixel's bucket means agree it is `radiance` up to the order of the float32 sums; a bucket that holds
        a firefly is left out.  return_stats=True returns (picture, stats): stats (H,W,2) float32 = the Gini coefficient of the
        pixel's bucket means and the number of buckets trimmed at either end."""
        out = np.empty((self.pixel_height, self.pixel_width, 3), np.float32)
        st = np.empty((self.pixel_height, self.pixel_width, 2), np.float32) if return_stats else None
        self._check(self._L.cl2_robust_picture(self._h, ptr(out), C.c_size_t(out.size), ptr(st), C.c_size_t(0 if st is None else st.size)),
                    "cl2_robust_picture")
        return (out, st) if return_stats else out

    @property
    def robust_image(self):
        """`image` of the robust radiance: tone_map(robust_radiance(), exposure=4.0) on the host, uint8 (H,W,3), BGR."""
        return tone_map(self.robust_radiance(), exposure=4.0)

    # ---- guided filter on the robust picture (cl2_denoise_robust, csrc/denoise_robust.hpp) ----
    # GUIDED_DEFAULTS, confirmed by the sweep of tools/robust_denoise_quality.py
    ROBUST_GUIDED_DEFAULTS = dict(iterations=4, sigma_luma=4.0, sigma_depth=0.1, sigma_albedo=0.1)

    def robust_guided_radiance(self, iterations=None, sigma_luma=None, sigma_depth=None, sigma_albedo=None, return_variance=False):
        """`robust_radiance()` after the variance-guided a-trous filter, its guide the variance of the mean of the buckets the trim
        kept (set_robust_buckets() before the samples, render_features() first; error tracking is not needed): float32 (H,W,3),
        BGR.  A trimmed firefly is in neither the colour nor the guide, so the filter does not open for it.  Unset arguments take
        ROBUST_GUIDED_DEFAULTS; iterations=0 returns robust_radiance() itself.  return_variance=True returns (picture, v'): v'
        (H,W) float32 is the filter's GUIDE after the last pass, not an error estimate."""
        d = self.ROBUST_GUIDED_DEFAULTS
        it = d["iterations"] if iterations is None else int(iterations)
        sl = d["sigma_luma"] if sigma_luma is None else float(sigma_luma)
        sd = d["sigma_depth"] if sigma_depth is None else float(sigma_depth)
        sa = d["sigma_albedo"] if sigma_albedo is None else float(sigma_albedo)
        out = np.empty((self.pixel_height, self.pixel_width, 3), np.float32)
        var = np.empty((self.pixel_height, self.pixel_width), np.float32) if return_variance else None
        self._check(self._L.cl2_denoise_robust(self._h, it, sl, sd, sa, ptr(out), C.c_size_t(out.size), ptr(var),
                                               C.c_size_t(0 if var is None else var.size)), "cl2_denoise_robust")
        return (out, var) if return_variance else out

    @property
    def robust_guided_image(self):
        """`image` of the filtered robust radiance: tone_map(robust_guided_radiance(), exposure=4.0) on the host, uint8 (H,W,3), BGR."""
        return tone_map(self.robust_guided_radiance(), exposure=4.0)

    def probe_math(self, which, x):
        """Device detmath / exact-reciprocal functions on a float32 array (`which`: sin cos acos atan exp asin rcp div_pi)."""
        code = ["sin", "cos", "acos", "atan", "exp", "asin", "rcp", "div_pi"].index(which)
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        self._check(self._L.cl2_probe_math(self._h, code, ptr(x), C.c_size_t(x.size), ptr(out)), "probe_math")
        return out

    def probe_bounce(self, items, from_camera=True):
        """Device bounce routines on an (n,12) float32 array {wi, n, rx, ry, ni, no, alpha, kind} -> (n,8)."""
        items = np.ascontiguousarray(items, dtype=np.float32).reshape(-1, 12)
        out = np.empty((len(items), 8), np.float32)
        self._check(self._L.cl2_probe_bounce(self._h, int(bool(from_camera)), ptr(items), C.c_size_t(len(items)), ptr(out)),
                    "probe_bounce")
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            if getattr(self, "_failed", False):
                self._L.cl2_comm_abort(self._h)
            self._L.cl2_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
