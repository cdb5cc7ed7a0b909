/* clive2_amd.h -- C ABI of the MI355X bidirectional path tracer (libclive2_amd.so).
 *
 * Drop-in boundary for the reference's Metal dispatch.  In pmclaugh/Clive2 the class
 * `Renderer` (src/renderer.py:16-352) owns ~25 `metalcompute` buffers and launches the eight
 * kernels of src/trace.metal through `dev.kernel(text).function(name)(n, *buffers)`
 * (src/renderer.py:27-37, :113-250); `create_scene` uploads nine scene buffers with
 * `dev.buffer(...)` (src/scene.py:74-89).  The entry points below are what a ctypes / cffi
 * binding of that class binds instead: plain pointers and sizes, no Python, no torch types.
 *
 *   - All record pointers use the reference's AoS layouts (src/struct_types.py:4-85):
 *     Box 48 B, Triangle 128 B, Material 48 B, Camera 112 B, Ray 128 B, Path 1040 B.
 *   - Every function returns 0 on success or a negative CL2_E_* code; cl2_last_error() returns
 *     a message for the last failure on that handle (replaces `metalcompute.error`,
 *     src/render.py:39).  No HIP failure aborts the process.
 *   - The library owns all device memory.  Host arrays passed in are copied during the call;
 *     outputs are written into caller-allocated arrays whose element counts are checked.
 *   - Calls are synchronous (they return after the stream has drained) and not re-entrant per
 *     handle; use one handle per GPU, one process (or thread) per handle.
 */
#ifndef CLIVE2_AMD_H
#define CLIVE2_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cl2_renderer cl2_renderer;

enum {
    CL2_OK = 0,
    CL2_E_INVALID = -1,      /* bad argument / scene failed validation */
    CL2_E_HIP = -2,          /* HIP runtime error (see cl2_last_error) */
    CL2_E_STATE = -3,        /* call sequence error (e.g. no scene uploaded) */
    CL2_E_NOMEM = -4,
    CL2_E_COMM = -5          /* RCCL error, or librccl could not be loaded (see cl2_last_error) */
};

/* Which subpath / ray buffer: reference `light_ray_buffer` / `camera_ray_buffer`,
 * `out_light_paths` / `out_camera_paths` (src/renderer.py:51-52, :58, :79). */
enum { CL2_LIGHT = 0, CL2_CAMERA = 1 };

/* Stage timers and tallies accumulated since cl2_reset_counters (replaces the reference's
 * `@timed` prints, src/constants.py:39-49).  One "ray" = one closest-hit BVH query =
 * one call of traverse_bvh (src/trace.metal:144).  Times are GPU milliseconds measured
 * with HIP events on the renderer's stream; they are only collected while profiling is on.
 * ms_traverse_paths = the subpath launches (closest hit + bounce per level; in the large-scene
 * organisation: the persistent traversal launches, with their bounce launches under ms_bounce). */
typedef struct {
    uint64_t rays;            /* all closest-hit queries */
    uint64_t conn_rays;       /* the subset issued by the connection stage */
    uint64_t box_tests;       /* node tests   (only counted while counting is on) */
    uint64_t tri_tests;       /* triangle tests (only counted while counting is on) */
    uint64_t counted_rays;    /* rays traced while counting was on */
    uint64_t samples;         /* completed run_sample iterations */
    double ms_generate, ms_traverse_paths, ms_bounce, ms_connect_setup, ms_traverse_conn,
           ms_connect_resolve, ms_finalize, ms_accumulate;
    uint64_t launches_traverse_paths, launches_traverse_conn;
    uint64_t rays_traverse_paths, rays_traverse_conn;   /* rays inside the timed launches */
} cl2_counters;

/* -- lifetime: replaces metalcompute.Device() + Renderer.__init__/__del__
 *    (src/scene.py:29, src/renderer.py:17-84, :318-352) -- */
int cl2_create(int device_ordinal, int pixel_width, int pixel_height, cl2_renderer** out);
void cl2_destroy(cl2_renderer* r);
const char* cl2_last_error(const cl2_renderer* r);   /* r may be NULL: error of the last failed cl2_create */
int cl2_abi_version(void);

/* -- native host BVH builder: construct_BVH + np_flatten_bvh (src/bvh.py:288-313, :329-389) in one
 *    call, O(n log n).  Inputs: per-triangle AABBs (float64, n x 3 each).  Outputs: Box records in the
 *    reference's flattened convention (capacity >= 2n-1 is always enough) and the leaf-ordered triangle
 *    permutation.  Needs no GPU.  On failure cl2_last_error(NULL) holds the message. -- */
int cl2_build_bvh(const double* tri_min, const double* tri_max, int64_t n_triangles, int max_members, int max_depth,
                  void* out_boxes, int64_t box_capacity, int64_t* n_boxes_out, int64_t* out_perm);

/* The same outputs from a GPU builder, for scenes whose set-up time matters (turntables: src/movie.py:29-55 builds one
 * scene per frame): triangles sorted along a 63-bit Morton curve of their centroids, the hierarchy above them built by
 * PLOC (every cluster merges with its nearest neighbour by union area within 8 positions along the curve, when the
 * choice is mutual; rounds until one cluster is left), subtrees of <= max_members triangles collapsed into leaves.
 * 1M triangles: 53 ms; renders a sample as fast as the reference's SAH tree (the round-2 radix tree, kept behind the
 * environment variable CLIVE2_GPU_BVH=lbvh, was 11 % slower).  Any tree in the convention renders the same picture as
 * far as the tracer is concerned; this one differs from the reference's.  The smaller child subtree is stored at left+1
 * (popped first by the traversal), which bounds the reference's traversal stack by log2(n).  Needs a GPU.  On failure
 * cl2_last_error(NULL) holds the message. */
int cl2_build_bvh_gpu(int device_ordinal, const double* tri_min, const double* tri_max, int64_t n_triangles, int max_members,
                      void* out_boxes, int64_t box_capacity, int64_t* n_boxes_out, int64_t* out_perm);
/* internal: lets the other translation units of the library leave a message for cl2_last_error(NULL) */
void cl2_set_create_error(const char* message);

/* -- scene upload: replaces the nine dev.buffer(...) uploads of create_scene
 *    (src/scene.py:74-89).  Arrays are in the reference layouts; light_* are the emitter
 *    triangle list, its areas and its indices into `triangles`. -- */
int cl2_upload_scene(cl2_renderer* r,
                     const void* boxes, int n_boxes,
                     const void* triangles, int n_triangles,
                     const void* materials, int n_materials,
                     const void* camera,
                     const void* light_triangles, const float* light_surface_areas,
                     const int32_t* light_triangle_indices, int light_count);

/* -- RNG state: the (batch,2) uint32 xorshift buffer of src/renderer.py:54,86-87 -- */
/*    n_words = 2 * streams * W * H (stream-major; see cl2_set_sample_streams) */
int cl2_set_seeds(cl2_renderer* r, const uint32_t* seeds, size_t n_words);
int cl2_get_seeds(cl2_renderer* r, uint32_t* seeds, size_t n_words);

/* -- sample streams: K independent samples of the frame per pass.  The reference's Renderer owns ONE seed buffer
 *    (src/renderer.py:54, :86-87), so K renderers -- the ranks of the sample split, SURVEY 8e -- own K; a handle with K
 *    streams holds those K buffers (seed words [2 k W H, 2 (k+1) W H) belong to stream k) and every stage call / every
 *    pass of cl2_run_samples renders one sample of EACH stream, stream k being exactly what a handle seeded with buffer k
 *    alone would render; the accumulators receive the streams' samples in stream order.  What it buys: every launch carries
 *    K x W x H work items (a per-level subpath launch of a 1080p frame is 2 M rays on 524 k resident lanes -- all tail).
 *    Default 1 = the reference's single-buffer sequence.  Needs K * W * H < 2^26.  The call frees and re-allocates the
 *    per-pixel device state (seeds return to 1; scene, accumulators and counters are kept).
 *    cl2_set_export_stream picks the stream that cl2_export_* and cl2_{ex,im}port_sample_images address. -- */
int cl2_set_sample_streams(cl2_renderer* r, int streams);
int cl2_get_sample_streams(const cl2_renderer* r);
int cl2_set_export_stream(cl2_renderer* r, int stream);

/* -- the per-sample pipeline.  The eight stage calls mirror Renderer's stage methods
 *    (src/renderer.py:113-278) for stage-level parity work; cl2_run_samples(n) is
 *    n x Renderer.run_sample (src/renderer.py:281-291) without returning to the host. -- */
int cl2_make_light_rays(cl2_renderer* r);
int cl2_make_camera_rays(cl2_renderer* r);
int cl2_trace_light_rays(cl2_renderer* r);
int cl2_trace_camera_rays(cl2_renderer* r);
int cl2_join_paths(cl2_renderer* r);
int cl2_finalize_samples(cl2_renderer* r);
int cl2_gather_light_image(cl2_renderer* r);
int cl2_process_images(cl2_renderer* r);
int cl2_run_samples(cl2_renderer* r, int n);
/* Two launch-organisation choices are MEASURED on the scene: bounces per launch for LDS-resident scenes (1 sample)
 * and the share of the machine each pipeline stage gets on large scenes (9 candidates x 6 samples, the best two twice more in turn: 54 samples, every candidate timed from device events).  By default they
 * are made inside the first cl2_run_samples call that is long enough (>= 2 / >= 66 samples); cl2_tune makes them now.
 * Its samples are real ones (seeds advance, accumulators grow, exactly as that many run_sample iterations would);
 * *samples_rendered (may be NULL) says how many.  Benchmarks call it in their warm-up.  No reference counterpart
 * (src/renderer.py:281-291 is one fixed launch sequence). */
int cl2_tune(cl2_renderer* r, int* samples_rendered);

/* Subpath levels (bounces) traced per launch: 6 walks a whole subpath in one launch with its state in
 * registers; 1 compacts the survivors after every bounce (pays when most paths die early: open
 * scenes); 0 (default) decides between 6 and 2 from the rays per subpath of the scene's first sample.
 * Results are identical for every setting. */
int cl2_set_levels_per_launch(cl2_renderer* r, int levels);
/* Traversal organisation: 1 = one ray per lane inside the subpath / connection kernels (best when the
 * tree is LDS-resident), 2 = persistent traversal launches with lane-level ray replacement + one
 * bounce launch per level (rays of very different cost: large trees), 3 = subpaths as in 1, connection
 * rays as in 2 (mid-size trees in serial order: no per-level launch tails), 4 = connection rays as in 2 and
 * both subpaths of a pixel -- light, then camera, all levels -- walked by one lane of ONE persistent launch
 * per sample, the bounces batched per wave (one launch tail instead of 24), 5 = as 2 with the connection rays walked
 * over an exact 4-wide collapse of the tree (half the dependent fetches, same decisions: csrc/bvh_wide.hpp), 0 (default)
 * = 1 for LDS-resident trees, otherwise 2 while the sample pipeline runs and 4 in serial order, with the 4-wide walk
 * for the connection rays when the tree is at most 16 MB.  Results are identical for every setting. */
int cl2_set_traversal_mode(cl2_renderer* r, int mode);
/* Sample pipeline of cl2_run_samples.  The seed buffer is the only state one sample hands to the next
 * (src/renderer.py:86-87) and only the subpath stage (K1, K2, K3) touches it, so later stages of
 * sample i can run beside the subpath stage of the following samples, on their own HIP streams and
 * buffer sets; every kernel sees the inputs of the serial order, results are the same.  The
 * reference's run_sample is strictly serial (src/renderer.py:281-291).
 *   0  serial, one stream
 *   1  two stages: subpaths of sample i+1 | connections, K6, accumulation of sample i
 *   2  three stages: subpaths of i+2 | connection set-up + connection rays of i+1 | resolve, K6,
 *      accumulation of i
 *  -1  (default) by frame size: three stages up to 2^19 pixels (small launches do not fill the
 *      machine: 256x256 runs at 10.1 / 13.9 / 18.4 Grays/s with 0 / 1 / 2), two above (equal from 1080p on) */
int cl2_set_pipelining(cl2_renderer* r, int stages);

/* -- accumulators: Renderer.summed_image / summed_sample_weights / summed_sample_counts /
 *    unidirectional_image_buffer (src/renderer.py:41-45).  Any pointer may be NULL. -- */
int cl2_read_accumulators(cl2_renderer* r, float* summed_image /*H*W*3*/, float* summed_sample_weights /*H*W*/,
                          int32_t* summed_sample_counts /*H*W*/, float* unidirectional /*H*W*3*/, size_t n_pixels);
int cl2_reset_accumulators(cl2_renderer* r);
/* -- output stage on the device: the tone map of src/camera.py:73-82 applied to one of the three pictures of
 *    src/renderer.py:293-316, straight from the accumulators (6 MB instead of 66 MB leave the device per 1080p frame;
 *    the host does no per-pixel work).  which: 0 `image` (summed_image / summed_sample_weights), 1 `unweighted_image`,
 *    2 `unidirectional_image`; all scrubbed with nan_to_num(neginf=0, posinf=0) and computed in the dtypes numpy's
 *    promotion gives the reference (csrc/tonemap.hpp).
 *      cl2_tone_log_sum   sum over the pixels of log(0.1 + luma) in float64 (the reference: np.sum(log_tone_sums));
 *                         the caller forms Lw = exp(sum / (H*W)) -- with numpy's exp if it wants numpy's last bit
 *      cl2_tone_map       (255 * result / (result + white_point^2)).astype(uint8), result = image * exposure / Lw, as
 *                         H*W*3 bytes, b, g, r per pixel
 *    Deterministic (fixed reduction tree).  The float64 sum is added in another order than numpy's pairwise sum, so Lw
 *    can differ from the host path's in its last bits; a byte of the picture changes only where 255*x/(x+w) lies within
 *    ~1e-13 of an integer.  `Renderer.image` keeps the host path (byte-exact against the reference's fixture);
 *    `Renderer.tone_mapped()` and movie.py use this one. -- */
int cl2_tone_log_sum(cl2_renderer* r, int which, double* sum_out);
int cl2_tone_map(cl2_renderer* r, int which, double exposure, double white_point, double log_average /* Lw */,
                 uint8_t* out_bgr, size_t n_bytes /* 3*H*W */);
/* packed planar form [8][H*W] = image b,g,r | weights | unidirectional b,g,r | counts(float):
 * the message of the multi-GPU sum-reduce, as host arrays (checkpointing, CPU-side tests). */
int cl2_read_accumulators_packed(cl2_renderer* r, float* host_dst, size_t n_floats);
int cl2_write_accumulators_packed(cl2_renderer* r, const float* host_src, size_t n_floats);

/* -- multi-GPU sample split (the reference is single-device, src/renderer.py:281-291).
 *    Samples are i.i.d. and the accumulators are pure sums (src/renderer.py:269-273): every rank
 *    renders its own samples of the replicated scene with its own seed buffer, then ONE in-place RCCL
 *    all-reduce (sum, float32) of the packed accumulators [8][H*W] combines them (66 MB at 1080p, over
 *    xGMI).  One communicator per handle, one handle per GPU, one process (or thread) per handle.
 *    librccl is loaded (dlopen) by the first of these calls; a failure is CL2_E_COMM, never fatal.
 *
 *      rank 0:  cl2_comm_get_unique_id(id)  -> hand the cl2_comm_unique_id_bytes() bytes to every rank
 *               (file, socket, launcher: the caller's business; clive2_amd/distributed.py uses a file)
 *      all   :  cl2_comm_init_rank(r, nranks, rank, id)      (collective: returns when all have called)
 *               ... cl2_run_samples(r, n_rank) ...
 *               cl2_reduce_accumulators(r)                  (collective; every rank then holds the sums)
 *               cl2_comm_destroy(r)                         (also done by cl2_destroy)
 *    failure:   cl2_comm_abort(r) on the rank that failed; the others get CL2_E_COMM from the collective -- */
int cl2_device_count(void);                          /* HIP devices visible to this process (0 on error) */
int cl2_synchronize(cl2_renderer* r);                /* drains the handle's streams, then the device */
int cl2_comm_unique_id_bytes(void);
int cl2_comm_get_unique_id(void* out_id, size_t n_bytes);           /* error text: cl2_last_error(NULL) */
int cl2_comm_init_rank(cl2_renderer* r, int nranks, int rank, const void* unique_id, size_t n_bytes);
/* With error tracking (cl2_set_error_tracking) the moment buffer is reduced too.  So that ranks which disagree never issue
 * different collectives, the call first all-reduces every rank's tracking state (cl2_comm_allreduce_f64, op max over [t, -t]):
 * one small collective more than the accumulators' all-reduce, whether tracking is on or not.  If tracking is on on some ranks
 * and off on others, the accumulators are reduced as usual, the moments are marked invalid everywhere and the call returns
 * CL2_E_STATE; moments invalid on any rank are invalid on every rank after the sum.
 * The robust buckets (cl2_set_robust_buckets) ride on the same handshake: when every rank has them on with the same M the bucket
 * buffer is reduced too (bucket k of the job = the sum of the ranks' buckets k: independent samples, the same estimator), and the
 * result is valid if it was valid on every rank.  If the ranks disagree (off on some, or another M), what is reduced without
 * buckets is reduced, the buckets are marked invalid on every rank and the call returns CL2_E_STATE. */
int cl2_reduce_accumulators(cl2_renderer* r);
/* n <= 16 host doubles, in place, op 0 = sum, 1 = max over the ranks: barrier, max-over-ranks clock,
 * whole-job ray tally, error-flag agreement before the collective */
int cl2_comm_allreduce_f64(cl2_renderer* r, double* values, int n, int op);
int cl2_comm_destroy(cl2_renderer* r);
/* No collective blocks for ever: the wait for an enqueued all-reduce polls the stream and ncclCommGetAsyncError under
 * a deadline (CLIVE2_COMM_TIMEOUT_S seconds, default 300); on a timeout or an asynchronous error the communicator is
 * torn down with ncclCommAbort and the call returns CL2_E_COMM (the handle stays usable for local work, its
 * communicator is gone).  A rank that fails locally calls cl2_comm_abort before it exits, so that its peers do not
 * have to wait for their deadline; cl2_comm_destroy / cl2_destroy abort instead of destroying when the handle is in
 * a failed state. */
int cl2_comm_abort(cl2_renderer* r);

/* What the communicator reports about itself (ncclCommCount / ncclCommUserRank / ncclCommCuDevice) and which GPU this
 * handle sits on (hipDeviceGetPCIBusId): the evidence that an N-rank job really spanned N devices (bench.py gathers the
 * addresses of all ranks into its JSON line).  Without a communicator nranks is 0 and the device fields are still filled. */
typedef struct {
    int32_t nranks, rank;           /* from the communicator; 0 / 0 without one */
    int32_t comm_device;            /* the device ordinal RCCL bound the communicator to */
    int32_t device_ordinal;         /* the ordinal this handle was created on */
    int64_t pci_address;            /* domain << 16 | bus << 8 | device << 3 | function */
    char pci_bus_id[32];            /* "0000:c1:00.0" */
} cl2_comm_info_t;
int cl2_comm_info(cl2_renderer* r, cl2_comm_info_t* out);

/* How the library organises the launches for the uploaded scene (all organisations give identical results;
 * this is what the automatic choices of cl2_set_traversal_mode / _levels_per_launch / _pipelining came to). */
typedef struct {
    int32_t tree_in_lds;            /* whole tree + all triangles staged in LDS by every workgroup (<= 512 records, <= 512 triangles) */
    int32_t persistent_subpaths;    /* subpath levels run as persistent traversal launches (+ one bounce launch per level) */
    int32_t persistent_connections; /* connection rays run as one persistent traversal launch */
    int32_t two_tris_per_step;      /* persistent walk tests two triangles per step (trees up to 16 MB) */
    int32_t n_records;              /* node records (>= reference boxes: leaves above 16 triangles are split) */
    int32_t n_lds_records;          /* records in the LDS window */
    int32_t n_top_renumbered;       /* boxes of the top levels numbered first so that the window holds them (0 = plain visit order) */
    int32_t lds_triangles;
    int32_t levels_per_launch;      /* effective subpath levels per launch */
    int32_t paths_share;            /* tuned share of the wave slots for the subpath stage, eighths (0 = not tuned yet, 9 = serial order won) */
    int32_t pipeline_stages;        /* effective setting of cl2_set_pipelining */
    int32_t wide_connections;       /* connection rays walk the exact 4-wide collapse of the tree (csrc/bvh_wide.hpp) */
    int32_t wide_nodes;             /* nodes of that collapse (0: not available: hand-made boxes that do not nest, leaves above 16 triangles) */
    int32_t pruned_records;         /* records of the pruned table of an LDS-resident tree (inner boxes whose test costs more than it saves are
                                       dropped: exact for rays with finite 1/d); 0: none */
    int64_t tree_bytes;             /* 32 B per record + 48 B per intersection triangle */
    int32_t sample_streams;         /* cl2_set_sample_streams */
    int32_t staged_bytes;         /* dynamic LDS of a launch that stages the tree: records, triangles with their pad records, pruned table */
} cl2_organisation;
int cl2_query_organisation(cl2_renderer* r, cl2_organisation* out);

/* -- counters / profiling -- */
int cl2_set_profiling(cl2_renderer* r, int level);  /* HIP-event timers: 0 off, 1 the traversal launches only (connection rays, subpath rays), 2 every stage */
/* mode 1: node / triangle test tallies of the REFERENCE's walk (src/trace.metal:144-176; the traversal kernels then run the
 * binary stackless walk, whose tests are the reference's one for one) -> cl2_counters.box_tests / tri_tests / counted_rays.
 * mode 2: what the exact 4-wide walk ITSELF fetches -> cl2_read_walk_tallies (the launches are the ones that run uncounted,
 * except that single run_sample() calls take the per-level organisation).  0: off. */
int cl2_set_counting(cl2_renderer* r, int mode);
int cl2_read_counters(cl2_renderer* r, cl2_counters* out);
typedef struct cl2_walk_tally {
    uint64_t rays, wide_visits, tri_records, stack_spills, binary_records;
} cl2_walk_tally;
typedef struct cl2_walk_tallies { cl2_walk_tally subpath, connection; } cl2_walk_tallies;
int cl2_read_walk_tallies(cl2_renderer* r, cl2_walk_tallies* out);
/* Launch-organisation switches for experiments and tests.  None of them changes a result.
 *   bit 3       accepted and ignored (rounds 2-3: the per-level subpath launches took the 4-wide walk in the serial order too; they
 *               always do since round 4)
 *   bits 4-6    7 = the second implementation of the resolve kernel, one wave per camera vertex (only in the test variant
 *               of the library); other values are refused
 *   bit 7       walk the full record table of an LDS-resident tree instead of the pruned one
 *   bits 8-10   eighths of the wave slots given to the subpath stage while the sample pipeline runs (0 = tuned)
 *   bit 11      walk a pruned table that is a plain list of leaves per lane instead of wave-uniformly (csrc/bvh_traverse.hpp,
 *               closest_hit_flat)
 *   bit 12      invert the one/two-triangles-per-step choice of the persistent walk
 *   bit 13      4-wide walk WITHOUT the speculative expansion of the stack top (round 5: a lane that is testing triangles expands
 *               the wide node on top of its stack in the same pass, csrc/bvh_wide.hpp): the pass as round 4 had it, for A/B runs and tests
 *   bit 14      4-wide walk with the 48-byte triangle records of the other walks (six 16-byte loads per pair) instead of its own
 *               36-byte ones, a pair fetched as one run of 72 bytes (five loads; round 6, csrc/bvh_wide.hpp: PACK), for A/B runs and tests
 *   bits 16-19  accepted and ignored (round 3: stack entries per lane in LDS of the 4-wide walk; a compile-time 8 since round 4)
 *   bits 20-23  4-wide walk: LDS window of the top of the wide tree in units of 32 nodes (0 = by tree size: 32 nodes, 64 when
 *               the tree streams from memory; 15 = no window)
 *   bit 25      connection rays of a tree wholly staged in LDS with a flat pruned table: the set-up launch and the walk
 *               launch over a global tag queue (csrc/kernels.hpp: k_connect_setup, k_traverse_conn) instead of the fused
 *               launch with a workgroup-local queue (k_connect_walk_lds), for A/B runs and tests
 *   bit 26      flat pruned table of an LDS-resident tree (closest_hit_flat): the loop with the next-record index clamped on the
 *               scalar unit and the leaf record read in three steps (closest_hit_flat_clamped) instead of the one that keeps the
 *               record address in a vector register and fetches past the last triangle into pad records, for A/B runs and tests
 *   bit 27      resolve stage: launch k_connect_resolve, the kernel that holds every register of its SIMDs, where the slim one
 *               that leaves room for a wave of the subpath stage would run (csrc/connect_resolve.hpp: k_connect_resolve_slim),
 *               for A/B runs and tests
 * Any other bit is refused (CL2_E_INVALID).  Bits 0-2 exist ONLY in the test variant of the library
 * (libclive2_amd_test.so, -DCL2_TEST_VARIANT), where they switch parts of the resolve stage off for timing
 * dissections -- bit 0 the t = 1 splat atomics, bit 1 / bit 2 the t >= 2 / t == 1 strategy pairs -- and make the
 * render INVALID; the shipped library refuses them. */
#define CL2_DEBUG_KNOWN_BITS 0x0EFF7FFF
int cl2_set_debug_flags(cl2_renderer* r, int flags);
/* Reproducible light image, off by default.  The reference's light-image chain (sort by target pixel, per-pixel gather:
 * src/renderer.py:97-111, :213-250, src/trace.metal:872-964) is deterministic; the float atomics that replace it add a pixel's
 * contributions in hardware order, so two renders agree to a few ulp only.  on = 1: k_connect_resolve writes the reference's
 * records (slot id + s * total_pixels), one radix sort orders them by (target pixel, s, source pixel) and each target's run is
 * summed front to back -- two renders of the same scene and seeds give identical bytes in all four accumulators.
 * Memory: 32 B x 6 x B of records, keys and slot ids (B = sample streams x W x H entries; the sort runs over 6 x B keys) plus
 * rocPRIM's temporary storage -- 0.4 GB at 1920 x 1080 with one stream, 12.7 GB at 3840 x 2160 with 8.  Refused together with
 * debug bits 4-6 = 7 (the test variant's cross-check resolve kernel writes no records). */
int cl2_set_reproducible(cl2_renderer* r, int on);
int cl2_get_reproducible(const cl2_renderer* r);
/* Child order of the 4-wide walks (ABI 5).  order = 0 (default): the reference's fixed order -- a box's second child is popped first,
 * whatever the ray (src/trace.metal:157-160) -- which is what makes every output byte-comparable with the reference's.  order = 1:
 * the passing children of a node are taken NEAREST FIRST (by slab entry distance).  A closest-hit query then prunes what lies behind
 * its first hit: fewer node visits and triangle tests per ray.  NOT the reference's result by construction -- the reference's hit
 * depends on its visit order where a hit lies a few ulp in front of its own leaf box's entry distance (the leaf is entered or not
 * depending on what was found before it, trace.metal:152); two triangles hit at exactly the same t (first visited wins,
 * trace.metal:170) ARE settled as the reference settles them (a table of each triangle's position in its visit order) -- so: opt-in,
 * never the default, never the parity path; bench.py's headline and every parity test run with 0, and tests/test_gpu_round6.py /
 * test_gpu_fullsize.py count the rays whose hit differs (2 to 5 in 3.4e8) and check that each is such a hit.  Applies to
 * scenes whose tree is read through the caches (the 4-wide walk; an LDS-resident tree such as the Cornell box renders the same
 * either way).  No reference counterpart (src/trace.metal:144-176 has one order). */
int cl2_set_traversal_order(cl2_renderer* r, int order);
int cl2_get_traversal_order(const cl2_renderer* r);
/* The 4-wide walk keeps a per-lane stack whose pushes are not clamped: the library sizes it from the uploaded tree and the child
 * order -- order 0 from the depth of the reference's stack, order 1 from the tree's deepest sum of (slots - 1) over a path of its
 * 4-wide collapse, which no walk in any order exceeds.  A tree whose bound for order 1 is beyond the stack's cap is refused
 * (CL2_E_INVALID) by cl2_set_traversal_order(1), and by cl2_upload_scene while order 1 is set; order 0 takes every tree
 * cl2_upload_scene accepts.  cl2_wide_stack_capacity: the entries a lane has for the current scene and order (0: no scene, or
 * no 4-wide collapse). */
int cl2_wide_stack_capacity(const cl2_renderer* r);
/* What a connection ray asks of the tree (additions to ABI 6).  mode = 0 (default): its closest hit, as the reference
 * (src/trace.metal:144-176).  mode = 1: for a pair with t >= 2 the resolve stage reads one bit of that result -- whether the hit
 * triangle is the camera vertex's triangle T -- so the ray becomes a VISIBILITY query seeded with T: T is tested first, the walk
 * prunes with T's distance from the root on and stops at the first blocker (csrc/bvh_wide.hpp, VIS, has the definition and why it
 * does not depend on the visit order).  The six t = 1 slots and rays with a zero direction component stay closest-hit queries,
 * byte for byte.  NOT the reference's result by construction: the verdict differs where a hit lies in front of its own leaf box's
 * entry distance, the order dependence cl2_set_traversal_order documents -- so: opt-in, never the default, never the parity path.
 * Applies wherever connection rays take the 4-wide walk; cl2_connection_query_active says whether the uploaded scene's connection
 * launch really runs the seeded walk (0 for a tree that is resident in LDS, for a tree without a 4-wide collapse, and while
 * cl2_set_counting(1) is on).  Other modes are CL2_E_INVALID and leave the setting alone.  Refused (CL2_E_INVALID), whichever
 * comes second: mode 1 with cl2_set_traversal_order(1), mode 1 with debug bit 13 or 14.  No reference counterpart. */
int cl2_set_connection_query(cl2_renderer* r, int mode);
int cl2_get_connection_query(const cl2_renderer* r);
int cl2_connection_query_active(const cl2_renderer* r);
/* Whole-subpath launch (traversal mode 4): lanes that must have gathered with a known closest hit before a wave runs
 * its bounce phase, and the steps the first of them waits at most.  0 = default (32 lanes, 48 steps).  Same results. */
int cl2_set_subpath_gather(cl2_renderer* r, int lanes, int wait_steps);
int cl2_reset_counters(cl2_renderer* r);

/* Exactness self-test: the kernels replace `1.0f/a` and `x/PI` by cheaper sequences that are proven
 * (exhaustively, over all 2^32 binary32 inputs) to return the correctly rounded IEEE result; this call
 * re-runs that proof on the device and returns the number of inputs that disagree (must be 0, 0). */
int cl2_selftest_exact_math(cl2_renderer* r, uint64_t* rcp_mismatches, uint64_t* divpi_mismatches);

/* Elementwise probe of the device's deterministic elementary functions: which = 0 sin, 1 cos, 2 acos,
 * 3 atan, 4 exp, 5 asin (csrc/detmath.hpp), 6 rcp_exact, 7 div_pi (csrc/vecmath.hpp).  Host arrays. */
int cl2_probe_math(cl2_renderer* r, int which, const float* in, size_t n, float* out);
/* Elementwise probe of the bounce routines (src/trace.metal:226-233, :254-264, :334-379).  in: 12 floats per
 * item {wi.xyz, n.xyz, rx, ry, ni, no, alpha, kind}, kind 0 diffuse / 1 reflect / 2 transmit / 3 GGX_sample
 * only; out: 8 floats {wo.xyz, f, c_p, l_p, fresnel(wi,m), m.x} with m = GGX_sample(n, rx, ry, alpha). */
int cl2_probe_bounce(cl2_renderer* r, int from_camera, const float* in, size_t n, float* out);

/* -- debug exports in the reference's AoS layouts (stage-level parity) -- */
int cl2_export_rays(cl2_renderer* r, int which, void* out_rays, size_t n_records);        /* Ray[batch]  */
int cl2_export_paths(cl2_renderer* r, int which, void* out_paths, size_t n_records);      /* Path[batch] */
int cl2_export_aggregators(cl2_renderer* r, void* out, size_t n_records);                 /* 128-B stride */
/* the connection stage's results of the last join_paths: per pixel the strategy-pair mask (bit (t-1)*6 + (s-1): the pair
 * passed the culls and has a ray), the closest-hit triangle of every pair (int32[36][n_pixels], slot-major; meaningful where
 * the mask bit is set) and the hit distance of the six t = 1 pairs (float[6][n_pixels]).  Any pointer may be NULL.
 * Under cl2_set_connection_query(1), where it is active, `tri` of a t >= 2 pair holds the camera vertex's triangle T where T is
 * visible and another value where it is not (the first blocker met, or -1 where the ray misses T): only `tri == T` means anything. */
int cl2_export_connections(cl2_renderer* r, uint64_t* cmask, int32_t* tri, float* t1, size_t n_pixels);
/* per-sample images: finalized_samples (float4), out_light_image rgb + summed light weight (float4),
 * sample_weights (K6 value only), out_camera_image (float4).  Any pointer may be NULL. */
int cl2_export_sample_images(cl2_renderer* r, float* finalized4, float* light4, float* sample_weights,
                             float* unidirectional4, size_t n_pixels);
/* the inverse of cl2_export_sample_images: per-sample images from host arrays (float4 / float per pixel),
 * so that the accumulation stage (process_images, src/renderer.py:253-278) can be checked on its own
 * against arrays produced by the reference's numpy code.  Any pointer may be NULL. */
int cl2_import_sample_images(cl2_renderer* r, const float* finalized4, const float* light4, const float* sample_weights,
                             const float* unidirectional4, size_t n_pixels);
/* closest-hit probe: n rays as Ray records -> (triangle, t, u, v) per ray; exercises the traversal
 * kernel alone (src/trace.metal:144-176). */
int cl2_probe_traverse(cl2_renderer* r, const void* rays, size_t n_rays, int32_t* best_i, float* best_t,
                       float* u, float* v);

/* visibility probe: n rays as Ray records with one target triangle each, every ray through the seeded walk of
 * cl2_set_connection_query(1) (whatever that setting is).  Per ray the stored triangle and its distance: (T, t_T) where the target is
 * visible, the first blocker met and its t where it is not, (-1, +inf) where the ray misses T.  target < 0: the plain closest hit,
 * as cl2_probe_traverse.  target >= the scene's triangle count: CL2_E_INVALID.  CL2_E_STATE when the scene has no 4-wide collapse
 * or debug bit 13 is set. */
int cl2_probe_visibility(cl2_renderer* r, const void* rays, size_t n_rays, const int32_t* target, int32_t* out_tri, float* out_t);

/* -- denoiser: first-hit guide buffers and an edge-avoiding a-trous filter (csrc/denoise.hpp).  No reference counterpart:
 *    the reference's picture is the raw estimate (src/renderer.py:293-316).  Neither call touches the sample pipeline: the
 *    seeds, accumulators, counters, walk tallies and profiling timers stay exactly as they were. --
 *
 * cl2_render_features: per pixel of the W x H frame (independent of the sample streams), `samples` camera rays and their
 * closest hits, averaged into two float4 buffers
 *     G0 = (shading normal x, y, z, depth)      G1 = (albedo b, g, r, coverage)
 * normal = normalize(sum of the hits' shading normals, each turned to face its ray) or 0; depth and albedo (the material
 * colour) = means over the rays that hit; coverage = hits / samples; a pixel without hits is all 0.  `seeds` has the
 * (W*H, 2) layout of cl2_set_seeds with one stream (n_words = 2*W*H); the pass draws from a private copy, sample k
 * continuing the xorshift state of sample k-1, so with samples = 1 its rays are exactly the ones cl2_make_camera_rays
 * makes from the same seeds.  The features hold until the next cl2_upload_scene. */
int cl2_render_features(cl2_renderer* r, const uint32_t* seeds, size_t n_words, int samples);
/* Both feature buffers as W*H float4 each (n_pixels = W*H).  CL2_E_STATE without current features. */
int cl2_read_features(cl2_renderer* r, float* g0, float* g1, size_t n_pixels);
/* The counterpart of cl2_read_features (ABI 6), for features made elsewhere, checkpoints and tests: allocates the feature set if
 * there is none, copies both W*H float4 arrays as they are and makes them the current features of the uploaded scene (they hold
 * until the next cl2_upload_scene, like rendered ones).  Touches nothing of the sample pipeline.  The filters expect what
 * cl2_render_features makes: finite values, coverage 0 where nothing was hit.  CL2_E_INVALID for a NULL array or n_pixels
 * other than W*H. */
int cl2_write_features(cl2_renderer* r, const float* g0, const float* g1, size_t n_pixels);
/* The filtered radiance, (H, W, 3) float32 b, g, r (n_floats = 3*W*H), from the accumulators in place (read, not changed).
 * Input c = scrub(summed_image / summed_sample_weights) (Renderer.radiance); `iterations` passes i = 0, 1, ... with step
 * s = 2^i: a pixel with coverage 0 passes through, every other one becomes sum(w c_q) / sum(w), or keeps its colour when
 * sum(w) is not greater than 0 (0 for a zero normal; NaN when sigma_depth z_p s is 0, that is depth 0 or an underflow),
 * over the taps q = p + s (dx, dy), dx, dy in -2..2 (dy outer), that lie in the frame and have coverage, with
 *     w = h(dx) h(dy) max(0, n_p.n_q)^32 exp(-|z_p - z_q| / (sigma_depth z_p s)) exp(-|a_p - a_q|^2 / sigma_albedo^2)
 *         exp(-|x_p - x_q|^2 / (sigma_color^2 4^-i)),   h = (1, 4, 6, 4, 1) / 16,   x = c / (1 + luma(c)).
 * Defaults of the Python binding: iterations 3, sigma_color 2.0, sigma_depth 0.1, sigma_albedo 0.1, settled on the Cornell
 * box and the glass scene at 256 x 192 and 4 samples against 1024-sample pictures: relative MSE 0.29 and 0.26 of the raw
 * picture's (5 passes over-blur the Cornell box's lighting, 0.72; sigma_color 0.6 leaves the glass noisy, 0.49).
 * iterations in 0..12 (0 = the input);
 * sigmas positive and finite, and neither sigma_albedo^2 nor, with iterations >= 1, sigma_color^2 4^-(iterations-1) (the float32
 * values the passes divide by) below FLT_MIN: a denominator that underflowed to 0 or to a subnormal is refused, not
 * trusted; else CL2_E_INVALID.  CL2_E_STATE without current features (none rendered, or a scene uploaded since). */
int cl2_denoise(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo, float* out_bgr,
                size_t n_floats);

/* -- error estimates: per-pixel standard errors and "render until the noise is below X" (csrc/error_estimate.hpp).  No
 *    reference counterpart.
 *
 * An ADDEND is what one sample stream of one pass adds to one pixel: x_c = the value added to accumulator row c (c = 0, 1, 2 =
 * b, g, r: scrub(light + finalized)), w = the value added to row 3 (sample weight + light weight), and
 * y = (x_b 0.0722 + x_g 0.7152) + x_r 0.2126 (float32).  While tracking is on, a moment buffer [8][W*H] of float32 sums gets
 *     x_c^2 (rows 0..2), w^2 (3), x_c w (4..6), y^2 (7)
 * from every addend, in stream order, one float32 add per row (the kernels are built with -ffp-contract=off).
 * The picture is the ratio Sum x / Sum w; its per-pixel standard error by the delta method (float64), n = acc row 7:
 *     Wt = acc row 3 not finite or <= 0: uncovered, 0 and not part of the frame metric;  n < 2: +inf;
 *     else I_c = X_c / Wt,  S_c = max(0, m_c - 2 I_c m_{4+c} + I_c^2 m_3),  var_c = n S_c / ((n - 1) Wt^2),
 *     luma likewise from L = luma(I), m_7 and luma(m_4, m_5, m_6).
 * Frame metric e(floor) = sqrt((1/N) sum_covered var_L / (L + floor)^2) over the N covered pixels (+inf if N = 0 or a covered
 * pixel has n < 2; a pixel with var_L = 0 adds 0), reduced in a fixed order on the device: the same bytes on every call.
 *
 * Tracking is off by default; with it off every kernel runs exactly the code it runs without this feature.  Turning it on
 * allocates and zeroes the moment buffer (32 W H bytes of device memory: 66 MB at 1080p) and costs the accumulation one more
 * read and write of it per pass; turning it off frees it.  The moments are VALID when every addend in the accumulators also
 * went into them: cl2_reset_accumulators zeroes them and makes them valid; turning tracking on while the accumulators hold
 * samples, or cl2_write_accumulators_packed, leaves them invalid until a reset (or, after a write, cl2_write_moments_packed).
 * Every call below but the first two returns CL2_E_STATE while tracking is off or the moments are invalid (writing needs
 * tracking on only). -- */
int cl2_set_error_tracking(cl2_renderer* r, int on);
int cl2_get_error_tracking(const cl2_renderer* r);
/* the moment buffer [8][W*H] as host floats, for checkpoints and tests (n_floats = 8*W*H); writing makes the moments valid */
int cl2_read_moments_packed(cl2_renderer* r, float* host_dst, size_t n_floats);
int cl2_write_moments_packed(cl2_renderer* r, const float* host_src, size_t n_floats);
/* (H, W, 4) float32 standard errors b, g, r, luma (n_floats = 4*W*H) */
int cl2_read_standard_error(cl2_renderer* r, float* out, size_t n_floats);
/* The variance-guided filter (csrc/denoise_guided.hpp): cl2_denoise's a-trous passes, with the colour edge-stop
 * replaced by one that compares luma differences with the centre pixel's standard error.  Everything float32.  Input per pixel:
 * c as cl2_denoise forms it, and v = (float) min(var_L, 2^100) with var_L the float64 luma variance above (the square of
 * cl2_read_standard_error's luma before its rounding); v = 2^100 where n < 2, v = 0 where the pixel is uncovered (Wt not
 * finite or <= 0).  Pass i (step s = 2^i), for a pixel p with feature coverage != 0:
 *     vbar_p = sum g(dy) g(dx) v_q / sum g(dy) g(dx) over the 3 x 3 around p (offsets -1..1, NOT scaled by s; g = (1/4, 1/2, 1/4);
 *              taps inside the frame with coverage != 0)
 *     den_l  = sigma_luma sqrt(vbar_p) + 1e-8,     l(x) = (x.b 0.0722 + x.g 0.7152) + x.r 0.2126 on the raw colour
 *     w_q    = h(dx) h(dy) w_n w_z w_a exp(-|l(c_p) - l(c_q)| / den_l)          (h, w_n, w_z, w_a: cl2_denoise's)
 *     c'_p   = sum w_q c_q / sum w_q,              v'_p = sum w_q^2 v_q / (sum w_q)^2
 * over the taps q = p + s (dx, dy), dx, dy in -2..2 (dy outer), in the frame and with coverage; a pixel without coverage or with
 * sum w = 0 keeps c and v.  sigma_luma is the same in every pass (the shrinking v' narrows the filter).  Where the estimate says
 * "converged" the filter closes (v = 0 everywhere returns the input); a firefly has a huge v of its own, accepts every neighbour
 * and is averaged away, while its neighbours reject it.
 * out_bgr: (H, W, 3), n_floats = 3*W*H.  out_var: NULL (n_var = 0) or W*H floats (n_var = W*H) that receive v' of the last pass
 * (v itself with iterations = 0).  v' treats the taps as independent, which holds for the first pass only: it is the filter's
 * GUIDE, NOT an error estimate of the filtered picture -- it underestimates that picture's squared error by a factor of 10 to 100.
 * Defaults of the Python binding (Renderer.GUIDED_DEFAULTS): iterations 4, sigma_luma 4.0, sigma_depth 0.1, sigma_albedo 0.1, settled on
 * the Cornell box and the glass scene at 256 x 192 against 1024-sample pictures: relative MSE 0.09 and 0.21 of the raw picture's at 4
 * passes, 0.38 and 0.13 at 256 (the fixed filter: 0.29 and 0.26 at 4 passes, 14 and 0.30 at 256).  iterations in 0..12 (0 = the
 * input); sigmas positive and finite, sigma_albedo^2 (float32) not below FLT_MIN as for cl2_denoise; else CL2_E_INVALID.
 * CL2_E_STATE without current features, with error tracking off, or with invalid moments.
 * Touches neither seeds, accumulators, moments, counters nor walk tallies; works with sample streams, with a sample density
 * and after cl2_reduce_accumulators (the moments are valid in all three). */
int cl2_denoise_guided(cl2_renderer* r, int iterations, float sigma_luma, float sigma_depth, float sigma_albedo, float* out_bgr,
                       size_t n_floats, float* out_var, size_t n_var);
/* e(floor), floor >= 0 and finite */
int cl2_relative_error(cl2_renderer* r, double floor, double* out);
/* The error of the FILTERED picture (csrc/denoise_error.hpp): Monte-Carlo SURE, Stein's unbiased risk estimate with the
 * filter's divergence taken from finite differences along `probes` random perturbations.  No reference counterpart: the reference has
 * neither a filter nor an error estimate (src/renderer.py:293-316).  kind 0: the passes of cl2_denoise (sigma = sigma_color), kind 1:
 * those of cl2_denoise_guided (sigma = sigma_luma), launched as those calls launch them.  Per pixel p, with err_pixel's state and
 * float64 variances (cl2_read_standard_error) and y the float32 colour cl2_denoise filters:
 *     v_p = (float) min(var_L, 2^100)    s_p = (float) sqrt(v_p)    d_p,c = (float)(se_c / luma(se)), 1 when luma(se) is not > 0 or
 *     not finite    a_p,c = s_p d_p,c (0 where the pixel is uncovered or has n < 2)      -- rank-1 colour noise of luma variance v_p
 *     b_q = sign bit of a hash of (pixel index q, seed + probe)      z = b (correlated 0), or b passed through the mean 3 x 3
 *     reconstruction weights of a camera sample and normalised to E z^2 = 1 over the in-frame sources (correlated 1)
 *     y' = y + (epsilon z) a   (float32)      u = luma(y') - luma(y)      g = luma(F(y')) - luma(F(y))            (float64)
 *     div_p = sum_probes u g / (epsilon^2 probes)          sure_p = (luma(F(y)) - luma(y))^2 - v_p + 2 div_p
 * out[8]: [0] e_dn = sqrt(max(0, [1] / N)), +inf when N = 0 or [3] > 0; [1] sum over estimated pixels of
 * sure_p / (luma(F(y)_p) + floor)^2 (a sure_p of exactly 0 adds 0); [2] N = covered pixels; [3] covered pixels with n < 2;
 * [4] sum sure_p; [5] sum of the fidelity terms; [6] sum v_p; [7] sum 2 div_p.  The sums are taken in a fixed order without atomics:
 * the same bytes on every call.  e_dn(floor) is cl2_relative_error's e(floor) for the filtered picture; with iterations 0 and
 * correlated 0 it is e(floor) up to the rounding of y + delta.
 * out_map: NULL (n_map 0) or W*H floats: 0 uncovered, +inf with n < 2, else (float) sure_p -- noisy and possibly negative for a
 * single probe; the totals are what is calibrated.  out_probe: NULL (n_probe 0) or 3*(3*W*H) floats that receive y', F(y) and
 * F(y') of the LAST probe, (H, W, 3) each; F(y) is cl2_denoise's / cl2_denoise_guided's picture byte for byte.
 * Limits: the weight 1 / (luma F + floor)^2 depends on the data (as e(floor)'s does); for kind 1 the guide variance is treated as a
 * fixed parameter of the filter; the estimate is unbiased under its own noise model and badly off under the other one (DESIGN 6.15
 * has both modes measured on real renders: at 64 x 48 independent signs give estimate / true error 0.88 .. 1.20; on the 1080p
 * Cornell box, where the filter removes 98 % of the variance, the truth lies between the modes, independent signs run low -- e_dn
 * by a factor of up to 1.6 -- and for kind 1 the total is negative).
 * Arguments: iterations and sigmas as the filter's own call checks them; probes 1..16; epsilon > 0 and finite (the Python binding:
 * 1/16); correlated 0 or 1; floor >= 0 and finite; else CL2_E_INVALID.  CL2_E_STATE without current features, with error tracking off
 * or with invalid moments.  Touches neither seeds, accumulators, moments, counters, a kept picture nor the guide variance of the
 * last cl2_denoise_guided. */
int cl2_denoise_error(cl2_renderer* r, int kind, int iterations, float sigma, float sigma_depth, float sigma_albedo, int probes,
                      float epsilon, int correlated, uint32_t seed, double floor, double* out, float* out_map, size_t n_map,
                      float* out_probe, size_t n_probe);
/* Renders until e(floor) <= target.  Units are passes, as for cl2_run_samples(n): first min_passes, then chunks of check_every
 * (the last one clipped to max_passes), each through cl2_run_samples; after each chunk e(floor) is evaluated on the device, and
 * the call stops at the first chunk boundary with e <= target, or at max_passes.  *passes_done = passes rendered (also when the
 * call fails part way), *error_out = the last e (evaluated once at the end if no chunk ran); either pointer may be NULL.
 * target > 0 and finite, floor >= 0 and finite, check_every >= 1, 0 <= min_passes <= max_passes, max_passes >= 1. */
int cl2_run_until(cl2_renderer* r, double target, double floor, int min_passes, int max_passes, int check_every, int* passes_done,
                  double* error_out);

/* Adaptive sampling (clive2_amd/csrc/adaptive.hpp).  A density m (W*H positive weights, normalised to mean 1 and
 * quantised to units of 2^-16) spreads each sample stream's W*H camera slots over the pixels: pixel q gets floor(m_q) or
 * ceil(m_q) of them per pass and stream, E = m_q, contiguous and in raster order, and each of its camera samples enters the
 * picture with the factor 1/m_q -- so the expected picture is the uniform one.  The light image, acc row 7 (one addend per pixel
 * and stream) and the moments keep their meaning.  Only cl2_run_samples / cl2_tune / cl2_run_until render with a density; one
 * rank only.
 *   - density NULL: uniform, the default kernels byte for byte.  Any density set explicitly, a flat one included, runs the
 *     mapped kernels.  CL2_E_INVALID for a NaN, +-inf or <= 0 weight or n != W*H.
 *   - While a density is set the stage calls cl2_make_light_rays ... cl2_process_images and the test variant's cross-check
 *     resolve (debug bits 4-6 = 7) return CL2_E_STATE.
 *   - Every density call returns CL2_E_STATE on a handle with a communicator, and cl2_comm_init_rank refuses a handle with a
 *     density or adaptive sampling on.
 *   - cl2_upload_scene keeps the density (it describes pixels, not the scene); cl2_set_sample_streams keeps it and re-allocates
 *     the slot maps with the other per-stream state. */
int cl2_set_sample_density(cl2_renderer* r, const float* density, size_t n);
/* the quantised density in use (M_q / 2^16 rounded to float: exact below 256); 1.0 everywhere without one */
int cl2_read_sample_density(cl2_renderer* r, float* out, size_t n);
/* Density from the error estimate: r_q = sqrt(var_L) / (L + floor) per pixel (0 uncovered; +inf with fewer than two addends),
 * clipped to 16 mean(r) (mean over the finite terms), m_q = uniform_share + (1 - uniform_share) r_q / mean(r).  CL2_E_STATE while
 * the moments are invalid (cl2_read_standard_error's rule) or when no term is finite.  floor >= 0, uniform_share in (0, 1]. */
int cl2_update_sample_density(cl2_renderer* r, double floor, double uniform_share);
/* on: cl2_run_until calls cl2_update_sample_density(floor, uniform_share) after min_passes and before every chunk; it then needs
 * min_passes * streams >= 2 (else CL2_E_INVALID).  Off (the default): cl2_run_until is unchanged. */
int cl2_set_adaptive_sampling(cl2_renderer* r, int on, double uniform_share);
int cl2_get_adaptive_sampling(const cl2_renderer* r);
/* camera samples each pixel received since the last cl2_reset_accumulators (one per stream and pass without a density) */
int cl2_read_camera_samples(cl2_renderer* r, float* out, size_t n);

/* -- robust picture: a Gini-trimmed median of means over per-pixel buckets (csrc/robust.hpp).  No reference
 *    counterpart.
 *
 * While the buckets are on, a buffer bkt [M][4][W*H] of float32 sums (bucket k: rows b, g, r, w) gets every addend (x_0, x_1, x_2,
 * w) of the error estimates' definition above: bucket k = (int)a7 % M with a7 = the pixel's accumulator row 7 before the addend,
 * rows 4k + c += x_c and 4k + 3 += w, one float32 add each, in stream order.  Accumulators and moments get the bytes they get
 * without buckets.  The picture, per pixel, in float64 from the float32 sums, every operation in the order written:
 *     bucket k is valid iff W_k > 0 and W_k < +inf;  m = valid buckets;  m = 0: the pixel is 0, 0, 0
 *     key_k = (I_b 0.0722f + I_g 0.7152f) + I_r 0.2126f with I_c = X_ck / W_k;  a NaN key counts as +inf
 *     rank the valid buckets by key ascending, equal keys in bucket order
 *     over the ranks j = 1 .. m:  v_j = key > 0 ? key : 0,  S += v_j,  N += (2j - m - 1) v_j
 *     G = 1 if S is NaN or +inf, 0 if !(S > 0), else N / (m S) (0 if !(G > 0), 1 if G > 1)         -- the Gini coefficient
 *     c = min(floor(G m / 2), (m - 1) / 2) (integer division);  kept = ranks c+1 .. m-c
 *     X_c, W = float32 sums over the kept buckets in ascending bucket index;  pixel = scrub(X_c / W) in float32, BGR
 * Where the bucket means agree nothing is trimmed and the pixel is the plain ratio estimator; a bucket that holds a firefly is
 * dropped, with the smallest one.
 *
 * Off by default; with it off every kernel runs exactly the code it runs without this feature.  M = 0 switches off and frees the
 * buffer; M = 3 .. 16 switches on (16 M W H bytes of device memory: 265 MB at 1080p with M = 8), zeroed; another M than the
 * current one frees, allocates and zeroes; anything else is CL2_E_INVALID.  The buckets are VALID when every addend in the
 * accumulators also went into them, by the rules of the moments: valid when switched on (or resized) over clean accumulators,
 * after cl2_reset_accumulators (which zeroes them) and after cl2_write_buckets_packed; invalid when switched on or resized over
 * accumulators that hold sums and after cl2_write_accumulators_packed. -- */
int cl2_set_robust_buckets(cl2_renderer* r, int M);
int cl2_get_robust_buckets(const cl2_renderer* r);               /* M, 0 = off */
/* the bucket buffer [M][4][W*H] as host floats, for checkpoints and tests (n_floats = 4*M*W*H, else CL2_E_INVALID); CL2_E_STATE
 * with the buckets off; reading works on invalid buckets too, writing makes them valid */
int cl2_read_buckets_packed(cl2_renderer* r, float* host_dst, size_t n_floats);
int cl2_write_buckets_packed(cl2_renderer* r, const float* host_src, size_t n_floats);
/* out_bgr: (H, W, 3) float32, n_floats = 3*W*H.  out_stats: NULL (n_stats = 0) or (H, W, 2) float32 (n_stats = 2*W*H) that
 * receive (float)G and (float)c per pixel.  CL2_E_STATE with the buckets off or invalid (the message says how to make them
 * valid).  Touches neither seeds, accumulators, moments, buckets nor counters. */
int cl2_robust_picture(cl2_renderer* r, float* out_bgr, size_t n_floats, float* out_stats, size_t n_stats);
/* The variance-guided filter on the robust picture (csrc/denoise_robust.hpp): cl2_denoise_guided's passes, unchanged, on
 * an input made from the buckets alone.  Per pixel:
 *     trim      valid, key_k (float64, a NaN key is +inf), ranks, m, G, c and the kept set exactly as stated above
 *     colour    c = the pixel of cl2_robust_picture, byte for byte (float32 sums over the kept buckets in ascending bucket index,
 *               divided and scrubbed; 0, 0, 0 at m = 0)
 *     variance  n = m - 2c, the number of kept buckets;  v = 0 for m = 0;  v = 2^100 for n < 2;  otherwise, in float64 over the kept
 *               buckets in ascending bucket index:
 *                   ybar = (sum key_k) / (double)n,   Q = sum (key_k - ybar) (key_k - ybar),   var = (Q / (double)(n - 1)) / (double)n
 *               v = var < 2^100 ? (float)var : 2^100     (a NaN or inf from a +inf key takes the cap)
 * v is the between-bucket variance of the mean of the kept bucket lumas: a firefly that was trimmed is in neither c nor v, so the
 * filter does not open for it.  v ignores that the buckets' weights differ; it is a filter GUIDE, like v' of cl2_denoise_guided,
 * and nothing may stop on it.
 * Arguments, outputs and their checks are cl2_denoise_guided's (iterations 0..12, 0 = the input: the robust picture and v; sigmas
 * positive and finite, sigma_albedo^2 not below FLT_MIN; out_var NULL with n_var 0, or W*H floats; else CL2_E_INVALID).
 * CL2_E_STATE without current features, with the buckets off or with invalid buckets (cl2_robust_picture's messages).  Error
 * tracking need not be on: neither accumulators nor moments are read.  Touches neither seeds, accumulators, moments, buckets,
 * features nor counters; allocates the filters' working buffers only.  Defaults of the Python binding:
 * Renderer.ROBUST_GUIDED_DEFAULTS. */
int cl2_denoise_robust(cl2_renderer* r, int iterations, float sigma_luma, float sigma_depth, float sigma_albedo, float* out_bgr,
                       size_t n_floats, float* out_var, size_t n_var);

/* ---- a kept picture and its tone map on the device (csrc/tonemap_picture.hpp) ----
 * The handle can keep ONE picture in device memory: (H, W, 3) float32 b, g, r, 12*W*H bytes, allocated on first use.  Its kind:
 *     0 none   1 denoised (cl2_denoise)   2 guided (cl2_denoise_guided)   3 robust (cl2_robust_picture)
 *     4 robust-guided (cl2_denoise_robust)   5 loaded (cl2_write_picture)
 *     6 one filtered layer, 7 the sum of the filtered layers (cl2_keep_layer_picture, below: cl2_keep_picture makes neither)
 * It is a snapshot: it holds until it is replaced, dropped (kind 0) or the handle is destroyed; later samples, resets and scene
 * uploads do not change it.
 *
 * cl2_keep_picture, kinds 1..4: exactly the launches of the call named above, with the same argument checks, the same CL2_E_STATE
 * conditions and the same messages; the last launch writes into the kept picture instead of the call's own output buffer, and
 * nothing is copied to the host.  `sigma` is sigma_color for kind 1 and sigma_luma for kinds 2 and 4; kind 3 ignores the four filter
 * arguments.  Kind 0 drops the picture and frees its buffer; any other kind is CL2_E_INVALID.  A refused call leaves the previous
 * kept picture as it was; a HIP failure part way through leaves kind 0.  The call touches what the corresponding call above
 * touches (the filters' working buffers) and the kept picture, nothing else.
 * cl2_kept_picture: the kind; 0 for none or a NULL handle (a plain read of the handle: no device work).
 * cl2_write_picture / cl2_read_picture: the picture as host floats, n_floats = 3*W*H (else CL2_E_INVALID); writing makes kind 5.
 * cl2_picture_log_sum / cl2_picture_tone_map: cl2_tone_log_sum and cl2_tone_map for the kept picture.  Per pixel, f the picture's
 * float32 value, c the channel:
 *     base_c = (double)f_c    luma = (base_b * 0.0722 + base_g * 0.7152) + base_r * 0.2126    term = log(0.1 + luma)
 *     pre_c = (double)(f_c * (float)exposure)  (a float32 product)    result = pre_c / Lw    v = 255 * result / (result + white_point^2)
 *     byte = cl2_tone_map's cast of v
 * This is picture 0's arithmetic WITHOUT the scrub, as the host path tone_map(picture) has none: a NaN pixel makes the log sum NaN
 * and the picture all zero bytes, exactly as on the host.  The sum is added in cl2_tone_log_sum's order (same workgroups, same tree).
 * n_bytes = 3*W*H.  The two share the partial-sum and byte buffers of cl2_tone_log_sum / cl2_tone_map.
 * cl2_read_picture, cl2_picture_log_sum and cl2_picture_tone_map return CL2_E_STATE without a kept picture; NULL pointers and wrong
 * sizes are CL2_E_INVALID.  All calls but cl2_kept_picture drain the handle's streams first.  None of them touches seeds,
 * accumulators, moments, buckets, features or counters. */
int cl2_keep_picture(cl2_renderer* r, int kind, int iterations, float sigma, float sigma_depth, float sigma_albedo);
int cl2_kept_picture(const cl2_renderer* r);
int cl2_write_picture(cl2_renderer* r, const float* bgr, size_t n_floats);
int cl2_read_picture(cl2_renderer* r, float* out_bgr, size_t n_floats);
int cl2_picture_log_sum(cl2_renderer* r, double* sum_out);
int cl2_picture_tone_map(cl2_renderer* r, double exposure, double white_point, double log_average /* Lw */, uint8_t* out_bgr,
                         size_t n_bytes);

/* ---- strategy mask: render any subset of the (s, t) connection strategies (csrc/connect_resolve.hpp STRAT) ----
 * A pixel-sample is a sum over the strategy pairs (s, t): s = light vertices used (0..6), t = camera vertices used (1..6),
 * s + t >= 2.  Pair (s, t) owns bit (t - 1) * 7 + s of a 64-bit mask: 41 valid bits (CL2_STRATEGY_ALL); the other 23 are dropped on
 * set and read back as 0.  The default is all 41 set.
 * While a pair's bit is clear, everything the reference computes for the pair is still computed -- the culls, the connection ray, the
 * visibility verdict, the MIS weight w -- and w still goes where it goes today: aggregator row 12 (contrib_weight_sum) for t >= 2,
 * the .w of the light-image splat or record for t = 1.  Only the COLOUR is left out: for t >= 2 the pair is not added to
 * total_contribution; for t = 1 the splat or record carries colour (+0, +0, +0) with its w.  The picture is the ratio sum x / sum w,
 * so keeping every w makes masked pictures a decomposition: for masks that partition the 41 pairs the pictures add up to the full
 * one, to float rounding.
 * NOT touched: the filter weights (aggregator rows 0..8), row 12, the light weight, the unidirectional estimate, the seeds and the
 * random numbers drawn (renders from the same seeds walk the same paths whatever the mask), the ray counters -- no connection ray is
 * skipped, a masked pair's w needs its verdict.  Moments, robust buckets, the sample density and the denoisers see the masked
 * addends (x masked, w full) and describe the masked picture.
 * A full mask runs the default kernels (byte-identical to a handle that never set one); a partial one runs the masked instantiations
 * of k_connect_resolve, at the occupancy of their default counterparts (no scratch).  The mask survives cl2_upload_scene, cl2_set_sample_streams and
 * cl2_reset_accumulators and applies to cl2_join_paths and to cl2_run_samples / cl2_tune / cl2_run_until alike.  A partial mask is
 * refused together with debug bits 4-6 = 7, whichever is set second (CL2_E_INVALID, the earlier setting is kept): the test variant's
 * cross-check resolve kernel has no masked form.  In a multi-rank job every rank must set the same mask: that is the caller's
 * business and is not checked.  NULL handle or NULL mask_out: CL2_E_INVALID.
 * No reference counterpart (src/trace.metal:649-825 sums all pairs). */
#define CL2_STRATEGY_BIT(s, t)  ((uint64_t)1 << (((t) - 1) * 7 + (s)))
#define CL2_STRATEGY_ALL        ((uint64_t)0x3FFFFFFFFFE)   /* the 41 valid bits: bits 1..41, (0, 1) is not a pair */
int cl2_set_strategy_mask(cl2_renderer* r, uint64_t mask);
int cl2_get_strategy_mask(const cl2_renderer* r, uint64_t* mask_out);

/* ---- layer accumulators: the layers of ONE render (csrc/layers.hpp, csrc/connect_resolve.hpp LAYERS) ----
 * A layer table assigns each of the 41 (s, t) pairs to at most one of n_layers <= CL2_MAX_LAYERS layers: masks[l] is the mask of
 * layer l in the bit layout of cl2_set_strategy_mask (pair (s, t) = bit (t - 1) * 7 + s; bits outside the 41 are dropped).  The masks
 * must be pairwise disjoint (else CL2_E_INVALID); they need not cover all pairs (a pair in no layer adds to no layer) and an empty
 * mask is a legal layer whose accumulator stays +0.  NULL / 0 switches the table off (the default).
 * While a table is set, every pass fills the ordinary accumulators, moments, buckets, seeds and ray counters with the bytes of a
 * pass without one, and additionally L colour accumulators lacc[L][3][W*H] (b, g, r): lacc[l] receives what rows 0..2 of the
 * accumulators receive in a render with cl2_set_strategy_mask(masks[l]) -- the same float operations on the same operands in the
 * same order, so with cl2_set_reproducible(1) the same bytes, and with float atomics the same sums in the hardware's order.  The
 * picture of layer l is nan_to_num(lacc[l] / accumulator row 3): the denominator is shared, which is why layers that partition the 41
 * pairs add up to the full picture, to float rounding.
 * Memory while set: 24 (+ 4 unused) bytes per layer and entry (streams x W x H), 12 per layer and pixel.  The per-entry buffers are
 * allocated by cl2_set_layers and again by cl2_set_sample_streams; the table survives cl2_upload_scene, cl2_set_sample_streams and
 * cl2_reset_accumulators, which zeroes lacc.
 * Validity follows the moment buffer's rule: lacc is valid only if every sample in the ordinary accumulators since their last reset
 * was rendered under this table.  Setting a DIFFERENT table on a handle that holds samples zeroes lacc and marks it invalid until
 * cl2_reset_accumulators (setting the table it already has changes nothing); so does cl2_write_accumulators_packed, until
 * cl2_write_layers_packed, which makes it valid.  cl2_read_layers_packed returns CL2_E_STATE while invalid or without a table.
 * n_floats = n_layers * 3 * W * H, layer-major, then b, g, r planes (else CL2_E_INVALID).  cl2_get_layers writes up to `capacity`
 * masks and returns n_layers.
 * Refused, whichever call comes second (CL2_E_STATE or CL2_E_INVALID, the earlier setting is kept, the message names the way out):
 * a table together with a partial strategy mask; with a sample density or adaptive sampling (there is no mapped form); with debug
 * bits 4-6 = 7 (the cross-check resolve kernel); more than CL2_MAX_LAYERS layers.  Error tracking, robust buckets, the
 * reproducible switch, sample streams, every traversal organisation, pipelining and the visibility-query walk combine with a table
 * and describe the full picture as before.
 * OUT OF SCOPE: cl2_reduce_accumulators neither reduces nor refuses the layer accumulators -- a multi-rank host sums
 * cl2_read_layers_packed itself (every rank must set the same table).  There are no per-layer moments or buckets.  The layers
 * have a filter and, through the kept picture, a device tone map of their own: cl2_denoise_layers and cl2_keep_layer_picture below.
 * No reference counterpart (src/trace.metal:649-825 sums all pairs). */
#define CL2_MAX_LAYERS 8
int cl2_set_layers(cl2_renderer* r, const uint64_t* masks, int n_layers);          /* NULL / 0 = off (the default) */
int cl2_get_layers(const cl2_renderer* r, uint64_t* masks_out, int capacity);      /* returns n_layers */
int cl2_read_layers_packed(cl2_renderer* r, float* host_dst, size_t n_floats);     /* [L][3][W*H], b g r */
int cl2_write_layers_packed(cl2_renderer* r, const float* host_src, size_t n_floats);

/* ---- the filter over the layers of one render (csrc/denoise_layers.hpp) ----
 * cl2_denoise_layers filters every layer of the table in one call and adds the results.  Layer l's colour is
 * c_l = scrub(lacc[l] / accumulator row 3) and goes through cl2_denoise's a-trous passes with its own sigma_color[l]; sigma_depth and
 * sigma_albedo are shared.  Per pixel and layer these are cl2_denoise's float operations on the same operands in the same order:
 * out_layers[l] holds the bytes cl2_denoise(iterations, sigma_color[l], ...) returns on a handle with the same features whose
 * accumulator rows 0..2 are lacc[l].  The part of a tap weight that has no colour in it -- B3-spline, normal, depth, albedo -- is
 * computed once per tap and pass and shared by the layers.  out_sum = F_0, then + F_l for l = 1 .. L-1: one float32 add per
 * component, in layer order.  iterations = 0 returns the layer pictures themselves (Renderer.layer_radiance() on the device).
 * Either output may be NULL, not both; n_layer_floats = n_layers*3*W*H ([L][H][W][3], b, g, r), n_sum_floats = 3*W*H.
 * Checks: cl2_denoise's for every sigma_color[l] (iterations in 0..12, positive finite sigmas, the two underflow refusals);
 * CL2_E_INVALID also for a NULL handle (nothing is dereferenced), a NULL sigma_color, both outputs NULL, a wrong size, and for
 * cl2_keep_layer_picture a layer outside -1..L-1; CL2_E_STATE without a layer table, while lacc is invalid (cl2_read_layers_packed's
 * condition and message) and without current features.
 * cl2_keep_layer_picture: the same launches for one layer (only that layer is filtered) or, with layer = -1, for the sum; the result
 * becomes the KEPT picture (kind 6 / 7) under cl2_keep_picture's rules: a snapshot, nothing is copied to the host, a refused call
 * leaves the previous kept picture, a HIP failure part way through leaves kind 0.  cl2_read_picture, cl2_picture_log_sum and
 * cl2_picture_tone_map serve kinds 6 and 7 like any other; cl2_keep_picture(0) drops them; cl2_keep_picture still takes 0..4 only.
 * Memory: two working buffers of n_layers*W*H float4, 32 bytes per layer and pixel (1080p: 199 MB with 3 layers, 531 MB with 8),
 * allocated by the first of these calls and released when the table changes, is switched off or the handle is destroyed.
 * Both calls drain the handle's streams and write only these buffers and, for the second, the kept picture: accumulators, lacc,
 * moments, buckets, seeds, features, counters and the buffers of cl2_denoise are read at most. */
int cl2_denoise_layers(cl2_renderer* r, int iterations, const float* sigma_color /* [n_layers] */, float sigma_depth,
                       float sigma_albedo, float* out_layers /* [L][H][W][3] b, g, r, or NULL */, size_t n_layer_floats,
                       float* out_sum /* (H, W, 3), or NULL */, size_t n_sum_floats);
int cl2_keep_layer_picture(cl2_renderer* r, int layer /* 0..L-1, or -1 = the sum */, int iterations,
                           const float* sigma_color /* [n_layers] */, float sigma_depth, float sigma_albedo);

#ifdef __cplusplus
}
#endif
#endif
