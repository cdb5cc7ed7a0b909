// renderer_api.hip -- host side of libclive2_amd.so: device-memory ownership, scene repacking,
// launch sequencing on one HIP stream, HIP-event stage timers, and the extern "C" entry points
// declared in include/clive2_amd.h.
//
// Stage order and buffer roles follow Renderer.run_sample (src/renderer.py:281-291); what differs
// is where the state lives (SoA on the device, accumulators included) and that nothing returns to
// the host between samples.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <limits>
#include <chrono>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/clive2_amd.h"
#include "../../include/clive2_amd_ext.h"
#include "kernels.hpp"
#include "denoise.hpp"
#include "denoise_error.hpp"
#include "denoise_guided.hpp"
#include "denoise_layers.hpp"
#include "denoise_robust.hpp"
#include "denoise_select.hpp"
#include "error_estimate.hpp"
#include "error_split.hpp"
#include "adaptive.hpp"
#include "layers.hpp"
#include "tonemap.hpp"
#include "tonemap_picture.hpp"
#include "det_splat.hpp"
#include "bvh_builder.hpp"
#include "comm_rccl.hpp"
#include "comm_wait.hpp"
#include "scene_prep.hpp"

using namespace cl2;

namespace {

thread_local std::string g_create_error;

enum Stage { ST_GENERATE, ST_TRAVERSE_PATHS, ST_BOUNCE, ST_CONNECT_SETUP, ST_TRAVERSE_CONN, ST_CONNECT_RESOLVE,
             ST_FINALIZE, ST_ACCUMULATE, ST_COUNT };

}  // namespace

struct cl2_renderer {
    // B = ENTRIES of every per-pixel array = streams x FB (cl2_set_sample_streams; kernels.hpp header): what every launch covers
    // and every stride is; FB = W x H, the pixels of the frame: accumulators, tone map, the multi-GPU reduce, exports of one stream
    int device = 0, W = 0, H = 0, B = 0, FB = 0;
    int streams = 1;                     // independent samples of the frame per pass (one seed buffer each, as K Renderers would hold)
    int export_stream = 0;               // the stream the debug exports / sample-image calls address
    hipStream_t stream = nullptr;        // subpath phase (and everything else when not pipelining)
    hipStream_t stream_conn = nullptr;   // sample pipeline: connection set-up + connection rays
    hipStream_t stream_res = nullptr;    // sample pipeline: resolve + K6 + accumulation
    hipEvent_t ev_paths[3] = {}, ev_conn[2] = {}, ev_res[6] = {};
    hipEvent_t ev_tune[2] = {};          // share tuner: end of the first / of the last sample of a candidate's run (timing events)
    double tune_period_ms = 0.0;         // ... and what they measured: ms per sample between the two
    bool pipe_active = false;            // inside a pipelined cl2_run_samples
    int paths_share = 0;                 // eighths of the wave slots given to the subpath stage while pipelining (0 = not tuned yet)
    int pipelining = -1;                 // sample pipeline inside cl2_run_samples: 0 serial, 1 two stages, 2 three stages, -1 by frame size
    std::string err;
    bool scene_ok = false;
    int counting = 0;                    // 0 off, 1 the reference walk's node / triangle tallies (binary walk), 2 the 4-wide walk's own tallies
    int profiling = 0;                   // 0 off, 1 the connection-ray traversal launch only, 2 every stage
    int debug_flags = 0;
    int traversal_order = 0;             // 0 = the reference's child order (exact); 1 = nearest child first in the 4-wide walks (opt-in, NOT bit-exact: bvh_wide.hpp ORDER)
    int gather_lanes = 32, gather_wait = 48;   // whole-subpath launch: lanes gathered / steps waited before a wave runs its bounce phase
    int traversal_mode = 0;              // 0 auto, 1 fused (one ray per lane), 2 split (persistent traversal + ray replacement)
    unsigned* d_work = nullptr;          // [8][WORK_STRIDE] work counters of the persistent traversal launches, a 64-byte line per launch slot
    int levels_per_launch = 0;           // subpath levels per launch (6 = one launch, 1 = compaction after every bounce, 0 = by survival)
    int levels_auto = 0;                 // the choice made for levels_per_launch == 0 (0 = not made yet)

    // scene
    BvhView bvh{};
    float4 *d_nodes = nullptr, *d_tris = nullptr, *d_tri_shade = nullptr, *d_light_tris = nullptr;
    int* d_light_tri_index = nullptr;
    float* d_light_areas = nullptr;
    MaterialDev* d_mats = nullptr;
    int n_mats = 0, light_count = 0;
    int n_top = 0;                       // boxes of the top levels renumbered to the front of the record array (0: plain visit order)
    // 4-wide collapse of the tree for the exact wide walk (bvh_wide.hpp); n_wide == 0: not available for this scene
    float4* d_wide = nullptr;
    int n_wide = 0;
    int connection_query = 0;            // 0 = connection rays are closest-hit queries; 1 = the t >= 2 ones are visibility queries seeded with their target (opt-in: bvh_wide.hpp VIS)
    int* d_tri_rank = nullptr;           // ORDER, VIS: each triangle's position in the reference's visit order (exact-t ties; bvh_wide.hpp)
    float* d_tris36 = nullptr;           // 36-byte triangle records of a tree that streams from beyond L2 (bvh_wide.hpp, PACK); nullptr: none
    int n_fast = 0;                      // records of the pruned table (bvh.n_fast_nodes unless debug_flags bit 7 switches it off)
    CamTris cam_tris{0, {0, 0, 0, 0}};   // the triangles with is_camera set, as kernel arguments of the resolve stage (n < 0: too many, look them up)
    int fast_flat = 0;                   // the pruned table is a plain list of leaves (bvh.fast_flat unless debug_flags bit 11 switches it off)
    float4* d_fast = nullptr;            // pruned record table of an LDS-resident tree (scene_prep.hpp); bvh.n_fast_nodes == 0: none
    WideView wide{};
    int2* d_wide_ovf = nullptr;          // per-lane stack overflow of the wide launches (one region per stage: [2]); allocated by the first wide launch
    int wide_ovf_entries = 0;            // entries per lane: wide_overflow_entries of this tree in the CURRENT child order (cl2_upload_scene, cl2_set_traversal_order)
    int max_pending = 0, order_depth = 0; // the uploaded tree's two stack depths (scene_prep.hpp): what that size is computed from
    CameraRec cam{};

    // state
    uint2* d_seeds = nullptr;
    PathBufs sets[3][2]{};             // subpath buffer sets of the sample pipeline
    int cur = 0;                       // the set stage calls and exports use (after run_samples: the last sample's)
    float4* d_hit = nullptr;
    float4* d_hit_cam0 = nullptr;      // closest hits of the camera subpaths' first rays, traced together with the light subpaths' (launch_trace)
    int* d_queue = nullptr;            // [6][B], shared by both subpath kinds (they run one after the other)
    unsigned* d_qcount = nullptr;      // [9]: [0] = B (level-0 count), [1..6] level counts, [7] connection rays, [8] = 2B
    int* d_ctag = nullptr;             // connection-ray queue: {slot, pixel} tags
    // reproducible light image (cl2_set_reproducible, det_splat.hpp): records of one pass, allocated on first use
    bool reproducible = false;
    uint64_t strategy_mask = CL2_STRATEGY_ALL;   // cl2_set_strategy_mask: the (s, t) pairs whose colour is kept (connect_resolve.hpp STRAT)
    // layer accumulators (cl2_set_layers, layers.hpp): the table, its per-entry buffers [L][3][B] / [L][B] and the sums [L][3][W*H]
    int n_layers = 0;                    // 0 = off (the default)
    uint64_t layer_masks[CL2_MAX_LAYERS] = {};
    LayerCodes lcodes{};                 // the table as the resolve kernel takes it
    float* d_lay_agg = nullptr;
    float4* d_lay_light = nullptr;
    float* d_lacc = nullptr;
    bool lay_valid = false;              // every sample in the accumulators was rendered under this table (the rules of mom_valid)
    float4* d_ldn[2] = {nullptr, nullptr};   // the layers' filter (cl2_denoise_layers, denoise_layers.hpp): ping-pong [L][W*H], made on first use
    unsigned *d_det_keys = nullptr, *d_det_keys_sorted = nullptr, *d_det_slots = nullptr, *d_det_slots_sorted = nullptr;
    float4* d_det_vals = nullptr;
    void* d_det_tmp = nullptr;
    size_t det_tmp_bytes = 0;
    float2* d_chit[2] = {nullptr, nullptr};            // two sets: connection rays of sample i+1 vs resolve of sample i
    unsigned long long* d_cmask[2] = {nullptr, nullptr};
    float* d_agg = nullptr;
    float4 *d_light_image = nullptr, *d_finalized = nullptr, *d_uni = nullptr;
    float* d_sample_w = nullptr;
    float* d_acc = nullptr;            // [8][B]
    double* d_tone_partial = nullptr;  // device tone map: per-workgroup partial sums + the total (allocated by the first call)
    uint8_t* d_tone_out = nullptr;     // device tone map: the uint8 picture before it is copied out
    float* d_pic = nullptr;            // kept picture (cl2_keep_picture, tonemap_picture.hpp): (H, W, 3) b, g, r, allocated on first use
    int pic_kind = 0;                  // ... 0 none, 1 denoised, 2 guided, 3 robust, 4 robust-guided, 5 loaded (cl2_write_picture), 6 layer, 7 sum of layers (cl2_keep_layer_picture), 8 selected (cl2_keep_selected_picture)
    Stats* d_stats = nullptr;
    unsigned long long* d_block_stats = nullptr;   // [grid][4]: rays, box tests, tri tests, counted rays per workgroup slot

    // host-side tallies
    uint64_t samples = 0, counted_rays = 0;
    double ms[ST_COUNT] = {0};
    uint64_t launches_tp = 0, launches_tc = 0, rays_tp = 0, rays_tc = 0;
    struct Span { hipEvent_t a, b; int stage; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> event_pool;

    std::vector<void*> allocs;

    // multi-GPU sample split: one RCCL communicator per handle (cl2_comm_init_rank)
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_nranks = 0;
    bool comm_poisoned = false;          // a collective failed or timed out (or the host said so): tear down with ncclCommAbort
    double* d_comm_scratch = nullptr;    // [COMM_SCRATCH] doubles for cl2_comm_allreduce_f64

    // first-hit features and the denoiser (denoise.hpp): W x H entries each, allocated by the first cl2_render_features
    uint2* d_feat_seeds = nullptr;       // private copy of the caller's seed buffer (d_seeds is never touched)
    float4 *d_feat_o = nullptr, *d_feat_d = nullptr, *d_feat_hit = nullptr;
    float4 *d_g0 = nullptr, *d_g1 = nullptr;   // {normal, depth}, {albedo b, g, r, coverage}
    unsigned* d_feat_count = nullptr;    // [1] = W x H: the ray count of the traversal launches
    unsigned* d_feat_work = nullptr;     // [WORK_STRIDE]: work counter of the 4-wide walk
    Stats* d_feat_stats = nullptr;       // ray tally of the feature launches: kept apart from d_stats (cl2_read_counters)
    bool features_valid = false;         // cleared by cl2_upload_scene
    float4* d_dn[2] = {nullptr, nullptr};   // ping-pong colour of the filter passes
    float* d_dn_out = nullptr;           // (H, W, 3) result of the last pass
    float* d_dn_var = nullptr;           // (H, W) guide variance after the last pass of cl2_denoise_guided (denoise_guided.hpp)
    // the error estimate of the filtered picture (cl2_denoise_error, denoise_error.hpp), allocated by its first call
    float4 *d_de_y = nullptr, *d_de_a = nullptr, *d_de_yp = nullptr;   // y, A = (a, code), y' of the current probe
    float* d_de_fy = nullptr;            // (H, W, 3) F(y); F(y') is the filters' d_dn_out
    float* d_de_map = nullptr;           // (H, W) the per-pixel estimate
    double* d_de_sum = nullptr;          // [W*H] sum over the probes of u g, then [DE_SUMS][ERR_BLOCKS] partials + [8] result
    // the per-pixel choice among the fixed filter's scales (cl2_denoise_select, denoise_select.hpp), allocated by its first call
    // and again when K grows
    int ds_levels = 0;                   // K + 1 the buffers below are sized for; 0: none
    float4* d_ds_lev = nullptr;          // [2][levels][W*H] L_j(y), then L_j(y') of the current probe
    float4* d_ds_a = nullptr;            // A = (a, code) of k_de_input
    double* d_ds_sum = nullptr;          // [levels][W*H] sums over the probes of u g_j, then [DE_SUMS][ERR_BLOCKS] partials + [8] result
    float* d_ds_map = nullptr;           // [3][levels][W*H] m and the two buffers the smoothing passes alternate between
    int* d_ds_scale = nullptr;           // (H, W) k*
    float* d_ds_out = nullptr;           // (H, W, 3) the selected picture

    // error tracking (cl2_set_error_tracking, error_estimate.hpp): second moments of the addends, [8][W*H], while tracking is on
    float* d_mom = nullptr;
    bool mom_valid = false;              // every addend in the accumulators also went into the moments
    bool acc_clean = true;               // the accumulators hold nothing (cl2_create, cl2_reset_accumulators)
    double* d_err_partial = nullptr;     // frame metric: [3][ERR_BLOCKS] per-workgroup partials + [4] result (first call)
    // split tracking (cl2_set_split_tracking, error_split.hpp): the camera and the light part of the luma moments, [6][W*H], while on
    float* d_smom = nullptr;
    bool smom_valid = false;             // every addend in the accumulators also went into the split rows (the rules of mom_valid)
    float* d_de_rho = nullptr;           // (H, W) the light share of noise model 2 (k_de_rho), allocated by its first use

    // robust picture (cl2_set_robust_buckets, robust.hpp): M partial sums per pixel, [M][4][W*H], while the buckets are on
    float* d_bkt = nullptr;
    int bkt_M = 0;
    bool bkt_valid = false;              // every addend in the accumulators also went into the buckets (the rules of mom_valid)

    // adaptive sampling (cl2_set_sample_density, adaptive.hpp): the density's buffers exist while one is set (`density`), W*H
    // entries each; the maps have one per subpath buffer set, B entries each (they are written and read with the set's pass)
    bool density = false;                // a density is set explicitly: run_chunk takes the mapped kernels
    uint64_t* d_dens_C = nullptr;        // inclusive prefix sum of the quantised density M (units of 2^-16)
    uint64_t* d_dens_M = nullptr;        // M before the scan (quantisation scratch)
    float* d_dens_invm = nullptr;        // 1/m_q = (float)(2^16 / M_q): the factor of every camera sample of pixel q
    float* d_dens_m = nullptr;           // the density being quantised (caller's weights or the update's m)
    double* d_dens_partial = nullptr;    // [3][DENS_BLOCKS] per-workgroup partials + [3] totals
    unsigned long long* d_dens_fsum = nullptr;
    void* d_dens_tmp = nullptr;          // rocPRIM scan scratch
    size_t dens_tmp_bytes = 0;
    int* d_map[3] = {nullptr, nullptr, nullptr};   // slot -> pixel of every plane, one per subpath buffer set
    unsigned* d_cam_count = nullptr;     // camera samples received by mapped passes since cl2_reset_accumulators (first density)
    uint64_t cam_uniform = 0;            // ... and per pixel by unmapped passes (one per stream and pass)
    uint32_t dens_pass = 0;              // passes rendered with a density: the input of the slot offsets' hash (never reset)
    bool adaptive = false;               // cl2_set_adaptive_sampling: cl2_run_until updates the density before every chunk
    double adaptive_share = 0.25;
};

namespace {

#define HIP_TRY(r, expr)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (r)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                         \
            return CL2_E_HIP;                                                                     \
        }                                                                                         \
    } while (0)

#define TRY(expr)                         \
    do {                                  \
        int rc_ = (expr);                 \
        if (rc_ != CL2_OK) return rc_;    \
    } while (0)

template <typename T> int dev_alloc(cl2_renderer* r, T** p, size_t count) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) { r->err = std::string("hipMalloc: ") + hipGetErrorString(e); return CL2_E_NOMEM; }
    r->allocs.push_back(q);
    *p = static_cast<T*>(q);
    return CL2_OK;
}

template <typename T> void dev_free(cl2_renderer* r, T*& p) {
    if (!p) return;
    auto it = std::find(r->allocs.begin(), r->allocs.end(), static_cast<void*>(p));
    if (it != r->allocs.end()) r->allocs.erase(it);
    (void)hipFree(p);
    p = nullptr;
}

// a device buffer that lives as long as one call: allocated through dev_alloc, released when the call returns, whichever way
template <typename T> struct Scratch {
    cl2_renderer* r;
    T* p = nullptr;
    explicit Scratch(cl2_renderer* r_) : r(r_) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { dev_free(r, p); }
    int alloc(size_t count) { return dev_alloc(r, &p, count); }
    operator T*() const { return p; }
};

// Run-time flags as template arguments: with_flags(f, a, b, ...) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...).
// f is instantiated for every combination, so a kernel launch inside it stands under an `if constexpr` that names the
// combinations that exist: no other kernel is emitted.  Template parameters that are no flags stay branches at the call site.
template <class F> void with_flags(F&& f) { f(); }
template <class F, class... Rest> void with_flags(F&& f, bool flag, Rest... rest) {
    if (flag) with_flags([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else with_flags([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}
template <int N> using int_c = std::integral_constant<int, N>;

// device copy of n host elements (a scene array)
template <typename T> int upload(cl2_renderer* r, T** p, const T* h, size_t n) {
    TRY(dev_alloc(r, p, n));
    HIP_TRY(r, hipMemcpy(*p, h, n * sizeof(T), hipMemcpyHostToDevice));
    return CL2_OK;
}

int fail(cl2_renderer* r, int code, const std::string& msg) { r->err = msg; return code; }

inline int grid_for(size_t n) { return (int)((n + BLOCK - 1) / BLOCK); }

// nullptr when no event can be created: the span is then simply not timed (profiling is best effort,
// the launch itself is unaffected)
hipEvent_t take_event(cl2_renderer* r) {
    if (!r->event_pool.empty()) { hipEvent_t e = r->event_pool.back(); r->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

struct Timed {   // records a HIP-event span around a launch when profiling is on
    cl2_renderer* r; int stage; hipStream_t st; hipEvent_t a = nullptr;
    Timed(cl2_renderer* r_, int stage_, hipStream_t st_) : r(r_), stage(stage_), st(st_) {
        // level 1: the two traversal stages only (the connection-ray launch and the subpath traversal launches: bench.py's rooflines)
        const bool wanted = r->profiling >= 2 || (r->profiling == 1 && (stage == ST_TRAVERSE_CONN || stage == ST_TRAVERSE_PATHS));
        if (wanted) {
            a = take_event(r);
            if (a && hipEventRecord(a, st) != hipSuccess) { r->event_pool.push_back(a); a = nullptr; }
        }
    }
    ~Timed() {
        if (!a) return;
        hipEvent_t b = take_event(r);
        if (b && hipEventRecord(b, st) == hipSuccess) { r->spans.push_back({a, b, stage}); return; }
        r->event_pool.push_back(a);
        if (b) r->event_pool.push_back(b);
    }
};

int drain(cl2_renderer* r) {
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream_conn));
    HIP_TRY(r, hipStreamSynchronize(r->stream_res));
    for (auto& s : r->spans) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) r->ms[s.stage] += ms;
        r->event_pool.push_back(s.a);
        r->event_pool.push_back(s.b);
    }
    r->spans.clear();
    return CL2_OK;
}

// ---- launches (asynchronous on the given stream; `set` = the two subpath buffers of the sample) ----
int launch_generate(cl2_renderer* r, int which, hipStream_t st, const PathBufs* set) {
    Timed t(r, ST_GENERATE, st);
    if (which == CL2_LIGHT)
        hipLaunchKernelGGL(k_gen_light_rays, dim3(grid_for(r->B)), dim3(BLOCK), 0, st, r->B, r->d_light_tris,
                           r->d_light_areas, r->d_light_tri_index, r->d_mats, r->light_count, r->d_seeds, set[CL2_LIGHT]);
    else
        hipLaunchKernelGGL(k_gen_camera_rays<false>, dim3(grid_for(r->B)), dim3(BLOCK), 0, st, r->B, r->cam, r->d_seeds,
                           set[CL2_CAMERA], (const int*)nullptr);
    HIP_TRY(r, hipGetLastError());
    return CL2_OK;
}

// `map`: the set's slot -> pixel map of a mapped pass (adaptive.hpp), nullptr = the default kernels
int launch_generate_both(cl2_renderer* r, hipStream_t st, const PathBufs* set, const int* map) {
    Timed t(r, ST_GENERATE, st);
    with_flags([&](auto MAPPED) {
        hipLaunchKernelGGL(k_gen_rays<MAPPED.value>, dim3(grid_for(r->B)), dim3(BLOCK), 0, st, r->B, r->d_light_tris, r->d_light_areas,
                           r->d_light_tri_index, r->d_mats, r->light_count, r->cam, r->d_seeds, set[CL2_LIGHT], set[CL2_CAMERA], map);
    }, map != nullptr);
    HIP_TRY(r, hipGetLastError());
    return CL2_OK;
}

// Trees that are not LDS-resident.  Connection rays (one big launch of rays of very different cost)
// run as a persistent launch with lane-level ray replacement.  Subpaths have two organisations:
//   persistent (mode 2, the automatic choice)  one persistent traversal launch + one bounce launch per
//               level: best lane use, but 24 small launches per sample, each ending in a tail;
//   fused (mode 3)  the whole-subpath kernel of the small scenes, its tree fetched through the caches:
//               one ray per lane (a wave is as slow as its slowest ray), but 2 launches and no tails.
// In serial order fused wins on mid-size trees (5k-triangle sphere: 5.7 vs 8.7 ms per sample), but
// the sample pipeline with stage shares hides the tails of the persistent form and then the two are
// equal there (6.05 vs 6.00 Grays/s) and persistent wins from 82k triangles on (4.7 vs 3.9).
// dynamic shared memory of a launch that stages the tree (stage_bvh), the pad records behind the triangles included
inline size_t bvh_lds_bytes(const cl2_renderer* r) {
    return ((size_t)2 * r->bvh.n_lds_nodes + (r->bvh.lds_tris ? (size_t)3 * (r->bvh.n_tris + LDS_TRI_PADS) : 0) + (size_t)2 * r->bvh.n_fast_nodes) * sizeof(float4);
}
// counting mode 1: the node / triangle tallies of the REFERENCE's walk (binary stackless walk; the wide walk steps aside);
// mode 2 tallies what the 4-wide walk itself fetches and changes no launch but the whole-subpath one (see whole_subpaths)
inline bool count_ref(const cl2_renderer* r) { return r->counting == 1; }
inline bool tree_in_lds(const cl2_renderer* r) { return r->bvh.lds_tris && r->bvh.n_nodes <= r->bvh.n_lds_nodes; }
inline bool split_paths(const cl2_renderer* r) {
    if (r->traversal_mode == 1 || r->traversal_mode == 3) return false;
    if (r->traversal_mode == 2 || r->traversal_mode >= 4) return true;
    return !tree_in_lds(r);
}
inline bool split_conn(const cl2_renderer* r) {
    return r->traversal_mode >= 2 || (r->traversal_mode == 0 && !tree_in_lds(r));
}
// Connection set-up and walk fused into one launch (k_connect_walk_lds): trees wholly staged in LDS whose pruned table is a
// flat list of leaves (closest_hit_flat), one ray per lane, not while counting.  Debug bit 25 keeps the two launches (A/B).
// Debug bit 26 walks the flat table with the clamped loop (closest_hit_flat_clamped) in every launch that walks it.
inline int flat_walk(const cl2_renderer* r) {
    if (!r->fast_flat || ((r->debug_flags >> 11) & 1)) return 0;
    return ((r->debug_flags >> 26) & 1) ? 2 : 1;
}
inline bool fused_conn(const cl2_renderer* r) {
    return tree_in_lds(r) && !split_conn(r) && !count_ref(r) && r->bvh.n_fast_nodes > 0 && r->bvh.fast_flat &&
           !((r->debug_flags >> 25) & 1);
}
// The exact 4-wide walk (bvh_wide.hpp) for the connection-ray launch and, while the sample pipeline runs, the per-level subpath
// launches: mode 5, and the automatic choice for every tree that is read through the caches.  Round 2 kept the binary walk above
// 16 MB (15.7 vs 18.6 ms on the 155 MB tree, one triangle per pass); with two triangle pairs per pass, 7 stack entries in LDS and
// the gathered refill the wide walk is ahead there too (round 3, same box: connection launch 14.08 -> 13.51 ms, sample 27.78 ->
// 27.22 ms).  Never while counting: the node-test tallies are defined by the binary walk.
inline bool wide_walk(const cl2_renderer* r) {
    if (r->n_wide <= 0 || count_ref(r)) return false;
    if (r->traversal_mode == 5) return true;
    return (r->traversal_mode == 0 || r->traversal_mode == 3 || r->traversal_mode == 4) && !tree_in_lds(r);
}
// Whole subpaths (light, then camera, all levels) in ONE persistent launch per sample (k_subpaths_persistent)
// instead of a traversal + a bounce launch per level and kind: mode 4.  Measured at 1080p (ms per sample, serial order /
// sample pipeline): glass 15.9 / 12.6 per level, 13.0 / 13.6 whole; interior 36.2 / 32.7 per level, 33.5 / 34.1 whole.
// One launch has one tail instead of 24, which is what the serial order pays for; the sample pipeline already fills
// those tails with the other stage's work, and there the whole-subpath launch loses to its own costs (5 instead of 8
// waves per SIMD for the bounce code's registers; vertex stores scattered over unrelated pixels: 7.7 GB written per
// launch against 1.7 GB of vertices).  And a level launch of a 4K frame (8.3 M rays, 16 per lane) has little tail to
// lose: there the per-level form wins in serial order too (interior 4K: 53.7 vs 61.6 ms of subpath time, blob 24.0 vs
// 28.1).  So the automatic choice takes it in the serial order and up to 2^22 pixels only.
// The connection launch really runs the seeded visibility walk (cl2_set_connection_query(1)): only where connection rays take
// k_traverse_wide -- not in the fused or grid-stride launches of an LDS-resident tree, not without a wide collapse, not while the
// reference walk's tallies are taken (count_ref: the binary walk).
inline bool conn_vis(const cl2_renderer* r) {
    return r->connection_query == 1 && !fused_conn(r) && split_conn(r) && wide_walk(r);
}
inline bool whole_subpaths(const cl2_renderer* r) {
    if (r->traversal_order != 0) return false;                       // nearest-first order exists in k_traverse_wide only: every ray goes through it
    if (r->counting == 2 && r->traversal_mode != 4) return false;   // the walk's own tallies are taken in k_traverse_wide: every ray goes through it
    return r->traversal_mode == 4 || (r->traversal_mode == 0 && !tree_in_lds(r) && !r->pipe_active && r->B <= (1 << 22));
}
// Two triangles per step of the persistent walk while the tree is cache-resident (the step is then
// issue-bound and fewer, fatter steps win: glass +5 %, blob +4 %); one when it streams from memory
// (1M triangles: two cost 3 %).  debug_flags bit 12 inverts the choice (tests run both forms).
inline bool two_tris_per_step_plain(const cl2_renderer* r) {      // the size rule itself: the tree is cache-resident (<= 16 MB)
    return (size_t)r->bvh.n_nodes * 32 + (size_t)r->bvh.n_tris * 48 <= ((size_t)16 << 20);
}
inline bool two_tris_per_step(const cl2_renderer* r) {
    const bool two = two_tris_per_step_plain(r);
    return ((r->debug_flags >> 12) & 1) ? !two : two;
}
inline int effective_levels(const cl2_renderer* r) {
    if (r->levels_per_launch > 0) return std::min(r->levels_per_launch, (int)MAX_VERTS);
    return r->levels_auto ? r->levels_auto : (int)MAX_VERTS;
}
// Stages of the sample pipeline.  Small frames do not fill the machine with one launch (256x256: 256
// workgroups on 256 CUs), so a third stage side by side pays (10.1 / 13.9 / 18.4 Grays/s with 0 / 1 / 2);
// from 1080p on two and three stages measure the same and two need less memory traffic in flight.
inline int pipeline_stages(const cl2_renderer* r) {
    if (r->pipelining >= 0) return r->pipelining;
    return r->B <= (1 << 19) ? 2 : 1;
}
inline int persistent_grid() { return 256 * 8; }      // 256 CUs x 8 workgroups of 4 waves = 32 waves per CU
// While the sample pipeline runs, the subpath stage and the connection stage of two samples are on the
// machine together.  Persistent launches hold their wave slots until the launch runs dry, so the two
// stages get a fixed share of the slots each (in eighths of the machine): the stage whose launch is in
// its tail (a few long rays) leaves the VALUs to the other one instead of leaving them idle.
constexpr int TUNE_SAMPLES = 6;       // samples timed per candidate organisation
constexpr int SHARE_SERIAL = 9;       // tuned result: the serial order beats every pipelined organisation
inline int paths_eighths(const cl2_renderer* r) {
    const int forced = (r->debug_flags >> 8) & 7;          // experiment switch
    return forced ? forced : ((r->paths_share && r->paths_share != SHARE_SERIAL) ? r->paths_share : 4);
}
// share 8 = no fixed shares: both stages launch full-size grids and take the slots as they come
// (large frames: the launches are long, their tails do not matter, and a full grid hides latency best)
inline int persistent_grid_paths(const cl2_renderer* r) {
    const int e = paths_eighths(r);
    return (r->pipe_active && e < 8) ? 256 * e : persistent_grid();
}
inline int persistent_grid_conn(const cl2_renderer* r) {
    const int e = paths_eighths(r);
    return (r->pipe_active && e < 8) ? 256 * (8 - e) : persistent_grid();
}

// One persistent launch of the exact 4-wide walk.  `stage` 0 = subpath stage, 1 = connection stage: each has its own
// stack-overflow region, since the two run side by side in the sample pipeline.
// The per-lane stack of a wide walk keeps its first entries in LDS and the rest in a global array.  How deep it can get
// is a static property of the tree and of the child order.  In the reference's order every entry pending on the reference's
// stack (at most `max_pending` of them, counted at upload) stands for at most two wide-stack entries, plus the four a visit
// pushes; nearest first, the bound is the tree's order_depth instead (scene_prep.hpp: build_wide, wide_overflow_entries; both
// bounds are tested against the walk's push rule in tests/test_wide_stack_cpu.py and on the device in
// tests/test_gpu_wide_stack.py).  The kernel does not clamp its pushes: wide_ovf_entries is recomputed whenever the scene or
// the order changes, and a tree that the cap cannot serve nearest first is refused there, so no launch sees a stack deeper
// than its array.  The array is sized for that bound (not for the 2 x 64 + 8 any admissible tree could reach) and exists only
// once a wide launch has been asked for: an LDS-resident scene never takes the wide walk on its own, and a turntable builds
// one renderer per frame.
int ensure_wide_overflow(cl2_renderer* r) {
    if (r->d_wide_ovf) return CL2_OK;
    const size_t lanes = (size_t)persistent_grid() * BLOCK;
    return dev_alloc(r, &r->d_wide_ovf, 2 * lanes * (size_t)std::max(r->wide_ovf_entries, 1));
}

// VIS: the seeded visibility walk (bvh_wide.hpp) -- a source that yields targets; the speculative walk in the reference's child order only.
template <class Source, bool VIS = false>
// quiet: the feature pass (denoise.hpp) -- the rays go to its own tally, not to cl2_read_counters / cl2_read_walk_tallies
int launch_wide(cl2_renderer* r, hipStream_t st, int stage, const unsigned* count, unsigned* work_counter, Source src, int is_conn,
                bool quiet = false) {
    Stats* const stats = quiet ? r->d_feat_stats : r->d_stats;
    const bool tally = !quiet && r->counting == 2;
    const int grid = stage == 0 ? persistent_grid_paths(r) : persistent_grid_conn(r);
    TRY(ensure_wide_overflow(r));
    WideView w = r->wide;
    w.ovf_stride = std::max(r->wide_ovf_entries, 1);
    w.overflow = r->d_wide_ovf + (size_t)stage * persistent_grid() * BLOCK * w.ovf_stride;
    // LDS per workgroup: per-lane stack (8 B per entry and lane) + the top of the tree (128 B per wide node); experiment
    // switches: debug_flags bits 16-19 stack entries (0 = default), bits 20-23 window in units of 32 wide nodes
    const int wflag = (r->debug_flags >> 20) & 0xF;
    // (round 3 ran 7 stack entries + a 64-node window, 22 KB per workgroup; its measurements are in DESIGN.md 6.1)
    // round 4: WIDE_STACK_LDS (8) entries, a compile-time constant (shift-addressed).  The window's lanes read LDS in a
    // branch of their own (the per-lane pointer select of round 3 made EVERY node fetch a flat load).  Same-box A/B of the
    // rewritten walk, ms (connection launch alone | sample), stack entries + window nodes:
    //   glass     8+0 3.28 | 8.17   8+32 3.09 | 7.90   7+64 3.19 | 7.79   8+64 3.35 | 7.98   6+64 3.11 | 7.91   6+128 3.68 | 8.68
    //   blob      8+0 4.18 | 10.30  8+32 3.90 | 9.95   7+64 4.02 | 9.97   8+64 4.15 | 10.15
    //   interior  8+0 12.0 | 24.2   8+32 11.2 | 22.8   7+64 11.2 | 23.3   8+64 11.2 | 22.3; one triangle pair per pass: 8+64 10.7 | 21.3
    // so: 32 nodes (20 KB per workgroup: 8 workgroups per CU) and two pairs per pass while the tree is cache-resident, 64
    // nodes and one pair when it streams from memory.  debug_flags bits 20-23 override the window (units of 32 nodes, 15 = none).
    const bool streams_from_memory = !two_tris_per_step_plain(r);
    w.stack_lds = WIDE_STACK_LDS;
    w.n_lds_nodes = std::min(r->n_wide, wflag == 15 ? 0 : (wflag ? 32 * wflag : (streams_from_memory ? 64 : 32)));
    // never more than the 64 KB a workgroup may ask for: the window gives way, the stack entries are needed
    w.n_lds_nodes = std::min<int>(w.n_lds_nodes, (int)(((size_t)64 * 1024 - (size_t)w.stack_lds * BLOCK * 8) / 128));
    const size_t lds = (size_t)w.stack_lds * BLOCK * 8 + (size_t)w.n_lds_nodes * 128;
    // the binary records (lanes whose ray has a non-finite 1/d) come through the caches: no window for them
    BvhView b = r->bvh;
    b.n_lds_nodes = 0; b.lds_tris = 0; b.n_fast_nodes = 0;
    // The opt-in nearest-first child order (cl2_set_traversal_order; NOT the parity path) exists for the speculative walk only, and
    // so does the seeded walk, which keeps the reference's order.
    const bool order = !VIS && r->traversal_order != 0;
    const bool spec = VIS || order || !((r->debug_flags >> 13) & 1);            // speculative expansion of the stack top (bvh_wide.hpp); bit 13: off
    // 36-byte triangle records, a pair fetched as one run of 72 bytes (bvh_wide.hpp: PACK); bit 14: the 48-byte records of the other
    // walks.
    const bool pack = w.tris36 && !((r->debug_flags >> 14) & 1);
    constexpr bool seeded_conn = std::is_same_v<Source, ConnVisRaySource>;
    // the seeded connection launch exists for the tree's own record form only: bit 14 is an A/B switch of the closest-hit walk and
    // is refused together with cl2_set_connection_query(1) (its 48-byte instantiation with one pair per pass would spill)
    if (seeded_conn && !pack) return fail(r, CL2_E_STATE, "the seeded connection walk reads the packed triangle records");
    auto launch = [&](auto REPS) {
        with_flags([&](auto TALLY, auto SPEC, auto PACK, auto ORDER) {
            if constexpr ((SPEC.value || !(ORDER.value || VIS)) && !(ORDER.value && VIS) && (PACK.value || !seeded_conn))
                hipLaunchKernelGGL((k_traverse_wide<REPS.value, Source, TALLY.value, SPEC.value, PACK.value, ORDER.value, VIS>), dim3(grid),
                                   dim3(BLOCK), lds, st, w, b, count, work_counter, src, stats, is_conn);
        }, tally, spec, pack, order);
    };
    if (streams_from_memory) launch(int_c<1>{}); else launch(int_c<WIDE_TRI_REPS>{});
    HIP_TRY(r, hipGetLastError());
    return CL2_OK;
}

// One persistent launch of the binary walk (k_traverse_persistent) over the rays of `src`: the subpath levels and the connection rays
// of trees that are not LDS-resident, where the 4-wide walk steps aside.
template <class Source>
int launch_persistent(cl2_renderer* r, hipStream_t st, int grid, const unsigned* count, unsigned* work_counter, Source src, int is_conn) {
    with_flags([&](auto CNT, auto TWO) {
        hipLaunchKernelGGL((k_traverse_persistent<CNT.value, TWO.value, Source>), dim3(grid), dim3(BLOCK), bvh_lds_bytes(r), st, r->bvh,
                           count, work_counter, src, r->d_stats, is_conn);
    }, count_ref(r), two_tris_per_step(r));
    HIP_TRY(r, hipGetLastError());
    return CL2_OK;
}

// Subpath phase scratch (d_queue, d_qcount[0..6], d_work[0..6], d_hit, d_block_stats) is touched by this
// phase only; the connection phase owns d_qcount[7] and d_work[7].
// `cam0`: 0 = plain; 1 (light subpaths) = the level-0 traversal launch also walks the camera subpaths' first rays (their
// hits go to d_hit_cam0); 2 (camera subpaths) = level 0 has no traversal launch of its own, its bounce reads d_hit_cam0.
// Only the persistent per-level organisation has separate traversal launches to merge.
int launch_trace(cl2_renderer* r, int which, hipStream_t st, const PathBufs* set, int cam0 = 0) {
    const int B = r->B;
    PathBufs pb = set[which];
    HIP_TRY(r, hipMemsetAsync(r->d_qcount + 1, 0, 6 * sizeof(unsigned), st));
    const bool split = split_paths(r);
    if (!split) cam0 = 0;
    if (split) HIP_TRY(r, hipMemsetAsync(r->d_work, 0, 7 * WORK_STRIDE * sizeof(unsigned), st));
    const int step = split ? 1 : effective_levels(r);
    for (int first = 0; first < MAX_VERTS; first += step) {
        const int end = std::min(first + step, (int)MAX_VERTS);
        // queue slot k holds the paths alive after level k-1 (slot 0 = everybody, count B)
        const int* q_in = first == 0 ? nullptr : r->d_queue + (size_t)(first - 1) * B;
        const unsigned* c_in = r->d_qcount + first;
        int* q_out = r->d_queue + (size_t)(end - 1) * B;
        unsigned* c_out = r->d_qcount + end;
        const bool merged = first == 0 && cam0 == 1, hits_ready = first == 0 && cam0 == 2;
        if (split && !hits_ready) {
            Timed t(r, ST_TRAVERSE_PATHS, st);
            PathRaySource src{q_in, pb.P0 + (size_t)first * B, pb.P1 + (size_t)first * B, r->d_hit};
            const PathBufs& cpb = set[CL2_CAMERA];
            DualPathRaySource dual{pb.P0, pb.P1, cpb.P0, cpb.P1, r->d_hit, r->d_hit_cam0, B};
            const unsigned* c_trav = merged ? r->d_qcount + 8 : c_in;
            // The per-level subpath launches take the 4-wide walk wherever the scene has it.  Rounds 2 / 3 took it only while the
            // sample pipeline ran (alone these launches were tail-bound and gained nothing: glass 7.43 -> 7.56 ms); with round 4's
            // pass the walk is ahead alone as well -- serial order at 3840 x 2160, subpath traversal per sample: blob 15.8 -> 12.6
            // ms, 1M triangles 44.2 -> 31.8 -- and with sample streams a launch is no longer all tail.  (debug_flags bit 3, which
            // forced it in the serial order, is accepted and has no effect any more; mode 2 still means the binary walk.)
            unsigned* const work = r->d_work + first * WORK_STRIDE;
            if (wide_walk(r)) {
                if (merged) TRY(launch_wide(r, st, 0, c_trav, work, dual, 0));
                else TRY(launch_wide(r, st, 0, c_trav, work, src, 0));
            } else {
                if (merged) TRY(launch_persistent(r, st, persistent_grid_paths(r), c_trav, work, dual, 0));
                else TRY(launch_persistent(r, st, persistent_grid_paths(r), c_trav, work, src, 0));
            }
            r->launches_tp++;
        }
        Timed t(r, split ? ST_BOUNCE : ST_TRAVERSE_PATHS, st);
        const float4* ext_hit = hits_ready ? r->d_hit_cam0 : r->d_hit;
        // EXT: the bounce of a level whose hits a traversal launch left in ext_hit; the reference walk's tallies are then that launch's
        with_flags([&](auto CAM, auto CNT, auto EXT) {
            if constexpr (!(EXT.value && CNT.value))
                hipLaunchKernelGGL((k_trace_subpath<CAM.value, CNT.value, EXT.value>), dim3(grid_for(B)), dim3(BLOCK),
                                   EXT.value ? 0 : bvh_lds_bytes(r), st, r->bvh, r->d_stats, first, end, q_in, c_in, q_out, c_out, B, pb,
                                   r->d_seeds, r->d_tri_shade, r->d_mats, r->n_mats, r->d_block_stats, ext_hit);
        }, which == CL2_CAMERA, !split && count_ref(r), split);
        if (!split) r->launches_tp++;
        HIP_TRY(r, hipGetLastError());
    }
    return CL2_OK;
}

// subpaths of every pixel: kinds = 1 light, 2 camera, 3 both (light first: one RNG stream per pixel)
int launch_subpaths(cl2_renderer* r, hipStream_t st, const PathBufs* set, int kinds) {
    if (!whole_subpaths(r)) {
        // both kinds in one call (cl2_run_samples): the camera subpaths' first rays ride in the light subpaths' level-0 launch
        const bool merge = kinds == 3;
        int rc = CL2_OK;
        if (kinds & 1) rc = launch_trace(r, CL2_LIGHT, st, set, merge ? 1 : 0);
        if (rc == CL2_OK && (kinds & 2)) rc = launch_trace(r, CL2_CAMERA, st, set, merge ? 2 : 0);
        return rc;
    }
    HIP_TRY(r, hipMemsetAsync(r->d_work, 0, WORK_STRIDE * sizeof(unsigned), st));
    Timed t(r, ST_TRAVERSE_PATHS, st);
    // lanes gathered / steps waited before a wave runs its bounce phase (cl2_set_subpath_gather)
    const int lanes = r->gather_lanes, wait = r->gather_wait;
    // the exact 4-wide walk inside the launch where the scene has it (same rule as the connection rays); round 4: also for trees
    // that stream from memory, with one triangle pair per pass there (as in launch_wide)
    const bool widew = wide_walk(r);
    WideView w = r->wide;
    w.stack_lds = 8; w.n_lds_nodes = 0;                        // 5 workgroups per CU here (registers): 24 KB each is free
    if (widew) {
        TRY(ensure_wide_overflow(r));
        w.n_lds_nodes = std::min(r->n_wide, 64);
        w.ovf_stride = std::max(r->wide_ovf_entries, 1);
        w.overflow = r->d_wide_ovf;                            // stage 0 region: the subpath stage
    }
    if ((r->debug_flags >> 14) & 1) w.tris36 = nullptr;         // bit 14: the 48-byte triangle records (bvh_wide.hpp: PACK off)
    const size_t lds = widew ? (size_t)w.stack_lds * BLOCK * 8 + (size_t)w.n_lds_nodes * 128 : bvh_lds_bytes(r);
    // register budget: 5 waves per SIMD (102 VGPRs: the bounce code; 6 waves cost 64 bytes of scratch per lane and measured
    // 13.0 -> 13.6 ms on the glass scene, 8 waves 24.5 ms); the grid holds as many workgroups as stay resident
    constexpr int WPS = 5;
    const int grid = std::max(1, persistent_grid_paths(r) * WPS / 8);
    // the WIDE forms are uncounted (wide_walk) and hold TWO_TRIS at true: what their walk varies is the triangle pairs per pass,
    // which the binary forms leave at the default
    auto launch = [&](auto REPS) {
        with_flags([&](auto CNT, auto TWO, auto WIDE) {
            if constexpr (WIDE.value ? (!CNT.value && TWO.value) : REPS.value == WIDE_TRI_REPS)
                hipLaunchKernelGGL((k_subpaths_persistent<CNT.value, TWO.value, WPS, WIDE.value, REPS.value>), dim3(grid), dim3(BLOCK), lds, st,
                                   r->bvh, w, r->B, r->d_work, set[CL2_LIGHT], set[CL2_CAMERA], r->d_seeds, r->d_tri_shade, r->d_mats,
                                   r->n_mats, r->d_stats, lanes, wait, kinds);
        }, !widew && count_ref(r), widew || two_tris_per_step(r), widew);
    };
    if (widew && !two_tris_per_step(r)) launch(int_c<1>{}); else launch(int_c<WIDE_TRI_REPS>{});
    r->launches_tp++;
    HIP_TRY(r, hipGetLastError());
    return CL2_OK;
}

// connection set-up + connection rays; `cs` = which {chit, cmask} set
int launch_connect(cl2_renderer* r, hipStream_t st, const PathBufs* set, int cs) {
    const int B = r->B;
    const PathBufs& lp = set[CL2_LIGHT];
    const PathBufs& cp = set[CL2_CAMERA];
    if (fused_conn(r)) {
        // one launch: cull, workgroup-local queue, walk (k_connect_walk_lds); the set-up stage takes no time of its own
        Timed t(r, ST_TRAVERSE_CONN, st);
        hipLaunchKernelGGL(k_connect_walk_lds, dim3(grid_for(B)), dim3(BLOCK), bvh_lds_bytes(r), st, r->bvh, B, lp, cp,
                           r->d_mats, r->n_mats, r->cam, r->d_cmask[cs], r->d_chit[cs], r->d_stats);
        r->launches_tc++;
        HIP_TRY(r, hipGetLastError());
        return CL2_OK;
    }
    HIP_TRY(r, hipMemsetAsync(r->d_qcount + 7, 0, sizeof(unsigned), st));
    {
        Timed t(r, ST_CONNECT_SETUP, st);
        // Large scenes: this launch (8,100 short workgroups at 7 waves per SIMD) runs beside the persistent subpath launches of
        // the next sample, whose chain is the critical path; left alone it floods the CUs and every level launch of that chain
        // starts late.  39 KB of unused dynamic LDS hold it to 4 workgroups per CU: glass 8.73 -> 8.46 ms per sample, blob 11.03
        // -> 10.85 (25 KB: 8.71 / 11.08; 31 KB: 8.44 / 10.98; 52 KB: 8.61 / 10.86).  The Cornell pipeline has no persistent
        // launches and wants the kernel at full speed.
        const size_t pad = split_conn(r) ? (size_t)39 * 1024 : 0;
        hipLaunchKernelGGL(k_connect_setup, dim3(grid_for(B)), dim3(BLOCK), pad, st, B, lp, cp,
                           r->d_mats, r->n_mats, r->cam, r->d_ctag, r->d_qcount + 7, r->d_cmask[cs]);
    }
    HIP_TRY(r, hipGetLastError());
    {
        Timed t(r, ST_TRAVERSE_CONN, st);
        if (split_conn(r)) {
            HIP_TRY(r, hipMemsetAsync(r->d_work + 7 * WORK_STRIDE, 0, WORK_STRIDE * sizeof(unsigned), st));
            ConnRaySource src{r->d_ctag, lp.P0, cp.P0, r->d_chit[cs],
                              V3{r->cam.focal_point[0], r->cam.focal_point[1], r->cam.focal_point[2]}, B};
            if (conn_vis(r)) {
                ConnVisRaySource vsrc{src, cp.tri};
                TRY((launch_wide<ConnVisRaySource, true>(r, st, 1, r->d_qcount + 7, r->d_work + 7 * WORK_STRIDE, vsrc, 1)));
            } else if (wide_walk(r)) {
                TRY(launch_wide(r, st, 1, r->d_qcount + 7, r->d_work + 7 * WORK_STRIDE, src, 1));
            } else {
                TRY(launch_persistent(r, st, persistent_grid_conn(r), r->d_qcount + 7, r->d_work + 7 * WORK_STRIDE, src, 1));
            }
        } else {
            // grid-stride over the (device-side) ray count; enough workgroups to fill 256 CUs several times over
            const int grid = std::min<size_t>(grid_for((size_t)B * 8), 256 * 32);
            with_flags([&](auto CNT) {
                hipLaunchKernelGGL(k_traverse_conn<CNT.value>, dim3(grid), dim3(BLOCK), bvh_lds_bytes(r), st, r->bvh, B, r->d_qcount + 7,
                                   r->d_ctag, lp.P0, cp.P0, r->cam, r->d_chit[cs], r->d_stats);
            }, count_ref(r));
        }
        r->launches_tc++;
    }
    HIP_TRY(r, hipGetLastError());
    return CL2_OK;
}

// buffers of the reproducible light image: one record slot per (light vertex, entry), as the reference's five arrays
inline unsigned det_key_bits(const cl2_renderer* r) {          // bits of a target entry (< B) plus one for DET_NO_KEY's
    unsigned bits = 1;
    while (((size_t)1 << bits) < (size_t)r->B) bits++;
    return bits + 1;
}
int ensure_det_buffers(cl2_renderer* r) {
    // guarded by the LAST thing set up: a set whose allocation failed half way (CL2_E_NOMEM) is not mistaken for a complete one
    // by the next sample -- it is freed (dev_free nulls the pointers) and built again
    if (r->d_det_tmp) return CL2_OK;
    dev_free(r, r->d_det_keys); dev_free(r, r->d_det_keys_sorted); dev_free(r, r->d_det_slots); dev_free(r, r->d_det_slots_sorted); dev_free(r, r->d_det_vals);
    const size_t n = (size_t)MAX_VERTS * r->B;
    TRY(dev_alloc(r, &r->d_det_keys, n));
    TRY(dev_alloc(r, &r->d_det_keys_sorted, n));
    TRY(dev_alloc(r, &r->d_det_slots, n));
    TRY(dev_alloc(r, &r->d_det_slots_sorted, n));
    TRY(dev_alloc(r, &r->d_det_vals, n));
    hipLaunchKernelGGL(k_iota, dim3(grid_for(n)), dim3(BLOCK), 0, r->stream, r->d_det_slots, n);
    HIP_TRY(r, hipGetLastError());
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    size_t bytes = 0;
    HIP_TRY(r, det_sort_pairs(nullptr, bytes, r->d_det_keys, r->d_det_keys_sorted, r->d_det_slots, r->d_det_slots_sorted, n, det_key_bits(r), r->stream));
    unsigned char* tmp = nullptr;
    TRY(dev_alloc(r, &tmp, bytes));
    r->d_det_tmp = tmp; r->det_tmp_bytes = bytes;
    return CL2_OK;
}

inline unsigned layer_row_host(const LayerCodes& lc, int t) { return (unsigned)(lc.w[(t - 1) >> 1] >> (((t - 1) & 1) * 32)); }

// the layers' share of launch_accumulate / launch_finalize_accumulate (layers.hpp): same stream, right beside the main kernel
int launch_layers_accumulate(cl2_renderer* r, hipStream_t st) {
    if (r->n_layers == 0) return CL2_OK;
    hipLaunchKernelGGL(k_layers_accumulate, dim3(grid_for(r->FB)), dim3(BLOCK), 0, st, r->B, r->W, r->H, r->n_layers,
                       (const float*)r->d_agg, (const float*)r->d_lay_agg, r->d_lay_light, r->d_lacc);
    HIP_TRY(r, hipGetLastError());
    return CL2_OK;
}

int launch_resolve(cl2_renderer* r, hipStream_t st, const PathBufs* set, int cs, const int* map = nullptr) {
    const int B = r->B;
    const PathBufs& lp = set[CL2_LIGHT];
    const PathBufs& cp = set[CL2_CAMERA];
    {
        Timed t(r, ST_CONNECT_RESOLVE, st);
        // a full strategy mask (the default, or set explicitly) runs the kernels without the STRAT code
        const bool masked = r->strategy_mask != CL2_STRATEGY_ALL;
        // a layer table (cl2_set_layers): the LAYERS instantiations, two waves per SIMD (their 24 layer totals are registers)
        const bool layered = r->n_layers > 0;
        // 3 waves per SIMD: what 165 VGPRs and 52 KB of LDS tables per workgroup allow (2 / 4 measured slower: DESIGN 6.1).  Debug
        // bits 4-6 = 7: one wave per camera vertex (tests/connect_resolve_wide.hpp: same results bit for bit, measured slower: 1.14 vs
        // 0.93 ms; a second implementation kept as a cross-check, built only with -DCL2_TEST_VARIANT = libclive2_amd_test.so)
        const int occ = (r->debug_flags >> 4) & 7;
        if (occ != 0 && occ != 7) return fail(r, CL2_E_INVALID, "debug bits 4-6 must be 0 or 7");
        if (occ == 7 && r->streams != 1) return fail(r, CL2_E_INVALID, "the cross-check resolve kernel handles one sample stream");
        // (it splats with atomics and writes no records: the sort + gather below would read buffers it never filled)
        if (occ == 7 && r->reproducible) return fail(r, CL2_E_INVALID, "the cross-check resolve kernel has no reproducible form: clear debug bits 4-6 or cl2_set_reproducible(0)");
        if (occ == 7 && r->density) return fail(r, CL2_E_STATE, "the cross-check resolve kernel has no mapped form: cl2_set_sample_density(NULL) or clear debug bits 4-6");
        if (occ == 7 && masked) return fail(r, CL2_E_INVALID, "the cross-check resolve kernel has no masked form: clear debug bits 4-6 or set the full strategy mask");
        // (the setters refuse these combinations; a pass must never run the layered kernels on them)
        if (layered && occ == 7) return fail(r, CL2_E_INVALID, "the cross-check resolve kernel has no layered form: clear debug bits 4-6 or cl2_set_layers(NULL, 0)");
        if (layered && masked) return fail(r, CL2_E_STATE, "layer accumulators need the full strategy mask: cl2_set_strategy_mask(CL2_STRATEGY_ALL) or cl2_set_layers(NULL, 0)");
        if (layered && map) return fail(r, CL2_E_STATE, "layer accumulators have no mapped form: cl2_set_sample_density(NULL) or cl2_set_layers(NULL, 0)");
#ifdef CL2_TEST_VARIANT
        if (occ == 7)
            hipLaunchKernelGGL(k_connect_resolve_wide, dim3((B + RW_PIX - 1) / RW_PIX), dim3(RW_BLOCK), 0, st, B, lp, cp, r->d_mats,
                               r->d_tri_shade, r->cam, r->d_cmask[cs], r->d_chit[cs], r->d_agg, r->d_light_image, r->d_uni,
                               r->d_stats, r->debug_flags);
        else
#else
        if (occ == 7) return fail(r, CL2_E_INVALID, "the one-wave-per-camera-vertex resolve kernel is only built into the test variant of the library");
#endif
        {
            if (r->reproducible) {
                // records instead of atomics: every slot starts empty (DET_NO_KEY = all ones)
                TRY(ensure_det_buffers(r));
                HIP_TRY(r, hipMemsetAsync(r->d_det_keys, 0xFF, (size_t)MAX_VERTS * B * sizeof(unsigned), st));
            }
            // the material table goes to LDS when it fits LDS_MAT_CAP entries (the reference ships 8): connect_resolve.hpp
            const bool mats_lds = r->n_mats <= LDS_MAT_CAP;
            // Three waves per SIMD take the LDS table and atomics.  The record stores of the reproducible form need registers the 168 of
            // three waves do not leave; with more than LDS_MAT_CAP materials the table stays in global memory and its addresses take the
            // registers that three waves per SIMD do not leave -- two waves, no scratch.
            const bool three_waves = mats_lds && !r->reproducible && !layered;
            auto launch = [&](auto W) {
                with_flags([&](auto ML, auto DET, auto MAPPED, auto STRAT, auto LAYERS) {
                    constexpr bool wants_three = ML.value && !DET.value && !LAYERS.value;
                    if constexpr (wants_three == (W.value == 3) && !(LAYERS.value && (MAPPED.value || STRAT.value)))
                        hipLaunchKernelGGL((k_connect_resolve<W.value, ML.value, DET.value, MAPPED.value, STRAT.value, LAYERS.value>),
                                           dim3(grid_for(B)), dim3(BLOCK), 0, st, B, lp, cp, r->d_mats, r->n_mats, r->d_tri_shade, r->cam_tris,
                                           r->cam, r->d_cmask[cs], r->d_chit[cs], r->d_agg, r->d_light_image, r->d_uni, r->d_stats,
                                           r->debug_flags, r->d_det_keys, r->d_det_vals, map, (unsigned long long)r->strategy_mask, r->lcodes,
                                           r->d_lay_agg, r->d_lay_light);
                }, mats_lds, r->reproducible, map != nullptr, masked, layered);
            };
            // The slim kernel (connect_resolve.hpp): three waves per SIMD, and room left on the SIMD and in LDS for a workgroup of
            // the subpath stage, whose launches of later samples are pending on the other stream.  Its DET form fits three waves too.
            if (resolve_runs_slim(r->bvh.n_tris, r->n_mats, map != nullptr, masked, layered, r->debug_flags)) {
                with_flags([&](auto DET) {
                    hipLaunchKernelGGL((k_connect_resolve_slim<DET.value>), dim3(grid_for(B)), dim3(BLOCK), 0, st, B, lp, cp, r->d_mats,
                                       r->n_mats, r->d_tri_shade, r->cam_tris, r->cam, r->d_cmask[cs], r->d_chit[cs], r->d_agg,
                                       r->d_light_image, r->d_uni, r->d_stats, r->debug_flags, r->d_det_keys, r->d_det_vals, map,
                                       (unsigned long long)r->strategy_mask, r->lcodes, r->d_lay_agg, r->d_lay_light);
                }, r->reproducible);
            } else if (three_waves) launch(int_c<3>{}); else launch(int_c<2>{});
        }
    }
    HIP_TRY(r, hipGetLastError());
    if (r->reproducible) {
        // a stable sort of {target entry, slot} on the target's bits: a target's run is then ordered by slot = (s, source pixel);
        // one thread per target sums its run front to back
        Timed t(r, ST_CONNECT_RESOLVE, st);
        const size_t n = (size_t)MAX_VERTS * B;
        size_t bytes = r->det_tmp_bytes;
        HIP_TRY(r, det_sort_pairs(r->d_det_tmp, bytes, r->d_det_keys, r->d_det_keys_sorted, r->d_det_slots, r->d_det_slots_sorted, n,
                                  det_key_bits(r), st));
        if (r->n_layers > 0)
            hipLaunchKernelGGL(k_det_gather_layers, dim3(grid_for(n)), dim3(BLOCK), 0, st, r->d_det_keys_sorted, r->d_det_slots_sorted, n,
                               r->d_det_vals, r->d_light_image, (unsigned)B, layer_row_host(r->lcodes, 1), r->n_layers, r->d_lay_light);
        else
            hipLaunchKernelGGL(k_det_gather, dim3(grid_for(n)), dim3(BLOCK), 0, st, r->d_det_keys_sorted, r->d_det_slots_sorted, n,
                               r->d_det_vals, r->d_light_image);
        HIP_TRY(r, hipGetLastError());
    }
    return CL2_OK;
}

int launch_finalize(cl2_renderer* r, hipStream_t st) {
    Timed t(r, ST_FINALIZE, st);
    hipLaunchKernelGGL(k_finalize, dim3(grid_for(r->B)), dim3(BLOCK), 0, st, r->B, r->W, r->H, r->d_agg, r->d_finalized,
                       r->d_sample_w);
    HIP_TRY(r, hipGetLastError());
    return CL2_OK;
}

// with error tracking on (r->d_mom allocated) the <true> forms also add every addend's second moments; with robust buckets on
// (r->d_bkt allocated) the <., true> forms also add every addend to its bucket: f(MOMENTS, BUCKETS) launches the kernel
template <class F> void launch_accumulating(cl2_renderer* r, F&& f) { with_flags(f, r->d_mom != nullptr, r->d_bkt != nullptr); }

int launch_accumulate(cl2_renderer* r, hipStream_t st) {
    Timed t(r, ST_ACCUMULATE, st);
    const dim3 grid(grid_for(r->FB)), block(BLOCK);
    if (r->d_smom)                       // split tracking: before the kernel that zeroes the light image (error_split.hpp)
        hipLaunchKernelGGL(k_split_moments_staged, grid, block, 0, st, r->FB, r->streams, (const float4*)r->d_finalized,
                           (const float*)r->d_sample_w, (const float4*)r->d_light_image, r->d_smom);
    launch_accumulating(r, [&](auto MOM, auto BKT) {
        hipLaunchKernelGGL((k_accumulate<MOM.value, BKT.value>), grid, block, 0, st, r->FB, r->streams, r->d_finalized, r->d_sample_w,
                           r->d_light_image, r->d_uni, r->d_acc, r->d_mom, r->d_bkt, r->bkt_M);
    });
    r->acc_clean = false;
    HIP_TRY(r, hipGetLastError());
    return launch_layers_accumulate(r, st);
}

// `mapped`: the pass ran with the density's slot maps, `pass` = its number (adaptive.hpp)
int launch_finalize_accumulate(cl2_renderer* r, hipStream_t st, bool mapped = false, uint32_t pass = 0) {
    Timed t(r, ST_FINALIZE, st);
    const dim3 grid(grid_for(r->FB)), block(BLOCK);
    if (r->d_smom) {                     // split tracking: before the kernel that zeroes the light image (error_split.hpp)
        if (mapped) return fail(r, CL2_E_STATE, "split tracking has no mapped form (cl2_set_sample_density refuses it)");
        hipLaunchKernelGGL(k_split_moments_fused, grid, block, 0, st, r->B, r->W, r->H, (const float*)r->d_agg,
                           (const float4*)r->d_light_image, r->d_smom);
    }
    launch_accumulating(r, [&](auto MOM, auto BKT) {
        if (mapped)
            hipLaunchKernelGGL((k_finalize_accumulate_mapped<MOM.value, BKT.value>), grid, block, 0, st, r->B, r->W, r->H, r->d_agg,
                               r->d_light_image, r->d_uni, r->d_acc, r->d_mom, r->d_dens_C, r->d_dens_invm, pass, r->d_cam_count, r->d_bkt,
                               r->bkt_M);
        else
            hipLaunchKernelGGL((k_finalize_accumulate<MOM.value, BKT.value>), grid, block, 0, st, r->B, r->W, r->H, r->d_agg,
                               r->d_light_image, r->d_uni, r->d_acc, r->d_mom, r->d_bkt, r->bkt_M);
    });
    r->acc_clean = false;
    HIP_TRY(r, hipGetLastError());
    return launch_layers_accumulate(r, st);       // (never after a mapped pass: launch_resolve refuses a density while a table is set)
}

int need_scene(cl2_renderer* r) {
    if (!r) return CL2_E_INVALID;
    r->pipe_active = false;
    if (!r->scene_ok) return fail(r, CL2_E_STATE, "no scene uploaded (call cl2_upload_scene first)");
    HIP_TRY(r, hipSetDevice(r->device));
    return CL2_OK;
}

// Everything that has one entry per (sample stream, pixel): allocated for r->B = r->streams x r->FB entries and initialised
// as cl2_create always did (seeds 1, zero lengths / images / masks).  cl2_set_sample_streams frees and re-allocates it.
void free_pixel_state(cl2_renderer* r) {
    dev_free(r, r->d_seeds);
    for (int q = 0; q < 3; q++)
        for (int k = 0; k < 2; k++) {
            PathBufs& pb = r->sets[q][k];
            dev_free(r, pb.P0); dev_free(r, pb.P1); dev_free(r, pb.P2); dev_free(r, pb.P3);
            dev_free(r, pb.tri); dev_free(r, pb.len); dev_free(r, pb.carry);
        }
    dev_free(r, r->d_hit); dev_free(r, r->d_hit_cam0); dev_free(r, r->d_queue); dev_free(r, r->d_ctag);
    dev_free(r, r->d_det_keys); dev_free(r, r->d_det_keys_sorted); dev_free(r, r->d_det_slots); dev_free(r, r->d_det_slots_sorted);
    dev_free(r, r->d_det_vals); dev_free(r, r->d_det_tmp);
    r->det_tmp_bytes = 0;
    for (int q = 0; q < 2; q++) { dev_free(r, r->d_chit[q]); dev_free(r, r->d_cmask[q]); }
    dev_free(r, r->d_agg); dev_free(r, r->d_light_image); dev_free(r, r->d_finalized); dev_free(r, r->d_uni);
    dev_free(r, r->d_sample_w); dev_free(r, r->d_block_stats);
    for (int q = 0; q < 3; q++) dev_free(r, r->d_map[q]);
    dev_free(r, r->d_lay_agg); dev_free(r, r->d_lay_light);
}

// the per-entry buffers of the layer table: allocated when the table is set and again by cl2_set_sample_streams
int alloc_layer_entries(cl2_renderer* r) {
    if (r->n_layers == 0) return CL2_OK;
    const size_t B = (size_t)r->B, L = (size_t)r->n_layers;
    TRY(dev_alloc(r, &r->d_lay_agg, 3 * L * B));
    TRY(dev_alloc(r, &r->d_lay_light, L * B));
    HIP_TRY(r, hipMemset(r->d_lay_agg, 0, 3 * L * B * sizeof(float)));
    HIP_TRY(r, hipMemset(r->d_lay_light, 0, L * B * sizeof(float4)));
    return CL2_OK;
}

int alloc_pixel_state(cl2_renderer* r) {
    const size_t B = (size_t)r->B;
    int rc = CL2_OK;
#define A(ptr, count) if (rc == CL2_OK) rc = dev_alloc(r, &(ptr), (count))
    A(r->d_seeds, B);
    for (int q = 0; q < 3; q++) {
        for (int k = 0; k < 2; k++) {
            PathBufs& pb = r->sets[q][k];
            A(pb.P0, MAX_VERTS * B); A(pb.P1, MAX_VERTS * B); A(pb.P2, MAX_VERTS * B); A(pb.P3, MAX_VERTS * B);
            A(pb.tri, MAX_VERTS * B); A(pb.len, B); A(pb.carry, B);
        }
    }
    A(r->d_hit, B);
    A(r->d_hit_cam0, B);
    A(r->d_queue, MAX_VERTS * B);
    A(r->d_ctag, (size_t)CONN_SLOTS * B);
    for (int q = 0; q < 2; q++) { A(r->d_chit[q], (size_t)CONN_SLOTS * B); A(r->d_cmask[q], B); }
    A(r->d_agg, (size_t)AGG_ROWS * B);
    A(r->d_light_image, B); A(r->d_finalized, B); A(r->d_uni, B);
    A(r->d_sample_w, B);
    A(r->d_block_stats, (size_t)grid_for(B) * 4);
#undef A
    if (rc != CL2_OK) return rc;
    unsigned qc[9] = {(unsigned)r->B, 0, 0, 0, 0, 0, 0, 0, 2u * (unsigned)r->B};      // [8]: ray count of the merged level-0 launch
    bool ok = hipMemcpy(r->d_qcount, qc, sizeof qc, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemset(r->d_light_image, 0, B * sizeof(float4)) == hipSuccess;
    ok = ok && hipMemset(r->d_finalized, 0, B * sizeof(float4)) == hipSuccess;
    ok = ok && hipMemset(r->d_uni, 0, B * sizeof(float4)) == hipSuccess;
    ok = ok && hipMemset(r->d_sample_w, 0, B * sizeof(float)) == hipSuccess;
    ok = ok && hipMemset(r->d_agg, 0, (size_t)AGG_ROWS * B * sizeof(float)) == hipSuccess;
    ok = ok && hipMemset(r->d_block_stats, 0, (size_t)grid_for(B) * 4 * sizeof(unsigned long long)) == hipSuccess;
    for (int q = 0; q < 2 && ok; q++) ok = hipMemset(r->d_cmask[q], 0, B * sizeof(unsigned long long)) == hipSuccess;
    for (int q = 0; q < 3 && ok; q++)
        for (int k = 0; k < 2 && ok; k++) ok = hipMemset(r->sets[q][k].len, 0, B * sizeof(int)) == hipSuccess;
    // default seeds: 1 everywhere (xorshift's only forbidden state is 0); callers set real seeds
    if (ok) {
        std::vector<uint32_t> ones(2 * B, 1u);
        ok = hipMemcpy(r->d_seeds, ones.data(), 2 * B * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) return fail(r, CL2_E_HIP, "device buffer initialisation failed");
    r->cur = 0;
    return alloc_layer_entries(r);
}

#define STAGE_PROLOGUE(r)                 \
    do {                                  \
        int rc_ = need_scene(r);          \
        if (rc_ != CL2_OK) return rc_;    \
    } while (0)

// the stage calls (cl2_make_light_rays ... cl2_process_images) have no mapped form: refused while a density is set
#define STAGE_CALL_PROLOGUE(r)                                                                                              \
    do {                                                                                                                  \
        STAGE_PROLOGUE(r);                                                                                                \
        if ((r)->density) return fail((r), CL2_E_STATE, "the stage calls have no mapped form: cl2_set_sample_density(NULL) first"); \
    } while (0)


// ---------------------------------------------------------------- what the picture filters' entry points share (templates: they
// cannot stand inside the extern "C" block below, beside their callers)
// the launch shape of the filters' 16 x 16 kernels
dim3 dn_tiles(const cl2_renderer* r) { return dim3((r->W + DN_TILE - 1) / DN_TILE, (r->H + DN_TILE - 1) / DN_TILE); }
const dim3 DN_BLOCK(DN_TILE, DN_TILE);

// Where pass i of a filter reads and writes: float4 working buffers, and on a last pass that leaves a picture the packed (H, W, 3)
struct PassIO {
    const float4* cin;
    float4* cout;
    float* out3;
};
// pass 0 reads `src`, the later ones ping-pong buf[1], buf[0]; the last pass writes the packed picture to `dst`
struct PingPong {
    const float4* src;
    float4* const* buf;
    float* dst;
    int iterations;
    PassIO operator()(int i) const { return {i == 0 ? src : buf[i & 1], buf[(i + 1) & 1], i == iterations - 1 ? dst : nullptr}; }
};
// pass i reads level i and writes level i + 1 of `lev` ([levels][FB] float4): every level is kept, none is packed
struct LevelChain {
    float4* lev;
    size_t FB;
    PassIO operator()(int i) const { return {lev + (size_t)i * FB, lev + (size_t)(i + 1) * FB, nullptr}; }
};

// The pass loop of every a-trous filter: pass i runs at step 2^i, staged in LDS at steps 1 and 2 (LDS_STEP = step) and from global
// memory beyond (LDS_STEP = 0).  launch(LDS_STEP as an int_c, i, step, io(i)) launches it.  With iterations = 0 nothing is
// launched: whoever made the input wrote the picture too.
template <class IO, class Launch>
int filter_passes(cl2_renderer* r, int iterations, IO io, Launch launch) {
    for (int i = 0; i < iterations; i++) {
        const int step = 1 << i;
        if (step == 1) launch(int_c<1>{}, i, step, io(i)); else if (step == 2) launch(int_c<2>{}, i, step, io(i)); else launch(int_c<0>{}, i, step, io(i));
        HIP_TRY(r, hipGetLastError());
    }
    return CL2_OK;
}

// cl2_denoise's passes from a prepared input
template <class IO>
int denoise_passes(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo, IO io) {
    const float den_a = sigma_albedo * sigma_albedo;
    return filter_passes(r, iterations, io, [&](auto LDS_STEP, int i, int step, PassIO b) {
        const float den_c = std::ldexp(sigma_color * sigma_color, -2 * i);      // sigma_color^2 * 4^-i, exact scaling
        hipLaunchKernelGGL(k_denoise_pass<LDS_STEP.value>, dn_tiles(r), DN_BLOCK, 0, r->stream, r->W, r->H, step, den_c, sigma_depth, den_a,
                           b.cin, r->d_g0, r->d_g1, b.cout, b.out3);
    });
}

// the guided passes from a prepared input, as denoise_passes; `dvar`: where the last pass leaves its guide variance, or NULL
template <class IO>
int guided_passes(cl2_renderer* r, int iterations, float sigma_luma, float sigma_depth, float sigma_albedo, IO io, float* dvar) {
    const float den_a = sigma_albedo * sigma_albedo;
    return filter_passes(r, iterations, io, [&](auto LDS_STEP, int, int step, PassIO b) {
        hipLaunchKernelGGL(k_denoise_guided_pass<LDS_STEP.value>, dn_tiles(r), DN_BLOCK, 0, r->stream, r->W, r->H, step, sigma_luma, sigma_depth,
                           den_a, b.cin, r->d_g0, r->d_g1, b.cout, b.out3, dvar);
    });
}

// The commit of a call that keeps a picture: `produce(d_pic)` runs the checks and launches that write it.  On CL2_OK the picture
// is of `kind`; after CL2_E_HIP launches may have written part of it, so there is none; every other refusal comes before the first
// launch and the previous picture stands.  A buffer made for a call that failed goes again.
template <class Producer>
int keep_into_picture(cl2_renderer* r, int kind, Producer produce) {
    const bool fresh = !r->d_pic;
    if (fresh) TRY(dev_alloc(r, &r->d_pic, 3 * (size_t)r->FB));
    const int rc = produce(r->d_pic);
    if (rc == CL2_OK) r->pic_kind = kind;
    else if (rc == CL2_E_HIP) r->pic_kind = 0;
    if (rc != CL2_OK && fresh) dev_free(r, r->d_pic);
    return rc;
}
}  // namespace

extern "C" {

int cl2_abi_version(void) { return 6; }

int cl2_build_bvh(const double* tri_min, const double* tri_max, int64_t n_triangles, int max_members, int max_depth,
                  void* out_boxes, int64_t box_capacity, int64_t* n_boxes_out, int64_t* out_perm) {
    if (!tri_min || !tri_max || !out_boxes || !n_boxes_out || !out_perm || n_triangles < 1 || max_members < 1 ||
        n_triangles > (int64_t)1 << 30) {
        g_create_error = "cl2_build_bvh: bad argument";
        return CL2_E_INVALID;
    }
    BvhBuildResult res;
    try {
        res = build_bvh_sah(tri_min, tri_max, n_triangles, max_members, max_depth);
    } catch (const std::exception& ex) {
        g_create_error = std::string("cl2_build_bvh: ") + ex.what();
        return CL2_E_NOMEM;
    }
    if ((int64_t)res.boxes.size() > box_capacity) { g_create_error = "cl2_build_bvh: box_capacity too small"; return CL2_E_INVALID; }
    static_assert(sizeof(HostBox) == 48, "Box record");
    std::memcpy(out_boxes, res.boxes.data(), res.boxes.size() * sizeof(HostBox));
    std::memcpy(out_perm, res.perm.data(), res.perm.size() * sizeof(int64_t));
    *n_boxes_out = (int64_t)res.boxes.size();
    return CL2_OK;
}

void cl2_set_create_error(const char* msg) { g_create_error = msg ? msg : ""; }   // for the entry points of other translation units

const char* cl2_last_error(const cl2_renderer* r) { return r ? r->err.c_str() : g_create_error.c_str(); }

int cl2_create(int device_ordinal, int pixel_width, int pixel_height, cl2_renderer** out) {
    if (!out) { g_create_error = "out is NULL"; return CL2_E_INVALID; }
    *out = nullptr;
    if (pixel_width < 1 || pixel_height < 1 || (long long)pixel_width * pixel_height >= (1ll << TAG_PID_BITS)) {     // also checked per stream count
        g_create_error = "frame size out of range (need 1 <= W*H < 2^26)";
        return CL2_E_INVALID;
    }
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev < 1) {
        g_create_error = std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        return CL2_E_HIP;
    }
    if (device_ordinal < 0 || device_ordinal >= n_dev) { g_create_error = "device ordinal out of range"; return CL2_E_INVALID; }
    cl2_renderer* r = new cl2_renderer();
    r->device = device_ordinal;
    r->W = pixel_width; r->H = pixel_height; r->FB = pixel_width * pixel_height;
    r->streams = 1; r->B = r->FB;
    auto bail = [&](int code) { g_create_error = r->err; cl2_destroy(r); return code; };
    if (hipSetDevice(device_ordinal) != hipSuccess) { r->err = "hipSetDevice failed"; return bail(CL2_E_HIP); }
    if (hipStreamCreate(&r->stream) != hipSuccess || hipStreamCreate(&r->stream_conn) != hipSuccess ||
        hipStreamCreate(&r->stream_res) != hipSuccess) {
        r->err = "hipStreamCreate failed"; return bail(CL2_E_HIP);
    }
    {
        bool ok_ev = true;
        for (auto& e : r->ev_paths) ok_ev = ok_ev && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        for (auto& e : r->ev_conn) ok_ev = ok_ev && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        for (auto& e : r->ev_res) ok_ev = ok_ev && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        for (auto& e : r->ev_tune) ok_ev = ok_ev && hipEventCreate(&e) == hipSuccess;
        if (!ok_ev) { r->err = "hipEventCreate failed"; return bail(CL2_E_HIP); }
    }
    int rc = CL2_OK;
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_qcount, (size_t)9);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_work, (size_t)8 * WORK_STRIDE);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_acc, 8 * (size_t)r->FB);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_stats, (size_t)1);
    if (rc != CL2_OK) return bail(rc);
    bool ok = hipMemset(r->d_acc, 0, 8 * (size_t)r->FB * sizeof(float)) == hipSuccess;
    ok = ok && hipMemset(r->d_stats, 0, sizeof(Stats)) == hipSuccess;
    if (!ok) { r->err = "device buffer initialisation failed"; return bail(CL2_E_HIP); }
    rc = alloc_pixel_state(r);
    if (rc != CL2_OK) return bail(rc);
    *out = r;
    return CL2_OK;
}

void cl2_destroy(cl2_renderer* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    // A handle whose collective failed or timed out was torn down with ncclCommAbort; whether that retires the collective's
    // kernel on r->stream is RCCL's business (unverified on hardware: RCCL has never run here with more than one rank), and
    // an unbounded hipStreamSynchronize on that stream would turn "exit non-zero" into "hang in destroy" (ADVICE r3).  Such a
    // handle polls its streams for a few seconds and then LEAKS its device resources (hipFree would wait as well): the
    // process is on its way out with an error.
    const bool poisoned = r->comm_poisoned;
    if (r->comm) (void)cl2_comm_destroy(r);
    auto settle = [&](hipStream_t s) -> bool {
        if (!s) return true;
        if (!poisoned) { (void)hipStreamSynchronize(s); return true; }
        const auto until = std::chrono::steady_clock::now() + std::chrono::seconds(5);
        for (;;) {
            const hipError_t e = hipStreamQuery(s);
            if (e != hipErrorNotReady) return true;          // drained, or in an error state: nothing left to wait for
            if (std::chrono::steady_clock::now() > until) return false;
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
        }
    };
    const bool s0 = settle(r->stream), s1 = settle(r->stream_conn), s2 = settle(r->stream_res);   // every stream gets its poll
    if (!(s0 && s1 && s2)) {
        std::fprintf(stderr, "clive2_amd: cl2_destroy: a stream did not drain after the communicator was aborted; leaking the handle\n");
        return;
    }
    for (auto e : r->ev_paths) if (e) (void)hipEventDestroy(e);
    for (auto e : r->ev_conn) if (e) (void)hipEventDestroy(e);
    for (auto e : r->ev_res) if (e) (void)hipEventDestroy(e);
    for (auto e : r->ev_tune) if (e) (void)hipEventDestroy(e);
    for (auto& s : r->spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
    for (auto e : r->event_pool) (void)hipEventDestroy(e);
    for (void* p : r->allocs) (void)hipFree(p);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    if (r->stream_conn) (void)hipStreamDestroy(r->stream_conn);
    if (r->stream_res) (void)hipStreamDestroy(r->stream_res);
    delete r;
}

int cl2_upload_scene(cl2_renderer* r, const void* boxes_v, int n_boxes, const void* tris_v, int n_tris, const void* mats_v,
                     int n_mats, const void* camera_v, const void* light_tris_v, const float* light_areas,
                     const int32_t* light_tri_index, int light_count) {
    if (!r) return CL2_E_INVALID;
    r->features_valid = false;           // the features describe the scene they were rendered from
    PreparedScene p;
    const std::string msg = prepare_scene(boxes_v, n_boxes, tris_v, n_tris, mats_v, n_mats, camera_v, light_tris_v, light_areas,
                                          light_tri_index, light_count, r->W, r->H, p);
    if (!msg.empty()) return fail(r, CL2_E_INVALID, msg);
    // the wide walk's stack in the current child order (see ensure_wide_overflow): a tree too deep for it is not uploaded
    const int ovf_entries = p.n_wide > 0 ? wide_overflow_entries(p.max_pending, p.order_depth, r->traversal_order) : 0;
    if (ovf_entries < 0) {
        r->scene_ok = false;
        return fail(r, CL2_E_INVALID, "tree too deep for the nearest-first child order: its 4-wide stack can reach " + std::to_string(p.order_depth) +
                                      " entries, the limit is " + std::to_string(WIDE_STACK_LDS + WIDE_STACK_OVERFLOW) + " (cl2_set_traversal_order(0) first)");
    }

    HIP_TRY(r, hipSetDevice(r->device));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    r->scene_ok = false;
    dev_free(r, r->d_nodes); dev_free(r, r->d_tris); dev_free(r, r->d_tri_shade);
    dev_free(r, r->d_mats); dev_free(r, r->d_light_tris); dev_free(r, r->d_light_areas); dev_free(r, r->d_light_tri_index);
    dev_free(r, r->d_wide); dev_free(r, r->d_tris36); dev_free(r, r->d_tri_rank); dev_free(r, r->d_fast);
    r->wide.tris36 = nullptr; r->wide.tri_rank = nullptr;
    r->bvh.fast_nodes = nullptr; r->bvh.n_fast_nodes = 0;
    r->n_wide = 0;
    TRY(upload(r, &r->d_nodes, p.nodes.data(), p.nodes.size()));
    TRY(upload(r, &r->d_tris, p.tris.data(), p.tris.size()));
    TRY(upload(r, &r->d_tri_shade, p.shade.data(), p.shade.size()));
    TRY(upload(r, &r->d_mats, p.mats.data(), p.mats.size()));
    TRY(upload(r, &r->d_light_tris, p.ltris.data(), p.ltris.size()));
    TRY(upload(r, &r->d_light_areas, light_areas, (size_t)light_count));
    TRY(upload(r, &r->d_light_tri_index, light_tri_index, (size_t)light_count));
    if (p.n_wide > 0) {
        TRY(upload(r, &r->d_tris36, p.tris36.data(), p.tris36.size()));
        TRY(upload(r, &r->d_wide, p.wide.data(), p.wide.size()));
        TRY(upload(r, &r->d_tri_rank, p.tri_rank.data(), p.tri_rank.size()));
        // deepest wide stack of THIS tree (see ensure_wide_overflow); a new scene may need a different size
        if (ovf_entries != r->wide_ovf_entries) { dev_free(r, r->d_wide_ovf); r->wide_ovf_entries = ovf_entries; }
        r->max_pending = p.max_pending; r->order_depth = p.order_depth;
        const BoxRec& root = static_cast<const BoxRec*>(boxes_v)[0];
        r->wide.nodes = r->d_wide; r->wide.tris = r->d_tris; r->wide.tris36 = r->d_tris36;
        r->wide.tri_rank = r->d_tri_rank + 1;   // read on exact-t ties only (ORDER); [-1] ranks "nothing held"
        r->wide.root_lo = make_float4(root.min[0], root.min[1], root.min[2], 0.0f);
        r->wide.root_hi = make_float4(root.max[0], root.max[1], root.max[2], 0.0f);
        r->n_wide = p.n_wide;
    }
    r->bvh.nodes = r->d_nodes; r->bvh.tris = r->d_tris;
    r->bvh.n_nodes = p.n_records; r->bvh.n_tris = n_tris;
    r->bvh.n_lds_nodes = std::min(p.n_records, LDS_NODE_CAP);
    r->bvh.lds_tris = n_tris <= LDS_TRI_CAP ? 1 : 0;
    if (p.n_fast > 0) {
        TRY(upload(r, &r->d_fast, p.fast.data(), p.fast.size()));
        r->bvh.fast_nodes = r->d_fast; r->bvh.n_fast_nodes = ((r->debug_flags >> 7) & 1) ? 0 : p.n_fast;
    }
    r->n_fast = p.n_fast;
    r->fast_flat = p.fast_flat;
    r->bvh.fast_flat = flat_walk(r);
    r->n_mats = n_mats; r->light_count = light_count; r->cam = p.cam;
    r->cam_tris = p.cam_tris;
    r->n_top = p.n_top;
    r->scene_ok = true;
    r->paths_share = 0;                  // re-tune the stage shares for the new scene
    r->levels_auto = 0;
    return CL2_OK;
}

int cl2_set_seeds(cl2_renderer* r, const uint32_t* seeds, size_t n_words) {
    if (!r || !seeds) return CL2_E_INVALID;
    if (n_words != 2 * (size_t)r->B) return fail(r, CL2_E_INVALID, "seed buffer must hold 2 words per pixel and sample stream (stream-major)");
    HIP_TRY(r, hipSetDevice(r->device));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipMemcpy(r->d_seeds, seeds, n_words * sizeof(uint32_t), hipMemcpyHostToDevice));
    return CL2_OK;
}

int cl2_get_seeds(cl2_renderer* r, uint32_t* seeds, size_t n_words) {
    if (!r || !seeds) return CL2_E_INVALID;
    if (n_words != 2 * (size_t)r->B) return fail(r, CL2_E_INVALID, "seed buffer must hold 2 words per pixel and sample stream (stream-major)");
    HIP_TRY(r, hipSetDevice(r->device));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipMemcpy(seeds, r->d_seeds, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CL2_OK;
}

/* K independent samples of the frame per pass.  Stream k has its own seed words [2*k*W*H, 2*(k+1)*W*H) of
 * the seed buffer and is exactly what a Renderer with that seed buffer -- rank k of the sample split -- would render; the
 * accumulators receive the streams' samples in stream order.  Every launch then covers K x W x H entries: a per-level subpath
 * launch of a 1080p frame is 2 M rays on 524 k resident lanes and all tail; with K = 4 it is the 8.3 M rays of a 4K frame.
 * Frees and re-allocates the per-pixel state (seeds back to 1: set them again), keeps scene, accumulators and counters. */
int cl2_set_sample_streams(cl2_renderer* r, int streams) {
    if (!r) return CL2_E_INVALID;
    if (streams < 1 || (long long)streams * r->FB >= (1ll << TAG_PID_BITS))
        return fail(r, CL2_E_INVALID, "sample streams: need streams >= 1 and streams * W * H < 2^26 (pixel-entry bits of a connection tag)");
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    if (streams == r->streams) return CL2_OK;
    const int before = r->streams;
    free_pixel_state(r);
    r->streams = streams; r->B = streams * r->FB; r->export_stream = 0;
    r->paths_share = 0; r->levels_auto = 0;                       // launch sizes changed: measure the organisation again
    int rc = alloc_pixel_state(r);
    if (rc != CL2_OK) {
        // not enough device memory for that many streams (about 3.4 KB per entry): the handle goes back to what it had
        const std::string why = r->err;
        free_pixel_state(r);
        r->streams = before; r->B = before * r->FB;
        if (alloc_pixel_state(r) != CL2_OK) { r->scene_ok = false; return fail(r, rc, why + "; and the previous stream count could not be restored: the handle is unusable"); }
        return fail(r, rc, why + " (sample streams unchanged; seeds were reset)");
    }
    return CL2_OK;
}
int cl2_get_sample_streams(const cl2_renderer* r) { return r ? r->streams : CL2_E_INVALID; }
/* the stream that cl2_export_* / cl2_import_sample_images address (one frame's worth of records each) */
int cl2_set_export_stream(cl2_renderer* r, int stream) {
    if (!r) return CL2_E_INVALID;
    if (stream < 0 || stream >= r->streams) return fail(r, CL2_E_INVALID, "export stream out of range");
    r->export_stream = stream;
    return CL2_OK;
}

int cl2_make_light_rays(cl2_renderer* r) { STAGE_CALL_PROLOGUE(r); TRY(launch_generate(r, CL2_LIGHT, r->stream, r->sets[r->cur])); return drain(r); }
int cl2_make_camera_rays(cl2_renderer* r) { STAGE_CALL_PROLOGUE(r); TRY(launch_generate(r, CL2_CAMERA, r->stream, r->sets[r->cur])); return drain(r); }
int cl2_trace_light_rays(cl2_renderer* r) { STAGE_CALL_PROLOGUE(r); TRY(launch_subpaths(r, r->stream, r->sets[r->cur], 1)); return drain(r); }
int cl2_trace_camera_rays(cl2_renderer* r) { STAGE_CALL_PROLOGUE(r); TRY(launch_subpaths(r, r->stream, r->sets[r->cur], 2)); return drain(r); }
int cl2_join_paths(cl2_renderer* r) {
    STAGE_CALL_PROLOGUE(r);
    TRY(launch_connect(r, r->stream, r->sets[r->cur], 0));
    TRY(launch_resolve(r, r->stream, r->sets[r->cur], 0));
    return drain(r);
}
int cl2_finalize_samples(cl2_renderer* r) { STAGE_CALL_PROLOGUE(r); TRY(launch_finalize(r, r->stream)); return drain(r); }
/* The t=1 splats were added to the light image by join_paths (float atomics); nothing is left of the
 * reference's sort + bincount + gather (src/renderer.py:212-250) but a synchronisation point. */
int cl2_gather_light_image(cl2_renderer* r) { STAGE_CALL_PROLOGUE(r); return drain(r); }
int cl2_process_images(cl2_renderer* r) {
    STAGE_CALL_PROLOGUE(r);
    TRY(launch_accumulate(r, r->stream));
    r->samples += (uint64_t)r->streams;
    r->cam_uniform += (uint64_t)r->streams;
    return drain(r);
}

/* n x run_sample as a three-stage pipeline over samples.  The only state a sample hands to the next
 * one is the seed buffer, and only the subpath stage (K1, K2, K3) touches it.  So with three subpath
 * buffer sets and two {hit, mask} sets
 *     stream       : subpaths of sample i+2
 *     stream_conn  : connection set-up + connection rays of sample i+1
 *     stream_res   : resolve, K6, accumulation of sample i
 * run side by side.  Every launch ends in a tail of a few long rays or late workgroups, the
 * streaming kernels leave the VALUs idle and the resolve kernel the memory system: the other stages'
 * workgroups fill what is left.  Each kernel sees exactly the inputs it would see in the serial
 * order (sums into the accumulators stay in sample order on stream_res), so results do not change. */
namespace {
// rays traced by the subpath kernels so far (per-workgroup slots, summed here)
int subpath_ray_tally(cl2_renderer* r, unsigned long long* out) {
    TRY(drain(r));
    std::vector<unsigned long long> slots((size_t)grid_for(r->B) * 4);
    HIP_TRY(r, hipMemcpy(slots.data(), r->d_block_stats, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long t = 0;
    for (size_t b = 0; b < slots.size(); b += 4) t += slots[b];
    *out = t;
    return CL2_OK;
}

// `count` samples, serial (one stream, the current buffer set) or pipelined (rotating sets, starting with
// the current one); ends with everything complete and `cur` = the set of the last sample.
// `steady`: r->tune_period_ms = the time from the end of the first sample to the end of the last one, per sample -- what a long run
// costs per sample, without the fill of the pipeline (the first sample's subpath stage has nothing beside it).
int ensure_maps(cl2_renderer* r) {
    for (int q = 0; q < 3; q++)
        if (!r->d_map[q]) TRY(dev_alloc(r, &r->d_map[q], (size_t)r->B));
    return CL2_OK;
}

int run_chunk(cl2_renderer* r, bool pipe, int count, bool steady = false) {
    const int first_set = r->cur;
    const bool mapped = r->density;           // adaptive sampling: every pass writes its set's slot map first (adaptive.hpp)
    if (mapped) TRY(ensure_maps(r));
    r->pipe_active = pipe;
    for (int i = 0; i < count; i++) {
        const int ps = pipe ? (first_set + i) % 3 : r->cur, cs = pipe ? (i & 1) : 0;
        const PathBufs* set = r->sets[ps];
        hipStream_t s_conn = pipe ? r->stream_conn : r->stream;
        hipStream_t s_res = pipe ? (pipeline_stages(r) == 2 ? r->stream_res : r->stream_conn) : r->stream;
        // resolve of sample i-3 was the last reader of this subpath set
        if (pipe && i >= 3) HIP_TRY(r, hipStreamWaitEvent(r->stream, r->ev_res[(i - 3) % 6], 0));
        // (the map belongs to the subpath set: the same event orders its reuse)
        const int* map = mapped ? r->d_map[ps] : nullptr;
        const uint32_t pass = mapped ? r->dens_pass++ : 0u;
        if (mapped) {
            Timed t(r, ST_GENERATE, r->stream);
            hipLaunchKernelGGL(k_dens_expand, dim3(grid_for(r->B)), dim3(BLOCK), 0, r->stream, r->B, r->FB, (const uint64_t*)r->d_dens_C,
                               pass, r->d_map[ps]);
            HIP_TRY(r, hipGetLastError());
        }
        TRY(launch_generate_both(r, r->stream, set, map));
        TRY(launch_subpaths(r, r->stream, set, 3));
        if (pipe) {
            HIP_TRY(r, hipEventRecord(r->ev_paths[i % 3], r->stream));
            HIP_TRY(r, hipStreamWaitEvent(s_conn, r->ev_paths[i % 3], 0));
            // resolve of sample i-2 was the last reader of this {hit, mask} set
            if (i >= 2) HIP_TRY(r, hipStreamWaitEvent(s_conn, r->ev_res[(i - 2) % 6], 0));
        }
        TRY(launch_connect(r, s_conn, set, cs));
        if (pipe) {
            HIP_TRY(r, hipEventRecord(r->ev_conn[i & 1], s_conn));
            HIP_TRY(r, hipStreamWaitEvent(s_res, r->ev_conn[i & 1], 0));
        }
        TRY(launch_resolve(r, s_res, set, cs, map));
        TRY(launch_finalize_accumulate(r, s_res, mapped, pass));
        if (steady && count >= 2 && (i == 0 || i == count - 1)) HIP_TRY(r, hipEventRecord(r->ev_tune[i == 0 ? 0 : 1], s_res));
        if (pipe) HIP_TRY(r, hipEventRecord(r->ev_res[i % 6], s_res));
        r->samples += (uint64_t)r->streams;
        if (!mapped) r->cam_uniform += (uint64_t)r->streams;
        // bound the number of in-flight event pairs while profiling
        if (r->profiling && r->spans.size() > 4096) TRY(drain(r));
    }
    r->pipe_active = false;
    TRY(drain(r));
    if (steady && count >= 2) {
        float ms = 0.0f;
        HIP_TRY(r, hipEventElapsedTime(&ms, r->ev_tune[0], r->ev_tune[1]));
        r->tune_period_ms = (double)ms / (count - 1);
    }
    if (pipe && count > 0) r->cur = (first_set + count - 1) % 3;
    return CL2_OK;
}
}  // namespace

namespace {
// The automatic choices that need measurements of the scene.  Both render real samples (every candidate
// organisation gives identical results), `done` counts them.
//
// Small scenes, levels_per_launch = 0: one whole-subpath launch keeps a wave busy as long as its
// longest path lives.  In a closed scene that is every path (6.0 rays per subpath: nothing to gain,
// compaction costs 35 %); in an open scene most paths leave after a bounce or two and a wave idles on
// its last survivor.  The first sample of a scene tells which: below 4 rays per subpath the walk is cut
// into launches of 2 bounces with the survivors compacted in between (open test scene: 2.02 -> 1.62 ms).
int tune_levels(cl2_renderer* r, int& done) {
    if (split_paths(r) || r->levels_per_launch != 0 || r->levels_auto != 0) return CL2_OK;
    unsigned long long before = 0, after = 0;
    TRY(subpath_ray_tally(r, &before));
    TRY(run_chunk(r, false, 1));
    TRY(subpath_ray_tally(r, &after));
    done += 1;
    r->levels_auto = (double)(after - before) < 4.0 * 2.0 * (double)r->B ? 2 : (int)MAX_VERTS;
    return CL2_OK;
}
// Large scenes: how the two stages share the machine while the pipeline runs.  Persistent launches hold
// their wave slots until they run dry, so the stages get fixed shares (persistent_grid_paths/_conn) -- 3, 4
// or 5 eighths for the subpath stage, no fixed shares, or the serial order.  The best choice depends on the
// scene and the frame size; every candidate renders TUNE_SAMPLES samples and is timed on the host.
constexpr int TUNE_TOTAL = 9 * TUNE_SAMPLES;     // five candidates once, the best two twice more
inline bool shares_untuned(const cl2_renderer* r) { return pipeline_stages(r) != 0 && split_conn(r) && r->paths_share == 0; }
int tune_shares(cl2_renderer* r, int& done) {
    if (!shares_untuned(r)) return CL2_OK;
    const int cand[5] = {3, 4, 5, 8, SHARE_SERIAL};
    double t_of[5];
    auto time_one = [&](int e, double& t) -> int {
        // Timed on the device from the end of the candidate's first sample to the end of its last: the host clock around six
        // samples charged a pipelined organisation its fill (about one sample in six) and the serial order nothing -- round 5: with
        // one sample stream the tuner took the serial order (8.35 / 10.3 ms per sample on the 5k- / 82k-triangle scene) although the
        // pipelined one runs at 8.0 / 9.9 in a long call.
        r->paths_share = e;
        TRY(run_chunk(r, e != SHARE_SERIAL, TUNE_SAMPLES, true));
        t = r->tune_period_ms;
        done += TUNE_SAMPLES;
        return CL2_OK;
    };
    for (int k = 0; k < 5; k++) TRY(time_one(cand[k], t_of[k]));
    // the two best twice more, in turn: neighbouring organisations differ by a few per cent and one timing of six samples by about
    // as much (round 5: on the 5k-triangle scene with one sample stream the pipelined order, 7.99 ms per sample, lost the run-off
    // against the serial order, 8.35, in four tunings out of five when each was timed once more)
    int a = 0, b = 1;
    if (t_of[b] < t_of[a]) std::swap(a, b);
    for (int k = 2; k < 5; k++) {
        if (t_of[k] < t_of[a]) { b = a; a = k; }
        else if (t_of[k] < t_of[b]) b = k;
    }
    double ta = 0, tb = 0;
    for (int round = 0; round < 2; round++) {
        double t1 = 0, t2 = 0;
        TRY(time_one(cand[a], t1));
        TRY(time_one(cand[b], t2));
        ta += t1; tb += t2;
    }
    r->paths_share = (t_of[a] + ta <= t_of[b] + tb) ? cand[a] : cand[b];
    return CL2_OK;
}
}  // namespace

int cl2_run_samples(cl2_renderer* r, int n) {
    STAGE_PROLOGUE(r);
    if (n < 0) return fail(r, CL2_E_INVALID, "negative sample count");
    bool pipe = pipeline_stages(r) != 0 && n > 1;
    int done = 0;
    if (n >= 2) TRY(tune_levels(r, done));
    // the share tuner runs inside the first LONG call of a scene (its 54 samples are part of the call's n) unless
    // cl2_tune() ran it before
    if (pipe && n - done >= TUNE_TOTAL + TUNE_SAMPLES + 6) TRY(tune_shares(r, done));
    if (pipe && split_conn(r) && r->paths_share == SHARE_SERIAL) pipe = false;
    return run_chunk(r, pipe, n - done);
}

/* Makes the measured choices of the launch organisation NOW instead of inside the first (long) cl2_run_samples
 * call: the levels-per-launch probe of a small scene (1 sample) and the stage-share tuner of a large one (54
 * samples: TUNE_TOTAL).  The samples are real ones -- they advance the seeds and add to the accumulators exactly as the same
 * number of run_sample iterations would -- and *samples_rendered says how many there were.  A benchmark calls
 * this in its warm-up so that no timing experiment runs inside its clock. */
int cl2_tune(cl2_renderer* r, int* samples_rendered) {
    STAGE_PROLOGUE(r);
    int done = 0;
    TRY(tune_levels(r, done));
    TRY(tune_shares(r, done));
    if (samples_rendered) *samples_rendered = done;
    return CL2_OK;
}

int cl2_set_pipelining(cl2_renderer* r, int on) {
    if (!r) return CL2_E_INVALID;
    if (on < -1 || on > 2) return fail(r, CL2_E_INVALID, "pipelining must be -1..2");
    r->pipelining = on;
    return CL2_OK;
}

int cl2_read_accumulators(cl2_renderer* r, float* img, float* wts, int32_t* counts, float* uni, size_t n_pixels) {
    if (!r) return CL2_E_INVALID;
    if (n_pixels != (size_t)r->FB) return fail(r, CL2_E_INVALID, "n_pixels must equal W*H");
    HIP_TRY(r, hipSetDevice(r->device));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    const size_t B = r->FB;
    std::vector<float> h(8 * B);
    HIP_TRY(r, hipMemcpy(h.data(), r->d_acc, 8 * B * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t p = 0; p < B; p++) {
        if (img) { img[3 * p] = h[p]; img[3 * p + 1] = h[B + p]; img[3 * p + 2] = h[2 * B + p]; }
        if (wts) wts[p] = h[3 * B + p];
        if (uni) { uni[3 * p] = h[4 * B + p]; uni[3 * p + 1] = h[5 * B + p]; uni[3 * p + 2] = h[6 * B + p]; }
        if (counts) counts[p] = (int32_t)std::lrintf(h[7 * B + p]);
    }
    return CL2_OK;
}

namespace {
// The side sums of the accumulators: moments (error_estimate.hpp), buckets (robust.hpp), layer accumulators (layers.hpp) and split
// rows (error_split.hpp).  Each
// is a float array that exists while its feature is on, and a flag: every addend in the accumulators also went into the side sum.
// The rules of that flag, for all of them:
//   switched on           valid if the accumulators hold nothing yet (side_sum_on)
//   cl2_reset_accumulators  zeroed, and valid if present (reset_side_sums)
//   accumulators written by the caller  invalid (invalidate_side_sums) until the matching cl2_write_*_packed brings the side sum
struct SideSum { float*& p; size_t n_floats; bool& valid; };
inline std::array<SideSum, 4> side_sums(cl2_renderer* r) {
    const size_t FB = (size_t)r->FB;
    return {{{r->d_mom, 8 * FB, r->mom_valid}, {r->d_bkt, 4 * (size_t)r->bkt_M * FB, r->bkt_valid}, {r->d_lacc, 3 * (size_t)r->n_layers * FB, r->lay_valid},
             {r->d_smom, (size_t)SPLIT_ROWS * FB, r->smom_valid}}};
}
int reset_side_sums(cl2_renderer* r) {
    for (SideSum& s : side_sums(r)) {
        if (s.p) HIP_TRY(r, hipMemset(s.p, 0, s.n_floats * sizeof(float)));
        s.valid = s.p != nullptr;
    }
    return CL2_OK;
}
void invalidate_side_sums(cl2_renderer* r) {
    for (SideSum& s : side_sums(r)) s.valid = false;
}
// allocates and zeroes a side sum of n floats; `what` names it in the error text
int side_sum_on(cl2_renderer* r, float*& p, size_t n_floats, bool& valid, const char* what) {
    TRY(dev_alloc(r, &p, n_floats));
    if (hipMemset(p, 0, n_floats * sizeof(float)) != hipSuccess) return fail(r, CL2_E_HIP, std::string(what) + ": initialisation failed");
    valid = r->acc_clean;                // samples rendered without it: invalid until cl2_reset_accumulators
    return CL2_OK;
}
// what every read / write of packed accumulators or side sums ends in, after the entry point's own refusals
int packed_copy(cl2_renderer* r, void* dst, const void* src, size_t n_floats, hipMemcpyKind kind) {
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    HIP_TRY(r, hipMemcpy(dst, src, n_floats * sizeof(float), kind));
    return CL2_OK;
}
}  // namespace

int cl2_reset_accumulators(cl2_renderer* r) {
    if (!r) return CL2_E_INVALID;
    HIP_TRY(r, hipSetDevice(r->device));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipMemset(r->d_acc, 0, 8 * (size_t)r->FB * sizeof(float)));
    if (r->d_cam_count) HIP_TRY(r, hipMemset(r->d_cam_count, 0, (size_t)r->FB * sizeof(unsigned)));
    r->cam_uniform = 0;
    TRY(reset_side_sums(r));
    r->acc_clean = true;
    r->samples = 0;
    return CL2_OK;
}

int cl2_read_accumulators_packed(cl2_renderer* r, float* dst, size_t n_floats) {
    if (!r || !dst) return CL2_E_INVALID;
    if (n_floats != 8 * (size_t)r->FB) return fail(r, CL2_E_INVALID, "packed accumulators hold 8*W*H floats");
    return packed_copy(r, dst, r->d_acc, n_floats, hipMemcpyDeviceToHost);
}
int cl2_write_accumulators_packed(cl2_renderer* r, const float* src, size_t n_floats) {
    if (!r || !src) return CL2_E_INVALID;
    if (n_floats != 8 * (size_t)r->FB) return fail(r, CL2_E_INVALID, "packed accumulators hold 8*W*H floats");
    TRY(packed_copy(r, r->d_acc, src, n_floats, hipMemcpyHostToDevice));
    r->acc_clean = false;
    invalidate_side_sums(r);
    return CL2_OK;
}

// ---------------------------------------------------------------- output stage: tone map on the device (csrc/tonemap.hpp)
namespace {
int tone_buffers(cl2_renderer* r) {
    if (!r->d_tone_partial) TRY(dev_alloc(r, &r->d_tone_partial, (size_t)TONE_BLOCKS + 1));
    if (!r->d_tone_out) TRY(dev_alloc(r, &r->d_tone_out, (size_t)3 * r->FB));
    return CL2_OK;
}
}  // namespace

int cl2_tone_log_sum(cl2_renderer* r, int which, double* sum_out) {
    if (!r || !sum_out) return CL2_E_INVALID;
    if (which < 0 || which > 2) return fail(r, CL2_E_INVALID, "picture: 0 image, 1 unweighted_image, 2 unidirectional_image");
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    TRY(tone_buffers(r));
    const int grid = std::min(grid_for(r->FB), TONE_BLOCKS);
    hipLaunchKernelGGL(k_tone_logsum, dim3(grid), dim3(256), 0, r->stream, r->d_acc, r->FB, which, r->d_tone_partial);
    hipLaunchKernelGGL(k_tone_logsum_final, dim3(1), dim3(256), 0, r->stream, r->d_tone_partial, grid, r->d_tone_partial + TONE_BLOCKS);
    HIP_TRY(r, hipGetLastError());
    HIP_TRY(r, hipMemcpyAsync(sum_out, r->d_tone_partial + TONE_BLOCKS, sizeof(double), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    return CL2_OK;
}

int cl2_tone_map(cl2_renderer* r, int which, double exposure, double white_point, double log_average, uint8_t* out_bgr, size_t n_bytes) {
    if (!r || !out_bgr) return CL2_E_INVALID;
    if (which < 0 || which > 2) return fail(r, CL2_E_INVALID, "picture: 0 image, 1 unweighted_image, 2 unidirectional_image");
    if (n_bytes != (size_t)3 * r->FB) return fail(r, CL2_E_INVALID, "the tone-mapped picture holds 3*W*H bytes");
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    TRY(tone_buffers(r));
    hipLaunchKernelGGL(k_tone_apply, dim3(grid_for(r->FB)), dim3(256), 0, r->stream, r->d_acc, r->FB, which, exposure, white_point * white_point,
                       log_average, r->d_tone_out);
    HIP_TRY(r, hipGetLastError());
    HIP_TRY(r, hipMemcpyAsync(out_bgr, r->d_tone_out, n_bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    return CL2_OK;
}

// ---------------------------------------------------------------- multi-GPU: RCCL behind the C ABI
namespace {
constexpr int COMM_SCRATCH = 16;
#define RCCL_TRY(r, api, expr)                                                                    \
    do {                                                                                          \
        ncclResult_t e_ = (expr);                                                                 \
        if (e_ != ncclSuccess) {                                                                  \
            (r)->err = std::string(#expr) + ": " + (api)->GetErrorString(e_);                     \
            return CL2_E_COMM;                                                                    \
        }                                                                                         \
    } while (0)
}  // namespace

int cl2_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int cl2_synchronize(cl2_renderer* r) {
    if (!r) return CL2_E_INVALID;
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    HIP_TRY(r, hipDeviceSynchronize());
    return CL2_OK;
}

int cl2_comm_unique_id_bytes(void) { return (int)sizeof(ncclUniqueId); }

int cl2_comm_get_unique_id(void* out, size_t n_bytes) {
    if (!out || n_bytes != sizeof(ncclUniqueId)) { g_create_error = "cl2_comm_get_unique_id: the id is cl2_comm_unique_id_bytes() long"; return CL2_E_INVALID; }
    std::string why;
    RcclApi* api = rccl_api(why);
    if (!api) { g_create_error = why; return CL2_E_COMM; }
    ncclUniqueId id;
    const ncclResult_t e = api->GetUniqueId(&id);
    if (e != ncclSuccess) { g_create_error = std::string("ncclGetUniqueId: ") + api->GetErrorString(e); return CL2_E_COMM; }
    std::memcpy(out, &id, sizeof id);
    return CL2_OK;
}

int cl2_comm_init_rank(cl2_renderer* r, int nranks, int rank, const void* unique_id, size_t n_bytes) {
    if (!r) return CL2_E_INVALID;
    if (!unique_id || n_bytes != sizeof(ncclUniqueId)) return fail(r, CL2_E_INVALID, "unique id must be cl2_comm_unique_id_bytes() long");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(r, CL2_E_INVALID, "need 0 <= rank < nranks");
    if (r->comm) return fail(r, CL2_E_STATE, "this renderer already has a communicator (cl2_comm_destroy first)");
    if (r->density || r->adaptive) return fail(r, CL2_E_STATE, "adaptive sampling is per handle: cl2_set_sample_density(NULL) and cl2_set_adaptive_sampling(0) first");
    std::string why;
    RcclApi* api = rccl_api(why);
    if (!api) return fail(r, CL2_E_COMM, why);
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    if (!r->d_comm_scratch) TRY(dev_alloc(r, &r->d_comm_scratch, (size_t)COMM_SCRATCH));
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof id);
    ncclComm_t comm = nullptr;
    RCCL_TRY(r, api, api->CommInitRank(&comm, nranks, id, rank));
    r->comm = comm; r->comm_rank = rank; r->comm_nranks = nranks;
    r->comm_poisoned = false;
    return CL2_OK;
}

namespace {
// Deadline for one collective (seconds): CLIVE2_COMM_TIMEOUT_S, default 300.  Ranks reach the reduce at
// different times (scene set-up, sample counts that differ by one), so the default is generous; what it
// bounds is the wait for a rank that will never come.
double comm_deadline_seconds() {
    if (const char* e = std::getenv("CLIVE2_COMM_TIMEOUT_S")) {
        char* end = nullptr;
        const double v = std::strtod(e, &end);
        if (end != e && v > 0.0) return v;
    }
    return 300.0;
}

// Tear the communicator down without waiting for anybody: ncclCommAbort ends kernels of it that are still
// spinning on a peer and frees its resources.  Used after a failed / timed-out collective and whenever the
// handle goes away in a failed state -- a clean ncclCommDestroy would itself wait for outstanding work.
void comm_abort(cl2_renderer* r, RcclApi* api) {
    if (!r->comm) return;
    ncclComm_t comm = r->comm;
    r->comm = nullptr; r->comm_nranks = 0; r->comm_rank = 0;
    if (api && api->CommAbort) (void)api->CommAbort(comm);
}

// Wait for the collective just enqueued on r->stream: polls the stream and the communicator's asynchronous
// error state under the deadline (comm_wait.hpp).  On any failure the communicator is aborted and the
// handle keeps the reason; the caller returns CL2_E_COMM and the process is expected to exit non-zero.
int comm_wait(cl2_renderer* r, RcclApi* api, const char* what) {
    int detail = 0;
    const double deadline = comm_deadline_seconds();
    const WaitResult res = wait_collective(
        [&]() -> int {
            const hipError_t e = hipStreamQuery(r->stream);
            return e == hipSuccess ? 0 : (e == hipErrorNotReady ? 1 : -(int)e);
        },
        [&]() -> int {
            ncclResult_t ae = ncclSuccess;
            if (!api->CommGetAsyncError || api->CommGetAsyncError(r->comm, &ae) != ncclSuccess) return 0;
            return (ae == ncclSuccess || ae == ncclInProgress) ? 0 : (int)ae;
        },
        deadline, &detail);
    if (res == WAIT_DONE) return CL2_OK;
    std::string why = std::string(what) + ": ";
    if (res == WAIT_TIMEOUT) why += "not complete after " + std::to_string((int)deadline) + " s (a rank never joined the collective?); communicator aborted";
    else if (res == WAIT_ASYNC_ERROR) why += std::string("asynchronous RCCL error: ") + api->GetErrorString((ncclResult_t)detail) + "; communicator aborted";
    else why += std::string("stream error: ") + hipGetErrorString((hipError_t)(-detail)) + "; communicator aborted";
    r->comm_poisoned = true;
    comm_abort(r, api);
    r->err = why;
    return CL2_E_COMM;
}

// every failure between "communicator exists" and "collective complete" poisons the communicator: the peers are
// (or will be) inside the collective and this rank will not complete it
#define COMM_HIP_TRY(r, api, expr)                                                                 \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (r)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                         \
            (r)->comm_poisoned = true; comm_abort((r), (api));                                    \
            return CL2_E_HIP;                                                                     \
        }                                                                                         \
    } while (0)
#define COMM_RCCL_TRY(r, api, expr)                                                                \
    do {                                                                                          \
        ncclResult_t e_ = (expr);                                                                 \
        if (e_ != ncclSuccess) {                                                                  \
            (r)->err = std::string(#expr) + ": " + (api)->GetErrorString(e_);                     \
            (r)->comm_poisoned = true; comm_abort((r), (api));                                    \
            return CL2_E_COMM;                                                                    \
        }                                                                                         \
    } while (0)
}  // namespace

/* The collective of SURVEY.md 8e: in place, on the stream every accumulating kernel ran on (drained
 * first: with the sample pipeline the accumulation runs on stream_res).  The wait for it has a deadline
 * (comm_wait): a rank that never joins makes this call fail with CL2_E_COMM instead of blocking for ever. */
int cl2_reduce_accumulators(cl2_renderer* r) {
    if (!r) return CL2_E_INVALID;
    if (!r->comm) return fail(r, CL2_E_STATE, r->comm_poisoned ? "the communicator was aborted after a failed collective" : "no communicator (call cl2_comm_init_rank first)");
    std::string why;
    RcclApi* api = rccl_api(why);
    if (!api) return fail(r, CL2_E_COMM, why);
    COMM_HIP_TRY(r, api, hipSetDevice(r->device));
    // error tracking: every rank must issue the same collectives.  One small all-reduce (max over [t, -t]: the largest and the
    // smallest t of the ranks) first, t = 0 tracking off, 1 on with invalid moments, 2 on with valid ones
    // robust buckets: the same for M (0 off) and for their validity (1 valid); they are reduced when M is the same > 0 everywhere
    const double t = r->d_mom ? (r->mom_valid ? 2.0 : 1.0) : 0.0;
    const double bm = r->d_bkt ? (double)r->bkt_M : 0.0, bv = r->d_bkt && r->bkt_valid ? 1.0 : 0.0;
    double tt[6] = {t, -t, bm, -bm, bv, -bv};
    TRY(cl2_comm_allreduce_f64(r, tt, 6, 1));
    const double t_max = tt[0], t_min = -tt[1], bm_max = tt[2], bm_min = -tt[3], bv_min = -tt[5];
    const bool bkt_agree = bm_min == bm_max;
    {
        const int rc = drain(r);
        if (rc != CL2_OK) { r->comm_poisoned = true; comm_abort(r, api); return rc; }
    }
    COMM_RCCL_TRY(r, api, api->AllReduce(r->d_acc, r->d_acc, 8 * (size_t)r->FB, ncclFloat, ncclSum, r->comm, r->stream));
    if (t_min >= 1.0)
        COMM_RCCL_TRY(r, api, api->AllReduce(r->d_mom, r->d_mom, 8 * (size_t)r->FB, ncclFloat, ncclSum, r->comm, r->stream));
    if (bkt_agree && bm_min >= 1.0)
        COMM_RCCL_TRY(r, api, api->AllReduce(r->d_bkt, r->d_bkt, 4 * (size_t)r->bkt_M * (size_t)r->FB, ncclFloat, ncclSum, r->comm, r->stream));
    TRY(comm_wait(r, api, "cl2_reduce_accumulators"));
    r->acc_clean = false;
    r->mom_valid = t_min == 2.0;
    r->bkt_valid = bkt_agree && bm_min >= 1.0 && bv_min == 1.0;
    r->smom_valid = false;               // the split rows are not reduced (error_split.hpp, DESIGN 6.17: a limit): cl2_reset_accumulators
    if (!bkt_agree)
        return fail(r, CL2_E_STATE, "the robust buckets are off on some ranks or differ in M: the accumulators were reduced, the buckets "
                                    "are invalid on every rank (cl2_reset_accumulators makes them valid again)");
    if (t_min == 0.0 && t_max >= 1.0)
        return fail(r, CL2_E_STATE, "error tracking is on on some ranks and off on others: the accumulators were reduced, the moments "
                                    "are invalid on every rank (cl2_reset_accumulators makes them valid again)");
    return CL2_OK;
}

/* n <= 16 host doubles, summed (op 0) or maximised (op 1) over the ranks, in place: barrier, the
 * max-over-ranks clock and the whole-job ray tally of bench.py / render.py. */
int cl2_comm_allreduce_f64(cl2_renderer* r, double* values, int n, int op) {
    if (!r || !values) return CL2_E_INVALID;
    if (n < 1 || n > COMM_SCRATCH || (op != 0 && op != 1)) return fail(r, CL2_E_INVALID, "allreduce_f64: 1..16 values, op 0 (sum) or 1 (max)");
    if (!r->comm) return fail(r, CL2_E_STATE, r->comm_poisoned ? "the communicator was aborted after a failed collective" : "no communicator (call cl2_comm_init_rank first)");
    std::string why;
    RcclApi* api = rccl_api(why);
    if (!api) return fail(r, CL2_E_COMM, why);
    COMM_HIP_TRY(r, api, hipSetDevice(r->device));
    {
        const int rc = drain(r);
        if (rc != CL2_OK) { r->comm_poisoned = true; comm_abort(r, api); return rc; }
    }
    COMM_HIP_TRY(r, api, hipMemcpyAsync(r->d_comm_scratch, values, (size_t)n * sizeof(double), hipMemcpyHostToDevice, r->stream));
    COMM_RCCL_TRY(r, api, api->AllReduce(r->d_comm_scratch, r->d_comm_scratch, (size_t)n, ncclDouble, op == 0 ? ncclSum : ncclMax, r->comm, r->stream));
    TRY(comm_wait(r, api, "cl2_comm_allreduce_f64"));
    HIP_TRY(r, hipMemcpy(values, r->d_comm_scratch, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return CL2_OK;
}

/* What the COMMUNICATOR says about itself (not what the launcher's environment says): ncclCommCount, ncclCommUserRank,
 * ncclCommCuDevice, and the PCI address of this rank's GPU as one integer, domain << 16 | bus << 8 | device << 3 | function
 * (hipDeviceGetPCIBusId).  A job line that lists nranks distinct addresses shows that RCCL saw that many GPUs. */
int cl2_comm_info(cl2_renderer* r, cl2_comm_info_t* out) {
    if (!r || !out) return CL2_E_INVALID;
    std::memset(out, 0, sizeof *out);
    out->device_ordinal = r->device;
    HIP_TRY(r, hipSetDevice(r->device));
    char bus[32] = {0};
    HIP_TRY(r, hipDeviceGetPCIBusId(bus, (int)sizeof bus, r->device));
    unsigned dom = 0, b = 0, dev = 0, fn = 0;
    if (std::sscanf(bus, "%x:%x:%x.%x", &dom, &b, &dev, &fn) >= 3)
        out->pci_address = ((int64_t)dom << 16) | ((int64_t)b << 8) | ((int64_t)dev << 3) | (int64_t)fn;
    std::snprintf(out->pci_bus_id, sizeof out->pci_bus_id, "%s", bus);
    if (!r->comm) return CL2_OK;                       // nranks = 0: no communicator
    std::string why;
    RcclApi* api = rccl_api(why);
    if (!api) return fail(r, CL2_E_COMM, why);
    int n = 0, rank = -1, cudev = -1;
    RCCL_TRY(r, api, api->CommCount(r->comm, &n));
    RCCL_TRY(r, api, api->CommUserRank(r->comm, &rank));
    RCCL_TRY(r, api, api->CommCuDevice(r->comm, &cudev));
    out->nranks = n; out->rank = rank; out->comm_device = cudev;
    return CL2_OK;
}

/* The host's way of saying "this rank failed, do not wait for anybody": the communicator is torn down with
 * ncclCommAbort at once, so peers blocked in a collective with this rank see an error or their own deadline
 * instead of waiting for a rank that is about to exit.  Harmless without a communicator. */
int cl2_comm_abort(cl2_renderer* r) {
    if (!r) return CL2_E_INVALID;
    if (!r->comm) return CL2_OK;
    std::string why;
    RcclApi* api = rccl_api(why);
    (void)hipSetDevice(r->device);
    r->comm_poisoned = true;
    comm_abort(r, api);
    return CL2_OK;
}

int cl2_comm_destroy(cl2_renderer* r) {
    if (!r) return CL2_E_INVALID;
    if (!r->comm) return CL2_OK;
    std::string why;
    RcclApi* api = rccl_api(why);
    if (!api) return fail(r, CL2_E_COMM, why);
    (void)hipSetDevice(r->device);
    // a handle whose own streams are in an error state, or whose last collective failed, must not wait in
    // ncclCommDestroy for work that will never finish
    if (r->comm_poisoned || drain(r) != CL2_OK) { comm_abort(r, api); return CL2_OK; }
    ncclComm_t comm = r->comm;
    r->comm = nullptr; r->comm_nranks = 0; r->comm_rank = 0;
    RCCL_TRY(r, api, api->CommDestroy(comm));
    return CL2_OK;
}

int cl2_set_profiling(cl2_renderer* r, int level) {
    if (!r) return CL2_E_INVALID;
    r->profiling = level < 0 ? 0 : (level > 2 ? 2 : level);
    return CL2_OK;
}
int cl2_set_levels_per_launch(cl2_renderer* r, int levels) {
    if (!r) return CL2_E_INVALID;
    if (levels < 0 || levels > MAX_VERTS) return fail(r, CL2_E_INVALID, "levels_per_launch must be 0 (by survival) or 1..6");
    r->levels_per_launch = levels;
    return CL2_OK;
}
int cl2_selftest_exact_math(cl2_renderer* r, uint64_t* rcp_mismatches, uint64_t* divpi_mismatches) {
    if (!r || !rcp_mismatches || !divpi_mismatches) return CL2_E_INVALID;
    HIP_TRY(r, hipSetDevice(r->device));
    unsigned long long* d = nullptr;
    TRY(dev_alloc(r, &d, (size_t)2));
    int rc = CL2_OK;
    if (hipMemset(d, 0, 16) != hipSuccess) rc = fail(r, CL2_E_HIP, "selftest memset failed");
    if (rc == CL2_OK) {
        hipLaunchKernelGGL(k_selftest_exact_math, dim3(4096), dim3(BLOCK), 0, r->stream, d);
        rc = drain(r);
    }
    unsigned long long h[2] = {0, 0};
    if (rc == CL2_OK && hipMemcpy(h, d, 16, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(r, CL2_E_HIP, "selftest copy failed");
    dev_free(r, d);
    *rcp_mismatches = h[0]; *divpi_mismatches = h[1];
    return rc;
}
int cl2_probe_math(cl2_renderer* r, int which, const float* in, size_t n, float* out) {
    if (!r || !in || !out || which < 0 || which > 7) return CL2_E_INVALID;
    if (n == 0) return CL2_OK;
    HIP_TRY(r, hipSetDevice(r->device));
    float *d_in = nullptr, *d_out = nullptr;
    int rc = dev_alloc(r, &d_in, n);
    if (rc == CL2_OK) rc = dev_alloc(r, &d_out, n);
    if (rc == CL2_OK && hipMemcpy(d_in, in, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = fail(r, CL2_E_HIP, "probe upload failed");
    if (rc == CL2_OK) {
        hipLaunchKernelGGL(k_probe_math, dim3(2048), dim3(BLOCK), 0, r->stream, which, n, d_in, d_out);
        rc = drain(r);
    }
    if (rc == CL2_OK && hipMemcpy(out, d_out, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(r, CL2_E_HIP, "probe download failed");
    dev_free(r, d_in); dev_free(r, d_out);
    return rc;
}
int cl2_probe_bounce(cl2_renderer* r, int from_camera, const float* in, size_t n, float* out) {
    if (!r || !in || !out) return CL2_E_INVALID;
    if (n == 0) return CL2_OK;
    HIP_TRY(r, hipSetDevice(r->device));
    float *d_in = nullptr, *d_out = nullptr;
    int rc = dev_alloc(r, &d_in, 12 * n);
    if (rc == CL2_OK) rc = dev_alloc(r, &d_out, 8 * n);
    if (rc == CL2_OK && hipMemcpy(d_in, in, 12 * n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = fail(r, CL2_E_HIP, "probe upload failed");
    if (rc == CL2_OK) {
        hipLaunchKernelGGL(k_probe_bounce, dim3(1024), dim3(BLOCK), 0, r->stream, n, from_camera, d_in, d_out);
        rc = drain(r);
    }
    if (rc == CL2_OK && hipMemcpy(out, d_out, 8 * n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(r, CL2_E_HIP, "probe download failed");
    dev_free(r, d_in); dev_free(r, d_out);
    return rc;
}
int cl2_set_traversal_mode(cl2_renderer* r, int mode) {
    if (!r) return CL2_E_INVALID;
    if (mode < 0 || mode > 5) return fail(r, CL2_E_INVALID, "traversal mode must be 0 (auto), 1 (fused), 2 (persistent, per level), 3 (fused subpaths, persistent connection rays), 4 (persistent whole subpaths) or 5 (persistent, exact 4-wide walk)");
    r->traversal_mode = mode;
    r->paths_share = 0;
    return CL2_OK;
}
int cl2_query_organisation(cl2_renderer* r, cl2_organisation* out) {
    if (!r || !out) return CL2_E_INVALID;
    if (!r->scene_ok) return fail(r, CL2_E_STATE, "no scene uploaded (call cl2_upload_scene first)");
    std::memset(out, 0, sizeof *out);
    out->tree_in_lds = tree_in_lds(r) ? 1 : 0;
    out->persistent_subpaths = split_paths(r) ? 1 : 0;
    out->persistent_connections = split_conn(r) ? 1 : 0;
    out->two_tris_per_step = two_tris_per_step(r) ? 1 : 0;
    out->n_records = r->bvh.n_nodes;
    out->n_lds_records = r->bvh.n_lds_nodes;
    out->n_top_renumbered = r->n_top;
    out->lds_triangles = r->bvh.lds_tris;
    out->levels_per_launch = split_paths(r) ? 1 : effective_levels(r);
    out->paths_share = r->paths_share;
    out->pipeline_stages = pipeline_stages(r);
    out->wide_nodes = r->n_wide;
    out->pruned_records = r->bvh.n_fast_nodes;
    out->wide_connections = (wide_walk(r) && split_conn(r)) ? 1 : 0;
    out->tree_bytes = (int64_t)r->bvh.n_nodes * 32 + (int64_t)r->bvh.n_tris * 48;
    out->sample_streams = r->streams;
    out->staged_bytes = (int32_t)bvh_lds_bytes(r);
    return CL2_OK;
}
/* Child order of the 4-wide walks (round 6).  0 (default) = the reference's fixed order (trace.metal:157-160): bit-exact.  1 = the
 * passing children of a node nearest first: fewer node visits and triangle tests per ray, NOT bit-exact by construction (exact-t ties
 * between two triangles, hits a few ulp in front of their leaf box; csrc/bvh_wide.hpp ORDER).  Opt-in; applies to scenes whose tree is
 * read through the caches (an LDS-resident tree such as the Cornell box has no 4-wide walk and renders the same either way); whole-
 * subpath launches give way to per-level ones, and the reference-walk tallies (cl2_set_counting(1)) stay the binary walk's. */
int cl2_set_traversal_order(cl2_renderer* r, int order) {
    if (!r) return CL2_E_INVALID;
    if (order != 0 && order != 1) return fail(r, CL2_E_INVALID, "traversal order must be 0 (reference order, exact) or 1 (nearest child first)");
    if (order == 1 && r->connection_query == 1) return fail(r, CL2_E_INVALID, "the seeded connection query keeps the reference's child order: cl2_set_connection_query(0) first");
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    if (r->n_wide > 0) {
        // the overflow array of the wide walk's stack is sized for the order (ensure_wide_overflow reallocates at the next launch)
        const int entries = wide_overflow_entries(r->max_pending, r->order_depth, order);
        if (entries < 0)
            return fail(r, CL2_E_INVALID, "tree too deep for the nearest-first child order: its 4-wide stack can reach " + std::to_string(r->order_depth) +
                                          " entries, the limit is " + std::to_string(WIDE_STACK_LDS + WIDE_STACK_OVERFLOW));
        if (entries != r->wide_ovf_entries) { dev_free(r, r->d_wide_ovf); r->wide_ovf_entries = entries; }
    }
    r->traversal_order = order;
    return CL2_OK;
}
int cl2_get_traversal_order(const cl2_renderer* r) { return r ? r->traversal_order : CL2_E_INVALID; }
/* Stack entries a lane of the 4-wide walk has for the uploaded scene in the current child order: those in LDS plus those of the
 * global overflow array.  0: no scene, or a scene without a 4-wide collapse. */
int cl2_wide_stack_capacity(const cl2_renderer* r) {
    if (!r) return CL2_E_INVALID;
    return (r->scene_ok && r->n_wide > 0) ? WIDE_STACK_LDS + std::max(r->wide_ovf_entries, 1) : 0;
}
/* What a connection ray asks of the tree.  0 (default) = its closest hit, as the reference.  1 = for a t >= 2 pair, whether the camera
 * vertex's triangle is what the ray sees: the walk starts from the target's distance and stops at the first blocker (csrc/bvh_wide.hpp
 * VIS).  Opt-in and NOT the parity path: the verdict is the reference's except where a hit lies in front of its own leaf box.  Applies
 * where connection rays take the 4-wide walk (cl2_connection_query_active). */
int cl2_set_connection_query(cl2_renderer* r, int mode) {
    if (!r) return CL2_E_INVALID;
    if (mode != 0 && mode != 1) return fail(r, CL2_E_INVALID, "connection query must be 0 (closest hit, exact) or 1 (seeded visibility walk)");
    if (mode == 1 && r->traversal_order != 0) return fail(r, CL2_E_INVALID, "the seeded connection query keeps the reference's child order: cl2_set_traversal_order(0) first");
    if (mode == 1 && (r->debug_flags & (3 << 13))) return fail(r, CL2_E_INVALID, "the seeded connection query has no form without the speculative expansion or the packed triangle records: clear debug bits 13 and 14 first");
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    r->connection_query = mode;
    return CL2_OK;
}
int cl2_get_connection_query(const cl2_renderer* r) { return r ? r->connection_query : CL2_E_INVALID; }
int cl2_connection_query_active(const cl2_renderer* r) {
    if (!r) return CL2_E_INVALID;
    return (r->scene_ok && conn_vis(r)) ? 1 : 0;
}
int cl2_set_debug_flags(cl2_renderer* r, int flags) {
    if (!r) return CL2_E_INVALID;
#ifndef CL2_TEST_VARIANT
    // bits 0-2 switch parts of the resolve stage OFF (timing dissection: the render is invalid); they exist only in
    // the test variant of the library and cannot be reached from the shipped one
    if (flags & 7) return fail(r, CL2_E_INVALID, "debug bits 0-2 (skip parts of the resolve stage: invalid renders) exist only in the test variant of the library");
#endif
    if (flags & ~CL2_DEBUG_KNOWN_BITS) return fail(r, CL2_E_INVALID, "unknown debug flag bits (see include/clive2_amd.h)");
    if (((flags >> 4) & 7) != 0 && ((flags >> 4) & 7) != 7) return fail(r, CL2_E_INVALID, "debug bits 4-6 must be 0 or 7");
    if ((flags & (3 << 13)) && r->connection_query == 1)
        return fail(r, CL2_E_INVALID, "debug bits 13 and 14 are A/B switches of the closest-hit walk; the seeded connection query has no such form: cl2_set_connection_query(0) first");
    if (((flags >> 4) & 7) == 7 && r->strategy_mask != CL2_STRATEGY_ALL)
        return fail(r, CL2_E_INVALID, "the cross-check resolve kernel (debug bits 4-6 = 7) has no masked form: set the full strategy mask first");
    if (((flags >> 4) & 7) == 7 && r->n_layers > 0)
        return fail(r, CL2_E_INVALID, "the cross-check resolve kernel (debug bits 4-6 = 7) has no layered form: cl2_set_layers(NULL, 0) first");
    r->debug_flags = flags;
    r->bvh.n_fast_nodes = ((flags >> 7) & 1) ? 0 : r->n_fast;      // bit 7: walk the full table (A/B of the pruned one)
    r->bvh.fast_flat = flat_walk(r);     // bit 11: per-lane walk of a flat pruned table (A/B of the wave-uniform one); bit 26: its clamped loop
    return CL2_OK;
}
/* Reproducible light image (off by default): the t = 1 contributions are written as records, sorted by (target pixel, s, source
 * pixel) and summed per target in that order (det_splat.hpp) instead of being added with float atomics in whatever order the
 * hardware serves them.  Two renders of the same scene and seeds then give the same bytes in all four accumulators -- as the
 * reference's sort + bincount + gather chain does (src/renderer.py:97-111, :213-250).  Costs a radix sort of 6 x W x H keys per
 * pass and 32 bytes of record space per slot. */
int cl2_set_reproducible(cl2_renderer* r, int on) {
    if (!r) return CL2_E_INVALID;
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    r->reproducible = on != 0;
    return CL2_OK;
}
int cl2_get_reproducible(const cl2_renderer* r) { return r ? (r->reproducible ? 1 : 0) : CL2_E_INVALID; }
/* Strategy mask (include/clive2_amd.h): bit (t - 1) * 7 + s keeps the colour of pair (s, t); every w is kept whatever the mask.  Only
 * launch_resolve reads it: a full mask launches the default kernels, a partial one the STRAT instantiations. */
int cl2_set_strategy_mask(cl2_renderer* r, uint64_t mask) {
    if (!r) return CL2_E_INVALID;
    mask &= CL2_STRATEGY_ALL;
    if (mask != CL2_STRATEGY_ALL && ((r->debug_flags >> 4) & 7) == 7)
        return fail(r, CL2_E_INVALID, "the cross-check resolve kernel (debug bits 4-6 = 7) has no masked form: clear debug bits 4-6 first");
    if (mask != CL2_STRATEGY_ALL && r->n_layers > 0)
        return fail(r, CL2_E_STATE, "a partial strategy mask and layer accumulators exclude each other (the layers are the masked renders): cl2_set_layers(NULL, 0) first");
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    r->strategy_mask = mask;
    return CL2_OK;
}
int cl2_get_strategy_mask(const cl2_renderer* r, uint64_t* mask_out) {
    if (!r || !mask_out) return CL2_E_INVALID;
    *mask_out = r->strategy_mask;
    return CL2_OK;
}

/* Layer accumulators (include/clive2_amd.h, layers.hpp).  The table is what launch_resolve, launch_accumulate and
 * launch_finalize_accumulate read; lay_valid follows the rules of mom_valid. */
namespace {
void free_layers(cl2_renderer* r) {
    dev_free(r, r->d_lay_agg); dev_free(r, r->d_lay_light); dev_free(r, r->d_lacc);
    dev_free(r, r->d_ldn[0]); dev_free(r, r->d_ldn[1]);
    r->n_layers = 0;
    r->lcodes = LayerCodes{};
    r->lay_valid = false;
}
int need_layers(cl2_renderer* r, size_t n_floats) {
    if (r->n_layers == 0) return fail(r, CL2_E_STATE, "no layer table is set (cl2_set_layers)");
    if (n_floats != 3 * (size_t)r->n_layers * (size_t)r->FB) return fail(r, CL2_E_INVALID, "packed layer accumulators hold n_layers*3*W*H floats");
    return CL2_OK;
}
// what reading lacc needs beyond a table (cl2_read_layers_packed, cl2_denoise_layers)
int need_valid_layers(cl2_renderer* r) {
    if (!r->lay_valid)
        return fail(r, CL2_E_STATE, "the layer accumulators do not cover every sample in the accumulators (the table was set or changed after "
                                    "samples, or accumulators were written without them): cl2_reset_accumulators or cl2_write_layers_packed");
    return CL2_OK;
}
}  // namespace
int cl2_set_layers(cl2_renderer* r, const uint64_t* masks, int n_layers) {
    static_assert(CL2_MAX_LAYERS == LAYERS_MAX, "CL2_MAX_LAYERS");
    if (!r) return CL2_E_INVALID;
    if (n_layers < 0) return fail(r, CL2_E_INVALID, "layers: n_layers must be >= 0");
    if (n_layers > CL2_MAX_LAYERS) return fail(r, CL2_E_INVALID, "layers: at most CL2_MAX_LAYERS (8) layers; merge layers or render the rest in a second pass over the same seeds");
    if (n_layers > 0 && !masks) return fail(r, CL2_E_INVALID, "layers: NULL masks with n_layers > 0");
    if (!masks) n_layers = 0;
    uint64_t m[CL2_MAX_LAYERS] = {};
    uint64_t seen = 0;
    for (int l = 0; l < n_layers; l++) {
        m[l] = masks[l] & CL2_STRATEGY_ALL;
        if (m[l] & seen) return fail(r, CL2_E_INVALID, "layers: the masks must be pairwise disjoint (a pair adds to at most one layer)");
        seen |= m[l];
    }
    if (n_layers > 0) {
        if (r->strategy_mask != CL2_STRATEGY_ALL)
            return fail(r, CL2_E_STATE, "layer accumulators and a partial strategy mask exclude each other: cl2_set_strategy_mask(CL2_STRATEGY_ALL) first");
        if (r->density || r->adaptive)
            return fail(r, CL2_E_STATE, "layer accumulators have no form for a sample density: cl2_set_sample_density(NULL) and cl2_set_adaptive_sampling(0) first");
        if (((r->debug_flags >> 4) & 7) == 7)
            return fail(r, CL2_E_INVALID, "the cross-check resolve kernel (debug bits 4-6 = 7) has no layered form: clear debug bits 4-6 first");
    }
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    if (n_layers == r->n_layers && std::equal(m, m + n_layers, r->layer_masks)) return CL2_OK;      // the table it has
    free_layers(r);
    if (n_layers == 0) return CL2_OK;
    LayerCodes lc{};
    for (int l = 0; l < n_layers; l++)
        for (int t = 1; t <= 6; t++)
            for (int s = 0; s <= 6; s++)
                if (m[l] & CL2_STRATEGY_BIT(s, t)) lc.w[(t - 1) >> 1] |= (unsigned long long)(l + 1) << (((t - 1) & 1) * 32 + 4 * s);
    lc.n_layers = n_layers;
    r->n_layers = n_layers;
    int rc = alloc_layer_entries(r);
    if (rc == CL2_OK) rc = side_sum_on(r, r->d_lacc, 3 * (size_t)n_layers * (size_t)r->FB, r->lay_valid, "layer accumulators");
    if (rc != CL2_OK) { const std::string why = r->err; free_layers(r); return fail(r, rc, why + " (layers are off)"); }
    std::copy(m, m + CL2_MAX_LAYERS, r->layer_masks);
    r->lcodes = lc;
    return CL2_OK;
}
int cl2_get_layers(const cl2_renderer* r, uint64_t* masks_out, int capacity) {
    if (!r || capacity < 0 || (capacity > 0 && !masks_out)) return CL2_E_INVALID;
    for (int l = 0; l < r->n_layers && l < capacity; l++) masks_out[l] = r->layer_masks[l];
    return r->n_layers;
}
int cl2_read_layers_packed(cl2_renderer* r, float* dst, size_t n_floats) {
    if (!r || !dst) return CL2_E_INVALID;
    TRY(need_layers(r, n_floats));
    TRY(need_valid_layers(r));
    return packed_copy(r, dst, r->d_lacc, n_floats, hipMemcpyDeviceToHost);
}
int cl2_write_layers_packed(cl2_renderer* r, const float* src, size_t n_floats) {
    if (!r || !src) return CL2_E_INVALID;
    TRY(need_layers(r, n_floats));
    TRY(packed_copy(r, r->d_lacc, src, n_floats, hipMemcpyHostToDevice));
    r->lay_valid = true;
    return CL2_OK;
}

int cl2_set_subpath_gather(cl2_renderer* r, int lanes, int wait_steps) {
    if (!r) return CL2_E_INVALID;
    if (lanes < 0 || lanes > 64 || wait_steps < 0 || wait_steps > 1000) return fail(r, CL2_E_INVALID, "subpath gather: 0..64 lanes (0 = default 32), 0..1000 steps (0 = default 48)");
    r->gather_lanes = lanes ? lanes : 32;
    r->gather_wait = wait_steps ? wait_steps : 48;
    return CL2_OK;
}
#ifdef CL2_WALK_HISTO
/* instrumentation build only: read (and clear) the pass statistics of the wide walk, 6 x 65 counters */
int cl2_walk_histo(cl2_renderer* r, unsigned long long* out) {
    if (!r || !out) return CL2_E_INVALID;
    TRY(drain(r));
    HIP_TRY(r, hipMemcpyFromSymbol(out, HIP_SYMBOL(g_walk_histo), sizeof(unsigned long long) * 6 * 65));
    std::vector<unsigned long long> z(6 * 65, 0ull);
    HIP_TRY(r, hipMemcpyToSymbol(HIP_SYMBOL(g_walk_histo), z.data(), sizeof(unsigned long long) * 6 * 65));
    return CL2_OK;
}
#endif
int cl2_set_counting(cl2_renderer* r, int mode) {
    if (!r) return CL2_E_INVALID;
    if (mode < 0 || mode > 2) return fail(r, CL2_E_INVALID, "counting: 0 off, 1 the reference walk's tallies (binary walk), 2 the 4-wide walk's own tallies");
    r->counting = mode;
    return CL2_OK;
}

/* cl2_set_counting(2): what the 4-wide walk itself fetched since the last cl2_reset_counters -- rays, wide nodes visited, distinct
 * triangle records read, stack entries spilled to the global overflow array, binary records visited by rays with a non-finite
 * 1/d -- separately for the subpath launches and the connection launch.  Zero where the scene does not take the wide walk. */
int cl2_read_walk_tallies(cl2_renderer* r, cl2_walk_tallies* out) {
    if (!r || !out) return CL2_E_INVALID;
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    Stats s;
    HIP_TRY(r, hipMemcpy(&s, r->d_stats, sizeof s, hipMemcpyDeviceToHost));
    static_assert(sizeof(out->subpath) == sizeof(s.walk[0]) && sizeof(out->connection) == sizeof(s.walk[1]), "tally layout");
    std::memcpy(&out->subpath, s.walk[0], sizeof s.walk[0]);
    std::memcpy(&out->connection, s.walk[1], sizeof s.walk[1]);
    return CL2_OK;
}

int cl2_read_counters(cl2_renderer* r, cl2_counters* out) {
    if (!r || !out) return CL2_E_INVALID;
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    Stats s;
    HIP_TRY(r, hipMemcpy(&s, r->d_stats, sizeof s, hipMemcpyDeviceToHost));
    {   // per-workgroup slots of the subpath kernel
        std::vector<unsigned long long> slots((size_t)grid_for(r->B) * 4);
        HIP_TRY(r, hipMemcpy(slots.data(), r->d_block_stats, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < slots.size(); b += 4) {
            s.rays += slots[b]; s.box_tests += slots[b + 1]; s.tri_tests += slots[b + 2]; s.counted_rays += slots[b + 3];
        }
    }
    std::memset(out, 0, sizeof *out);
    out->rays = s.rays; out->conn_rays = s.conn_rays; out->box_tests = s.box_tests; out->tri_tests = s.tri_tests;
    out->counted_rays = s.counted_rays;
    out->samples = r->samples;
    out->ms_generate = r->ms[ST_GENERATE]; out->ms_traverse_paths = r->ms[ST_TRAVERSE_PATHS]; out->ms_bounce = r->ms[ST_BOUNCE];
    out->ms_connect_setup = r->ms[ST_CONNECT_SETUP]; out->ms_traverse_conn = r->ms[ST_TRAVERSE_CONN];
    out->ms_connect_resolve = r->ms[ST_CONNECT_RESOLVE]; out->ms_finalize = r->ms[ST_FINALIZE]; out->ms_accumulate = r->ms[ST_ACCUMULATE];
    out->launches_traverse_paths = r->launches_tp; out->launches_traverse_conn = r->launches_tc;
    out->rays_traverse_paths = s.rays - s.conn_rays; out->rays_traverse_conn = s.conn_rays;
    return CL2_OK;
}

int cl2_reset_counters(cl2_renderer* r) {
    if (!r) return CL2_E_INVALID;
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    HIP_TRY(r, hipMemset(r->d_stats, 0, sizeof(Stats)));
    HIP_TRY(r, hipMemset(r->d_block_stats, 0, (size_t)grid_for(r->B) * 4 * sizeof(unsigned long long)));
    for (double& m : r->ms) m = 0.0;
    r->launches_tp = r->launches_tc = 0;
    return CL2_OK;
}

int cl2_export_rays(cl2_renderer* r, int which, void* out, size_t n_records) {
    STAGE_PROLOGUE(r);
    if (!out || (which != CL2_LIGHT && which != CL2_CAMERA) || n_records != (size_t)r->FB) return fail(r, CL2_E_INVALID, "bad export_rays arguments");
    Scratch<RayRec> d(r);
    TRY(d.alloc((size_t)r->FB));
    hipLaunchKernelGGL(k_export_rays, dim3(grid_for(r->FB)), dim3(BLOCK), 0, r->stream, r->FB, r->export_stream * r->FB, r->sets[r->cur][which], which == CL2_CAMERA ? 1 : 0, d.p);
    TRY(drain(r));
    HIP_TRY(r, hipMemcpy(out, d, (size_t)r->FB * sizeof(RayRec), hipMemcpyDeviceToHost));
    return CL2_OK;
}

int cl2_export_paths(cl2_renderer* r, int which, void* out, size_t n_records) {
    STAGE_PROLOGUE(r);
    if (!out || (which != CL2_LIGHT && which != CL2_CAMERA) || n_records != (size_t)r->FB) return fail(r, CL2_E_INVALID, "bad export_paths arguments");
    Scratch<unsigned char> d(r);
    TRY(d.alloc((size_t)r->FB * 1040));
    hipLaunchKernelGGL(k_export_paths, dim3(grid_for(r->FB)), dim3(BLOCK), 0, r->stream, r->FB, r->export_stream * r->FB, r->B, r->sets[r->cur][which], which == CL2_CAMERA ? 1 : 0, d.p);
    TRY(drain(r));
    HIP_TRY(r, hipMemcpy(out, d, (size_t)r->FB * 1040, hipMemcpyDeviceToHost));
    return CL2_OK;
}

int cl2_export_aggregators(cl2_renderer* r, void* out, size_t n_records) {
    STAGE_PROLOGUE(r);
    if (!out || n_records != (size_t)r->FB) return fail(r, CL2_E_INVALID, "bad export_aggregators arguments");
    Scratch<float> d(r);
    TRY(d.alloc((size_t)r->FB * 32));
    hipLaunchKernelGGL(k_export_aggregators, dim3(grid_for(r->FB)), dim3(BLOCK), 0, r->stream, r->FB, r->export_stream * r->FB, r->B, r->d_agg, d.p);
    TRY(drain(r));
    HIP_TRY(r, hipMemcpy(out, d, (size_t)r->FB * 128, hipMemcpyDeviceToHost));
    return CL2_OK;
}

int cl2_export_connections(cl2_renderer* r, uint64_t* cmask, int32_t* tri, float* t1, size_t n_pixels) {
    STAGE_PROLOGUE(r);
    if (n_pixels != (size_t)r->B) return fail(r, CL2_E_INVALID, "n_pixels must equal the batch size");
    TRY(drain(r));
    const size_t B = r->B;
    if (cmask) HIP_TRY(r, hipMemcpy(cmask, r->d_cmask[0], B * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (tri) HIP_TRY(r, hipMemcpy(tri, r->d_chit[0], (size_t)CONN_SLOTS * B * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (t1) HIP_TRY(r, hipMemcpy(t1, reinterpret_cast<const float*>(r->d_chit[0]) + (size_t)CONN_SLOTS * B,
                                 (size_t)MAX_VERTS * B * sizeof(float), hipMemcpyDeviceToHost));
    return CL2_OK;
}

int cl2_export_sample_images(cl2_renderer* r, float* fin4, float* light4, float* sw, float* uni4, size_t n_pixels) {
    STAGE_PROLOGUE(r);
    if (n_pixels != (size_t)r->FB) return fail(r, CL2_E_INVALID, "n_pixels must equal W*H");
    TRY(drain(r));
    const size_t B = r->FB, off = (size_t)r->export_stream * r->FB;
    if (fin4) HIP_TRY(r, hipMemcpy(fin4, r->d_finalized + off, B * sizeof(float4), hipMemcpyDeviceToHost));
    if (light4) HIP_TRY(r, hipMemcpy(light4, r->d_light_image + off, B * sizeof(float4), hipMemcpyDeviceToHost));
    if (sw) HIP_TRY(r, hipMemcpy(sw, r->d_sample_w + off, B * sizeof(float), hipMemcpyDeviceToHost));
    if (uni4) HIP_TRY(r, hipMemcpy(uni4, r->d_uni + off, B * sizeof(float4), hipMemcpyDeviceToHost));
    return CL2_OK;
}

int cl2_import_sample_images(cl2_renderer* r, const float* fin4, const float* light4, const float* sw, const float* uni4, size_t n_pixels) {
    STAGE_PROLOGUE(r);
    if (n_pixels != (size_t)r->FB) return fail(r, CL2_E_INVALID, "n_pixels must equal W*H");
    TRY(drain(r));
    const size_t B = r->FB, off = (size_t)r->export_stream * r->FB;
    if (fin4) HIP_TRY(r, hipMemcpy(r->d_finalized + off, fin4, B * sizeof(float4), hipMemcpyHostToDevice));
    if (light4) HIP_TRY(r, hipMemcpy(r->d_light_image + off, light4, B * sizeof(float4), hipMemcpyHostToDevice));
    if (sw) HIP_TRY(r, hipMemcpy(r->d_sample_w + off, sw, B * sizeof(float), hipMemcpyHostToDevice));
    if (uni4) HIP_TRY(r, hipMemcpy(r->d_uni + off, uni4, B * sizeof(float4), hipMemcpyHostToDevice));
    return CL2_OK;
}

namespace {
// the device side of a probe call: origins, directions, hit records, seeded targets (cl2_probe_visibility only), the ray count
struct ProbeRays {
    Scratch<float4> o, d, h;
    Scratch<int> t;
    Scratch<unsigned> n;
    explicit ProbeRays(cl2_renderer* r) : o(r), d(r), h(r), t(r), n(r) {}
};

// The front of both probe calls after their own checks: the ray count's bound, `target` (if any) checked against the scene, the
// RayRec array as float4 origins and directions on the device, the count beside them; `wide`: the walk's work counter starts at 0.
int probe_upload(cl2_renderer* r, const void* rays_v, size_t n_rays, const int32_t* target, bool wide, ProbeRays& p) {
    if (n_rays > (size_t)1 << 30) return fail(r, CL2_E_INVALID, "too many probe rays");
    for (size_t i = 0; target && i < n_rays; i++)
        if (target[i] >= r->bvh.n_tris) return fail(r, CL2_E_INVALID, "probe target is not a triangle of the scene");
    const RayRec* rays = static_cast<const RayRec*>(rays_v);
    std::vector<float4> o(n_rays), d(n_rays);
    for (size_t i = 0; i < n_rays; i++) {
        o[i] = make_float4(rays[i].origin[0], rays[i].origin[1], rays[i].origin[2], 0.0f);
        d[i] = make_float4(rays[i].direction[0], rays[i].direction[1], rays[i].direction[2], 0.0f);
    }
    TRY(p.o.alloc(n_rays));
    TRY(p.d.alloc(n_rays));
    TRY(p.h.alloc(n_rays));
    if (target) TRY(p.t.alloc(n_rays));
    TRY(p.n.alloc(1));
    const unsigned n = (unsigned)n_rays;
    HIP_TRY(r, hipMemcpy(p.o, o.data(), n_rays * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(r, hipMemcpy(p.d, d.data(), n_rays * sizeof(float4), hipMemcpyHostToDevice));
    if (target) HIP_TRY(r, hipMemcpy(p.t, target, n_rays * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(r, hipMemcpy(p.n, &n, sizeof n, hipMemcpyHostToDevice));
    if (wide) HIP_TRY(r, hipMemsetAsync(r->d_work, 0, WORK_STRIDE * sizeof(unsigned), r->stream));
    return CL2_OK;
}

// ... and their end: the hit records of the finished launch, on the host
int probe_read_back(cl2_renderer* r, const ProbeRays& p, size_t n_rays, std::vector<float4>& h) {
    TRY(drain(r));
    h.resize(n_rays);
    HIP_TRY(r, hipMemcpy(h.data(), p.h, n_rays * sizeof(float4), hipMemcpyDeviceToHost));
    return CL2_OK;
}
}  // namespace

int cl2_probe_traverse(cl2_renderer* r, const void* rays_v, size_t n_rays, int32_t* best_i, float* best_t, float* u, float* v) {
    STAGE_PROLOGUE(r);
    if (!rays_v || !best_i || !best_t || !u || !v) return fail(r, CL2_E_INVALID, "NULL probe array");
    if (n_rays == 0) return CL2_OK;
    // the probe through the exact 4-wide walk (rays with a non-finite 1/d take the binary walk inside it)
    const bool wide = r->traversal_mode == 5 && r->n_wide > 0 && !count_ref(r);
    ProbeRays p(r);
    TRY(probe_upload(r, rays_v, n_rays, nullptr, wide, p));
    if (wide) {
        PathRaySource src{nullptr, p.o, p.d, p.h};
        TRY(launch_wide(r, r->stream, 0, p.n, r->d_work, src, 0));
    } else {
        with_flags([&](auto CNT) {
            hipLaunchKernelGGL(k_traverse_paths<CNT.value>, dim3(grid_for(n_rays)), dim3(BLOCK), bvh_lds_bytes(r), r->stream, r->bvh,
                               (const int*)nullptr, p.n.p, p.o.p, p.d.p, p.h.p, r->d_stats);
        }, count_ref(r));
    }
    std::vector<float4> h;
    TRY(probe_read_back(r, p, n_rays, h));
    for (size_t i = 0; i < n_rays; i++) {
        std::memcpy(&best_i[i], &h[i].x, 4);
        best_t[i] = h[i].y; u[i] = h[i].z; v[i] = h[i].w;
    }
    return CL2_OK;
}

int cl2_probe_visibility(cl2_renderer* r, const void* rays_v, size_t n_rays, const int32_t* target, int32_t* out_tri, float* out_t) {
    STAGE_PROLOGUE(r);
    if (!rays_v || !target || !out_tri || !out_t) return fail(r, CL2_E_INVALID, "NULL probe array");
    if (r->n_wide <= 0) return fail(r, CL2_E_STATE, "the uploaded scene has no 4-wide collapse: no seeded walk");
    if ((r->debug_flags >> 13) & 1) return fail(r, CL2_E_STATE, "the seeded walk exists for the speculative walk only: clear debug bit 13");
    if (n_rays == 0) return CL2_OK;
    ProbeRays p(r);
    TRY(probe_upload(r, rays_v, n_rays, target, true, p));
    ProbeVisRaySource src{p.o, p.d, p.t, p.h};
    TRY((launch_wide<ProbeVisRaySource, true>(r, r->stream, 0, p.n, r->d_work, src, 0)));
    std::vector<float4> h;
    TRY(probe_read_back(r, p, n_rays, h));
    for (size_t i = 0; i < n_rays; i++) {
        std::memcpy(&out_tri[i], &h[i].x, 4);
        out_t[i] = h[i].y;
    }
    return CL2_OK;
}

// ---- first-hit features and the denoiser (denoise.hpp) ----
namespace {
// the feature set (cl2_render_features, cl2_write_features), allocated by the first call of either
int need_feature_buffers(cl2_renderer* r) {
    if (r->d_g0) return CL2_OK;
    const size_t FB = (size_t)r->FB;
    int rc = dev_alloc(r, &r->d_feat_seeds, FB);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_feat_o, FB);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_feat_d, FB);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_feat_hit, FB);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_feat_count, (size_t)1);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_feat_work, (size_t)WORK_STRIDE);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_feat_stats, (size_t)1);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_g1, FB);
    if (rc != CL2_OK) return rc;
    const unsigned n = (unsigned)FB;
    HIP_TRY(r, hipMemcpy(r->d_feat_count, &n, sizeof n, hipMemcpyHostToDevice));
    return dev_alloc(r, &r->d_g0, FB);                              // last: its presence says the set is complete
}
}  // namespace

int cl2_render_features(cl2_renderer* r, const uint32_t* seeds, size_t n_words, int samples) {
    STAGE_PROLOGUE(r);
    if (!seeds) return fail(r, CL2_E_INVALID, "NULL seed buffer");
    if (n_words != 2 * (size_t)r->FB) return fail(r, CL2_E_INVALID, "feature seeds: 2 words per pixel of the frame ((W*H, 2) uint32)");
    if (samples < 1 || samples > 65536) return fail(r, CL2_E_INVALID, "feature samples must be in 1..65536");
    const size_t FB = (size_t)r->FB;
    TRY(need_feature_buffers(r));
    r->features_valid = false;
    hipStream_t st = r->stream;
    HIP_TRY(r, hipMemcpyAsync(r->d_feat_seeds, seeds, FB * sizeof(uint2), hipMemcpyHostToDevice, st));
    HIP_TRY(r, hipMemsetAsync(r->d_g0, 0, FB * sizeof(float4), st));
    HIP_TRY(r, hipMemsetAsync(r->d_g1, 0, FB * sizeof(float4), st));
    // the closest-hit dispatch of cl2_probe_traverse, in its uncounted form
    const bool wide = r->traversal_mode == 5 && r->n_wide > 0 && !count_ref(r);
    for (int k = 0; k < samples; k++) {
        hipLaunchKernelGGL(k_feat_rays, dim3(grid_for(FB)), dim3(BLOCK), 0, st, r->FB, r->cam, r->d_feat_seeds, r->d_feat_o, r->d_feat_d);
        HIP_TRY(r, hipGetLastError());
        if (wide) {
            HIP_TRY(r, hipMemsetAsync(r->d_feat_work, 0, WORK_STRIDE * sizeof(unsigned), st));
            PathRaySource src{nullptr, r->d_feat_o, r->d_feat_d, r->d_feat_hit};
            TRY(launch_wide(r, st, 0, r->d_feat_count, r->d_feat_work, src, 0, true));
        } else {
            hipLaunchKernelGGL(k_traverse_paths<false>, dim3(grid_for(FB)), dim3(BLOCK), bvh_lds_bytes(r), st, r->bvh, (const int*)nullptr,
                               r->d_feat_count, r->d_feat_o, r->d_feat_d, r->d_feat_hit, r->d_feat_stats);
            HIP_TRY(r, hipGetLastError());
        }
        hipLaunchKernelGGL(k_feat_shade, dim3(grid_for(FB)), dim3(BLOCK), 0, st, r->FB, r->d_feat_d, r->d_feat_hit, r->d_tri_shade,
                           r->d_mats, r->d_g0, r->d_g1);
        HIP_TRY(r, hipGetLastError());
    }
    hipLaunchKernelGGL(k_feat_finish, dim3(grid_for(FB)), dim3(BLOCK), 0, st, r->FB, samples, r->d_g0, r->d_g1);
    HIP_TRY(r, hipGetLastError());
    TRY(drain(r));
    r->features_valid = true;
    return CL2_OK;
}

int cl2_read_features(cl2_renderer* r, float* g0, float* g1, size_t n_pixels) {
    STAGE_PROLOGUE(r);
    if (!g0 || !g1) return fail(r, CL2_E_INVALID, "NULL feature array");
    if (n_pixels != (size_t)r->FB) return fail(r, CL2_E_INVALID, "feature arrays must hold W*H float4 entries");
    if (!r->features_valid) return fail(r, CL2_E_STATE, "no features for the current scene (call cl2_render_features first)");
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipMemcpy(g0, r->d_g0, n_pixels * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(r, hipMemcpy(g1, r->d_g1, n_pixels * sizeof(float4), hipMemcpyDeviceToHost));
    return CL2_OK;
}

// The counterpart of cl2_read_features: the filters then read these buffers as if cl2_render_features had made them.
int cl2_write_features(cl2_renderer* r, const float* g0, const float* g1, size_t n_pixels) {
    STAGE_PROLOGUE(r);
    if (!g0 || !g1) return fail(r, CL2_E_INVALID, "NULL feature array");
    if (n_pixels != (size_t)r->FB) return fail(r, CL2_E_INVALID, "feature arrays must hold W*H float4 entries");
    TRY(need_feature_buffers(r));
    r->features_valid = false;
    TRY(drain(r));
    HIP_TRY(r, hipMemcpy(r->d_g0, g0, n_pixels * sizeof(float4), hipMemcpyHostToDevice));
    HIP_TRY(r, hipMemcpy(r->d_g1, g1, n_pixels * sizeof(float4), hipMemcpyHostToDevice));
    r->features_valid = true;
    return CL2_OK;
}

namespace {
// working buffers of both filters (cl2_denoise, cl2_denoise_guided), allocated by the first call of either
int need_filter_buffers(cl2_renderer* r) {
    if (r->d_dn_out) return CL2_OK;
    const size_t FB = (size_t)r->FB;
    int rc = dev_alloc(r, &r->d_dn[0], FB);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_dn[1], FB);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_dn_out, 3 * FB);     // last: its presence says the set is complete
    return rc;
}
}  // namespace

namespace {
// The argument checks of every filter call, in the order the callers' tests pin: iterations, then every sigma (`sigma`: the n colour
// sigmas of cl2_denoise / cl2_denoise_layers, or the luma sigma of the guided filters), then the denominators.  `colour`: the
// sigmas are colour sigmas, whose square shrinks by 4 per pass and must stay a normal float32 in the last one.
int filter_arg_checks(cl2_renderer* r, int iterations, const float* sigma, int n, bool colour, float sigma_depth, float sigma_albedo) {
    if (iterations < 0 || iterations > 12) return fail(r, CL2_E_INVALID, "iterations must be in 0..12");
    auto bad = [](float x) { return !(x > 0.0f) || !std::isfinite(x); };
    bool any_bad = bad(sigma_depth) || bad(sigma_albedo);
    for (int l = 0; l < n; l++) any_bad = any_bad || bad(sigma[l]);
    if (any_bad) return fail(r, CL2_E_INVALID, "sigmas must be positive and finite");
    // a denominator below the smallest normal float32 (0 or subnormal) would turn every weight into 0/0 or an untested division
    if (sigma_albedo * sigma_albedo < FLT_MIN) return fail(r, CL2_E_INVALID, "sigma_albedo^2 underflows float32");
    for (int l = 0; colour && l < n; l++)
        if (iterations >= 1 && std::ldexp(sigma[l] * sigma[l], -2 * (iterations - 1)) < FLT_MIN)
            return fail(r, CL2_E_INVALID, "sigma_color^2 * 4^-(iterations-1) underflows float32");
    return CL2_OK;
}

int need_features(cl2_renderer* r) {
    if (!r->features_valid) return fail(r, CL2_E_STATE, "no features for the current scene (call cl2_render_features first)");
    return CL2_OK;
}

// the argument and feature checks of cl2_denoise (`colour`; also cl2_denoise_error's for kind 0) and of cl2_denoise_guided /
// cl2_denoise_robust (also cl2_denoise_error's for kind 1)
int filter_checks(cl2_renderer* r, int iterations, float sigma, bool colour, float sigma_depth, float sigma_albedo) {
    TRY(filter_arg_checks(r, iterations, &sigma, 1, colour, sigma_depth, sigma_albedo));
    return need_features(r);
}

// cl2_denoise after its output checks, shared with cl2_keep_picture: the remaining checks and every launch; the last launch
// writes the (H, W, 3) picture to `dst` (device memory; nullptr: d_dn_out)
int run_denoise(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo, float* dst) {
    TRY(filter_checks(r, iterations, sigma_color, true, sigma_depth, sigma_albedo));
    const size_t FB = (size_t)r->FB;
    TRY(need_filter_buffers(r));
    if (!dst) dst = r->d_dn_out;
    hipLaunchKernelGGL(k_denoise_input, dim3(grid_for(FB)), dim3(BLOCK), 0, r->stream, r->FB, (const float*)r->d_acc, r->d_dn[0],
                       iterations == 0 ? dst : (float*)nullptr);
    HIP_TRY(r, hipGetLastError());
    TRY(denoise_passes(r, iterations, sigma_color, sigma_depth, sigma_albedo, PingPong{r->d_dn[0], r->d_dn, dst, iterations}));
    return drain(r);
}
}  // namespace

int cl2_denoise(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo, float* out_bgr,
                size_t n_floats) {
    STAGE_PROLOGUE(r);
    if (!out_bgr) return fail(r, CL2_E_INVALID, "NULL output");
    if (n_floats != 3 * (size_t)r->FB) return fail(r, CL2_E_INVALID, "denoised picture must hold 3*W*H floats");
    TRY(run_denoise(r, iterations, sigma_color, sigma_depth, sigma_albedo, nullptr));
    HIP_TRY(r, hipMemcpy(out_bgr, r->d_dn_out, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return CL2_OK;
}

// ---------------------------------------------------------------- error estimates (csrc/error_estimate.hpp)
namespace {
int need_moments(cl2_renderer* r) {
    if (!r->d_mom) return fail(r, CL2_E_STATE, "error tracking is off (cl2_set_error_tracking)");
    if (!r->mom_valid)
        return fail(r, CL2_E_STATE, "the moments do not cover every sample in the accumulators (tracking was switched on after samples, "
                                    "or accumulators were written without their moments): cl2_reset_accumulators or cl2_write_moments_packed");
    return CL2_OK;
}

// e(floor) of the current accumulators and moments, reduced on the device in a fixed order
int eval_rel_error(cl2_renderer* r, double floor, double* out) {
    if (!r->d_err_partial) TRY(dev_alloc(r, &r->d_err_partial, (size_t)3 * ERR_BLOCKS + 4));
    const int grid = std::min(grid_for(r->FB), ERR_BLOCKS);
    double* res = r->d_err_partial + 3 * ERR_BLOCKS;
    hipLaunchKernelGGL(k_rel_error_partial, dim3(grid), dim3(256), 0, r->stream, r->FB, (const float*)r->d_acc, (const float*)r->d_mom,
                       floor, r->d_err_partial);
    hipLaunchKernelGGL(k_rel_error_final, dim3(1), dim3(256), 0, r->stream, (const double*)r->d_err_partial, grid, res);
    HIP_TRY(r, hipGetLastError());
    HIP_TRY(r, hipMemcpyAsync(out, res, sizeof(double), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    return CL2_OK;
}

// ---- adaptive sampling (adaptive.hpp) ----
int ensure_density_buffers(cl2_renderer* r) {
    const size_t FB = (size_t)r->FB;
    if (!r->d_cam_count) {                                   // kept for the life of the handle: counts survive a NULL density
        TRY(dev_alloc(r, &r->d_cam_count, FB));
        HIP_TRY(r, hipMemset(r->d_cam_count, 0, FB * sizeof(unsigned)));
    }
    if (r->d_dens_tmp) return CL2_OK;                        // the last thing set up (see ensure_det_buffers)
    dev_free(r, r->d_dens_C); dev_free(r, r->d_dens_M); dev_free(r, r->d_dens_invm); dev_free(r, r->d_dens_m);
    dev_free(r, r->d_dens_partial); dev_free(r, r->d_dens_fsum);
    TRY(dev_alloc(r, &r->d_dens_C, FB));
    TRY(dev_alloc(r, &r->d_dens_M, FB));
    TRY(dev_alloc(r, &r->d_dens_invm, FB));
    TRY(dev_alloc(r, &r->d_dens_m, FB));
    TRY(dev_alloc(r, &r->d_dens_partial, (size_t)3 * DENS_BLOCKS + 3));
    TRY(dev_alloc(r, &r->d_dens_fsum, (size_t)1));
    size_t bytes = 0;
    HIP_TRY(r, dens_scan(nullptr, bytes, r->d_dens_M, r->d_dens_C, FB, r->stream));
    unsigned char* tmp = nullptr;
    TRY(dev_alloc(r, &tmp, bytes));
    r->d_dens_tmp = tmp; r->dens_tmp_bytes = bytes;
    return CL2_OK;
}

void free_density(cl2_renderer* r) {
    dev_free(r, r->d_dens_C); dev_free(r, r->d_dens_M); dev_free(r, r->d_dens_invm); dev_free(r, r->d_dens_m);
    dev_free(r, r->d_dens_partial); dev_free(r, r->d_dens_fsum);
    unsigned char* tmp = static_cast<unsigned char*>(r->d_dens_tmp);
    dev_free(r, tmp);
    r->d_dens_tmp = nullptr; r->dens_tmp_bytes = 0;
    for (int q = 0; q < 3; q++) dev_free(r, r->d_map[q]);
    r->density = false;
}

// d_dens_m holds W*H positive finite weights: normalise to mean 1, quantise (M, sum M = W*H 2^16), 1/m and the prefix sum C
int dens_quantise(cl2_renderer* r) {
    const int FB = r->FB;
    hipStream_t st = r->stream;
    const int grid = std::min((FB + 255) / 256, DENS_BLOCKS);
    double* tot = r->d_dens_partial + 3 * DENS_BLOCKS;
    hipLaunchKernelGGL(k_dens_sum, dim3(grid), dim3(256), 0, st, FB, (const float*)r->d_dens_m, r->d_dens_partial);
    hipLaunchKernelGGL(k_dens_final, dim3(1), dim3(256), 0, st, (const double*)r->d_dens_partial, grid, tot);
    HIP_TRY(r, hipMemsetAsync(r->d_dens_fsum, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_dens_floor, dim3((FB + 255) / 256), dim3(256), 0, st, FB, (const float*)r->d_dens_m, (const double*)tot,
                       r->d_dens_M, r->d_dens_fsum);
    HIP_TRY(r, hipGetLastError());
    unsigned long long fsum = 0;
    HIP_TRY(r, hipMemcpyAsync(&fsum, r->d_dens_fsum, sizeof fsum, hipMemcpyDeviceToHost, st));
    HIP_TRY(r, hipStreamSynchronize(st));
    const uint64_t target = (uint64_t)FB * 65535u;
    if (fsum > target) { r->density = false; return fail(r, CL2_E_STATE, "density quantisation: the floors exceed the frame's units"); }
    hipLaunchKernelGGL(k_dens_finish, dim3((FB + 255) / 256), dim3(256), 0, st, FB, (uint64_t)(target - fsum), r->d_dens_M, r->d_dens_invm);
    HIP_TRY(r, hipGetLastError());
    size_t bytes = r->dens_tmp_bytes;
    HIP_TRY(r, dens_scan(r->d_dens_tmp, bytes, r->d_dens_M, r->d_dens_C, (size_t)FB, st));
    uint64_t last = 0;
    HIP_TRY(r, hipMemcpyAsync(&last, r->d_dens_C + (FB - 1), sizeof last, hipMemcpyDeviceToHost, st));
    HIP_TRY(r, hipStreamSynchronize(st));
    if (last != ((uint64_t)FB << DENS_SHIFT)) { r->density = false; return fail(r, CL2_E_STATE, "density quantisation: the units do not add up"); }
    r->density = true;
    return CL2_OK;
}

int dens_update(cl2_renderer* r, double floor, double share) {
    TRY(ensure_density_buffers(r));
    hipStream_t st = r->stream;
    const int grid = std::min((r->FB + 255) / 256, DENS_BLOCKS);
    double* tot = r->d_dens_partial + 3 * DENS_BLOCKS;
    hipLaunchKernelGGL(k_dens_terms, dim3(grid), dim3(256), 0, st, r->FB, (const float*)r->d_acc, (const float*)r->d_mom, floor,
                       r->d_dens_m, r->d_dens_partial);
    hipLaunchKernelGGL(k_dens_final, dim3(1), dim3(256), 0, st, (const double*)r->d_dens_partial, grid, tot);
    HIP_TRY(r, hipGetLastError());
    double h[3] = {0, 0, 0};
    HIP_TRY(r, hipMemcpyAsync(h, tot, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(r, hipStreamSynchronize(st));
    if (!(h[1] > 0.0)) return fail(r, CL2_E_STATE, "no pixel has a finite error term (fewer than two samples everywhere)");
    hipLaunchKernelGGL(k_dens_from_terms, dim3((r->FB + 255) / 256), dim3(256), 0, st, r->FB, (const double*)tot, share, r->d_dens_m);
    HIP_TRY(r, hipGetLastError());
    return dens_quantise(r);
}

int no_comm(cl2_renderer* r) {
    if (r->comm) return fail(r, CL2_E_STATE, "adaptive sampling is per handle: not on a handle with a communicator");
    return CL2_OK;
}
}  // namespace

int cl2_set_error_tracking(cl2_renderer* r, int on) {
    if (!r) return CL2_E_INVALID;
    if (on != 0 && on != 1) return fail(r, CL2_E_INVALID, "error tracking: 0 off, 1 on");
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    if (!on) {
        dev_free(r, r->d_mom);
        r->mom_valid = false;
        return CL2_OK;
    }
    if (r->d_mom) return CL2_OK;
    return side_sum_on(r, r->d_mom, 8 * (size_t)r->FB, r->mom_valid, "moments");
}

int cl2_get_error_tracking(const cl2_renderer* r) { return r ? (r->d_mom ? 1 : 0) : CL2_E_INVALID; }

int cl2_read_moments_packed(cl2_renderer* r, float* dst, size_t n_floats) {
    if (!r || !dst) return CL2_E_INVALID;
    if (n_floats != 8 * (size_t)r->FB) return fail(r, CL2_E_INVALID, "packed moments hold 8*W*H floats");
    TRY(need_moments(r));
    return packed_copy(r, dst, r->d_mom, n_floats, hipMemcpyDeviceToHost);
}

int cl2_write_moments_packed(cl2_renderer* r, const float* src, size_t n_floats) {
    if (!r || !src) return CL2_E_INVALID;
    if (n_floats != 8 * (size_t)r->FB) return fail(r, CL2_E_INVALID, "packed moments hold 8*W*H floats");
    if (!r->d_mom) return fail(r, CL2_E_STATE, "error tracking is off (cl2_set_error_tracking)");
    TRY(packed_copy(r, r->d_mom, src, n_floats, hipMemcpyHostToDevice));
    r->mom_valid = true;
    return CL2_OK;
}

int cl2_read_standard_error(cl2_renderer* r, float* out, size_t n_floats) {
    if (!r || !out) return CL2_E_INVALID;
    if (n_floats != 4 * (size_t)r->FB) return fail(r, CL2_E_INVALID, "the standard errors hold 4*W*H floats");
    TRY(need_moments(r));
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    Scratch<float4> d(r);
    TRY(d.alloc((size_t)r->FB));
    hipLaunchKernelGGL(k_standard_error, dim3((r->FB + 255) / 256), dim3(256), 0, r->stream, r->FB, (const float*)r->d_acc,
                       (const float*)r->d_mom, d.p);
    HIP_TRY(r, hipGetLastError());
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipMemcpy(out, d, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return CL2_OK;
}

// ---------------------------------------------------------------- robust picture (csrc/robust.hpp)
int cl2_set_robust_buckets(cl2_renderer* r, int M) {
    if (!r) return CL2_E_INVALID;
    if (M != 0 && (M < ROBUST_MIN_BUCKETS || M > ROBUST_MAX_BUCKETS)) return fail(r, CL2_E_INVALID, "robust buckets: 0 off, 3..16 on");
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    if (M == r->bkt_M) return CL2_OK;
    dev_free(r, r->d_bkt);                                       // off, or another M: the sums of the old buckets mean nothing
    r->bkt_M = 0;
    r->bkt_valid = false;
    if (M == 0) return CL2_OK;
    TRY(side_sum_on(r, r->d_bkt, 4 * (size_t)M * (size_t)r->FB, r->bkt_valid, "robust buckets"));
    r->bkt_M = M;
    return CL2_OK;
}

int cl2_get_robust_buckets(const cl2_renderer* r) { return r ? r->bkt_M : CL2_E_INVALID; }

int cl2_read_buckets_packed(cl2_renderer* r, float* dst, size_t n_floats) {
    if (!r || !dst) return CL2_E_INVALID;
    if (!r->d_bkt) return fail(r, CL2_E_STATE, "the robust buckets are off (cl2_set_robust_buckets)");
    if (n_floats != 4 * (size_t)r->bkt_M * (size_t)r->FB) return fail(r, CL2_E_INVALID, "packed buckets hold 4*M*W*H floats");
    return packed_copy(r, dst, r->d_bkt, n_floats, hipMemcpyDeviceToHost);
}

int cl2_write_buckets_packed(cl2_renderer* r, const float* src, size_t n_floats) {
    if (!r || !src) return CL2_E_INVALID;
    if (!r->d_bkt) return fail(r, CL2_E_STATE, "the robust buckets are off (cl2_set_robust_buckets)");
    if (n_floats != 4 * (size_t)r->bkt_M * (size_t)r->FB) return fail(r, CL2_E_INVALID, "packed buckets hold 4*M*W*H floats");
    TRY(packed_copy(r, r->d_bkt, src, n_floats, hipMemcpyHostToDevice));
    r->bkt_valid = true;
    return CL2_OK;
}

namespace {
// the state cl2_robust_picture and cl2_denoise_robust need of the buckets
int robust_ready(cl2_renderer* r) {
    if (!r->d_bkt) return fail(r, CL2_E_STATE, "the robust buckets are off (cl2_set_robust_buckets)");
    if (!r->bkt_valid)
        return fail(r, CL2_E_STATE, "the buckets do not cover every sample in the accumulators (they were switched on or resized after "
                                    "samples, or accumulators were written without their buckets): cl2_reset_accumulators or "
                                    "cl2_write_buckets_packed");
    return CL2_OK;
}

// cl2_robust_picture's launch on drained streams, shared with cl2_keep_picture: the picture to `d` (device memory, 3*W*H floats),
// the statistics to d_stats (or nullptr); returns when the kernel has finished
int run_robust(cl2_renderer* r, float* d, float2* d_stats) {
    const size_t FB = (size_t)r->FB;
    hipLaunchKernelGGL(k_robust_picture, dim3((unsigned)((FB + 255) / 256)), dim3(256), 0, r->stream, FB, r->bkt_M, (const float*)r->d_bkt,
                       d, d_stats);
    int rc = hipGetLastError() == hipSuccess ? CL2_OK : fail(r, CL2_E_HIP, "k_robust_picture launch failed");
    if (rc == CL2_OK && hipStreamSynchronize(r->stream) != hipSuccess) rc = fail(r, CL2_E_HIP, "k_robust_picture failed");
    return rc;
}
}  // namespace

int cl2_robust_picture(cl2_renderer* r, float* out_bgr, size_t n_floats, float* out_stats, size_t n_stats) {
    if (!r || !out_bgr) return CL2_E_INVALID;
    if (n_floats != 3 * (size_t)r->FB) return fail(r, CL2_E_INVALID, "the robust picture holds 3*W*H floats");
    if (out_stats ? n_stats != 2 * (size_t)r->FB : n_stats != 0)
        return fail(r, CL2_E_INVALID, "the robust statistics hold 2*W*H floats (or are NULL with n_stats 0)");
    TRY(robust_ready(r));
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    const size_t FB = (size_t)r->FB;
    Scratch<float> d(r);
    TRY(d.alloc(5 * FB + 1));
    float2* d_stats = out_stats ? reinterpret_cast<float2*>(d.p + 3 * FB + (FB & 1)) : nullptr;   // 8-byte aligned: 3 FB + (FB & 1) is even
    TRY(run_robust(r, d, d_stats));
    HIP_TRY(r, hipMemcpy(out_bgr, d, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    if (out_stats) HIP_TRY(r, hipMemcpy(out_stats, d_stats, n_stats * sizeof(float), hipMemcpyDeviceToHost));
    return CL2_OK;
}

// The variance-guided filter (denoise_guided.hpp): cl2_denoise's passes with the luma edge-stop driven by the moments.
namespace {
// cl2_denoise_guided / cl2_denoise_robust after their output checks, shared with cl2_keep_picture: the remaining checks and every
// launch.  `robust`: the input pass reads the buckets (cl2_denoise_robust) instead of accumulators and moments.  `want_var`: the
// guide variance is carried into d_dn_var.  The last launch writes the (H, W, 3) picture to `dst` (device memory; nullptr: d_dn_out).
int run_guided(cl2_renderer* r, bool robust, int iterations, float sigma_luma, float sigma_depth, float sigma_albedo, bool want_var,
               float* dst) {
    TRY(filter_checks(r, iterations, sigma_luma, false, sigma_depth, sigma_albedo));
    if (robust)
        TRY(robust_ready(r));
    else
        TRY(need_moments(r));
    const size_t FB = (size_t)r->FB;
    TRY(need_filter_buffers(r));
    if (!r->d_dn_var) TRY(dev_alloc(r, &r->d_dn_var, FB));
    if (!dst) dst = r->d_dn_out;
    hipStream_t st = r->stream;
    float* const dvar = want_var ? r->d_dn_var : nullptr;
    if (robust)
        hipLaunchKernelGGL(k_denoise_robust_input, dim3((unsigned)((FB + 255) / 256)), dim3(256), 0, st, FB, r->bkt_M, (const float*)r->d_bkt,
                           r->d_dn[0], iterations == 0 ? dst : (float*)nullptr, dvar);
    else
        hipLaunchKernelGGL(k_denoise_guided_input, dim3(grid_for(FB)), dim3(BLOCK), 0, st, r->FB, (const float*)r->d_acc,
                           (const float*)r->d_mom, r->d_dn[0], iterations == 0 ? dst : (float*)nullptr, dvar);
    HIP_TRY(r, hipGetLastError());
    TRY(guided_passes(r, iterations, sigma_luma, sigma_depth, sigma_albedo, PingPong{r->d_dn[0], r->d_dn, dst, iterations}, dvar));
    return drain(r);
}

// the output checks and the downloads of cl2_denoise_guided and cl2_denoise_robust
int guided_call(cl2_renderer* r, bool robust, int iterations, float sigma_luma, float sigma_depth, float sigma_albedo, float* out_bgr,
                size_t n_floats, float* out_var, size_t n_var) {
    STAGE_PROLOGUE(r);
    if (!out_bgr) return fail(r, CL2_E_INVALID, "NULL output");
    if (n_floats != 3 * (size_t)r->FB) return fail(r, CL2_E_INVALID, "denoised picture must hold 3*W*H floats");
    if (out_var ? n_var != (size_t)r->FB : n_var != 0)
        return fail(r, CL2_E_INVALID, "guide variance must hold W*H floats (or be NULL with n_var 0)");
    TRY(run_guided(r, robust, iterations, sigma_luma, sigma_depth, sigma_albedo, out_var != nullptr, nullptr));
    HIP_TRY(r, hipMemcpy(out_bgr, r->d_dn_out, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    if (out_var) HIP_TRY(r, hipMemcpy(out_var, r->d_dn_var, n_var * sizeof(float), hipMemcpyDeviceToHost));
    return CL2_OK;
}
}  // namespace

int cl2_denoise_guided(cl2_renderer* r, int iterations, float sigma_luma, float sigma_depth, float sigma_albedo, float* out_bgr,
                       size_t n_floats, float* out_var, size_t n_var) {
    return guided_call(r, false, iterations, sigma_luma, sigma_depth, sigma_albedo, out_bgr, n_floats, out_var, n_var);
}

// The guided filter on the robust picture (denoise_robust.hpp): colour and guide variance from the kept buckets, then
// cl2_denoise_guided's passes.  Reads the buckets and the features only.
int cl2_denoise_robust(cl2_renderer* r, int iterations, float sigma_luma, float sigma_depth, float sigma_albedo, float* out_bgr,
                       size_t n_floats, float* out_var, size_t n_var) {
    return guided_call(r, true, iterations, sigma_luma, sigma_depth, sigma_albedo, out_bgr, n_floats, out_var, n_var);
}

// The error estimate of the filtered picture (denoise_error.hpp): Monte-Carlo SURE over the passes of cl2_denoise
// (kind 0) or cl2_denoise_guided (kind 1).  Reads accumulators, moments and features; writes its own buffers and the filters'
// working buffers (d_dn[], d_dn_out); d_dn_var, a kept picture, seeds and counters are not touched.
namespace {
// the noise model of the SURE calls: 0 independent signs, 1 reconstruction-correlated, 2 split (error_split.hpp).  `legacy`: the call
// came through an entry point that takes `correlated`, 0 or 1, and keeps its message
int check_noise_model(cl2_renderer* r, int model, bool legacy) {
    if (legacy) return (model < 0 || model > 1) ? fail(r, CL2_E_INVALID, "correlated must be 0 or 1") : CL2_OK;
    return (model < 0 || model > 2) ? fail(r, CL2_E_INVALID, "noise_model must be 0 (independent), 1 (correlated) or 2 (split)") : CL2_OK;
}
// the arguments every SURE call shares, in the order their tests pin
int sure_arg_checks(cl2_renderer* r, int probes, float epsilon, int model, bool legacy, double floor) {
    if (probes < 1 || probes > 16) return fail(r, CL2_E_INVALID, "probes must be in 1..16");
    if (!(epsilon > 0.0f) || !std::isfinite(epsilon)) return fail(r, CL2_E_INVALID, "epsilon must be positive and finite");
    TRY(check_noise_model(r, model, legacy));
    if (!(floor >= 0.0) || !std::isfinite(floor)) return fail(r, CL2_E_INVALID, "floor must be >= 0 and finite");
    return CL2_OK;
}
// The mean reconstruction weights of a camera sample, in float64 with erf (denoise_error.hpp).  `correlated`: the noise model reads
// them (1 and 2), so weights that are not positive and finite are refused; the independent model carries them unread.
int reconstruction_weights(cl2_renderer* r, bool correlated, DeKernel& K) {
    const float ppw = r->cam.phys_width / r->cam.pixel_width, pph = r->cam.phys_height / r->cam.pixel_height;
    const double s2 = (double)ppw * ppw + (double)pph * pph;
    const double c[2] = {s2 / (2.0 * ppw * ppw), s2 / (2.0 * pph * pph)};
    for (int a = 0; a < 2; a++)
        for (int i = -1; i <= 1; i++) {
            const double q = std::sqrt(c[a]);
            const double k = 0.5 * std::sqrt(c[a] * 3.14159265358979323846) * (std::erf((1.0 - i) / q) - std::erf(-i / q));
            if (correlated && !(k > 0.0 && std::isfinite(k)))
                return fail(r, CL2_E_STATE, "the camera's pixel sizes give no reconstruction weights");
            (a == 0 ? K.kx : K.ky)[i + 1] = (float)k;
        }
    return CL2_OK;
}
int need_split_rows(cl2_renderer* r) {
    if (!r->d_smom) return fail(r, CL2_E_STATE, "split tracking is off (cl2_set_split_tracking)");
    if (!r->smom_valid)
        return fail(r, CL2_E_STATE, "the split rows do not cover every sample in the accumulators (tracking was switched on after samples, "
                                    "accumulators were written without them, or they were reduced over ranks): cl2_reset_accumulators or "
                                    "cl2_write_split_moments_packed");
    return CL2_OK;
}
// the light share of noise model 2 into d_de_rho, on `st`
int launch_de_rho(cl2_renderer* r, hipStream_t st) {
    hipLaunchKernelGGL(k_de_rho, dim3((unsigned)(((size_t)r->FB + 255) / 256)), dim3(256), 0, st, r->FB, (const float*)r->d_acc,
                       (const float*)r->d_mom, (const float*)r->d_smom, r->d_de_rho);
    HIP_TRY(r, hipGetLastError());
    return CL2_OK;
}
// k_de_perturb, or k_de_perturb_split for model 2
void launch_de_perturb(cl2_renderer* r, hipStream_t st, int model, uint32_t t, float eps, const DeKernel& K, const float4* Y,
                       const float4* A, float4* Yp, float* out3) {
    const dim3 grid(grid_for((size_t)r->FB)), block(BLOCK);
    if (model == 2)
        hipLaunchKernelGGL(k_de_perturb_split, grid, block, 0, st, r->W, r->H, t, eps, K, (const float*)r->d_de_rho, Y, A, Yp, out3);
    else
        hipLaunchKernelGGL(k_de_perturb, grid, block, 0, st, r->W, r->H, t, eps, model, K, Y, A, Yp, out3);
}

int run_denoise_error(cl2_renderer* r, int kind, int iterations, float sigma, float sigma_depth, float sigma_albedo, int probes,
                      float epsilon, int model, bool legacy, uint32_t seed, double floor, double* out, float* out_map, size_t n_map,
                      float* out_probe, size_t n_probe) {
    STAGE_PROLOGUE(r);
    if (!out) return fail(r, CL2_E_INVALID, "NULL output");
    if (kind < 0 || kind > 1) return fail(r, CL2_E_INVALID, "denoise error: kind 0 (cl2_denoise) or 1 (cl2_denoise_guided)");
    TRY(sure_arg_checks(r, probes, epsilon, model, legacy, floor));
    const size_t FB = (size_t)r->FB;
    if (out_map ? n_map != FB : n_map != 0) return fail(r, CL2_E_INVALID, "the error map must hold W*H floats (or be NULL with n_map 0)");
    if (out_probe ? n_probe != 9 * FB : n_probe != 0)
        return fail(r, CL2_E_INVALID, "the probe pictures must hold 3*(3*W*H) floats (or be NULL with n_probe 0)");
    TRY(filter_checks(r, iterations, sigma, kind == 0, sigma_depth, sigma_albedo));
    TRY(need_moments(r));
    if (model == 2) TRY(need_split_rows(r));
    DeKernel K;
    TRY(reconstruction_weights(r, model != 0, K));
    TRY(drain(r));
    TRY(need_filter_buffers(r));
    if (model == 2 && !r->d_de_rho) TRY(dev_alloc(r, &r->d_de_rho, FB));
    const int grid = std::min(grid_for(FB), ERR_BLOCKS);
    if (!r->d_de_sum) {
        int rc = dev_alloc(r, &r->d_de_y, FB);
        if (rc == CL2_OK) rc = dev_alloc(r, &r->d_de_a, FB);
        if (rc == CL2_OK) rc = dev_alloc(r, &r->d_de_yp, FB);
        if (rc == CL2_OK) rc = dev_alloc(r, &r->d_de_fy, 3 * FB);
        if (rc == CL2_OK) rc = dev_alloc(r, &r->d_de_map, FB);
        if (rc == CL2_OK) rc = dev_alloc(r, &r->d_de_sum, FB + (size_t)DE_SUMS * ERR_BLOCKS + 8);   // last: the set is complete
        if (rc != CL2_OK) return rc;
    }
    double* const partial = r->d_de_sum + FB;
    double* const res = partial + (size_t)DE_SUMS * ERR_BLOCKS;
    hipStream_t st = r->stream;
    auto passes = [&](const float4* src, float* dst) {
        const PingPong io{src, r->d_dn, dst, iterations};
        return kind == 0 ? denoise_passes(r, iterations, sigma, sigma_depth, sigma_albedo, io)
                         : guided_passes(r, iterations, sigma, sigma_depth, sigma_albedo, io, nullptr);
    };
    hipLaunchKernelGGL(k_de_input, dim3(grid_for(FB)), dim3(BLOCK), 0, st, r->FB, kind, (const float*)r->d_acc, (const float*)r->d_mom,
                       r->d_de_y, r->d_de_a, iterations == 0 ? r->d_de_fy : (float*)nullptr);
    HIP_TRY(r, hipGetLastError());
    TRY(passes(r->d_de_y, r->d_de_fy));
    HIP_TRY(r, hipMemsetAsync(r->d_de_sum, 0, FB * sizeof(double), st));
    if (model == 2) TRY(launch_de_rho(r, st));
    const double scale = ((double)epsilon * (double)epsilon) * (double)probes;
    for (int k = 0; k < probes; k++) {
        launch_de_perturb(r, st, model, seed + (uint32_t)k, epsilon, K, (const float4*)r->d_de_y, (const float4*)r->d_de_a, r->d_de_yp,
                          iterations == 0 ? r->d_dn_out : (float*)nullptr);
        HIP_TRY(r, hipGetLastError());
        TRY(passes(r->d_de_yp, r->d_dn_out));
        auto terms = [&](auto LAST) {
            hipLaunchKernelGGL(k_de_terms<LAST.value != 0>, dim3(grid), dim3(256), 0, st, r->FB, (const float4*)r->d_de_y,
                               (const float4*)r->d_de_yp, (const float*)r->d_de_fy, (const float*)r->d_dn_out, (const float4*)r->d_de_a,
                               r->d_de_sum, scale, floor, r->d_de_map, partial);
        };
        if (k == probes - 1) terms(int_c<1>{}); else terms(int_c<0>{});
        HIP_TRY(r, hipGetLastError());
    }
    hipLaunchKernelGGL(k_de_final, dim3(1), dim3(256), 0, st, (const double*)partial, grid, res);
    HIP_TRY(r, hipGetLastError());
    TRY(drain(r));
    HIP_TRY(r, hipMemcpy(out, res, 8 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_map) HIP_TRY(r, hipMemcpy(out_map, r->d_de_map, FB * sizeof(float), hipMemcpyDeviceToHost));
    if (out_probe) {
        // y' is a float4 buffer: its colours go out through d_de_fy, once F(y) has left it
        HIP_TRY(r, hipMemcpy(out_probe + 3 * FB, r->d_de_fy, 3 * FB * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(r, hipMemcpy(out_probe + 6 * FB, r->d_dn_out, 3 * FB * sizeof(float), hipMemcpyDeviceToHost));
        hipLaunchKernelGGL(k_de_pack, dim3(grid_for(FB)), dim3(BLOCK), 0, st, r->FB, (const float4*)r->d_de_yp, r->d_de_fy);
        HIP_TRY(r, hipGetLastError());
        HIP_TRY(r, hipStreamSynchronize(st));
        HIP_TRY(r, hipMemcpy(out_probe, r->d_de_fy, 3 * FB * sizeof(float), hipMemcpyDeviceToHost));
    }
    return CL2_OK;
}
}  // namespace

int cl2_denoise_error(cl2_renderer* r, int kind, int iterations, float sigma, float sigma_depth, float sigma_albedo, int probes,
                      float epsilon, int correlated, uint32_t seed, double floor, double* out, float* out_map, size_t n_map,
                      float* out_probe, size_t n_probe) {
    return run_denoise_error(r, kind, iterations, sigma, sigma_depth, sigma_albedo, probes, epsilon, correlated, true, seed, floor, out,
                             out_map, n_map, out_probe, n_probe);
}

// ---------------------------------------------------------------- kept picture and its tone map (csrc/tonemap_picture.hpp)
namespace {
int need_picture(cl2_renderer* r) {
    if (!r->pic_kind) return fail(r, CL2_E_STATE, "no kept picture (cl2_keep_picture or cl2_write_picture first)");
    return CL2_OK;
}
}  // namespace

int cl2_keep_picture(cl2_renderer* r, int kind, int iterations, float sigma, float sigma_depth, float sigma_albedo) {
    if (!r) return CL2_E_INVALID;
    if (kind < 0 || kind > 4) return fail(r, CL2_E_INVALID, "kept picture: 0 none, 1 denoised, 2 guided, 3 robust, 4 robust-guided");
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    if (kind == 0) {
        dev_free(r, r->d_pic);
        r->pic_kind = 0;
        return CL2_OK;
    }
    if (kind == 3)
        TRY(robust_ready(r));
    else
        STAGE_PROLOGUE(r);
    return keep_into_picture(r, kind, [&](float* pic) {
        if (kind == 1) return run_denoise(r, iterations, sigma, sigma_depth, sigma_albedo, pic);
        if (kind == 3) return run_robust(r, pic, nullptr);
        return run_guided(r, kind == 4, iterations, sigma, sigma_depth, sigma_albedo, false, pic);
    });
}

int cl2_kept_picture(const cl2_renderer* r) { return r ? r->pic_kind : 0; }

// ---------------------------------------------------------------- the filter over the layers (csrc/denoise_layers.hpp)
namespace {
int need_layer_filter_buffers(cl2_renderer* r) {
    if (r->d_ldn[1]) return CL2_OK;
    const size_t n = (size_t)r->n_layers * (size_t)r->FB;
    int rc = dev_alloc(r, &r->d_ldn[0], n);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_ldn[1], n);          // last: its presence says the pair is complete
    if (rc != CL2_OK) dev_free(r, r->d_ldn[0]);
    return rc;
}

// cl2_denoise_layers and cl2_keep_layer_picture after their own argument checks (a table is set, sigma_color is not NULL): the
// checks of run_denoise for every layer's sigma, the state checks, and every launch on drained streams.
//   layer >= 0   only that layer is filtered; the last launch writes its (H, W, 3) picture to `dst` (device memory)
//   layer == -1  every layer; the packed pictures [L][H][W][3] end in one working buffer (*layers_out) and, if `want_sum`, their sum
//                goes to `dst`, or with dst == nullptr into the other working buffer (*sum_out)
// Every refusal comes before the first launch.
int run_denoise_layers(cl2_renderer* r, int layer, int iterations, const float* sigma_color, float sigma_depth, float sigma_albedo,
                       bool want_sum, float* dst, const float** layers_out, const float** sum_out) {
    const int L = r->n_layers;
    TRY(filter_arg_checks(r, iterations, sigma_color, L, true, sigma_depth, sigma_albedo));
    TRY(need_valid_layers(r));
    TRY(need_features(r));
    TRY(need_layer_filter_buffers(r));
    const size_t FB = (size_t)r->FB;
    const int l0 = layer < 0 ? 0 : layer, nl = layer < 0 ? L : 1;
    float* const packed = layer < 0 ? (float*)r->d_ldn[iterations & 1] : dst;      // [nl][H][W][3], written by the last launch
    hipStream_t st = r->stream;
    hipLaunchKernelGGL(k_layers_input, dim3(grid_for(FB)), dim3(BLOCK), 0, st, r->FB, l0, nl, (const float*)r->d_acc,
                       (const float*)r->d_lacc, r->d_ldn[0], iterations == 0 ? packed : (float*)nullptr);
    HIP_TRY(r, hipGetLastError());
    const float den_a = sigma_albedo * sigma_albedo;
    TRY(filter_passes(r, iterations, PingPong{r->d_ldn[0], r->d_ldn, packed, iterations}, [&](auto LDS_STEP, int i, int step, PassIO b) {
        LayerDen den{};
        for (int l = 0; l < L; l++) den.den_c[l] = std::ldexp(sigma_color[l] * sigma_color[l], -2 * i);      // as denoise_passes
        hipLaunchKernelGGL(k_layers_denoise_pass<LDS_STEP.value>, dn_tiles(r), DN_BLOCK, 0, st, r->W, r->H, step, l0, nl, den, sigma_depth, den_a,
                           b.cin, r->d_g0, r->d_g1, b.cout, b.out3);
    }));
    if (layers_out) *layers_out = packed;
    if (layer < 0 && want_sum) {
        // the packed pictures fill 3/4 of their buffer; the other buffer was last read by the launch that wrote them
        float* sum = dst ? dst : (float*)r->d_ldn[(iterations + 1) & 1];
        hipLaunchKernelGGL(k_layers_sum, dim3(grid_for(3 * FB)), dim3(BLOCK), 0, st, 3 * FB, L, (const float*)packed, sum);
        HIP_TRY(r, hipGetLastError());
        if (sum_out) *sum_out = sum;
    }
    return drain(r);
}
}  // namespace

int cl2_denoise_layers(cl2_renderer* r, int iterations, const float* sigma_color, float sigma_depth, float sigma_albedo,
                       float* out_layers, size_t n_layer_floats, float* out_sum, size_t n_sum_floats) {
    STAGE_PROLOGUE(r);
    if (!sigma_color) return fail(r, CL2_E_INVALID, "NULL sigma_color (one per layer)");
    if (!out_layers && !out_sum) return fail(r, CL2_E_INVALID, "NULL outputs: out_layers, out_sum or both");
    if (r->n_layers == 0) return fail(r, CL2_E_STATE, "no layer table is set (cl2_set_layers)");
    const size_t FB = (size_t)r->FB;
    if (out_layers && n_layer_floats != 3 * (size_t)r->n_layers * FB) return fail(r, CL2_E_INVALID, "denoised layers must hold n_layers*3*W*H floats");
    if (out_sum && n_sum_floats != 3 * FB) return fail(r, CL2_E_INVALID, "the sum of the denoised layers must hold 3*W*H floats");
    TRY(drain(r));
    const float *layers = nullptr, *sum = nullptr;
    TRY(run_denoise_layers(r, -1, iterations, sigma_color, sigma_depth, sigma_albedo, out_sum != nullptr, nullptr, &layers, &sum));
    if (out_layers) HIP_TRY(r, hipMemcpy(out_layers, layers, n_layer_floats * sizeof(float), hipMemcpyDeviceToHost));
    if (out_sum) HIP_TRY(r, hipMemcpy(out_sum, sum, n_sum_floats * sizeof(float), hipMemcpyDeviceToHost));
    return CL2_OK;
}

int cl2_keep_layer_picture(cl2_renderer* r, int layer, int iterations, const float* sigma_color, float sigma_depth, float sigma_albedo) {
    STAGE_PROLOGUE(r);
    if (!sigma_color) return fail(r, CL2_E_INVALID, "NULL sigma_color (one per layer)");
    if (r->n_layers == 0) return fail(r, CL2_E_STATE, "no layer table is set (cl2_set_layers)");
    if (layer < -1 || layer >= r->n_layers) return fail(r, CL2_E_INVALID, "kept layer picture: a layer of the table (0..n_layers-1) or -1 for the sum");
    TRY(drain(r));
    return keep_into_picture(r, layer < 0 ? 7 : 6, [&](float* pic) {
        return run_denoise_layers(r, layer, iterations, sigma_color, sigma_depth, sigma_albedo, true, pic, nullptr, nullptr);
    });
}

// ---------------------------------------------------------------- the filter's scale per pixel (csrc/denoise_select.hpp, DESIGN 6.16;
// declared in include/clive2_amd_ext.h)
namespace {
// buffers for K + 1 = `levels` candidates: kept while they are large enough, made again when K grows
int need_select_buffers(cl2_renderer* r, int levels) {
    if (r->ds_levels >= levels) return CL2_OK;
    dev_free(r, r->d_ds_lev); dev_free(r, r->d_ds_a); dev_free(r, r->d_ds_sum); dev_free(r, r->d_ds_map);
    dev_free(r, r->d_ds_scale); dev_free(r, r->d_ds_out);
    r->ds_levels = 0;
    const size_t FB = (size_t)r->FB, n = (size_t)levels * FB;
    int rc = dev_alloc(r, &r->d_ds_lev, 2 * n);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_ds_a, FB);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_ds_sum, n + (size_t)DE_SUMS * ERR_BLOCKS + 8);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_ds_map, 3 * n);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_ds_scale, FB);
    if (rc == CL2_OK) rc = dev_alloc(r, &r->d_ds_out, 3 * FB);
    if (rc == CL2_OK) r->ds_levels = levels;                       // last: the set is complete
    return rc;
}

// The checks that follow the callers' own (handle, outputs, sizes) and every launch, on drained streams; the picture goes to `dst`
// (device memory; nullptr: d_ds_out).  Every refusal but CL2_E_NOMEM and CL2_E_HIP comes before the first allocation and launch.
// *maps_out: where M lies (m is d_ds_map).  The buffers are laid out for r->ds_levels, the launches use K + 1 of them.
int run_select(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo, int probes, float epsilon,
               int model, bool legacy, uint32_t seed, int smooth_passes, double floor, float* dst, const float** maps_out) {
    if (iterations < 1 || iterations > 12) return fail(r, CL2_E_INVALID, "scale selection: iterations must be in 1..12");
    if (smooth_passes < 0 || smooth_passes > DS_MAX_SMOOTH) return fail(r, CL2_E_INVALID, "smooth_passes must be in 0..4");
    TRY(sure_arg_checks(r, probes, epsilon, model, legacy, floor));
    TRY(filter_checks(r, iterations, sigma_color, true, sigma_depth, sigma_albedo));
    TRY(need_moments(r));
    if (model == 2) TRY(need_split_rows(r));
    DeKernel K;
    TRY(reconstruction_weights(r, model != 0, K));
    TRY(drain(r));
    const int levels = iterations + 1;
    TRY(need_select_buffers(r, levels));
    if (model == 2 && !r->d_de_rho) TRY(dev_alloc(r, &r->d_de_rho, (size_t)r->FB));
    const size_t FB = (size_t)r->FB, n = (size_t)levels * FB;
    float4* const L = r->d_ds_lev;
    float4* const Lp = r->d_ds_lev + (size_t)r->ds_levels * FB;
    double* const partial = r->d_ds_sum + (size_t)r->ds_levels * FB;
    double* const res = partial + (size_t)DE_SUMS * ERR_BLOCKS;
    float* const maps[3] = {r->d_ds_map, r->d_ds_map + (size_t)r->ds_levels * FB, r->d_ds_map + 2 * (size_t)r->ds_levels * FB};
    if (!dst) dst = r->d_ds_out;
    hipStream_t st = r->stream;
    // cl2_denoise's passes, every one into the next level's float4 buffer
    auto passes = [&](float4* lev) { return denoise_passes(r, iterations, sigma_color, sigma_depth, sigma_albedo, LevelChain{lev, FB}); };
    const int blocks = grid_for(FB);
    hipLaunchKernelGGL(k_de_input, dim3(blocks), dim3(BLOCK), 0, st, r->FB, 0, (const float*)r->d_acc, (const float*)r->d_mom, L,
                       r->d_ds_a, (float*)nullptr);
    HIP_TRY(r, hipGetLastError());
    TRY(passes(L));
    HIP_TRY(r, hipMemsetAsync(r->d_ds_sum, 0, n * sizeof(double), st));
    if (model == 2) TRY(launch_de_rho(r, st));
    for (int k = 0; k < probes; k++) {
        launch_de_perturb(r, st, model, seed + (uint32_t)k, epsilon, K, (const float4*)L, (const float4*)r->d_ds_a, Lp, (float*)nullptr);
        HIP_TRY(r, hipGetLastError());
        TRY(passes(Lp));
        hipLaunchKernelGGL(k_ds_terms, dim3((unsigned)((FB + 255) / 256)), dim3(256), 0, st, r->FB, levels, (const float4*)L,
                           (const float4*)Lp, r->d_ds_sum);
        HIP_TRY(r, hipGetLastError());
    }
    const double scale = ((double)epsilon * (double)epsilon) * (double)probes;
    hipLaunchKernelGGL(k_ds_map, dim3((unsigned)((FB + 255) / 256)), dim3(256), 0, st, r->FB, levels, (const float4*)L,
                       (const float4*)r->d_ds_a, (const double*)r->d_ds_sum, scale, maps[0]);
    HIP_TRY(r, hipGetLastError());
    const float* M = maps[0];
    for (int s = 0; s < smooth_passes; s++) {
        float* const to = maps[1 + (s & 1)];
        hipLaunchKernelGGL(k_ds_smooth, dn_tiles(r), DN_BLOCK, 0, st, r->W, r->H, levels, 1 << s, sigma_depth, sigma_albedo * sigma_albedo, M, (const float4*)r->d_g0,
                           (const float4*)r->d_g1, (const float4*)r->d_ds_a, to);
        HIP_TRY(r, hipGetLastError());
        M = to;
    }
    const int grid = std::min(blocks, ERR_BLOCKS);
    hipLaunchKernelGGL(k_ds_select, dim3(grid), dim3(256), 0, st, r->FB, levels, (const float4*)L, (const float4*)r->d_ds_a, M, floor,
                       r->d_ds_scale, dst, partial);
    hipLaunchKernelGGL(k_de_final, dim3(1), dim3(256), 0, st, (const double*)partial, grid, res);
    HIP_TRY(r, hipGetLastError());
    if (maps_out) *maps_out = M;
    return drain(r);
}
}  // namespace

int cl2_ext_version(void) { return 1; }

namespace {
int denoise_select_call(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo, int probes,
                        float epsilon, int model, bool legacy, uint32_t seed, int smooth_passes, double floor, float* out_bgr,
                        size_t n_floats, int32_t* out_scale, size_t n_scale, double* out, float* out_maps, size_t n_maps,
                        float* out_levels, size_t n_levels) {
    STAGE_PROLOGUE(r);
    if (!out) return fail(r, CL2_E_INVALID, "NULL output");
    if (iterations < 1 || iterations > 12) return fail(r, CL2_E_INVALID, "scale selection: iterations must be in 1..12");
    const size_t FB = (size_t)r->FB, levels = (size_t)iterations + 1;
    if (out_bgr ? n_floats != 3 * FB : n_floats != 0) return fail(r, CL2_E_INVALID, "the selected picture must hold 3*W*H floats (or be NULL with n_floats 0)");
    if (out_scale ? n_scale != FB : n_scale != 0) return fail(r, CL2_E_INVALID, "the scale map must hold W*H int32 (or be NULL with n_scale 0)");
    if (out_maps ? n_maps != 2 * levels * FB : n_maps != 0)
        return fail(r, CL2_E_INVALID, "the maps must hold 2*(iterations+1)*W*H floats (or be NULL with n_maps 0)");
    if (out_levels ? n_levels != 6 * levels * FB : n_levels != 0)
        return fail(r, CL2_E_INVALID, "the levels must hold 2*(iterations+1)*3*W*H floats (or be NULL with n_levels 0)");
    const float* M = nullptr;
    TRY(run_select(r, iterations, sigma_color, sigma_depth, sigma_albedo, probes, epsilon, model, legacy, seed, smooth_passes, floor, nullptr, &M));
    const double* res = r->d_ds_sum + (size_t)r->ds_levels * FB + (size_t)DE_SUMS * ERR_BLOCKS;
    HIP_TRY(r, hipMemcpy(out, res, 8 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_bgr) HIP_TRY(r, hipMemcpy(out_bgr, r->d_ds_out, 3 * FB * sizeof(float), hipMemcpyDeviceToHost));
    if (out_scale) HIP_TRY(r, hipMemcpy(out_scale, r->d_ds_scale, FB * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (out_maps) {
        HIP_TRY(r, hipMemcpy(out_maps, r->d_ds_map, levels * FB * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(r, hipMemcpy(out_maps + levels * FB, M, levels * FB * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (out_levels) {
        // the levels are float4 buffers: their colours go out through d_ds_out, once the picture has left it
        for (size_t k = 0; k < 2 * levels; k++) {
            const float4* src = r->d_ds_lev + ((k / levels) * (size_t)r->ds_levels + k % levels) * FB;
            hipLaunchKernelGGL(k_de_pack, dim3(grid_for(FB)), dim3(BLOCK), 0, r->stream, r->FB, src, r->d_ds_out);
            HIP_TRY(r, hipGetLastError());
            HIP_TRY(r, hipStreamSynchronize(r->stream));
            HIP_TRY(r, hipMemcpy(out_levels + k * 3 * FB, r->d_ds_out, 3 * FB * sizeof(float), hipMemcpyDeviceToHost));
        }
    }
    return CL2_OK;
}

int keep_selected_call(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo, int probes,
                       float epsilon, int model, bool legacy, uint32_t seed, int smooth_passes) {
    STAGE_PROLOGUE(r);
    TRY(drain(r));
    // the totals are formed with floor 0 and stay on the device: only the picture is kept
    return keep_into_picture(r, 8, [&](float* pic) {
        return run_select(r, iterations, sigma_color, sigma_depth, sigma_albedo, probes, epsilon, model, legacy, seed, smooth_passes, 0.0, pic,
                          nullptr);
    });
}
}  // namespace

int cl2_denoise_select(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo, int probes,
                       float epsilon, int correlated, uint32_t seed, int smooth_passes, double floor, float* out_bgr, size_t n_floats,
                       int32_t* out_scale, size_t n_scale, double* out, float* out_maps, size_t n_maps, float* out_levels,
                       size_t n_levels) {
    return denoise_select_call(r, iterations, sigma_color, sigma_depth, sigma_albedo, probes, epsilon, correlated, true, seed,
                               smooth_passes, floor, out_bgr, n_floats, out_scale, n_scale, out, out_maps, n_maps, out_levels, n_levels);
}

int cl2_keep_selected_picture(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo, int probes,
                              float epsilon, int correlated, uint32_t seed, int smooth_passes) {
    return keep_selected_call(r, iterations, sigma_color, sigma_depth, sigma_albedo, probes, epsilon, correlated, true, seed, smooth_passes);
}

// ---------------------------------------------------------------- the split noise model (csrc/error_split.hpp; declared
// in include/clive2_amd_ext.h)
int cl2_ext_features(void) { return 1; }

int cl2_denoise_error_model(cl2_renderer* r, int kind, int iterations, float sigma, float sigma_depth, float sigma_albedo, int probes,
                            float epsilon, int noise_model, uint32_t seed, double floor, double* out, float* out_map, size_t n_map,
                            float* out_probe, size_t n_probe) {
    return run_denoise_error(r, kind, iterations, sigma, sigma_depth, sigma_albedo, probes, epsilon, noise_model, false, seed, floor, out,
                             out_map, n_map, out_probe, n_probe);
}

int cl2_denoise_select_model(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo, int probes,
                             float epsilon, int noise_model, uint32_t seed, int smooth_passes, double floor, float* out_bgr,
                             size_t n_floats, int32_t* out_scale, size_t n_scale, double* out, float* out_maps, size_t n_maps,
                             float* out_levels, size_t n_levels) {
    return denoise_select_call(r, iterations, sigma_color, sigma_depth, sigma_albedo, probes, epsilon, noise_model, false, seed,
                               smooth_passes, floor, out_bgr, n_floats, out_scale, n_scale, out, out_maps, n_maps, out_levels, n_levels);
}

int cl2_keep_selected_picture_model(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo,
                                    int probes, float epsilon, int noise_model, uint32_t seed, int smooth_passes) {
    return keep_selected_call(r, iterations, sigma_color, sigma_depth, sigma_albedo, probes, epsilon, noise_model, false, seed,
                              smooth_passes);
}

int cl2_set_split_tracking(cl2_renderer* r, int on) {
    if (!r) return CL2_E_INVALID;
    if (on != 0 && on != 1) return fail(r, CL2_E_INVALID, "split tracking: 0 off, 1 on");
    if (on && r->density)
        return fail(r, CL2_E_STATE, "split tracking and a sample density exclude each other (no mapped form): cl2_set_sample_density(NULL) first");
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    if (!on) {
        dev_free(r, r->d_smom);
        r->smom_valid = false;
        return CL2_OK;
    }
    if (r->d_smom) return CL2_OK;
    return side_sum_on(r, r->d_smom, (size_t)SPLIT_ROWS * (size_t)r->FB, r->smom_valid, "split rows");
}

int cl2_get_split_tracking(const cl2_renderer* r) { return r ? (r->d_smom ? 1 : 0) : CL2_E_INVALID; }

int cl2_read_split_moments_packed(cl2_renderer* r, float* dst, size_t n_floats) {
    if (!r || !dst) return CL2_E_INVALID;
    if (n_floats != (size_t)SPLIT_ROWS * (size_t)r->FB) return fail(r, CL2_E_INVALID, "packed split moments hold 6*W*H floats");
    TRY(need_split_rows(r));
    return packed_copy(r, dst, r->d_smom, n_floats, hipMemcpyDeviceToHost);
}

int cl2_write_split_moments_packed(cl2_renderer* r, const float* src, size_t n_floats) {
    if (!r || !src) return CL2_E_INVALID;
    if (n_floats != (size_t)SPLIT_ROWS * (size_t)r->FB) return fail(r, CL2_E_INVALID, "packed split moments hold 6*W*H floats");
    if (!r->d_smom) return fail(r, CL2_E_STATE, "split tracking is off (cl2_set_split_tracking)");
    TRY(packed_copy(r, r->d_smom, src, n_floats, hipMemcpyHostToDevice));
    r->smom_valid = true;
    return CL2_OK;
}

int cl2_light_share(cl2_renderer* r, float* out_map, size_t n_map, double* out) {
    if (!r || !out) return CL2_E_INVALID;
    const size_t FB = (size_t)r->FB;
    if (out_map ? n_map != FB : n_map != 0) return fail(r, CL2_E_INVALID, "the light-share map must hold W*H floats (or be NULL with n_map 0)");
    TRY(need_moments(r));
    TRY(need_split_rows(r));
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    if (!r->d_err_partial) TRY(dev_alloc(r, &r->d_err_partial, (size_t)3 * ERR_BLOCKS + 4));
    if (out_map && !r->d_de_rho) TRY(dev_alloc(r, &r->d_de_rho, FB));
    const int grid = std::min(grid_for(FB), ERR_BLOCKS);
    double* res = r->d_err_partial + 3 * ERR_BLOCKS;
    hipLaunchKernelGGL(k_light_share_partial, dim3(grid), dim3(256), 0, r->stream, r->FB, (const float*)r->d_acc, (const float*)r->d_mom,
                       (const float*)r->d_smom, out_map ? r->d_de_rho : (float*)nullptr, r->d_err_partial);
    hipLaunchKernelGGL(k_light_share_final, dim3(1), dim3(256), 0, r->stream, (const double*)r->d_err_partial, grid, res);
    HIP_TRY(r, hipGetLastError());
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipMemcpy(out, res, 4 * sizeof(double), hipMemcpyDeviceToHost));
    if (out_map) HIP_TRY(r, hipMemcpy(out_map, r->d_de_rho, FB * sizeof(float), hipMemcpyDeviceToHost));
    return CL2_OK;
}

int cl2_write_picture(cl2_renderer* r, const float* bgr, size_t n_floats) {
    if (!r || !bgr) return CL2_E_INVALID;
    if (n_floats != 3 * (size_t)r->FB) return fail(r, CL2_E_INVALID, "the kept picture holds 3*W*H floats");
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    if (!r->d_pic) TRY(dev_alloc(r, &r->d_pic, n_floats));
    r->pic_kind = 0;
    HIP_TRY(r, hipMemcpy(r->d_pic, bgr, n_floats * sizeof(float), hipMemcpyHostToDevice));
    r->pic_kind = 5;
    return CL2_OK;
}

int cl2_read_picture(cl2_renderer* r, float* out_bgr, size_t n_floats) {
    if (!r || !out_bgr) return CL2_E_INVALID;
    if (n_floats != 3 * (size_t)r->FB) return fail(r, CL2_E_INVALID, "the kept picture holds 3*W*H floats");
    TRY(need_picture(r));
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    HIP_TRY(r, hipMemcpy(out_bgr, r->d_pic, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return CL2_OK;
}

int cl2_picture_log_sum(cl2_renderer* r, double* sum_out) {
    if (!r || !sum_out) return CL2_E_INVALID;
    TRY(need_picture(r));
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    TRY(tone_buffers(r));
    const int grid = std::min(grid_for(r->FB), TONE_BLOCKS);
    hipLaunchKernelGGL(k_picture_logsum, dim3(grid), dim3(256), 0, r->stream, (const float*)r->d_pic, r->FB, r->d_tone_partial);
    hipLaunchKernelGGL(k_tone_logsum_final, dim3(1), dim3(256), 0, r->stream, r->d_tone_partial, grid, r->d_tone_partial + TONE_BLOCKS);
    HIP_TRY(r, hipGetLastError());
    HIP_TRY(r, hipMemcpyAsync(sum_out, r->d_tone_partial + TONE_BLOCKS, sizeof(double), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    return CL2_OK;
}

int cl2_picture_tone_map(cl2_renderer* r, double exposure, double white_point, double log_average, uint8_t* out_bgr, size_t n_bytes) {
    if (!r || !out_bgr) return CL2_E_INVALID;
    if (n_bytes != (size_t)3 * r->FB) return fail(r, CL2_E_INVALID, "the tone-mapped picture holds 3*W*H bytes");
    TRY(need_picture(r));
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    TRY(tone_buffers(r));
    const size_t quads = (n_bytes + 3) / 4;                       // four values per thread (k_picture_apply)
    hipLaunchKernelGGL(k_picture_apply, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, r->stream, (const float*)r->d_pic, n_bytes,
                       (float)exposure, white_point * white_point, log_average, r->d_tone_out);
    HIP_TRY(r, hipGetLastError());
    HIP_TRY(r, hipMemcpyAsync(out_bgr, r->d_tone_out, n_bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    return CL2_OK;
}

int cl2_relative_error(cl2_renderer* r, double floor, double* out) {
    if (!r || !out) return CL2_E_INVALID;
    if (!(floor >= 0.0) || !std::isfinite(floor)) return fail(r, CL2_E_INVALID, "floor must be >= 0 and finite");
    TRY(need_moments(r));
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    return eval_rel_error(r, floor, out);
}

int cl2_run_until(cl2_renderer* r, double target, double floor, int min_passes, int max_passes, int check_every, int* passes_done,
                  double* error_out) {
    if (!r) return CL2_E_INVALID;
    if (passes_done) *passes_done = 0;
    if (!(target > 0.0) || !std::isfinite(target)) return fail(r, CL2_E_INVALID, "target must be > 0 and finite");
    if (!(floor >= 0.0) || !std::isfinite(floor)) return fail(r, CL2_E_INVALID, "floor must be >= 0 and finite");
    if (check_every < 1) return fail(r, CL2_E_INVALID, "check_every must be >= 1");
    if (max_passes < 1 || min_passes < 0 || min_passes > max_passes) return fail(r, CL2_E_INVALID, "need 0 <= min_passes <= max_passes, max_passes >= 1");
    if (r->adaptive && (long long)min_passes * r->streams < 2)
        return fail(r, CL2_E_INVALID, "adaptive sampling needs two addends per pixel before its first update: min_passes * streams >= 2");
    STAGE_PROLOGUE(r);
    TRY(need_moments(r));
    if (r->adaptive) TRY(no_comm(r));
    if (r->adaptive && r->d_smom) return fail(r, CL2_E_STATE, "adaptive sampling and split tracking exclude each other (no mapped form): cl2_set_split_tracking(0) first");
    int done = 0;
    double e = std::numeric_limits<double>::infinity();
    bool evaluated = false;
    if (min_passes > 0) {
        TRY(cl2_run_samples(r, min_passes));
        done = min_passes;
        if (passes_done) *passes_done = done;
    }
    while (done < max_passes) {
        const int chunk = std::min(check_every, max_passes - done);
        if (r->adaptive) TRY(dens_update(r, floor, r->adaptive_share));
        TRY(cl2_run_samples(r, chunk));
        done += chunk;
        if (passes_done) *passes_done = done;
        TRY(eval_rel_error(r, floor, &e));
        evaluated = true;
        if (e <= target) break;
    }
    if (!evaluated) TRY(eval_rel_error(r, floor, &e));
    if (error_out) *error_out = e;
    return CL2_OK;
}

// ---------------------------------------------------------------- adaptive sampling (csrc/adaptive.hpp)
int cl2_set_sample_density(cl2_renderer* r, const float* density, size_t n) {
    if (!r) return CL2_E_INVALID;
    TRY(no_comm(r));
    if (density && r->n_layers > 0) return fail(r, CL2_E_STATE, "a sample density and layer accumulators exclude each other (no mapped form): cl2_set_layers(NULL, 0) first");
    if (density && r->d_smom) return fail(r, CL2_E_STATE, "a sample density and split tracking exclude each other (no mapped form): cl2_set_split_tracking(0) first");
    if (density) {
        if (n != (size_t)r->FB) return fail(r, CL2_E_INVALID, "the density holds W*H weights");
        for (size_t i = 0; i < n; i++)
            if (!(density[i] > 0.0f) || !std::isfinite(density[i])) return fail(r, CL2_E_INVALID, "density weights must be positive and finite");
    }
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    if (!density) { free_density(r); return CL2_OK; }
    TRY(ensure_density_buffers(r));
    HIP_TRY(r, hipMemcpy(r->d_dens_m, density, n * sizeof(float), hipMemcpyHostToDevice));
    return dens_quantise(r);
}

int cl2_read_sample_density(cl2_renderer* r, float* out, size_t n) {
    if (!r || !out) return CL2_E_INVALID;
    if (n != (size_t)r->FB) return fail(r, CL2_E_INVALID, "the density holds W*H weights");
    if (!r->density) { for (size_t i = 0; i < n; i++) out[i] = 1.0f; return CL2_OK; }
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    std::vector<uint64_t> c(n);
    HIP_TRY(r, hipMemcpy(c.data(), r->d_dens_C, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) out[i] = (float)((double)(c[i] - (i ? c[i - 1] : 0)) / 65536.0);
    return CL2_OK;
}

int cl2_update_sample_density(cl2_renderer* r, double floor, double uniform_share) {
    if (!r) return CL2_E_INVALID;
    if (!(floor >= 0.0) || !std::isfinite(floor)) return fail(r, CL2_E_INVALID, "floor must be >= 0 and finite");
    if (!(uniform_share > 0.0 && uniform_share <= 1.0)) return fail(r, CL2_E_INVALID, "uniform_share must be in (0, 1]");
    TRY(no_comm(r));
    if (r->n_layers > 0) return fail(r, CL2_E_STATE, "a sample density and layer accumulators exclude each other (no mapped form): cl2_set_layers(NULL, 0) first");
    if (r->d_smom) return fail(r, CL2_E_STATE, "a sample density and split tracking exclude each other (no mapped form): cl2_set_split_tracking(0) first");
    TRY(need_moments(r));
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    return dens_update(r, floor, uniform_share);
}

int cl2_set_adaptive_sampling(cl2_renderer* r, int on, double uniform_share) {
    if (!r) return CL2_E_INVALID;
    if (on != 0 && on != 1) return fail(r, CL2_E_INVALID, "adaptive sampling: 0 off, 1 on");
    if (on && !(uniform_share > 0.0 && uniform_share <= 1.0)) return fail(r, CL2_E_INVALID, "uniform_share must be in (0, 1]");
    if (on) TRY(no_comm(r));
    if (on && r->n_layers > 0) return fail(r, CL2_E_STATE, "adaptive sampling and layer accumulators exclude each other (no mapped form): cl2_set_layers(NULL, 0) first");
    r->adaptive = on != 0;
    if (on) r->adaptive_share = uniform_share;
    return CL2_OK;
}
int cl2_get_adaptive_sampling(const cl2_renderer* r) { return r ? (r->adaptive ? 1 : 0) : CL2_E_INVALID; }

int cl2_read_camera_samples(cl2_renderer* r, float* out, size_t n) {
    if (!r || !out) return CL2_E_INVALID;
    if (n != (size_t)r->FB) return fail(r, CL2_E_INVALID, "the camera sample counts hold W*H entries");
    HIP_TRY(r, hipSetDevice(r->device));
    TRY(drain(r));
    std::vector<unsigned> c(n, 0u);
    if (r->d_cam_count) HIP_TRY(r, hipMemcpy(c.data(), r->d_cam_count, n * sizeof(unsigned), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) out[i] = (float)((uint64_t)c[i] + r->cam_uniform);
    return CL2_OK;
}

}  // extern "C"
