// connect_resolve.hpp -- MIS weights and contributions of every (t,s) strategy pair of one pixel.
//
// Reference: the strategy loop of `connect_paths` (src/trace.metal:649-825) with its two BVH
// queries replaced by the results of k_traverse_conn, the filter-weight epilogue (:827-868), the
// light-image gather K8 (:937-964, here a float-atomic splat) and the unidirectional estimate of
// `generate_paths` (:523-528).
//
// Formulation.  For a pair (t,s) the unified path is x_0..x_k, k = s+t-1, x_i = light[i] for i < s
// and camera[t+s-i-1] otherwise (get_ray, :546-549).  The reference rebuilds all k+1 pdf ratios
//     r_0 = l_0 / (c_0 G_01)      r_i = (l_i G_{i-1,i}) / (c_i G_{i,i+1})      r_k = (l_k G_{k,k-1}) / c_k
// for every pair (:709-735).  All but the (at most) two ratios that touch the connection edge
// depend on one subpath only, so they are evaluated ONCE per pixel with exactly the reference's
// operations -- RL[i] for the light side, RC[m] for the camera side -- and each pair only computes
// the junction geometry term, the two junction ratios and the two running products (:745-755).
// Same float operations on the same operands in the same order => the aggregator is reproduced
// exactly; per-pixel divisions drop from ~400 to ~250 and every path vertex is read from HBM once
// (light subpath: registers, statically indexed because the s-loop is unrolled) or twice (camera).
#pragma once
#include "vecmath.hpp"
#include "bsdf.hpp"
#include "scene_layout.hpp"

namespace cl2 {

// Is triangle i one of the camera quad's (CamTris, scene_layout.hpp)?
__device__ __forceinline__ bool is_camera_tri(const CamTris& ct, const float4* __restrict__ tri_shade, int i) {
    if (ct.n < 0) return __float_as_int(tri_shade[4 * i + 2].w) != 0;
    bool hit = false;
#pragma unroll
    for (int k = 0; k < CAM_TRI_ARGS; k++) hit = hit || (k < ct.n && i == ct.idx[k]);
    return hit;
}

struct LightVtx {          // the part of a light vertex every pair touches: registers
    V3 o;
    float c, l, tot, cosv;
    int tri, meta;
};
// Normal and colour of the light vertices are read once per contributing pair only: they live in LDS
// ([word][thread], conflict-free) so the kernel fits 3 waves per SIMD instead of 2.
__device__ __forceinline__ V3 lds_v3(const float* base, int v) {
    return v3(base[(3 * v + 0) * BLOCK + threadIdx.x], base[(3 * v + 1) * BLOCK + threadIdx.x], base[(3 * v + 2) * BLOCK + threadIdx.x]);
}

// Layer accumulators (cl2_set_layers, layers.hpp): the handle's table as the resolve kernel takes it, by value.  Pair (s, t) has a
// 4-bit code at bits 4 s .. 4 s + 3 of the 32-bit row of t: 0 = in no layer, l + 1 = in layer l.  Rows t = 1, 2 are the halves of
// w[0], rows 3, 4 of w[1], rows 5, 6 of w[2] -- chosen with selects, so the argument is only ever indexed by constants.
constexpr int LAYERS_MAX = 8;              // CL2_MAX_LAYERS (include/clive2_amd.h)
struct LayerCodes {
    unsigned long long w[3];
    int n_layers;
};
__device__ __forceinline__ unsigned layer_row(const LayerCodes& lc, int t) {
    const unsigned long long w = (t <= 2) ? lc.w[0] : ((t <= 4) ? lc.w[1] : lc.w[2]);
    return (unsigned)(w >> (((t - 1) & 1) * 32));
}
// `code` is the same in every lane of the wave (S is a template parameter and the lanes run the t loop in lockstep): a scalar
// switch picks the registers, there is no register array indexed by a lane value.
__device__ __forceinline__ void layer_add(V3 (&lt)[LAYERS_MAX], unsigned code, const V3& term) {
    switch (code) {
        case 1: lt[0] = lt[0] + term; break;
        case 2: lt[1] = lt[1] + term; break;
        case 3: lt[2] = lt[2] + term; break;
        case 4: lt[3] = lt[3] + term; break;
        case 5: lt[4] = lt[4] + term; break;
        case 6: lt[5] = lt[5] + term; break;
        case 7: lt[6] = lt[6] + term; break;
        case 8: lt[7] = lt[7] + term; break;
        default: break;
    }
}

// One strategy pair with s = S (compile time).  Returns true when a contribution was produced.
// DET (cl2_set_reproducible): a t = 1 contribution is not added to the light image with float atomics but WRITTEN as a record
// {target pixel, source slot} / {c.xyz, w} at slot (S-1) * B + pid -- the reference's own scatter `id + s * total_pixels`
// (trace.metal:817-823) -- and summed per target pixel in a fixed order afterwards (det_splat.hpp).
// STRAT (cl2_set_strategy_mask): `srow` holds the strategy bits of this t, bit S = pair (S, t).  A pair whose bit is clear is
// evaluated exactly as before -- culls, verdict, MIS weight w, and w goes where it always goes -- but its COLOUR is left out: the
// `total +=` statement is not executed, and the t = 1 splat or record carries (+0, +0, +0) with its w.  No reference counterpart
// (trace.metal:649-825 sums all pairs).  STRAT = false is the kernel as it was: `srow` is not read.
// LAYERS (cl2_set_layers): everything is computed as with STRAT = false; in addition the colour term of a t >= 2 or s = 0 pair --
// the very value added to `total`, computed once -- is added to the running total `ltot` of the pair's layer (code `lrow >> 4 S`),
// in the kernel's pair order, which is the sequence of additions the masked kernel performs for that layer's mask; a t = 1 pair
// with atomics also adds its colour to lay_light[layer][entry] (the records of DET need nothing: a record's slot names its pair).
// LAYERS = false: `lrow`, `ltot` and `lay_light` are not read.
// SLIM (k_connect_resolve_slim below): a light vertex's `tri` word holds {triangle << 8 | material byte} (its `meta` is not kept:
// the pairs read the material byte of a light vertex and nothing else of it), and the LDS rows that no pair reads -- the normal of
// light vertex 0, the colour of light vertex 5 -- do not exist: row v of LNs is vertex v + 1.  TK: what is known of t at compile
// time -- 0 nothing, 1 t == 1, 2 t >= 2 (the slim kernel peels t = 1 out of its t loop; `h.y` is then only carried where it is read).
template <int S, bool DET, bool STRAT, bool LAYERS = false, bool SLIM = false, int TK = 0>
__device__ __forceinline__ void resolve_pair(
        int t, int B, int pid, const LightVtx (&lv)[MAX_VERTS], const float (&GL)[MAX_VERTS], const float (&RL)[MAX_VERTS],
        unsigned l_spec, unsigned c_spec, bool spec7,
        // camera junction vertex t-1 and per-path camera tables (LDS)
        V3 c_o_in, V3 c_n_in, float c_c, float c_l, float c_tot_in, float c_cos_in, int c_tri, int c_meta,
        V3 prior_camera_color, const float* GCs, const float* RCs /* [m*BLOCK + tid] */, const float* LNs, const float* LCs,
        unsigned long long mask, float2 h, const float4* __restrict__ tri_shade, const CamTris& cam_tris,
        const MaterialDev* __restrict__ mats, const CameraRec& cam, V3 focal, V3 cam_dir,
        V3& total, float& contrib_weight_sum, float4* __restrict__ light_image, float* splat_tab, int debug_flags,
        unsigned* __restrict__ det_keys, float4* __restrict__ det_vals, [[maybe_unused]] unsigned srow,
        [[maybe_unused]] unsigned lrow, [[maybe_unused]] V3 (&ltot)[LAYERS_MAX], [[maybe_unused]] float4* __restrict__ lay_light) {
    const int tid = threadIdx.x;
    const bool t_is_1 = (TK == 0) ? (t == 1) : (TK == 1);
    constexpr int LN_OFF = SLIM ? 1 : 0;                                      // first light vertex with a row in LNs
    auto lv_tri = [](const LightVtx& x) -> int { return SLIM ? resolve_packed_tri(x.tri) : x.tri; };
    auto lv_mat = [](const LightVtx& x) -> int { return SLIM ? resolve_packed_mat(x.tri) : (x.meta & 0xFF); };
    [[maybe_unused]] const unsigned lcode = LAYERS ? ((lrow >> (4 * S)) & 15u) : 0u;     // wave-uniform
    bool keep = true;                                                         // this pair's colour is wanted
    if constexpr (STRAT) keep = (srow >> S) & 1u;
    V3 c_o = c_o_in, c_n = c_n_in;
    float c_tot = c_tot_in, c_cos = c_cos_in;
    V3 dir_l_to_c = v3(0, 0, 0);
    int light_pixel_idx = -1;
    float Gj = 0.0f;

    if (S == 0) {
        if (!(c_meta & META_HIT_LIGHT)) return;                               // :665
    } else {
        if (!((mask >> conn_slot(t, S)) & 1ull)) return;                      // culled in k_connect_setup
        const LightVtx& a = lv[S - 1];
        const int best_i = __float_as_int(h.x);
        if (best_i == -1) return;                                             // :193 / :593
        if (t_is_1) {
            // world_ray_to_camera_ray, :595-616
            if (!is_camera_tri(cam_tris, tri_shade, best_i)) return;         // !is_camera
            const V3 tdir = normalize(focal - a.o);
            const V3 camera_point = a.o + h.y * tdir;
            const float x = dot(camera_point - cam3(cam.center), cam3(cam.dx));
            const float y = dot(camera_point - cam3(cam.center), cam3(cam.dy));
            const int pixel_x = (int)__builtin_roundf((x / cam.phys_width + 0.5f) * cam.pixel_width);
            const int pixel_y = (int)__builtin_roundf((y / cam.phys_height + 0.5f) * cam.pixel_height);
            light_pixel_idx = pixel_y * cam.pixel_width + pixel_x;
            if (light_pixel_idx == -1) return;                                // :671
            c_o = camera_point;
            const V3 cdir = normalize(focal - camera_point);
            c_n = cam_dir;
            c_cos = __builtin_fabsf(dot(cdir, cam_dir));
            c_tot = 1.0f;
        } else {
            if (best_i == lv_tri(a)) return;                                  // visibility_test, :194-196
            if (best_i != c_tri) return;
        }
        dir_l_to_c = normalize(c_o - a.o);
        Gj = geom_term(a.cosv, c_cos, a.o, c_o);
    }

    // ---- p_s and the two running products (:737-757) ----
    const float p_s = c_tot * ((S == 0) ? 1.0f : lv[S > 0 ? S - 1 : 0].tot);
    // backward (light side): p[i] = p[i+1] / r_i for i = S-1 .. 0
    float pb[MAX_VERTS > 0 ? MAX_VERTS : 1];
    if (S > 0) {
        const LightVtx& a = lv[S - 1];
        const float r_junc = (S == 1) ? a.l / (a.c * Gj) : (a.l * GL[S - 2]) / (a.c * Gj);
        float v = p_s / r_junc;
        pb[S - 1] = v;
#pragma unroll
        for (int i = S - 2; i >= 0; i--) { v = v / RL[i]; pb[i] = v; }
    }
    // specular zeroing (:759-764): p[i] is zeroed when x_i or x_{i-1} is specular
    auto spec_at = [&](int i) -> bool {        // unified index -> material type > 0
        if (i < S) return (l_spec >> i) & 1u;
        const int m = t + S - i - 1;
        if (t_is_1 && S > 0) return spec7;       // projected camera vertex carries material 7 (:611)
        return (c_spec >> m) & 1u;
    };
    float sum = 0.0f;
    bool prev_spec = false;
#pragma unroll
    for (int i = 0; i < S; i++) {
        const bool sp = (l_spec >> i) & 1u;
        sum += (sp || prev_spec) ? 0.0f : pb[i];
        prev_spec = sp;
    }
    // i = S: p[S] = p_s
    bool sp_s = spec_at(S);
    const float p_at_s = (sp_s || prev_spec) ? 0.0f : p_s;
    sum += p_at_s;
    prev_spec = sp_s;
    // forward (camera side): p[i+1] = r_i * p[i], i = S .. S+t-2 useful (p[S+t] is overwritten by 0, :766)
    {
        float v = p_s;
        for (int i = S; i < S + t - 1; i++) {
            float r;
            if (i == S) {
                if (S == 0) r = c_l / (c_c * GCs[(t - 2) * BLOCK + tid]);            // i == 0 form, x_1 = camera[t-2]
                else r = (c_l * Gj) / (c_c * GCs[(t - 2) * BLOCK + tid]);           // interior form at the junction
            } else {
                r = RCs[(t + S - i - 1) * BLOCK + tid];
            }
            v = r * v;
            const bool sp = spec_at(i + 1);
            sum += (sp || prev_spec) ? 0.0f : v;
            prev_spec = sp;
        }
    }
    sum += 0.0f;                                                              // p[S+t] = 0
    if (!(p_at_s > 0.0f && sum > 0.0f)) return;                               // :773-776
    const float w = p_at_s / sum;

    if (S == 0) {                                                             // :783-786
        const V3 emission = v3(mats[c_meta & 0xFF].emission_alpha);
        const V3 color = prior_camera_color * emission;
        if constexpr (LAYERS) {
            const V3 term = ((w * 1.0f) * color) / p_s;
            total = total + term;
            layer_add(ltot, lcode, term);
        } else if (keep) total = total + ((w * 1.0f) * color) / p_s;
        contrib_weight_sum += w;
    } else if (t_is_1) {                                                      // :787-793, :817-823, K8 :952-961
        const LightVtx& a = lv[S - 1];
        const V3 prior_color = lds_v3(LCs, (S - 2) > 0 ? (S - 2) : 0);
        float new_light_f = 1.0f;
        if (S > 1) new_light_f = div_pi(__builtin_fabsf(dot(dir_l_to_c, lds_v3(LNs, S - 1 - LN_OFF))));
        const V3 mcol = v3(mats[lv_mat(a)].color_type);
        const float shade = new_light_f * Gj / p_s;
#ifdef CL2_TEST_VARIANT
        const bool splat_on = !(debug_flags & 1);          // timing dissection (test variant only): no splat = invalid render
#else
        const bool splat_on = true;
#endif
        const int frame_pixels = cam.pixel_width * cam.pixel_height;
        if (light_pixel_idx >= 0 && light_pixel_idx < frame_pixels && splat_on) {
            V3 c = ((w * shade) * prior_color) * mcol;
            if constexpr (STRAT) { if (!keep) c = v3(0, 0, 0); }
            // the light image of THIS entry's sample stream (computed here, in the rare branch, not carried through the kernel:
            // it runs at 162 of 168 VGPRs)
            const int splat_idx = (pid - pid % frame_pixels) + light_pixel_idx;
            if (DET) {
                const size_t rec = (size_t)(S > 0 ? S - 1 : 0) * B + pid;
                det_vals[rec] = make_float4(c.x, c.y, c.z, w);
                det_keys[rec] = (unsigned)splat_idx;
                return;
            }
            // Splat {c.xyz, w} into light_image[pixel] (float4).  The lanes that reach this point
            // exchange their 4 values through a per-wave LDS table so that four CONSECUTIVE lanes
            // add the four components of one pixel: each atomic wave-instruction then carries whole
            // 16-byte segments instead of 64 unrelated dwords (4x fewer memory-side requests).
            float* tab = splat_tab + (threadIdx.x >> 6) * (5 * 64);
            const unsigned long long here = __ballot(true);
            const int n_here = __popcll(here), k = __popcll(here & ((1ull << (threadIdx.x & 63)) - 1ull));
            tab[0 * 64 + k] = __int_as_float(splat_idx);
            tab[1 * 64 + k] = c.x; tab[2 * 64 + k] = c.y; tab[3 * 64 + k] = c.z; tab[4 * 64 + k] = w;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int item = k + j * n_here, slot = item >> 2, comp = item & 3;
                const int pix = __float_as_int(tab[slot]);
                const float val = tab[(1 + comp) * 64 + slot];
                atomicAdd(reinterpret_cast<float*>(&light_image[pix]) + comp, val);
                if constexpr (LAYERS) {
                    // the same exchange, so consecutive lanes still cover one pixel's components; the layer is the same in
                    // every lane of this branch.  pix < B (splat_idx above) and lcode - 1 < n_layers (the host's table).
                    if (lcode != 0u && comp < 3)
                        atomicAdd(reinterpret_cast<float*>(&lay_light[(size_t)(lcode - 1u) * B + pix]) + comp, val);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    } else {                                                                  // :794-816
        const LightVtx& a = lv[S - 1];
        const MaterialDev cmat = mats[c_meta & 0xFF];
        const float new_camera_f = div_pi(__builtin_fabsf(dot(-dir_l_to_c, c_n)));
        const V3 camera_color = (prior_camera_color * new_camera_f) * v3(cmat.color_type);
        V3 light_color;
        if (S == 1) light_color = v3(mats[lv_mat(a)].emission_alpha);
        else {
            const V3 prior_light_color = lds_v3(LCs, S >= 2 ? S - 2 : 0);
            const float new_light_f = div_pi(__builtin_fabsf(dot(dir_l_to_c, lds_v3(LNs, S - 1 - LN_OFF))));
            light_color = (prior_light_color * new_light_f) * v3(mats[lv_mat(a)].color_type);
        }
        const V3 color = camera_color * light_color;
        if constexpr (LAYERS) {
            const V3 term = ((w * Gj) * color) / p_s;
            total = total + term;
            layer_add(ltot, lcode, term);
        } else if (keep) total = total + ((w * Gj) * color) / p_s;
        contrib_weight_sum += w;
    }
}

// MAPPED (adaptive sampling, adaptive.hpp): the pixel of the filter weights is the slot map's map[pid] instead of pid % (W*H);
// nothing else in the kernel takes an image pixel from a slot (the t = 1 splat takes only its plane base from it).
// STRAT: `strat` is the handle's strategy mask, bit (t - 1) * 7 + s for pair (s, t) (include/clive2_amd.h); launched only when the
// mask is partial.  With STRAT = false the argument is not read.
// LAYERS: `lcodes` is the handle's layer table; the layer totals go to lay_agg[l][3][B] (the stride of the aggregator rows) for
// l < lcodes.n_layers, everything else is written as with STRAT = false.  Launched only while a table is set, only with
// MAPPED = false and STRAT = false, at two waves per SIMD: the 24 layer totals are registers (3 waves leave 168, the kernel
// alone takes 163).  With LAYERS = false the three arguments are not read.
#define CL2_RESOLVE_PARAMS                                                                                                         \
        int B, PathBufs lp, PathBufs cp, const MaterialDev* __restrict__ mats_g, int n_mats,                                        \
        const float4* __restrict__ tri_shade, CamTris cam_tris, CameraRec cam, const unsigned long long* __restrict__ cmask,        \
        const float2* __restrict__ chit, float* __restrict__ agg, float4* __restrict__ light_image,                                 \
        float4* __restrict__ uni_out, Stats* stats, int debug_flags,                                                                \
        unsigned* __restrict__ det_keys, float4* __restrict__ det_vals, const int* __restrict__ map,                                \
        [[maybe_unused]] unsigned long long strat, [[maybe_unused]] LayerCodes lcodes, [[maybe_unused]] float* __restrict__ lay_agg, \
        [[maybe_unused]] float4* __restrict__ lay_light

template <int WAVES_PER_SIMD, bool MATS_LDS, bool DET = false, bool MAPPED = false, bool STRAT = false, bool LAYERS = false>
__global__ __launch_bounds__(BLOCK, WAVES_PER_SIMD) void k_connect_resolve(CL2_RESOLVE_PARAMS) {
    constexpr bool SLIM = false;
#include "connect_resolve_body.hpp"
}

// The slim form: three waves per SIMD that leave room for a fourth wave of ANOTHER kernel.  A SIMD has 512 registers per lane and
// a CU 163,840 B of LDS; beside three of these workgroups one workgroup of k_trace_subpath<., false, false> (80 registers, 9,808 B
// static + the staged tree) fits when this kernel takes at most SLIM_VGPRS registers and (163,840 - L_subpath) / 3 bytes.
// Material table in LDS, no slot map, no strategy mask, no layers: every other combination runs k_connect_resolve.
constexpr int SLIM_VGPRS = 144;                    // 3 * 144 + 80 = 512
template <bool DET>
__global__ __launch_bounds__(BLOCK, 3) __attribute__((amdgpu_num_vgpr(SLIM_VGPRS))) void k_connect_resolve_slim(CL2_RESOLVE_PARAMS) {
    constexpr bool SLIM = true, MATS_LDS = true, MAPPED = false, STRAT = false, LAYERS = false;
#include "connect_resolve_body.hpp"
}
#undef CL2_RESOLVE_PARAMS

}  // namespace cl2
