// denoise.hpp -- first-hit feature buffers and an edge-avoiding a-trous filter over the accumulated radiance.
//
// No reference counterpart: the reference stops at the Monte Carlo estimate (src/renderer.py:293-316).  Everything here
// reads the handle's scene and accumulators and writes buffers of its own; the sample pipeline, its seeds, accumulators
// and counters never see it.
//
// Feature pass (cl2_render_features), per pixel p of the W x H frame, `samples` times:
//   k_feat_rays    the camera ray of camera_ray() (kernels.hpp) from a private copy of the caller's seed buffer; sample k
//                  continues the xorshift state sample k-1 left, so with one sample the rays are the bytes
//                  cl2_make_camera_rays makes from the same seeds
//   closest hit    k_traverse_paths<false> / the 4-wide walk, into a private ray tally (renderer_api.hip)
//   k_feat_shade   G0 += (shading normal facing the ray, t), G1 += (material colour b, g, r, 1) for a hit
// then k_feat_finish turns the sums into
//   G0 = (normalize(sum n) or 0, mean depth)     G1 = (mean albedo b, g, r, coverage = hits / samples)
//
// Filter (cl2_denoise): c = scrub(acc_image / acc_weight) as Renderer.radiance computes it; `iterations` passes of the
// 5 x 5 B3-spline a-trous kernel at steps 1, 2, 4, ..., each tap weighted by the normals, depths and albedos of the two
// pixels and by the distance of their colours after x = c / (1 + luma(c)).  Pixels without coverage pass through, and so do
// pixels whose weight sum is not greater than 0 (NaN included); taps without coverage or outside the frame are skipped.  tests/denoise_reference.py restates every operation below in numpy, in
// the same order.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.hpp"

namespace cl2 {

constexpr int DN_TILE = 16;                   // filter workgroup: 16 x 16 pixels, one per thread

// ---------------------------------------------------------------- feature pass
__global__ __launch_bounds__(BLOCK) void k_feat_rays(int FB, CameraRec c, uint2* __restrict__ seeds, float4* __restrict__ O,
                                                     float4* __restrict__ D) {
    const int id = blockIdx.x * BLOCK + threadIdx.x;
    if (id >= FB) return;
    uint2 sd = seeds[id];
    uint32_t seed0 = sd.x, seed1 = sd.y;
    V3 o, d;
    camera_ray(id, c, seed0, seed1, o, d);
    O[id] = f4(o, 0.0f);
    D[id] = f4(d, 0.0f);
    seeds[id] = make_uint2(seed0, seed1);
}

// hit = {tri (int bits), t, u, v}; tri_shade = 4 float4 per triangle {n0, material}, {n1, is_light}, {n2, is_camera}, {normal}
__global__ __launch_bounds__(BLOCK) void k_feat_shade(int FB, const float4* __restrict__ D, const float4* __restrict__ hit,
                                                      const float4* __restrict__ tri_shade, const MaterialDev* __restrict__ mats,
                                                      float4* __restrict__ G0, float4* __restrict__ G1) {
    const int id = blockIdx.x * BLOCK + threadIdx.x;
    if (id >= FB) return;
    const float4 h = hit[id];
    const int tri = __float_as_int(h.x);
    if (tri < 0) return;                                                        // a miss adds nothing
    const float t = h.y, u = h.z, v = h.w;
    const float4 s0 = tri_shade[4 * tri], s1 = tri_shade[4 * tri + 1], s2 = tri_shade[4 * tri + 2], s3 = tri_shade[4 * tri + 3];
    const V3 rd = v3(D[id]);
    V3 sn = normalize((v3(s0) * (1 - u - v) + v3(s1) * u) + v3(s2) * v);       // as shade_and_bounce (kernels.hpp)
    if (dot(rd, v3(s3)) > 0.0f) sn = -sn;                                       // facing the ray
    const float4 col = mats[__float_as_int(s0.w)].color_type;
    float4 g0 = G0[id], g1 = G1[id];
    g0.x += sn.x; g0.y += sn.y; g0.z += sn.z; g0.w += t;
    g1.x += col.x; g1.y += col.y; g1.z += col.z; g1.w += 1.0f;
    G0[id] = g0;
    G1[id] = g1;
}

__global__ __launch_bounds__(BLOCK) void k_feat_finish(int FB, int samples, float4* __restrict__ G0, float4* __restrict__ G1) {
    const int id = blockIdx.x * BLOCK + threadIdx.x;
    if (id >= FB) return;
    float4 g0 = G0[id], g1 = G1[id];
    const float hits = g1.w;
    if (hits > 0.0f) {
        const V3 s = v3(g0);
        const V3 n = dot(s, s) > 0.0f ? normalize(s) : v3(0.0f, 0.0f, 0.0f);
        g0 = make_float4(n.x, n.y, n.z, g0.w / hits);
        g1 = make_float4(g1.x / hits, g1.y / hits, g1.z / hits, hits / (float)samples);
    }
    G0[id] = g0;
    G1[id] = g1;
}

// ---------------------------------------------------------------- the core every picture filter shares
// (denoise_guided.hpp, denoise_layers.hpp, denoise_error.hpp and denoise_select.hpp build on it; tests/*_reference.py restate it)

// Input colour: Renderer.radiance's arithmetic, row k of `rows` ([3][FB]: b, g, r sums) over the weight w of the pixel, non-finite
// values set to 0.
__device__ __forceinline__ void dn_input_colour(const float* __restrict__ rows, size_t FB, size_t p, float w, float (&c)[3]) {
    for (int k = 0; k < 3; k++) {
        const float x = rows[k * FB + p] / w;
        c[k] = isfinite(x) ? x : 0.0f;
    }
}

// pixel p of a packed (H, W, 3) picture
__device__ __forceinline__ void dn_store3(float* __restrict__ out3, size_t p, float b, float g, float r) {
    out3[3 * p] = b; out3[3 * p + 1] = g; out3[3 * p + 2] = r;
}

__device__ __forceinline__ V3 dn_compress(float4 c) {          // x = c / (1 + luma(c)), luma of camera.py (b, g, r weights)
    const float l = (c.x * 0.0722f + c.y * 0.7152f) + c.z * 0.2126f;
    const float d = 1.0f + l;
    return v3(c.x / d, c.y / d, c.z / d);
}

__device__ __forceinline__ float dn_pow32(float x) {            // five squarings: numpy restates them exactly
    x = x * x; x = x * x; x = x * x; x = x * x; return x * x;
}

// The feature edge-stop of a tap q seen from the centre (normal n, albedo a, depth zp): ((hh wn) wz) wa with hh = h(dx) h(dy),
// den_z = (sigma_depth * zp) * (float) step and den_a = sigma_albedo^2.  A filter multiplies its colour or luma term on last.
__device__ __forceinline__ float dn_feature_weight(float hh, V3 n, V3 a, float zp, float den_z, float den_a, float4 nq, float4 aq) {
    const float wn = dn_pow32(max_msl(0.0f, dot(n, v3(nq))));
    const float wz = expf(-fabsf(zp - nq.w) / den_z);
    const V3 da = a - v3(aq);
    const float wa = expf(-dot(da, da) / den_a);
    return ((hh * wn) * wz) * wa;
}

// Where a pass finds the features of the pixels around its own, (px + ox, py + oy).  LDS_STEP = 1 or 2: those of the workgroup's
// 16 x 16 pixels and of the halo of two steps around them are staged in LDS first and |ox|, |oy| <= 2 LDS_STEP; LDS_STEP = 0: every
// tap is two bounds-checked 16-byte global loads.  Staged entries outside the frame are 0: their coverage 0 skips them exactly as
// the bounds test of the global form does.
template <int LDS_STEP>
struct DnTile {
    static constexpr int T = LDS_STEP ? DN_TILE + 4 * LDS_STEP : 1;      // side of the staged tile
    int W, H, px, py;
    const float4 *G0, *G1;
    float4 *s_n, *s_a;                                                   // T * T entries each

    __device__ __forceinline__ int at(int ox, int oy) const {            // the staged index of a tap
        return ((int)threadIdx.y + 2 * LDS_STEP + oy) * T + (int)threadIdx.x + 2 * LDS_STEP + ox;
    }
    // by every thread of the workgroup, before any leaves: ends in the barrier
    __device__ __forceinline__ void stage() const {
        if constexpr (LDS_STEP != 0) {
            const int x0 = blockIdx.x * DN_TILE - 2 * LDS_STEP, y0 = blockIdx.y * DN_TILE - 2 * LDS_STEP;
            for (int k = threadIdx.y * DN_TILE + threadIdx.x; k < T * T; k += DN_TILE * DN_TILE) {
                const int gx = x0 + k % T, gy = y0 + k / T;
                if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                    const int q = gy * W + gx;
                    s_n[k] = G0[q]; s_a[k] = G1[q];
                } else {
                    s_n[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); s_a[k] = s_n[k];
                }
            }
            __syncthreads();
        }
    }
    // normal | depth and albedo | coverage of a tap ((0, 0): the centre); false: outside the frame, skipped
    __device__ __forceinline__ bool features(int ox, int oy, float4& n, float4& a) const {
        if constexpr (LDS_STEP != 0) {
            const int k = at(ox, oy);
            n = s_n[k]; a = s_a[k];
        } else {
            const int qx = px + ox, qy = py + oy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) return false;
            const int q = qy * W + qx;
            n = G0[q]; a = G1[q];
        }
        return true;
    }
    // the offset of tap d (-2 .. 2) of a pass at `step`: a staged pass runs at step = LDS_STEP
    __device__ __forceinline__ static int offset(int d, int step) { return d * (LDS_STEP ? LDS_STEP : step); }
};

// ---------------------------------------------------------------- filter
// Writes the float4 working buffer from the packed accumulators [8][FB] (image b, g, r | weight | ...), or the packed (H, W, 3)
// output when no pass follows.
__global__ __launch_bounds__(BLOCK) void k_denoise_input(int FB, const float* __restrict__ acc, float4* __restrict__ cout,
                                                         float* __restrict__ out3) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= FB) return;
    float c[3];
    dn_input_colour(acc, (size_t)FB, (size_t)p, acc[3 * (size_t)FB + p], c);
    if (out3) dn_store3(out3, (size_t)p, c[0], c[1], c[2]);
    else cout[p] = make_float4(c[0], c[1], c[2], 0.0f);
}

// k_denoise_pass and k_denoise_guided_pass (denoise_guided.hpp) keep bodies of their own, tile staging and tap weight written out:
// one body over an edge-stop policy, built on DnTile and dn_feature_weight, gives the same bits but was measured 1 - 4 % slower per
// launch on the MI355X in every form tried (profiles/r28_README.md), and so was sharing only the stager and the feature weight.
// The instructions are the same; their schedule is not.  k_layers_denoise_pass and k_ds_smooth do use the shared pieces.
//
// One a-trous pass at step `step` (= 2^i).  den_c = sigma_color^2 * 4^-i, den_a = sigma_albedo^2 (host-computed, float32).
// LDS_STEP = 1 or 2: the workgroup's 16 x 16 pixels and the halo of two steps around them are staged in LDS first (24^2 x 48 B
// = 27 KB at step 2); LDS_STEP = 0: every tap is three 16-byte global loads.  Staged entries outside the frame carry coverage 0,
// which skips them exactly as the bounds test of the global form does.
template <int LDS_STEP>
__global__ __launch_bounds__(DN_TILE * DN_TILE) void k_denoise_pass(int W, int H, int step, float den_c, float sigma_depth,
                                                                     float den_a, const float4* __restrict__ cin,
                                                                     const float4* __restrict__ G0, const float4* __restrict__ G1,
                                                                     float4* __restrict__ cout, float* __restrict__ out3) {
    constexpr int T = LDS_STEP ? DN_TILE + 4 * LDS_STEP : 1;
    __shared__ float4 s_c[T * T], s_n[T * T], s_a[T * T];
    const int lx = threadIdx.x, ly = threadIdx.y;
    const int px = blockIdx.x * DN_TILE + lx, py = blockIdx.y * DN_TILE + ly;
    if (LDS_STEP) {
        const int x0 = blockIdx.x * DN_TILE - 2 * LDS_STEP, y0 = blockIdx.y * DN_TILE - 2 * LDS_STEP;
        for (int k = ly * DN_TILE + lx; k < T * T; k += DN_TILE * DN_TILE) {
            const int gx = x0 + k % T, gy = y0 + k / T;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const int q = gy * W + gx;
                s_c[k] = cin[q]; s_n[k] = G0[q]; s_a[k] = G1[q];
            } else {
                s_c[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); s_n[k] = s_c[k]; s_a[k] = s_c[k];
            }
        }
        __syncthreads();
    }
    if (px >= W || py >= H) return;
    const int p = py * W + px;
    float4 cp, np_, ap;
    if (LDS_STEP) {
        const int k = (ly + 2 * LDS_STEP) * T + lx + 2 * LDS_STEP;
        cp = s_c[k]; np_ = s_n[k]; ap = s_a[k];
    } else {
        cp = cin[p]; np_ = G0[p]; ap = G1[p];
    }
    float o0 = cp.x, o1 = cp.y, o2 = cp.z;
    if (ap.w != 0.0f) {
        const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
        const V3 xp = dn_compress(cp), n = v3(np_), a = v3(ap);
        const float zp = np_.w;
        const float den_z = (sigma_depth * zp) * (float)step;
        float sw = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                float4 cq, nq, aq;
                if (LDS_STEP) {
                    const int k = (ly + (2 + dy) * LDS_STEP) * T + lx + (2 + dx) * LDS_STEP;
                    cq = s_c[k]; nq = s_n[k]; aq = s_a[k];
                } else {
                    const int qx = px + dx * step, qy = py + dy * step;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const int q = qy * W + qx;
                    cq = cin[q]; nq = G0[q]; aq = G1[q];
                }
                if (aq.w == 0.0f) continue;
                const float wn = dn_pow32(max_msl(0.0f, dot(n, v3(nq))));
                const float wz = expf(-fabsf(zp - nq.w) / den_z);
                const V3 da = a - v3(aq);
                const float wa = expf(-dot(da, da) / den_a);
                const V3 dxc = xp - dn_compress(cq);
                const float wc = expf(-dot(dxc, dxc) / den_c);
                const float w = ((((h[dx + 2] * h[dy + 2]) * wn) * wz) * wa) * wc;
                sw += w;
                s0 += w * cq.x; s1 += w * cq.y; s2 += w * cq.z;
            }
        }
        // A weight sum that is not greater than 0 keeps the colour: 0 for a pixel whose normal is 0, NaN when a denominator is 0
        // (depth 0, or sigma_depth * z_p underflowing: the centre tap's 0 / 0); cl2_denoise refuses den_c and den_a below FLT_MIN.
        if (sw > 0.0f) { o0 = s0 / sw; o1 = s1 / sw; o2 = s2 / sw; }
    }
    if (out3) { out3[3 * (size_t)p] = o0; out3[3 * (size_t)p + 1] = o1; out3[3 * (size_t)p + 2] = o2; }
    else cout[p] = make_float4(o0, o1, o2, 0.0f);
}

}  // namespace cl2
