// denoise_guided.hpp -- the a-trous filter of denoise.hpp with its colour edge-stop replaced by one that knows the noise: the luma
// difference of two pixels is compared with the standard error of the centre pixel (the spatial edge-stopping function of SVGF,
// Schied et al. 2017), taken from the per-pixel variance estimate of error_estimate.hpp.  A second filter beside the fixed one:
// the input colour, the packed store and the feature edge-stop it shares with denoise.hpp are defined there.
//
// No reference counterpart (the reference stops at the Monte Carlo estimate, src/renderer.py:293-316).  Reads the handle's
// accumulators, moments and feature buffers; writes buffers of its own.
//
// Input per pixel p: colour c_p = scrub(acc_image / acc_weight) as k_denoise_input forms it, and a variance
//     v_p = (float) min(var_L, 2^100)   var_L = err_pixel's float64 luma variance (state 2)
//     v_p = 2^100                        with fewer than two addends (state 1)
//     v_p = 0                            uncovered by the render (state 0)
// The cap keeps every product with a weight <= 1 and every 25-term sum finite: no inf or NaN enters a pass.  (c, v) travel as one
// float4: the working buffers of the fixed filter carry 0 in .w, so the variance costs no extra bytes per tap.
//
// Pass i (step s = 2^i), for a pixel with feature coverage != 0:
//     vbar_p = sum g(dy) g(dx) v_q / sum g(dy) g(dx)   over the 3 x 3 around p (offsets -1..1, NOT scaled by s), g = (1/4, 1/2, 1/4),
//              taps inside the frame with coverage != 0
//     den_l  = sigma_luma * sqrt(vbar_p) + 1e-8f
//     l(x)   = (x.b 0.0722f + x.g 0.7152f) + x.r 0.2126f                                on the raw colour, no compression
//     w_q    = ((((h(dx) h(dy)) w_n) w_z) w_a) exp(-|l(c_p) - l(c_q)| / den_l)          w_n, w_z, w_a, h as k_denoise_pass
//     c'_p   = sum w_q c_q / sum w_q            v'_p = sum w_q^2 v_q / (sum w_q)^2
// Taps dy outer, dx inner; taps off the frame or with coverage 0 are skipped; a pixel without coverage or with sum w = 0 keeps
// c and v.  sigma_luma is the same in every pass: the shrinking v' narrows the filter.  v' treats the taps as independent, which
// holds for the first pass only: it is the filter's guide, NOT an error estimate of the filtered picture (it is far too small).
// tests/guided_denoise_reference.py restates every operation below in numpy, in the same order.
#pragma once
#include <hip/hip_runtime.h>
#include "denoise.hpp"
#include "error_estimate.hpp"

namespace cl2 {

constexpr float DNG_VAR_CAP = 0x1p100f;

// the guide variance of a pixel from err_pixel's state and float64 luma variance: v_p of the header
__device__ __forceinline__ float dng_guide_variance(int state, double var_L) {
    if (state == 1) return DNG_VAR_CAP;
    if (state == 2) return var_L < (double)DNG_VAR_CAP ? (float)var_L : DNG_VAR_CAP;      // a NaN takes the cap too
    return 0.0f;
}

__global__ __launch_bounds__(BLOCK) void k_denoise_guided_input(int FB, const float* __restrict__ acc, const float* __restrict__ mom,
                                                                float4* __restrict__ cout, float* __restrict__ out3,
                                                                float* __restrict__ outv) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= FB) return;
    float c[3];
    dn_input_colour(acc, (size_t)FB, (size_t)p, acc[3 * (size_t)FB + p], c);
    double var[4] = {0, 0, 0, 0}, L = 0.0;
    const int state = err_pixel(acc, mom, (size_t)FB, (size_t)p, var, L);
    const float v = dng_guide_variance(state, var[3]);
    if (out3) {
        dn_store3(out3, (size_t)p, c[0], c[1], c[2]);
        if (outv) outv[p] = v;
    } else cout[p] = make_float4(c[0], c[1], c[2], v);
}

__device__ __forceinline__ float dng_luma(float4 c) { return (c.x * 0.0722f + c.y * 0.7152f) + c.z * 0.2126f; }

// The body is this kernel's own, like k_denoise_pass's: see the note there.
// One guided pass at step `step` (= 2^i).  den_a = sigma_albedo^2 (host-computed, float32).  LDS_STEP as k_denoise_pass: 1 or 2
// stage the workgroup's pixels and a halo of two steps (>= 2 pixels, so the 3 x 3 of v comes from the same tile) in LDS;
// 0 takes every tap from global memory and the 3 x 3 as eight more 4-byte loads each of coverage and v (the centre is at hand).
template <int LDS_STEP>
__global__ __launch_bounds__(DN_TILE * DN_TILE) void k_denoise_guided_pass(int W, int H, int step, float sigma_luma, float sigma_depth,
                                                                            float den_a, const float4* __restrict__ cin,
                                                                            const float4* __restrict__ G0, const float4* __restrict__ G1,
                                                                            float4* __restrict__ cout, float* __restrict__ out3,
                                                                            float* __restrict__ outv) {
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
    float o0 = cp.x, o1 = cp.y, o2 = cp.z, ov = cp.w;
    if (ap.w != 0.0f) {
        const float g[3] = {0.25f, 0.5f, 0.25f};
        float sg = 0.0f, sv = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                float vq, covq;
                if (LDS_STEP) {
                    const int k = (ly + 2 * LDS_STEP + dy) * T + lx + 2 * LDS_STEP + dx;
                    vq = s_c[k].w; covq = s_a[k].w;
                } else if (dy == 0 && dx == 0) {
                    vq = cp.w; covq = ap.w;
                } else {
                    const int qx = px + dx, qy = py + dy;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const int q = qy * W + qx;
                    vq = cin[q].w; covq = G1[q].w;
                }
                if (covq == 0.0f) continue;
                const float gg = g[dy + 1] * g[dx + 1];
                sg += gg;
                sv += gg * vq;
            }
        }
        const float vbar = sv / sg;                          // the centre always counts: sg >= 1/4
        const float den_l = sigma_luma * sqrtf(vbar) + 1e-8f;
        const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
        const V3 n = v3(np_), a = v3(ap);
        const float lp = dng_luma(cp);
        const float zp = np_.w;
        const float den_z = (sigma_depth * zp) * (float)step;
        float sw = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
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
                const float wl = expf(-fabsf(lp - dng_luma(cq)) / den_l);
                const float w = ((((h[dx + 2] * h[dy + 2]) * wn) * wz) * wa) * wl;
                sw += w;
                s0 += w * cq.x; s1 += w * cq.y; s2 += w * cq.z;
                s3 += (w * w) * cq.w;
            }
        }
        if (sw > 0.0f) { o0 = s0 / sw; o1 = s1 / sw; o2 = s2 / sw; ov = s3 / (sw * sw); }
    }
    if (out3) {
        out3[3 * (size_t)p] = o0; out3[3 * (size_t)p + 1] = o1; out3[3 * (size_t)p + 2] = o2;
        if (outv) outv[p] = ov;
    } else cout[p] = make_float4(o0, o1, o2, ov);
}

}  // namespace cl2
