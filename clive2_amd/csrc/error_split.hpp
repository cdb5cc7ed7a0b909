// error_split.hpp -- the luma variance of the picture split into its CAMERA part and its LIGHT part, per pixel, and the light part's
// share of it (cl2_set_split_tracking, cl2_light_share).
//
// No reference counterpart: the reference keeps first sums only (src/renderer.py:253-278).
//
// Why.  The camera image of a pass is spread over 3 x 3 pixels by the reconstruction filter, so its noise is correlated between
// neighbours; the light image (t = 1 splats) is not reconstructed, so its noise is independent.  The moment buffer of
// error_estimate.hpp sees only their sum x = scrub(light + camera).  The SPLIT ROWS smom [6][W*H] (float32 sums, 24 bytes per
// pixel, while split tracking is on) keep the two apart.  One sample stream of one pass adds one addend per pixel; its parts are
// exactly what k_finalize_accumulate / k_accumulate (kernels.hpp) form:
//     t, wc   the camera part: `total`, `wsum` of the nine-tap gather (or finalized.xyz, sample_w of the stage calls)
//     l, wl   the light part: light_image[e], wl = l.w
//     yc = (scrub(t.x) 0.0722f + scrub(t.y) 0.7152f) + scrub(t.z) 0.2126f        yl = the same of l
//     row 0 += yc yc    1 += yc wc    2 += wc wc    3 += yl yl    4 += yl wl    5 += wl wl
// one float32 add per row and addend, in stream order.  The rows are filled by two kernels of their own, launched on the stream of
// the accumulating kernel immediately before it (it zeroes the light image): the accumulating kernels keep their text, and with
// split tracking off nothing here runs.
//
// The share.  Per pixel in float64, with `state` and L from err_pixel (error_estimate.hpp):
//     S_c = max(0, m0 - 2 L m1 + L^2 m2)      S_l = max(0, m3 - 2 L m4 + L^2 m5)
//     rho = S_l / (S_c + S_l) when that sum is > 0 and finite, else 1;  rho = 1 in states 0 and 1
// so a pixel without a usable split behaves as the default noise model, independent signs.  Every comparison is written so that a
// NaN falls to 1: the clamp is `S < 0 ? 0 : S`, which keeps a NaN (a NaN or an overflowed row, inf - inf), and the sum is then
// not > 0.  The sharing is PROPORTIONAL on purpose: the variance that enters SURE stays err_pixel's var_L exactly -- sum v
// and the fidelity term do not move -- and no camera-light cross term is needed (S_c + S_l is not S: the scrub of the sum and
// the cross term 2 sum (yc - L wc)(yl - L wl) separate them; only the ratio is used).
//
// cl2_light_share: the map (float) rho and, over the state-2 pixels with finite var_L, the totals
//     [1] sum rho var_L    [2] sum var_L    [3] their count    [0] = [1] / [2], 0 when [2] is not > 0
// summed as k_rel_error_partial / k_rel_error_final sum: no atomics, the same bytes on every call.
// tests/error_split_reference.py restates every operation below in numpy, in the same order.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "error_estimate.hpp"

namespace cl2 {

constexpr int SPLIT_ROWS = 6;

__device__ __forceinline__ float split_luma(float b, float g, float r) {
    return (scrub(b) * 0.0722f + scrub(g) * 0.7152f) + scrub(r) * 0.2126f;
}

__device__ __forceinline__ void add_split(float (&m)[SPLIT_ROWS], float yc, float wc, float yl, float wl) {
    m[0] += yc * yc;
    m[1] += yc * wc;
    m[2] += wc * wc;
    m[3] += yl * yl;
    m[4] += yl * wl;
    m[5] += wl * wl;
}

// Before k_finalize_accumulate, from the aggregator rows: the nine-tap gather is that kernel's, statement for statement, so `total`
// and `wsum` have its bits.  One thread per PIXEL adds its streams in order.
__global__ __launch_bounds__(BLOCK) void k_split_moments_fused(int B, int W, int H, const float* __restrict__ agg,
                                                               const float4* __restrict__ light_image, float* __restrict__ smom) {
    const int id = blockIdx.x * BLOCK + threadIdx.x;
    const int FB = W * H;
    if (id >= FB) return;
    float m[SPLIT_ROWS];
#pragma unroll
    for (int c = 0; c < SPLIT_ROWS; c++) m[c] = smom[(size_t)c * FB + id];
#pragma unroll 1
    for (size_t base = 0; base < (size_t)B; base += (size_t)FB) {
        V3 total = v3(0, 0, 0);
        float wsum = 0.0f;
        // one row of three neighbours in flight at a time, as k_finalize_accumulate
#pragma unroll 1
        for (int i = -1; i < 2; i++) {
#pragma unroll
            for (int j = -1; j < 2; j++) {
                const int sx = (id % W) + i, sy = (id / W) + j;
                if (sx < 0 || sx >= W || sy < 0 || sy >= H) continue;
                const size_t k = base + (size_t)sy * W + sx;
                const float weight = agg[(size_t)((1 - i) * 3 + (1 - j)) * B + k];
                total = total + weight * v3(agg[(size_t)9 * B + k], agg[(size_t)10 * B + k], agg[(size_t)11 * B + k]);
                wsum += weight * agg[(size_t)12 * B + k];
            }
        }
        const float4 l = light_image[base + id];
        add_split(m, split_luma(total.x, total.y, total.z), wsum, split_luma(l.x, l.y, l.z), l.w);
    }
#pragma unroll
    for (int c = 0; c < SPLIT_ROWS; c++) smom[(size_t)c * FB + id] = m[c];
}

// Before k_accumulate, from the per-sample images of the stage calls (cl2_process_images after cl2_finalize_samples or
// cl2_import_sample_images)
__global__ __launch_bounds__(BLOCK) void k_split_moments_staged(int FB, int streams, const float4* __restrict__ finalized,
                                                                const float* __restrict__ sample_w,
                                                                const float4* __restrict__ light_image, float* __restrict__ smom) {
    const int id = blockIdx.x * BLOCK + threadIdx.x;
    if (id >= FB) return;
    float m[SPLIT_ROWS];
#pragma unroll
    for (int c = 0; c < SPLIT_ROWS; c++) m[c] = smom[(size_t)c * FB + id];
#pragma unroll 1
    for (int s = 0; s < streams; s++) {
        const size_t e = (size_t)s * FB + id;
        const float4 f = finalized[e], l = light_image[e];
        add_split(m, split_luma(f.x, f.y, f.z), sample_w[e], split_luma(l.x, l.y, l.z), l.w);
    }
#pragma unroll
    for (int c = 0; c < SPLIT_ROWS; c++) smom[(size_t)c * FB + id] = m[c];
}

// rho of one pixel (see the header); `state`, `var` and L are err_pixel's
__device__ __forceinline__ double split_rho(const float* __restrict__ acc, const float* __restrict__ mom,
                                            const float* __restrict__ smom, size_t FB, size_t p, int& state, double (&var)[4]) {
    double L = 0.0;
    state = err_pixel(acc, mom, FB, p, var, L);
    if (state != 2) return 1.0;
    const double Sc = (double)smom[p] - 2.0 * L * (double)smom[FB + p] + L * L * (double)smom[2 * FB + p];
    const double Sl = (double)smom[3 * FB + p] - 2.0 * L * (double)smom[4 * FB + p] + L * L * (double)smom[5 * FB + p];
    const double sc = Sc < 0.0 ? 0.0 : Sc, sl = Sl < 0.0 ? 0.0 : Sl;           // a NaN stays: the sum is then not > 0, rho = 1
    const double sum = sc + sl;
    return (sum > 0.0 && sum < __builtin_inf()) ? sl / sum : 1.0;
}

// the map alone: the rho buffer of k_de_perturb_split (denoise_error.hpp)
__global__ __launch_bounds__(256) void k_de_rho(int FB, const float* __restrict__ acc, const float* __restrict__ mom,
                                                const float* __restrict__ smom, float* __restrict__ rho) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)FB) return;
    int state;
    double var[4] = {0, 0, 0, 0};
    rho[p] = (float)split_rho(acc, mom, smom, (size_t)FB, p, state, var);
}

// per workgroup: partial[3 b + 0] = sum rho var_L, [+1] = sum var_L, [+2] = the pixels summed; the map when `map` is not NULL
__global__ __launch_bounds__(256) void k_light_share_partial(int FB, const float* __restrict__ acc, const float* __restrict__ mom,
                                                             const float* __restrict__ smom, float* __restrict__ map,
                                                             double* __restrict__ partial) {
    double v[3] = {0.0, 0.0, 0.0};
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < (size_t)FB; p += (size_t)gridDim.x * 256) {
        int state;
        double var[4] = {0, 0, 0, 0};
        const double rho = split_rho(acc, mom, smom, (size_t)FB, p, state, var);
        if (map) map[p] = (float)rho;
        if (state != 2 || !(var[3] < __builtin_inf())) continue;       // var_L is never negative; a NaN is left out
        v[0] += rho * var[3];
        v[1] += var[3];
        v[2] += 1.0;
    }
    err_block_sum3(v, partial + 3 * (size_t)blockIdx.x);
}

// out[1..3] = the three totals, out[0] = the frame's light share
__global__ __launch_bounds__(256) void k_light_share_final(const double* __restrict__ partial, int n, double* __restrict__ out) {
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] += partial[3 * i + k];
    err_block_sum3(v, out + 1);
    if (threadIdx.x == 0) out[0] = out[2] > 0.0 ? out[1] / out[2] : 0.0;
}

}  // namespace cl2
