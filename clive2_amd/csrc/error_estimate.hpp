// error_estimate.hpp -- per-pixel standard errors of the rendered picture and one frame metric, from the accumulators and the
// moment buffer that k_accumulate<true> / k_finalize_accumulate<true> (kernels.hpp) fill while cl2_set_error_tracking is on.
//
// No reference counterpart: the reference keeps first sums only (src/renderer.py:253-278).
//
// Definitions.  An ADDEND is what one sample stream of one pass adds to one pixel: x_c to accumulator row c (c = 0, 1, 2 =
// b, g, r), w to row 3; y = (x_b 0.0722 + x_g 0.7152) + x_r 0.2126 in float32.  The moment buffer mom [8][W*H] holds float32
// sums over the addends of   x_c^2 (rows 0..2), w^2 (3), x_c w (4..6), y^2 (7).
//
// The picture is the ratio estimator I_c = X_c / Wt (X_c = acc row c, Wt = acc row 3, renderer.py:293-297); its standard error
// by the delta method, per pixel, in float64 from the float32 sums, with n = acc row 7 (addends so far):
//     Wt not finite or Wt <= 0   uncovered: standard error 0, left out of the frame metric
//     n < 2                      +inf
//     else                       S_c = max(0, m_c - 2 I_c m_{4+c} + I_c^2 m_3),   var_c = n S_c / ((n - 1) Wt^2)
// and for luma the same with L = luma(I), m_7 and luma(m_4, m_5, m_6) in place of I_c, m_c and m_{4+c} (luma's weights are the
// float32 constants of y, widened).  S is the residual sum of squares sum (x - I w)^2 written out in raw moments: where a pixel
// is nearly noiseless (an emitter, a flat wall seen through many identical samples) its three terms are large and almost cancel,
// and the float32 rounding of the sums can leave a small negative remainder.  The clamp at 0 is the answer to that: the true
// value is >= 0 and about as small as the rounding, not a bug to be fixed by a wider type.
//
// Frame metric e(floor) = sqrt((1/N) sum_covered var_L / (L + floor)^2), N = covered pixels; +inf when N = 0 or a covered pixel
// has n < 2.  A covered pixel with var_L = 0 adds 0 (also when L + floor = 0).  The sum is per thread, per wave, per workgroup
// (a fixed grid) and then one final launch, as k_tone_logsum does: no atomics, the same bytes on every call.
#pragma once
#include <hip/hip_runtime.h>

namespace cl2 {

constexpr int ERR_BLOCKS = 1024;

__device__ __forceinline__ double err_luma(double b, double g, double r) {
    return (b * (double)0.0722f + g * (double)0.7152f) + r * (double)0.2126f;
}

// 0 uncovered, 1 too few addends (n < 2), 2 var[] holds b, g, r, luma; L = luma of the picture
__device__ __forceinline__ int err_pixel(const float* __restrict__ acc, const float* __restrict__ mom, size_t FB, size_t p,
                                         double (&var)[4], double& L) {
    const double Wt = (double)acc[3 * FB + p];
    if (!(Wt > 0.0) || !(Wt < __builtin_inf())) return 0;
    const double n = (double)acc[7 * FB + p];
    if (n < 2.0) return 1;
    double I[3];
#pragma unroll
    for (int c = 0; c < 3; c++) I[c] = (double)acc[(size_t)c * FB + p] / Wt;
    L = err_luma(I[0], I[1], I[2]);
    const double m3 = (double)mom[3 * FB + p];
    const double scale = n / ((n - 1.0) * (Wt * Wt));
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double S = (double)mom[(size_t)c * FB + p] - 2.0 * I[c] * (double)mom[(size_t)(4 + c) * FB + p] + I[c] * I[c] * m3;
        var[c] = (S > 0.0 ? S : 0.0) * scale;                 // cancellation: see the header
    }
    const double myw = err_luma((double)mom[4 * FB + p], (double)mom[5 * FB + p], (double)mom[6 * FB + p]);
    const double S = (double)mom[7 * FB + p] - 2.0 * L * myw + L * L * m3;
    var[3] = (S > 0.0 ? S : 0.0) * scale;
    return 2;
}

// (H, W, 4) float32: standard errors of b, g, r and luma
__global__ __launch_bounds__(256) void k_standard_error(int FB, const float* __restrict__ acc, const float* __restrict__ mom,
                                                        float4* __restrict__ out) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)FB) return;
    double var[4] = {0, 0, 0, 0}, L = 0.0;
    const int k = err_pixel(acc, mom, (size_t)FB, p, var, L);
    float4 o;
    if (k == 0) o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    else if (k == 1) o = make_float4(__builtin_inff(), __builtin_inff(), __builtin_inff(), __builtin_inff());
    else o = make_float4((float)sqrt(var[0]), (float)sqrt(var[1]), (float)sqrt(var[2]), (float)sqrt(var[3]));
    out[p] = o;
}

__device__ __forceinline__ void err_block_sum3(double (&v)[3], double* __restrict__ dst) {
    __shared__ double s_wave[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++)
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 3; k++) s_wave[k][threadIdx.x >> 6] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 3; k++) dst[k] = (s_wave[k][0] + s_wave[k][1]) + (s_wave[k][2] + s_wave[k][3]);
}

// per workgroup: partial[3 b + 0] = sum var_L / (L + floor)^2, [+1] = covered pixels, [+2] = covered pixels with n < 2
__global__ __launch_bounds__(256) void k_rel_error_partial(int FB, const float* __restrict__ acc, const float* __restrict__ mom,
                                                           double floor, double* __restrict__ partial) {
    double v[3] = {0.0, 0.0, 0.0};
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < (size_t)FB; p += (size_t)gridDim.x * 256) {
        double var[4] = {0, 0, 0, 0}, L = 0.0;
        const int k = err_pixel(acc, mom, (size_t)FB, p, var, L);
        if (k == 0) continue;
        v[1] += 1.0;
        if (k == 1) { v[2] += 1.0; continue; }
        if (var[3] > 0.0) {
            const double d = L + floor;
            v[0] += var[3] / (d * d);
        }
    }
    err_block_sum3(v, partial + 3 * (size_t)blockIdx.x);
}

// out[0] = e(floor), out[1..3] = the three totals
__global__ __launch_bounds__(256) void k_rel_error_final(const double* __restrict__ partial, int n, double* __restrict__ out) {
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] += partial[3 * i + k];
    err_block_sum3(v, out + 1);
    if (threadIdx.x == 0) out[0] = (out[2] == 0.0 || out[3] != 0.0) ? __builtin_inf() : sqrt(out[1] / out[2]);
}

}  // namespace cl2
