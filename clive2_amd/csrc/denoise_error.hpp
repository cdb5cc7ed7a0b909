// denoise_error.hpp -- an estimate of the squared luma error of the FILTERED picture (cl2_denoise or cl2_denoise_guided) by
// Monte-Carlo SURE: Stein's unbiased risk estimate with the filter's divergence taken from finite differences along random
// probes (Ramani, Blu, Unser 2008).  It needs only what the handle already holds -- accumulators, the moments of
// cl2_set_error_tracking, the feature buffers -- and runs the filters' own pass kernels on perturbed inputs.
//
// No reference counterpart (the reference stops at the Monte Carlo estimate, src/renderer.py:293-316).  Reads accumulators,
// moments and features; writes buffers of its own and the filters' shared working buffers.
//
// Per pixel p, from err_pixel (error_estimate.hpp) and the colour k_denoise_input forms:
//     y_p      the scrubbed float32 radiance (b, g, r)
//     state    err_pixel's 0 (uncovered), 1 (n < 2) or 2
//     v_p      (float) min(var_L, 2^100), the cap of k_denoise_guided_input; a NaN takes the cap            (state 2)
//     s_p      (float) sqrt((double) v_p)
//     d_p,c    (float)(se_c / err_luma(se_b, se_g, se_r)), se_c = sqrt(var_c) in float64; 1.0f for every channel when that luma
//              is not > 0 or is not finite (a moment sum that overflowed: inf / inf would put a NaN into every pass)
//     a_p,c    s_p * d_p,c in float32; states 0 and 1 take a_p = 0: no perturbation
// The noise model is rank 1 per pixel, n_p = eta_p d_p with Var eta_p = v_p: consistent with the per-channel and the luma
// variances the moments give.  The moments hold no cross-channel terms, which is why the estimate is of the LUMA error, like
// cl2_relative_error.
//
// Signs.  Probe k of a call with seed S uses t = S + k (uint32, wrapping); for pixel index q
//     h = q * 0x9E3779B9 + t * 0x85EBCA6B;  h ^= h >> 16;  h *= 0x7FEB352D;  h ^= h >> 15;  h *= 0x846CA68B;  h ^= h >> 16
//     b_q = (h >> 31) ? -1.0f : 1.0f
// so probe k of seed S is probe 0 of seed S + k.
//
// Perturbation field z.  correlated = 0: z_p = b_p.  correlated = 1: the signs passed through the mean reconstruction weights
// of the render (connect_resolve_body.hpp:150-179: every camera sample is spread over 3 x 3 pixels),
//     z_p = (sum_j sum_i (K_y(j) K_x(i)) b_(x-i, y-j)) / sqrt(sum_j sum_i (K_y(j) K_x(i))^2)
// both sums over the in-frame sources only (E z^2 = 1 at the borders too), j outer, i inner, j, i in -1, 0, 1, in float32; the
// quotient is formed once in float64 and rounded to float32.  K_x(i) = int_0^1 exp(-(i - u)^2 / c_x) du with
// c_x = (ppw^2 + pph^2) / (2 ppw^2), K_y the same with c_y = (ppw^2 + pph^2) / (2 pph^2), ppw and pph the camera's physical
// pixel sizes (float32, as the resolve kernel forms them); the host evaluates them in float64 with erf and rounds to float32.
// Square pixels: K = (0.135257, 0.746824, 0.746824) -- a sample of pixel k lies at k + U[0, 1) while pixel centres sit at the
// integers, so the spread is lopsided.  The light image (t = 1 splats) is not reconstructed: real renders lie between the modes.
//
// Perturbed input  y'_p,c = y_p,c + (epsilon * z_p) * a_p,c  in float32.  .w of the working float4 is what the filter expects:
// 0 for the fixed filter, k_denoise_guided_input's v (2^100 in state 1, 0 in state 0) for the guided one.
//
// F = the chosen filter's passes, by k_denoise_pass / k_denoise_guided_pass with cl2_denoise's / cl2_denoise_guided's
// parameters: F(y) is, byte for byte, what those calls return.
//
// Terms, float64, luma = err_luma of the float32 values, probes k = 0 .. P-1:
//     u_pk   = luma(y'_pk) - luma(y_p)                      the realised perturbation
//     g_pk   = luma(F(y'_k)_p) - luma(F(y)_p)
//     div_p  = (sum_k u_pk g_pk, in probe order, from 0.0) / (((double) eps * (double) eps) * P)
//     fid_p  = (luma(F(y)_p) - luma(y_p))^2
//     sure_p = (fid_p - v_p) + 2 div_p
// Map, float32: 0 in state 0, +inf in state 1, (float) sure_p in state 2.
// Totals out[8], each summed as k_rel_error_partial / k_rel_error_final sum (at most ERR_BLOCKS workgroups of 256 threads,
// strided; the wave tree and four-wave sum of err_block_sum3; no atomics: the same bytes on every call):
//     [1] sum over state 2 of sure_p / (luma(F(y)_p) + floor)^2; a sure_p of exactly 0 adds 0 whatever the denominator
//     [2] N = pixels in state 1 or 2      [3] pixels in state 1
//     [4] sum sure_p      [5] sum fid_p      [6] sum v_p      [7] sum 2 div_p          (state 2)
//     [0] e_dn = +inf when N = 0 or [3] > 0; else with t = [1] / N: 0 when t < 0, sqrt(t) otherwise (a NaN stays a NaN)
// e_dn(floor) is the counterpart of cl2_relative_error's e(floor) for the filtered picture; with iterations = 0 and
// correlated = 0 it IS e(floor), up to the rounding of y + delta.
//
// Known limits.  The weight 1 / (luma F + floor)^2 depends on the data -- the liberty e(floor) takes too.  For the guided filter
// v is treated as a fixed parameter of F although it comes from the same samples.  A single probe's map is noisy and can be
// negative: the frame totals are what is calibrated.  The estimate is unbiased under ITS noise model (tests/
// test_denoise_error_cpu.py); with the wrong covariance it is badly off, which is why both modes exist.  Where the filter removes nearly all of
// the variance the estimate is a small difference of large terms and the divergence decides it: on the 1080p Cornell box real
// renders lie between the two modes, independent signs run low (e_dn 0.0086 for a true 0.0139 at 10 passes, R 0.30 .. 0.72) and the
// guided filter's total is negative.
// tests/denoise_error_reference.py restates every operation below in numpy, in the same order.
#pragma once
#include <hip/hip_runtime.h>
#include "denoise_guided.hpp"
#include "error_estimate.hpp"
#include "error_split.hpp"

namespace cl2 {

struct DeKernel {          // the reconstruction weights of the correlated mode: index i + 1, j + 1
    float kx[3], ky[3];
};

// y (the filter's working float4) and A = (a_b, a_g, a_r, code): code = v_p in state 2 (>= 0), -1 in state 0, -2 in state 1 -- the
// fixed filter's working buffer carries 0 in .w, so this is where k_de_terms finds v_p for both kinds.  out3: the packed picture
// too, when no pass follows
__global__ __launch_bounds__(BLOCK) void k_de_input(int FB, int guided, const float* __restrict__ acc, const float* __restrict__ mom,
                                                    float4* __restrict__ Y, float4* __restrict__ A, float* __restrict__ out3) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= FB) return;
    float c[3];
    dn_input_colour(acc, (size_t)FB, (size_t)p, acc[3 * (size_t)FB + p], c);
    double var[4] = {0, 0, 0, 0}, L = 0.0;
    const int state = err_pixel(acc, mom, (size_t)FB, (size_t)p, var, L);
    const float v = dng_guide_variance(state, var[3]);
    float a[3] = {0.0f, 0.0f, 0.0f};
    if (state == 2) {
        const float s = (float)sqrt((double)v);
        const double se[3] = {sqrt(var[0]), sqrt(var[1]), sqrt(var[2])};
        const double l = err_luma(se[0], se[1], se[2]);
        const bool ok = l > 0.0 && l < __builtin_inf();
        for (int k = 0; k < 3; k++) a[k] = s * (ok ? (float)(se[k] / l) : 1.0f);
    }
    Y[p] = make_float4(c[0], c[1], c[2], guided ? v : 0.0f);
    A[p] = make_float4(a[0], a[1], a[2], state == 2 ? v : (state == 1 ? -2.0f : -1.0f));
    if (out3) dn_store3(out3, (size_t)p, c[0], c[1], c[2]);
}

__device__ __forceinline__ float de_sign(uint32_t q, uint32_t t) {
    uint32_t h = q * 0x9E3779B9u + t * 0x85EBCA6Bu;
    h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
    return (h >> 31) ? -1.0f : 1.0f;
}

// the correlated field of (p, t): the up to nine signs are hashed here, there is no sign buffer
__device__ __forceinline__ float de_correlated_z(int W, int H, int p, uint32_t t, const DeKernel& K) {
    const int x = p % W, y = p / W;
    float num = 0.0f, den = 0.0f;
#pragma unroll
    for (int j = -1; j <= 1; j++) {
#pragma unroll
        for (int i = -1; i <= 1; i++) {
            const int sx = x - i, sy = y - j;
            if (sx < 0 || sx >= W || sy < 0 || sy >= H) continue;
            const float k = K.ky[j + 1] * K.kx[i + 1];
            num += k * de_sign((uint32_t)(sy * W + sx), t);
            den += k * k;
        }
    }
    return (float)((double)num / sqrt((double)den));
}

// y' = y + (eps z) a of pixel p into the working buffer, and into the packed picture when no pass follows
__device__ __forceinline__ void de_store_perturbed(int p, float ez, const float4* __restrict__ Y, const float4* __restrict__ A,
                                                   float4* __restrict__ Yp, float* __restrict__ out3) {
    const float4 y4 = Y[p], a = A[p];
    const float4 o = make_float4(y4.x + ez * a.x, y4.y + ez * a.y, y4.z + ez * a.z, y4.w);
    Yp[p] = o;
    if (out3) dn_store3(out3, (size_t)p, o.x, o.y, o.z);
}

// the pure modes: z the sign of (p, t), or the correlated field
__global__ __launch_bounds__(BLOCK) void k_de_perturb(int W, int H, uint32_t t, float eps, int correlated, DeKernel K,
                                                      const float4* __restrict__ Y, const float4* __restrict__ A,
                                                      float4* __restrict__ Yp, float* __restrict__ out3) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= W * H) return;
    const float z = correlated ? de_correlated_z(W, H, p, t, K) : de_sign((uint32_t)p, t);
    de_store_perturbed(p, eps * z, Y, A, Yp, out3);
}

// Noise model 2, "split" (error_split.hpp): z_p = cs_p zK_p + cl_p b'_p with zK the correlated field of (p, t)
// above, b'_p = de_sign(p, t ^ 0xA5A5A5A5), cs = (float) sqrt(1.0 - (double) rho_p), cl = (float) sqrt((double) rho_p) from the
// float32 rho_p of k_de_rho; z in float32.  E z^2 = 1 (the two fields are independent and each has E = 1), so Var y' = eps^2 v as
// in the pure modes, and a pair p != q carries cs_p cs_q times the reconstruction covariance.  rho = 1 is the independent mode
// with other signs; rho = 0 gives the correlated mode's bytes (0 * b' adds +-0 to zK).
__global__ __launch_bounds__(BLOCK) void k_de_perturb_split(int W, int H, uint32_t t, float eps, DeKernel K,
                                                            const float* __restrict__ rho, const float4* __restrict__ Y,
                                                            const float4* __restrict__ A, float4* __restrict__ Yp,
                                                            float* __restrict__ out3) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= W * H) return;
    const float r = rho[p];
    const float cs = (float)sqrt(1.0 - (double)r), cl = (float)sqrt((double)r);
    const float z = cs * de_correlated_z(W, H, p, t, K) + cl * de_sign((uint32_t)p, t ^ 0xA5A5A5A5u);
    de_store_perturbed(p, eps * z, Y, A, Yp, out3);
}

// the colours of a working buffer as a packed (H, W, 3) picture (out_probe's y')
__global__ __launch_bounds__(BLOCK) void k_de_pack(int FB, const float4* __restrict__ C4, float* __restrict__ out3) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= FB) return;
    const float4 c = C4[p];
    dn_store3(out3, (size_t)p, c.x, c.y, c.z);
}

constexpr int DE_SUMS = 7;     // out[1..7] of the header

// err_block_sum3 for DE_SUMS values: the same wave tree, the same four-wave sum
__device__ __forceinline__ void de_block_sum(double (&v)[DE_SUMS], double* __restrict__ dst) {
    __shared__ double s_wave[DE_SUMS][4];
#pragma unroll
    for (int k = 0; k < DE_SUMS; k++)
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < DE_SUMS; k++) s_wave[k][threadIdx.x >> 6] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < DE_SUMS; k++) dst[k] = (s_wave[k][0] + s_wave[k][1]) + (s_wave[k][2] + s_wave[k][3]);
}

__device__ __forceinline__ double de_luma3(const float* __restrict__ c, size_t p) {
    return err_luma((double)c[3 * p], (double)c[3 * p + 1], (double)c[3 * p + 2]);
}

// One probe's u g into sum[]; LAST: the map and the workgroup's partial totals, partial[DE_SUMS b + k] = out[1 + k]'s share.
// scale = ((double) eps * (double) eps) * probes.
template <bool LAST>
__global__ __launch_bounds__(256) void k_de_terms(int FB, const float4* __restrict__ Y, const float4* __restrict__ Yp,
                                                  const float* __restrict__ Fy, const float* __restrict__ Fyp,
                                                  const float4* __restrict__ A, double* __restrict__ sum, double scale, double floor,
                                                  float* __restrict__ map, double* __restrict__ partial) {
    double v[DE_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < (size_t)FB; p += (size_t)gridDim.x * 256) {
        const float4 y = Y[p], yp = Yp[p], a = A[p];
        const double ly = err_luma((double)y.x, (double)y.y, (double)y.z);
        const double lf = de_luma3(Fy, p);
        const double u = err_luma((double)yp.x, (double)yp.y, (double)yp.z) - ly;
        const double g = de_luma3(Fyp, p) - lf;
        const double s = sum[p] + u * g;
        sum[p] = s;
        if (!LAST) continue;
        if (a.w == -1.0f) { if (map) map[p] = 0.0f; continue; }                              // state 0
        v[1] += 1.0;
        if (a.w == -2.0f) { v[2] += 1.0; if (map) map[p] = __builtin_inff(); continue; }     // state 1
        const double vp = (double)a.w;
        const double d2 = 2.0 * (s / scale);
        const double fid = (lf - ly) * (lf - ly);
        const double sure = (fid - vp) + d2;
        if (map) map[p] = (float)sure;
        if (sure != 0.0) {
            const double d = lf + floor;
            v[0] += sure / (d * d);
        }
        v[3] += sure; v[4] += fid; v[5] += vp; v[6] += d2;
    }
    if (LAST) de_block_sum(v, partial + DE_SUMS * (size_t)blockIdx.x);
}

// out[1..7] = the totals, out[0] = e_dn
__global__ __launch_bounds__(256) void k_de_final(const double* __restrict__ partial, int n, double* __restrict__ out) {
    double v[DE_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int k = 0; k < DE_SUMS; k++) v[k] += partial[DE_SUMS * i + k];
    de_block_sum(v, out + 1);
    if (threadIdx.x == 0) {
        const double t = out[1] / out[2];
        out[0] = (out[2] == 0.0 || out[3] != 0.0) ? __builtin_inf() : (t < 0.0 ? 0.0 : sqrt(t));
    }
}

}  // namespace cl2
