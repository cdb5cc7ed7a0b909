// denoise_select.hpp -- a per-pixel choice among the scales of the fixed a-trous filter (cl2_denoise, denoise.hpp) by smoothed
// SURE maps: the selection scheme of Li, Wu and Chuang 2012 applied to the passes of the filter the handle already
// has.  Pass i of k_denoise_pass depends only on i (den_c = sigma_color^2 4^-i, step 2^i), so the output after pass k of a K-pass
// run is, byte for byte, cl2_denoise(iterations = k): one K-pass run on y and one per probe on the perturbed y' give the picture
// and the Monte-Carlo SURE terms (denoise_error.hpp) of all K + 1 candidates F_0 = y, F_1, ..., F_K.
//
// No reference counterpart (the reference stops at the Monte Carlo estimate, src/renderer.py:293-316).  Reads accumulators, moments
// and features; writes buffers of its own only.  The levels are made by k_de_input, k_de_perturb and k_denoise_pass themselves.
//
// Inputs: exactly cl2_denoise_error's for kind 0 -- y and A = (a, code) from k_de_input, y' of probe k from k_de_perturb with
// t = seed + k, epsilon, correlated.
//
// Levels, K = iterations in 1..12:  L_0 = y;  L_(i+1) = k_denoise_pass at step 2^i with den_c = ldexp(sigma_color^2, -2i) from L_i,
// every pass into a float4 buffer (out3 = NULL, .w = 0 as that kernel writes it).  The same for y'.
//
// Per-level terms, float64, luma = err_luma of the float32 values, probes k = 0 .. P-1, levels j = 0 .. K:
//     u_pk    = luma(y'_pk) - luma(y_p)
//     g_jpk   = luma(L_j(y'_k)_p) - luma(L_j(y)_p)
//     div_jp  = (sum_k u_pk g_jpk, in probe order, from 0.0) / (((double) eps * (double) eps) * P)
//     fid_jp  = (luma(L_j(y)_p) - luma(y_p))^2
//     sure_jp = (fid_jp - v_p) + 2 div_jp
// Raw maps m_j, float32 [K+1][H][W]: (float) sure_jp in state 2, 0 in state 0, +inf in state 1 -- the coding of cl2_denoise_error's
// map, so m_K is that map bit for bit and m_0 is v up to the rounding of y + delta.
//
// Smoothing: S = smooth_passes in 0..4 passes of the 5 x 5 B3 kernel at steps 1, 2, 4, ...; a tap's weight is
//     w = dn_feature_weight(h[dx+2] * h[dy+2], ...)
// of denoise.hpp, the filter's own feature edge-stop (den_z = (sigma_depth * z_p) * (float) step, den_a = sigma_albedo^2), with no
// colour term.  Skipped taps: outside the frame, feature coverage 0, or a pixel not in state 2.  A centre pixel that is not in
// state 2 or has coverage 0 keeps its K + 1 values.  The K + 1 maps share every weight: s_j += w * m_j(q), sw += w, row-major over
// dy, dx like the filter; M_j = s_j / sw, and a weight sum that is not greater than 0 (NaN included) keeps the pixel's K + 1 values.
// All of it float32.  S = 0: M = m.
//
// Selection k*_p, int32: state 0 takes 0; state 1 takes K (no variance estimate: treated as noisy); state 2 starts with best = 0
// and for j = 1 .. K takes j if M_j < M_best, or if M_best is NaN and M_j is not -- ties go to the smaller j, a NaN never wins
// over a number.
//
// Picture out_p = L_(k*_p)(y)_p, float32 (H, W, 3) b, g, r: every pixel a copy of bytes.
//
// Totals out[8], summed as cl2_denoise_error's are (at most ERR_BLOCKS workgroups of 256 threads, strided; de_block_sum's wave tree
// and four-wave sum; k_de_final; no atomics: the same bytes on every call):
//     [1] sum over state 2 of M_(k*),p / (luma(out_p) + floor)^2; an M of exactly 0 adds 0
//     [2] N = pixels in state 1 or 2      [3] pixels in state 1
//     [4] sum M_(k*),p      [5] sum M_K,p      [6] sum M_0,p          (state 2)
//     [7] sum of k*_p over states 1 and 2
//     [0] e_sel = +inf when N = 0 or [3] > 0; else with t = [1] / N: 0 when t < 0, sqrt(t) otherwise (a NaN stays a NaN)
// e_sel IS BIASED LOW: the minimum over noisy estimates always lies below the estimate of the level it picks, on top of the
// calibration limits of denoise_error.hpp.  It is a diagnostic; nothing stops a render on it.
//
// Device memory, allocated by the first call, regrown when K grows: both level sets 2 (K+1) 16 B, the sums (K+1) 8 B and three map
// buffers 3 (K+1) 4 B per pixel, plus A, the scale map and the picture (32 B): 52 (K+1) + 32 B per pixel.
// tests/denoise_select_reference.py restates every operation below in numpy, in the same order.
#pragma once
#include <hip/hip_runtime.h>
#include "denoise_error.hpp"

namespace cl2 {

constexpr int DS_MAX_SMOOTH = 4;              // smooth_passes 0..4: steps 1, 2, 4, 8

__device__ __forceinline__ double ds_luma4(float4 c) { return err_luma((double)c.x, (double)c.y, (double)c.z); }

__device__ __forceinline__ int ds_state(float code) { return code == -1.0f ? 0 : (code == -2.0f ? 1 : 2); }     // A.w of k_de_input

// One probe's u g_j into sum[j][p] for every level: L, Lp = the levels of y and of this probe's y', [levels][FB] each
__global__ __launch_bounds__(256) void k_ds_terms(int FB, int levels, const float4* __restrict__ L, const float4* __restrict__ Lp,
                                                  double* __restrict__ sum) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)FB) return;
    const double u = ds_luma4(Lp[p]) - ds_luma4(L[p]);
    for (int j = 0; j < levels; j++) {
        const size_t at = (size_t)j * FB + p;
        const double g = ds_luma4(Lp[at]) - ds_luma4(L[at]);
        sum[at] = sum[at] + u * g;
    }
}

// m_j from the sums; scale = ((double) eps * (double) eps) * probes
__global__ __launch_bounds__(256) void k_ds_map(int FB, int levels, const float4* __restrict__ L, const float4* __restrict__ A,
                                                const double* __restrict__ sum, double scale, float* __restrict__ m) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)FB) return;
    const float code = A[p].w;
    const int state = ds_state(code);
    const double ly = ds_luma4(L[p]), vp = (double)code;
    for (int j = 0; j < levels; j++) {
        const size_t at = (size_t)j * FB + p;
        float o = state == 0 ? 0.0f : __builtin_inff();
        if (state == 2) {
            const double lf = ds_luma4(L[at]);
            const double d2 = 2.0 * (sum[at] / scale);
            const double fid = (lf - ly) * (lf - ly);
            o = (float)((fid - vp) + d2);
        }
        m[at] = o;
    }
}

// One smoothing pass at step `step` over all `levels` maps: the 25 weights are formed once and kept in registers (the tap loops
// are unrolled, so w[] is never indexed by a run-time value), then every level is one row-major sweep over them.  Every tap is two
// 16-byte feature loads, one 4-byte state load and `levels` 4-byte map loads from global memory.
__global__ __launch_bounds__(DN_TILE * DN_TILE) void k_ds_smooth(int W, int H, int levels, int step, float sigma_depth, float den_a,
                                                                  const float* __restrict__ m_in, const float4* __restrict__ G0,
                                                                  const float4* __restrict__ G1, const float4* __restrict__ A,
                                                                  float* __restrict__ mout) {
    const int px = blockIdx.x * DN_TILE + threadIdx.x, py = blockIdx.y * DN_TILE + threadIdx.y;
    if (px >= W || py >= H) return;
    const size_t FB = (size_t)W * H;
    const int p = py * W + px;
    const float4 np_ = G0[p], ap = G1[p];
    float w[25];
    unsigned valid = 0;
    float sw = 0.0f;
    const bool open = ap.w != 0.0f && ds_state(A[p].w) == 2;
    if (open) {
        const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
        const V3 n = v3(np_), a = v3(ap);
        const float zp = np_.w;
        const float den_z = (sigma_depth * zp) * (float)step;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int t = (dy + 2) * 5 + dx + 2;
                w[t] = 0.0f;
                const int qx = px + dx * step, qy = py + dy * step;
                if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                const int q = qy * W + qx;
                const float4 aq = G1[q];
                if (aq.w == 0.0f || ds_state(A[q].w) != 2) continue;
                const float4 nq = G0[q];
                w[t] = dn_feature_weight(h[dx + 2] * h[dy + 2], n, a, zp, den_z, den_a, nq, aq);
                valid |= 1u << t;
                sw += w[t];
            }
        }
    }
    const bool keep = !open || !(sw > 0.0f);
    for (int j = 0; j < levels; j++) {
        const float* __restrict__ mj = m_in + (size_t)j * FB;
        float o = mj[p];
        if (!keep) {
            float s = 0.0f;
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    const int t = (dy + 2) * 5 + dx + 2;
                    if (valid & (1u << t)) s += w[t] * mj[(py + dy * step) * W + px + dx * step];
                }
            }
            o = s / sw;
        }
        mout[(size_t)j * FB + p] = o;
    }
}

// The argmin over the smoothed maps, the gathered picture and the workgroup's partial totals, partial[DE_SUMS b + k] = out[1 + k]'s
// share (k_de_final finishes them).  L = the levels of y, M = the smoothed maps.
__global__ __launch_bounds__(256) void k_ds_select(int FB, int levels, const float4* __restrict__ L, const float4* __restrict__ A,
                                                   const float* __restrict__ M, double floor, int* __restrict__ scale,
                                                   float* __restrict__ out3, double* __restrict__ partial) {
    double v[DE_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < (size_t)FB; p += (size_t)gridDim.x * 256) {
        const int state = ds_state(A[p].w);
        int best = state == 1 ? levels - 1 : 0;
        const float m0 = M[p];
        float mb = m0, mk = m0;
        if (state == 2) {
            for (int j = 1; j < levels; j++) {
                mk = M[(size_t)j * FB + p];
                if (mk < mb || (mb != mb && mk == mk)) { best = j; mb = mk; }
            }
        }
        const float4 c = L[(size_t)best * FB + p];
        scale[p] = best;
        dn_store3(out3, p, c.x, c.y, c.z);
        if (state == 0) continue;
        v[1] += 1.0;
        v[6] += (double)best;
        if (state == 1) { v[2] += 1.0; continue; }
        if (mb != 0.0f) {
            const double d = ds_luma4(c) + floor;
            v[0] += (double)mb / (d * d);
        }
        v[3] += (double)mb; v[4] += (double)mk; v[5] += (double)m0;
    }
    de_block_sum(v, partial + DE_SUMS * (size_t)blockIdx.x);
}

}  // namespace cl2
