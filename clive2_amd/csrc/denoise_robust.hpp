// denoise_robust.hpp -- the robust picture (robust.hpp) as the input of the variance-guided filter (denoise_guided.hpp).  The
// guided filter fed from the moments counts a firefly in its variance, opens wide exactly there and spreads the firefly over the
// neighbourhood; the robust picture drops the firefly and leaves every other pixel its noise.  Here the filter takes the trimmed
// colour, and for its guide the variance of the mean of the KEPT buckets, which the firefly never entered.
//
// No reference counterpart (the reference keeps first sums only, src/renderer.py:253-278).  Reads the buckets bkt [M][4][FB] only:
// no accumulator, no moment; error tracking need not be on.  The passes are k_denoise_guided_pass<1|2|0>, unchanged.
//
// Input per pixel p, from the float32 bucket sums:
//     trim      valid, key_k (float64, a NaN key is +inf), ranks, m, G, c and the kept set exactly as robust.hpp states them
//     colour    c_p = the pixel of k_robust_picture, byte for byte: float32 sums over the kept buckets in ascending bucket index,
//               divided and scrubbed; 0, 0, 0 at m = 0
//     variance  n = m - 2 c, the number of kept buckets
//               v_p = 0       for m = 0
//               v_p = 2^100   for n < 2  (DNG_VAR_CAP)
//               otherwise, in float64 over the kept buckets in ascending bucket index:
//                   ybar = (sum key_k) / (double)n
//                   Q    = sum (key_k - ybar) (key_k - ybar)
//                   var  = (Q / (double)(n - 1)) / (double)n
//               v_p = var < 2^100 ? (float)var : 2^100        (a NaN or inf from a +inf key takes the cap)
// v is the between-bucket variance of the mean of the kept bucket lumas.  It ignores that the buckets' weights differ: it is a
// filter guide, like v' of denoise_guided.hpp, and nothing may stop on it.
// (c, v) go out as k_denoise_guided_input writes them: float4 {c.b, c.g, c.r, v}, or the packed picture and, if asked, v when no
// pass follows.  tests/robust_denoise_reference.py restates every operation in numpy, in the same order.
#pragma once
#include <hip/hip_runtime.h>
#include "denoise_guided.hpp"
#include "robust.hpp"

namespace cl2 {

// One thread per pixel, registers only, as k_robust_picture: every loop over the buckets runs to ROBUST_MAX_BUCKETS with its index
// known at compile time and the test k < M inside.  The trim is restated here, operation for operation, so that k_robust_picture's
// instructions stay what they are.
__global__ __launch_bounds__(256) void k_denoise_robust_input(size_t FB, int M, const float* __restrict__ bkt, float4* __restrict__ cout,
                                                              float* __restrict__ out3, float* __restrict__ outv) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= FB) return;
    constexpr int MAXM = ROBUST_MAX_BUCKETS;
    double key[MAXM];
    unsigned valid = 0;
    int m = 0;
#pragma unroll
    for (int k = 0; k < MAXM; k++) {
        key[k] = 0.0;
        if (k < M) {
            const float* b = bkt + (size_t)(4 * k) * FB + p;
            const double W = (double)b[3 * FB];
            if (W > 0.0 && W < __builtin_inf()) {
                const double q = rb_luma((double)b[0] / W, (double)b[FB] / W, (double)b[2 * FB] / W);
                key[k] = q != q ? __builtin_inf() : q;
                valid |= 1u << k;
                m++;
            }
        }
    }
    int rank[MAXM];
#pragma unroll
    for (int k = 0; k < MAXM; k++) {
        int n = 0;
#pragma unroll
        for (int j = 0; j < MAXM; j++)
            if (j != k && ((valid >> j) & 1u) && (key[j] < key[k] || (key[j] == key[k] && j < k))) n++;
        rank[k] = ((valid >> k) & 1u) ? n : MAXM;                 // 0-based; an invalid bucket has no rank
    }
    double S = 0.0, N = 0.0;
#pragma unroll
    for (int j = 0; j < MAXM; j++) {
        if (j < m) {
            double q = 0.0;
#pragma unroll
            for (int k = 0; k < MAXM; k++) q = rank[k] == j ? key[k] : q;
            const double v = q > 0.0 ? q : 0.0;
            S += v;
            N += (double)(2 * (j + 1) - m - 1) * v;
        }
    }
    double G;
    if (S != S || S == __builtin_inf()) G = 1.0;
    else if (!(S > 0.0)) G = 0.0;
    else {
        G = N / ((double)m * S);
        G = !(G > 0.0) ? 0.0 : (G > 1.0 ? 1.0 : G);
    }
    int c = (int)floor(G * (double)m / 2.0);
    const int cmax = m > 0 ? (m - 1) / 2 : 0;
    c = c < cmax ? c : cmax;
    float X0 = 0.0f, X1 = 0.0f, X2 = 0.0f, Wt = 0.0f;
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < MAXM; k++) {
        if (rank[k] >= c && rank[k] < m - c) {                    // invalid: rank MAXM >= m
            const float* b = bkt + (size_t)(4 * k) * FB + p;
            X0 += b[0];
            X1 += b[FB];
            X2 += b[2 * FB];
            Wt += b[3 * FB];
            sum += key[k];
        }
    }
    float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
    if (m > 0) { o0 = rb_scrub(X0 / Wt); o1 = rb_scrub(X1 / Wt); o2 = rb_scrub(X2 / Wt); }
    const int n = m - 2 * c;
    float v = 0.0f;
    if (m > 0) {
        v = DNG_VAR_CAP;
        if (n >= 2) {
            const double ybar = sum / (double)n;
            double Q = 0.0;
#pragma unroll
            for (int k = 0; k < MAXM; k++) {
                if (rank[k] >= c && rank[k] < m - c) {
                    const double d = key[k] - ybar;
                    Q += d * d;
                }
            }
            const double var = (Q / (double)(n - 1)) / (double)n;
            v = var < (double)DNG_VAR_CAP ? (float)var : DNG_VAR_CAP;      // a NaN takes the cap too
        }
    }
    if (out3) {
        out3[3 * p] = o0; out3[3 * p + 1] = o1; out3[3 * p + 2] = o2;
        if (outv) outv[p] = v;
    } else cout[p] = make_float4(o0, o1, o2, v);
}

}  // namespace cl2
