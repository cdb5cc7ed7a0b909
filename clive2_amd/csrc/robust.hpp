// robust.hpp -- a firefly-robust picture of the render: a Gini-trimmed median of means over per-pixel buckets (after the G-MoN
// idea of Buisine et al., EGSR 2021; the formula below is this project's own statement).  The buckets are filled by the BUCKETS
// form of k_accumulate / k_finalize_accumulate (kernels.hpp) and k_finalize_accumulate_mapped (adaptive.hpp) while
// cl2_set_robust_buckets is on.
//
// No reference counterpart: the reference keeps first sums only (src/renderer.py:253-278).
//
// Buckets.  bkt [M][4][FB] float32, M = 3 .. 16: bucket k holds rows b, g, r, w.  An ADDEND (error_estimate.hpp) is (x_0, x_1,
// x_2, w), the very values added to accumulator rows 0 .. 3.  It goes to bucket
//     k = (int)a7 % M,        a7 = the pixel's row-7 value BEFORE this addend's += 1.0f (the addends the pixel had so far)
//     bkt[(4 k + c) FB + id] += x_c  (c = 0, 1, 2),      bkt[(4 k + 3) FB + id] += w
// one float32 add each, in stream order.  Row 7 counts addends, so it is >= 0 in every state the kernels make; a state written
// with a negative count gives a negative remainder, which is moved into 0 .. M-1 by adding M (a bound of the store, not a rule
// anybody should rely on).  acc and mom receive exactly the bytes they receive without buckets.
//
// Picture, per pixel, in float64 from the float32 sums unless stated, each operation in the order written:
//     bucket k is VALID iff W_k > 0 and W_k < +inf;  m = number of valid buckets
//     key_k = luma(X_0k / W_k, X_1k / W_k, X_2k / W_k)  (err_luma: (I_b 0.0722f + I_g 0.7152f) + I_r 0.2126f); a NaN key is +inf
//     rank the valid buckets by key ascending, equal keys in bucket order (rank_k = valid j with key_j < key_k, or equal and j < k)
//     over the ranks j = 1 .. m in order, v_j = key_(j) > 0 ? key_(j) : 0:   S += v_j,   N += (2 j - m - 1) v_j
//     G = 1 if S is NaN or +inf;  0 if !(S > 0);  else N / (m S), taken as 0 if !(G > 0) and as 1 if G > 1
//     c = min((int)floor(G m / 2), (m - 1) / 2)     (integer division in the second term: 0 for m < 3)
//     kept = the valid buckets with ranks c + 1 .. m - c
//     X_c, W = float32 sums over the kept buckets in ascending bucket index, from 0.0f;  pixel = scrub(X_c / W) in float32, BGR
//     m = 0: 0, 0, 0 (as `radiance`)
// Where the bucket means agree G is small and nothing is trimmed: the pixel is the ratio estimator over every valid bucket.  One
// bucket with a firefly raises G and is dropped together with the smallest one.
// Optional second output, per pixel: (float)G, (float)c  (0, 0 for m = 0).
#pragma once
#include <hip/hip_runtime.h>

namespace cl2 {

constexpr int ROBUST_MIN_BUCKETS = 3, ROBUST_MAX_BUCKETS = 16;

// the hook of the accumulate kernels: BUCKETS = false is the default path and adds no instruction (`bkt` is not read)
template <bool BUCKETS>
__device__ __forceinline__ void add_bucket(float* __restrict__ bkt, int M, size_t FB, size_t id, float a7, float x0, float x1,
                                           float x2, float w) {
    if constexpr (BUCKETS) {
        int k = (int)a7 % M;
        if (k < 0) k += M;
        float* b = bkt + (size_t)(4 * k) * FB + id;
        b[0] += x0;
        b[FB] += x1;
        b[2 * FB] += x2;
        b[3 * FB] += w;
    }
}

__device__ __forceinline__ double rb_luma(double b, double g, double r) {   // err_luma (error_estimate.hpp)
    return (b * (double)0.0722f + g * (double)0.7152f) + r * (double)0.2126f;
}

__device__ __forceinline__ float rb_scrub(float x) {   // scrub (kernels.hpp)
    return (x != x || __builtin_isinf(x)) ? 0.0f : x;
}

// The trim of one pixel: keys, ranks, Gini G and trim count c as the header states them.  Everything lives in registers: every loop
// over the buckets runs to ROBUST_MAX_BUCKETS with its index known at compile time and the test k < M inside, so nothing is indexed
// at run time and nothing goes to scratch -- in rb_trim and in every loop a caller writes over key[] and rank[].
struct RbTrim {
    double key[ROBUST_MAX_BUCKETS];       // 0.0 for an invalid bucket
    int rank[ROBUST_MAX_BUCKETS];         // 0-based; an invalid bucket has none: ROBUST_MAX_BUCKETS
    unsigned valid;                       // bit k: bucket k is valid
    int m, c;
    double G;
    __device__ __forceinline__ bool kept(int k) const { return rank[k] >= c && rank[k] < m - c; }      // invalid: rank >= m
};

__device__ __forceinline__ void rb_trim(const float* __restrict__ bkt, int M, size_t FB, size_t p, RbTrim& t) {
    constexpr int MAXM = ROBUST_MAX_BUCKETS;
    t.valid = 0;
    int m = 0;
#pragma unroll
    for (int k = 0; k < MAXM; k++) {
        t.key[k] = 0.0;
        if (k < M) {
            const float* b = bkt + (size_t)(4 * k) * FB + p;
            const double W = (double)b[3 * FB];
            if (W > 0.0 && W < __builtin_inf()) {
                const double q = rb_luma((double)b[0] / W, (double)b[FB] / W, (double)b[2 * FB] / W);
                t.key[k] = q != q ? __builtin_inf() : q;
                t.valid |= 1u << k;
                m++;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < MAXM; k++) {
        int n = 0;
#pragma unroll
        for (int j = 0; j < MAXM; j++)
            if (j != k && ((t.valid >> j) & 1u) && (t.key[j] < t.key[k] || (t.key[j] == t.key[k] && j < k))) n++;
        t.rank[k] = ((t.valid >> k) & 1u) ? n : MAXM;
    }
    double S = 0.0, N = 0.0;
#pragma unroll
    for (int j = 0; j < MAXM; j++) {
        if (j < m) {
            double q = 0.0;
#pragma unroll
            for (int k = 0; k < MAXM; k++) q = t.rank[k] == j ? t.key[k] : q;
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
    t.c = c < cmax ? c : cmax;
    t.m = m;
    t.G = G;
}

// the pixel of the robust picture: float32 sums over the kept buckets in ascending bucket index, divided and scrubbed; 0 at m = 0
__device__ __forceinline__ void rb_kept_colour(const float* __restrict__ bkt, size_t FB, size_t p, const RbTrim& t, float (&o)[3]) {
    float X0 = 0.0f, X1 = 0.0f, X2 = 0.0f, Wt = 0.0f;
#pragma unroll
    for (int k = 0; k < ROBUST_MAX_BUCKETS; k++) {
        if (t.kept(k)) {
            const float* b = bkt + (size_t)(4 * k) * FB + p;
            X0 += b[0];
            X1 += b[FB];
            X2 += b[2 * FB];
            Wt += b[3 * FB];
        }
    }
    o[0] = o[1] = o[2] = 0.0f;
    if (t.m > 0) { o[0] = rb_scrub(X0 / Wt); o[1] = rb_scrub(X1 / Wt); o[2] = rb_scrub(X2 / Wt); }
}

// One thread per pixel.  out (H, W, 3) float32; stats NULL or (H, W, 2) float32 = G, c.
__global__ __launch_bounds__(256) void k_robust_picture(size_t FB, int M, const float* __restrict__ bkt, float* __restrict__ out,
                                                        float2* __restrict__ stats) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= FB) return;
    RbTrim t;
    rb_trim(bkt, M, FB, p, t);
    float o[3];
    rb_kept_colour(bkt, FB, p, t, o);
    out[3 * p] = o[0];
    out[3 * p + 1] = o[1];
    out[3 * p + 2] = o[2];
    if (stats) stats[p] = make_float2((float)t.G, (float)t.c);
}

}  // namespace cl2
