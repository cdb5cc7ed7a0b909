// denoise_robust.hpp -- the robust picture (robust.hpp) as the input of the variance-guided filter (denoise_guided.hpp).  The
// guided filter fed from the moments counts a firefly in its variance, opens wide exactly there and spreads the firefly over the
// neighbourhood; the robust picture drops the firefly and leaves every other pixel its noise.  Here the filter takes the trimmed
// colour, and for its guide the variance of the mean of the KEPT buckets, which the firefly never entered.
//
// No reference counterpart (the reference keeps first sums only, src/renderer.py:253-278).  Reads the buckets bkt [M][4][FB] only:
// no accumulator, no moment; error tracking need not be on.  The passes are k_denoise_guided_pass<1|2|0>.
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

// One thread per pixel, registers only, as k_robust_picture: the trim and the colour are rb_trim and rb_kept_colour of robust.hpp.
// What is this kernel's own is the float64 sum of the kept keys and the between-bucket variance, in loops of rb_trim's form (to
// ROBUST_MAX_BUCKETS, compile-time indices).
__global__ __launch_bounds__(256) void k_denoise_robust_input(size_t FB, int M, const float* __restrict__ bkt, float4* __restrict__ cout,
                                                              float* __restrict__ out3, float* __restrict__ outv) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= FB) return;
    constexpr int MAXM = ROBUST_MAX_BUCKETS;
    RbTrim t;
    rb_trim(bkt, M, FB, p, t);
    float o[3];
    rb_kept_colour(bkt, FB, p, t, o);
    const int n = t.m - 2 * t.c;
    float v = 0.0f;
    if (t.m > 0) {
        v = DNG_VAR_CAP;
        if (n >= 2) {
            double sum = 0.0;
#pragma unroll
            for (int k = 0; k < MAXM; k++)
                if (t.kept(k)) sum += t.key[k];
            const double ybar = sum / (double)n;
            double Q = 0.0;
#pragma unroll
            for (int k = 0; k < MAXM; k++) {
                if (t.kept(k)) {
                    const double d = t.key[k] - ybar;
                    Q += d * d;
                }
            }
            v = dng_guide_variance(2, (Q / (double)(n - 1)) / (double)n);      // capped; a NaN takes the cap too
        }
    }
    if (out3) {
        dn_store3(out3, p, o[0], o[1], o[2]);
        if (outv) outv[p] = v;
    } else cout[p] = make_float4(o[0], o[1], o[2], v);
}

}  // namespace cl2
