// adaptive.hpp -- adaptive sampling (cl2_set_sample_density / cl2_update_sample_density): camera slots are spread
// over the pixels by a density m, and every camera sample of pixel q enters the picture with the factor 1/m_q.
//
// Reference: generate_camera_rays takes the pixel of a slot from indices[id] (trace.metal:1034) and adaptive_finalize_samples
// gathers each pixel's slots through the CSR offsets sample_bin_offsets (:1007); renderer.py:89-94 fills both with the identity.
//
// Policy.  A PLANE is one sample stream's FB = W*H slots (entries s*FB + j).  The density m_q > 0 (mean 1) is quantised to
// integers M_q in units of 2^-16 with sum M = FB * 2^16 exactly (dens_quantise below); C = the inclusive prefix sum of M (uint64).
// Pass p, plane s draws the offset u = dens_offset(p, s) in [0, 2^16), and pixel q gets the slots
//     [ (C_{q-1} + u) >> 16, (C_q + u) >> 16 )
// of plane s: systematic sampling, so n_q is floor(m_q) or ceil(m_q), sum n = FB, E_u[n_q] = M_q / 2^16, a pixel's slots are
// contiguous and in raster order, and a flat density (M = 2^16 everywhere) maps slot j to pixel j.  Every camera-side addend of a
// slot of pixel q is scaled by invm_q = (float)(2^16 / M_q) -- filtered contribution and filtered weight alike -- so each plane's
// addend to each pixel has the expectation of a uniform pass; the light image (t = 1 splats, generated per slot from the slot's
// seed, independently of its pixel) is untouched.  One addend per pixel and plane: acc row 7 and the moments keep their meaning.
//
// Density from the error estimate (k_dens_terms / k_dens_from_terms): r_q = sqrt(var_L) / (L + floor), pixel q's term of
// e(floor) (error_estimate.hpp); 0 uncovered or var_L = 0; +inf (n < 2, L + floor = 0) and every term above KAPPA * mean(r) --
// mean over the finite terms -- clipped to KAPPA * mean(r); m_q = beta + (1 - beta) r_q / mean(r); mean(r) = 0 gives m = 1.
// Every reduction is per thread, per wave, per workgroup over a fixed grid and then one final launch (no float atomics): an update
// gives the same bytes on every call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.hpp"
#include "error_estimate.hpp"

namespace cl2 {

constexpr int DENS_SHIFT = 16;                    // density unit 2^-16
constexpr double DENS_KAPPA = 16.0;               // clip of the error terms, in units of their mean
constexpr int DENS_BLOCKS = 1024;                 // fixed grid of the reductions

// murmur3's 32-bit finaliser
__host__ __device__ __forceinline__ uint32_t dens_fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
// offset u in [0, 2^16) of pass `pass` (the handle's count of passes rendered with a density), plane s
__host__ __device__ __forceinline__ uint32_t dens_offset(uint32_t pass, uint32_t s) {
    return dens_fmix32(0x9E3779B9u * pass + s) >> 16;
}
// slots [lo, hi) of pixel q in a plane drawn with offset u
__device__ __forceinline__ void dens_range(const uint64_t* __restrict__ C, int q, uint32_t u, int& lo, int& hi) {
    const uint64_t c0 = q > 0 ? C[q - 1] : 0ull, c1 = C[q];
    lo = (int)((c0 + u) >> DENS_SHIFT);
    hi = (int)((c1 + u) >> DENS_SHIFT);
}

// ---- density from the error estimate ----
// r[q] (float32: +inf for a term to be clipped); partial[3 b + 0] = sum of the finite terms, [+1] = their count
__global__ __launch_bounds__(256) void k_dens_terms(int FB, const float* __restrict__ acc, const float* __restrict__ mom, double floor,
                                                    float* __restrict__ r, double* __restrict__ partial) {
    double v[3] = {0.0, 0.0, 0.0};
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < (size_t)FB; p += (size_t)gridDim.x * 256) {
        double var[4] = {0, 0, 0, 0}, L = 0.0;
        const int k = err_pixel(acc, mom, (size_t)FB, p, var, L);
        double t = 0.0;
        if (k == 1) t = __builtin_inf();
        else if (k == 2 && var[3] > 0.0) {
            t = sqrt(var[3]) / (L + floor);
            if (!(t >= 0.0) || !(t < __builtin_inf())) t = __builtin_inf();    // L + floor = 0 (or a NaN): clipped
        }
        const float tf = (float)t;
        r[p] = tf;
        if (tf < __builtin_inff()) { v[0] += (double)tf; v[1] += 1.0; }
    }
    err_block_sum3(v, partial + 3 * (size_t)blockIdx.x);
}

// out[0..2] = the sums of the n per-workgroup triples
__global__ __launch_bounds__(256) void k_dens_final(const double* __restrict__ partial, int n, double* __restrict__ out) {
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] += partial[3 * i + k];
    err_block_sum3(v, out);
}

// m[q] = beta + (1 - beta) min(r_q, KAPPA mean) / mean, in place; tot = {sum of finite terms, their count}
__global__ __launch_bounds__(256) void k_dens_from_terms(int FB, const double* __restrict__ tot, double beta, float* __restrict__ rm) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)FB) return;
    const double mean = tot[0] / tot[1];
    if (!(mean > 0.0)) { rm[p] = 1.0f; return; }
    const double clip = DENS_KAPPA * mean;
    double t = (double)rm[p];
    if (!(t <= clip)) t = clip;
    rm[p] = (float)(beta + (1.0 - beta) * (t / mean));
}

// ---- quantisation: M_q = 1 + F_q + extra_q, F_q = floor(m_q * scale) ----
// partial[3 b] = sum of m over the workgroup's pixels (fixed grid)
__global__ __launch_bounds__(256) void k_dens_sum(int FB, const float* __restrict__ m, double* __restrict__ partial) {
    double v[3] = {0.0, 0.0, 0.0};
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < (size_t)FB; p += (size_t)gridDim.x * 256) v[0] += (double)m[p];
    err_block_sum3(v, partial + 3 * (size_t)blockIdx.x);
}

// scale = FB (2^16 - 1) / sum m, shrunk by 2^-30 so that sum F <= FB (2^16 - 1) whatever the rounding of the double sum: the
// deficit D = FB (2^16 - 1) - sum F is >= 0 (one unit per pixel, up to a few more with FB near 2^26).  F -> M[q], sum F -> *fsum
// (integers: the order of the additions does not matter).
__global__ __launch_bounds__(256) void k_dens_floor(int FB, const float* __restrict__ m, const double* __restrict__ msum,
                                                    uint64_t* __restrict__ M, unsigned long long* __restrict__ fsum) {
    __shared__ unsigned long long s_wave[4];
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const double scale = ((double)FB * 65535.0 / msum[0]) * (1.0 - 0x1p-30);
    unsigned long long f = 0;
    if (p < (size_t)FB) {
        f = (unsigned long long)floor((double)m[p] * scale);
        M[p] = f;
    }
    for (int off = 32; off > 0; off >>= 1) f += __shfl_down(f, off);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = f;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(fsum, (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]));
}

// M[q] = 1 + F_q + extra_q with extra_q = floor((q+1) D / FB) - floor(q D / FB): the deficit spread evenly over the frame, one unit
// per pixel; invm[q] = (float)(2^16 / M_q).  (q+1) D < 2^53: no overflow.
__global__ __launch_bounds__(256) void k_dens_finish(int FB, uint64_t D, uint64_t* __restrict__ M, float* __restrict__ invm) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)FB) return;
    const uint64_t extra = ((uint64_t)(p + 1) * D) / (uint64_t)FB - ((uint64_t)p * D) / (uint64_t)FB;
    const uint64_t mq = 1ull + M[p] + extra;
    M[p] = mq;
    invm[p] = (float)(65536.0 / (double)mq);
}

// inclusive prefix sum of n uint64 (rocPRIM, det_splat.hip); tmp == nullptr: only sets tmp_bytes
hipError_t dens_scan(void* tmp, size_t& tmp_bytes, const uint64_t* in, uint64_t* out, size_t n, hipStream_t st);

// ---- expansion, once per pass: the slot -> pixel map of every plane (the reference's Ray.pixel_idx) ----
// one thread per (plane, pixel) entry; each writes its pixel's slots (at most ceil(m_q) of them)
__global__ __launch_bounds__(BLOCK) void k_dens_expand(int B, int FB, const uint64_t* __restrict__ C, uint32_t pass, int* __restrict__ map) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= B) return;
    const int s = e / FB, q = e - s * FB;
    int lo, hi;
    dens_range(C, q, dens_offset(pass, (uint32_t)s), lo, hi);
    int* plane = map + (size_t)s * FB;
    hi = hi < FB ? hi : FB;                          // C_{FB-1} = FB 2^16 makes hi <= FB; kept as a guard of the plane's bounds
    for (int j = lo; j < hi; j++) plane[j] = q;
}

// ---- K6 + process_images of a mapped pass (the counterpart of k_finalize_accumulate<MOMENTS>) ----
// Per pixel p and plane s: the 3x3 neighbours q in k_finalize_accumulate's (i, j) order; within a neighbour its slots in
// ascending order, each as (weight invm_q) agg; the unidirectional rows add invm_p scrub(uni) over p's own slots; row 7 += 1 per
// plane; moments and buckets as k_finalize_accumulate.  cam_count[p] += the camera samples p received (n_p summed over the planes).
// A flat density (invm = 1.0f, one slot per pixel: slot q) performs exactly the float operations of k_finalize_accumulate.
template <bool MOMENTS, bool BUCKETS = false>
__global__ __launch_bounds__(BLOCK) void k_finalize_accumulate_mapped(int B, int W, int H, const float* __restrict__ agg,
                                                                      float4* __restrict__ light_image, const float4* __restrict__ uni,
                                                                      float* __restrict__ acc, float* __restrict__ mom,
                                                                      const uint64_t* __restrict__ C, const float* __restrict__ invm,
                                                                      uint32_t pass, unsigned* __restrict__ cam_count,
                                                                      float* __restrict__ bkt, int M) {
    const int id = blockIdx.x * BLOCK + threadIdx.x;
    const int FB = W * H;
    if (id >= FB) return;
    float a[8], m[8];
#pragma unroll
    for (int c = 0; c < 8; c++) a[c] = acc[(size_t)c * FB + id];
    if constexpr (MOMENTS) {
#pragma unroll
        for (int c = 0; c < 8; c++) m[c] = mom[(size_t)c * FB + id];
    }
    const float inv_p = invm[id];
    unsigned received = 0;
    uint32_t s = 0;
#pragma unroll 1
    for (size_t base = 0; base < (size_t)B; base += (size_t)FB, s++) {
        const uint32_t u = dens_offset(pass, s);
        V3 total = v3(0, 0, 0);
        float wsum = 0.0f;
#pragma unroll 1
        for (int i = -1; i < 2; i++) {
#pragma unroll 1
            for (int j = -1; j < 2; j++) {
                const int sx = (id % W) + i, sy = (id / W) + j;
                if (sx < 0 || sx >= W || sy < 0 || sy >= H) continue;
                const int q = sy * W + sx;
                int lo, hi;
                dens_range(C, q, u, lo, hi);
                const float inv_q = invm[q];
                const size_t row = (size_t)((1 - i) * 3 + (1 - j)) * B;
                for (int slot = lo; slot < hi; slot++) {
                    const size_t k = base + (size_t)slot;
                    const float weight = agg[row + k] * inv_q;
                    total = total + weight * v3(agg[(size_t)9 * B + k], agg[(size_t)10 * B + k], agg[(size_t)11 * B + k]);
                    wsum += weight * agg[(size_t)12 * B + k];
                }
            }
        }
        const float4 l = light_image[base + id];
        const float x0 = scrub(l.x + total.x), x1 = scrub(l.y + total.y), x2 = scrub(l.z + total.z);
        const float w = wsum + l.w;
        a[0] += x0;
        a[1] += x1;
        a[2] += x2;
        a[3] += w;
        add_bucket<BUCKETS>(bkt, M, (size_t)FB, (size_t)id, a[7], x0, x1, x2, w);
        int lo, hi;
        dens_range(C, id, u, lo, hi);
        for (int slot = lo; slot < hi; slot++) {
            const float4 uv = uni[base + (size_t)slot];
            a[4] += inv_p * scrub(uv.x);
            a[5] += inv_p * scrub(uv.y);
            a[6] += inv_p * scrub(uv.z);
        }
        received += (unsigned)(hi - lo);
        a[7] += 1.0f;
        add_moments<MOMENTS>(m, x0, x1, x2, w);
        light_image[base + id] = make_float4(0, 0, 0, 0);
    }
#pragma unroll
    for (int c = 0; c < 8; c++) acc[(size_t)c * FB + id] = a[c];
    if constexpr (MOMENTS) {
#pragma unroll
        for (int c = 0; c < 8; c++) mom[(size_t)c * FB + id] = m[c];
    }
    cam_count[id] += received;
}

}  // namespace cl2
