// tonemap_picture.hpp -- the log-average tone map of `camera.py:73-82` on the device for a KEPT PICTURE: (H, W, 3) float32 b, g, r
// in device memory (cl2_keep_picture, cl2_write_picture), the form in which the denoised, guided, robust and robust-guided pictures
// leave their last launch.  The arithmetic is tonemap.hpp's for picture 0 with the pixel itself in the place of v / w, and WITHOUT
// the scrub: the host path of these pictures, tone_map(picture), has none either, so a NaN pixel makes the log sum NaN and the
// picture all zero bytes, exactly as on the host.
//
//     base_c = (double)f_c,  luma = (base_b * 0.0722 + base_g * 0.7152) + base_r * 0.2126,  term = log(0.1 + luma)
//     pre_c = (double)(f_c * (float)exposure)   (a float32 product),  result = pre_c / Lw,  v = 255 * result / (result + wp^2)
//
// The sum is k_tone_logsum's tree unchanged (per-thread grid-stride sums in pixel order, the shuffle tree, (w0+w1)+(w2+w3)), and
// its second stage IS k_tone_logsum_final; both write the handle's d_tone_partial.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tonemap.hpp"

namespace cl2 {

__global__ __launch_bounds__(256) void k_picture_logsum(const float* __restrict__ pic, int FB, double* __restrict__ partial) {
    __shared__ double s_wave[4];
    double sum = 0.0;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < (size_t)FB; p += (size_t)gridDim.x * 256) {
        const double b = (double)pic[3 * p], g = (double)pic[3 * p + 1], r = (double)pic[3 * p + 2];
        const double luma = (b * 0.0722 + g * 0.7152) + r * 0.2126;     // np.sum(image * tone_vector, axis=2)
        sum += log(0.1 + luma);
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

// one value of the picture -> its byte: k_tone_apply's chain and cast
__device__ __forceinline__ unsigned picture_byte(float f, float exposure, double wp2, double Lw) {
    const double result = (double)(f * exposure) / Lw;
    const double v = 255.0 * result / (result + wp2);
    const int iv = (v > -2147483648.0 && v < 2147483648.0) ? (int)v : 0;
    return (unsigned)(iv & 0xFF);
}

// A byte depends on its own float alone (given Lw), so the picture is mapped as n = 3*W*H values, four to a thread: one 16-byte
// load, one 4-byte store per lane (both buffers come from hipMalloc: the float4 and uint32 views are aligned).  The last n % 4
// values are written byte by byte by the thread after the last full quad.
__global__ __launch_bounds__(256) void k_picture_apply(const float* __restrict__ pic, size_t n, float exposure, double wp2, double Lw,
                                                       uint8_t* __restrict__ out) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t e = 4 * q;
    if (e + 3 < n) {
        const float4 f = reinterpret_cast<const float4*>(pic)[q];
        reinterpret_cast<uint32_t*>(out)[q] = picture_byte(f.x, exposure, wp2, Lw) | (picture_byte(f.y, exposure, wp2, Lw) << 8) |
                                              (picture_byte(f.z, exposure, wp2, Lw) << 16) | (picture_byte(f.w, exposure, wp2, Lw) << 24);
    } else {
        for (size_t i = e; i < n; i++) out[i] = (uint8_t)picture_byte(pic[i], exposure, wp2, Lw);
    }
}

}  // namespace cl2
