// denoise_layers.hpp -- the a-trous filter of denoise.hpp over the layers of one render (cl2_denoise_layers).
//
// Layer l's colour is scrub(lacc[l] / accumulator row 3) and is filtered with its own sigma_color[l]; the normal, depth and
// albedo edge-stops are the ones of cl2_denoise.  Per pixel and layer every kernel below performs k_denoise_input's and
// k_denoise_pass's float operations on the same operands in the same order, so layer l is, byte for byte, what cl2_denoise
// returns on a handle whose accumulator rows 0..2 are lacc[l].  What the layers share is computed once:
//   per tap   f = (((h[dx] h[dy]) wn) wz) wa   depends on the features only: the feature buffers are read once per pixel and pass,
//             and wn, wz, wa with their two expf are computed once per tap.  The 25 factors stay in registers (the tap loops are
//             unrolled, every index is a constant) beside a 25-bit mask of the taps that are skipped.
//   per layer dn_compress, wc = expf(..) and the four sums, w = f * wc.
// The staged forms additionally keep x = dn_compress(c) of every tile entry in LDS, so the three divisions are done once per
// entry and layer instead of once per tap: the same function of the same operand, hence the same bits.
// No reference counterpart (the reference stops at the Monte Carlo estimate, src/renderer.py:293-316).
#pragma once
#include <hip/hip_runtime.h>
#include "denoise.hpp"

namespace cl2 {

struct LayerDen { float den_c[8]; };          // sigma_color[l]^2 * 4^-i per layer (CL2_MAX_LAYERS entries), host-computed

// k_denoise_input for layers l0 .. l0 + nl - 1: lacc is [L][3][FB], the weight is accumulator row 3.  Writes layer l's float4
// working buffer cout[l][FB], or the packed pictures out3[l - l0][FB][3] when no pass follows.
__global__ __launch_bounds__(BLOCK) void k_layers_input(int FB, int l0, int nl, const float* __restrict__ acc,
                                                        const float* __restrict__ lacc, float4* __restrict__ cout,
                                                        float* __restrict__ out3) {
    const int p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= FB) return;
    const float w = acc[3 * (size_t)FB + p];
#pragma unroll 1
    for (int l = l0; l < l0 + nl; l++) {
        float c[3];
        dn_input_colour(lacc + (size_t)3 * l * FB, (size_t)FB, (size_t)p, w, c);
        if (out3) dn_store3(out3, (size_t)(l - l0) * FB + p, c[0], c[1], c[2]);
        else cout[(size_t)l * FB + p] = make_float4(c[0], c[1], c[2], 0.0f);
    }
}

// One a-trous pass at step `step` (= 2^i) over layers l0 .. l0 + nl - 1: cin / cout are [L][FB] float4, out3 (last pass) is
// [nl][FB][3].  LDS_STEP as in k_denoise_pass.  Staged: the features of the tile and its halo once (2 x 16 B per entry), then per
// layer the colours with their compressed form (24 B per entry): 23 KB at step 1, 32 KB at step 2, five workgroups per CU.
// Every thread of the workgroup stages and meets the barriers; threads outside the frame compute nothing.
template <int LDS_STEP>
__global__ __launch_bounds__(DN_TILE * DN_TILE) void k_layers_denoise_pass(int W, int H, int step, int l0, int nl, LayerDen den,
                                                                            float sigma_depth, float den_a,
                                                                            const float4* __restrict__ cin,
                                                                            const float4* __restrict__ G0, const float4* __restrict__ G1,
                                                                            float4* __restrict__ cout, float* __restrict__ out3) {
    constexpr int T = DnTile<LDS_STEP>::T;
    __shared__ float4 s_n[T * T], s_a[T * T], s_c[T * T];      // s_c = (c.b, c.g, c.r, x.b)
    __shared__ float2 s_x[T * T];                              // (x.g, x.r), x = dn_compress(c)
    const int lx = threadIdx.x, ly = threadIdx.y;
    const int px = blockIdx.x * DN_TILE + lx, py = blockIdx.y * DN_TILE + ly;
    const int x0 = blockIdx.x * DN_TILE - 2 * LDS_STEP, y0 = blockIdx.y * DN_TILE - 2 * LDS_STEP;
    const size_t FB = (size_t)W * H;
    const bool inside = px < W && py < H;
    // the features of the tile once, by DnTile; the colours are staged per layer below, with their compressed form
    const DnTile<LDS_STEP> tile{W, H, px, py, G0, G1, s_n, s_a};
    tile.stage();
    if (!LDS_STEP && !inside) return;                           // the global form has no barrier
    const int p = inside ? py * W + px : 0;
    const int kp = tile.at(0, 0);

    // the layer-free part of the 25 tap weights, and the taps that count
    const float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float f[25];
    unsigned taps = 0;
    if (inside) {
        float4 np_, ap;
        tile.features(0, 0, np_, ap);
        if (ap.w != 0.0f) {
            const V3 n = v3(np_), a = v3(ap);
            const float zp = np_.w;
            const float den_z = (sigma_depth * zp) * (float)step;
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    const int t = (dy + 2) * 5 + dx + 2;
                    f[t] = 0.0f;
                    float4 nq, aq;
                    if (!tile.features(tile.offset(dx, step), tile.offset(dy, step), nq, aq)) continue;
                    if (aq.w == 0.0f) continue;
                    f[t] = dn_feature_weight(h[dx + 2] * h[dy + 2], n, a, zp, den_z, den_a, nq, aq);
                    taps |= 1u << t;
                }
            }
        }
    }

#pragma unroll 1
    for (int l = l0; l < l0 + nl; l++) {
        const float4* __restrict__ cl = cin + (size_t)l * FB;
        const float den_c = den.den_c[l];
        if (LDS_STEP) {
            if (l != l0) __syncthreads();                       // the previous layer's taps are read
            for (int k = ly * DN_TILE + lx; k < T * T; k += DN_TILE * DN_TILE) {
                const int gx = x0 + k % T, gy = y0 + k / T;
                float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (gx >= 0 && gx < W && gy >= 0 && gy < H) c = cl[gy * W + gx];
                const V3 x = dn_compress(c);
                s_c[k] = make_float4(c.x, c.y, c.z, x.x);
                s_x[k] = make_float2(x.y, x.z);
            }
            __syncthreads();
        }
        if (!inside) continue;
        float4 cp;
        V3 xp;
        if (LDS_STEP) {
            cp = s_c[kp];
            const float2 x = s_x[kp];
            xp = v3(cp.w, x.x, x.y);
        } else {
            cp = cl[p];
            xp = dn_compress(cp);
        }
        float o0 = cp.x, o1 = cp.y, o2 = cp.z;
        float sw = 0.0f, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int t = (dy + 2) * 5 + dx + 2;
                if (!((taps >> t) & 1u)) continue;
                float4 cq;
                V3 xq;
                if (LDS_STEP) {
                    const int k = tile.at(dx * LDS_STEP, dy * LDS_STEP);
                    cq = s_c[k];
                    const float2 x = s_x[k];
                    xq = v3(cq.w, x.x, x.y);
                } else {
                    cq = cl[(py + dy * step) * W + px + dx * step];      // in the frame: its bit of `taps` is set
                    xq = dn_compress(cq);
                }
                const V3 dxc = xp - xq;
                const float wc = expf(-dot(dxc, dxc) / den_c);
                const float w = f[t] * wc;
                sw += w;
                s0 += w * cq.x; s1 += w * cq.y; s2 += w * cq.z;
            }
        }
        // as k_denoise_pass: a weight sum that is not greater than 0 keeps the colour; a pixel without coverage has no taps
        if (sw > 0.0f) { o0 = s0 / sw; o1 = s1 / sw; o2 = s2 / sw; }
        if (out3) dn_store3(out3, (size_t)(l - l0) * FB + p, o0, o1, o2);
        else cout[(size_t)l * FB + p] = make_float4(o0, o1, o2, 0.0f);
    }
}

// S = F_0, then S = S + F_l in layer order: one float32 add per component.  `layers` is [L][n] packed pictures, n = 3 * W * H.
__global__ __launch_bounds__(BLOCK) void k_layers_sum(size_t n, int L, const float* __restrict__ layers, float* __restrict__ sum) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    float s = layers[i];
#pragma unroll 1
    for (int l = 1; l < L; l++) s = s + layers[(size_t)l * n + i];
    sum[i] = s;
}

}  // namespace cl2
