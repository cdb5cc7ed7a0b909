// layers.hpp -- per-layer colour accumulators (cl2_set_layers): the layers of ONE render instead of one masked
// render per layer.
//
// While a layer table is set, k_connect_resolve<.., LAYERS = true> (connect_resolve.hpp) writes, beside the aggregator, the colour
// total of every layer's pairs to lay_agg[l][3][B], and the t = 1 colours of a layer go to the layer's own light image
// lay_light[l][B] (float4, .w unused): with float atomics from the resolve kernel, or in reproducible mode from the records by
// k_det_gather_layers below.  k_layers_accumulate then does for every layer what k_finalize_accumulate / k_finalize + k_accumulate
// (kernels.hpp) do for rows 0..2 of the accumulators.  Every float operation is the one a render with
// cl2_set_strategy_mask(mask of the layer) performs for those rows, on the same operands in the same order, so in reproducible
// mode lacc[l] holds the bytes of that render's rows 0..2.  No reference counterpart (src/trace.metal sums all pairs into one
// picture).
#pragma once
#include "kernels.hpp"

namespace cl2 {

// k_det_gather (kernels.hpp) with the layers' light images.  The main sum is k_det_gather's, statement for statement.  A record's
// slot is (s - 1) * B + source entry, so its pair (s, 1) and with it its layer follow from the slot: `row1` is the table's row of
// t = 1 (LayerCodes).  Layer l sums the colour of ITS records of the run, front to back.  The masked render's gather sums the whole
// run, in which the other records carry (+0, +0, +0): a sum that starts at +0 never holds -0 (x + -0 = x, and +0 + -0 = +0), so
// x + +0 = x at every step and skipping a record is the same as adding +0 for it.
__global__ __launch_bounds__(BLOCK) void k_det_gather_layers(const unsigned* __restrict__ keys, const unsigned* __restrict__ slots,
                                                             size_t n, const float4* __restrict__ vals,
                                                             float4* __restrict__ light_image, unsigned B, unsigned row1, int n_layers,
                                                             float4* __restrict__ lay_light) {
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned pix = keys[i];
    if (pix == ~0u) return;
    if (i > 0 && keys[i - 1] == pix) return;
    float4 acc = make_float4(0, 0, 0, 0);
    for (size_t j = i; j < n && keys[j] == pix; j++) {
        const float4 v = vals[slots[j]];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    float4 l = light_image[pix];
    l.x += acc.x; l.y += acc.y; l.z += acc.z; l.w += acc.w;
    light_image[pix] = l;
#pragma unroll 1
    for (int layer = 0; layer < n_layers; layer++) {
        float x = 0.0f, y = 0.0f, z = 0.0f;
        for (size_t j = i; j < n && keys[j] == pix; j++) {
            const unsigned slot = slots[j];
            if (((row1 >> (4u * (slot / B + 1u))) & 15u) != (unsigned)(layer + 1)) continue;
            const float4 v = vals[slot];
            x += v.x; y += v.y; z += v.z;
        }
        float4 q = lay_light[(size_t)layer * B + pix];
        q.x += x; q.y += y; q.z += z;
        lay_light[(size_t)layer * B + pix] = q;
    }
}

// One thread per PIXEL.  For each layer and each stream, in stream order, the statements of k_finalize_accumulate for rows 0..2:
// the nine filter weights are the main aggregator's rows 0..8 of the neighbours, total += weight * lay_agg[l] in the same (i, j)
// order, x = scrub(lay_light.c + total.c), lacc[l][c] += x; the layer's light image is zeroed for the next pass.  The main kernels
// are launched beside this one on the same stream and are not changed: they zero the main light image and only read `agg`.
// `B` = entries (streams x W x H, the stride of agg, lay_agg and lay_light), lacc is [L][3][W*H].
__global__ __launch_bounds__(BLOCK) void k_layers_accumulate(int B, int W, int H, int n_layers, const float* __restrict__ agg,
                                                             const float* __restrict__ lay_agg, float4* __restrict__ lay_light,
                                                             float* __restrict__ lacc) {
    const int id = blockIdx.x * BLOCK + threadIdx.x;
    const int FB = W * H;
    if (id >= FB) return;
#pragma unroll 1
    for (int l = 0; l < n_layers; l++) {
        const float* __restrict__ la = lay_agg + (size_t)3 * l * B;
        float4* __restrict__ ll = lay_light + (size_t)l * B;
        float* __restrict__ a = lacc + (size_t)3 * l * FB;
        float a0 = a[id], a1 = a[(size_t)FB + id], a2 = a[(size_t)2 * FB + id];
#pragma unroll 1
        for (size_t base = 0; base < (size_t)B; base += (size_t)FB) {
            V3 total = v3(0, 0, 0);
            // one row of three neighbours in flight at a time, as k_finalize_accumulate (unrolled all the way the nine gathers
            // take 136 VGPRs there)
#pragma unroll 1
            for (int i = -1; i < 2; i++) {
#pragma unroll
                for (int j = -1; j < 2; j++) {
                    const int sx = (id % W) + i, sy = (id / W) + j;
                    if (sx < 0 || sx >= W || sy < 0 || sy >= H) continue;
                    const size_t k = base + (size_t)sy * W + sx;
                    const float weight = agg[(size_t)((1 - i) * 3 + (1 - j)) * B + k];
                    total = total + weight * v3(la[k], la[(size_t)B + k], la[(size_t)2 * B + k]);
                }
            }
            const float4 li = ll[base + id];
            const float x0 = scrub(li.x + total.x), x1 = scrub(li.y + total.y), x2 = scrub(li.z + total.z);
            a0 += x0;
            a1 += x1;
            a2 += x2;
            ll[base + id] = make_float4(0, 0, 0, 0);
        }
        a[id] = a0; a[(size_t)FB + id] = a1; a[(size_t)2 * FB + id] = a2;
    }
}

}  // namespace cl2
