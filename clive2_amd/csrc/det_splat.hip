// det_splat.hip -- the rocPRIM calls of the library: the radix sort of the reproducible light image (det_splat.hpp) and the
// prefix sum of the sample density (adaptive.hpp); their own translation unit so that renderer_api.hip does not have to parse
// rocPRIM.
#include <cstring>
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "det_splat.hpp"
#include <stdint.h>

namespace cl2 {

hipError_t det_sort_pairs(void* tmp, size_t& tmp_bytes, const unsigned* keys_in, unsigned* keys_out, const unsigned* slots_in,
                          unsigned* slots_out, size_t n, unsigned end_bit, hipStream_t st) {
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, keys_in, keys_out, slots_in, slots_out, n, 0u, end_bit, st);
}

hipError_t dens_scan(void* tmp, size_t& tmp_bytes, const uint64_t* in, uint64_t* out, size_t n, hipStream_t st) {
    return rocprim::inclusive_scan(tmp, tmp_bytes, in, out, n, rocprim::plus<uint64_t>(), st);
}

}  // namespace cl2
