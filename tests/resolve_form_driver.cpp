// The host-side rule that picks the resolve kernel of a pass (clive2_amd/csrc/scene_layout.hpp: resolve_runs_slim), built with g++
// for tests/test_resolve_form_cpu.py -- no GPU, and nothing of the hipcc-built library.
#include "../clive2_amd/csrc/scene_layout.hpp"

extern "C" {
int rf_runs_slim(long long n_tris, int n_mats, int mapped, int masked, int layered, int debug_flags) {
    return cl2::resolve_runs_slim(n_tris, n_mats, mapped != 0, masked != 0, layered != 0, debug_flags) ? 1 : 0;
}
int rf_tri_bits() { return cl2::RESOLVE_SLIM_TRI_BITS; }
int rf_parent_bit() { return cl2::RESOLVE_DEBUG_PARENT_BIT; }
int rf_mat_cap() { return cl2::LDS_MAT_CAP; }
// the packed word of a light vertex as the slim kernel builds and reads it
int rf_pack(int tri, int meta) { return cl2::resolve_pack_tri(tri, meta); }
int rf_packed_tri(int word) { return cl2::resolve_packed_tri(word); }
int rf_packed_mat(int word) { return cl2::resolve_packed_mat(word); }
}
