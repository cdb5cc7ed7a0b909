// scene_layout.hpp -- record layouts and capacities that the kernels and the host-side scene preparation (scene_prep.hpp)
// share.  Plain C++ over the HIP vector types: no device code, so a host compiler reads it as well as hipcc.
#pragma once
#include <hip/hip_vector_types.h>

namespace cl2 {

constexpr int LDS_NODE_CAP = 512;   // records in the LDS window: at most 512 * 32 B = 16 KB
constexpr int LDS_TRI_CAP = 512;    // triangles staged in LDS when the whole scene has no more: at most 512 * 48 B = 24 KB
constexpr int LDS_TRI_PADS = 2;     // pad records behind the staged triangles: fetched by the flat walk, never tested (bvh_traverse.hpp)
constexpr int LEAF_PACK_MAX = 16;   // triangles per leaf record
constexpr int WIDE_EMPTY = (int)0x80000000;   // ref of an empty slot of a wide node (bvh_wide.hpp)
// Per-lane stack of the 4-wide walk (bvh_wide.hpp): the first WIDE_STACK_LDS entries in LDS, at most WIDE_STACK_OVERFLOW more in a
// per-lane global array that scene_prep.hpp's wide_overflow_entries sizes from the tree.
#ifndef CL2_WIDE_STACK_LDS
#define CL2_WIDE_STACK_LDS 8
#endif
constexpr int WIDE_STACK_LDS = CL2_WIDE_STACK_LDS;
constexpr int WIDE_STACK_OVERFLOW = 136;
constexpr int SHADE_LDS_CAP = 128; // shading triangles staged in LDS by the subpath kernel (64 B each)
constexpr int LDS_MAT_CAP = 32;     // materials staged in LDS by the subpath kernel

// The triangles of the camera quad (is_camera, scene.py): the t = 1 pairs ask whether the triangle their ray hit is one of
// them.  As a look-up in the shading records (tri_shade[4 i + 2].w) that was a dependent load -- a memory round trip of its
// own -- inside each of the six t = 1 pairs; the reference's scenes have two such triangles, which travel as kernel arguments.
// More than CAM_TRI_ARGS of them: n < 0 and the look-up stays.
constexpr int CAM_TRI_ARGS = 4;
struct CamTris { int n; int idx[CAM_TRI_ARGS]; };

struct CameraRec {   // byte-identical to struct Camera, trace.metal:72-85
    float center[4], focal_point[4], direction[4], dx[4], dy[4];
    int pixel_width, pixel_height;
    float phys_width, phys_height, h_fov, v_fov;
    int pad[2];
};

struct MaterialDev { float4 color_type; float4 emission_alpha; float ior; float pad[3]; };  // 48 B

// The slim resolve kernel (connect_resolve.hpp, k_connect_resolve_slim) keeps a light vertex's triangle and material byte in one
// 32-bit word, {triangle << 8 | material}: a triangle index, or the -1 of "no triangle", must survive the shift as a signed value.
constexpr int RESOLVE_SLIM_TRI_BITS = 23;
constexpr int resolve_pack_tri(int tri, int meta) { return (int)(((unsigned)tri << 8) | ((unsigned)meta & 0xFFu)); }
constexpr int resolve_packed_tri(int word) { return word >> 8; }
constexpr int resolve_packed_mat(int word) { return word & 0xFF; }
constexpr int RESOLVE_DEBUG_PARENT_BIT = 27;       // debug bit: launch k_connect_resolve where the slim kernel would run
// Which resolve kernel a pass launches: the slim one for the combinations it is built for -- material table in LDS, no slot map,
// no partial strategy mask, no layer table -- while every triangle index fits the packed word and the debug bit is clear.
inline bool resolve_runs_slim(long long n_tris, int n_mats, bool mapped, bool masked, bool layered, int debug_flags) {
    if (n_mats > LDS_MAT_CAP || mapped || masked || layered) return false;
    if ((debug_flags >> RESOLVE_DEBUG_PARENT_BIT) & 1) return false;
    return n_tris <= (1ll << RESOLVE_SLIM_TRI_BITS);
}

// The subpath kernel's static LDS: shading records and materials of small scenes (kernels.hpp, ShadeSrc).
struct ShadeLds {
    float4 tri_shade[4 * SHADE_LDS_CAP];
    MaterialDev mats[LDS_MAT_CAP];
};

}  // namespace cl2
