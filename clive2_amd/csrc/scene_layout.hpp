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
constexpr int SHADE_LDS_CAP = 128;  // shading triangles staged in LDS by the subpath kernel (64 B each)
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

// The subpath kernel's static LDS: shading records and materials of small scenes (kernels.hpp, ShadeSrc).
struct ShadeLds {
    float4 tri_shade[4 * SHADE_LDS_CAP];
    MaterialDev mats[LDS_MAT_CAP];
};

}  // namespace cl2
