// scene_prep_driver.cpp -- a host-compiler build of clive2_amd/csrc/scene_prep.hpp, the scene preparation behind
// cl2_upload_scene, for tests/test_scene_prep_cpu.py (ctypes).  Nothing of the product library is linked.
#include "../clive2_amd/csrc/scene_prep.hpp"

#include <cstdio>
#include <cstring>

using cl2::PreparedScene;

extern "C" {

// The prepared scene, or nullptr with the refusal in msg.  Arguments as cl2_upload_scene's, plus the renderer's frame size.
void* sp_prepare(const void* boxes, int n_boxes, const void* tris, int n_tris, const void* mats, int n_mats, const void* camera,
                 const void* light_tris, const float* light_areas, const int32_t* light_tri_index, int light_count, int W, int H,
                 char* msg, int msg_len) {
    auto* s = new PreparedScene;
    const std::string err = cl2::prepare_scene(boxes, n_boxes, tris, n_tris, mats, n_mats, camera, light_tris, light_areas,
                                               light_tri_index, light_count, W, H, *s);
    if (err.empty()) return s;
    delete s;
    std::snprintf(msg, msg_len, "%s", err.c_str());
    return nullptr;
}

// Bytes of the named array (-1: no such name); *data points at them.
long long sp_array(void* h, const char* name, const void** data) {
    const PreparedScene& s = *static_cast<PreparedScene*>(h);
    auto out = [&](const auto& v) { *data = v.data(); return (long long)(v.size() * sizeof(v[0])); };
    if (!std::strcmp(name, "nodes")) return out(s.nodes);
    if (!std::strcmp(name, "fast")) return out(s.fast);
    if (!std::strcmp(name, "wide")) return out(s.wide);
    if (!std::strcmp(name, "tris")) return out(s.tris);
    if (!std::strcmp(name, "tris36")) return out(s.tris36);
    if (!std::strcmp(name, "shade")) return out(s.shade);
    if (!std::strcmp(name, "ltris")) return out(s.ltris);
    if (!std::strcmp(name, "mats")) return out(s.mats);
    if (!std::strcmp(name, "tri_rank")) return out(s.tri_rank);
    if (!std::strcmp(name, "cam_tris")) { *data = &s.cam_tris; return sizeof s.cam_tris; }
    return -1;
}

int sp_scalar(void* h, const char* name) {
    const PreparedScene& s = *static_cast<PreparedScene*>(h);
    if (!std::strcmp(name, "n_records")) return s.n_records;
    if (!std::strcmp(name, "n_top")) return s.n_top;
    if (!std::strcmp(name, "n_fast")) return s.n_fast;
    if (!std::strcmp(name, "fast_flat")) return s.fast_flat;
    if (!std::strcmp(name, "n_wide")) return s.n_wide;
    if (!std::strcmp(name, "max_pending")) return s.max_pending;
    if (!std::strcmp(name, "order_depth")) return s.order_depth;
    return -1;
}

// cl2::wide_overflow_entries and the two capacities it works with
int sp_wide_overflow_entries(int max_pending, int order_depth, int order) { return cl2::wide_overflow_entries(max_pending, order_depth, order); }
int sp_wide_stack_lds() { return cl2::WIDE_STACK_LDS; }
int sp_wide_stack_overflow() { return cl2::WIDE_STACK_OVERFLOW; }

void sp_free(void* h) { delete static_cast<PreparedScene*>(h); }

}  // extern "C"
