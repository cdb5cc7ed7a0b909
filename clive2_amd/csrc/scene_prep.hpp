// scene_prep.hpp -- the host half of cl2_upload_scene: validates the caller's reference arrays (src/struct_types.py) and builds
// every device record from them.  Standard library only, no HIP runtime call and no device code, so the stages run and are
// tested on a CPU (tests/test_scene_prep_cpu.py); cl2_upload_scene only copies the result to the device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "scene_layout.hpp"

namespace cl2 {

// Reference AoS records as the host hands them over (src/struct_types.py).
struct BoxRec { float min[4], max[4]; int32_t left, right, pad[2]; };
struct TriRec { float v0[4], v1[4], v2[4], n0[4], n1[4], n2[4], normal[4]; int32_t material, is_light, is_camera, pad; };
struct MatRec { float color[4], emission[4]; int32_t type; float alpha, ior; int32_t pad; };
static_assert(sizeof(BoxRec) == 48 && sizeof(TriRec) == 128 && sizeof(MatRec) == 48 && sizeof(CameraRec) == 112, "ABI");

// What cl2_upload_scene copies to the device (layouts: bvh_traverse.hpp, bvh_wide.hpp, kernels.hpp); fast, wide, tris36 and
// tri_rank are empty when the scene has no pruned table / no 4-wide collapse.
struct PreparedScene {
    std::vector<float4> nodes, fast, wide, tris, shade, ltris;
    std::vector<float> tris36;
    std::vector<MaterialDev> mats;
    std::vector<int> tri_rank;
    int n_records = 0, n_top = 0, n_fast = 0, fast_flat = 0, n_wide = 0, max_pending = 0;
    int order_depth = 0;                 // deepest stack of the 4-wide walk in ANY child order (build_wide); 0 without a collapse
    CamTris cam_tris{0, {0, 0, 0, 0}};
    CameraRec cam{};
};

namespace prep {

inline float as_f(int32_t i) { float f; std::memcpy(&f, &i, 4); return f; }

struct Scene {                       // the caller's arrays, typed
    const BoxRec* boxes; int n_boxes;
    const TriRec* tris; int n_tris;
    const MatRec* mats; int n_mats;
    const TriRec* ltris; const int32_t* light_tri_index; int light_count;
};

// Per box: records of its subtree, its first record in visit order, entries pending under it on the reference's stack; and
// renum: visit-order record -> record number ([n_records] = n_records).  A leaf of more than LEAF_PACK_MAX triangles takes more records.
struct Order { std::vector<int> subtree, rec_index, pending, renum; };

inline int leaf_records(const BoxRec& b) { return (b.right - b.left + LEAF_PACK_MAX - 1) / LEAF_PACK_MAX; }

// 1. argument counts and the camera
inline std::string check_arguments(const void* boxes, int n_boxes, const void* tris, int n_tris, const void* mats, int n_mats,
                                   const void* camera, const void* light_tris, const float* light_areas,
                                   const int32_t* light_tri_index, int light_count, int W, int H, CameraRec& cam) {
    if (!boxes || !tris || !mats || !camera || !light_tris || !light_areas || !light_tri_index) return "NULL scene array";
    if (n_boxes < 1 || n_tris < 1 || light_count < 1) return "scene needs >=1 box, triangle and light";
    if (n_tris >= (1 << 27)) return "at most 2^27 triangles (leaf records pack begin<<4 | count-1)";
    // material 7 is hard-wired into the camera vertices (trace.metal:611, :1053); at most 256 fit the packed meta word
    if (n_mats < 8 || n_mats > 256) return "material table must have 8..256 entries";
    std::memcpy(&cam, camera, sizeof cam);
    if (cam.pixel_width != W || cam.pixel_height != H) return "camera resolution differs from the renderer's";
    return "";
}

// 2. the tree: every index in range, children after their parent (breadth-first numbering, src/bvh.py:345-351) and every box
// reached exactly once -- which also guarantees that the stackless walk terminates
inline std::string check_tree(const Scene& s) {
    std::vector<char> reached(s.n_boxes, 0);
    reached[0] = 1;
    for (int i = 0; i < s.n_boxes; i++) {
        const BoxRec& b = s.boxes[i];
        if (!reached[i]) return "box " + std::to_string(i) + " is not reachable from the root";
        if (b.right == 0) {
            if (b.left <= i || b.left + 1 >= s.n_boxes) return "inner box child index out of order/range";
            if (reached[b.left] || reached[b.left + 1]) return "box has two parents";
            reached[b.left] = reached[b.left + 1] = 1;
        } else {
            if (b.left < 0 || b.right > s.n_tris || b.left >= b.right) return "leaf triangle range out of range";
        }
    }
    return "";
}

// 3. visit order (node, right subtree, left subtree = the reference's pop order, trace.metal:150-160), subtree sizes in records
// and pending stack depths.  The reference's loop runs `while (stack_ptr > 0 && stack_ptr < 64)` (trace.metal:149): a walk that
// enters an inner box with 62 entries pending pushes to 64 and ENDS there, whatever is still unvisited (quirk Q18).  The
// stackless walk has no such limit, so a tree that could reach it is refused instead of being rendered differently; the
// reference's builder stops splitting at 32 pending boxes (bvh.py:294, Q13), far below.
inline std::string visit_order(const Scene& s, Order& o) {
    o.subtree.assign(s.n_boxes, 0);
    for (int i = s.n_boxes - 1; i >= 0; i--) {          // children have larger indices than their parent
        const BoxRec& b = s.boxes[i];
        o.subtree[i] = b.right == 0 ? 1 + o.subtree[b.left] + o.subtree[b.left + 1] : leaf_records(b);
    }
    o.rec_index.assign(s.n_boxes, -1);
    o.pending.assign(s.n_boxes, 0);
    o.rec_index[0] = 0;
    for (int i = 0; i < s.n_boxes; i++) {                // parents before children: their record index is known
        const BoxRec& b = s.boxes[i];
        if (b.right == 0) {
            if (o.pending[i] + 2 >= 64)
                return "tree too deep: the reference's 64-entry traversal stack would overflow at box " + std::to_string(i);
            o.rec_index[b.left + 1] = o.rec_index[i] + 1;                          // right child: adjacent
            o.rec_index[b.left] = o.rec_index[i] + 1 + o.subtree[b.left + 1];      // left child: after the right subtree
            o.pending[b.left + 1] = o.pending[i] + 1;                              // popped first, its sibling waits below it
            o.pending[b.left] = o.pending[i];
        }
    }
    return "";
}

// 4. record numbering.  Small trees: plain visit order.  Trees larger than the LDS window: the boxes of the TOP levels (the
// reference array is breadth-first, so a prefix of it) are numbered first, [0, n_top), so that the window staged in LDS holds
// the records every ray visits; the rest keep their visit order behind them.  Links are explicit (skip, and the right child in
// `info`), so the numbering has no influence on the walk.
inline int number_records(const Scene& s, int n_records, Order& o) {
    int n_top = 0;
    while (n_records > LDS_NODE_CAP && n_top < s.n_boxes && n_top < LDS_NODE_CAP &&
           (s.boxes[n_top].right == 0 || leaf_records(s.boxes[n_top]) == 1)) n_top++;
    o.renum.assign((size_t)n_records + 1, 0);
    std::vector<char> is_top((size_t)n_records, 0);
    for (int i = 0; i < n_top; i++) is_top[o.rec_index[i]] = 1;
    int tops_before = 0;
    for (int k = 0; k < n_records; k++) {
        if (is_top[k]) { tops_before++; continue; }
        o.renum[k] = n_top + k - tops_before;
    }
    for (int i = 0; i < n_top; i++) o.renum[o.rec_index[i]] = i;
    o.renum[n_records] = n_records;
    return n_top;
}

// 5. material and light indices
inline std::string check_indices(const Scene& s) {
    for (int t = 0; t < s.n_tris; t++)
        if (s.tris[t].material < 0 || s.tris[t].material >= s.n_mats) return "triangle material index out of range";
    for (int l = 0; l < s.light_count; l++) {
        if (s.light_tri_index[l] < 0 || s.light_tri_index[l] >= s.n_tris) return "light triangle index out of range";
        if (s.ltris[l].material < 0 || s.ltris[l].material >= s.n_mats) return "light material index out of range";
    }
    return "";
}

// 6. 4-wide collapse for the exact wide walk (bvh_wide.hpp).  Conditions: the root is an inner box, every box nests its children
// exactly (what the exactness argument rests on; true for trees that np_flatten_bvh or either native builder made, not guaranteed
// for hand-made Box[] arrays) and no leaf exceeds one record.  Returns whether the boxes nest that way.
// order_depth: a walk that stands at a wide node has left at most (slots - 1) of each node on its path on the stack, whichever slot
// it took first and whichever boxes passed, so D(node) = (slots - 1) + max over the node's inner slots of D(slot), D(leaf) = 0, bounds
// the stack of the walk in any child order (the nearest-first walk's bound: wide_overflow_entries).
inline bool build_wide(const Scene& s, PreparedScene& out) {
    const BoxRec* boxes = s.boxes;
    bool ok = s.n_boxes >= 3 && boxes[0].right == 0;
    auto inside = [&](const BoxRec& c, const BoxRec& p) {
        for (int k = 0; k < 3; k++) if (!(c.min[k] >= p.min[k] && c.max[k] <= p.max[k])) return false;
        return true;
    };
    for (int i = 0; i < s.n_boxes && ok; i++) {
        const BoxRec& b = boxes[i];
        if (b.right == 0) ok = inside(boxes[b.left], b) && inside(boxes[b.left + 1], b);
        else ok = (b.right - b.left) <= LEAF_PACK_MAX;
    }
    if (!ok) return false;
    // slots of reference box x in its visit order: child left+1 first, each inner child replaced by its children
    auto slots_of = [&](int x, int* sl) {
        int n = 0;
        for (int c : {boxes[x].left + 1, boxes[x].left}) {
            if (boxes[c].right != 0) sl[n++] = c;
            else { sl[n++] = boxes[c].left + 1; sl[n++] = boxes[c].left; }
        }
        return n;
    };
    std::vector<int> wide_of(s.n_boxes, -1), order;
    order.push_back(0); wide_of[0] = 0;
    for (size_t h = 0; h < order.size(); h++) {
        int sl[4];
        const int n = slots_of(order[h], sl);
        for (int k = 0; k < n; k++)
            if (boxes[sl[k]].right == 0) { wide_of[sl[k]] = (int)order.size(); order.push_back(sl[k]); }
    }
    out.n_wide = (int)order.size();
    out.wide.assign((size_t)8 * out.n_wide, make_float4(0, 0, 0, 0));
    for (int wn = 0; wn < out.n_wide; wn++) {
        int sl[4];
        const int n = slots_of(order[wn], sl);
        float v[6][4];
        int ref[4];
        for (int k = 0; k < 4; k++) {
            ref[k] = WIDE_EMPTY;
            // an empty slot holds a box at +inf: for a ray with finite 1/d its slab test gives tmin = +inf or tmax = -inf,
            // so `tmin <= tmax && tmin < best_t` fails without the walk looking at the reference (bvh_wide.hpp)
            for (int c = 0; c < 6; c++) v[c][k] = std::numeric_limits<float>::infinity();
            if (k >= n) continue;
            const BoxRec& b = boxes[sl[k]];
            for (int c = 0; c < 3; c++) { v[c][k] = b.min[c]; v[3 + c][k] = b.max[c]; }
            ref[k] = b.right == 0 ? wide_of[sl[k]] : ~((b.left << 4) | (b.right - b.left - 1));
        }
        for (int c = 0; c < 6; c++) out.wide[(size_t)8 * wn + c] = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        out.wide[(size_t)8 * wn + 6] = make_float4(as_f(ref[0]), as_f(ref[1]), as_f(ref[2]), as_f(ref[3]));
    }
    std::vector<int> depth((size_t)out.n_wide, 0);
    for (int wn = out.n_wide - 1; wn >= 0; wn--) {                  // breadth-first numbering: a node's inner slots come after it
        int sl[4];
        const int n = slots_of(order[wn], sl);
        int below = 0;
        for (int k = 0; k < n; k++) if (boxes[sl[k]].right == 0) below = std::max(below, depth[wide_of[sl[k]]]);
        depth[wn] = n - 1 + below;
    }
    out.order_depth = depth[0];
    return true;
}

// 7. node records (bvh_traverse.hpp): inner info = ~(record of the right child, visited first), negative; a leaf of more than
// LEAF_PACK_MAX triangles continues in follow-up records with an unbounded box, so they are always entered
inline void pack_nodes(const Scene& s, const Order& o, PreparedScene& out) {
    const float inf = std::numeric_limits<float>::infinity();
    out.nodes.resize(2 * (size_t)out.n_records);
    for (int i = 0; i < s.n_boxes; i++) {
        const BoxRec& b = s.boxes[i];
        const int k = o.rec_index[i], skip = o.renum[k + o.subtree[i]];
        if (b.right == 0) {
            out.nodes[2 * (size_t)o.renum[k]] = make_float4(b.min[0], b.min[1], b.min[2], as_f(skip));
            out.nodes[2 * (size_t)o.renum[k] + 1] = make_float4(b.max[0], b.max[1], b.max[2], as_f(~o.renum[k + 1]));
            continue;
        }
        int begin = b.left;
        for (int part = 0; begin < b.right; part++, begin += LEAF_PACK_MAX) {
            const int count = std::min(LEAF_PACK_MAX, b.right - begin);
            const int info = (begin << 4) | (count - 1);
            const int nxt = o.renum[k + part + 1];
            out.nodes[2 * (size_t)o.renum[k + part]] = part == 0 ? make_float4(b.min[0], b.min[1], b.min[2], as_f(nxt))
                                                                 : make_float4(-inf, -inf, -inf, as_f(nxt));
            out.nodes[2 * (size_t)o.renum[k + part] + 1] = part == 0 ? make_float4(b.max[0], b.max[1], b.max[2], as_f(info))
                                                                     : make_float4(inf, inf, inf, as_f(info));
        }
    }
}

// 8a. pruned table for the LDS-resident walk.  For a ray with finite 1/d an inner box's test can only prune (same argument as the
// wide walk: a child that passes its test implies its parent passed), so an inner record may be dropped and its children visited
// unconditionally without changing any hit.  A record is dropped when the test is expected to cost more than it saves:
// (1 - area / area of the nearest tested ancestor) x cost of the subtree < 1 box test, the surface-area estimate of the chance
// that a ray that reached the ancestor misses this box.  The Cornell box loses its root and its one other inner box (both span
// the room): 3 box tests per ray instead of 5.  Rays with a non-finite 1/d, and the counting mode, walk the full table.
// fast_flat: the table holds leaves only, each skip link pointing at the next record, so all rays visit the same records in the
// same order and the walk's control flow can be wave-uniform (closest_hit_flat).
inline void build_fast(const Scene& s, const Order& o, PreparedScene& out) {
    const BoxRec* boxes = s.boxes;
    const int n_records = out.n_records;
    auto area = [&](const BoxRec& b) {
        const double x = (double)b.max[0] - b.min[0], y = (double)b.max[1] - b.min[1], z = (double)b.max[2] - b.min[2];
        return 2.0 * (x * y + y * z + z * x);
    };
    std::vector<double> cost(s.n_boxes, 0.0), anc_area(s.n_boxes, 0.0);
    for (int i = s.n_boxes - 1; i >= 0; i--) {
        const BoxRec& b = boxes[i];
        cost[i] = b.right == 0 ? 1.0 + cost[b.left] + cost[b.left + 1] : 1.0 + 2.5 * (b.right - b.left);
    }
    std::vector<char> dropped((size_t)n_records + 1, 0);
    anc_area[0] = area(boxes[0]);
    for (int i = 0; i < s.n_boxes; i++) {
        const BoxRec& b = boxes[i];
        if (b.right != 0) continue;
        const double a = area(b);
        const double p_miss = anc_area[i] > 0.0 ? std::max(0.0, 1.0 - a / anc_area[i]) : 0.0;
        const bool drop = p_miss * (cost[i] - 1.0) < 1.0;
        dropped[o.rec_index[i]] = drop ? 1 : 0;
        anc_area[b.left] = anc_area[b.left + 1] = drop ? anc_area[i] : a;
    }
    int n_fast = 0;
    std::vector<int> fast_index((size_t)n_records + 1);
    for (int k = 0; k <= n_records; k++) { fast_index[k] = n_fast; if (k < n_records && !dropped[k]) n_fast++; }
    // LDS budget: the pruned table sits beside the full one (rays with a non-finite 1/d need that) in every workgroup that stages
    // the tree.  Three such workgroups per CU (160 KB) is what the subpath kernel runs at with its 9.7 KB of static shading
    // tables; a scene near the 512-record / 512-triangle caps would lose a workgroup per CU to the extra table (and a
    // 64-KB-per-workgroup part would refuse the launch), so there it is not built.  The staged triangles end in LDS_TRI_PADS pad
    // records (bvh_traverse.hpp: stage_bvh).
    const size_t lds_with_fast = ((size_t)2 * n_records + (size_t)3 * (s.n_tris + LDS_TRI_PADS) + (size_t)2 * n_fast) * sizeof(float4) + sizeof(ShadeLds);
    if (n_fast == n_records || lds_with_fast > (size_t)160 * 1024 / 3) return;
    out.n_fast = n_fast;
    out.fast_flat = 1;
    out.fast.resize(2 * (size_t)n_fast);
    for (int i = 0; i < s.n_boxes; i++) {
        const int k = o.rec_index[i];
        if (dropped[k]) continue;
        float4 lo = out.nodes[2 * (size_t)k], hi = out.nodes[2 * (size_t)k + 1];
        lo.w = as_f(fast_index[k + o.subtree[i]]);             // a leaf's is fast_index[k] + 1: it is one record and kept
        if (boxes[i].right == 0) { hi.w = as_f(~fast_index[k + 1]); out.fast_flat = 0; }
        out.fast[2 * (size_t)fast_index[k]] = lo;
        out.fast[2 * (size_t)fast_index[k] + 1] = hi;
    }
}

// 8b. triangle, shading, light and material records, and the camera quad's triangles
inline void pack_records(const Scene& s, PreparedScene& out) {
    for (int t = 0; t < s.n_tris; t++) {
        if (!s.tris[t].is_camera || out.cam_tris.n < 0) continue;
        if (out.cam_tris.n == CAM_TRI_ARGS) out.cam_tris.n = -1;
        else out.cam_tris.idx[out.cam_tris.n++] = t;
    }
    out.tris.resize(3 * (size_t)s.n_tris);
    out.shade.resize(4 * (size_t)s.n_tris);
    for (int t = 0; t < s.n_tris; t++) {
        const TriRec& T = s.tris[t];
        // edge vectors: the same binary32 subtractions ray_triangle_intersect performs (trace.metal:118-119)
        out.tris[3 * t] = make_float4(T.v0[0], T.v0[1], T.v0[2], 0.0f);
        out.tris[3 * t + 1] = make_float4(T.v1[0] - T.v0[0], T.v1[1] - T.v0[1], T.v1[2] - T.v0[2], 0.0f);
        out.tris[3 * t + 2] = make_float4(T.v2[0] - T.v0[0], T.v2[1] - T.v0[1], T.v2[2] - T.v0[2], 0.0f);
        out.shade[4 * t] = make_float4(T.n0[0], T.n0[1], T.n0[2], as_f(T.material));
        out.shade[4 * t + 1] = make_float4(T.n1[0], T.n1[1], T.n1[2], as_f(T.is_light ? 1 : 0));
        out.shade[4 * t + 2] = make_float4(T.n2[0], T.n2[1], T.n2[2], as_f(T.is_camera ? 1 : 0));
        out.shade[4 * t + 3] = make_float4(T.normal[0], T.normal[1], T.normal[2], 0.0f);
    }
    out.ltris.resize(5 * (size_t)s.light_count);
    for (int l = 0; l < s.light_count; l++) {
        const TriRec& T = s.ltris[l];
        out.ltris[5 * l] = make_float4(T.v0[0], T.v0[1], T.v0[2], 0.0f);
        out.ltris[5 * l + 1] = make_float4(T.v1[0], T.v1[1], T.v1[2], 0.0f);
        out.ltris[5 * l + 2] = make_float4(T.v2[0], T.v2[1], T.v2[2], 0.0f);
        out.ltris[5 * l + 3] = make_float4(T.normal[0], T.normal[1], T.normal[2], 0.0f);
        out.ltris[5 * l + 4] = make_float4(as_f(T.material), 0.0f, 0.0f, 0.0f);
    }
    out.mats.resize(s.n_mats);
    for (int m = 0; m < s.n_mats; m++) {
        const MatRec& M = s.mats[m];
        out.mats[m].color_type = make_float4(M.color[0], M.color[1], M.color[2], as_f(M.type));
        out.mats[m].emission_alpha = make_float4(M.emission[0], M.emission[1], M.emission[2], M.alpha);
        out.mats[m].ior = M.ior;
        out.mats[m].pad[0] = out.mats[m].pad[1] = out.mats[m].pad[2] = 0.0f;
    }
}

// 9. what only the wide walk reads: the triangle records without their three padding words (36 bytes each, + one record that
// the pair load of the last triangle reads; bvh_wide.hpp, PACK), and each triangle's position in the reference's visit order
// (child left+1 first, a leaf's triangles in index order), by which the nearest-first walk (ORDER) settles exact-t ties the way
// the reference does -- the triangle it meets FIRST wins, trace.metal:170.  np_flatten_bvh numbers leaves breadth-first, so the
// index alone does not say it.  [0]: "nothing held" (best.tri = -1) ranks before everything; [1 + n_tris]: behind the last.
inline void pack_wide_extras(const Scene& s, const Order& o, PreparedScene& out) {
    out.tris36.assign((size_t)9 * s.n_tris + 9, 0.0f);
    for (size_t k = 0; k < out.tris.size(); k++) {                 // vertex v of triangle t: k = 3 t + v
        out.tris36[3 * k] = out.tris[k].x; out.tris36[3 * k + 1] = out.tris[k].y; out.tris36[3 * k + 2] = out.tris[k].z;
    }
    std::vector<int> leaf_at((size_t)out.n_records, -1);            // the leaves by visit order
    for (int i = 0; i < s.n_boxes; i++) if (s.boxes[i].right != 0) leaf_at[o.rec_index[i]] = i;
    out.tri_rank.assign((size_t)s.n_tris + 2, 0x7fffffff);
    out.tri_rank[0] = (int)0x80000000;
    int next_rank = 0;
    for (int x : leaf_at) {
        if (x < 0) continue;
        for (int t = s.boxes[x].left; t < s.boxes[x].right; t++)
            if (out.tri_rank[1 + (size_t)t] == 0x7fffffff) out.tri_rank[1 + (size_t)t] = next_rank++;
    }
}

}  // namespace prep

// Entries per lane of the wide walk's global overflow array (bvh_wide.hpp) for a tree with these two depths and this child order
// (cl2_set_traversal_order), or -1: the tree cannot be served in that order.  Order 0, the reference's: twice the reference's
// pending depth plus the four a visit pushes.  Order 1, nearest first: the pending depth says nothing about it; what bounds it is
// order_depth (build_wide), of which WIDE_STACK_LDS entries live in LDS -- never less than order 0's size, with the same slack, and
// never beyond what order_depth itself needs at the cap.  tests/test_wide_stack_cpu.py holds both against the walk's push rule.
inline int wide_overflow_entries(int max_pending, int order_depth, int order) {
    const int reference = std::min(WIDE_STACK_OVERFLOW, 2 * max_pending + 4);
    if (order == 0) return reference;
    if (order_depth > WIDE_STACK_LDS + WIDE_STACK_OVERFLOW) return -1;
    return std::max(reference, std::min(WIDE_STACK_OVERFLOW, order_depth - WIDE_STACK_LDS + 4));
}

// Validates cl2_upload_scene's arguments against a W x H renderer and builds the device records into `out`: "" on success,
// else the refusal (the checks run in a fixed order, and the first that fails is reported).
inline std::string prepare_scene(const void* boxes, int n_boxes, const void* tris, int n_tris, const void* mats, int n_mats,
                                 const void* camera, const void* light_tris, const float* light_areas,
                                 const int32_t* light_tri_index, int light_count, int W, int H, PreparedScene& out) {
    using namespace prep;
    std::string err = check_arguments(boxes, n_boxes, tris, n_tris, mats, n_mats, camera, light_tris, light_areas,
                                      light_tri_index, light_count, W, H, out.cam);
    if (!err.empty()) return err;
    const Scene s{static_cast<const BoxRec*>(boxes), n_boxes, static_cast<const TriRec*>(tris), n_tris,
                  static_cast<const MatRec*>(mats), n_mats, static_cast<const TriRec*>(light_tris), light_tri_index, light_count};
    Order o;
    if (!(err = check_tree(s)).empty() || !(err = visit_order(s, o)).empty()) return err;
    out.n_records = o.subtree[0];
    out.max_pending = *std::max_element(o.pending.begin(), o.pending.end());
    out.n_top = number_records(s, out.n_records, o);
    if (!(err = check_indices(s)).empty()) return err;
    const bool nests = build_wide(s, out);
    pack_nodes(s, o, out);
    if (nests && out.n_top == 0 && out.n_records <= LDS_NODE_CAP && n_tris <= LDS_TRI_CAP) build_fast(s, o, out);
    pack_records(s, out);
    if (out.n_wide > 0) pack_wide_extras(s, o, out);
    return "";
}

}  // namespace cl2
