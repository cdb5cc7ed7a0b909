// connect_resolve_body.hpp -- the statements of the resolve kernels (connect_resolve.hpp), included as the body of k_connect_resolve
// and of k_connect_resolve_slim: two kernels of one text, so that the first one's code does not depend on the second one's
// existence.  The including kernel declares the parameters CL2_RESOLVE_PARAMS and the compile-time flags MATS_LDS, DET, MAPPED,
// STRAT, LAYERS and SLIM.  No include guard.
// SLIM: the same statements on the same operands, with fewer words held per thread (see k_connect_resolve_slim).
    static_assert(!LAYERS || (!MAPPED && !STRAT), "layer accumulators: no mapped and no masked form");
    __shared__ float GCs[(MAX_VERTS - 1) * BLOCK];     // GC[v] = G(camera[v], camera[v+1])
    __shared__ float RCs[(MAX_VERTS - 1) * BLOCK];     // RC[m]: ratio of camera vertex m with both neighbours on the camera side
    // (SLIM: without the two rows no pair reads -- the normal of light vertex 0 and the colour of light vertex MAX_VERTS - 1)
    constexpr int LN_OFF = SLIM ? 1 : 0, L_ROWS = MAX_VERTS - LN_OFF;
    __shared__ float LNs[3 * L_ROWS * BLOCK];          // light vertex normals
    __shared__ float LCs[3 * L_ROWS * BLOCK];          // light vertex colours (throughput numerators)
    __shared__ float splat_tab[WAVES_PER_BLOCK * 5 * 64];   // per-wave exchange table of the light-image splat
    // The material table in LDS (up to LDS_MAT_CAP entries; the reference ships 8): every contributing pair reads a colour or an
    // emission by the material index of a vertex -- as global loads those were two dependent fetches inside each pair's code.
    __shared__ MaterialDev s_mats[LDS_MAT_CAP];
    const int tid = threadIdx.x;
    if (MATS_LDS) {
        for (int i = tid; i < n_mats; i += BLOCK) s_mats[i] = mats_g[i];
        __syncthreads();                               // before any thread leaves
    }
    const MaterialDev* __restrict__ mats = MATS_LDS ? s_mats : mats_g;     // compile-time choice: plain LDS reads, not generic ones
    const int pid = blockIdx.x * BLOCK + tid;           // entry: pixel pid % (W*H) of sample stream pid / (W*H) (kernels.hpp, header)
    // The `pid >= B` contract (clamped_pid, kernels.hpp): the light-subpath fetches below are decided per WAVE, so every lane
    // that reaches them must own a pixel.  This return guarantees it -- it must stay in FRONT of the first such fetch, and no
    // block-wide barrier may follow it (the LDS rows are private per thread, the splat exchange is per wave).
    if (pid >= B) return;
    __builtin_assume(pid < B);
    const int Lc = cp.len[pid], Ll = lp.len[pid];
    const unsigned long long mask = cmask[pid];
    const V3 focal = cam3(cam.focal_point), cam_dir = cam3(cam.direction);
    const bool spec7 = __float_as_int(mats[7].color_type.w) > 0;

    // ---- camera subpath: its per-path tables (GC, RC, specular bits) are built incrementally inside the
    // t loop below from the vertex that iteration loads anyway -- pair (t,s) only needs GC[0..t-2],
    // RC[0..t-2] and the specular bits of camera[0..t-1] -- so the camera subpath is read once. ----
    unsigned c_spec = 0;
    bool light_hit_seen = false;                     // a camera vertex v >= 1 with hit_light was met
    V3 cam_prev_o = v3(0, 0, 0);
    float cam_prev_cos = 0.0f, cam_prev_l = 0.0f, cam_prev_c = 0.0f, cam_prev_G = 0.0f;

    // ---- the whole light subpath is fetched back to back (with each vertex's loads inside its own `if (v < Ll)` the kernel
    // made a memory round trip per light vertex), and each iteration of the t loop fetches its camera vertex and the
    // closest-hit results of its pairs together (they were two round trips).  With the is_camera flags as kernel arguments
    // that is 8 dependent round trips per pixel instead of 25.  Measured: resolve 0.838 -> 0.822 ms -- the kernel waits for
    // its dependent ARITHMETIC (division chains at three waves per SIMD) more than for memory; fetching the first camera
    // vertex up here as well costs 168 VGPRs + 16 B of scratch and is slower (0.87 ms).  A vertex slot is fetched when SOME
    // lane of the wave has it (open scenes: most subpaths are short). ----
    float4 La[MAX_VERTS], Lb[MAX_VERTS], Lcn[MAX_VERTS], Ld[MAX_VERTS];
    int Lt[MAX_VERTS];
#pragma unroll
    for (int v = 0; v < MAX_VERTS; v++) {
        if (__builtin_amdgcn_ballot_w64(v < Ll) != 0ull) {
            const size_t k = (size_t)v * B + pid;
            La[v] = lp.P0[k]; Lb[v] = lp.P1[k]; Lcn[v] = lp.P2[k]; Ld[v] = lp.P3[k]; Lt[v] = lp.tri[k];
        } else {
            La[v] = Lb[v] = Lcn[v] = Ld[v] = make_float4(0, 0, 0, 0); Lt[v] = -1;
        }
    }
    float4 cP0 = make_float4(0, 0, 0, 0), cP1 = cP0, cP2 = cP0, cP3 = cP0;
    int c_tri = -1;
    float2 hits[MAX_VERTS + 1];
    // (TK as in resolve_pair: with t >= 2 known the hit records are their triangle words, the distance word is a constant)
    auto load_camera_vertex = [&](auto TKC, int t) {   // camera vertex t-1 and the results of the connection rays that end at it
        constexpr int TK = decltype(TKC)::value;
        const size_t ck = (size_t)(t - 1) * B + pid;
        cP0 = cp.P0[ck]; cP1 = cp.P1[ck]; cP2 = cp.P2[ck]; cP3 = cp.P3[ck];
        c_tri = cp.tri[ck];
#pragma unroll
        for (int s = 1; s <= MAX_VERTS; s++) {
            if constexpr (TK == 2) hits[s] = make_float2(__int_as_float(reinterpret_cast<const int*>(chit)[(size_t)conn_slot(t, s) * B + pid]), 0.0f);
            else hits[s] = chit_load(chit, B, t, s, pid);
        }
    };
    hits[0] = make_float2(0.0f, 0.0f);
#pragma unroll
    for (int s = 1; s <= MAX_VERTS; s++) hits[s] = make_float2(0.0f, 0.0f);

    // ---- light subpath -> registers; adjacent geometry terms and interior ratios ----
    LightVtx lv[MAX_VERTS];
    float GL[MAX_VERTS], RL[MAX_VERTS];
    unsigned l_spec = 0;
#pragma unroll
    for (int v = 0; v < MAX_VERTS; v++) {
        lv[v] = LightVtx{v3(0, 0, 0), 0.0f, 0.0f, 0.0f, 0.0f, -1, 0};
        GL[v] = 0.0f; RL[v] = 0.0f;
        if (v < Ll) {
            const float4 a = La[v], b = Lb[v], c = Lcn[v], d = Ld[v];
            lv[v].o = v3(a);
            if (v >= LN_OFF) {
                const int w = 3 * (v - LN_OFF);
                LNs[(w + 0) * BLOCK + tid] = c.x; LNs[(w + 1) * BLOCK + tid] = c.y; LNs[(w + 2) * BLOCK + tid] = c.z;
            }
            if (v < L_ROWS) {
                LCs[(3 * v + 0) * BLOCK + tid] = d.x; LCs[(3 * v + 1) * BLOCK + tid] = d.y; LCs[(3 * v + 2) * BLOCK + tid] = d.z;
            }
            lv[v].c = a.w; lv[v].l = b.w; lv[v].tot = d.w;
            lv[v].cosv = __builtin_fabsf(dot(v3(b), v3(c)));
            lv[v].tri = Lt[v];
            lv[v].meta = __float_as_int(c.w);
            if (__float_as_int(mats[lv[v].meta & 0xFF].color_type.w) > 0) l_spec |= 1u << v;
            if constexpr (SLIM) {                      // {triangle, material byte} in one word (the host's rule: resolve_runs_slim)
                lv[v].tri = resolve_pack_tri(Lt[v], lv[v].meta);
                lv[v].meta = 0;
            }
        }
    }
#pragma unroll
    for (int v = 0; v + 1 < MAX_VERTS; v++)
        if (v + 1 < Ll) GL[v] = geom_term(lv[v].cosv, lv[v + 1].cosv, lv[v].o, lv[v + 1].o);
#pragma unroll
    for (int i = 0; i + 1 < MAX_VERTS; i++) {
        if (i + 1 < Ll) {
            if (i == 0) RL[0] = lv[0].l / (lv[0].c * GL[0]);
            else RL[i] = (lv[i].l * GL[i - 1]) / (lv[i].c * GL[i]);
        }
    }

    V3 total = v3(0, 0, 0);
    float contrib_weight_sum = 0.0f;
    V3 ltot[LAYERS_MAX];                             // LAYERS: the layers' running totals (dead code otherwise)
    if constexpr (LAYERS) {
#pragma unroll
        for (int l = 0; l < LAYERS_MAX; l++) ltot[l] = v3(0, 0, 0);
    }
    float4 uni = make_float4(0, 0, 0, 0);

    V3 prior_camera_color = v3(0, 0, 0);            // rays[t-2].color: the previous iteration's P3 (read once, not again)
    if constexpr (SLIM) {
        // t = 1 peeled: only its six hit records carry a distance, and the t >= 2 pairs carry none of the film projection
        if (Lc >= 1) do {
            const int t = 1;
#define CL2_TK 1
#include "connect_resolve_iteration.hpp"
#undef CL2_TK
        } while (0);
        for (int t = 2; t < Lc + 1; t++) {
#define CL2_TK 2
#include "connect_resolve_iteration.hpp"
#undef CL2_TK
        }
    } else {
        for (int t = 1; t < Lc + 1; t++) {
#define CL2_TK 0
#include "connect_resolve_iteration.hpp"
#undef CL2_TK
        }
    }

    // ---- reconstruction-filter weights, trace.metal:827-862.  A zero-length camera path is the
    // reference's zero-filled Path: pixel 0, film point (0,0,0). ----
    int pixel_idx = 0;
    if constexpr (MAPPED) { if (Lc > 0) pixel_idx = map[pid]; }
    else pixel_idx = (Lc > 0) ? pid % (cam.pixel_width * cam.pixel_height) : 0;
    V3 film = v3(0, 0, 0);
    if (Lc > 0) film = v3(cp.P0[pid]);
    const float ppw = cam.phys_width / cam.pixel_width, pph = cam.phys_height / cam.pixel_height;
    const float sigma = 0.5f * __builtin_sqrtf(ppw * ppw + pph * pph);
    float wts[9];
    float weight_sum = 0.0f;
#pragma unroll
    for (int i = -1; i < 2; i++) {
#pragma unroll
        for (int j = -1; j < 2; j++) {
            wts[(i + 1) * 3 + (j + 1)] = 0.0f;
            const int nx = (pixel_idx % cam.pixel_width) + i, ny = (pixel_idx / cam.pixel_width) + j;
            if (nx < 0 || nx >= cam.pixel_width || ny < 0 || ny >= cam.pixel_height) continue;
            // pixel_center, trace.metal:551-562 (no +0.5)
            const float xn = (nx - 0.5f * cam.pixel_width) / (float)cam.pixel_width;
            const float yn = (ny - 0.5f * cam.pixel_height) / (float)cam.pixel_height;
            const V3 pc = (cam3(cam.center) + (xn * cam.phys_width) * cam3(cam.dx)) + (yn * cam.phys_height) * cam3(cam.dy);
            const float dist = length3(pc - film);
            const float wgt = det_expf(-dist * dist / (2.0f * sigma * sigma));
            wts[(i + 1) * 3 + (j + 1)] = wgt;
            weight_sum += wgt;
        }
    }
#pragma unroll
    for (int r = 0; r < 9; r++) agg[(size_t)r * B + pid] = (weight_sum != 0.0f) ? wts[r] / weight_sum : wts[r];
    agg[(size_t)9 * B + pid] = total.x;
    agg[(size_t)10 * B + pid] = total.y;
    agg[(size_t)11 * B + pid] = total.z;
    agg[(size_t)12 * B + pid] = contrib_weight_sum;
    if constexpr (LAYERS) {
#pragma unroll
        for (int l = 0; l < LAYERS_MAX; l++) {
            if (l < lcodes.n_layers) {
                lay_agg[(size_t)(3 * l + 0) * B + pid] = ltot[l].x;
                lay_agg[(size_t)(3 * l + 1) * B + pid] = ltot[l].y;
                lay_agg[(size_t)(3 * l + 2) * B + pid] = ltot[l].z;
            }
        }
    }

    uni_out[pid] = uni;
