// connect_resolve_iteration.hpp -- one iteration of the reference's t loop (camera vertex t - 1 and its seven pairs), the text of
// the loop body of the resolve kernels (connect_resolve_body.hpp), which includes it once per form of its t loop with CL2_TK set:
// 0 the loop as the reference has it, 1 the peeled iteration t = 1 of the slim kernel, 2 its loop over t >= 2.  No include guard.
// `continue` leaves the iteration (the peeled one stands in a do { } while (0)).
        prior_camera_color = v3(cP3); load_camera_vertex(std::integral_constant<int, CL2_TK>{}, t);
        const int c_meta = __float_as_int(cP2.w);
        const V3 c_o = v3(cP0), c_n = v3(cP2);
        const float c_cos = __builtin_fabsf(dot(v3(cP1), c_n));
        // per-path camera tables, vertex v = t-1 (same statements as the light side above)
        {
            const int v = t - 1;
            if (__float_as_int(mats[c_meta & 0xFF].color_type.w) > 0) c_spec |= 1u << v;
            if (v > 0) {
                const float G = geom_term(cam_prev_cos, c_cos, cam_prev_o, c_o);           // GC[v-1]
                GCs[(v - 1) * BLOCK + tid] = G;
                const int m = v - 1;                       // ratio of camera vertex m, its far neighbour now known
                RCs[m * BLOCK + tid] = (m == 0) ? (cam_prev_l * G) / cam_prev_c : (cam_prev_l * G) / (cam_prev_c * cam_prev_G);
                cam_prev_G = G;
            }
            cam_prev_o = c_o; cam_prev_cos = c_cos; cam_prev_l = cP1.w; cam_prev_c = cP0.w;
        }
        // unidirectional estimate of generate_paths (camera pass), trace.metal:523-528: first stored
        // vertex v >= 1 with hit_light -> rays[v-1].color / rays[v].tot_importance; both are this iteration's loads
        if (t >= 2 && !light_hit_seen && (c_meta & META_HIT_LIGHT)) {
            light_hit_seen = true;
            const V3 c = prior_camera_color / cP3.w;
            uni = make_float4(c.x, c.y, c.z, 1.0f);
        }
#ifdef CL2_TEST_VARIANT
        if ((debug_flags & 2) && t >= 2) continue;       // timing dissection (test variant only): skip the t >= 2 / t == 1 pairs
        if ((debug_flags & 4) && t == 1) continue;
#endif
        unsigned srow = 0;
        if constexpr (STRAT) srow = (unsigned)(strat >> ((t - 1) * 7)) & 0x7Fu;
        unsigned lrow = 0;
        if constexpr (LAYERS) lrow = layer_row(lcodes, t);
#define CL2_PAIR(S)                                                                                             \
        if ((S) <= Ll && t + (S) >= 2)                                                                          \
            resolve_pair<S, DET, STRAT, LAYERS, SLIM, CL2_TK>(t, B, pid, lv, GL, RL, l_spec, c_spec, spec7, c_o, c_n, cP0.w, cP1.w, cP3.w, c_cos, \
                            c_tri, c_meta, prior_camera_color, GCs, RCs, LNs, LCs, mask, hits[S], tri_shade, cam_tris, mats, cam, \
                            focal, cam_dir, total, contrib_weight_sum, light_image, splat_tab, debug_flags, det_keys, det_vals, srow, \
                            lrow, ltot, lay_light)
        CL2_PAIR(0); CL2_PAIR(1); CL2_PAIR(2); CL2_PAIR(3); CL2_PAIR(4); CL2_PAIR(5); CL2_PAIR(6);
#undef CL2_PAIR
