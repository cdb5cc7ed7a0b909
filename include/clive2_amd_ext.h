/* clive2_amd_ext.h -- additions to the C ABI of libclive2_amd.so.
 *
 * The ABI-6 surface of clive2_amd.h (cl2_abi_version returns 6; 108 entry points) is CLOSED: nothing is added to that header
 * any more, so a host built against it keeps working unchanged.  Entry points added since live here, in the same library, under
 * the same conventions (int return codes CL2_OK / CL2_E_*, cl2_last_error for the message, synchronous calls, one handle per
 * GPU).  cl2_ext_version counts the revisions of THIS header.
 *
 *   ext 1: cl2_denoise_select, cl2_keep_selected_picture -- a per-pixel choice among the scales of the fixed a-trous filter.
 *
 * cl2_ext_version stays 1; what came later is announced by the bits of cl2_ext_features:
 *   bit 0: the split noise model -- cl2_set_split_tracking .. cl2_light_share and the three *_model calls at the end of this header.
 */
#ifndef CLIVE2_AMD_EXT_H
#define CLIVE2_AMD_EXT_H

#include "clive2_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int cl2_ext_version(void);                                   /* 1 */

/* ---- the scale of the fixed filter, chosen per pixel by smoothed SURE maps (csrc/denoise_select.hpp) ----
 * Pass i of cl2_denoise does not depend on `iterations`, so one run of K = `iterations` passes on the picture y and one per probe
 * on the perturbed picture y' (cl2_denoise_error's, kind 0: the same inputs, signs, epsilon, correlated and seed) give the
 * pictures F_0 = y, F_1 .. F_K of cl2_denoise with iterations = 0 .. K and one Monte-Carlo SURE map m_j of each.  The maps are
 * smoothed by `smooth_passes` passes of the 5 x 5 B3 kernel at steps 1, 2, 4, ... under the filter's normal, depth and albedo
 * weights (no colour weight; pixels with fewer than 2 samples, uncovered pixels and taps without feature coverage are skipped),
 * which gives M_j; every pixel then takes the level k* with the smallest M_j (ties: the smaller j; a NaN never wins over a
 * number; a pixel with fewer than 2 samples takes K, an uncovered one 0) and the picture is gathered: out_p = F_(k*_p),p.
 * Every operation is stated in the header comment of csrc/denoise_select.hpp and restated in tests/denoise_select_reference.py.
 *
 *   out_bgr     (H, W, 3) float32 b, g, r, or NULL (n_floats 0)
 *   out_scale   (H, W) int32 k*, or NULL (n_scale 0)
 *   out[8]      [0] e_sel   [1] sum over the pixels with an estimate of M_(k*) / (luma(out) + floor)^2   [2] N = covered pixels
 *               [3] pixels with fewer than 2 samples   [4] sum M_(k*)   [5] sum M_K   [6] sum M_0   [7] sum k* over the N pixels.
 *               e_sel = +inf when N = 0 or [3] > 0, else sqrt(max([1] / N, 0)); summed without atomics, the same bytes on every call.
 *   out_maps    [2][K+1][H][W] float32: the raw maps m, then the smoothed maps M; or NULL (n_maps 0).  m_K is cl2_denoise_error's
 *               map of the same arguments bit for bit; 0 where uncovered, +inf with fewer than 2 samples.
 *   out_levels  [2][K+1][H][W][3] float32: F_j(y), then F_j(y') of the last probe; or NULL (n_levels 0)
 *
 * e_sel IS BIASED LOW.  It is the estimate of the level that LOOKED best, and the minimum over noisy estimates lies below the
 * estimate of any fixed level -- on top of the calibration limits of cl2_denoise_error.  It is a diagnostic; nothing stops a
 * render on it.
 *
 * Checks: cl2_denoise_error's with their codes (a NULL handle or a NULL `out`, probes in 1..16, epsilon > 0 and finite, correlated
 * 0 or 1, floor >= 0 and finite, cl2_denoise's checks of the sigmas, every size exact: CL2_E_INVALID; no current features, error
 * tracking off or invalid moments: CL2_E_STATE), and iterations in 1..12 (0 leaves nothing to choose), smooth_passes in 0..4.
 * A refused call changes nothing.  The call writes buffers of its own only: accumulators, moments, features, seeds, counters, the
 * guide variance of cl2_denoise_guided and a kept picture do not move.
 *
 * Device memory, allocated by the first call, regrown when K grows, freed with the handle: 52 (K + 1) + 32 bytes per pixel --
 * both level sets 32 (K + 1), the float64 sums 8 (K + 1), three map buffers 12 (K + 1), and 32 for A, the scale map and the
 * picture.  K = 3 at 1920 x 1080: 240 bytes per pixel, 498 MB. */
int cl2_denoise_select(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo,
                       int probes, float epsilon, int correlated, uint32_t seed, int smooth_passes, double floor,
                       float* out_bgr /* (H,W,3) or NULL */, size_t n_floats,
                       int32_t* out_scale /* (H,W) or NULL */, size_t n_scale,
                       double* out /* [8] */,
                       float* out_maps /* [2][K+1][H][W]: m then M; or NULL */, size_t n_maps,
                       float* out_levels /* [2][K+1][H][W][3]: L_j(y), then L_j(y') of the last probe; or NULL */, size_t n_levels);

/* The same launches; the selected picture becomes the KEPT picture, kind 8 (clive2_amd.h: "the kept picture"), under
 * cl2_keep_picture's rules: a snapshot, nothing is copied to the host, a refused call leaves the previous kept picture, a HIP
 * failure part way through leaves kind 0.  cl2_kept_picture reports 8; cl2_read_picture, cl2_picture_log_sum and
 * cl2_picture_tone_map serve kind 8 like any other kind; cl2_keep_picture with kind 0 drops it; cl2_keep_picture still takes 0..4 only. */
int cl2_keep_selected_picture(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo,
                              int probes, float epsilon, int correlated, uint32_t seed, int smooth_passes);

/* ---- the split noise model (csrc/error_split.hpp) ----
 * The camera image of a pass is spread over 3 x 3 pixels, so its noise is correlated between neighbours; the light image (t = 1
 * splats) is not reconstructed, so its noise is independent.  Neither perturbation of cl2_denoise_error matches a real render
 * (clive2_amd.h: "real renders lie between the modes").  With split tracking on, every addend's luma moments are also kept apart
 * for its camera part (t, wc) and its light part (l, wl): smom [6][W*H] float32, 24 bytes per pixel,
 *     yc = (scrub(t.b) 0.0722f + scrub(t.g) 0.7152f) + scrub(t.r) 0.2126f, yl the same of l
 *     row 0 += yc yc   1 += yc wc   2 += wc wc   3 += yl yl   4 += yl wl   5 += wl wl
 * by a kernel of their own in front of the accumulating one: accumulators, moments, buckets and layers get the bytes they get
 * without it.  The rows follow the rules of the moments (cl2_set_error_tracking): switched on over existing samples, or after
 * cl2_write_accumulators_packed, they are INVALID until cl2_reset_accumulators, which zeroes them, or cl2_write_split_moments_packed.
 * cl2_upload_scene leaves them as it leaves the moments.
 * Limits: a sample density has no split form -- cl2_set_split_tracking(r, 1) while one is set, and cl2_set_sample_density /
 * cl2_update_sample_density / an adaptive cl2_run_until while split tracking is on, return CL2_E_STATE.  cl2_reduce_accumulators does
 * not reduce the rows: after it they are invalid on every rank. */
int cl2_ext_features(void);                                  /* bit 0: the split noise model */
int cl2_set_split_tracking(cl2_renderer* r, int on);
int cl2_get_split_tracking(const cl2_renderer* r);           /* 1 on, 0 off */
int cl2_read_split_moments_packed(cl2_renderer* r, float* dst, size_t n_floats);          /* n_floats = 6*W*H; CL2_E_STATE unless valid */
int cl2_write_split_moments_packed(cl2_renderer* r, const float* src, size_t n_floats);   /* makes them valid */

/* The light part's share of the luma variance.  Per pixel in float64, with the state and L = luma of the picture of the standard
 * errors (cl2_read_standard_error):  S_c = max(0, m0 - 2 L m1 + L^2 m2),  S_l = max(0, m3 - 2 L m4 + L^2 m5),
 * rho = S_l / (S_c + S_l) when that sum is > 0 and finite, else 1; rho = 1 for uncovered pixels and pixels with fewer than 2
 * samples: a pixel without a usable split behaves as the default model, independent signs.  A NaN row gives 1.
 * The sharing is PROPORTIONAL on purpose: the variance v_p that enters SURE stays the one of the moments exactly, so sum v and the
 * fidelity term do not move, and no camera-light cross term is needed.
 *   out_map  (H, W) float32 rho, or NULL (n_map 0)
 *   out[4]   over the pixels with an estimate and a finite var_L:  [1] sum rho var_L   [2] sum var_L   [3] their count
 *            [0] = [1] / [2], 0 when [2] is not > 0.  Summed without atomics, the same bytes on every call.
 * CL2_E_STATE unless both the moments and the split rows are valid. */
int cl2_light_share(cl2_renderer* r, float* out_map /* (H,W) or NULL */, size_t n_map, double* out /* [4] */);

/* cl2_denoise_error, cl2_denoise_select and cl2_keep_selected_picture with `noise_model` where they take `correlated`:
 *   0 independent signs, 1 reconstruction-correlated signs -- the bytes of the old call with correlated = 0, 1
 *   2 split: z_p = cs_p zK_p + cl_p b'_p, zK the correlated field of (p, t), b'_p the sign of (p, t ^ 0xA5A5A5A5),
 *     cs = (float) sqrt(1 - rho_p), cl = (float) sqrt(rho_p) from the float32 rho_p above.  E z^2 = 1; a pair p != q carries
 *     cs_p cs_q times the reconstruction covariance.  Needs valid split rows, else CL2_E_STATE.
 * Every other argument, check and output is the old call's; noise_model outside 0..2 is CL2_E_INVALID.  A refused call changes
 * nothing. */
int cl2_denoise_error_model(cl2_renderer* r, int kind, int iterations, float sigma, float sigma_depth, float sigma_albedo,
                            int probes, float epsilon, int noise_model, uint32_t seed, double floor, double* out /* [8] */,
                            float* out_map /* (H,W) or NULL */, size_t n_map, float* out_probe /* 3 x (H,W,3) or NULL */, size_t n_probe);
int cl2_denoise_select_model(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo,
                             int probes, float epsilon, int noise_model, uint32_t seed, int smooth_passes, double floor,
                             float* out_bgr, size_t n_floats, int32_t* out_scale, size_t n_scale, double* out /* [8] */,
                             float* out_maps, size_t n_maps, float* out_levels, size_t n_levels);
int cl2_keep_selected_picture_model(cl2_renderer* r, int iterations, float sigma_color, float sigma_depth, float sigma_albedo,
                                    int probes, float epsilon, int noise_model, uint32_t seed, int smooth_passes);

#ifdef __cplusplus
}
#endif
#endif
