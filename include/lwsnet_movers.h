/* Moving objects between two consecutive frames of a sequence: which pixels of the current frame disagree with a rigid scene under
 * the given camera motion, and the connected groups of them ("movers").  Geometric evidence by the one-tap projective association of
 * lws_tsdf_integrate and lws_track, photometric evidence by lws_ego_normal's blend, components by lws_speckle_filter's join rule,
 * numbering and per-component records as lws_objects.  Additive after v8: LWS_ABI_VERSION stays 8; a header of its own that
 * includes lwsnet_hip.h, as lwsnet_track.h.  lwsnet_amd._lib reads this header into MOVERS_ABI. */
#ifndef LWSNET_MOVERS_H
#define LWSNET_MOVERS_H
#include "lwsnet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device workspace lws_movers needs for B images of H x W: per pixel one int32 parent word, one record of 12 words and two
 * bytes of flags; four int32 per tile of 4 rows x 64 columns and two per block of 2048 pixels; each part rounded up to 256 bytes.
 * max_movers is checked (1..65536) and does not change the size. */
int64_t lws_movers_workspace(int B, int H, int W, int max_movers);

/* Inputs, all in device memory; "prev" is the previous frame, "cur" the current one, and every output is in the CURRENT frame:
 * rgb_prev, rgb_cur uint8 [B,H,W,3], turned to grey by lws_egomotion's rule g = (float)(77 R + 150 G + 29 B) / 256.0f; disp_prev,
 * disp_cur float32 [B,1,H,W]; sigma_prev, sigma_cur float32 [B,1,H,W] in px or NULL: sigma0 everywhere; mask_prev, mask_cur uint8
 * [B,1,H,W] lws_lr_check code maps (1 = usable) or NULL: every pixel (ok_mask); cam float32 [B][5] = {fx, fy, cx, cy, fb} as
 * lws_depth_maps; pose float32 [B][2][12] as lws_egomotion and lws_track write it: pose[b][0] maps a point of the previous camera's
 * frame into the current one and is not read here, pose[b][1] is its inverse, row-major 3 x 4 [R|t].
 * Scalars: min_disp > 0, sigma0 >= 0, sigma_min > 0, gate_g > 0, all finite; gate_p > 0 (grey levels; +inf switches the photometric
 * test off); radius in 0..2; cand_bits in 0..31 with bits 0 and 1 clear; max_diff >= 0 (+inf allowed); min_pixels >= 1; grow in 0..8;
 * max_movers in 1..65536.  B in 1..65535, H * W < 2^31, H and W <= 2^24.
 * Every per-pixel step is one IEEE float32 operation in the order written (no contraction, correctly rounded division and square
 * root); every compare is false on NaN.
 *
 * Evidence, per current pixel p = (x, y) of image b, M = pose[b][1]:
 *   d = disp_cur[p];  use = ok_mask_cur[p] && isfinite(d) && d >= min_disp
 *   z = fb / d;  X = (((float)x - cx) * z) / fx;  Y = (((float)y - cy) * z) / fy                (lws_depth_maps)
 *   Q_r = ((m_r0 * X + m_r1 * Y) + m_r2 * z) + m_r3, r = x, y, z  (the M . P of lws_temporal_step);  use &= Qz > 0
 *   u = (fx * Qx) / Qz + cx;  v = (fy * Qy) / Qz + cy;  use &= 0 <= u <= (float)(W - 1) && 0 <= v <= (float)(H - 1)
 *   iu = (int)rintf(u);  iv = (int)rintf(v)                    (ties to even)
 *   dq = fb / Qz                                               (the disparity the static point would have had in the previous frame)
 *   sc = sigma_cur ? sigma_cur[p] : sigma0;  use &= isfinite(sc) && sc >= 0
 * Geometric residual: the taps (iv + j, iu + i), j = -radius .. radius outside, i = -radius .. radius inside (row-major).  A tap t
 * is usable iff it lies inside the image, ok_mask_prev[t], dp = disp_prev[t] is finite and >= min_disp, sp = sigma_prev ?
 * sigma_prev[t] : sigma0 is finite and >= 0, and its r is not a NaN:
 *   s = sqrtf(sc * sc + sp * sp);  sg = fmaxf(s, sigma_min);  r = (dp - dq) / sg
 * rg = the r of the usable tap with the smallest fabsf(r); of equal ones the first in scan order.  A pixel with use false or without
 * a usable tap is untested.  The window keeps a one-pixel association error at a depth edge from reading as motion.
 * Photometric residual, on iff 1 <= u <= (float)(W - 2) && 1 <= v <= (float)(H - 2) && W >= 4 && H >= 4:
 * lws_ego_normal's blend of the previous grey image at (u, v):
 *   i0 = min((int)floorf(u), W - 3);  j0 = min((int)floorf(v), H - 3);  a = u - (float)i0;  b = v - (float)j0
 *   top = g00 + a * (g01 - g00);  bot = g10 + a * (g11 - g10);  Ip = top + b * (bot - top);  rp = grey_cur[p] - Ip
 * with g00 = grey_prev[j0, i0], g01 = [j0, i0 + 1], g10 = [j0 + 1, i0], g11 = [j0 + 1, i0 + 1].
 * evidence uint8 [B,1,H,W], every element written:
 *   0 untested;
 *   1 static     fabsf(rg) <= gate_g and (the photometric test is off or fabsf(rp) <= gate_p);
 *   2 appeared   rg < -gate_g: the previous frame saw farther there, so the surface stands in what was free space;
 *   3 uncovered  rg > gate_g: the previous frame saw something nearer -- a disocclusion, a receding mover, the place a lateral mover left;
 *   4 changed    fabsf(rg) <= gate_g, the photometric test is on and fabsf(rp) > gate_p: the interior of a textured thing that moves
 *                at constant depth.
 *
 * Components: a pixel is a candidate iff bit evidence[p] of cand_bits is set (bits 0 and 1 cannot be: untested and static pixels are
 * never candidates).  Two candidates that are 4-neighbours are joined iff fabsf(d_p - d_q) <= max_diff on disp_cur
 * (lws_speckle_filter's rule); a component is a class of the transitive closure, n its pixels, its root its first pixel in raster
 * order.  A component is a mover iff n >= min_pixels; the movers are numbered j = 0, 1, .. by increasing root.
 *
 * Outputs; every element is written, the caller clears nothing:
 *   labels   int32 [B,1,H,W] (NULL: skipped) = j for a member of a mover with j < max_movers, -1 for every other pixel (before grow)
 *   mask_out uint8 [B,1,H,W]: 4 ("mover", free among lws_lr_check's 0..3) for every member of a mover, capped or not, and for every
 *            pixel within Chebyshev distance grow of one; every other pixel: mask_cur[p] when a mask was given, else 1 iff
 *            isfinite(d) && d > 0, else 0.  mask_out may be mask_cur itself.  Consumers keep code 1 only and take it unchanged
 *   rows     int32 [B,max_movers,8] = {n, x_min, x_max, y_min, y_max, n2, n3, n4} of mover j: its pixel box and its members per
 *            evidence code 2, 3, 4
 *   vals     float32 [B,max_movers,2] = {d, z}: d = (float)(((double)SQ / (double)n) / 256.0), SQ the int64 sum of (int)u16(d_p) over
 *            the members (u16 of lws_depth_maps), and z = fb / d, as lws_objects.  A slot j >= the number of movers holds
 *            {0, -1, -1, -1, -1, -1, -1, 0} and two +0.0f, as lws_objects fills it.  Movers with j >= max_movers are counted, not written
 *   info     int32 [B][8] = {tested pixels (evidence != 0), pixels of evidence 1, 2, 3, 4, components, movers (before the cap), pixels
 *            of code 4 in mask_out}
 * Argument errors -- a null pointer (sigmas, masks and labels may be null) or a misaligned one (4 bytes; the workspace 16), a bad
 * shape or scalar, any overlap between inputs, outputs and the workspace other than mask_out == mask_cur -- return LWS_ERR_INVALID
 * with a message before any GPU call.  workspace: lws_movers_workspace(B, H, W, max_movers) bytes, contents undefined before and
 * after: the call clears what it uses.
 * Eleven launches on `stream` -- the evidence (a wave's pixels are 64 consecutive ones of a row); the candidates
 * labelled per tile of 32 rows x 64 columns in LDS (union-find), unions across the tile edges, flatten; every member into its root's
 * record (the lanes of a wave that share its first root combined first); the movers numbered in raster order by the three-launch
 * scan of lws_point_cloud (per-block counts, a per-image exclusive scan with info and the empty slots, the ranked write of rows and
 * vals); the member flags with the labels, their dilation along the rows, then along the columns with mask_out -- a fixed list that
 * depends on the arguments but never on the data, with no device-to-host read, so the call can be captured into a hipGraph.  What
 * crosses lanes or workgroups is an integer add, min or max, whose order cannot show: every output is the same bytes in any batch,
 * at any position in it, on every run.  Every union-find loop keeps parent[i] <= i and waits for no other thread.  No scratch memory.
 * Limits, stated and left as they are: a receding mover shares code 3 with the disocclusions, so it is a candidate only when bit 3
 * of cand_bits is set, together with them; no velocity and no identity over frames; a mover that stands still for a frame is static
 * for that frame; the poses are taken as given, a wrong pose moves everything; the defaults of the Python layer have met synthetic
 * scenes only: real-data behaviour is unknown. */
int lws_movers(const uint8_t *rgb_prev, const float *disp_prev, const float *sigma_prev, const uint8_t *mask_prev,
               const uint8_t *rgb_cur, const float *disp_cur, const float *sigma_cur, const uint8_t *mask_cur,
               const float *cam, const float *pose, int B, int H, int W,
               float min_disp, float sigma0, float sigma_min, float gate_g, float gate_p, int radius,
               int cand_bits, float max_diff, int min_pixels, int grow, int max_movers, void *workspace,
               uint8_t *evidence, uint8_t *mask_out, int32_t *labels, int32_t *rows, float *vals, int32_t *info, void *stream);

#ifdef __cplusplus
}
#endif
#endif
