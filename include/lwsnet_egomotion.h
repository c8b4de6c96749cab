/* Ego-motion from two consecutive frames: dense direct alignment of the left images, with the previous frame's disparity (additive
 * after v8: LWS_ABI_VERSION stays 8; a header of its own that includes lwsnet_hip.h, as lwsnet_temporal.h).  lwsnet_amd._lib reads
 * this header into EGOMOTION_PROTOTYPES. */
#ifndef LWSNET_EGOMOTION_H
#define LWSNET_EGOMOTION_H
#include "lwsnet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device workspace lws_egomotion needs for `levels` pyramid levels (1..8) of B images of H x W; lws_ego_normal needs what
 * this answers for levels = 1 */
int64_t lws_egomotion_workspace(int B, int H, int W, int levels);

/* One linearisation of the photometric error at one pyramid level (Steinbruecker et al. 2011, Kerl et al. 2013): every usable pixel
 * of the reference (previous) image is carried with its depth through the motion M into the current image, the current image is
 * sampled there, and the 6 x 6 normal equations of the intensity difference are summed.
 * Inputs, all in device memory: grey_ref, grey_cur float32 [B,1,H,W], the images of this level; disp_ref float32 [B,1,H,W], the
 * reference disparity of this level in FULL-resolution pixels; mask uint8 [B,1,H,W] or NULL, the lws_lr_check code map (1 = usable);
 * cam [B][5] the full-resolution camera as lws_depth_maps; M double [B][12], row-major 3 x 4 [R|t] that maps a point of the
 * reference camera's frame into the current one.  level in 0..7 scales the camera:
 *   fx_l = fx * 2^-l, fy_l = fy * 2^-l, cx_l = (cx + 0.5f) * 2^-l - 0.5f, cy_l likewise; fb is unchanged, so z = fb / d at every level.
 * Scalars: min_disp > 0, huber > 0 (grey levels), both finite.  B in 1..65535, H * W < 2^31, H and W <= 2^24.
 * Every per-pixel step is one IEEE float32 operation in the order written (no contraction, correctly rounded division), every
 * compare is false on NaN.  M . P for a 3 x 4 M means ((m0 * X + m1 * Y) + m2 * Z) + m3 per row (lws_temporal_step's rule).
 * Mf is M rounded to float32.  One pixel (y, x), I = grey_cur:
 *   d = disp_ref;  use = ok_mask && isfinite(d) && d >= min_disp
 *   z = fb / d;  X = (((float)x - cx_l) * z) / fx_l;  Y = (((float)y - cy_l) * z) / fy_l
 *   Q = Mf . (X, Y, z);  use &= Qz > 0
 *   u = (fx_l * Qx) / Qz + cx_l;  v = (fy_l * Qy) / Qz + cy_l
 *   use &= 1 <= u <= (float)(W - 2) && 1 <= v <= (float)(H - 2) && W >= 4 && H >= 4
 *   i0 = min((int)floorf(u), W - 3), a = u - (float)i0;  j0 = min((int)floorf(v), H - 3), b = v - (float)j0
 *       (so the taps' neighbours i0 - 1 .. i0 + 2, j0 - 1 .. j0 + 2 are inside the image)
 *   blend(t) = top + b * (bot - top), top = t00 + a * (t01 - t00), bot = t10 + a * (t11 - t10), tap rc = (j0 + r, i0 + c)
 *   Ic = blend(I);  gx = blend(0.5f * (I[j, i + 1] - I[j, i - 1]));  gy = blend(0.5f * (I[j + 1, i] - I[j - 1, i]))
 *   r = Ic - grey_ref[y, x]
 *   w = fabsf(r) <= huber ? 1.0f : huber / fabsf(r)
 *   ju = (gx * fx_l) / Qz;  jv = (gy * fy_l) / Qz;  jz = -((ju * Qx + jv * Qy) / Qz)
 *   J = (ju, jv, jz,  jz * Qy - jv * Qz,  ju * Qz - jz * Qx,  jv * Qx - ju * Qy)
 *   use &= isfinite(r) && isfinite(gx) && isfinite(gy) && isfinite(J0) && .. && isfinite(J5)
 * J is d r / d delta for the update M <- exp(delta) . M, delta = (translation, rotation vector).  Requiring finite J (the one
 * exclusion this header adds to the rule it was asked to state) keeps every sum finite whatever the images hold.
 * terms: float32 [B,H,W,8] = {r, w, J0..J5} per pixel, all 0 where use is false; NULL: skipped.  It is the hook that lets the
 * per-pixel arithmetic be tested bit for bit.
 * sums: double [B][29] in device memory: the 21 upper-triangle entries of sum w J J^T (row by row: 00 01 .. 05 11 12 .. 55), the 6
 * of sum w J r, sum w r^2, the number of used pixels.  Each product is formed in double from the float32 values:
 *   wJ_i = (double)w * (double)J_i;  H_ij += wJ_i * (double)J_j;  b_i += wJ_i * (double)r;  e += ((double)w * (double)r) * (double)r
 * The reduction: a workgroup of 256 threads takes 1024 consecutive pixels of one image, thread t the pixels t, t + 256, t + 512,
 * t + 768 of them in that order; the 64 lanes of a wave are added with shuffles (offsets 32, 16, .., 1), the four waves as
 * (w0 + w1) + (w2 + w3), and the workgroup's 29 sums go to the workspace.  A second kernel, one workgroup per image, adds the
 * partials: thread t those of the workgroups t, t + 256, .. in that order, then the same tree.  No float atomics: the order is
 * fixed, so an image gives the same 29 doubles in any batch, at any position in it, on every run.  It is NOT the order of a
 * float64 restatement that adds the pixels one after the other: the sums agree with such a restatement to summation rounding
 * (n * 2^-53 * sum |term|), not to the bit.
 * Argument errors -- a null or misaligned pointer (floats 4 bytes, M, sums and the workspace 8), a bad shape, level or scalar, any
 * overlap between sums, terms or the workspace and anything else -- return LWS_ERR_INVALID with a message before any GPU call.
 * workspace: lws_egomotion_workspace(B, H, W, 1) bytes, contents undefined before and after.  Two launches on `stream`, nothing read
 * back, no scratch memory. */
int lws_ego_normal(const float *grey_ref, const float *disp_ref, const uint8_t *mask, const float *grey_cur, const float *cam,
                   const double *M, int B, int H, int W, int level, float min_disp, float huber, void *workspace, double *sums,
                   float *terms, void *stream);

/* The whole estimate: pyramids, levels x iters Gauss-Newton steps from the coarsest level to level 0, and the pose block that
 * lws_temporal_step reads.
 * Inputs: rgb_ref, rgb_cur uint8 [B,H,W,3], the left images of the previous and the current frame; disp_ref float32 [B,1,H,W] and
 * mask (uint8 or NULL) the previous frame's disparity and its code map; cam [B][5]; init float32 [B][12] in device memory, the
 * motion to start from, or NULL for the identity.  levels in 1..8, iters in 1..64, min_disp > 0, max_jump >= 0 (+inf allowed),
 * huber > 0, damping >= 0, all finite but max_jump; min_pixels >= 1.
 * Pyramids.  Grey: g = (float)(77 R + 150 G + 29 B) / 256.0f (the sum is an integer, the division exact).  Level l + 1 has
 * H/2 x W/2 pixels (floor); each is ((a + b) + (c + d)) * 0.25f of its 2 x 2 block, taps 00, 01, 10, 11.  The reference disparity
 * stays in full-resolution pixels: a block gives that mean when all four taps are usable (mask ok -- level 0 only --, finite,
 * >= min_disp) and their max - min is <= max_jump (max / min folded over the taps in that order, `b > a ? b : a`), else 0: none.
 * Steps.  Step s = 0 .. levels * iters - 1 works on level levels - 1 - s / iters: lws_ego_normal's sums at the current M, then, in
 * double, one image per workgroup:
 *   n < min_pixels                       -> M stays, code 1 (a level under 4 x 4 has n = 0: it is skipped this way)
 *   a sum is not finite                  -> M stays, code 4
 *   A = H + damping * diag(H);  Cholesky A = L L^T, column by column; a pivot that is not > 0 -> M stays, code 2
 *   delta = -(A^-1 b);  |delta|^2 = ((((d0^2 + d1^2) + d2^2) + d3^2) + d4^2) + d5^2 not finite -> M stays, code 4
 *   |delta|^2 < 2^-46                    -> M stays, code 16: the step is below the float32 resolution of the pose block (2^-23
 *                                           rad, 2^-23 m); with it two identical frames give the identity exactly
 *   otherwise M <- exp(delta) . M, code 0: with (v, om) = delta, t = |om|, K = [om]x:
 *       exp = [I + A K + B K^2 | (I + B K + C K^2) v],  A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3,
 *       below t < 0.05 their series to t^6 (A = 1 - t^2/6 + t^4/120 - t^6/5040, B = 1/2 - t^2/24 + t^4/720 - t^6/40320,
 *       C = 1/6 - t^2/120 + t^4/5040 - t^6/362880; the truncation is below 2^-52 there)
 * After the last step one more linearisation at level 0 gives n, sum w r^2 and resid for the final M.
 * Outputs; every element is written: pose float32 [B][2][12], pose[b][0] the float32 rounding of M (reference camera into the
 * current one), pose[b][1] of its inverse formed in double as R^T and, per row i,
 * 0 - ((R0i t0 + R1i t1) + R2i t2) (so the identity's inverse is the identity in bits, +0 and not -0); status int32 [B], the codes of all steps or-ed
 * together (bit 0 a level had too few pixels, bit 1 a singular step, bit 2 a non-finite step, bit 4 a step below resolution) and
 * bit 3: the final level-0 linearisation has n < min_pixels, the pose is not to be trusted; info double [B][4]: n and
 * sqrt(sum w r^2 / n) (0 for n = 0) at level 0 for the final pose, |delta| of the last step taken, the steps taken (code 0);
 * trace double [B][levels * iters][48] or NULL: per step M before it (12), the 29 sums, delta (6; 0 for codes 1, 2, 4) and the
 * code; resid float32 [B,1,H,W] or NULL: r of the final linearisation, 0 where the pixel is unused.
 * Argument errors as lws_ego_normal (info and trace 8 bytes, the others 4; rgb and mask any), before any GPU call.  workspace:
 * lws_egomotion_workspace bytes, contents undefined before and after.
 * Launches on `stream`, a list fixed by (levels, iters), never by the data, nothing read back, no scratch memory, so the call can be
 * captured into a hipGraph: one kernel for both level-0 grey images and the start M; one per further level for its three
 * images (so `levels` launches for the pyramids, not the one or two a fused pyramid would take: a level needs the level below it
 * complete); two per step; two for the final linearisation: levels + 2 * levels * iters + 2.
 * Out of scope, stated and left as it is: movers are neither tracked nor segmented (resid only shows them; include/lwsnet_movers.h segments them, given the motion); no loop closure,
 * keyframes or bundle adjustment; no geometric (disparity) error term here (lws_track of
 * lwsnet_track.h has one, against the TSDF model); no photometric gain and offset; drift over long sequences
 * is not bounded; real KITTI accuracy is unknown -- the defaults of the Python layer have met a synthetic scene only. */
int lws_egomotion(const uint8_t *rgb_ref, const float *disp_ref, const uint8_t *mask, const uint8_t *rgb_cur, const float *cam,
                  const float *init, int B, int H, int W, int levels, int iters, float min_disp, float max_jump, float huber,
                  float damping, int min_pixels, void *workspace, float *pose, int32_t *status, double *info, double *trace,
                  float *resid, void *stream);

#ifdef __cplusplus
}
#endif
#endif
