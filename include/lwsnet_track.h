/* Tracking the camera against the TSDF model: one joint cost, photometric + point-to-plane, over the pixels of a reference view
 * ray-cast from the volume (Newcombe et al. 2011: projective association; Whelan et al. 2013: RGB-D + ICP).  Additive after v8:
 * LWS_ABI_VERSION stays 8; a header of its own that includes lwsnet_hip.h, as lwsnet_egomotion.h.  lwsnet_amd._lib reads this header
 * into TRACK_ABI. */
#ifndef LWSNET_TRACK_H
#define LWSNET_TRACK_H
#include "lwsnet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device workspace lws_track and lws_track_normal need for B images of H x W */
int64_t lws_track_workspace(int B, int H, int W);

/* One linearisation of the joint cost at full resolution; the counterpart of lws_ego_normal (include/lwsnet_egomotion.h), whose
 * words -- Mf, M . P, blend, the reduction -- mean here what they mean there.
 * Inputs, all in device memory: grey_ref, grey_cur float32 [B,1,H,W]; disp_ref float32 [B,1,H,W], the model's disparity in the
 * reference camera as lws_tsdf_raycast writes it; normals_ref float32 [B,3,H,W] or NULL, the raycast's normals in the reference
 * camera's frame (n.z < 0 faces the camera); mask_ref uint8 [B,1,H,W] or NULL (1 = usable); disp_cur float32 [B,1,H,W], the current
 * frame's own disparity; sigma_cur float32 [B,1,H,W] in px or NULL: sigma0 everywhere; mask_cur uint8 or NULL; cam [B][5] as
 * lws_depth_maps; M double [B][12], row-major 3 x 4 [R|t] that maps a point of the reference camera's frame into the current one.
 * Scalars: min_disp > 0; huber_p > 0 (grey levels); sigma_p > 0 (grey levels); huber_g > 0 and gate_g >= huber_g (standard
 * deviations; gate_g may be +inf); sigma0 >= 0; sigma_min > 0; lambda_g >= 0 (0 switches the geometric term off); all finite but
 * gate_g.  B in 1..65535, H * W < 2^31, H and W <= 2^24.
 * Every per-pixel step is one IEEE float32 operation in the order written (no contraction, correctly rounded division), every
 * compare is false on NaN.  fx, fy, cx, cy are lws_ego_normal's at level 0 (so cx = (cam.cx + 0.5f) * 1.0f - 0.5f, cy likewise: with
 * lambda_g = 0 the photometric half of terms is lws_ego_normal's in bits).  One reference pixel (y, x):
 *   d = disp_ref;  use = ok_mask_ref && isfinite(d) && d >= min_disp
 *   z = fb / d;  X = (((float)x - cx) * z) / fx;  Y = (((float)y - cy) * z) / fy
 *   Q = Mf . (X, Y, z);  use &= Qz > 0
 *   u = (fx * Qx) / Qz + cx;  v = (fy * Qy) / Qz + cy
 * Photometric term p, on iff use && 1 <= u <= (float)(W - 2) && 1 <= v <= (float)(H - 2) && W >= 4 && H >= 4: lws_ego_normal's
 * rule at level 0 from i0 on, with huber_p: rp, wp, Jp, and its requirement that rp, gx, gy and Jp0..5 be finite.
 * Geometric term g, on iff use && normals_ref && lambda_g > 0 && 0 <= u <= (float)(W - 1) && 0 <= v <= (float)(H - 1) and, with
 * n = normals_ref[:, y, x], isfinite(n.x) && isfinite(n.y) && isfinite(n.z) && !(n.x == 0 && n.y == 0 && n.z == 0), and all of:
 *   iu = (int)rintf(u);  iv = (int)rintf(v)                    (one tap, ties to even, as lws_tsdf_integrate)
 *   dc = disp_cur[iv, iu];  ok_mask_cur[iv, iu] && isfinite(dc) && dc >= min_disp
 *   zc = fb / dc;  Pc = ((((float)iu - cx) * zc) / fx, (((float)iv - cy) * zc) / fy, zc)
 *   n' = R . n:  n'_r = (m_r0 * n.x + m_r1 * n.y) + m_r2 * n.z  with Mf's rotation
 *   s = sigma_cur ? sigma_cur[iv, iu] : sigma0;  s >= 0 && isfinite(s)
 *   sg = fmaxf(s, sigma_min);  sz = sg * ((Qz * Qz) / fb)      (the depth's standard deviation, so that far points do not dominate;
 *       taken at the model's depth Qz, not at the tap's zc: 1 / zc^4 weighs a tap that the noise brought nearer more than one it
 *       pushed away, and that correlation of weight and residual pulled the pose by centimetres per frame at 0.3 px of noise)
 *   e = Q - Pc;  rg = ((e.x * n'.x + e.y * n'.y) + e.z * n'.z) / sz
 *   fabsf(rg) <= gate_g                                        (drops movers, occlusions, associations across a depth edge)
 *   wg = fabsf(rg) <= huber_g ? 1.0f : huber_g / fabsf(rg)
 *   c = Pc x n':  c.x = Pc.y * n'.z - Pc.z * n'.y;  c.y = Pc.z * n'.x - Pc.x * n'.z;  c.z = Pc.x * n'.y - Pc.y * n'.x
 *   Jg = (n'.x / sz, n'.y / sz, n'.z / sz, c.x / sz, c.y / sz, c.z / sz)
 *   isfinite(rg) && isfinite(Jg0) && .. && isfinite(Jg5)
 * Jg is d rg / d delta for M <- exp(delta) . M with the tap and sz held (sz is a weight, taken anew at every linearisation as wg
 * is): the normal rotates with the point, so d / d om is (Q - e) x n' = Pc x n'.  A pixel may carry both terms, one, or none.
 * terms: float32 [B,H,W,16] = {rp, wp, Jp0..5, rg, wg, Jg0..5} per pixel, zeros where a term is off; NULL: skipped.
 * sums: double [B][32] in device memory: [0..20] the upper triangle of the joint sum k w J J^T (row by row), [21..26] sum k w J r,
 * [27] sum kp wp rp^2, [28] n_p, [29] sum kg wg rg^2, [30] n_g, [31] 0.  The weights: kp = 1.0 / ((double)sigma_p * (double)sigma_p),
 * kg = (double)lambda_g.  Per pixel the photometric term is added first, then the geometric one; a term with weight k adds
 *   kw = k * (double)w;  wJ_i = kw * (double)J_i;  H_ij += wJ_i * (double)J_j;  b_i += wJ_i * (double)r;  e += (kw * (double)r) * (double)r
 * The reduction is lws_ego_normal's: 256 threads and 1024 consecutive pixels per workgroup, thread t the pixels t, t + 256, t + 512,
 * t + 768, wave shuffles (offsets 32 .. 1), (w0 + w1) + (w2 + w3), and a second kernel, one workgroup per image, that adds the
 * partials in workgroup order through the same tree.  No float atomics: an image gives the same 32 doubles in any batch, at any
 * position in it, on every run; they agree with a restatement that adds pixel after pixel to summation rounding.
 * Argument errors -- a null or misaligned pointer (floats 4 bytes, M, sums and the workspace 8), a bad shape or scalar, any overlap
 * between sums, terms or the workspace and anything else -- return LWS_ERR_INVALID with a message before any GPU call.
 * workspace: lws_track_workspace(B, H, W) bytes, contents undefined before and after.  Two launches on `stream`, nothing read back,
 * no scratch memory. */
int lws_track_normal(const float *grey_ref, const float *disp_ref, const float *normals_ref, const uint8_t *mask_ref,
                     const float *grey_cur, const float *disp_cur, const float *sigma_cur, const uint8_t *mask_cur, const float *cam,
                     const double *M, int B, int H, int W, float min_disp, float huber_p, float sigma_p, float huber_g, float gate_g,
                     float sigma0, float sigma_min, float lambda_g, void *workspace, double *sums, float *terms, void *stream);

/* The whole refinement: iters Gauss-Newton steps at full resolution and the pose block that lws_temporal_step and lws_tsdf_integrate's
 * callers read.
 * Inputs: rgb_ref, rgb_cur uint8 [B,H,W,3], the reference and the current left image, turned to grey by lws_egomotion's rule; the
 * model maps (disp_ref, normals_ref, mask_ref) and the current maps (disp_cur, sigma_cur, mask_cur) as lws_track_normal; cam;
 * init float32 [B][12] in device memory, the motion to start from, or NULL for the identity.  iters in 1..64; the scalars of
 * lws_track_normal; damping >= 0, finite; min_pixels >= 1.
 * Step s = 0 .. iters - 1: lws_track_normal's sums at the current M, then lws_egomotion's update in double with its codes, where
 * "n" is n_p + n_g: 1 too few pixels, 4 a sum not finite, 2 a pivot not > 0, 4 |delta|^2 not finite, 16 |delta|^2 < 2^-46, else
 * M <- exp(delta) . M.  After the last step one more linearisation gives the sums and resid for the final M.
 * Outputs; every element is written: pose float32 [B][2][12] as lws_egomotion writes it; status int32 [B]: the codes of all steps
 * or-ed together, bit 3 (8): the final linearisation has n_p + n_g < min_pixels, the pose is not to be trusted, and bit 5 (32): the
 * final linearisation has n_g < min_pixels: the model did not constrain the pose, the photometric term alone did; info double
 * [B][6]: n_p, the photometric rms in grey levels sqrt(e_p / (kp * n_p)), n_g, the geometric rms in standard deviations
 * sqrt(e_g / (kg * n_g)) (0 where the count is 0), |delta| of the last step taken, the steps taken; trace double [B][iters][51] or
 * NULL: per step M before it (12), the 32 sums, delta (6; 0 for codes 1, 2, 4) and the code; resid float32 [B,2,H,W] or NULL: rp
 * and rg of the final linearisation, 0 where the term is off.
 * Argument errors as lws_track_normal (info and trace 8 bytes, the others 4; rgb and masks any), before any GPU call.
 * Launches on `stream`, a list fixed by iters, never by the data, nothing read back, no scratch memory, so the call can be captured
 * into a hipGraph: one grey kernel, two per step, two for the final linearisation: 2 * iters + 3.
 * Out of scope, stated and left as it is: no pyramid for the geometric term -- the coarse-to-fine work stays in lws_egomotion, which
 * supplies init; the volume neither moves nor is hashed; no loop closure, keyframes or bundle adjustment; movers are not segmented here (include/lwsnet_movers.h does that),
 * the gate only drops them; no photometric gain and offset; real-data accuracy is unknown -- the defaults of the Python layer have
 * met a synthetic scene only. */
int lws_track(const uint8_t *rgb_ref, const float *disp_ref, const float *normals_ref, const uint8_t *mask_ref, const uint8_t *rgb_cur,
              const float *disp_cur, const float *sigma_cur, const uint8_t *mask_cur, const float *cam, const float *init, int B, int H,
              int W, int iters, float min_disp, float huber_p, float sigma_p, float huber_g, float gate_g, float sigma0,
              float sigma_min, float lambda_g, float damping, int min_pixels, void *workspace, float *pose, int32_t *status,
              double *info, double *trace, float *resid, void *stream);

#ifdef __cplusplus
}
#endif
#endif
