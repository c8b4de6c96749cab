/* Temporal fusion of disparity maps over a sequence with known poses (additive after v8: LWS_ABI_VERSION stays 8; a header of
 * its own that includes lwsnet_hip.h, as lwsnet_objects.h).  lwsnet_amd._lib reads this header into TEMPORAL_PROTOTYPES. */
#ifndef LWSNET_TEMPORAL_H
#define LWSNET_TEMPORAL_H
#include "lwsnet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device workspace lws_temporal_step needs: one uint64 per pixel (the z-buffer of the hold) when hold is 1, else 0 */
int64_t lws_temporal_workspace(int B, int H, int W, int hold);
/* One step of a per-pixel Kalman filter on disparity: the state of the previous frame is carried into the current left camera
 * with a known rigid motion, gated against the new measurement and fused with it; optionally a pixel without a measurement
 * holds what was seen there before.
 * State per pixel: D float32 [B,1,H,W] the fused disparity, expressed in the frame it was last written for; V float32 its
 * variance, px^2; A uint16 the frames fused, 0 = no state.
 * Inputs: meas [B,1,H,W]; sigma [B,1,H,W] in px, or NULL for the scalar sigma0 (finite, >= 0) everywhere; mask uint8 or NULL, the
 * lws_lr_check code map (1 = usable); cam [B][5] as lws_depth_maps; pose [B][2][12] float32 in device memory, each a row-major
 * 3 x 4 [R|t]: pose[b][0] maps a point of the previous left camera's frame into the current one, pose[b][1] is its inverse
 * (computed by the caller in float64); Dp, Vp, Ap the previous state, all three NULL on the first frame (pose may then be NULL).
 * Scalars: min_disp > 0, sigma_min > 0, gate > 0 (standard deviations), q >= 0 (process noise, px^2 per frame), max_jump >= 0
 * (+inf allowed), hold 0 or 1, q_hold >= 0, max_var > 0 (+inf allowed).  B in 1..65535, H * W < 2^31.
 * Every step below is one IEEE float32 operation (no contraction, correctly rounded division), every compare is false on NaN,
 * max / min of floats are `b > a ? b : a` / `b < a ? b : a` folded over the taps 00, 01, 10, 11 in that order.
 * M . P for a 3 x 4 M means ((m0 * X + m1 * Y) + m2 * Z) + m3 per row.
 *
 * Fuse, per current pixel (y, x):
 *   m = meas, s = sigma or sigma0;  valid = ok_mask && isfinite(m) && m >= min_disp && s >= 0 && isfinite(s)
 *   sg = fmaxf(s, sigma_min), r = sg * sg
 *   z = fb / m, X = (((float)x - cx) * z) / fx, Y = (((float)y - cy) * z) / fy      (the point of lws_depth_maps)
 *   Q = pose[1] . (X, Y, z);  assoc = a previous state is given && Qz > 0
 *   u = (fx * Qx) / Qz + cx, v = (fy * Qy) / Qz + cy;  assoc &= 0 <= u <= (float)(W - 1) && 0 <= v <= (float)(H - 1)
 *   dexp = fb / Qz
 *   i0 = (int)floorf(u), i1 = min(i0 + 1, W - 1), a = u - (float)i0;  j0, j1, b likewise from v;  tap rc = (j_r, i_c)
 *   assoc &= all four Ap taps > 0 && (max - min of the four Dp taps) <= max_jump
 *   ds = top + b * (bot - top), top = d00 + a * (d01 - d00), bot = d10 + a * (d11 - d10);  vs the same blend of Vp
 *   ag = the smallest of the four Ap
 *   k = dexp / ds;  Z' = row 2 of pose[0] applied to (Qx * k, Qy * k, Qz * k);  assoc &= Z' > 0;  dpred = fb / Z'
 *   g = dpred / ds, g2 = g * g, vpred = vs * (g2 * g2) + q            (d d'/d d = (d'/d)^2 along a ray)
 *   innov = m - dpred, S = vpred + r;  pass = valid && assoc && innov * innov <= (gate * gate) * S
 *   pass:             K = vpred / S, D = dpred + K * innov, V = vpred - K * vpred, A = min(ag + 1, 65535), code 2 (fused)
 *   valid, not pass:  D = m, V = r, A = 1; code 3 when assoc holds (history disagreed: a mover, a disocclusion or an outlier),
 *                     code 1 otherwise (new)
 *   not valid:        D = 0, V = 0, A = 0, code 0
 * Hold, only with hold == 1 and a previous state; it touches only the pixels fuse left at code 0.  Every previous pixel
 * s = y * W + x with Ap > 0 is pushed forward: d = Dp, its point P as above, P' = pose[0] . P; it needs P'z > 0 and u, v (from P'
 * as above) in range; dn = fb / P'z; target ((int)rintf(v), (int)rintf(u)), ONE tap;
 *   Zbuf[target] = max(Zbuf[target], ((uint64)key(dn) << 32) | s), key the order-preserving word of lws_occlusion_check:
 * the nearest surface wins, on equal dn the larger source index; 0 is "empty".  A code-0 pixel with a non-empty word reads s and
 * dn back: g = dn / Dp[s], g2 = g * g, vh = (Vp[s] * (g2 * g2) + q) + q_hold; if dn >= min_disp && vh <= max_var: D = dn, V = vh,
 * A = Ap[s], code 4 (held).
 * One tap, not the four-tap splat of lws_occlusion_check: held pixels are pushed forward again every frame, so ceil taps fatten
 * the foreground by a pixel per frame, and the max biases a slanted road upward.  With one tap a held pixel carries up to half a
 * pixel of positional error and an expanding image leaves pinholes.  Held pixels are flagged (code 4) and their variance is
 * inflated by q_hold per frame, so that nobody mistakes them for measurements.
 * A sigma whose square overflows, or a state the caller made up with non-finite D or V at A > 0, is followed as it is.
 * Outputs; every element is written, the caller clears nothing: D, V, A the new state (they may not alias the previous one);
 * code uint8 [B,1,H,W]; counts int64 [B][5] (NULL: skipped), the pixels of each code 0..4.
 * Argument errors -- a null or misaligned pointer (floats 4 bytes, A and Ap 2, counts and the workspace 8), a previous state given
 * in part, or without pose, a bad shape or scalar, hold without a workspace, any overlap between an output or the workspace and
 * anything else -- return LWS_ERR_INVALID with a message before any GPU call.  workspace: lws_temporal_workspace bytes, contents
 * undefined before and after.
 * Launches on `stream`, a fixed list that depends on the arguments, never on the data, nothing read back, so the call can be
 * captured into a hipGraph: (counts without a hold pass: a kernel that clears them;) the fuse kernel, one thread per quad of a row
 * -- without hold and counts the call is this one launch; with hold and a previous state two more, the splat (one thread per
 * previous pixel, the 64-bit integer max issued only where the target's code is 0) and the hold.  Counts are summed per wave and
 * workgroup first, then added with 64-bit integer atomics by the last kernel.  What crosses threads is an integer max or an
 * integer add, whose order cannot show: an image gives the same bytes in any batch, at any position in it, on every run.  No
 * scratch memory.
 * Limits, stated and left as they are: the poses are taken as the left camera's; the rig and the static scene are assumed rigid;
 * the gate resets what moves (code 3) and does not track it (include/lwsnet_movers.h
 * segments it, for the caller's mask); held pixels drift. */
int lws_temporal_step(const float *meas, const float *sigma, const uint8_t *mask, const float *cam, const float *pose, const float *Dp,
                      const float *Vp, const uint16_t *Ap, int B, int H, int W, float sigma0, float min_disp, float sigma_min, float gate,
                      float q, float max_jump, int hold, float q_hold, float max_var, void *workspace, float *D, float *V, uint16_t *A,
                      uint8_t *code, int64_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif
