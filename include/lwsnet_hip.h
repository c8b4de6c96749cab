/* lwsnet_hip.h -- C ABI of the MI355X (gfx950) LWSNet disparity hot path.
 *
 * The reference (PrinceVictor/LWSNet) has no FFI/plugin layer: the path is Python
 * calling PaddlePaddle ops (models/models.py).  This header is the boundary a
 * maintainer binds with ctypes from models/models.py; every
 * entry point names the reference lines it replaces.  Plain pointers and sizes
 * only; all tensors are float32, contiguous, NCHW, in DEVICE memory unless the
 * parameter is called `host`.  `stream` is a hipStream_t passed as void*
 * (NULL = the default stream).  Calls are asynchronous on that stream, with one exception: at batch 1 lws_forward and
 * lws_forward_conf may hold the calling thread at their three cross-stream joins (option "host_joins" below).
 *
 * Every function returns 0 on success or a negative lws_status; the message of
 * the last failure on the calling thread is lws_last_error().
 * A handle is NOT thread-safe; use one handle per (process, device, stream); distinct handles may be driven from
 * distinct host threads concurrently (lws_clone, lws_pool).
 * A handle belongs to the HIP device that was current when lws_create ran (or lws_set_option(h, "device", n) before
 * anything was allocated): every call that touches the GPU through it returns LWS_ERR_INVALID unless that device is the
 * calling thread's current device.  The library never changes the caller's current device.
 */
#ifndef LWSNET_HIP_H
#define LWSNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LWS_ABI_VERSION 8

typedef enum {
    LWS_OK = 0,
    LWS_ERR_INVALID = -1,      /* bad argument / unsupported shape (Python shim raises ValueError) */
    LWS_ERR_HIP = -2,          /* a HIP runtime call failed (RuntimeError) */
    LWS_ERR_STATE = -3,        /* missing tensor / not finalized (RuntimeError) */
    LWS_ERR_NOMEM = -4
} lws_status;

/* Constructor arguments of LWSNet(args): models/models.py:8-14, defaults inference.py:23-26. */
typedef struct {
    int32_t maxdisplist[3];   /* {24,5,5}: stage-1 hypotheses, stage-2/3 residual half-range m (D = 2m-1) */
    int32_t layers_3d;        /* 4 */
    int32_t channels_3d;      /* 8 */
    int32_t growth_rate[3];   /* {4,1,1}: c3 of stage i = channels_3d * growth_rate[i] */
    int32_t feature_fp16;     /* 0 (reference behaviour).  1 = BASELINE config 5: the three feature maps are rounded to
                                 fp16 (round-to-nearest-even) where the volume kernels read them; everything else,
                                 including the soft-argmin, stays float32.  Not part of the reference; cannot meet the
                                 1e-3 px tolerance, judged on 3-px error. */
    int32_t interp_align_mode; /* 0 (default) / 1: which source index F.interpolate(mode="bilinear") uses in the reference's four
                                 resizes (models/models.py:119,146,154,161; Paddle's align_corners=False, align_mode).
                                 0 = half-pixel centres, src = ratio * (dst + 0.5) - 0.5 -- what the oracle bets Paddle 2.0rc0
                                 does; 1 = src = ratio * dst, the Paddle 1.x / 2.0-beta default.  The
                                 reference cannot be run here (no Paddle wheel), so the bet is a switch, not a constant: every
                                 resize of the path takes its taps from one helper (src_index, lws_device_math.h), the C oracle
                                 has the same switch (lwso_set_align_mode) and both values are bit-exact against it
                                 (tests/test_gpu_parity.py::test_interp_align_mode_*).  The per-op entry points without a
                                 handle (lws_volume_l1_warp, lws_upsample_add) compute mode 0.  (ABI v8) */
} lws_config;

typedef struct lws_ctx *lws_handle;

int lws_abi_version(void);
const char *lws_last_error(void);

/* Number of HIP devices visible / name of device `dev` (diagnostics only). */
int lws_device_count(void);

/* ---- model object: models/models.py:8-26 -------------------------------------------- */
int lws_create(const lws_config *cfg, lws_handle *out);
int lws_destroy(lws_handle h);

/* model.set_state_dict (inference.py:45): one call per state-dict entry, HOST pointer.
 * Keys are the Paddle structured names, e.g. "volume_postprocess.0.1.2.weight"
 * (lwsnet_amd/weights.py lists all 226).  Keys outside the hot path are stored too
 * (used by lws_forward once the 2D networks run natively) and unknown keys are an error. */
int lws_set_tensor(lws_handle h, const char *key, const float *host, const int64_t *shape, int ndim);

/* Folds eval-mode BatchNorm3D into (scale, shift) pairs, packs the Conv3D weights into
 * MFMA fragment order and uploads them.  Must be called after the last lws_set_tensor
 * and before any function that takes a handle + stage. */
int lws_finalize(lws_handle h);

/* Pre-allocates the activation workspace for batches up to B pairs of H x W and creates the handle's side stream
 * and cross-stream events (unless option "side_streams" is 0), so that later calls allocate nothing (required before
 * hipGraph capture). */
int lws_reserve(lws_handle h, int B, int H, int W);

/* ---- per-op entry points (each is one kernel launch) --------------------------------- */

/* LWSNet._build_volume_2d, models/models.py:58-76 (stride 1).
 * cost[b,d,y,x] = sum_c |L[b,c,y,x] - (x>=d ? R[b,c,y,x-d] : 0)|;  L,R [B,C,h,w] -> cost [B,D,h,w]. */
int lws_volume_l1_shift(const float *L, const float *R, float *cost,
                        int B, int C, int h, int w, int D, void *stream);

/* forward() glue models/models.py:119-121 + LWSNet._build_volume_2d3 :78-104 + warp :28-55.
 * prev_disp [B,1,H,W] is the previous stage's full-resolution disparity; the kernel
 * resizes it to [h,w] (half-pixel bilinear), scales by h/H, and for k = 0..2m-2 samples R at
 * x - wflow + (k-(m-1)) through the reference's normalise/grid_sample float32 round trip.
 * L,R [B,C,h,w] -> cost [B,2m-1,h,w].  If wflow_out != NULL the resized flow [B,h,w] is stored. */
int lws_volume_l1_warp(const float *L, const float *R, const float *prev_disp, float *cost,
                       float *wflow_out, int B, int C, int h, int w, int H, int W, int m, void *stream);

/* volume_postprocess[stage](cost) + cost, models/models.py:136-138 with post_3dconvs,
 * models/submodules.py:190-221: 6 x (BatchNorm3D(eval) -> ReLU -> Conv3D 3x3x3 s1 p1) + skip.
 * cost_in, cost_out [B,D,h,w] (may not alias). */
int lws_conv3d_stack(lws_handle h, int stage, const float *cost_in, float *cost_out,
                     int B, int D, int hh, int ww, void *stream);

/* F.softmax(-cost, axis=1) + disparity_regression, models/models.py:142,151-152,167-179.
 * cost [B,D,h,w] -> disp_low [B,h,w]; hypothesis values are start, start+1, ... */
int lws_softargmin(const float *cost, float *disp_low, int B, int D, int h, int w, float start, void *stream);

/* models/models.py:145-148,153-156: out = bilinear_resize(disp_low * H / h -> [H,W]) (+ prev).
 * disp_low [B,h,w]; prev (may be NULL) and out [B,1,H,W]. */
int lws_upsample_add(const float *disp_low, const float *prev, float *out,
                     int B, int h, int w, int H, int W, void *stream);

/* ---- whole path: the body of `for scale in range(3)`, models/models.py:115-156 ------ */
/* featsL/featsR: the three feature maps of feature_extraction.  With H2 = ceil(H/2), W2 = ceil(W/2) (the stem
 * convolution is k3 s2 dil2 pad2, models/submodules.py:118-125; both must be divisible by 4):
 * 1/8: [B,16,H2/4,W2/4], 1/4: [B,16,H2/2,W2/2], 1/2: [B,8,H2,W2] -- for H = 8k these are H/8, H/4, H/2, for the equally
 * legal H = 8k-1 they are NOT floor(H/8) ... (63 rows -> 8, 16, 32).  pred_out[s] [B,1,H,W] for s = 0..2. */
int lws_disparity_stages(lws_handle h, const float *const featsL[3], const float *const featsR[3],
                         int B, int H, int W, float *const pred_out[3], void *stream);

/* ---- the 2D networks around the path ---------- */
/* feature_extraction, models/submodules.py:113-188 (+ hourglass :35-109): img [N,3,H,W] ->
 * f8 [N,16,H2/4,W2/4], f4 [N,16,H2/2,W2/2], f2 [N,8,H2,W2] with H2 = ceil(H/2), W2 = ceil(W/2) as above. */
int lws_feature_extraction(lws_handle h, const float *img, int N, int H, int W, float *f8, float *f4, float *f2,
                           void *stream);

/* models/models.py:158-162 with refinement1/refinement2, models/submodules.py:223-327:
 * pred4 = pred3 + refinement2(concat(refinement1_left(left), refinement1_disp(pred3))).
 * left [B,3,H,W]; pred3, pred4 [B,1,H,W].  Any H, W > 0 (the refinement has no stride, hence no size rule). */
int lws_refine(lws_handle h, const float *left, const float *pred3, int B, int H, int W, float *pred4, void *stream);

/* LWSNet.forward, models/models.py:106-164: left, right [B,3,H,W] -> pred_out[0..3] [B,1,H,W]. */
int lws_forward(lws_handle h, const float *left, const float *right, int B, int H, int W, float *const pred_out[4],
                void *stream);

/* ---- per-pixel confidence and disparity sigma of a stage's soft-argmin (not in the reference) ---------------------------
 * The softmax over the D hypotheses that the regression takes the mean of, kept: how peaked it is and how wide.
 * cost [B,D,h,w], hypothesis values v_k = start + (float)k, full resolution H x W (H >= h, W >= w, H/h and W/w <= 1024).
 * Per low-resolution pixel, every step one IEEE float32 operation, sums ascending in k from 0.0f:
 *   m = max_k(-c_k);  e_k = expf(-c_k - m) (the library's own polynomial);  S = sum e_k;  p_k = e_k / S;
 *   d = sum p_k * v_k                     -- lws_softargmin's operations in its order: d is bit-equal to its output;
 *   t_k = v_k - d;
 *   peak = sum over {k : |t_k| <= 1.0f} p_k   -- the probability mass within one hypothesis step of the regressed value: about 1
 *                                            for a unimodal match, about 3/D for a flat volume, low for a bimodal one;
 *   var = sum p_k * (t_k * t_k)           -- separate multiply and add, no fused multiply-add;
 *   sig = sqrtf(var), correctly rounded.
 * Full resolution, with the source taps and the blend expression of lws_upsample_add (half-pixel centres):
 *   conf  [B,1,H,W] = bilinear_resize(peak)
 *   sigma [B,1,H,W] = bilinear_resize((sig * (float)H) * (1.0f / (float)h)) -- the standard deviation in full-resolution pixels.
 * disp_low, peak_low, sigma_low [B,h,w] receive d, peak and sig (sig in hypothesis steps, not rescaled).  Each of the five
 * outputs may be NULL (not written), not all of them.  Costs are assumed finite; what NaN costs give is whatever this arithmetic
 * gives.  One launch, no atomics, no workspace: an image gives the same bytes in any batch.  Element alignment only. */
int lws_softargmin_conf(const float *cost, int B, int D, int h, int w, float start, int H, int W, float *disp_low,
                        float *peak_low, float *sigma_low, float *conf, float *sigma, void *stream);

/* lws_forward plus the confidence and sigma maps of the three volume stages: pred_out[0..3] are lws_forward's bits;
 * conf_out[s], sigma_out[s] [B,1,H,W] (s = 0..2; an entry, or a whole array, may be NULL) are lws_softargmin_conf of stage s's
 * filtered cost, resized the way the handle's interp_align_mode says.  It runs the plan that keeps every filtered cost (no fused
 * last Conv3D layer, no deferred map; bit-exact like every plan) and one more launch per stage, under kernel class
 * LWS_KC_CONFIDENCE.  lws_reserve(B, H, W) covers it, and it is capturable into a hipGraph like lws_forward.  B <= 65535. */
int lws_forward_conf(lws_handle h, const float *left, const float *right, int B, int H, int W, float *const pred_out[4],
                     float *const conf_out[3], float *const sigma_out[3], void *stream);

/* ---- the per-pixel steps of the I/O harness on either side of forward (ABI v8) ------------- */
/* inference.py:83-85,102-103: ToTensor + Normalize of the (already cropped) image.  rgb [B,H,W,3] uint8, device memory ->
 * out [B,3,H,W] float32 = ((v / 255) - mean[c]) / std[c], one IEEE float32 operation each -- bit for bit what numpy computes in
 * lwsnet_amd/imageio.py:to_input.  mean, std: HOST pointers to 3 floats (the ImageNet constants of dataloader/dataloader.py:10-11). */
int lws_preprocess_rgb8(const uint8_t *rgb, float *out, int B, int H, int W, const float *mean, const float *std, void *stream);
/* inference.py:114-115: `.astype(np.uint8)` (C cast: truncation toward zero, wrap-around outside 0..255) + cv2.applyColorMap.
 * disp [n] float32 -> rgb [n,3] uint8 = lut[(uint8)(int64)disp]; lut: 256 x 3 bytes in device memory (lwsnet_amd.imageio.jet_lut). */
int lws_apply_lut8(const float *disp, const uint8_t *lut, uint8_t *rgb, int64_t n, void *stream);

/* ---- evaluation: the metrics of finetune.py:184-219 (test + error_estimating) and train.py:169-199 (test) (additive after v8) ---- */
/* For each stage map s and image b, over the ground-truth pixels: e = |pred - gt| (float32), valid = the reference's mask, bad =
 * valid & e > 3 & e / gt > 0.05 (finetune.py:217), abs_sum = the fp64 sum of e over the valid pixels -- one IEEE float32 operation
 * per step, so valid / bad are exactly numpy's counts; NaN / +inf ground truth is never valid, a NaN prediction never bad.
 * Deterministic (no float atomics, fixed-order sums) and independent of B and of the other images of the batch.
 * pred[s] [B,1,Hp,W], gt [B,Hg,W], both float32 contiguous in device memory; Hp = Hg + row_offset, row_offset >= 0 (SceneFlow's
 * 544-row crop against its 540 ground-truth rows: 4, train.py:189 `output[:, 4:, :]`).  Two launches on `stream`. */
/* bytes of device workspace lws_stage_metrics needs for this geometry */
int64_t lws_stage_metrics_workspace(int B, int Hg, int Wg);
/* mode 0: KITTI 3-px (valid = 0 < gt < maxdisp); mode 1: EPE (valid = gt < maxdisp).  Outputs (device):
   counts[4][B][2] = {valid, bad}, abs_sum[4][B].  Hp = Hg + row_offset, row_offset >= 0. */
int lws_stage_metrics(const float *const pred[4], int B, int Hp, int W, int row_offset, const float *gt, int Hg,
                      float maxdisp, int mode, void *workspace, int64_t *counts, double *abs_sum, void *stream);

/* ---- sparsification histograms: how well sigma or conf ranks the pixels by their error (additive after v8) ---- */
/* The inputs of the sparsification curve and its area against the oracle curve (AUSE, Ilg et al. 2018), as integers.  pred[s],
 * unc[s] [B,1,Hp,W] float32 for s < nmaps (1..4); gt [B,Hg,W]; Hp = Hg + row_offset, maxdisp and mode as for lws_stage_metrics.
 * Per ground-truth pixel, one IEEE float32 operation per step, no contraction:
 *   valid, bad  as lws_stage_metrics (mode 0: valid = 0 < g < maxdisp, mode 1: g < maxdisp; bad = valid & e > 3 & e / g > 0.05);
 *               an invalid pixel contributes nothing;
 *   e  = fabsf(p - g);  ec = fminf(e, 65536.0f) (a NaN e becomes 65536: the worst error, never dropped);
 *   q  = (int64)rintf(ec * 1024.0f), the error in 1/1024 px (the scaling is exact: the only rounding is to the 2^-10 grid);
 *   u  = unc (kind 0: sigma, lower = more trusted) or 1.0f - unc (kind 1: conf);
 *   bin(v) = 1025 if v is NaN or v >= 256.0f;  0 if v < 0x1p-24f (negatives and both zeros);  otherwise
 *            1 + ((bits(v) >> 18) - 3296): 32 logarithmic bins per octave over [2^-24, 2^8), 3296 = (127 - 24) << 5;
 *   hist[s][b][0][bin(u)] += {1, bad, q}   (the ranking under test)
 *   hist[s][b][1][bin(e)] += {1, bad, q}   (the oracle ranking)
 * hist: int64 [nmaps][B][2][LWS_SPARS_BINS][3] in device memory; bin 0 is the most trusted, bin 1025 the least.  The call clears
 * hist with one asynchronous memset on `stream` and runs one kernel: a fixed launch list, no workspace, no device-to-host read
 * (capturable into a hipGraph), element alignment only.  All accumulation is integer (LDS and global integer atomics, no float
 * atomics), so an image gives the same bytes in any batch, at any position, on every run.  Argument errors -- a NULL pointer (an
 * element below nmaps included), nmaps outside 1..4, kind or mode outside 0 / 1, row_offset < 0, Hp != Hg + row_offset, maxdisp
 * not > 0, B outside 1..65535, hist overlapping an input -- return LWS_ERR_INVALID before any GPU call. */
#define LWS_SPARS_BINS 1026
int lws_sparsification(const float *const pred[4], const float *const unc[4], int nmaps, int kind, int B, int Hp, int W,
                       int row_offset, const float *gt, int Hg, float maxdisp, int mode, int64_t *hist, void *stream);

/* ---- left-right consistency check of the stage maps (additive after v8) ---- */
/* The right view's disparity is the same left-reference network run on the mirrored, swapped pair (mirror_w(R), mirror_w(L)),
 * mirror_w(t)[..., x] = t[..., W-1-x]: lws_lr_pairs builds the input of ONE forward of 2B pairs, whose first B stage maps are the
 * left-view maps dL and whose last B are the mirrored right-view maps dRm (positive disparities).  Both functions are one launch on
 * `stream`, deterministic (no atomics) and independent of B and of the other images of the batch; argument errors return
 * LWS_ERR_INVALID before any GPU call. */
/* left, right [B,3,H,W] float32 -> left2 = [left; mirror_w(right)], right2 = [right; mirror_w(left)], each [2B,3,H,W]: bit copies. */
int lws_lr_pairs(const float *left, const float *right, float *left2, float *right2, int B, int H, int W, void *stream);
/* For s < nmaps (1..4), dL[s], dRm[s] [B,1,H,W] float32, W <= 8192 (the row is staged in LDS), tau finite and >= 0.  Per pixel x of
 * row y, d = dL[x], one IEEE float32 operation per step:
 *   t = (float)(W-1-x) + d                                        (mirrored column of the matching right pixel x - d)
 *   NaN d: code 0;  !(0 <= t <= W-1) (+-inf included): code 2 (out of the right camera's view);  otherwise
 *   i0 = (int)floorf(t), i1 = min(i0+1, W-1), a = t - i0, r = R[i0] + a * (R[i1] - R[i0]) (R = the dRm row), code = |d - r| <= tau
 *   (1 = consistent, 0 = not; a NaN r gives 0).
 * Outputs: mask[s] uint8 [B,1,H,W] = code;  out[s] float32 [B,1,H,W]: fill 0 -> d where code == 1, else 0.0f;  fill 1 -> code-1
 * pixels keep d, every other pixel gets min(d at the nearest code-1 pixel to its left, d at the nearest to its right) in its row
 * (the left value on a tie), one side's value when only that side has one, 0.0f when the row has none (background fill; O(W) per
 * row: a max-scan of the last and a min-scan of the next consistent index);  right[s] (right or right[s] NULL: skipped) float32
 * [B,1,H,W] = the un-mirrored right-view map dRm[W-1-x];  row_kept (NULL: skipped) int32 [nmaps][B][H] = the code-1 pixels of each
 * row.  No scratch memory. */
int lws_lr_check(const float *const dL[4], const float *const dRm[4], int nmaps, int B, int H, int W, float tau, int fill,
                 float *const out[4], uint8_t *const mask[4], float *const right[4], int32_t *row_kept, void *stream);

/* ---- one-forward occlusion check of the stage maps (additive after v8) ---- */
/* The classical alternative to lws_lr_check that needs no right-view map: the left-view disparities are splatted into the right
 * view with a z-buffer (the nearest surface, i.e. the largest disparity, wins), and a left pixel is occluded when something nearer
 * landed where it lands.  It finds occlusions, not mismatches.  For s < nmaps (1..4), dL[s] [B,1,H,W] float32, W <= 8192 (the row
 * and its z-buffer are held in LDS), tau finite and >= 0, fill 0 or 1.  One IEEE float32 operation per step, no contraction.
 *   key(d) = bits ^ (bits >> 31 ? 0xffffffff : 0x80000000), the order-preserving 32-bit word of a float (unsigned order of the keys
 *            = float order of the values, -0.0 below +0.0), unkey its inverse.  0 is no finite float's or infinity's key: "empty".
 *   Pass 1, splat.  Per row, Z[0..W-1] = 0.  Per pixel x, d = dL[x], t = (float)x - d.  A NaN d does not splat;
 *            !(0 <= t <= W-1) (+-inf included) does not splat; otherwise Z[j] = max(Z[j], key(d)) for j = (int)floorf(t) and, when
 *            ceilf(t) != floorf(t), also for j + 1 (<= W-1 because t <= W-1).  The max is over unsigned words.  Two taps keep a
 *            surface watertight while neighbouring targets are at most 2 columns apart.
 *   Pass 2, test.  NaN d: code 0;  !(0 <= t <= W-1): code 2 (out of the right camera's view);  otherwise j = (int)rintf(t) (half
 *            to even), z = unkey(Z[j]) (non-empty: x itself splatted there), code = z - d <= tau (1 = visible, 0 = occluded by a
 *            nearer surface).
 * Outputs: mask[s] uint8 [B,1,H,W] = code, with the meaning of lws_lr_check's codes, so every consumer of a code map takes it
 * unchanged;  out[s] float32 [B,1,H,W] = lws_lr_check's rule on these codes: fill 0 -> d where code == 1, else 0.0f;  fill 1 ->
 * code-1 pixels keep d, every other pixel gets min(d at the nearest code-1 pixel to its left, d at the nearest to its right) in its
 * row (the left value on a tie), one side's value when only that side has one, 0.0f when the row has none;  right[s] (right or
 * right[s] NULL: skipped) float32 [B,1,H,W]: right[x] = Z[x] == 0 ? 0.0f : unkey(Z[x]), the right-view disparity in the right
 * camera's own frame, 0 = a hole;  row_kept (NULL: skipped) int32 [nmaps][B][H] = the code-1 pixels of each row.
 * One launch on `stream`, no workspace, no device-to-host read (capturable into a hipGraph), element alignment only; out[s] may
 * be dL[s] (in place).  Deterministic: the only atomics are unsigned integer max on LDS words of the workgroup's own row, whose
 * order cannot show; nothing is shared between rows, images or maps, so an image gives the same bytes in any batch.  Argument
 * errors return LWS_ERR_INVALID before any GPU call.  No scratch memory. */
int lws_occlusion_check(const float *const dL[4], int nmaps, int B, int H, int W, float tau, int fill, float *const out[4],
                        uint8_t *const mask[4], float *const right[4], int32_t *row_kept, void *stream);

/* ---- geometry of a disparity map: depth, KITTI 16-bit PNG values, point cloud (additive after v8) ---- */
/* disp [B,1,H,W] float32; mask (NULL: every pixel) uint8 [B,1,H,W], the lws_lr_check code map; cam float32 [B][5] =
 * {fx, fy, cx, cy, fb} in device memory, one row per image, cx / cy in the map's (cropped) coordinates, fb = fx * baseline
 * (fx, fy, fb > 0).  min_disp finite and > 0, max_depth > 0 (+inf allowed); H*W < 2^31, B <= 65535.  Per pixel (b, y, x),
 * d = disp[b,0,y,x], one IEEE float32 operation per step in this order:
 *   ok_mask = mask == NULL || mask[b,0,y,x] == 1;   z = fb / d
 *   valid   = ok_mask && isfinite(d) && d >= min_disp && z <= max_depth
 *   X = (((float)x - cx) * z) / fx;   Y = (((float)y - cy) * z) / fy;   Z = z
 *   u16(v)  = (uint16)fminf(fmaxf(rintf(v * 256.0f), 0.0f), 65535.0f)     (rintf: half to even)
 * Deterministic (no atomics) and independent of B and of the other images of the batch; argument errors return
 * LWS_ERR_INVALID before any GPU call.  No scratch memory. */
/* One launch.  Each output may be NULL (skipped; not all three).  depth float32 [B,1,H,W] = valid ? z : 0.0f;  depth16 uint16 =
 * valid ? u16(z) : 0 (KITTI depth PNG: metres = value / 256, 0 = none);  disp16 uint16 = (ok_mask && isfinite(d) && d > 0) ?
 * u16(d) : 0 (KITTI disparity PNG; ignores min_disp, max_depth and cam).  cam may be NULL when only disp16 is requested. */
int lws_depth_maps(const float *disp, const uint8_t *mask, const float *cam, int B, int H, int W, float min_disp, float max_depth,
                   float *depth, uint16_t *depth16, uint16_t *disp16, void *stream);
/* bytes of device workspace lws_point_cloud needs for this geometry */
int64_t lws_point_cloud_workspace(int B, int H);
/* The valid pixels of image b, packed in raster order from points + b*H*W records of 16 bytes {float X, Y, Z; uint8 r, g, b,
 * a = 255} (points 16-byte aligned, room for B*H*W records); colour from rgb uint8 [B,H,W,3] (the cropped left image; NULL:
 * white).  counts int64 [B] = the valid pixels per image; records past counts[b] are left unwritten.  Three launches on
 * `stream`: per-row counts, a per-image exclusive scan of them (in the workspace), a per-row scatter ranked by wave ballots. */
int lws_point_cloud(const float *disp, const uint8_t *mask, const uint8_t *rgb, const float *cam, int B, int H, int W, float min_disp,
                    float max_depth, void *workspace, void *points, int64_t *counts, void *stream);

/* ---- surface normals and a triangle mesh of a disparity map: the pixel grid as neighbourhood (additive after v8) ---- */
/* disp, mask, cam, min_disp, max_depth: as lws_depth_maps, with its validity rule and its P = (X, Y, Z) unchanged; cam is required.
 * max_jump float32, finite and >= 0: the largest disparity step a surface may take between two neighbouring pixels.  H*W < 2^30
 * (a face count fits an int32), B <= 65535.  One IEEE float32 operation per step, no fmaf:
 *   connected  two pixels p, q are connected iff both are valid and fabsf(d_p - d_q) <= max_jump (one subtraction, one compare:
 *              the join rule of lws_speckle_filter)
 *   normal of a valid pixel p with the neighbours R (x+1), D (y+1), L (x-1), U (y-1); a pixel outside the image is invalid:
 *     e_Q = P_Q - P_p componentwise, for a connected neighbour Q
 *     the quadrants are the ordered pairs (D,R), (R,U), (U,L), (L,D), in this order; (A,B) is present iff A and B are both connected
 *     to p.  0, 1, 2 or 4 quadrants are present, never 3: three present quadrants need all four neighbours connected
 *     c = cross(e_A, e_B):  c.x = a.y*b.z - a.z*b.y;  c.y = a.z*b.x - a.x*b.z;  c.z = a.x*b.y - a.y*b.x
 *     s = (0, 0, 0);  s += c for the present quadrants in the order above
 *     len = sqrtf((s.x*s.x + s.y*s.y) + s.z*s.z);  n = s / len (three divisions)
 *     n = (+0, +0, +0) if no quadrant is present, or len is not finite, or not len > 0; and for an invalid pixel
 *   a surface that faces the camera has n.z < 0; a fronto-parallel plane gives exactly (0, 0, -1)
 *   u8(v) = (uint8)(int)rintf((v * 0.5f + 0.5f) * 255.0f)      (separate operations, rintf: half to even, the low 8 bits of the int)
 *   normal-map pixel = {u8(n.x), u8(-n.y), u8(-n.z)}: OpenGL convention (x right, y up, z towards the viewer); the zero normal
 *   gives 128, 128, 128
 * Deterministic (no atomics) and independent of B and of the other images of the batch; argument errors -- a null or misaligned
 * pointer, a bad shape or threshold, outputs that overlap each other or an input -- return LWS_ERR_INVALID before any GPU call.
 * No scratch memory. */
/* One launch, no workspace.  normals float32 [B,3,H,W] planar (NULL: skipped), normals8 uint8 [B,H,W,3] (NULL: skipped; any
 * alignment); not both NULL. */
int lws_surface_normals(const float *disp, const uint8_t *mask, const float *cam, int B, int H, int W, float min_disp, float max_depth,
                        float max_jump, float *normals, uint8_t *normals8, void *stream);
/* bytes of device workspace lws_surface_mesh needs for this geometry: two int32 per row (vertex and face counts), each part
 * rounded up to 256 bytes */
int64_t lws_surface_mesh_workspace(int B, int H);
/* An indexed triangle mesh that does not span depth discontinuities.
 *   vertices  the valid pixels of image b in raster order: vertex i is record i of lws_point_cloud, with the same bits (points:
 *             16-byte records {float X, Y, Z; uint8 r, g, b, a = 255} from points + b*H*W, 16-byte aligned, room for B*H*W; colour
 *             from rgb uint8 [B,H,W,3], NULL: white).  A vertex no face uses stays.
 *   vnormals  16-byte records {n.x, n.y, n.z, 0.0f}, record i = normals[b,:,y,x] of vertex i's pixel, where normals float32 [B,3,H,W]
 *             is what lws_surface_normals wrote (same layout and alignment as points).  vnormals is required iff normals is given,
 *             and NULL otherwise
 *   faces     int32 [B][2*(H-1)*(W-1)][3] (never NULL: at least one record).  The cell (x, y), x < W-1, y < H-1, has the corners
 *             a = (x, y), b = (x+1, y), c = (x, y+1), e = (x+1, y+1).  A triangle is emitted iff all three of its corner pairs are
 *             connected (so its corners are valid), the diagonal included.  If b and c are both valid the diagonal is b-c:
 *             T0 = (a, c, b), T1 = (b, c, e).  Otherwise, if a and e are both valid, it is a-e: T0 = (a, c, e), T1 = (a, e, b), of which
 *             at most one passes.  Otherwise nothing.  Faces are packed per image in raster order of the cells, T0 before T1, each
 *             three vertex indices of image b in the order written; each has a geometric normal with negative z
 *   index     (NULL: skipped) int32 [B,1,H,W]: a pixel's vertex index, -1 for an invalid pixel
 *   counts    int64 [B][2] = {vertices, faces}; records of points, vnormals and faces past them are left unwritten
 * workspace: lws_surface_mesh_workspace(B, H) bytes, 4-byte aligned, contents undefined before and after.  Three launches on
 * `stream` -- per-row counts of vertices and faces, a per-image exclusive scan of both, a per-row scatter that ranks the pixels of
 * rows y and y+1 and the faces of cell row y by wave ballots -- a fixed list with no device-to-host read, so the call can be
 * captured into a hipGraph. */
int lws_surface_mesh(const float *disp, const uint8_t *mask, const uint8_t *rgb, const float *cam, const float *normals, int B, int H,
                     int W, float min_disp, float max_depth, float max_jump, void *workspace, void *points, void *vnormals,
                     int32_t *faces, int32_t *index, int64_t *counts, void *stream);

/* ---- the road under a disparity map: v-disparity, ground plane, obstacle codes, bird's-eye grid, stixels (additive after v8) ---- */
/* disp, mask, cam, min_disp, max_depth: as lws_depth_maps, with its validity rule, its P = (X, Y, Z) and its u16() unchanged.  One
 * IEEE operation per step in the order written, no fma: float32 per pixel, float64 for the plane, integers for every sum.  What
 * crosses lanes or workgroups is an integer add or an integer max, whose order cannot show, so every output is a pure function
 * of the image: the same bytes in any batch, at any position in it, on every run.  Argument errors -- a null or misaligned
 * pointer, a bad shape, range or threshold, outputs that overlap each other or an input -- return LWS_ERR_INVALID before any
 * GPU call.  Every call is a fixed list of launches on `stream` with no device-to-host read, so it can be captured into a
 * hipGraph.  No scratch memory.
 * Limits, stated and left as they are: the fit starts from a line without roll.  On synthetic roads a roll of 2 degrees at 96 x 160
 * and of 1.5 degrees at KITTI size is recovered within three passes; a roll of 3 degrees with a pitch of 2 degrees is not (the
 * inliers of pass 0 then lie on one side of the image, and the passes do not leave it).  Tracking over frames is not here. */
/* Row histograms of a disparity map (the v-disparity image).  sub in 1..16: bins per pixel of disparity; nbins in 1..4096 and
 * <= 256 * sub (disparities below 256 px: the 64-bit sums of lws_ground_fit stay in range).  Per pixel, d = disp[b,0,y,x]:
 *   t = floorf(d * (float)sub);   counted = ok_mask && isfinite(d) && d >= min_disp && t < (float)nbins;   q = (int)t
 * (the compare is on the float, so a huge product is never converted).  hist uint32 [B,H,nbins]: hist[b,y,k] = the counted
 * pixels of row y with q = k.  Every bin is written, zeros included: the caller does not clear the buffer.  One launch. */
int lws_vdisparity(const float *disp, const uint8_t *mask, int B, int H, int W, float min_disp, int sub, int nbins, uint32_t *hist,
                   void *stream);
/* bytes of device workspace lws_ground_fit needs: 16 64-bit words per image, rounded up to 256 bytes */
int64_t lws_ground_workspace(int B, int H, int nbins);
/* The road's plane in disparity space, d = a*x + b*y + c in the map's pixel coordinates: a Hough vote on hist for a start, then
 * iters + 1 least-squares passes on the map.  hist: what lws_vdisparity wrote for the same disp, mask, min_disp, sub, nbins.
 * H, W <= 16384.
 * Step A, integers only.  The candidates are the pairs (yh, qB), yh_lo <= yh <= yh_hi, qb_lo <= qB <= qb_hi: a line through the
 * horizon row yh (disparity 0) and the bin qB of the bottom row H - 1.  -65536 <= yh_lo (the horizon may lie above the image),
 * yh_hi <= H - 2, 1 <= qb_lo <= qb_hi < nbins, at most 2^22 candidates; tol_bins in 0..8; min_score >= 0.  With
 * den = H - 1 - yh, a row y > yh expects the bin k(y) = (2*qB*(y - yh) + den) / (2*den) (integer division of non-negative values);
 *   score(yh, qB) = sum over y = max(yh + 1, 0) .. H - 1 of hist[b, y, max(k - tol_bins, 0) .. min(k + tol_bins, nbins - 1)]
 * The winner has the highest score; ties go to the smaller qB, then to the smaller yh.  A best score < min_score: status 1.
 * Step B.  Q = u16(d) as an integer: the fit is to what a _disp16.png stores.  The plane Q = a*x + b*y + c is held in float64.
 * Pass 0 takes the winner's line, with den of the winner:
 *   a = 0.0;   b = (256.0 * qB) / ((double)sub * den);   c = (-b) * yh + 128.0 / sub        (half a bin, for the floor in q)
 * and the tolerance tol0 pixels; passes 1 .. iters (iters in 0..8) take the plane of the pass before and tol pixels (both
 * float32, finite, >= 0).  In each pass a pixel is an inlier iff lws_vdisparity counts it and
 *   fabs((double)Q - ((a*x + b*y) + c)) <= (double)tol * 256.0
 * and n, Sx, Sy, SQ, Sxx, Sxy, Syy, SxQ, SyQ are the int64 sums of 1, x, y, Q, x*x, x*y, y*y, x*Q, y*Q over the inliers.  Then
 *   mx = Sx / n;  my = Sy / n;  mq = SQ / n                                (each sum converted to float64, rounded to nearest)
 *   cxx = Sxx / n - mx*mx;  cxy = Sxy / n - mx*my;  cyy = Syy / n - my*my;  cxq = SxQ / n - mx*mq;  cyq = SyQ / n - my*mq
 *   det = cxx*cyy - cxy*cxy
 *   a = (cxq*cyy - cyq*cxy) / det;   b = (cyq*cxx - cxq*cxy) / det;   c = (mq - a*mx) - b*my
 * n < 3, or not det > 0, or an a, b or c that is not finite: status 2, and no further pass runs.
 * plane float32 [B][4] = {(float)(a / 256.0), (float)(b / 256.0), (float)(c / 256.0), 0.0f} of the last pass, in pixels of
 * disparity; four NaN unless the status is 0.  info int32 [B][8] = {status (0 ok, 1 no ground, 2 degenerate), yh, qB and score
 * of the winner, the inliers of the last pass that ran (0 with status 1), 0, 0, 0}.
 * workspace: lws_ground_workspace(B, H, nbins) bytes, 8-byte aligned, contents undefined before and after: the call clears what
 * it uses.  3 + 2 * (iters + 1) launches: clear, vote (one packed 64-bit atomic max of (score << 32) | ~candidate per workgroup, the
 * candidates numbered by qB, then yh), seed, and per pass the sums (wave sums, then 64-bit atomic adds) and the solve. */
int lws_ground_fit(const float *disp, const uint8_t *mask, const uint32_t *hist, int B, int H, int W, float min_disp, int sub, int nbins,
                   int yh_lo, int yh_hi, int qb_lo, int qb_hi, int tol_bins, int min_score, float tol0, float tol, int iters,
                   void *workspace, float *plane, int32_t *info, void *stream);
/* Height over the plane and a code per pixel.  cam is required; plane float32 [B][4] in device memory, one row per image, as
 * lws_ground_fit writes it; ground_tol and max_height in metres, finite, 0 <= ground_tol <= max_height.  With (a, b, c) = plane[b],
 * valid and z of lws_depth_maps, in float32:
 *   dp = (a*(float)x + b*(float)y) + c
 *   nx = a*fx;   ny = b*fy;   nz = (a*cx + b*cy) + c;   len = sqrtf((nx*nx + ny*ny) + nz*nz)
 *   h  = ((d - dp) * z) / len
 * h is the signed distance of the pixel's point from the plane nx*X + ny*Y + nz*Z = fb, positive on the camera's side; the camera
 * stands fb / len above the plane.  Codes, tested in this order: 0 invalid (not a valid pixel); 5 no plane (a, b, c or h is not
 * finite); 1 ground (fabsf(h) <= ground_tol); 4 below (h < 0); 2 obstacle (h <= max_height); 3 overhead.
 * height float32 [B,1,H,W] (NULL: skipped) = h, 0.0f for the codes 0 and 5; codes uint8 [B,1,H,W] (NULL: skipped; not both);
 * counts int64 [B][6] (NULL: skipped) = the pixels of each code.  One launch, plus one that clears counts when it is given. */
int lws_ground_classify(const float *disp, const uint8_t *mask, const float *cam, const float *plane, int B, int H, int W, float min_disp,
                        float max_depth, float ground_tol, float max_height, float *height, uint8_t *codes, int64_t *counts, void *stream);
/* An occupancy grid seen from above.  codes and height: what lws_ground_classify wrote (height may be NULL when hmax is).  A pixel
 * takes part iff it is valid (the rule of lws_depth_maps without a mask) and its code is below 6 with bit codes[p] of code_bits
 * (0..63) set.  Its cell, with X and Z of lws_depth_maps; x_min finite, cell finite and > 0, in metres; Gx, Gz in 1..4096:
 *   u = (X - x_min) / cell;   v = Z / cell;   kept iff u >= 0 && u < (float)Gx && v >= 0 && v < (float)Gz
 *   ix = (int)floorf(u);   iz = (int)floorf(v)          (after the compares: a huge or NaN coordinate is never converted)
 * count uint32 [B,Gz,Gx] (NULL: skipped) = the pixels of the cell; hmax float32 [B,Gz,Gx] (NULL: skipped; not both) = the largest
 * height in the cell, +0.0f for an empty one -- the unsigned maximum of the heights' bit patterns, which is their maximum because
 * they are positive: a code_bits with one of the bits 0, 1, 4, 5 set is refused when hmax is requested.  The call clears both
 * grids itself.  Two launches: clear, scatter (atomic add and atomic unsigned max). */
int lws_bev_grid(const float *disp, const float *cam, const uint8_t *codes, const float *height, int B, int H, int W, float min_disp,
                 float max_depth, int code_bits, float x_min, float cell, int Gx, int Gz, uint32_t *count, float *hmax, void *stream);
/* Stixels and the u-disparity of the obstacle columns: per strip of `width` columns, where the road ends, how far away what stands
 * there is and how tall.  codes and height: what lws_ground_classify wrote for the same map, both required; there is no mask (an
 * invalid pixel has code 0).  H, W <= 16384; width in 1..64; sub in 1..16 and nbins in 1..4096, <= 256 * sub, as for lws_vdisparity;
 * tol_bins in 0..8; min_count >= 1; min_row >= 1; max_gap >= 0; layers in 1..4; code_bits in 0..63 with none of the bits 0, 1, 4, 5
 * (the maximum below relies on positive heights, as hmax of lws_bev_grid does).  S = ceil(W / width) strips; strip s holds the columns
 * x0 = s*width .. x1 = min(x0 + width, W) - 1 of every row.  Per image and strip:
 *   take(p), d = disp[p]:  valid (the rule of lws_depth_maps without a mask) && codes[p] < 6 with bit codes[p] of code_bits set &&
 *            t = floorf(d * (float)sub) < (float)nbins;   q = (int)t (the compare is on the float);   Q = (int)u16(d) as in lws_ground_fit
 *   U[k] = the taking pixels of the strip with q == k.  udisp uint32 [B,S,nbins] (NULL: skipped) = U, every bin written.
 * Layers j = 0 .. layers - 1, nearest first, kmax_0 = nbins - 1; layer j searches the bins 0 .. kmax_j:
 *   Wn(k)  = the sum of U[max(k - tol_bins, 0) .. min(k + tol_bins, kmax_j)]
 *   k_near = the largest k <= kmax_j with Wn(k) >= min_count; none (or kmax_j < 0): this layer and all later ones are empty, k_peak = -1
 *   k_peak = the bin of the largest U within max(k_near - tol_bins, 0) .. min(k_near + tol_bins, kmax_j); the larger k wins a tie
 *   kmax_{j+1} = k_peak - tol_bins - 1, whatever follows
 *   members: the taking pixels with |q - k_peak| <= tol_bins and q <= kmax_j;   r[y] = the members in row y;   f[y] = r[y] >= min_row
 *   y_base = the largest flagged row; none: the slot is a hole, {0, -1, -1, k_peak} and zeros, and the next layer still runs (slots
 *            are not compacted)
 *   y_top: y_top = y_base, gap = 0; for y = y_base - 1 down to 0: a flagged row sets y_top = y, gap = 0; any other row does ++gap,
 *            and the walk stops once gap > max_gap
 *   over the members in the rows y_top .. y_base: n = their count, SQ = the int64 sum of Q, hb = the unsigned maximum of the bit
 *            patterns of height
 *   d_st = (float)(((double)SQ / (double)n) / 256.0);   z = fb / d_st;   xc = (float)(x0 + x1) * 0.5f;   X = ((xc - cx) * z) / fx
 * rows int32 [B,S,layers,4] = {n, y_top, y_base, k_peak}; vals float32 [B,S,layers,4] = {d_st, z, X, the height of bits hb}; an empty
 * slot is {0, -1, -1, k_peak or -1} and four +0.0f.  Every element is written: the caller clears nothing.  No workspace.  One
 * launch, one workgroup per strip and image: the histogram and r[y] live in LDS (adds), n, SQ and hb are wave and LDS reductions
 * (adds, unsigned max); no global atomic. */
int lws_stixels(const float *disp, const float *cam, const uint8_t *codes, const float *height, int B, int H, int W, float min_disp,
                float max_depth, int code_bits, int width, int sub, int nbins, int tol_bins, int min_count, int min_row, int max_gap,
                int layers, int32_t *rows, float *vals, uint32_t *udisp, void *stream);
/* Obstacle objects -- the connected components of udisp, with pixel labels and boxes -- are declared in lwsnet_objects.h. */

/* ---- speckle filter: connected components of a disparity map (additive after v8) ---- */
/* bytes of device workspace lws_speckle_filter needs for this geometry: per pixel one int32 parent word and one int32 size word
 * (8 bytes), plus three int32 per row for the counts, each part rounded up to 256 bytes */
int64_t lws_speckle_workspace(int B, int H, int W);
/* Removes the small connected blobs of a disparity map -- OpenCV's filterSpeckles rule on float32 instead of 12.4 fixed point.
 * disp, out float32 [B,1,H,W]; mask (NULL: every pixel) and mask_out uint8 [B,1,H,W], the lws_lr_check code map; labels (NULL:
 * skipped) int32 [B,1,H,W]; counts (NULL: skipped) int64 [B][3]; workspace: lws_speckle_workspace(B, H, W) bytes, 16-byte
 * aligned, contents undefined before and after.  max_diff finite and >= 0, max_size >= 0, fill 0 or 1 (1 needs W <= 8192: the
 * row is staged in LDS, as in lws_lr_check); H*W < 2^31, B <= 65535.  Per image, d = disp[b,0,y,x]:
 *   valid     = (mask == NULL || mask[b,0,y,x] == 1) && isfinite(d) && d > 0.0f     (the d > 0 rule of disp16; 0.0f is what
 *               lws_lr_check writes for a dropped pixel, so an unfilled checked map can be passed with or without its mask)
 *   joined    two valid pixels p, q that are 4-neighbours are joined iff fabsf(dp - dq) <= max_diff (one float32 subtraction,
 *               one compare); a component is a class of the transitive closure
 *   speckle   a component of size <= max_size pixels (OpenCV's maxSpeckleSize; max_size = 0 removes nothing)
 *   mask_out  1 for a valid pixel of a kept component, 3 ("speckle") for a valid pixel of a removed one; for an invalid pixel
 *             the input code if a mask was given and that code is not 1, else 0.  lws_depth_maps / lws_point_cloud keep code 1
 *             only, so they take mask_out as it is
 *   out       fill = 0: d where mask_out == 1, else 0.0f;  fill = 1: the background fill of lws_lr_check applied to mask_out
 *             (code-1 pixels keep d, every other pixel the smaller of d at the nearest code-1 pixel to its left and to its right
 *             in its row, the left one on a tie, one side's value if only that side exists, 0.0f if the row has none)
 *   labels    for a valid pixel the raster index y*W + x of the first pixel of its component in raster order (speckles keep
 *             theirs); -1 for an invalid pixel
 *   counts[b] = {valid pixels, kept pixels (code 1 in mask_out), removed components}
 * Every output is a pure function of the image: the same bytes in any batch, at any position in it, on every run (the atomics
 * inside are integer min / add, whose order cannot show).  out may be disp itself and mask_out may be mask itself (in place);
 * any other overlap between disp, mask, out, mask_out, labels, counts and the workspace returns LWS_ERR_INVALID, as every
 * argument error does, before any GPU call.  Four launches on `stream` (tile labelling in LDS, unions across tile edges,
 * flatten + sizes, apply with the row fill) plus one when counts is requested: a fixed list that does not depend on the data,
 * with no device-to-host read, so the call can be captured into a hipGraph.  No scratch memory. */
int lws_speckle_filter(const float *disp, const uint8_t *mask, int B, int H, int W, float max_diff, int max_size, int fill,
                       void *workspace, float *out, uint8_t *mask_out, int32_t *labels, int64_t *counts, void *stream);

/* ---- edge-aware weighted median filter of a disparity map (additive after v8) ---- */
/* Smooths a disparity map and fills its small holes without smearing across colour edges: every pixel takes the lower weighted
 * median of the valid disparities in its window, the integer weights coming from the colour distance to the window's centre in
 * the left image.  disp, out float32 [B,1,H,W]; mask (NULL: every pixel) uint8 [B,1,H,W], the lws_lr_check / lws_speckle_filter
 * code map; rgb (NULL: the unweighted median -- every weight is 1 and wlut is ignored) uint8 [B,H,W,3], the guide: the cropped left
 * image in the layout lws_point_cloud takes; wlut uint16 [766] in device memory, required when rgb is not NULL (Python:
 * lwsnet_amd.ops.wmedian_lut); radius 1, 2 or 3 (windows of 3x3, 5x5, 7x7); fill_min >= 0 (0: holes are not filled); counts (NULL:
 * skipped) int64 [B][2]; any H, W > 0 with H*W < 2^31, B <= 65535.  Per image, d_q = disp[b,0,qy,qx]:
 *   valid(q)    = (mask == NULL || mask[q] == 1) && isfinite(d_q) && d_q > 0.0f              (the rule of lws_speckle_filter)
 *   window of p = the pixels q with |qx - px| <= radius and |qy - py| <= radius that lie inside the image (the window is clipped
 *                 at the border; nothing is replicated or mirrored)
 *   s(p,q)      = |r_p - r_q| + |g_p - g_q| + |b_p - b_q|                                    (0 .. 765, on the uint8 guide)
 *   w(p,q)      = rgb ? wlut[s(p,q)] : 1
 *   candidates  = the valid q of the window with w(p,q) > 0 (a valid p is its own candidate when wlut[0] > 0);  n(p) = their number,
 *                 T(p) = the sum of their weights (int32: 49 x 65535 fits)
 *   m(p)        = the smallest candidate value v with 2 * sum{w(p,q) : q a candidate, d_q <= v} >= T(p): the LOWER weighted median
 *                 (float32 compares and integer sums only, so the order in which candidates are visited cannot show; with equal
 *                 weights and odd n the ordinary median, with even n the lower of the two middle values)
 *   out[p]      = valid p:   m(p), or d_p itself when T(p) == 0
 *                 invalid p: m(p) when fill_min > 0 && n(p) >= fill_min, else 0.0f
 *   counts[b]   = {valid pixels whose out bits differ from their disp bits, invalid pixels that were filled}
 * No code map is written: the filter never changes which pixels are trusted, and a filled pixel keeps its input code (as with the
 * row fill, pass no mask to lws_depth_maps / lws_point_cloud for a filled map).  Every output is a pure function of the image: the
 * same bytes in any batch, at any position in it, on every run (no float atomics; the counts are integer adds, whose order
 * cannot show).  out must not overlap disp (a neighbourhood is read); an overlap between any two of disp, mask, rgb, wlut, out,
 * counts that involves an output (out, counts) returns LWS_ERR_INVALID, as every argument error does -- radius outside 1..3,
 * fill_min < 0, rgb without wlut, NULL disp or out, sizes outside the limits -- before any GPU call.  One launch on `stream` plus
 * one (clearing counts) when counts is requested: a fixed list that does not depend on the data, with no device-to-host read, so
 * the call can be captured into a hipGraph.  No workspace and no scratch memory. */
int lws_wmedian_filter(const float *disp, const uint8_t *mask, const uint8_t *rgb, const uint16_t *wlut, int B, int H, int W, int radius,
                       int fill_min, float *out, int64_t *counts, void *stream);

/* ---- undistortion + rectification of a raw stereo pair, fused with the input transform (additive after v8) ---- */
/* The front end of the chain: raw left and right camera images in, the rectified window of both views out, as uint8 images (the
 * rgb of lws_point_cloud / lws_wmedian_filter), as the network's float32 input planes, with a validity map and, on request, the
 * sampling map itself.  raw[c] (c = 0 left, 1 right) uint8 [B,Hs,Ws,3], both cameras of one raw size; the window is rows
 * [y0, y0+H) x columns [x0, x0+W) of the rectified frame.  Outputs, per camera c:
 *   rect[c]  uint8   [B,H,W,3]   the rectified image
 *   input[c] float32 [B,3,H,W]   exactly the bits lws_preprocess_rgb8(rect[c], mean, std) gives; mean, std: HOST pointers to 3
 *                                floats, read before the launch, required only when an input is requested
 *   valid[c] uint8   [B,1,H,W]   1 where all four taps lie inside the raw image, else 0
 *   map[c]   float32 [B,H,W,2]   (sx, sy), the raw position sampled (for tests and callers that want the map; a NaN in it is some
 *                                NaN: IEEE 754 fixes neither its sign nor its payload)
 * Each of the four array pointers and each element may be NULL (that output is skipped); at least one output must be requested.
 * params float32 [B][2][18] in device memory, one record per image and camera:
 *   {iR[9] row-major, fx, fy, cx, cy, k1, k2, p1, p2, k3}
 * iR = inv(P_rect[:, :3] * R_rect) computed in float64 and rounded to float32 (the matrix cv2.initUndistortRectifyMap uses),
 * fx .. cy the raw camera's intrinsics, k1 .. k3 its radial-tangential distortion coefficients in OpenCV's order (Python:
 * lwsnet_amd.geometry.RectifyCalib.params).  Per output pixel (b, c, v, u), one IEEE float32 operation per step in the order
 * written, products and sums left to right (no fused multiply-add, correctly rounded division):
 *   xr = (float)(u + x0);  yr = (float)(v + y0)
 *   X  = iR0*xr + iR1*yr + iR2;   Y = iR3*xr + iR4*yr + iR5;   Wc = iR6*xr + iR7*yr + iR8
 *   x  = X / Wc;  y = Y / Wc;  x2 = x*x;  y2 = y*y;  r2 = x2 + y2;  t = (2.0f*x)*y
 *   kr = 1.0f + ((k3*r2 + k2)*r2 + k1)*r2
 *   xd = (x*kr + p1*t) + p2*(r2 + 2.0f*x2)
 *   yd = (y*kr + p1*(r2 + 2.0f*y2)) + p2*t
 *   sx = fx*xd + cx;   sy = fy*yd + cy                                  -> map
 *   ok = fabsf(sx) <= 32768.0f && fabsf(sy) <= 32768.0f                 (false for NaN)
 *   qx = (int)rintf(sx*32.0f);  qy = (int)rintf(sy*32.0f)               (half to even; only when ok)
 *   X0 = qx >> 5;  ax = qx & 31;  Y0 = qy >> 5;  ay = qy & 31           (arithmetic shift = floor)
 *   tap(X,Y) = raw[c][b, Y, X, ch] inside the raw image, else `border` (an int 0..255, on every channel)
 *   rect  = ((32-ax)*(32-ay)*tap(X0,Y0) + ax*(32-ay)*tap(X0+1,Y0) + (32-ax)*ay*tap(X0,Y0+1) + ax*ay*tap(X0+1,Y0+1) + 512) >> 10
 *   valid = ok && 0 <= X0 && X0 <= Ws-2 && 0 <= Y0 && Y0 <= Hs-2
 *   !ok:  rect = border on every channel, valid = 0
 *   input[ch] = (((float)rect[ch] / 255.0f) - mean[ch]) / std[ch]
 * This is OpenCV's INTER_LINEAR / BORDER_CONSTANT rule with five fractional bits, written in plain integers: the result is exact
 * bits (tests/rectify_reference.py restates it in numpy), NOT OpenCV's bits -- cv2.remap rounds a float weight table to int16.
 * Limits: Hs, Ws <= 16384; Hs*Ws < 2^31 and H*W < 2^31; B <= 32767; x0, y0 >= 0; x0+W, y0+H <= 32768.  Every output is a pure
 * function of its own image and record: the same bytes in any batch, at any position in it, on every run (no atomics).  An overlap
 * between an output and any other device buffer of the call (another output, raw, params), a NULL raw element or NULL params,
 * border outside 0..255, std[ch] == 0 with an input requested, no output requested and sizes outside the limits return
 * LWS_ERR_INVALID before any GPU call.  One launch on `stream`, no workspace, no scratch memory and no device-to-host read, so the
 * call can be captured into a hipGraph. */
int lws_rectify_pair(const uint8_t *const raw[2], const float *params, int B, int Hs, int Ws, int H, int W, int x0, int y0, int border,
                     const float *mean, const float *std, uint8_t *const rect[2], float *const input[2], uint8_t *const valid[2],
                     float *const map[2], void *stream);

/* ---- photometric reprojection error: a score for disparity maps that needs no ground truth (additive after v8) ---- */
/* The right image is warped into the left view with the map and compared with the left image by L1 and a 3 x 3 SSIM term (Godard
 * et al. 2017): a correct map reproduces the left image, a wrong one does not.  disp[s] [B,1,H,W] float32 for s < nmaps (1..4);
 * left, right uint8 [B,H,W,3] RGB (the layout of lws_preprocess_rgb8 and of lws_wmedian_filter's guide); mask (NULL, or per map NULL:
 * every pixel) uint8 [B,1,H,W], the lws_lr_check code map; rvalid (NULL: every tap) uint8 [B,1,H,W], lws_rectify_pair's valid map
 * of the right camera; alpha finite, in [0, 1]; H*W < 2^31, B * nmaps <= 65535; element alignment only (an image row has a pitch
 * of 3 W bytes).  Per pixel (y, x) of image b and map s, d = disp[s][b,0,y,x], every step one IEEE float32 operation in the order
 * written (no contraction, correctly rounded division):
 *   t  = (float)x - d
 *   warpable = !isnan(d) && 0 <= t && t <= W-1                       (a disparity of +-inf fails the range test)
 *   i0 = (int)floorf(t);  i1 = min(i0+1, W-1);  with rvalid, warpable also needs rvalid[y,i0] == 1 && rvalid[y,i1] == 1
 *   a  = t - (float)i0
 *   per channel c: r0 = (float)right[y,i0,c];  r1 = (float)right[y,i1,c];  w_c = r0 + a * (r1 - r0)   (multiply, then add)
 *   warped[y,x,c] = warpable ? (uint8)rintf(w_c) : 0                 (w_c stays in [0, 255]: rounding is monotonic)
 *   scored   = every pixel of the 3 x 3 window of (y, x) lies inside the image and is warpable, (y, x) itself included, and
 *              (mask == NULL || mask[y,x] == 1) at the pixel itself (the neighbours' codes do not matter); H < 3 or W < 3 scores nothing
 *   l1 = (((|L_r - w_r| + |L_g - w_g|) + |L_b - w_b|) / 3.0f) / 255.0f,  L_c = (float)left[y,x,c]
 *   per channel, with X = L_c, Y = w_c, five quantities v in {X, Y, X*X, Y*Y, X*Y} (each product rounded first), summed over the
 *   window HORIZONTALLY FIRST:  h(y',x) = (v(y',x-1) + v(y',x)) + v(y',x+1);  S = (h(y-1,x) + h(y,x)) + h(y+1,x)
 *   mx = Sx/9.0f;  my = Sy/9.0f;  vx = Sxx/9.0f - mx*mx;  vy = Syy/9.0f - my*my;  cxy = Sxy/9.0f - mx*my
 *   n  = ((2.0f*mx)*my + C1) * (2.0f*cxy + C2);   m = ((mx*mx + my*my) + C1) * ((vx + vy) + C2)
 *   C1 = 6.5025f, C2 = 58.5225f  ((0.01 * 255)^2, (0.03 * 255)^2;  m > 0: the rounding of the variances is far below C2)
 *   ds_c = fminf(fmaxf((1.0f - n/m) * 0.5f, 0.0f), 1.0f);   ds = ((ds_r + ds_g) + ds_b) / 3.0f
 *   pe = alpha*ds + (1.0f - alpha)*l1                                 (in [0, 1])
 * Outputs, each optional per map (the array pointer or its element NULL: skipped) except sums:
 *   err[s]    float32 [B,1,H,W] = scored ? pe : 0.0f
 *   scored[s] uint8   [B,1,H,W] = scored ? 1 : 0
 *   warped[s] uint8   [B,H,W,3]
 *   sums      int64   [nmaps][B][4] = {scored pixels, sum q(pe), sum q(l1), sum q(ds)} over the scored pixels,
 *             q(v) = (int64)rintf(v * 1048576.0f): the scaling is exact, the only rounding is to the 2^-20 grid
 * The call clears sums with one small kernel on `stream` and runs one more: a fixed launch list of two, no workspace, no
 * device-to-host read (capturable into a hipGraph: two kernel nodes), no scratch memory.  All accumulation is integer (wave sums, then one 64-bit
 * integer atomic per workgroup and counter; no float atomics), so an image gives the same bytes in any batch, at any position, on
 * every run.  The call writes every element of every output it is given and nothing else.  Argument errors -- NULL disp, disp[s]
 * below nmaps, left, right or sums; nmaps outside 1..4; alpha outside [0, 1] or NaN; sizes outside the limits; an output
 * overlapping an input or another output -- return LWS_ERR_INVALID before any GPU call. */
int lws_photometric(const float *const disp[4], int nmaps, const uint8_t *left, const uint8_t *right, const uint8_t *const mask[4],
                    const uint8_t *rvalid, int B, int H, int W, float alpha, float *const err[4], uint8_t *const scored[4],
                    uint8_t *const warped[4], int64_t *sums, void *stream);

/* Launch-plan options of lws_forward / lws_disparity_stages.  They change which kernels / streams carry the work, never
 * the arithmetic: every setting returns the same bits (tests/test_gpu_parity.py::test_forward_schedule_options) -- except
 * the opt-in numerics mode "split_bf16".  (ABI v8 removed the options two rounds of sweeps had retired: left_at, split_heads,
 * fuse_shift, conv3d_order, mid8_tile, mid8_balance, fork_ext, tail_at, and folded mid8_form / mid16_form / conv64_form into
 * "split_bf16"; what was measured against what is in profiles/NOTES.md.)
 *   "fuse_first"     bit mask, 3 (default): bit 0 = refinement1_disp's 1 -> 32 convolution, bit 1 = refinement1_left's 3 -> 32
 *                    convolution inside their first depthwise blocks (k_ref_dws<CIN>: the convolution recomputed on the halo
 *                    tile on fp32 MFMA; one launch and one 32-channel map less each)
 *   "defer_upsample" 1 (default) = at batches <= 2 the consumers evaluate the stage-2/3 maps
 *   "split_bf16"     0 (default) or a bit mask: 1 = the 32 -> 32 Conv3D layers (k_conv3d_mid16x), 2 = the 8 -> 8 Conv3D layers
 *                    of stages 2, 3 (k_conv3d_mid8x; samples under 256 tiles stay on the exact kernel), 4 = refinement2[0]
 *                    (k_ref_conv64x); 7 = all of them.  Split-bf16 MFMA: each float32 operand as three bf16 values, six exact
 *                    cross products accumulated in float32 -- ~2.5x the MFMA issue rate at float32-level accuracy, gated
 *                    against the float64 oracle by tests/test_gpu_parity.py::test_split_bf16_*, but NOT the oracle's bits: an
 *                    opt-in numerics mode, never what bench.py's headline measures
 *   "side_streams"   1 (default) = refinement1_left and the feature-extractor tail run on a handle-owned side stream;
 *                    0 = the whole forward on the caller's stream, no forks / joins (what lws_pool workers use)
 *   "ref_chunk_mb"   72 (default): the refinement runs in chunks of pairs whose [b,H,W,32] maps are at most this many MB
 *                    each, so that a chunk's maps stay in the 256 MiB Infinity Cache between layers (batch 8 at 256x512:
 *                    two chunks of 4; 368x1232: one pair per chunk); 0 = one chunk
 *   "ref_pipe"       -1 (default: on from four chunks up), 0 / 1: consecutive refinement chunks alternate between the caller's
 *                    stream and the handle's side stream, one chunk's memory-bound blocks beside the other's 64 -> 32 convolution
 *   "fork2_after"    -1 (default: behind the last middle layer) / 0 / k: where the second fork of lws_forward sits -- behind
 *                    stage 1's last Conv3D layer (0) or behind its k-th middle layer, so that the side branch starts beside the
 *                    end of the stage-1 stack
 *   "warp_form"      residual volumes of stages 2 and 3: 1 (default) = k_volume_l1_warp stages the right-feature window of a
 *                    64-pixel row segment (all channels, zero-filled outside the image) in LDS and computes the 2m - 1
 *                    hypotheses from it; 0 = every tap gathered from global memory (the form a tile falls back to when its
 *                    flow range needs more than 160 window columns)
 *   "fuse_last1"     1 (default) / 0: batches <= 2 (with "defer_upsample"): stage 1's last Conv3D layer and the soft-argmin run in
 *                    one launch (24 x 2 x 4 tiles spanning D) and NO launch materialises pred1: stage 2's warp kernel evaluates
 *                    the taps it needs from the 1/8 map, stage 3's warp kernel writes pred1 beside pred2;
 *                    0 = k_conv3d_last + k_softargmin_upsample
 *   "fuse_ref_last"  -1 (default: batch 1 only) / 0 / 1: refinement2's last depthwise-separable block (dilation 1), the 32 -> 1
 *                    convolution and "+ pred3" in one launch (k_ref_dws_last: the block recomputed on the one-pixel ring the
 *                    convolution needs) instead of k_ref_dws + k_ref_last
 *   "host_joins"     -1 (default: automatic) / 0 / 1: the three joins of lws_forward -- the 1/4 feature map before stage 2, the
 *                    1/2 map before stage 3, refinement1_left before the refinement -- are resolved by the HOST: it polls
 *                    hipEventQuery on the side stream's event, and once it has seen the event complete it queues nothing (every
 *                    later launch on the caller's stream is then ordered behind the side work).  A wait queued on an event that
 *                    is not yet complete costs the chain 5 to 7 us even when the side work finished long before the queue gets
 *                    there, which is every join of a batch-1 throughput loop.  0 = hipStreamWaitEvent always.  Automatic = on
 *                    when the batch is 1 AND the calling thread's previous forward ran on this same handle: a thread that
 *                    feeds several handles in turn is never held (its first forward, and every forward after a change of
 *                    handle, queues its waits).  Ignored (no polling) with "side_streams" = 0, which has no joins, and while
 *                    `stream` is being captured into a hipGraph, where the waits are the graph's edges.  The capture check
 *                    looks at `stream` only: a caller that captures ANOTHER stream of the process in global capture mode
 *                    while it runs eager forwards (hipEventQuery is not allowed then), must set 0 for the duration.
 *                    WHAT CHANGES FOR THE CALLER: with host joins on, lws_forward / lws_forward_conf may hold the
 *                    calling thread until the device has reached roughly the middle of THAT forward (the end of the side
 *                    stream's refinement1_left); it stays asynchronous with respect to the forward's tail, the refinement.
 *                    lws_pool sets 0 on its workers' clones whatever the source handle says: a worker issues for a queue of jobs.
 *   "host_join_budget_us"  900 (default), 0..1000000: how long a join polls before it falls back to hipStreamWaitEvent; 0 =
 *                    every join falls back at once.  After the first fallback the forward's remaining joins queue without
 *                    polling, so one forward spins for one budget at the most.  The budget never changes a result, only
 *                    where the host waits.
 *   "device"         the HIP device the handle belongs to; settable only before lws_finalize / lws_reserve allocate
 * Unknown names and out-of-range values return LWS_ERR_INVALID.
 * hipGraph capture: lws_reserve first (nothing may allocate while capturing), then capture lws_forward on a non-default
 * stream; the library sees the capture (hipStreamIsCapturing), records its forks as capture-time events instead of binding
 * them to kernel completion signals, and times nothing (tests/test_gpu_parity.py::test_graph_capture_replays_the_forward). */
int lws_set_option(lws_handle h, const char *name, int value);
int lws_get_option(lws_handle h, const char *name, int *value);

/* ---- measurement hooks (bench.py) ------------------------------------------------------ */
/* Kernel classes timed by the built-in profiler. */
typedef enum {
    LWS_KC_VOLUME_SHIFT = 0,   /* k_volume_l1_shift                      */
    LWS_KC_VOLUME_WARP = 1,    /* k_volume_l1_warp                       */
    LWS_KC_CONV3D_FIRST = 2,   /* k_conv3d_first  (1 -> C3)              */
    LWS_KC_CONV3D_MID16 = 3,   /* k_conv3d_mid16 / k_conv3d_mid16x (C3 -> C3, C3 % 16 == 0, MFMA) */
    LWS_KC_CONV3D_MID8 = 4,    /* k_conv3d_mid8q / k_conv3d_mid8x (8 -> 8, MFMA) */
    LWS_KC_CONV3D_LAST = 5,    /* k_conv3d_last   (C3 -> 1, + skip)      */
    LWS_KC_SOFTARGMIN = 6,     /* k_softargmin                           */
    LWS_KC_UPSAMPLE = 7,       /* k_upsample_add                         */
    LWS_KC_FEATURE2D = 8,      /* k_conv2d_nchw (feature extractor)      */
    LWS_KC_REF_FIRST = 9,      /* k_ref_first (only with option "fuse_first" < 3) */
    LWS_KC_REF_DWS = 10,       /* k_ref_dws                              */
    LWS_KC_REF_CONV64 = 11,    /* k_ref_conv64                           */
    LWS_KC_REF_LAST = 12,      /* k_ref_last                             */
    LWS_KC_CONFIDENCE = 13,    /* k_softargmin_conf (lws_forward_conf only) */
    LWS_KC_COUNT = 14
} lws_kernel_class;

/* class_mask != 0: every launch whose kernel class bit (1 << lws_kernel_class) is set is bracketed from now
 * on by a hipEvent pair recorded on the launch stream (records are dropped, never blocking, beyond 65536
 * launches); -1 selects all classes.  class_mask == 0: stop.  Either way the accumulated records are cleared. */
int lws_profile_enable(lws_handle h, int class_mask);
/* After lws_profile_enable: lws_forward records events on every `every_n`-th call only (1 = every call).  Timing a
 * kernel with its own begin / end events keeps the next dispatch from being queued behind it, so bracketing every
 * launch of a latency-bound step perturbs the step; sampling bounds that cost.  Reset to 1 by lws_profile_enable. */
int lws_profile_sample(lws_handle h, int every_n);
/* Synchronises the recorded events and returns, per kernel class, the summed device time in
 * milliseconds and the number of launches.  Both arrays have LWS_KC_COUNT entries. */
int lws_profile_read(lws_handle h, double *total_ms, int64_t *launches);
/* The individual launches of one kernel class, in launch order: ms_out[0 .. min(*count, capacity)) receives their
 * durations in milliseconds, *count the number of recorded launches (bench.py separates the stage-2 from the stage-3
 * launches of k_conv3d_mid8 with it). */
int lws_profile_read_class(lws_handle h, int kernel_class, float *ms_out, int capacity, int *count);
const char *lws_kernel_class_name(int kernel_class);
/* The clock the dominant kernel really runs at (ABI v8).  lws_clock_stamp(h, 1): from now on every k_conv3d_mid16 launch made
 * through this handle (the four 32 -> 32 Conv3D layers of stage 1) has its first 64 workgroups leave s_memtime (shader clock)
 * and s_memrealtime (100 MHz) of their first and last instruction in a handle-owned buffer (a scalar branch in the kernel,
 * nothing when off); the latest launch wins.  lws_clock_read synchronises the device and returns the median over those
 * workgroups of d s_memtime / d s_memrealtime x 100 MHz for the latest stamped launch.  bench.py stamps a few forwards right
 * after its timed region -- same queue depth, same mix of kernels -- and reports roofline.clock_ghz (per rank for N > 1): a box
 * or rank that holds a lower clock shows up there, not as an unexplained slower step.  LWS_ERR_STATE when stage 1's C3 is 8. */
int lws_clock_stamp(lws_handle h, int enable);
int lws_clock_read(lws_handle h, double *ghz);
/* Test hook (additive after v8): fills the handle's WHOLE current activation workspace -- the one slab lws_reserve / the first
 * call of a geometry allocates and every later call carves up per (B, H, W) -- with the 32-bit pattern `word`, as one asynchronous
 * 32-bit memset on `stream`.  The library never clears that slab and promises that no result depends on what it holds
 * ("memory contract"); tests/test_gpu_memory_contract.py poisons it with a quiet NaN and with +-FLT_MAX before every
 * call to hold the kernels to that.  Only the workspace is touched: the parameter slab and the clock buffer are left alone.
 * LWS_ERR_INVALID unless the handle's device is the current one (the rule of every handle call), LWS_ERR_STATE when no workspace
 * exists yet -- call lws_reserve first, at the largest geometry that will follow: a call that has to regrow the slab swaps the
 * poison for fresh memory.  Must NOT be called while `stream` is being captured into a hipGraph (a replay would poison the
 * slab under whatever runs then), nor while a forward of this handle is in flight on another stream. */
int lws_debug_fill_workspace(lws_handle h, uint32_t word, void *stream);
/* Measurement hook (additive after v8): what the joins of lws_forward / lws_forward_conf did on this handle since the last reset.
 * out (optional) receives 3 x 4 values, joins in chain order (the 1/4 map, the 1/2 map, refinement1_left): {joins the host saw
 * complete, joins queued with hipStreamWaitEvent, host nanoseconds spent polling in total, the longest single poll}.  reset != 0
 * clears the counters afterwards.  Host-side only: no GPU call, any current device.  Forwards with "side_streams" = 0 count
 * nothing (they have no joins). */
int lws_join_stats(lws_handle h, int64_t *out, int reset);
/* Test hook (additive after v8): a late side branch.  On an idle device the side stream's work is done long before the caller's
 * chain reaches the join that waits for it, so a missing join, a misplaced record or a stage buffer laid over one the side branch
 * still uses gives the right bits by timing alone.  From the next lws_forward / lws_forward_conf / lws_refine of this handle on,
 * the library queues one bounded delay kernel of `microseconds` on the handle's SIDE stream at the head of every side segment
 * selected in `segments` -- behind the segment's own wait for its producer, in front of its first kernel.  These are all the
 * places where the library puts work on a stream that is not the caller's (lws_pool's worker streams are the caller's stream of
 * the workers' forwards):
 *   LWS_DELAY_F4     (bit 0)  conv5, which writes the 1/4 map stage 2 joins on;
 *   LWS_DELAY_F2     (bit 1)  conv6 + classif1, which write the 1/2 map stage 3 joins on;
 *   LWS_DELAY_LEFT   (bit 2)  refinement1_left, which the refinement joins on;
 *   LWS_DELAY_CHUNKS (bit 3)  every refinement chunk option "ref_pipe" places on the side stream (a plan without such chunks
 *                             has no such segment and queues nothing for this bit).
 * The kernel is one wave that reads the 100 MHz counter (s_memrealtime, the one lws_clock_stamp reads) and sleeps between reads;
 * it stores nothing, and it leaves after a number of sleeps fixed by the request even if the counter stood still (about twice
 * the request at the shader clocks the kernels here hold).  segments == 0 or microseconds == 0 switches the hook off, and off means nothing: no launch, no
 * event, one host branch per segment.  With option "side_streams" = 0 there is no side stream and nothing is queued.  Under
 * hipGraph capture the delay kernel is captured like every other launch of the side branch.  The setting is handle state that
 * lws_clone copies as it copies the options, so a pool created from a delayed handle has delayed workers (with
 * LWS_POOL_SIDE_STREAMS; their "host_joins" stay 0).  microseconds: 0..250000.  LWS_ERR_INVALID for a null handle, unknown
 * bits and values out of range; the earlier setting then stays.  Host-side only: no GPU call, any current device.
 * tests/test_gpu_side_delay.py holds every join of the forward with it. */
#define LWS_DELAY_F4 1
#define LWS_DELAY_F2 2
#define LWS_DELAY_LEFT 4
#define LWS_DELAY_CHUNKS 8
#define LWS_DELAY_ALL 15
int lws_debug_delay_side(lws_handle h, int segments, int microseconds);

/* ---- several forwards in flight (no counterpart in the reference: inference.py:105-109 is one thread, one stream) ---- */
/* A second handle for the same model on the same device: shares src's (read-only) parameter slab, owns its workspace,
 * streams and options.  src must outlive it and must not be re-finalized while clones exist; a clone refuses
 * lws_set_tensor / lws_finalize.  Use: one clone per host thread / stream. */
int lws_clone(lws_handle src, lws_handle *out);

/* A pool of `workers` host threads, each with its own clone of `model` and ONE HIP stream.  A batch-1 forward is a chain
 * of ~35 dependent launches (launch-latency-bound, ~345 us of host time to issue); the pool keeps `workers` of them in
 * flight so that they overlap on the device and their host cost runs in parallel.  Results are bit-identical to
 * lws_forward.  flags: 0, or LWS_POOL_SIDE_STREAMS to let every worker also use its per-handle side stream
 * (2 streams per worker; more streams than hardware queues makes throughput depend on the stream -> queue mapping).
 * `model` must outlive the pool. */
typedef struct lws_pool *lws_pool_handle;
#define LWS_POOL_SIDE_STREAMS 1
int lws_pool_create(lws_handle model, int workers, int flags, lws_pool_handle *out);
int lws_pool_destroy(lws_pool_handle p);            /* runs what is queued, then joins the workers */
int lws_pool_workers(lws_pool_handle p);
/* Pre-allocates every worker's workspace (waits for the jobs in flight first). */
int lws_pool_reserve(lws_pool_handle p, int B, int H, int W);
/* Queues one lws_forward(left, right -> pred_out[0..3]) and returns its ticket.  The job starts behind everything
 * already queued on `after_stream` (the stream that produces left / right; NULL = the default stream).  The buffers
 * must stay valid, and pred_out unread, until lws_pool_wait(ticket) has returned.  At most 4 x workers jobs are kept
 * in flight: a further submit first waits for the oldest one.  Thread-safe. */
int lws_pool_submit(lws_pool_handle p, const float *left, const float *right, int B, int H, int W,
                    float *const pred_out[4], void *after_stream, int64_t *ticket);
/* Blocks the calling thread until the job's outputs are complete in device memory; returns the job's status
 * (lws_last_error() then holds the worker's message).  A ticket may be waited for any number of times while its slot is
 * live (the 4 x workers most recent tickets); for an older, recycled ticket the job is complete by construction and its own
 * status is gone: the call then returns the pool's STICKY status -- the status and message of the first job that failed since
 * the pool was created (or since lws_pool_clear_error) -- unless the ticket is older than the SMALLEST failed ticket (those
 * jobs ran to completion: LWS_OK), so a failed forward is never reported as success once its slot has been reused.  The same sticky
 * status is returned by lws_pool_wait_all and refuses further lws_pool_submit calls until it is cleared.
 * Options are FROZEN at lws_pool_create: the workers are clones taken then; a later lws_set_option on `model` does not reach
 * them (create a new pool after changing options). */
int lws_pool_wait(lws_pool_handle p, int64_t ticket);
int lws_pool_wait_all(lws_pool_handle p);
int lws_pool_clear_error(lws_pool_handle p);          /* ABI v6 */
/* Kernel timing inside the pool (ABI v7): lws_profile_enable(class_mask) + lws_profile_sample(every_n) on every worker's
 * clone, and the per-class sums over the workers (arrays of LWS_KC_COUNT entries, as lws_profile_read).  Call both with
 * nothing in flight (after lws_pool_wait_all).  bench.py prices `pipelined` with it: k_conv3d_mid16 as it runs beside the
 * other workers' kernels. */
int lws_pool_profile_enable(lws_pool_handle p, int class_mask, int every_n);
int lws_pool_profile_read(lws_pool_handle p, double *total_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* LWSNET_HIP_H */
