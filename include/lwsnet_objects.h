/* Obstacle objects on top of the ground and stixel calls of lwsnet_hip.h (additive after v8: LWS_ABI_VERSION stays 8).
 * lwsnet_hip.h is the table of the 66 entry points of ABI v8 as it was frozen; entry points added behind it without a new ABI
 * version come in a header of their own that includes it, so that a caller built against v8 reads the same table as before.
 * lwsnet_amd._lib reads this header too (EXTENSION_PROTOTYPES); the library exports these symbols beside the others. */
#ifndef LWSNET_OBJECTS_H
#define LWSNET_OBJECTS_H
#include "lwsnet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device workspace lws_objects needs for this geometry: per cell of the u-disparity image (S = ceil(W / width) strips x
 * nbins bins) one int32 parent word and one record of 16 words (68 bytes), and four int32 per block of 2048 cells of an image,
 * each part rounded up to 256 bytes */
int64_t lws_objects_workspace(int B, int W, int width, int nbins);
/* Obstacle objects: which pixels belong to the same thing, and where that thing is and how large.  The objects are the connected
 * components of the occupied cells of the u-disparity image; each pixel is mapped back to its cell's component, and the pixels of
 * a component are reduced to a box in the image and a box in camera coordinates.
 * disp, cam, codes, min_disp, max_depth, width, sub, nbins: exactly as lws_stixels, with the same limits (H, W <= 16384; width in
 * 1..64; sub in 1..16; nbins in 1..4096 and <= 256 * sub); cam and codes are required.  S * nbins <= 2^22 cells (the workspace
 * stays below 286 MB per image).  code_bits in 0..63: no height is read, so no bit is
 * refused.  udisp uint32 [B,S,nbins]: what lws_stixels wrote for the same map and parameters.  min_count >= 1, min_pixels >= 1,
 * max_objects in 1..65536.
 *   take(p), q, Q   the definitions of lws_stixels: take(p) = valid (the rule of lws_depth_maps without a mask) && codes[p] < 6 with
 *                   bit codes[p] of code_bits set && t = floorf(d * (float)sub) < (float)nbins;  q = (int)t;  Q = (int)u16(d)
 *   occupied        the cell (s, k) is occupied iff udisp[b,s,k] >= min_count
 *   joined          two occupied cells (s, k), (s', k') are joined iff |s - s'| <= 1 && |k - k'| <= 1 (8-neighbours); a component is a
 *                   class of the transitive closure
 *   member          a pixel p = (x, y) is a member of a component iff take(p) and its own cell (x / width, q) is an occupied cell of
 *                   that component; a taking pixel in a cell that is not occupied belongs to nothing
 * The call is a pure function of its inputs as they are, also when udisp is not the histogram of this map: occupied and joined
 * read udisp alone, member reads the map and the occupied cells; a component may then have no member at all.
 * Per component:
 *   cells           the number of its occupied cells;  k_min, k_max: the smallest and the largest bin of its occupied cells
 *   over its members: n = their count;  x_min, x_max, y_min, y_max = their pixel box;  SQ = the int64 sum of Q;  and the minima and
 *                   maxima of the float32 X, Y, Z of lws_depth_maps -- z = fb / d;  X = (((float)x - cx) * z) / fx;
 *                   Y = (((float)y - cy) * z) / fy;  Z = z, each per pixel with its operations in this order, no fma -- in the order
 *                   -inf < ... < -0.0f < +0.0f < ... < +inf.  A NaN cannot occur: a valid pixel has a finite d >= min_disp > 0
 *   kept            iff n >= min_pixels
 *   root            every cell has the index c = (nbins - 1 - k) * S + s; a component's root is its smallest c: its nearest cell, the
 *                   leftmost one on a tie
 *   numbered        the kept components j = 0, 1, .. by increasing root: object 0 is the one whose nearest cell is nearest
 * Outputs; every element is written, the caller clears nothing:
 *   rows   int32 [B,max_objects,8] = {n, x_min, x_max, y_min, y_max, k_min, k_max, cells} of object j
 *   vals   float32 [B,max_objects,8] = {d, z, X_min, X_max, Y_min, Y_max, Z_min, Z_max};  d = (float)(((double)SQ / (double)n) / 256.0)
 *          and z = fb / d, as a stixel's.  A slot j >= the number of kept components holds {0, -1, -1, -1, -1, -1, -1, 0} and eight
 *          +0.0f.  Kept components with j >= max_objects are counted but not written
 *   labels int32 [B,1,H,W] (NULL: skipped) = j for a member of a kept component with j < max_objects, -1 for every other pixel
 *   info   int32 [B][4] = {occupied cells, components, kept components (before the cap), member pixels of the kept components}
 * Argument errors -- a null or misaligned pointer (4 bytes; the workspace 16), a bad shape or range, any overlap between inputs,
 * outputs and the workspace -- return LWS_ERR_INVALID with a message before any GPU call.  workspace: lws_objects_workspace(B, W,
 * width, nbins) bytes, contents undefined before and after: the call clears what it uses.  Eight launches on `stream`, nine with
 * labels -- the cells labelled per tile of 64 strips x 32 bins in LDS (union-find), unions across the tile edges, flatten; every
 * member pixel into its cell's record (one workgroup per strip, the lanes of a wave that hit its first cell combined first); every
 * cell's record into its root's; the kept roots numbered in c order by the three-launch scan of lws_point_cloud (per-block counts, a
 * per-image exclusive scan with info and the empty slots, the ranked write of rows and vals); the labels -- a fixed
 * list that depends on the arguments but never on the data, with no device-to-host read, so the call can be captured into a
 * hipGraph.  What crosses lanes or workgroups is an integer add, min or max (the float minima and maxima on the monotone key:
 * all bits of a negative float flipped, the sign bit of a non-negative one set), whose order cannot show: every output is the same
 * bytes in any batch, at any position in it, on every run.  No scratch memory.
 * Limits, stated and left as they are: an object split in the image by a nearer one comes out as two components; things that touch
 * in (strip, bin) merge; a surface whose disparity changes by more than one bin between neighbouring strips without covering the
 * bins in between is fragmented (a continuous slanted wall covers them).  Tracking over frames is not here. */
int lws_objects(const float *disp, const float *cam, const uint8_t *codes, const uint32_t *udisp, int B, int H, int W, float min_disp,
                float max_depth, int code_bits, int width, int sub, int nbins, int min_count, int min_pixels, int max_objects,
                void *workspace, int32_t *rows, float *vals, int32_t *labels, int32_t *info, void *stream);

#ifdef __cplusplus
}
#endif
#endif
