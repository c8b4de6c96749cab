/* A TSDF volume seen through an integer offset: the one primitive that lets the volume of include/lwsnet_tsdf.h follow the camera
 * (additive after v8: LWS_ABI_VERSION stays 8; a header of its own that includes lwsnet_hip.h, as lwsnet_tsdf_mesh.h).
 * lwsnet_amd._lib reads this header into WINDOW_ABI.
 *
 * The volumes, as in lwsnet_tsdf.h: T float32 [Gz][Gy][Gx], x fastest; Wt float32 of the same shape; C uint8 [Gz][Gy][Gx][4] or NULL.
 * The destination T2, Wt2, C2 has the dims (Dx, Dy, Dz) and the same layout.  Destination voxel (ix, iy, iz) takes source voxel
 * (ix + sx, iy + sy, iz + sz):
 *   live = the source index lies in [0, G) on all three axes && !(Wt_src == 0)
 *          (a NaN or negative Wt is followed as it is: it is live; -0.0 compares equal to 0 and is dead; nothing is read outside [0, G))
 *   live:      T2, Wt2 and C2 (all four bytes) get the source's bits unchanged
 *   not live:  T2 = +0.0f, Wt2 = +0.0f, C2 = {0, 0, 0, 0}
 * Every element of the destination is written, whatever it held.  What an unobserved source voxel held in T and C -- a volume's T is
 * never initialised where Wt == 0 -- therefore never reaches the destination: the window also scrubs.
 * counts int64 [2] or NULL: {live, not live} voxels of the destination, which sum to Dx * Dy * Dz; summed per wave and per workgroup
 * first, then added with 64-bit integer atomics (agent scope, relaxed), whose order cannot show, as `updated` of lws_tsdf_integrate.
 * Limits: Gx, Gy, Gz and Dx, Dy, Dz each in 2..4096, Gx * Gy * Gz < 2^31 and Dx * Dy * Dz < 2^31; sx, sy, sz each in -4096..4096.  C and
 * C2 are both given or both NULL.
 * Argument errors -- a null or misaligned pointer (T, Wt, C, T2, Wt2, C2 4 bytes, counts 8), a bad shape or shift, C on one side only,
 * any overlap between a destination array or counts and anything else (the same pointer twice included) -- return LWS_ERR_INVALID
 * with a message that begins `tsdf_window: ` before any GPU call.
 * The uses: the shift of a volume that follows the camera (D = G, s = the shift in voxels; the new origin is the old one plus
 * s * vs); cutting a box out of a volume before it is shifted away, for lws_tsdf_points / lws_tsdf_mesh to extract (D = the box,
 * s = its first voxel); resizing (D != G).
 * Deliberately out of place.  An in-place shift of a 3-D array by parallel threads has no safe sweep order -- a destination may be
 * another thread's source on any of the three axes, in either direction -- and a second volume costs 12 MB at the default size of
 * 128 x 32 x 256 voxels with colour.  The caller keeps two sets of tensors and swaps them.
 * What the window does not do: re-entering space that was left is mapped afresh (the voxels that come in are cleared), so a loop
 * gives two surfaces in the chunks that were cut out; a box cut out with its neighbours missing has zero vertex normals at its
 * border, as at any volume border; a vertex on the seam of two boxes appears in both. */
#ifndef LWSNET_TSDF_WINDOW_H
#define LWSNET_TSDF_WINDOW_H
#include "lwsnet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Launches on `stream`, a list fixed by the arguments: (counts: a kernel that clears it;) one sweep of the destination, one thread
 * per four voxels along x, at most 2048 workgroups of 256 that stride over the quads.  The destination quad is stored as 16-byte
 * words where it is whole (x + 4 <= Dx) and its addresses are 16-byte aligned, scalar otherwise.  The source quad is loaded as 16-byte
 * words where it lies wholly inside the source row and its addresses are 16-byte aligned (sx a multiple of 4 on aligned bases with
 * Gx and Dx multiples of 4), scalar otherwise; a quad that straddles the source's border mixes live and cleared voxels.  Both
 * paths give the same bytes.  Nothing is read back, no scratch memory: the call can be captured into a hipGraph. */
int lws_tsdf_window(const float *T, const float *Wt, const uint8_t *C, int Gx, int Gy, int Gz, int sx, int sy, int sz, float *T2,
                    float *Wt2, uint8_t *C2, int Dx, int Dy, int Dz, int64_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif
