/* A triangle mesh of a TSDF volume's zero level set: marching cubes on the device, whose vertex list is exactly the record list of
 * lws_tsdf_points (include/lwsnet_tsdf.h) and whose faces index that list (additive after v8: LWS_ABI_VERSION stays 8; a header of
 * its own that includes lwsnet_hip.h, as lwsnet_tsdf.h).  lwsnet_amd._lib reads this header into MESH_ABI.
 *
 * The volume, as in lwsnet_tsdf.h: T float32 [Gz][Gy][Gx], x fastest, positive on the free side; Wt float32 of the same shape; C uint8
 * [Gz][Gy][Gx][4] or NULL.  Gx, Gy, Gz in 2..4096, Gx * Gy * Gz < 2^31; ox, oy, oz finite, vs finite and > 0; w_min >= 0 finite.  A
 * voxel is observed iff Wt > 0 && Wt >= w_min.
 * House rules, as lws_tsdf_points: every step is one IEEE float32 operation in the order written (no contraction, correctly rounded
 * division and square root), every compare is false on NaN.  No atomics: the same bytes on every run.
 * Argument errors -- a null or misaligned pointer (T, Wt, C and faces 4 bytes, points and vnormals 16, counts and the workspace 8), a
 * bad shape or scalar, any overlap between an output or the workspace and anything else -- return LWS_ERR_INVALID with a message
 * that begins `tsdf_mesh: ` before any GPU call.
 * Limits, stated and left as they are: a vertex that no face uses stays in the list (as in lws_surface_mesh); a surface next to
 * unobserved space ends in a boundary and is not capped; a corner with T == 0 exactly gives degenerate triangles (two or three of a
 * triangle's vertices at one place), which are kept; no decimation; the inside of an ambiguous cube is not told apart (no MC33):
 * the faces of a cube always separate its positive corners. */
#ifndef LWSNET_TSDF_MESH_H
#define LWSNET_TSDF_MESH_H
#include "lwsnet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the most triangles a case of the table holds (the construction below, run over all 256 cases) */
#define LWS_TSDF_MESH_MAX_TRIS 5

/* bytes of device workspace lws_tsdf_mesh needs: one int64 per x-row of the volume (Gy * Gz) and one per row of cubes
 * ((Gy - 1) * (Gz - 1)), each part rounded up to 256 bytes */
int64_t lws_tsdf_mesh_workspace(int Gy, int Gz);

/* Vertices: points (16-byte records), vnormals (or NULL) and counts[0] are what lws_tsdf_points writes for the same T, Wt, C, grid,
 * w_min and max_points, bit for bit: the crossings of T on the grid's edges in the order voxel (z, y, x), then axis x, y, z.
 *
 * Cubes: a = (ix, iy, iz) with ix < Gx - 1, iy < Gy - 1, iz < Gz - 1.  Corner k = dx + 2 * dy + 4 * dz is voxel a + (dx, dy, dz);
 * pos_k = T_k > 0 (false for NaN); the case is the sum of pos_k << k.  A cube is valid iff all eight corners are observed and no
 * corner's T is NaN; on each of the twelve edges of a valid cube pos differs exactly where lws_tsdf_points emits a crossing.  An
 * invalid cube emits nothing.
 * Edges: the edge that leaves the owner corner (dx, dy, dz) towards +e has the id 4 * e + j, j = dy + 2 * dz for e = x, dx + 2 * dz
 * for e = y, dx + 2 * dy for e = z.  Its vertex index is the rank of that crossing in lws_tsdf_points' order: the crossings of the
 * x-rows before the owner voxel's, plus those of its row at smaller ix, plus the owner's crossings on earlier axes.
 * The table, [256][32] bytes, by construction: on each of the cube's six faces the crossing edges are joined by segments -- two
 * crossings by one segment, four by two segments that each cut off one POSITIVE corner, so that the non-positive corners stay
 * joined across the face.  The segments depend on the face's four signs only: two cubes that share a face agree on them.  A segment
 * is directed so that, seen from outside the cube, its positive corner(s) lie on its left.  Every crossing edge lies on two faces, so
 * the directed segments close into loops; a loop starts at its smallest edge id, v0, v1, .., v(k-1), and is fanned as (v0, vi, vi+1),
 * i = 1 .. k - 2; the loops of a case go in the order of their smallest edge ids.  Row c: byte 0 = n triangles, bytes 1 .. 3n their
 * edge ids in that order, the rest 255; n <= LWS_TSDF_MESH_MAX_TRIS.  With only corner 0 non-positive the one triangle is
 * x-edge 0 -> y-edge 4 -> z-edge 8, whose normal cross(v1 - v0, v2 - v0) is (+, +, +): it points to the free side, as the gradient
 * normals of lws_tsdf_points do.  A directed triangle edge on a cube's face never meets its reverse inside the cube, and the fan
 * edges inside a cube cancel: two valid cubes that share a face always close.
 * Faces: int32 [max_faces][3], the cubes in raster order (z, y, x), a cube's triangles in the table's order, each the three vertex
 * indices of its edges.  counts int64 [2]: counts[0] the vertices, counts[1] the faces, however many fit.  Only faces of rank
 * < max_faces are written and nothing past them is touched.  If counts[0] > max_points no face is written -- a mesh whose vertices
 * do not fit is not a mesh -- and counts still holds both totals.  max_points and max_faces each in 1 .. 2^31 - 1.
 * Launches on `stream`, a list fixed by the arguments: the three of lws_tsdf_points (count, scan, scatter); the faces of each row of
 * cubes (iy, iz) counted; their exclusive scan, with counts[1]; the face scatter, one workgroup of 256 per row of cubes, which ranks
 * the crossings of the four x-rows a cube touches in chunks of 256 voxels (255 cubes) and the triangles by a scan of the per-cube
 * count.  counts[0] > max_points is tested inside that kernel: nothing is read back, no scratch memory, the call can be captured
 * into a hipGraph.  workspace: lws_tsdf_mesh_workspace bytes, contents undefined before and after. */
int lws_tsdf_mesh(const float *T, const float *Wt, const uint8_t *C, int Gx, int Gy, int Gz, float ox, float oy, float oz, float vs,
                  float w_min, int64_t max_points, int64_t max_faces, void *workspace, void *points, float *vnormals,
                  int32_t *faces, int64_t *counts, void *stream);

/* The case table, [256][32] bytes, to host memory: no GPU call.  Returns LWS_ERR_INVALID for a null pointer. */
int lws_tsdf_mesh_table(uint8_t *table);

#ifdef __cplusplus
}
#endif
#endif
