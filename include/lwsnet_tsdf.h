/* Volumetric fusion of a sequence: a truncated signed distance (TSDF) volume on the device that the frames of a sequence are
 * integrated into with their poses, that is ray-cast back into any camera and extracted as an oriented, coloured point cloud
 * (additive after v8: LWS_ABI_VERSION stays 8; a header of its own that includes lwsnet_hip.h, as lwsnet_temporal.h).
 * lwsnet_amd._lib reads this header into TSDF_PROTOTYPES.
 *
 * The volume: T float32 [Gz][Gy][Gx], x fastest, the truncated signed distance in metres, positive on the free side; Wt float32 of
 * the same shape, the accumulated weight; C uint8 [Gz][Gy][Gx][4] {r, g, b, a} or NULL.  Gx, Gy, Gz in 2..4096, Gx * Gy * Gz < 2^31.
 * ox, oy, oz finite, vs finite and > 0: voxel (ix, iy, iz) has its centre at xw = ox + (float)ix * vs, yw = oy + (float)iy * vs,
 * zw = oz + (float)iz * vs.  The world frame is the one the poses refer to.  A voxel is unobserved iff Wt == 0 (Wt is never negative);
 * T and C never reach a result from there, so a volume is cleared by zeroing Wt alone.  C's a byte is 255 once a colour has been
 * written since the voxel was first observed and 0 before.
 * House rules, as lws_temporal_step: every step below is one IEEE float32 operation in the order written (no contraction, correctly
 * rounded division and square root), every compare is false on NaN, fmaxf / fminf return the other operand of a NaN.
 * M . P for a 3 x 4 M means ((m0 * X + m1 * Y) + m2 * Z) + m3 per row; R . g, its rotation alone, (m0 * X + m1 * Y) + m2 * Z.
 * pose float32 [B][2][12] in device memory, each a row-major 3 x 4 [R|t]: pose[b][0] world -> camera b, pose[b][1] camera b -> world
 * (the caller computes the inverse in float64).  cam [B][5] as lws_depth_maps.  B in 1..65535, H * W < 2^31, H, W <= 2^24.
 * Argument errors -- a null or misaligned pointer (floats and C 4 bytes, points and vnormals 16, the int64s and the workspace 8), a
 * bad shape or scalar, rgb without C or C without rgb, any overlap between an output, the volume or the workspace and anything
 * else -- return LWS_ERR_INVALID with a message before any GPU call.
 * Limits, stated and left as they are: a dense volume of fixed extent, what leaves it is not mapped; no voxel hashing and no moving
 * volume (include/lwsnet_tsdf_window.h moves one between calls); movers smear unless the caller masks them (include/lwsnet_movers.h
 * segments them); the poses are taken as given. */
#ifndef LWSNET_TSDF_H
#define LWSNET_TSDF_H
#include "lwsnet_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Integrates B frames into the volume, per voxel in the order b = 0 .. B - 1: the call equals B calls of one frame each, in bits.
 * disp [B,1,H,W]; sigma [B,1,H,W] in px or NULL (sigma0 everywhere); mask uint8 or NULL, the lws_lr_check code map (1 = usable);
 * normals float32 [B,3,H,W] or NULL, as lws_surface_normals writes them; rgb uint8 [B,H,W,3] or NULL, required iff C is given.
 * Scalars: min_disp > 0 finite, max_depth > 0 (+inf allowed), mu0 > 0 finite (metres), mu_d >= 0 finite (px), sigma0 >= 0 finite,
 * sigma_min > 0 finite, wmode 0 or 1, w_max > 0 (+inf allowed).
 * Per voxel and frame, (To, Wo, Co) the voxel's state before the frame:
 *   Pc = pose[b][0] . (xw, yw, zw);  in = Pc.z > 0
 *   u = (fx * Pc.x) / Pc.z + cx, v = (fy * Pc.y) / Pc.z + cy;  in &= 0 <= u <= (float)(W - 1) && 0 <= v <= (float)(H - 1)
 *   iu = (int)rintf(u), iv = (int)rintf(v)                                          (ONE tap; nothing is read unless `in`)
 *   d = disp[b,iv,iu];  z = fb / d;  valid = ok_mask && isfinite(d) && d >= min_disp && z <= max_depth       (lws_depth_maps)
 *   s = sigma ? sigma[b,iv,iu] : sigma0;  valid &= s >= 0 && isfinite(s);  sg = fmaxf(s, sigma_min)
 *   X = (((float)iu - cx) * z) / fx, Y = (((float)iv - cy) * z) / fy                (the point of lws_depth_maps)
 *   n = normals ? normals[b,:,iv,iu] : 0;  has_n = n.x != 0 || n.y != 0 || n.z != 0          (a NaN component: has_n)
 *   sdf = has_n ? -(((X - Pc.x) * n.x + (Y - Pc.y) * n.y) + (z - Pc.z) * n.z) : z - Pc.z
 *         (the distance to the pixel's tangent plane, positive on the camera's side: n.z < 0 faces the camera, n = (0, 0, -1) gives
 *          z - Pc.z.  The plain projective distance starves the voxels under a surface seen at a grazing angle -- a road -- of
 *          updates: they lie far behind the surface along the ray and near it along the normal.)
 *   zz = (z * z) / fb;  mu = fmaxf(mu0, mu_d * zz)       (metres of depth per pixel of disparity: the band grows as z^2)
 *   w = wmode == 0 ? 1.0f : 1.0f / ((sg * zz) * (sg * zz))                          (1 / sigma_z^2: 1 / Wt is a variance in m^2)
 *   take = in && valid && sdf >= -mu && isfinite(w) && w > 0
 *   t = fminf(sdf, mu);  Wn = Wo + w;  Tn = Wo > 0 ? (To * Wo + t * w) / Wn : t
 *   take:  T = Tn, Wt = fminf(Wn, w_max)
 *   take && C given, c the pixel rgb[b,iv,iu]:
 *     sdf <= mu:  per channel  Cn = Wo > 0 && Co.a == 255 ? sat8(rintf(((float)Co * Wo + (float)c * w) / Wn)) : c;  C.a = 255
 *                 (sat8(x) = (uint8)fminf(fmaxf(x, 0.0f), 255.0f))
 *     otherwise, and not Wo > 0:  C = {0, 0, 0, 0}       (the first touch: what C held while the voxel was unobserved is dropped)
 * updated int64 [B] or NULL: the voxels taken per frame, summed per wave and per workgroup first, then added with 64-bit integer
 * atomics (agent scope, relaxed), whose order cannot show.  A state the caller made up with a non-finite T or Wt is followed as it is.
 * Launches on `stream`, a list fixed by the arguments: (updated: a kernel that clears it;) one sweep of the volume, one thread per
 * four voxels along x, the frame loop inside the thread with the voxel's state in registers; T, Wt and C are loaded once some frame
 * takes one of the four voxels and stored only then, as 16-byte words where the quad is whole and 16-byte aligned, scalar otherwise.
 * Nothing is read back, no scratch memory: the call can be captured into a hipGraph. */
int lws_tsdf_integrate(const float *disp, const float *sigma, const uint8_t *mask, const float *normals, const uint8_t *rgb,
                       const float *cam, const float *pose, int B, int H, int W, float *T, float *Wt, uint8_t *C, int Gx, int Gy, int Gz,
                       float ox, float oy, float oz, float vs, float sigma0, float min_disp, float max_depth, float mu0, float mu_d,
                       float sigma_min, int wmode, float w_max, int64_t *updated, void *stream);

/* Casts B views of H x W from the volume.  Scalars: z_near > 0 finite, step > 0 finite, nsteps in 2..65535, w_min >= 0 finite.
 * sample(Pw): g = (Pw - o) / vs per axis;  inside = 0 <= g < (float)(G - 1) on all three axes (tested before the cast);
 *   i0 = (int)floorf(g), a = g - (float)i0 per axis;  the eight taps (i0 + 0/1) of Wt;  known = inside && every tap > 0 && >= w_min
 *   f = lerp(lerp(lerp(t000, t001, a.x), lerp(t010, t011, a.x), a.y), lerp(lerp(t100, t101, a.x), lerp(t110, t111, a.x), a.y), a.z),
 *   t_zyx the taps of T, lerp(p, q, s) = p + s * (q - p): along x, then y, then z;  wf the same blend of the Wt taps
 * Per pixel (y, x):  xn = ((float)x - cx) / fx, yn = ((float)y - cy) / fy;  ray(zc) = pose[b][1] . (xn * zc, yn * zc, zc)
 *   for k = 0 .. nsteps - 1:  zc = z_near + (float)k * step;  (f, known) = sample(ray(zc))
 *     known && prev_known && fp >  0 && f <= 0  ->  hit:  zs = zp + (fp / (fp - f)) * (zc - zp);  stop
 *     known && prev_known && fp <= 0 && f >  0  ->  miss (the ray left the back of a surface);  stop
 *     else (prev_known, fp, zp) = (known, f, zc)                                    (prev_known is false before k = 0)
 * Outputs, every element written: disp float32 [B,1,H,W] = fb / zs, 0 for a miss; weight float32 [B,1,H,W] or NULL: wf of
 * sample(Ph), Ph = ray(zs), where that sample is inside, else 0, and 0 for a miss; normals float32 [B,3,H,W] or NULL: the six
 * samples at Ph with vs added to (+) and subtracted from (-) one world coordinate; all six known: gw = (f+x - f-x, f+y - f-y,
 * f+z - f-z), g = R . gw with pose[b][0]'s rotation, len = sqrtf((g.x * g.x + g.y * g.y) + g.z * g.z), n = g / len (three
 * divisions) if len is finite and > 0; zero otherwise and for a miss.  The gradient points to the free side: a surface that
 * faces the camera has n.z < 0, the convention of lws_surface_normals.
 * One launch, one thread per pixel; the loop's exit depends on the data, the launch does not.  Every step of every ray samples the
 * volume: empty-space skipping through a coarse occupancy level is out of scope. */
int lws_tsdf_raycast(const float *T, const float *Wt, int Gx, int Gy, int Gz, float ox, float oy, float oz, float vs, const float *cam,
                     const float *pose, int B, int H, int W, float z_near, float step, int nsteps, float w_min, float *disp, float *weight,
                     float *normals, void *stream);

/* bytes of device workspace lws_tsdf_points needs: one int64 per x-row of the volume */
int64_t lws_tsdf_points_workspace(int Gy, int Gz);
/* The zero crossings of T on the voxel grid's edges as points, packed in a fixed order: voxel a = (ix, iy, iz) in raster order
 * (z, y, x), and for each a the axes e = x, y, z in that order.  b = a + e must be inside the volume and both voxels observed:
 * Wt > 0 && Wt >= w_min (w_min >= 0 finite).  A point is emitted iff (Ta > 0 && Tb <= 0) || (Ta <= 0 && Tb > 0):
 *   s = Ta / (Ta - Tb);  its position is a's centre with s * vs added along e (one multiplication, one addition)
 *   near = a iff s <= 0.5f, else b;  its colour is C[near], all four bytes, or {255, 255, 255, 255} when C is NULL
 *   its normal: near's six neighbours all inside the volume and observed: g = (T[x+1] - T[x-1], T[y+1] - T[y-1], T[z+1] - T[z-1]),
 *   len = sqrtf((g.x * g.x + g.y * g.y) + g.z * g.z), n = g / len if len is finite and > 0; zero otherwise (world frame)
 * points: 16 bytes per record {float X, Y, Z; uint8 r, g, b, a}, the record of lws_point_cloud; vnormals {n.x, n.y, n.z, 0.0f} per
 * record, or NULL; max_points in 1 .. 2^31 - 1, the capacity of both in records.  counts int64 [1]: the number of crossings, however
 * many fit; only records of rank < max_points are written and nothing past them is touched.
 * Three launches, as lws_point_cloud: per x-row counts, an exclusive scan in the workspace, a scatter ranked by wave ballots.  No
 * atomics: the same bytes on every run.  workspace: lws_tsdf_points_workspace bytes, contents undefined before and after.
 * The triangles between these points: lws_tsdf_mesh (include/lwsnet_tsdf_mesh.h), whose vertex list is this record list. */
int lws_tsdf_points(const float *T, const float *Wt, const uint8_t *C, int Gx, int Gy, int Gz, float ox, float oy, float oz, float vs,
                    float w_min, int64_t max_points, void *workspace, void *points, float *vnormals, int64_t *counts, void *stream);

#ifdef __cplusplus
}
#endif
#endif
