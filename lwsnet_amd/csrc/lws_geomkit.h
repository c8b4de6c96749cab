// What the geometry translation units share (lws_geometry.hip: depth maps and the point cloud; lws_mesh.hip: surface normals and the
// triangle mesh; lws_ground.hip: ground plane, obstacle codes and the bird's-eye grid; lws_stixels.hip: stixels; lws_objects.hip:
// obstacle objects; lws_temporal.hip: temporal fusion; lws_egomotion.hip: ego-motion; lws_tsdf.hip: the TSDF volume): the camera
// row, the quad loads of a disparity row and its code map, the validity rule and the argument checks, so that "a valid pixel" is
// written once (contract: include/lwsnet_hip.h, lws_depth_maps); and what the sequence ops share on top: a pixel to its point and
// back, the pose block, the four-tap blend and jump.  Every function here is the float32 operations it shows in the order it
// shows them: the numpy references restate them.
#pragma once
#include "lws_common.h"
#include "lws_opkit.h"

namespace lws::geomkit {

using namespace opkit;

// One row of cam[B][5]
struct Cam {
    float fx, fy, cx, cy, fb;
};

__device__ __forceinline__ Cam load_cam(const float *__restrict__ cam, int b)
{
    const float *c = cam + 5 * (int64_t)b;
    return Cam{c[0], c[1], c[2], c[3], c[4]};
}

// The 4 pixels x .. x+3 of a row: float4 where the row is 16-byte aligned, scalar for a misaligned row and the tail (NaN beyond
// the row: never valid).
__device__ __forceinline__ void load_quad(const float *__restrict__ p, int x, int W, bool vec, float d[4])
{
    if (vec && x + 4 <= W) {
        const float4 v = *reinterpret_cast<const float4 *>(p + x);
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    } else {
        const float nan = __builtin_nanf("");
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = x + i < W ? p[x + i] : nan;
    }
}

// ok_mask of the 4 pixels: mask == NULL, or the lws_lr_check code is 1
__device__ __forceinline__ void load_ok(const uint8_t *__restrict__ m, int x, int W, bool vec, bool ok[4])
{
    if (!m) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ok[i] = true;
    } else if (vec && x + 4 <= W) {
        const uchar4 v = *reinterpret_cast<const uchar4 *>(m + x);
        ok[0] = v.x == 1, ok[1] = v.y == 1, ok[2] = v.z == 1, ok[3] = v.w == 1;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) ok[i] = x + i < W && m[x + i] == 1;
    }
}

// The validity rule shared by lws_depth_maps, lws_point_cloud, lws_surface_normals, lws_surface_mesh, lws_ground_classify,
// lws_bev_grid, lws_stixels and lws_objects; z = fb / d is returned for every pixel.
__device__ __forceinline__ bool valid_z(float d, bool ok, float fb, float min_disp, float max_depth, float &z)
{
    z = fb / d;
    return ok && __builtin_isfinite(d) && d >= min_disp && z <= max_depth;
}

// X and Y of pixel column x / row y at depth z
__device__ __forceinline__ float back_x(const Cam &c, int x, float z) { return (((float)x - c.cx) * z) / c.fx; }
__device__ __forceinline__ float back_y(const Cam &c, int y, float z) { return (((float)y - c.cy) * z) / c.fy; }

// The pixel (u, v) of the point P, and whether it lies in the image less `margin` columns and rows at every edge (false for a
// NaN).  The caller asks for Pz > 0.
__device__ __forceinline__ bool project(const Cam &c, float Px, float Py, float Pz, int H, int W, int margin, float &u, float &v)
{
    u = (c.fx * Px) / Pz + c.cx;
    v = (c.fy * Py) / Pz + c.cy;
    return u >= (float)margin && u <= (float)(W - 1 - margin) && v >= (float)margin && v <= (float)(H - 1 - margin);
}

// pose[B][2][12]: image b's row-major 3 x 4 [R|t] and, 12 floats on, its inverse
constexpr int kPoseFloats = 24, kPoseInverse = 12;
__device__ __forceinline__ const float *pose_of(const float *__restrict__ pose, int b) { return pose + kPoseFloats * (int64_t)b; }
__device__ __forceinline__ const float *inverse_of(const float *__restrict__ pose, int b) { return pose_of(pose, b) + kPoseInverse; }

// row r of the 3 x 4 matrix m applied to (X, Y, Z); rot_dot: its rotation alone
__device__ __forceinline__ float row_dot(const float *__restrict__ m, int r, float X, float Y, float Z)
{
    return ((m[4 * r] * X + m[4 * r + 1] * Y) + m[4 * r + 2] * Z) + m[4 * r + 3];
}
__device__ __forceinline__ float rot_dot(const float *__restrict__ m, int r, float X, float Y, float Z)
{
    return (m[4 * r] * X + m[4 * r + 1] * Y) + m[4 * r + 2] * Z;
}

// The four taps t00 t01 / t10 t11 blended with the weights a (across) and b (down), and their largest difference
__device__ __forceinline__ float lerp(float p, float q, float s) { return p + s * (q - p); }
__device__ __forceinline__ float blend4(float t00, float t01, float t10, float t11, float a, float b)
{
    return lerp(lerp(t00, t01, a), lerp(t10, t11, a), b);
}
__device__ __forceinline__ float jump4(float t00, float t01, float t10, float t11)
{
    float mx = t00, mn = t00;
    mx = t01 > mx ? t01 : mx, mx = t10 > mx ? t10 : mx, mx = t11 > mx ? t11 : mx;
    mn = t01 < mn ? t01 : mn, mn = t10 < mn ? t10 : mn, mn = t11 < mn ? t11 : mn;
    return mx - mn;
}

// A view is projected into: its pixel coordinates, up to (float)(W - 1) and (float)(H - 1), have to be exact floats
constexpr int kMaxViewDim = 1 << 24;
static inline int check_view_shape(const char *who, int B, int H, int W)
{
    LWS_CHECK_RC(check_image_shape(who, B, H, W, 31));
    LWS_CHECK_ARG(H <= kMaxViewDim && W <= kMaxViewDim, "%s: H=%d W=%d exceed %d (pixel coordinates are exact floats)", who, H, W, kMaxViewDim);
    return LWS_OK;
}

static inline int check_geometry_args(const char *who, const float *disp, int B, int H, int W, float min_disp, float max_depth)
{
    LWS_CHECK_ARG(disp, "%s: disp is null", who);
    LWS_CHECK_RC(check_image_shape(who, B, H, W, 31));
    LWS_CHECK_ARG(finite_pos(min_disp),"%s: min_disp must be finite and > 0, got %g", who, (double)min_disp);
    LWS_CHECK_ARG(max_depth > 0.0f, "%s: max_depth must be > 0 (+inf allowed), got %g", who, (double)max_depth);   // (false for NaN)
    LWS_CHECK_ARG(aligned(disp, 4), "%s: disp is not 4-byte aligned", who);
    return LWS_OK;
}

}  // namespace lws::geomkit
