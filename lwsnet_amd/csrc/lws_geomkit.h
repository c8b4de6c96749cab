// What the geometry translation units share (lws_geometry.hip: depth maps and the point cloud; lws_mesh.hip: surface normals and the
// triangle mesh; lws_ground.hip: ground plane, obstacle codes and the bird's-eye grid; lws_stixels.hip: stixels; lws_objects.hip: obstacle objects): the camera row, the quad loads of a disparity row and its code map, the validity rule and the argument checks, so
// that "a valid pixel" is written once.  Contract: include/lwsnet_hip.h, lws_depth_maps.
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

static inline int check_geometry_args(const char *who, const float *disp, int B, int H, int W, float min_disp, float max_depth)
{
    LWS_CHECK_ARG(disp, "%s: disp is null", who);
    LWS_CHECK_RC(check_image_shape(who, B, H, W, 31));
    LWS_CHECK_ARG(min_disp > 0.0f && finite_nonneg(min_disp), "%s: min_disp must be finite and > 0, got %g", who, (double)min_disp);
    LWS_CHECK_ARG(max_depth > 0.0f, "%s: max_depth must be > 0 (+inf allowed), got %g", who, (double)max_depth);   // (false for NaN)
    LWS_CHECK_ARG(aligned(disp, 4), "%s: disp is not 4-byte aligned", who);
    return LWS_OK;
}

}  // namespace lws::geomkit
