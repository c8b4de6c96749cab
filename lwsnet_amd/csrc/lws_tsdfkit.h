// What the read-only calls on a TSDF volume share: the volume as a kernel sees it, the crossings on a voxel's three edges and the
// normal of a voxel -- the rules of lws_tsdf_points (include/lwsnet_tsdf.h), which lws_tsdf_mesh (lws_tsdf_mesh.hip) numbers its
// vertices by -- and the two host steps both calls take: the check of a volume's arguments and the three launches that extract the
// points (defined in lws_tsdf.hip, beside the kernels they launch).
#pragma once
#include "lws_geomkit.h"
#include "lws_packkit.h"

namespace lws::tsdfkit {

using namespace geomkit;

constexpr int kMaxGrid = 4096;

// g / |g| as lws_surface_normals normalises, zero where the length is not finite or not > 0
__device__ __forceinline__ void normalise(float gx, float gy, float gz, float n[3])
{
    const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
    const bool good = __builtin_isfinite(len) && len > 0.0f;
    n[0] = good ? gx / len : 0.0f, n[1] = good ? gy / len : 0.0f, n[2] = good ? gz / len : 0.0f;
}

struct Vol {                                                // the volume as the read-only kernels see it
    const float *T, *Wt;
    int Gx, Gy, Gz;
    float ox, oy, oz, vs, w_min;
};

__device__ __forceinline__ bool observed(float w, float w_min) { return w > 0.0f && w >= w_min; }

// The crossings on the three edges that leave voxel (ix, iy, iz) towards +x, +y, +z: bit e = axis e; Ta and Tb[e] of a set bit.
__device__ __forceinline__ unsigned edge_bits(const Vol &v, int ix, int iy, int iz, float &Ta, float Tb[3])
{
    const int i = (iz * v.Gy + iy) * v.Gx + ix;
    if (!observed(v.Wt[i], v.w_min)) return 0u;
    Ta = v.T[i];
    const int stride[3] = {1, v.Gx, v.Gy * v.Gx};
    const bool in[3] = {ix + 1 < v.Gx, iy + 1 < v.Gy, iz + 1 < v.Gz};
    unsigned bits = 0u;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        Tb[e] = 0.0f;
        if (!in[e] || !observed(v.Wt[i + stride[e]], v.w_min)) continue;
        Tb[e] = v.T[i + stride[e]];
        bits |= ((Ta > 0.0f && Tb[e] <= 0.0f) || (Ta <= 0.0f && Tb[e] > 0.0f) ? 1u : 0u) << e;
    }
    return bits;
}

// the central difference of T over the six neighbours of voxel (ix, iy, iz), normalised; zero unless all six are inside and observed
__device__ __forceinline__ void voxel_normal(const Vol &v, int ix, int iy, int iz, float n[3])
{
    n[0] = n[1] = n[2] = 0.0f;
    if (ix < 1 || iy < 1 || iz < 1 || ix + 1 >= v.Gx || iy + 1 >= v.Gy || iz + 1 >= v.Gz) return;
    const int i = (iz * v.Gy + iy) * v.Gx + ix, sy = v.Gx, sz = v.Gy * v.Gx;
    const int o[6] = {i + 1, i - 1, i + sy, i - sy, i + sz, i - sz};
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (!observed(v.Wt[o[k]], v.w_min)) return;
    normalise(v.T[o[0]] - v.T[o[1]], v.T[o[2]] - v.T[o[3]], v.T[o[4]] - v.T[o[5]], n);
}

// ---- host (lws_tsdf.hip) ----
// the checks of a volume's pointers, shape, origin and voxel that every TSDF call begins with; messages start with `who`
int check_volume(const char *who, const float *T, const float *Wt, int Gx, int Gy, int Gz, float ox, float oy, float oz, float vs);

// The three launches of lws_tsdf_points on `st`: per x-row counts into rows[Gy * Gz], their exclusive scan in place with the total
// in counts[0], the ranked scatter of the records of rank < max_points.  The arguments have been checked by the caller.
int launch_points(const Vol &v, const uint8_t *C, int64_t max_points, int64_t *rows, void *points, float *vnormals, int64_t *counts,
                  hipStream_t st);

}  // namespace lws::tsdfkit
