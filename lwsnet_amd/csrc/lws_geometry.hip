// Geometry of a disparity map: metric depth, KITTI's 16-bit disparity / depth PNG values and a coloured point cloud of the pixels
// to trust.  Arithmetic contract (include/lwsnet_hip.h, lws_depth_maps): one IEEE float32 operation per step (the build has no
// contraction and correctly rounded division), so tests/geometry_reference.py restates every output bit for bit in numpy.
// Determinism: no atomics; the point cloud is packed in raster order by a per-row count, a per-image scan and a per-row scatter
// whose ranks come from wave ballots, so an image gives the same bytes in any batch.  0 bytes of scratch.
#include "lws_geomkit.h"
#include "lws_packkit.h"

namespace lws {

namespace {

using namespace geomkit;
using namespace packkit;                                    // kThreads, kWaves

// KITTI's 16-bit PNG value of v (> 0): v * 256 rounded half to even, clamped to 0 .. 65535
__device__ __forceinline__ uint16_t to_u16x256(float v)
{
    return (uint16_t)fminf(fmaxf(rintf(v * 256.0f), 0.0f), 65535.0f);
}

// grid (ceil(H * nq / 256), B): one thread per quad of a row.
__global__ __launch_bounds__(kThreads) void k_depth_maps(const float *__restrict__ disp, const uint8_t *__restrict__ mask,
                                                        const float *__restrict__ cam, int H, int W, int nq, float min_disp,
                                                        float max_depth, float *__restrict__ depth, uint16_t *__restrict__ depth16,
                                                        uint16_t *__restrict__ disp16)
{
    const int g = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
    if (g >= H * nq) return;
    const int y = g / nq, x = 4 * (g - y * nq);
    const int64_t row = ((int64_t)b * H + y) * W;
    const float *dp = disp + row;
    const uint8_t *mk = mask ? mask + row : nullptr;
    float d[4];
    bool ok[4];
    load_quad(dp, x, W, aligned(dp, 16), d);
    load_ok(mk, x, W, aligned(mk, 4), ok);
    const bool full = x + 4 <= W;
    if (disp16) {
        uint16_t v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = ok[i] && __builtin_isfinite(d[i]) && d[i] > 0.0f ? to_u16x256(d[i]) : (uint16_t)0;
        uint16_t *p = disp16 + row;
        if (full && aligned(p + x, 8)) {
            *reinterpret_cast<ushort4 *>(p + x) = make_ushort4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < W) p[x + i] = v[i];
        }
    }
    if (!depth && !depth16) return;
    const Cam c = load_cam(cam, b);
    float zo[4];
    uint16_t z16[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float z;
        const bool v = valid_z(d[i], ok[i], c.fb, min_disp, max_depth, z);
        zo[i] = v ? z : 0.0f;
        z16[i] = v ? to_u16x256(z) : (uint16_t)0;
    }
    if (depth) {
        float *p = depth + row;
        if (full && aligned(p + x, 16)) {
            *reinterpret_cast<float4 *>(p + x) = make_float4(zo[0], zo[1], zo[2], zo[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < W) p[x + i] = zo[i];
        }
    }
    if (depth16) {
        uint16_t *p = depth16 + row;
        if (full && aligned(p + x, 8)) {
            *reinterpret_cast<ushort4 *>(p + x) = make_ushort4(z16[0], z16[1], z16[2], z16[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < W) p[x + i] = z16[i];
        }
    }
}

// The valid bits of the quad q (pixels 4q .. 4q+3) of row y of image b: bit i = pixel 4q + i; z[i] = its depth.
__device__ __forceinline__ unsigned quad_valid(const float *__restrict__ dp, const uint8_t *__restrict__ mk, bool vd, bool vm, int q,
                                               int W, const Cam &c, float min_disp, float max_depth, float d[4], float z[4])
{
    bool ok[4];
    load_quad(dp, 4 * q, W, vd, d);
    load_ok(mk, 4 * q, W, vm, ok);
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) bits |= (valid_z(d[i], ok[i], c.fb, min_disp, max_depth, z[i]) ? 1u : 0u) << i;
    return bits;
}

// grid (H, B), 256 threads: the valid pixels of each row -> row_count[b * H + y].
__global__ __launch_bounds__(kThreads) void k_pc_count(const float *__restrict__ disp, const uint8_t *__restrict__ mask,
                                                      const float *__restrict__ cam, int H, int W, float min_disp, float max_depth,
                                                      int *__restrict__ row_count)
{
    __shared__ int s_n[kWaves];
    const int y = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int64_t row = ((int64_t)b * H + y) * W;
    const float *dp = disp + row;
    const uint8_t *mk = mask ? mask + row : nullptr;
    const bool vd = aligned(dp, 16), vm = aligned(mk, 4);
    const Cam c = load_cam(cam, b);
    const int nq = (W + 3) >> 2;
    int n = 0;
    for (int q = t; q < nq; q += kThreads) {
        float d[4], z[4];
        n += __builtin_popcount(quad_valid(dp, mk, vd, vm, q, W, c, min_disp, max_depth, d, z));
    }
    n = block_sum(n, s_n);
    if (t == 0) row_count[(int64_t)b * H + y] = n;
}

// grid (B), 256 threads: row_count[b][.] -> its exclusive scan, in place (packkit::row_scan); counts[b] = the total.
__global__ __launch_bounds__(kThreads) void k_pc_scan(int *__restrict__ row, int H, int64_t *__restrict__ counts)
{
    __shared__ int s_w[kWaves];
    const int b = blockIdx.x;
    const int total = row_scan(row + (int64_t)b * H, H, s_w);
    if (threadIdx.x == 0) counts[b] = total;
}

// grid (H, B), 256 threads: the valid pixels of row y of image b, in raster order, to points + (b * H * W + row_off[b][y]) * 16 B.
// A chunk is 256 quads; in it, the rank of pixel i of quad q is the valid pixels of the chunk's earlier quads (packkit::block_rank,
// one bit slot per pixel) plus the valid pixels of q before i.
__global__ __launch_bounds__(kThreads) void k_pc_scatter(const float *__restrict__ disp, const uint8_t *__restrict__ mask,
                                                        const uint8_t *__restrict__ rgb, const float *__restrict__ cam, int H, int W,
                                                        float min_disp, float max_depth, const int *__restrict__ row_off,
                                                        uint4 *__restrict__ points)
{
    __shared__ int s_w[kWaves];
    const int y = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int64_t row = ((int64_t)b * H + y) * W;
    const float *dp = disp + row;
    const uint8_t *mk = mask ? mask + row : nullptr;
    const uint8_t *cp = rgb ? rgb + 3 * row : nullptr;
    const bool vd = aligned(dp, 16), vm = aligned(mk, 4), vc = aligned(cp, 4);
    const Cam c = load_cam(cam, b);
    uint4 *out = points + (int64_t)b * H * W + row_off[(int64_t)b * H + y];
    const int nq = (W + 3) >> 2;
    int carry = 0;                                          // uniform: the valid pixels of the earlier chunks
    for (int q0 = 0; q0 < nq; q0 += kThreads) {
        const int q = q0 + t;
        float d[4], z[4];
        const unsigned bits = q < nq ? quad_valid(dp, mk, vd, vm, q, W, c, min_disp, max_depth, d, z) : 0u;
        int rank = block_rank<4>(bits, s_w, carry);
        if (bits) {
            const int x = 4 * q;
            uint8_t px[12];
            if (!cp) {
#pragma unroll
                for (int k = 0; k < 12; ++k) px[k] = 255;
            } else if (vc && x + 4 <= W) {
                const unsigned *v = reinterpret_cast<const unsigned *>(cp + 3 * x);     // 4-byte aligned: 3 * x = 12 q
                const unsigned w3[3] = {v[0], v[1], v[2]};
#pragma unroll
                for (int k = 0; k < 12; ++k) px[k] = (uint8_t)(w3[k >> 2] >> (8 * (k & 3)));
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) px[k] = x + k / 3 < W ? cp[3 * x + k] : (uint8_t)0;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!((bits >> i) & 1u)) continue;
                const float X = back_x(c, x + i, z[i]), Y = back_y(c, y, z[i]);
                const unsigned col = (unsigned)px[3 * i] | ((unsigned)px[3 * i + 1] << 8) | ((unsigned)px[3 * i + 2] << 16) | (255u << 24);
                out[rank] = make_uint4(__float_as_uint(X), __float_as_uint(Y), __float_as_uint(z[i]), col);
                ++rank;
            }
        }
        __syncthreads();                                    // s_w is rewritten by the next chunk
    }
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int lws_depth_maps(const float *disp, const uint8_t *mask, const float *cam, int B, int H, int W, float min_disp, float max_depth,
                   float *depth, uint16_t *depth16, uint16_t *disp16, void *stream)
{
    LWS_CHECK_RC(check_geometry_args("depth_maps", disp, B, H, W, min_disp, max_depth));
    LWS_CHECK_ARG(depth || depth16 || disp16, "depth_maps: no output requested (depth, depth16 and disp16 are all null)");
    LWS_CHECK_ARG(cam || !(depth || depth16), "depth_maps: cam is null but depth or depth16 is requested");
    LWS_CHECK_ARG(aligned(cam, 4) && aligned(depth, 4) && aligned(depth16, 2) && aligned(disp16, 2),
                  "depth_maps: cam / depth must be 4-byte, depth16 / disp16 2-byte aligned");
    const int nq = (W + 3) / 4;
    const int64_t n = (int64_t)H * nq;
    hipLaunchKernelGGL(k_depth_maps, dim3((unsigned)((n + kThreads - 1) / kThreads), B), dim3(kThreads), 0, (hipStream_t)stream, disp,
                       mask, cam, H, W, nq, min_disp, max_depth, depth, depth16, disp16);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

int64_t lws_point_cloud_workspace(int B, int H)
{
    LWS_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1, "point_cloud_workspace: bad shape B=%d H=%d", B, H);
    return ((int64_t)B * H * (int64_t)sizeof(int) + 255) / 256 * 256;
}

int lws_point_cloud(const float *disp, const uint8_t *mask, const uint8_t *rgb, const float *cam, int B, int H, int W, float min_disp,
                    float max_depth, void *workspace, void *points, int64_t *counts, void *stream)
{
    LWS_CHECK_RC(check_geometry_args("point_cloud", disp, B, H, W, min_disp, max_depth));
    LWS_CHECK_ARG(cam && workspace && points && counts, "point_cloud: cam, workspace, points and counts must not be null");
    LWS_CHECK_ARG(aligned(cam, 4) && aligned(workspace, 4) && aligned(points, 16) && aligned(counts, 8),
                  "point_cloud: cam / workspace must be 4-byte, points 16-byte, counts 8-byte aligned");
    int *rows = static_cast<int *>(workspace);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_pc_count, dim3(H, B), dim3(kThreads), 0, st, disp, mask, cam, H, W, min_disp, max_depth, rows);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pc_scan, dim3(B), dim3(kThreads), 0, st, rows, H, counts);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pc_scatter, dim3(H, B), dim3(kThreads), 0, st, disp, mask, rgb, cam, H, W, min_disp, max_depth, rows,
                       static_cast<uint4 *>(points));
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // extern "C"
