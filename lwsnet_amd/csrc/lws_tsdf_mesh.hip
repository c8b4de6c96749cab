// Marching cubes on a TSDF volume: an indexed triangle mesh whose vertex list is the record list of lws_tsdf_points.  Contract and
// the rule of the case table: include/lwsnet_tsdf_mesh.h; the table's numbers: lws_tsdf_mesh_table.h, printed by
// tools/make_tsdf_mesh_table.py; tests/tsdf_mesh_reference.py restates every output bit for bit in numpy.
//
// Launches (a fixed list: it depends on the arguments, never on the data; nothing is read back):
//   tsdfkit::launch_points   k_ts_count, k_ts_scan, k_ts_scatter of lws_tsdf.hip: the vertices, their row offsets left in the workspace
//   k_tm_count               one workgroup per row of cubes (iy, iz): the triangles of its cubes -> cube_rows[iz * (Gy - 1) + iy]
//   k_tm_scan                cube_rows -> its exclusive scan, counts[1] = the total
//   k_tm_scatter             one workgroup per row of cubes.  A chunk is 256 voxels of the four x-rows (iy + dy, iz + dz) and the 255
//                            cubes between them: four packkit::block_rank<3> passes give every voxel the rank of its first crossing
//                            in its row, kept in LDS with the voxel's edge bits, sign and validity, so that a cube reads its +x
//                            corners from the next thread's slots.  The last voxel of a chunk is the first of the next: it is ranked
//                            with no bits of its own, so the carry counts it once.  The triangles are ranked by packkit::block_scan
//                            of the per-cube count and stored as three int32.  The case table sits in LDS, 16 bytes a row: threads
//                            of a wave index it with different cases.
// Determinism: a face belongs to one thread; what crosses threads are ballots and integer scans.  0 bytes of scratch.
#include <string.h>

#include "lws_tsdfkit.h"
#include "lwsnet_tsdf_mesh.h"

namespace lws {

namespace {

using namespace tsdfkit;
using namespace packkit;                                    // kThreads, kWaves, block_rank, block_scan, row_scan

constexpr int kRowBytes = 32;                               // a row of the table as exported
constexpr int kRowLds = 16;                                 // ... and as the kernels keep it: n and up to five triangles
static_assert(1 + 3 * LWS_TSDF_MESH_MAX_TRIS <= kRowLds, "a row of the case table does not fit its LDS slot");

const uint8_t h_table[256][kRowBytes] = {
#include "lws_tsdf_mesh_table.h"
};
__device__ const uint8_t d_table[256][kRowBytes] __attribute__((aligned(16))) = {
#include "lws_tsdf_mesh_table.h"
};

// voxel (ix, iy, iz) as a cube's corner: bit 0 = T > 0, bit 1 = observed and T is not NaN
__device__ __forceinline__ unsigned corner_bits(const Vol &v, int ix, int iy, int iz)
{
    const int i = (iz * v.Gy + iy) * v.Gx + ix;
    if (!observed(v.Wt[i], v.w_min)) return 0u;
    const float t = v.T[i];
    return (t > 0.0f ? 1u : 0u) | (t == t ? 2u : 0u);
}

// grid (Gy - 1, Gz - 1), 256 threads: the triangles of each row of cubes -> cube_rows[iz * (Gy - 1) + iy]
__global__ __launch_bounds__(kThreads) void k_tm_count(Vol v, int64_t *__restrict__ cube_rows)
{
    __shared__ int s_n[kWaves];
    __shared__ uint8_t s_tris[256];
    const int iy = blockIdx.x, iz = blockIdx.y, t = threadIdx.x;
    s_tris[t] = d_table[t][0];
    __syncthreads();
    int n = 0;
    for (int ix = t; ix + 1 < v.Gx; ix += kThreads) {
        unsigned c = 0u, valid = 2u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned b = corner_bits(v, ix + (k & 1), iy + ((k >> 1) & 1), iz + (k >> 2));
            c |= (b & 1u) << k;
            valid &= b;
        }
        n += valid ? s_tris[c] : 0;
    }
    n = block_sum(n, s_n);
    if (t == 0) cube_rows[(int64_t)iz * (v.Gy - 1) + iy] = n;
}

// grid (1), 256 threads: cube_rows[0 .. R) -> its exclusive scan, in place; counts[1] = the total
__global__ __launch_bounds__(kThreads) void k_tm_scan(int64_t *__restrict__ r, int R, int64_t *__restrict__ counts)
{
    __shared__ int64_t s_w[kWaves];
    const int64_t total = row_scan(r, R, s_w);
    if (threadIdx.x == 0) counts[1] = total;
}

// grid (Gy - 1, Gz - 1), 256 threads: the triangles of the row of cubes (iy, iz) to faces[cube_off[iz * (Gy - 1) + iy] ..] in the
// order (ix, the table's).  row_off: the scanned x-row counts k_ts_scan left; counts[0]: the vertices it found.
__global__ __launch_bounds__(kThreads) void k_tm_scatter(Vol v, const int64_t *__restrict__ row_off, const int64_t *__restrict__ cube_off,
                                                        const int64_t *__restrict__ counts, int64_t max_points, int64_t max_faces,
                                                        int *__restrict__ faces)
{
    __shared__ uint4 s_table[256];                          // 16 bytes a case
    __shared__ int s_w[4][kWaves], s_wf[kWaves];
    __shared__ int s_rank[4][kThreads];                     // the vertex index of the voxel's first crossing (< 2^31: the vertices fit)
    __shared__ uint8_t s_info[4][kThreads];                 // bits 0..2 the edge bits, bit 3 T > 0, bit 4 a valid corner
    const int iy = blockIdx.x, iz = blockIdx.y, t = threadIdx.x;
    if (counts[0] > max_points) return;                     // (uniform) the vertices do not fit: no mesh
    const int64_t first = cube_off[(int64_t)iz * (v.Gy - 1) + iy];
    if (first >= max_faces) return;                         // (uniform) nothing of this row fits
    s_table[t] = *reinterpret_cast<const uint4 *>(d_table[t]);
    const uint8_t *table = reinterpret_cast<const uint8_t *>(s_table);
    int64_t base[4];                                        // the first record of each of the four x-rows
#pragma unroll
    for (int r = 0; r < 4; ++r) base[r] = row_off[(int64_t)(iz + (r >> 1)) * v.Gy + iy + (r & 1)];
    int carry[4] = {0, 0, 0, 0}, fcarry = 0;                // uniform: the crossings and the triangles of the earlier chunks
    for (int x0 = 0; x0 + 1 < v.Gx; x0 += kThreads - 1) {
        const int ix = x0 + t;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float Ta = 0.0f, Tb[3];
            unsigned bits = 0u, corner = 0u;
            if (ix < v.Gx) {
                bits = edge_bits(v, ix, iy + (r & 1), iz + (r >> 1), Ta, Tb);
                corner = corner_bits(v, ix, iy + (r & 1), iz + (r >> 1));
            }
            s_rank[r][t] = (int)(base[r] + block_rank<3>(t == kThreads - 1 ? 0u : bits, s_w[r], carry[r]));
            s_info[r][t] = (uint8_t)(bits | (corner << 3));
        }
        __syncthreads();
        unsigned c = 0u, valid = 0u;
        if (t < kThreads - 1 && ix + 1 < v.Gx) {
            valid = 16u;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned info = s_info[k >> 1][t + (k & 1)];
                c |= ((info >> 3) & 1u) << k;
                valid &= info;
            }
        }
        const uint8_t *row = table + kRowLds * c;
        const int n = valid ? row[0] : 0;
        const int64_t rank = first + block_scan<int>(n, s_wf, fcarry);
        for (int k = 0; k < n; ++k) {
            if (rank + k >= max_faces) break;
            int idx[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int id = row[1 + 3 * k + m], e = id >> 2, j = id & 3;
                const int dx = e == 0 ? 0 : j & 1, r = e == 0 ? j : e == 1 ? j & 2 : j >> 1;      // the owner: r = dy + 2 * dz
                const unsigned own = s_info[r][t + dx];
                idx[m] = s_rank[r][t + dx] + __builtin_popcount(own & ((1u << e) - 1u));
            }
            int *f = faces + 3 * (rank + k);
            f[0] = idx[0], f[1] = idx[1], f[2] = idx[2];
        }
        __syncthreads();                                    // the slots are rewritten by the next chunk
    }
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int64_t lws_tsdf_mesh_workspace(int Gy, int Gz)
{
    LWS_CHECK_ARG(Gy >= 2 && Gy <= kMaxGrid && Gz >= 2 && Gz <= kMaxGrid, "tsdf_mesh_workspace: bad volume Gy=%d Gz=%d (each in 2..%d)", Gy, Gz,
                  kMaxGrid);
    const int64_t rows = ((int64_t)Gy * Gz * (int64_t)sizeof(int64_t) + 255) / 256 * 256;
    return rows + ((int64_t)(Gy - 1) * (Gz - 1) * (int64_t)sizeof(int64_t) + 255) / 256 * 256;
}

int lws_tsdf_mesh(const float *T, const float *Wt, const uint8_t *C, int Gx, int Gy, int Gz, float ox, float oy, float oz, float vs,
                  float w_min, int64_t max_points, int64_t max_faces, void *workspace, void *points, float *vnormals, int32_t *faces,
                  int64_t *counts, void *stream)
{
    const char *who = "tsdf_mesh";
    LWS_CHECK_RC(check_volume(who, T, Wt, Gx, Gy, Gz, ox, oy, oz, vs));
    LWS_CHECK_ARG(workspace && points && faces && counts, "%s: workspace, points, faces and counts must not be null", who);
    LWS_CHECK_ARG(finite_nonneg(w_min), "%s: w_min must be finite and >= 0, got %g", who, (double)w_min);
    LWS_CHECK_ARG(max_points >= 1 && max_points < ((int64_t)1 << 31), "%s: max_points %lld outside 1 .. 2^31 - 1", who, (long long)max_points);
    LWS_CHECK_ARG(max_faces >= 1 && max_faces < ((int64_t)1 << 31), "%s: max_faces %lld outside 1 .. 2^31 - 1", who, (long long)max_faces);
    LWS_CHECK_ARG(aligned(C, 4) && aligned(faces, 4) && aligned(workspace, 8) && aligned(points, 16) && aligned(vnormals, 16) && aligned(counts, 8),
                  "%s: C / faces must be 4-byte, workspace / counts 8-byte, points / vnormals 16-byte aligned", who);
    const int64_t vox = (int64_t)Gx * Gy * Gz;
    const Buf bufs[] = {{workspace, lws_tsdf_mesh_workspace(Gy, Gz), "workspace"}, {points, 16 * max_points, "points"},
                        {vnormals, 16 * max_points, "vnormals"}, {faces, 12 * max_faces, "faces"}, {counts, 16, "counts"}, {T, 4 * vox, "T"},
                        {Wt, 4 * vox, "Wt"}, {C, 4 * vox, "C"}};
    LWS_CHECK_RC(check_no_overlap(who, bufs, 8, 5));

    const Vol v = {T, Wt, Gx, Gy, Gz, ox, oy, oz, vs, w_min};
    int64_t *rows = static_cast<int64_t *>(workspace);
    int64_t *cube_rows = rows + ((int64_t)Gy * Gz + 31) / 32 * 32;           // behind the x-row part, rounded up to 256 bytes
    hipStream_t st = (hipStream_t)stream;
    LWS_CHECK_RC(launch_points(v, C, max_points, rows, points, vnormals, counts, st));
    const dim3 grid(Gy - 1, Gz - 1);
    hipLaunchKernelGGL(k_tm_count, grid, dim3(kThreads), 0, st, v, cube_rows);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tm_scan, dim3(1), dim3(kThreads), 0, st, cube_rows, (Gy - 1) * (Gz - 1), counts);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tm_scatter, grid, dim3(kThreads), 0, st, v, rows, cube_rows, counts, max_points, max_faces, faces);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

int lws_tsdf_mesh_table(uint8_t *table)
{
    LWS_CHECK_ARG(table, "tsdf_mesh_table: table is null");
    memcpy(table, h_table, sizeof(h_table));
    return LWS_OK;
}

}  // extern "C"
