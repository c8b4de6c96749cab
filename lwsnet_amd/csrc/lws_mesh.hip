// Surface normals and an indexed triangle mesh of a disparity map: what the pixel grid knows about neighbours and an unorganised
// cloud does not.  Arithmetic contract (include/lwsnet_hip.h, lws_surface_normals): one IEEE float32 operation per step (the build
// has no contraction and correctly rounded division and square root; no fmaf here), so tests/mesh_reference.py restates every
// output bit for bit in numpy.  Determinism: no atomics; vertices and faces are packed in raster order by a per-row count, a
// per-image scan and a per-row scatter whose ranks come from wave ballots, so an image gives the same bytes in any batch.
//   k_normals       one workgroup of 256 threads per 16 x 64 tile: P, d and valid of the tile and a one-pixel halo are computed once
//                   into LDS (three divisions per pixel, not per stencil member); the 3-byte normal-map pixels leave packed
//   k_mesh_count    one workgroup per row y: the vertices of row y and the faces of cell row y
//   k_mesh_scan     one workgroup per image and count array: the exclusive scans, the totals to counts[b]
//   k_mesh_scatter  one workgroup per row y: ranks the pixels of rows y and y + 1 and the faces of cell row y, writes row y's records
// 0 bytes of scratch.
#include "lws_geomkit.h"
#include "lws_packkit.h"

namespace lws {

namespace {

using namespace geomkit;
using namespace packkit;                // kThreads, kWaves
constexpr int kTW = 64;                 // tile width: one wave = 64 consecutive pixels of a row
constexpr int kTH = 16;                 // tile height: four rows per wave
constexpr int kPW = kTW + 2;            // the tile and its halo
constexpr int kPH = kTH + 2;

// "Connected" on effective disparities (NaN for an invalid pixel, so that the compare is false): the speckle filter's join rule.
__device__ __forceinline__ bool connected(float dp, float dq, float max_jump) { return fabsf(dp - dq) <= max_jump; }

// The byte of a normal-map channel: rintf is half to even; the conversion goes through int and keeps the low 8 bits (v lies in
// -1 .. 1 unless the squares under the root went subnormal).
__device__ __forceinline__ uint8_t normal_u8(float v) { return (uint8_t)(int)rintf((v * 0.5f + 0.5f) * 255.0f); }

// grid (tiles, B), 256 threads.
__global__ __launch_bounds__(kThreads) void k_normals(const float *__restrict__ disp, const uint8_t *__restrict__ mask,
                                                     const float *__restrict__ cam, int H, int W, int ntx, float min_disp,
                                                     float max_depth, float max_jump, float *__restrict__ normals,
                                                     uint8_t *__restrict__ normals8)
{
    __shared__ float s_x[kPH * kPW], s_y[kPH * kPW], s_z[kPH * kPW], s_d[kPH * kPW];
    __shared__ uint32_t s_px[kTH][kTW * 3 / 4 + 1];         // one packed row segment per tile row, shifted by the row's byte alignment
    const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int x0 = tx * kTW, y0 = ty * kTH;
    const Cam c = load_cam(cam, b);
    const int64_t plane = (int64_t)H * W;
    const float *dp = disp + b * plane;
    const uint8_t *mk = mask ? mask + b * plane : nullptr;
    const float nan = __builtin_nanf("");
    for (int i = t; i < kPH * kPW; i += kThreads) {
        const int r = i / kPW, q = i - r * kPW;
        const int y = y0 + r - 1, x = x0 + q - 1;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;                     // a pixel outside the image is invalid
        const int64_t pix = (int64_t)y * W + x;
        const float d = in ? dp[pix] : nan;
        const bool ok = in && (!mk || mk[pix] == 1);
        float z;
        const bool v = valid_z(d, ok, c.fb, min_disp, max_depth, z);
        s_x[i] = back_x(c, x, z);
        s_y[i] = back_y(c, y, z);
        s_z[i] = z;
        s_d[i] = v ? d : nan;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kTH / kWaves; ++k) {
        const int r = wave * (kTH / kWaves) + k, y = y0 + r, x = x0 + lane;
        const int i = (r + 1) * kPW + lane + 1;
        const float d = s_d[i];
        const float px = s_x[i], py = s_y[i], pz = s_z[i];
        // neighbours in the order R, D, L, U; quadrant j is the pair (nb[j], nb[j + 1]) rotated: (D,R), (R,U), (U,L), (L,D)
        const int off[4] = {1, kPW, -1, -kPW};
        bool con[4];
        float ex[4], ey[4], ez[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            con[j] = connected(d, s_d[i + off[j]], max_jump);
            ex[j] = s_x[i + off[j]] - px, ey[j] = s_y[i + off[j]] - py, ez[j] = s_z[i + off[j]] - pz;
        }
        const int qa[4] = {1, 0, 3, 2}, qb[4] = {0, 3, 2, 1};                   // (D,R), (R,U), (U,L), (L,D)
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int A = qa[j], Bq = qb[j];
            const float cx = ey[A] * ez[Bq] - ez[A] * ey[Bq];
            const float cy = ez[A] * ex[Bq] - ex[A] * ez[Bq];
            const float cz = ex[A] * ey[Bq] - ey[A] * ex[Bq];
            const bool present = con[A] && con[Bq];
            sx = present ? sx + cx : sx, sy = present ? sy + cy : sy, sz = present ? sz + cz : sz;
            any = any || present;
        }
        const float len = sqrtf((sx * sx + sy * sy) + sz * sz);
        const bool good = any && __builtin_isfinite(len) && len > 0.0f;
        const float nx = good ? sx / len : 0.0f, ny = good ? sy / len : 0.0f, nz = good ? sz / len : 0.0f;
        const bool in = y < H && x < W;
        if (normals && in) {
            float *o = normals + (int64_t)b * 3 * plane + (int64_t)y * W + x;  // a wave stores 64 consecutive floats of a plane's row
            o[0] = nx, o[plane] = ny, o[2 * plane] = nz;
        }
        if (normals8 && in) {
            const uint8_t *g = normals8 + (b * plane + (int64_t)y * W + x0) * 3;
            uint8_t *s = reinterpret_cast<uint8_t *>(s_px[r]) + ((uintptr_t)g & 3) + 3 * lane;
            s[0] = normal_u8(nx), s[1] = normal_u8(-ny), s[2] = normal_u8(-nz);
        }
    }
    if (!normals8) return;                                  // (uniform)
    __syncthreads();
    // A tile row's segment [x0, x0 + cnt) as bytes g[0 .. 3 cnt): up to 3 head bytes, aligned dwords, up to 3 tail bytes.  The bytes
    // sit in LDS at the offset g & 3, so that a global dword is an aligned LDS dword (as the rect rows of k_rectify_pair).
    const int cnt = min(kTW, W - x0);
#pragma unroll
    for (int k = 0; k < kTH / kWaves; ++k) {
        const int r = wave * (kTH / kWaves) + k, y = y0 + r;
        if (y >= H) break;                                  // (wave-uniform)
        uint8_t *g = normals8 + (b * plane + (int64_t)y * W + x0) * 3;
        const int shift = (int)((uintptr_t)g & 3);
        const uint8_t *s = reinterpret_cast<const uint8_t *>(s_px[r]);
        const int nbytes = 3 * cnt;
        const int head = min((4 - shift) & 3, nbytes);
        const int ndw = (nbytes - head) >> 2, tail = nbytes - head - 4 * ndw;
        if (lane < head) g[lane] = s[shift + lane];
        if (lane < ndw) *reinterpret_cast<uint32_t *>(g + head + 4 * lane) = s_px[r][((shift + head) >> 2) + lane];
        if (lane < tail) g[head + 4 * ndw + lane] = s[shift + head + 4 * ndw + lane];
    }
}

// The two rows of a workgroup of the mesh kernels: row y and row y + 1 (null pointers below the last row)
struct RowPair {
    const float *d0, *d1;
    const uint8_t *m0, *m1;
    bool vd0, vd1, vm0, vm1;
};

__device__ __forceinline__ RowPair row_pair(const float *__restrict__ disp, const uint8_t *__restrict__ mask, int b, int y, int H, int W)
{
    const int64_t row = ((int64_t)b * H + y) * W;
    RowPair r;
    r.d0 = disp + row, r.m0 = mask ? mask + row : nullptr;
    r.d1 = y + 1 < H ? r.d0 + W : nullptr, r.m1 = y + 1 < H && mask ? r.m0 + W : nullptr;
    r.vd0 = aligned(r.d0, 16), r.vd1 = aligned(r.d1, 16), r.vm0 = aligned(r.m0, 4), r.vm1 = aligned(r.m1, 4);
    return r;
}

// The effective disparities (NaN: invalid) of the 5 pixels 4q .. 4q+4 of a row -- the corners of the cells 4q .. 4q+3 -- their valid
// bits (bit i = pixel 4q + i) and the depths.  dp == NULL (the row below the image): all invalid.
__device__ __forceinline__ unsigned penta(const float *__restrict__ dp, const uint8_t *__restrict__ mk, bool vd, bool vm, int q, int W,
                                          const Cam &c, float min_disp, float max_depth, float de[5], float z[5])
{
    const float nan = __builtin_nanf("");
    if (!dp) {
#pragma unroll
        for (int i = 0; i < 5; ++i) de[i] = z[i] = nan;
        return 0u;
    }
    float d[5];
    bool ok[5];
    load_quad(dp, 4 * q, W, vd, d);
    load_ok(mk, 4 * q, W, vm, ok);
    const int x4 = 4 * q + 4;
    d[4] = x4 < W ? dp[x4] : nan;
    ok[4] = x4 < W && (!mk || mk[x4] == 1);
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const bool v = valid_z(d[i], ok[i], c.fb, min_disp, max_depth, z[i]);
        de[i] = v ? d[i] : nan;
        bits |= (v ? 1u : 0u) << i;
    }
    return bits;
}

// The face bits of the cells 4q .. 4q+3 of cell row y: bit 2i = T0, bit 2i + 1 = T1 of cell 4q + i; diag bit i = 1 where the cell's
// diagonal is a-e.  t = the row y, u = the row y + 1 (effective disparities).
__device__ __forceinline__ unsigned cell_faces(const float t[5], const float u[5], float max_jump, unsigned &diag)
{
    unsigned f = 0;
    diag = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a = t[i], b = t[i + 1], c = u[i], e = u[i + 1];
        const bool ab = connected(a, b, max_jump), ac = connected(a, c, max_jump), be = connected(b, e, max_jump),
                   ce = connected(c, e, max_jump);
        bool t0, t1;
        if (b == b && c == c) {                             // b and c valid: the diagonal is b-c
            const bool bc = connected(b, c, max_jump);
            t0 = bc && ab && ac, t1 = bc && be && ce;
        } else {                                            // else a-e (connected() is false unless both are valid)
            const bool ae = connected(a, e, max_jump);
            t0 = ae && ac && ce, t1 = ae && ab && be;
            diag |= 1u << i;
        }
        f |= (t0 ? 1u : 0u) << (2 * i) | (t1 ? 1u : 0u) << (2 * i + 1);
    }
    return f;
}

// grid (H, B), 256 threads: vertices of row y -> rows[0][b * H + y], faces of cell row y -> rows[1][b * H + y].
__global__ __launch_bounds__(kThreads) void k_mesh_count(const float *__restrict__ disp, const uint8_t *__restrict__ mask,
                                                        const float *__restrict__ cam, int H, int W, float min_disp, float max_depth,
                                                        float max_jump, int *__restrict__ vrow, int *__restrict__ frow)
{
    __shared__ int s_n[kWaves][2];
    const int y = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const RowPair r = row_pair(disp, mask, b, y, H, W);
    const Cam c = load_cam(cam, b);
    const int nq = (W + 3) >> 2;
    int n[2] = {0, 0};
    for (int q = t; q < nq; q += kThreads) {
        float d0[5], d1[5], z[5];
        unsigned diag;
        n[0] += __builtin_popcount(penta(r.d0, r.m0, r.vd0, r.vm0, q, W, c, min_disp, max_depth, d0, z) & 15u);
        penta(r.d1, r.m1, r.vd1, r.vm1, q, W, c, min_disp, max_depth, d1, z);
        n[1] += __builtin_popcount(cell_faces(d0, d1, max_jump, diag));
    }
    block_sum_n(n, s_n);
    if (t < 2) (t ? frow : vrow)[(int64_t)b * H + y] = block_total(s_n, t);
}

// grid (B, 2), 256 threads: the row counts of image b (blockIdx.y: 0 = vertices, 1 = faces) -> their exclusive scan, in place
// (packkit::row_scan); counts[b][blockIdx.y] = the total.
__global__ __launch_bounds__(kThreads) void k_mesh_scan(int *__restrict__ vrow, int *__restrict__ frow, int H, int64_t *__restrict__ counts)
{
    __shared__ int s_w[kWaves];
    const int b = blockIdx.x, which = blockIdx.y;
    const int total = row_scan((which ? frow : vrow) + (int64_t)b * H, H, s_w);
    if (threadIdx.x == 0) counts[2 * (int64_t)b + which] = total;
}

struct MeshOut {
    uint4 *points;
    float4 *vnormals;
    int32_t *faces, *index;
};

// grid (H, B), 256 threads: row y's vertices (points, vnormals, index) and cell row y's faces.  A chunk is 256 quads; in it the
// vertex index of pixel i of quad q of row y is voff[y] + the valid pixels of the row's earlier quads + those of q before i, the
// same for row y + 1 with voff[y + 1], and the pixel 4q + 4 continues the count; a face's slot is foff[y] + the faces of the earlier
// quads' cells + those of q's before it.  So no index map is read back, and nothing is atomic.
__global__ __launch_bounds__(kThreads) void k_mesh_scatter(const float *__restrict__ disp, const uint8_t *__restrict__ mask,
                                                          const uint8_t *__restrict__ rgb, const float *__restrict__ cam,
                                                          const float *__restrict__ normals, int H, int W, float min_disp,
                                                          float max_depth, float max_jump, const int *__restrict__ vrow,
                                                          const int *__restrict__ frow, const MeshOut o)
{
    __shared__ int s_w[3][kWaves];
    const int y = blockIdx.x, b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const RowPair r = row_pair(disp, mask, b, y, H, W);
    const int64_t plane = (int64_t)H * W, row = ((int64_t)b * H + y) * W;
    const uint8_t *cp = rgb ? rgb + 3 * row : nullptr;
    const bool vc = aligned(cp, 4);
    const float *np = normals ? normals + (int64_t)b * 3 * plane + (int64_t)y * W : nullptr;
    const bool vn = aligned(np, 16) && (plane & 3) == 0;
    int32_t *ix = o.index ? o.index + row : nullptr;
    const Cam c = load_cam(cam, b);
    const int64_t brow = (int64_t)b * H + y;
    const int voff0 = vrow[brow], voff1 = y + 1 < H ? vrow[brow + 1] : 0;
    uint4 *pts = o.points + b * plane;
    float4 *vnr = o.vnormals ? o.vnormals + b * plane : nullptr;
    int32_t *fc = o.faces + ((int64_t)b * 2 * (H - 1) * (W - 1) + frow[brow]) * 3;
    const int nq = (W + 3) >> 2;
    int carry[3] = {voff0, voff1, 0};                       // uniform: the index of the chunk's first vertex of each row, its first face
    for (int q0 = 0; q0 < nq; q0 += kThreads) {
        const int q = q0 + t;
        float d0[5], d1[5], z[5], z1[5];
        unsigned bits0 = 0, bits1 = 0, fbits = 0, diag = 0;
        if (q < nq) {
            bits0 = penta(r.d0, r.m0, r.vd0, r.vm0, q, W, c, min_disp, max_depth, d0, z);
            bits1 = penta(r.d1, r.m1, r.vd1, r.vm1, q, W, c, min_disp, max_depth, d1, z1);
            fbits = cell_faces(d0, d1, max_jump, diag);
        }
        int wn[3], rank[3];
        rank[0] = wave_rank<4>(bits0, wn[0]);
        rank[1] = wave_rank<4>(bits1, wn[1]);
        rank[2] = wave_rank<8>(fbits, wn[2]);
        if (lane == 0) s_w[0][wave] = wn[0], s_w[1][wave] = wn[1], s_w[2][wave] = wn[2];
        __syncthreads();                                    // (one barrier for the three ranks)
#pragma unroll
        for (int k = 0; k < 3; ++k) rank[k] = add_earlier_waves(rank[k], s_w[k], carry[k]);
        const int x = 4 * q;
        if (q < nq && ix) {
            int v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (bits0 >> i) & 1u ? rank[0] + __builtin_popcount(bits0 & ((1u << i) - 1u)) : -1;
            if (x + 4 <= W && aligned(ix + x, 16)) {
                *reinterpret_cast<int4 *>(ix + x) = make_int4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (x + i < W) ix[x + i] = v[i];
            }
        }
        if (bits0 & 15u) {
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
            float n3[3][4];
            if (np) {
#pragma unroll
                for (int k = 0; k < 3; ++k) load_quad(np + k * plane, x, W, vn, n3[k]);
            }
            int at = rank[0];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!((bits0 >> i) & 1u)) continue;
                const float X = back_x(c, x + i, z[i]), Y = back_y(c, y, z[i]);
                const unsigned col = (unsigned)px[3 * i] | ((unsigned)px[3 * i + 1] << 8) | ((unsigned)px[3 * i + 2] << 16) | (255u << 24);
                pts[at] = make_uint4(__float_as_uint(X), __float_as_uint(Y), __float_as_uint(z[i]), col);
                if (np) vnr[at] = make_float4(n3[0][i], n3[1][i], n3[2][i], 0.0f);
                ++at;
            }
        }
        if (fbits) {
            int32_t *f = fc + 3 * (int64_t)rank[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int a = rank[0] + __builtin_popcount(bits0 & ((1u << i) - 1u)), bb = rank[0] + __builtin_popcount(bits0 & ((2u << i) - 1u));
                const int cc = rank[1] + __builtin_popcount(bits1 & ((1u << i) - 1u)), e = rank[1] + __builtin_popcount(bits1 & ((2u << i) - 1u));
                const bool ae = (diag >> i) & 1u;
                if ((fbits >> (2 * i)) & 1u) {              // T0 = (a, c, b), or (a, c, e) on the a-e diagonal
                    f[0] = a, f[1] = cc, f[2] = ae ? e : bb;
                    f += 3;
                }
                if ((fbits >> (2 * i + 1)) & 1u) {          // T1 = (b, c, e), or (a, e, b)
                    f[0] = ae ? a : bb, f[1] = ae ? e : cc, f[2] = ae ? bb : e;
                    f += 3;
                }
            }
        }
        __syncthreads();                                    // s_w is rewritten by the next chunk
    }
}

int check_mesh_args(const char *who, const float *disp, const float *cam, int B, int H, int W, float min_disp, float max_depth,
                    float max_jump)
{
    LWS_CHECK_RC(check_image_shape(who, B, H, W, 30));      // a face count, 2 (H-1) (W-1), fits an int32
    LWS_CHECK_RC(check_geometry_args(who, disp, B, H, W, min_disp, max_depth));
    LWS_CHECK_ARG(finite_nonneg(max_jump), "%s: max_jump must be finite and >= 0, got %g", who, (double)max_jump);
    LWS_CHECK_ARG(cam, "%s: cam is null", who);
    LWS_CHECK_ARG(aligned(cam, 4), "%s: cam is not 4-byte aligned", who);
    return LWS_OK;
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int lws_surface_normals(const float *disp, const uint8_t *mask, const float *cam, int B, int H, int W, float min_disp, float max_depth,
                        float max_jump, float *normals, uint8_t *normals8, void *stream)
{
    LWS_CHECK_RC(check_mesh_args("surface_normals", disp, cam, B, H, W, min_disp, max_depth, max_jump));
    LWS_CHECK_ARG(normals || normals8, "surface_normals: no output requested (normals and normals8 are both null)");
    LWS_CHECK_ARG(aligned(normals, 4), "surface_normals: normals is not 4-byte aligned");
    const int64_t px = (int64_t)B * H * W;
    const Buf bufs[] = {{normals, 12 * px, "normals"}, {normals8, 3 * px, "normals8"}, {disp, 4 * px, "disp"}, {mask, px, "mask"},
                        {cam, 20 * (int64_t)B, "cam"}};
    LWS_CHECK_RC(check_no_overlap("surface_normals", bufs, 5, 2));
    const int ntx = (W + kTW - 1) / kTW, nty = (H + kTH - 1) / kTH;
    hipLaunchKernelGGL(k_normals, dim3((unsigned)((int64_t)ntx * nty), B), dim3(kThreads), 0, (hipStream_t)stream, disp, mask, cam, H, W,
                       ntx, min_disp, max_depth, max_jump, normals, normals8);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

int64_t lws_surface_mesh_workspace(int B, int H)
{
    LWS_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1, "surface_mesh_workspace: bad shape B=%d H=%d", B, H);
    return 2 * round256((int64_t)B * H * (int64_t)sizeof(int));
}

int lws_surface_mesh(const float *disp, const uint8_t *mask, const uint8_t *rgb, const float *cam, const float *normals, int B, int H,
                     int W, float min_disp, float max_depth, float max_jump, void *workspace, void *points, void *vnormals,
                     int32_t *faces, int32_t *index, int64_t *counts, void *stream)
{
    LWS_CHECK_RC(check_mesh_args("surface_mesh", disp, cam, B, H, W, min_disp, max_depth, max_jump));
    LWS_CHECK_ARG(workspace && points && faces && counts, "surface_mesh: workspace, points, faces and counts must not be null");
    LWS_CHECK_ARG((normals != nullptr) == (vnormals != nullptr),
                  "surface_mesh: normals and vnormals go together (%s is null)", normals ? "vnormals" : "normals");
    LWS_CHECK_ARG(aligned(workspace, 4) && aligned(normals, 4) && aligned(faces, 4) && aligned(index, 4),
                  "surface_mesh: workspace / normals / faces / index must be 4-byte aligned");
    LWS_CHECK_ARG(aligned(points, 16) && aligned(vnormals, 16) && aligned(counts, 8),
                  "surface_mesh: points / vnormals must be 16-byte, counts 8-byte aligned");
    const int64_t px = (int64_t)B * H * W, rows_bytes = round256((int64_t)B * H * (int64_t)sizeof(int));
    const int64_t nfaces = (int64_t)B * 2 * (H - 1) * (W - 1);
    const Buf bufs[] = {{workspace, 2 * rows_bytes, "workspace"}, {points, 16 * px, "points"}, {vnormals, 16 * px, "vnormals"},
                        {faces, 12 * (nfaces > 0 ? nfaces : 1), "faces"}, {index, 4 * px, "index"}, {counts, 16 * (int64_t)B, "counts"},
                        {disp, 4 * px, "disp"}, {mask, px, "mask"}, {rgb, 3 * px, "rgb"}, {cam, 20 * (int64_t)B, "cam"},
                        {normals, 12 * px, "normals"}};
    LWS_CHECK_RC(check_no_overlap("surface_mesh", bufs, 11, 6));
    int *vrow = static_cast<int *>(workspace);
    int *frow = reinterpret_cast<int *>(static_cast<char *>(workspace) + rows_bytes);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mesh_count, dim3(H, B), dim3(kThreads), 0, st, disp, mask, cam, H, W, min_disp, max_depth, max_jump, vrow, frow);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mesh_scan, dim3(B, 2), dim3(kThreads), 0, st, vrow, frow, H, counts);
    LWS_LAUNCH_CHECK();
    const MeshOut o{static_cast<uint4 *>(points), static_cast<float4 *>(vnormals), faces, index};
    hipLaunchKernelGGL(k_mesh_scatter, dim3(H, B), dim3(kThreads), 0, st, disp, mask, rgb, cam, normals, H, W, min_disp, max_depth,
                       max_jump, vrow, frow, o);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // extern "C"
