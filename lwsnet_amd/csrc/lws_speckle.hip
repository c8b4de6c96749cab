// Speckle filter of a disparity map: connected components (4-neighbours joined iff |dp - dq| <= max_diff, float32) by union-find,
// components of at most max_size pixels dropped (code 3) and optionally background-filled.  Contract: include/lwsnet_hip.h,
// lws_speckle_filter; tests/speckle_reference.py restates every output bit for bit.
//
// Launches (a fixed list: it depends on the arguments `fill` and `counts`, never on the data; nothing is read back):
//   k_sp_tile     one workgroup per 32 x 64 tile: union-find of the tile in LDS; parent[p] = the raster index of p's tile-local root
//                 (-1: invalid pixel), size[p] = the pixels of the tile-local component at its root, 0 elsewhere
//   k_sp_border   one thread per pair of pixels across a tile edge: unions of the tile-local roots, agent-scope atomics
//   k_sp_flatten  every tile-local root finds its global root, points at it and adds its size to the global root's
//   k_sp_apply    one workgroup per row: codes, out (with the row fill of lws_rowkit.h), labels, per-row counts
//   k_sp_counts   (counts != NULL) one workgroup per image: the per-row counts summed in a fixed order
//
// lws_cclkit.h holds the steps this labeller shares with lws_objects.hip and lws_movers.hip -- the union-find, the tile geometry,
// the tile-edge pairs, the flatten -- and the invariant (parent[p] <= p in raster order), termination and memory-scope arguments
// they rest on.  The words shared inside a launch here: parent[] in k_sp_border and k_sp_flatten, size[] in k_sp_flatten.  Only
// ROOTS are ever re-parented, so a non-root pixel keeps the parent k_sp_tile gave it, and after k_sp_flatten every pixel is two
// plain loads from its label: parent[parent[p]].
// Sizes: counted per tile in LDS (one add per wave for the wave's leading root, an LDS add for the other lanes), then ONE integer
// atomic add per tile-local component to its global root: a 450 k-pixel component costs a few hundred adds on its word, not 450 k.
// Integer atomics only, so the result does not depend on their order.  0 bytes of scratch.
#include "lws_cclkit.h"
#include "lws_common.h"
#include "lws_rowkit.h"

namespace lws {

namespace {

using namespace rowkit;                                     // kThreads, kWaves, kMaxW and the pieces of k_sp_apply
using namespace opkit;
using namespace cclkit;                                    // the tile, the union-find, the tile edges, the flatten
constexpr int kQuadsPerThread = kTile / 4 / kThreads;       // 2

__device__ __forceinline__ bool sp_valid(float d, bool ok) { return ok && __builtin_isfinite(d) && d > 0.0f; }

__device__ __forceinline__ void store_quad_i(int *__restrict__ p, int x, int W, const int v[4])
{
    if (x + 4 <= W && aligned(p + x, 16)) {
        *reinterpret_cast<int4 *>(p + x) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i < W) p[x + i] = v[i];
    }
}

// grid (ntx * nty, B), 256 threads: tile (tx, ty) of image b.  Thread t owns the quads t and t + 256 of the tile's 32 rows x 16
// quads (a wave: 4 rows), read with one float4 / uchar4 each where the address allows.  LDS 24 KiB: s_d (the value, NaN where the
// pixel is invalid or outside the image), s_par, s_cnt.
__global__ __launch_bounds__(kThreads) void k_sp_tile(const float *__restrict__ disp, const uint8_t *__restrict__ mask, int H, int W,
                                                     int ntx, float max_diff, int *__restrict__ parent, int *__restrict__ size)
{
    __shared__ __attribute__((aligned(16))) float s_d[kTile];
    __shared__ __attribute__((aligned(16))) int s_par[kTile];
    __shared__ __attribute__((aligned(16))) int s_cnt[kTile];
    const int t = threadIdx.x, lane = t & 63, b = blockIdx.y;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * kTileRows, x0 = tx * kTileCols;
    const int64_t img = (int64_t)b * H * W;
    const float nan = __builtin_nanf("");

    for (int k = 0; k < kQuadsPerThread; ++k) {
        const int q = t + k * kThreads, ry = q / (kTileCols / 4), rx = 4 * (q % (kTileCols / 4));
        const int y = y0 + ry, x = x0 + rx;
        float d[4] = {nan, nan, nan, nan};
        if (y < H && x < W) {
            const float *dp = disp + img + (int64_t)y * W;
            const uint8_t *mk = mask ? mask + img + (int64_t)y * W : nullptr;
            bool ok[4] = {true, true, true, true};
            if (x + 4 <= W && aligned(dp + x, 16)) {
                const float4 v = *reinterpret_cast<const float4 *>(dp + x);
                d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) d[i] = x + i < W ? dp[x + i] : nan;
            }
            if (mk) {
                if (x + 4 <= W && aligned(mk + x, 4)) {
                    const uchar4 v = *reinterpret_cast<const uchar4 *>(mk + x);
                    ok[0] = v.x == 1, ok[1] = v.y == 1, ok[2] = v.z == 1, ok[3] = v.w == 1;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) ok[i] = x + i < W && mk[x + i] == 1;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) d[i] = sp_valid(d[i], ok[i]) ? d[i] : nan;
        }
        const int l = ry * kTileCols + rx;
        *reinterpret_cast<float4 *>(s_d + l) = make_float4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<int4 *>(s_par + l) = make_int4(l, l + 1, l + 2, l + 3);
        *reinterpret_cast<int4 *>(s_cnt + l) = make_int4(0, 0, 0, 0);
    }
    __syncthreads();

    // the joins to the right and below, inside the tile
    for (int k = 0; k < kQuadsPerThread; ++k) {
        const int q = t + k * kThreads, ry = q / (kTileCols / 4), rx = 4 * (q % (kTileCols / 4));
#pragma unroll
        for (int i = 0; i < 4; ++i) join_right_below(s_d, s_par, ry * kTileCols + rx + i, rx + i + 1 < kTileCols, ry + 1 < kTileRows, max_diff);
    }
    __syncthreads();

    // roots (s_par is read-only from here), then the sizes: the lanes of a wave that share the root of its first valid lane add
    // once, the others one by one -- a tile inside one plateau costs 32 LDS adds, not 2048 on one word
    int root[kQuadsPerThread][4];
    for (int k = 0; k < kQuadsPerThread; ++k) {
        const int q = t + k * kThreads, l0 = (q / (kTileCols / 4)) * kTileCols + 4 * (q % (kTileCols / 4));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int l = l0 + i;
            const int r = __builtin_isnan(s_d[l]) ? -1 : lds_find(s_par, l);
            root[k][i] = r;
            const unsigned long long any = __ballot(r >= 0);
            if (any == 0) continue;                         // wave-uniform
            const int r0 = __shfl(r, __ffsll((long long)any) - 1, 64);
            const unsigned long long same = __ballot(r == r0);
            if (r == r0) {
                if (lane == __ffsll((long long)same) - 1) atomicAdd(&s_cnt[r0], __popcll(same));
            } else if (r >= 0) {
                atomicAdd(&s_cnt[r], 1);
            }
        }
    }
    __syncthreads();

    for (int k = 0; k < kQuadsPerThread; ++k) {
        const int q = t + k * kThreads, ry = q / (kTileCols / 4), rx = 4 * (q % (kTileCols / 4));
        const int y = y0 + ry, x = x0 + rx;
        if (y >= H || x >= W) continue;
        int pv[4], sv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = root[k][i], l = ry * kTileCols + rx + i;
            pv[i] = r < 0 ? -1 : tile_to_index(r, y0, x0, W);
            sv[i] = r == l ? s_cnt[l] : 0;
        }
        const int64_t row = img + (int64_t)y * W;
        store_quad_i(parent + row, x, W, pv);
        store_quad_i(size + row, x, W, sv);
    }
}

// grid (ceil(n / 256), B), n = (nty - 1) * W + (ntx - 1) * H: one thread per pair of pixels across a tile edge (lws_cclkit.h)
__global__ __launch_bounds__(kThreads) void k_sp_border(const float *__restrict__ disp, int H, int W, int nty, int ntx, float max_diff,
                                                       int *__restrict__ parent)
{
    unite_tile_edges(disp, H, W, nty, ntx, max_diff, parent);
}

// grid (ceil(H * W / 256), B): one thread per pixel; the tile-local roots (size > 0) find their global root r, point at it and
// hand it their size.  parent[] and size[] are shared between workgroups here: agent-scope atomics only.  size[p] is read for
// its sign alone, which the additions to a global root's word cannot change.
__global__ __launch_bounds__(kThreads) void k_sp_flatten(int HW, int *__restrict__ parent, int *__restrict__ size)
{
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= HW) return;
    const int p = (int)g;
    int *par = parent + (int64_t)blockIdx.y * HW, *sz = size + (int64_t)blockIdx.y * HW;
    const int n = ld_agent(sz + p);
    if (n <= 0) return;
    const int r = point_at_root(par, p);
    if (r != p) a_add(sz + r, n);
}

// grid (H, B), 256 threads: one workgroup per row, thread t owns the quads t, t + 256, ... of it (lws_rowkit.h).  parent[] and
// size[] were written by earlier launches: plain loads.  out may be disp and mask_out may be mask (no __restrict__ on them): a
// thread reads its quad before it writes it, and the fill stages the row before any of it is written.  LDS (dynamic, fill only):
// row[4 nq] floats, last[nq], first[nq] ints.
__global__ __launch_bounds__(kThreads) void k_sp_apply(const float *disp, const uint8_t *mask, int H, int W, int max_size, int fill,
                                                      const int *__restrict__ parent, const int *__restrict__ size, float *out,
                                                      uint8_t *mask_out, int32_t *__restrict__ labels, int *__restrict__ row_cnt)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_wl[kWaves], s_wf[kWaves], s_n[kWaves * 3];
    const int y = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int nq = (W + 3) >> 2;
    float *s_row = lds;
    int *s_last = reinterpret_cast<int *>(lds + 4 * nq), *s_first = s_last + nq;
    const int64_t img = (int64_t)b * H * W, row = img + (int64_t)y * W;
    const float *dp = disp + row;
    const uint8_t *mk = mask ? mask + row : nullptr;
    const int *par = parent + img, *sz = size + img;
    float *op = out + row;
    uint8_t *mo = mask_out + row;
    const bool vd = aligned(dp, 16), vout = aligned(op, 16), vmk = aligned(mk, 4), vmo = aligned(mo, 4);

    KeptFlags kept;
    int n_valid = 0, n_removed = 0;
    for (int k = 0, q = t; q < nq; ++k, q += kThreads) {
        const int x = 4 * q;
        float d[4];
        int m[4] = {0, 0, 0, 0};
        load_quad(dp, x, W, vd, 0.0f, d);
        if (mk) {
            if (vmk && x + 4 <= W) {
                const uchar4 v = *reinterpret_cast<const uchar4 *>(mk + x);
                m[0] = v.x, m[1] = v.y, m[2] = v.z, m[3] = v.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) m[i] = x + i < W ? mk[x + i] : 0;
            }
        }
        int c[4], lab[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = y * W + x + i;
            const int l = x + i < W ? par[p] : -1;          // the tile-local root, or -1
            if (l < 0) {
                c[i] = m[i] != 1 ? m[i] : 0;                // (m = 0 without a mask and beyond the row)
                lab[i] = -1;
            } else {
                const int r = par[l];                       // the global root: the first pixel of the component
                const bool speckle = sz[r] <= max_size;
                c[i] = speckle ? 3 : 1;
                lab[i] = r;
                n_valid += 1;
                n_removed += speckle && r == p ? 1 : 0;
            }
        }
        bool ok[4];
        kept.add(k, c, ok);
        store_codes(mo, x, W, vmo, c);
        if (labels) store_quad_i(labels + row, x, W, lab);
        if (fill) {
            quad_last_first(ok, x, s_last[q], s_first[q]);
        } else {
            store_kept(op, x, W, vout, c, d);
        }
    }
    if (row_cnt) wave_sums<3>({n_valid, kept.count, n_removed}, s_n);
    if (fill) {
        stage_row(s_row, dp, W, nq);                        // (out may be disp itself: the row is read before it is written)
        __syncthreads();
        fill_row(s_row, s_last, s_first, s_wl, s_wf, kept.bits, nq, W, op, vout);
    }
    if (row_cnt) {
        __syncthreads();
        if (t < 3) row_cnt[3 * ((int64_t)b * H + y) + t] = row_total<3>(s_n, t);
    }
}

// grid (B), 256 threads: counts[b][j] = the sum over the rows of row_cnt[b][y][j] (integers; a fixed tree).
__global__ __launch_bounds__(kThreads) void k_sp_counts(const int *__restrict__ row_cnt, int H, int64_t *__restrict__ counts)
{
    __shared__ long long s_n[kWaves][3];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int *r = row_cnt + 3 * (int64_t)b * H;
    long long n[3] = {0, 0, 0};
    for (int64_t y = t; y < H; y += kThreads)
        for (int j = 0; j < 3; ++j) n[j] += r[3 * y + j];
    for (int o = 32; o > 0; o >>= 1)                        // (wave_sum_n, spelt out: through it the 64-bit adds come out commuted)
        for (int j = 0; j < 3; ++j) n[j] += __shfl_down(n[j], o, 64);
    if (lane == 0)
        for (int j = 0; j < 3; ++j) s_n[wave][j] = n[j];
    __syncthreads();
    if (t < 3) counts[3 * (int64_t)b + t] = sum4(s_n[0][t], s_n[1][t], s_n[2][t], s_n[3][t]);
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int64_t lws_speckle_workspace(int B, int H, int W)
{
    LWS_CHECK_RC(check_image_shape("speckle_workspace", B, H, W, 31));
    const int64_t px = (int64_t)B * H * W;
    return 2 * round256(px * (int64_t)sizeof(int)) + round256(3 * (int64_t)B * H * (int64_t)sizeof(int));
}

int lws_speckle_filter(const float *disp, const uint8_t *mask, int B, int H, int W, float max_diff, int max_size, int fill,
                       void *workspace, float *out, uint8_t *mask_out, int32_t *labels, int64_t *counts, void *stream)
{
    LWS_CHECK_RC(check_image_shape("speckle_filter", B, H, W, 31));
    LWS_CHECK_ARG(disp && workspace && out && mask_out, "speckle_filter: disp, workspace, out and mask_out must not be null");
    LWS_CHECK_ARG(finite_nonneg(max_diff), "speckle_filter: max_diff must be finite and >= 0, got %g", (double)max_diff);
    LWS_CHECK_ARG(max_size >= 0, "speckle_filter: max_size must be >= 0, got %d", max_size);
    LWS_CHECK_RC(check_fill("speckle_filter", fill));
    LWS_CHECK_ARG(!fill || W <= kMaxW, "speckle_filter: fill needs W <= %d (the row is staged in LDS), got %d", kMaxW, W);
    LWS_CHECK_ARG(aligned(disp, 4) && aligned(out, 4) && aligned(workspace, 16) && aligned(labels, 4) && aligned(counts, 8),
                  "speckle_filter: disp / out / labels must be 4-byte, counts 8-byte, workspace 16-byte aligned");
    const int64_t px = (int64_t)B * H * W;
    const int64_t ws = lws_speckle_workspace(B, H, W);
    // out may be disp itself and mask_out may be mask itself (a row is read before it is written, the labelling before both);
    // any other overlap between an input, an output and the workspace is an error, disp and mask included: every pair is checked
    const Buf bufs[] = {{workspace, ws, "workspace"}, {counts, 24 * (int64_t)B, "counts"}, {labels, 4 * px, "labels"}, {mask_out, px, "mask_out"},
                        {out, 4 * px, "out"},         {mask, px, "mask"},                  {disp, 4 * px, "disp"}};
    const int in_place[][2] = {{4, 6}, {3, 5}};             // out / disp, mask_out / mask
    LWS_CHECK_RC(check_no_overlap("speckle_filter", bufs, 7, 7, in_place, 2));

    int *parent = static_cast<int *>(workspace);
    int *size = reinterpret_cast<int *>(static_cast<char *>(workspace) + round256(px * (int64_t)sizeof(int)));
    int *row_cnt = counts ? reinterpret_cast<int *>(static_cast<char *>(workspace) + 2 * round256(px * (int64_t)sizeof(int))) : nullptr;
    const int ntx = (W + kTileCols - 1) / kTileCols, nty = (H + kTileRows - 1) / kTileRows;
    const int64_t pairs = (int64_t)(nty - 1) * W + (int64_t)(ntx - 1) * H;
    const int HW = H * W;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_sp_tile, dim3((unsigned)((int64_t)ntx * nty), B), dim3(kThreads), 0, st, disp, mask, H, W, ntx, max_diff, parent,
                       size);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sp_border, dim3((unsigned)((pairs + kThreads - 1) / kThreads > 0 ? (pairs + kThreads - 1) / kThreads : 1), B),
                       dim3(kThreads), 0, st, disp, H, W, nty, ntx, max_diff, parent);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sp_flatten, dim3((unsigned)(((int64_t)HW + kThreads - 1) / kThreads), B), dim3(kThreads), 0, st, HW, parent, size);
    LWS_LAUNCH_CHECK();
    const int nq = (W + 3) / 4;
    const size_t lds = fill ? (size_t)4 * nq * sizeof(float) + (size_t)2 * nq * sizeof(int) : 0;
    hipLaunchKernelGGL(k_sp_apply, dim3(H, B), dim3(kThreads), lds, st, disp, mask, H, W, max_size, fill, parent, size, out, mask_out,
                       labels, row_cnt);
    LWS_LAUNCH_CHECK();
    if (counts) {
        hipLaunchKernelGGL(k_sp_counts, dim3(B), dim3(kThreads), 0, st, row_cnt, H, counts);
        LWS_LAUNCH_CHECK();
    }
    return LWS_OK;
}

}  // extern "C"
