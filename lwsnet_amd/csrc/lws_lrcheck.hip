// Left-right consistency check of the stage maps: the right view's disparity comes from the same left-reference network run on
// the mirrored, swapped pair (mirror(R), mirror(L)) in one forward of 2B pairs (k_lr_pairs builds its input), and k_lr_check
// compares the two per pixel, marks the pixels to trust and optionally fills the others with background values.
// Arithmetic contract (include/lwsnet_hip.h, lws_lr_check): one IEEE float32 operation per step (the build has no contraction),
// so tests/lr_reference.py restates every output bit for bit in numpy.  Determinism: no atomics; a workgroup owns one row of one
// image and map, so an image gives the same bits in any batch.  0 bytes of scratch; the row lives in LDS.
#include "lws_common.h"
#include "lws_rowkit.h"

namespace lws {

namespace {

using namespace rowkit;                                     // kThreads, kWaves, kMaxW: dRm / dL row + two int per quad, 48 KiB of LDS at most

struct LrMaps {                                             // the nmaps stage maps of one call, by value in the kernel arguments
    const float *dl[4];
    const float *drm[4];
    float *out[4];
    uint8_t *mask[4];
    float *right[4];
};

// 1 = consistent, 0 = inconsistent (or NaN), 2 = the matching right pixel x - d is outside the right camera's view (incl. +-inf)
__device__ __forceinline__ int lr_code(float d, int x, int W, const float *__restrict__ R, float tau)
{
    if (__builtin_isnan(d)) return 0;
    const float t = (float)(W - 1 - x) + d;                 // mirrored column of x - d
    if (!(t >= 0.0f && t <= (float)(W - 1))) return 2;
    const int i0 = (int)floorf(t);
    const int i1 = min(i0 + 1, W - 1);
    const float a = t - (float)i0;
    const float r = R[i0] + a * (R[i1] - R[i0]);
    return fabsf(d - r) <= tau ? 1 : 0;                     // NaN r -> 0
}

// grid (H, B, nmaps), 256 threads: one workgroup per row, thread t owns the quads t, t + 256, ... of it (lws_rowkit.h).
// LDS (dynamic): row[4 nq] floats (first dRm, then dL for the fill), last[nq], first[nq] ints (fill only).
__global__ __launch_bounds__(kThreads) void k_lr_check(LrMaps m, int H, int W, float tau, int fill, int *__restrict__ row_kept)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int s_wl[kWaves], s_wf[kWaves], s_kept[kWaves];
    const int y = blockIdx.x, b = blockIdx.y, s = blockIdx.z, t = threadIdx.x;
    const int nq = (W + 3) >> 2;
    float *s_row = lds;
    int *s_last = reinterpret_cast<int *>(lds + 4 * nq), *s_first = s_last + nq;
    const int64_t row = ((int64_t)b * H + y) * W;
    const float *dl = m.dl[s] + row, *rm = m.drm[s] + row;
    float *out = m.out[s] + row, *rt = m.right[s] ? m.right[s] + row : nullptr;
    uint8_t *mk = m.mask[s] + row;
    const bool vdl = aligned(dl, 16), vout = aligned(out, 16), vrt = aligned(rt, 16), vmk = aligned(mk, 4);

    stage_row(s_row, rm, W, nq);                            // the mirrored right-view row
    __syncthreads();

    // ---- phase 1: codes, mask, right, out (no fill), kept count, per-quad last / first consistent pixel ----
    KeptFlags kept;
    for (int k = 0, q = t; q < nq; ++k, q += kThreads) {
        const int x = 4 * q;
        float d[4];
        int c[4];
        load_quad(dl, x, W, vdl, __builtin_nanf(""), d);    // NaN beyond the row: code 0, never kept
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = lr_code(d[i], x + i, W, s_row, tau);
        store_codes(mk, x, W, vmk, c);
        if (rt) {                                           // right[x] = dRm[W-1-x]
            const int xr = W - 1 - x;
            store_quad(rt, x, W, vrt, s_row[xr], s_row[max(xr - 1, 0)], s_row[max(xr - 2, 0)], s_row[max(xr - 3, 0)]);
        }
        if (!fill) store_kept(out, x, W, vout, c, d);
        bool ok[4];
        kept.add(k, c, ok);
        if (fill) quad_last_first(ok, x, s_last[q], s_first[q]);
    }

    if (row_kept) wave_sums<1>({kept.count}, s_kept);
    if (fill) {
        __syncthreads();                                    // every read of the staged dRm row is done
        stage_row(s_row, dl, W, nq);                        // the left-view row, for the fill values
        // phases 2 and 3: scans of last / first over the quads, then consistent pixels keep d and the others take the background
        // value of their row
        fill_row(s_row, s_last, s_first, s_wl, s_wf, kept.bits, nq, W, out, vout);
    }
    if (row_kept) {
        __syncthreads();
        if (t == 0) row_kept[((int64_t)s * gridDim.y + b) * H + y] = row_total<1>(s_kept, 0);
    }
}

// One thread per quad of a row of the [B,3,H,W] inputs (rows = B * 3 * H): left2 = [left; mirror_w(right)],
// right2 = [right; mirror_w(left)].  vec (launch-uniform): W % 4 == 0 and every base 16-byte aligned, so every quad and its mirror
// image are aligned float4s.
__global__ __launch_bounds__(kThreads) void k_lr_pairs(const float *__restrict__ L, const float *__restrict__ R, float *__restrict__ L2,
                                                      float *__restrict__ R2, int rows, int W, int nq, int vec)
{
    const int g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= rows * nq) return;
    const int row = g / nq, x = 4 * (g - row * nq);
    const int64_t top = (int64_t)row * W, bot = ((int64_t)rows + row) * W;
    const float *l = L + top, *r = R + top;
    float *lt = L2 + top, *rt = R2 + top, *lb = L2 + bot, *rb = R2 + bot;
    if (vec) {
        const float4 a = *reinterpret_cast<const float4 *>(l + x), c = *reinterpret_cast<const float4 *>(r + x);
        *reinterpret_cast<float4 *>(lt + x) = a;
        *reinterpret_cast<float4 *>(rt + x) = c;
        *reinterpret_cast<float4 *>(lb + W - 4 - x) = make_float4(c.w, c.z, c.y, c.x);
        *reinterpret_cast<float4 *>(rb + W - 4 - x) = make_float4(a.w, a.z, a.y, a.x);
    } else {
        for (int i = 0; i < 4 && x + i < W; ++i) {
            const float a = l[x + i], c = r[x + i];
            lt[x + i] = a;
            rt[x + i] = c;
            lb[W - 1 - x - i] = c;
            rb[W - 1 - x - i] = a;
        }
    }
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int lws_lr_pairs(const float *left, const float *right, float *left2, float *right2, int B, int H, int W, void *stream)
{
    LWS_CHECK_ARG(left && right && left2 && right2, "lr_pairs: null pointer");
    LWS_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "lr_pairs: bad shape B=%d H=%d W=%d", B, H, W);
    const int64_t rows = (int64_t)B * 3 * H, nq = ((int64_t)W + 3) / 4;
    LWS_CHECK_ARG(rows * nq <= (int64_t)INT32_MAX - kThreads, "lr_pairs: %dx3x%dx%d is too large", B, H, W);
    const int vec = (W % 4 == 0) && ((((uintptr_t)left | (uintptr_t)right | (uintptr_t)left2 | (uintptr_t)right2) & 15) == 0);
    const int64_t n = rows * nq;
    hipLaunchKernelGGL(k_lr_pairs, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, left, right,
                       left2, right2, (int)rows, W, (int)nq, vec);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

int lws_lr_check(const float *const dL[4], const float *const dRm[4], int nmaps, int B, int H, int W, float tau, int fill,
                 float *const out[4], uint8_t *const mask[4], float *const right[4], int32_t *row_kept, void *stream)
{
    LWS_CHECK_ARG(dL && dRm && out && mask, "lr_check: null pointer");
    LWS_CHECK_RC(opkit::check_row_check_args("lr_check", "(the row is staged in LDS)", kMaxW, dL, dRm, nmaps, B, H, W, tau, fill, out, mask));
    LrMaps m = {};
    for (int s = 0; s < nmaps; ++s) {
        m.dl[s] = dL[s];
        m.drm[s] = dRm[s];
        m.out[s] = out[s];
        m.mask[s] = mask[s];
        m.right[s] = right ? right[s] : nullptr;
    }
    const int nq = (W + 3) / 4;
    const size_t lds = (size_t)4 * nq * sizeof(float) + (fill ? (size_t)2 * nq * sizeof(int) : 0);
    hipLaunchKernelGGL(k_lr_check, dim3(H, B, nmaps), dim3(kThreads), lds, (hipStream_t)stream, m, H, W, tau, fill, row_kept);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // extern "C"
