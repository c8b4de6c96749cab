// Stixels and the u-disparity of the obstacle columns: per strip of `width` columns, the histogram of the obstacle pixels'
// disparities over all rows, and per layer -- nearest first -- the nearest well-supported bin, the rows where it stands, and the
// disparity, depth, lateral position and height of what stands there.  Contract: include/lwsnet_hip.h, lws_stixels; restated bit
// for bit by tests/stixel_reference.py.  One IEEE operation per step (no fma), float32 per pixel, integers for every sum, float64
// only for the mean disparity.
//   k_stixels   one workgroup per strip and image, one launch.  The strip is read as items of 4 columns (float4 / uchar4 where
//               the strip's start is aligned and the item whole, scalar otherwise).  In LDS: the strip's histogram U (<= 4096 words),
//               the members per row r[y] as one byte per row, four rows to a word (<= 4096 words), and 256 + 16 words of the
//               reductions: 33.1 KB.  Per layer: the window scan over the bins, a pass over the strip for r[y], the walk on a
//               64-row bit mask per thread, and a pass over the rows y_top .. y_base for n, SQ and the top.  The later passes read the
//               strip again where it lies (a few KB, in L2).
// Determinism: what crosses lanes or waves is an integer add or an integer / unsigned maximum (LDS atomics, wave shuffles);
// a strip belongs to one workgroup, so there is no global atomic.  0 bytes of scratch.
#include "lws_geomkit.h"
#include "lws_opkit.h"
#include "lws_takekit.h"

namespace lws {

namespace {

using namespace geomkit;
using namespace takekit;                    // the limits, Item / load_item, Rule / bin_of, u16f
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxTolBins = 8;
constexpr int kMaxLayers = 4;

typedef unsigned long long u64;

// The maximum over the workgroup's 256 threads, in every thread.  s_m: kWaves words nobody else uses; two barriers, so that the
// next call may write them again.
__device__ __forceinline__ int block_max(int v, int *s_m)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = v;
    __syncthreads();
    v = max(max(s_m[0], s_m[1]), max(s_m[2], s_m[3]));
    __syncthreads();
    return v;
}

__device__ __forceinline__ void store_slot(int32_t *__restrict__ rows, float *__restrict__ vals, int n, int y_top, int y_base, int k_peak,
                                           float d, float z, float X, float h)
{
    rows[0] = n, rows[1] = y_top, rows[2] = y_base, rows[3] = k_peak;
    vals[0] = d, vals[1] = z, vals[2] = X, vals[3] = h;
}

// grid (S, B), 256 threads: the strip blockIdx.x of image blockIdx.y.
__global__ __launch_bounds__(kThreads) void k_stixels(const float *__restrict__ disp, const float *__restrict__ cam,
                                                     const uint8_t *__restrict__ codes, const float *__restrict__ height, int H, int W,
                                                     float min_disp, float max_depth, unsigned code_bits, int width, int sub, int nbins,
                                                     int tol_bins, int min_count, int min_row, int max_gap, int layers,
                                                     int32_t *__restrict__ rows, float *__restrict__ vals, uint32_t *__restrict__ udisp)
{
    __shared__ unsigned s_u[kMaxBins];                      // U[k]
    __shared__ unsigned s_r[kMaxDim / 4];                   // r[y], byte y & 3 of word y >> 2
    __shared__ int s_last[kThreads];                        // the walk: the last flagged row of each thread's 64
    __shared__ int s_m[kWaves];
    __shared__ long long s_s[2][kWaves];
    __shared__ unsigned s_h[kWaves];
    const int s = blockIdx.x, b = blockIdx.y, S = gridDim.x, t = threadIdx.x;
    const int x0 = s * width, x1 = min(x0 + width, W) - 1, ws = x1 - x0 + 1;
    const int nc = (ws + 3) >> 2, items = H * nc, rwords = (H + 3) >> 2;
    const int64_t base = (int64_t)b * H * W + x0;           // the strip's first pixel
    const Cam c = load_cam(cam, b);
    const Rule rule = {c.fb, min_disp, max_depth, (float)sub, (float)nbins, code_bits};

    // ---- the u-disparity column of the strip ----
    for (int i = t; i < nbins; i += kThreads) s_u[i] = 0u;
    __syncthreads();
    for (int i = t; i < items; i += kThreads) {
        const int y = i / nc, xs = 4 * (i - y * nc);
        const int64_t at = base + (int64_t)y * W;
        const Item it = load_item(disp + at, codes + at, xs, ws);
        int q[4];
        unsigned n[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = bin_of(it.d[j], it.code[j], rule), n[j] = 1u;
        // a fronto-parallel obstacle puts its pixels into few bins: the runs of equal bins of an item are added once
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if (q[j] >= 0 && q[j] == q[j - 1]) n[j] += n[j - 1], q[j - 1] = -1;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q[j] >= 0) atomicAdd(&s_u[q[j]], n[j]);
    }
    __syncthreads();
    if (udisp) {
        uint32_t *o = udisp + ((int64_t)b * S + s) * nbins;
        for (int i = t; i < nbins; i += kThreads) o[i] = s_u[i];
    }

    int32_t *orow = rows + ((int64_t)b * S + s) * layers * 4;
    float *oval = vals + ((int64_t)b * S + s) * layers * 4;
    int kmax = nbins - 1;
    for (int layer = 0; layer < layers; ++layer, orow += 4, oval += 4) {       // (every branch below is uniform over the workgroup)
        // ---- the nearest bin whose window holds min_count pixels, and the peak beside it ----
        int near = -1;
        for (int k = t; k <= kmax; k += kThreads) {
            unsigned wn = 0u;
            for (int j = max(k - tol_bins, 0); j <= min(k + tol_bins, kmax); ++j) wn += s_u[j];
            if (wn >= (unsigned)min_count) near = k;        // ascending k: the thread's largest stays
        }
        near = block_max(near, s_m);
        if (near < 0) {                                     // this layer and every later one are empty
            if (t == 0)
                for (; layer < layers; ++layer, orow += 4, oval += 4) store_slot(orow, oval, 0, -1, -1, -1, 0.0f, 0.0f, 0.0f, 0.0f);
            return;
        }
        int peak = max(near - tol_bins, 0);
        unsigned most = s_u[peak];
        for (int j = peak + 1; j <= min(near + tol_bins, kmax); ++j) {
            const unsigned u = s_u[j];
            if (u >= most) most = u, peak = j;              // the larger bin wins a tie
        }
        const int q_lo = peak - tol_bins, q_hi = min(peak + tol_bins, kmax);    // the members' bins
        kmax = peak - tol_bins - 1;

        // ---- r[y] ----
        for (int i = t; i < rwords; i += kThreads) s_r[i] = 0u;
        __syncthreads();
        for (int i = t; i < items; i += kThreads) {
            const int y = i / nc, xs = 4 * (i - y * nc);
            const int64_t at = base + (int64_t)y * W;
            const Item it = load_item(disp + at, codes + at, xs, ws);
            unsigned n = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = bin_of(it.d[j], it.code[j], rule);
                n += q >= q_lo && q <= q_hi && q >= 0 ? 1u : 0u;
            }
            if (n) atomicAdd(&s_r[y >> 2], n << (8 * (y & 3)));     // at most 64 per row: no carry into the next byte
        }
        __syncthreads();

        // ---- the walk: thread t holds the flags of the rows 64 t .. 64 t + 63 ----
        u64 flags = 0ull;
        for (int j = 0; j < 16; ++j) {
            const int wi = 16 * t + j;
            const unsigned w = wi < rwords ? s_r[wi] : 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((int)((w >> (8 * k)) & 0xffu) >= min_row) flags |= 1ull << (4 * j + k);
        }
        const int last = flags ? 64 * t + 63 - __clzll((long long)flags) : -1;
        s_last[t] = last;
        const int y_base = block_max(last, s_m);            // (its barrier publishes s_last)
        if (y_base < 0) {                                   // a hole: the next layer still runs
            if (t == 0) store_slot(orow, oval, 0, -1, -1, peak, 0.0f, 0.0f, 0.0f, 0.0f);
            continue;
        }
        // A flagged row is a top when no flagged row lies above it or more than max_gap unflagged rows lie between the two; the
        // walk from y_base stops at the lowest top, the largest such row.
        int top = -1;
        if (flags) {
            int prev = -1;
            for (int u = t - 1; u >= 0 && prev < 0; --u) prev = s_last[u];
            while (flags) {
                const int y = 64 * t + __ffsll((long long)flags) - 1;
                flags &= flags - 1;
                if (prev < 0 || y - prev - 1 > max_gap) top = y;
                prev = y;
            }
        }
        const int y_top = block_max(top, s_m);

        // ---- n, SQ and the top over the members in the rows y_top .. y_base ----
        long long sum[2] = {0, 0};
        unsigned hb = 0u;
        for (int i = y_top * nc + t; i < (y_base + 1) * nc; i += kThreads) {
            const int y = i / nc, xs = 4 * (i - y * nc);
            const int64_t at = base + (int64_t)y * W;
            const Item it = load_item(disp + at, codes + at, xs, ws);
            float h[4];
            load_quad(height + at, xs, ws, aligned(height + at, 16), h);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = bin_of(it.d[j], it.code[j], rule);
                if (!(q >= q_lo && q <= q_hi && q >= 0)) continue;
                sum[0] += 1, sum[1] += (int)u16f(it.d[j]);
                hb = max(hb, __float_as_uint(h[j]));
            }
        }
        wave_sum_n(sum);
        for (int o = 32; o > 0; o >>= 1) hb = max(hb, (unsigned)__shfl_xor((int)hb, o, 64));
        if ((t & 63) == 0) s_s[0][t >> 6] = sum[0], s_s[1][t >> 6] = sum[1], s_h[t >> 6] = hb;
        __syncthreads();
        if (t == 0) {
            const long long n = sum4(s_s[0][0], s_s[0][1], s_s[0][2], s_s[0][3]), sq = sum4(s_s[1][0], s_s[1][1], s_s[1][2], s_s[1][3]);
            const unsigned top_bits = max(max(s_h[0], s_h[1]), max(s_h[2], s_h[3]));
            const float d_st = (float)(((double)sq / (double)n) / 256.0);
            const float z = c.fb / d_st;
            const float xc = (float)(x0 + x1) * 0.5f;
            const float X = ((xc - c.cx) * z) / c.fx;
            store_slot(orow, oval, (int)n, y_top, y_base, peak, d_st, z, X, __uint_as_float(top_bits));
        }
        __syncthreads();                                    // s_s, s_h and s_r are free for the next layer
    }
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int lws_stixels(const float *disp, const float *cam, const uint8_t *codes, const float *height, int B, int H, int W, float min_disp,
                float max_depth, int code_bits, int width, int sub, int nbins, int tol_bins, int min_count, int min_row, int max_gap,
                int layers, int32_t *rows, float *vals, uint32_t *udisp, void *stream)
{
    LWS_CHECK_RC(check_geometry_args("stixels", disp, B, H, W, min_disp, max_depth));
    LWS_CHECK_ARG(H <= kMaxDim && W <= kMaxDim, "stixels: H=%d W=%d exceed %d (a row's byte in LDS, the 64-bit sums)", H, W, kMaxDim);
    LWS_CHECK_ARG(cam && codes && height, "stixels: cam, codes and height must not be null");
    LWS_CHECK_ARG(rows && vals, "stixels: rows and vals must not be null");
    LWS_CHECK_ARG(aligned(cam, 4) && aligned(height, 4) && aligned(rows, 4) && aligned(vals, 4) && aligned(udisp, 4),
                  "stixels: cam / height / rows / vals / udisp must be 4-byte aligned");
    LWS_CHECK_ARG(code_bits >= 0 && code_bits < 64, "stixels: code_bits %d outside 0..63", code_bits);
    LWS_CHECK_ARG((code_bits & 0x33) == 0, "stixels: code_bits %d selects a code other than 2 and 3, whose heights are not positive",
                  code_bits);
    LWS_CHECK_ARG(width >= 1 && width <= kMaxWidth, "stixels: width %d outside 1..%d", width, kMaxWidth);
    LWS_CHECK_ARG(sub >= 1 && sub <= kMaxSub, "stixels: sub %d outside 1..%d", sub, kMaxSub);
    LWS_CHECK_ARG(nbins >= 1 && nbins <= kMaxBins && nbins <= 256 * sub, "stixels: nbins %d outside 1..min(%d, 256 * sub = %d)", nbins,
                  kMaxBins, 256 * sub);
    LWS_CHECK_ARG(tol_bins >= 0 && tol_bins <= kMaxTolBins, "stixels: tol_bins %d outside 0..%d", tol_bins, kMaxTolBins);
    LWS_CHECK_ARG(min_count >= 1, "stixels: min_count %d < 1", min_count);
    LWS_CHECK_ARG(min_row >= 1, "stixels: min_row %d < 1", min_row);
    LWS_CHECK_ARG(max_gap >= 0, "stixels: max_gap %d < 0", max_gap);
    LWS_CHECK_ARG(layers >= 1 && layers <= kMaxLayers, "stixels: layers %d outside 1..%d", layers, kMaxLayers);
    const int S = (W + width - 1) / width;
    const int64_t px = (int64_t)B * H * W, slots = 16 * (int64_t)B * S * layers;
    const Buf bufs[] = {{rows, slots, "rows"}, {vals, slots, "vals"}, {udisp, 4 * (int64_t)B * S * nbins, "udisp"}, {disp, 4 * px, "disp"},
                        {cam, 20 * (int64_t)B, "cam"}, {codes, px, "codes"}, {height, 4 * px, "height"}};
    LWS_CHECK_RC(check_no_overlap("stixels", bufs, 7, 3));
    hipLaunchKernelGGL(k_stixels, dim3(S, B), dim3(kThreads), 0, (hipStream_t)stream, disp, cam, codes, height, H, W, min_disp, max_depth,
                       (unsigned)code_bits, width, sub, nbins, tol_bins, min_count, min_row, max_gap, layers, rows, vals, udisp);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // extern "C"
