// The road under a disparity map: the classic v-disparity pipeline -- row histograms, a Hough vote for the road's line, an iterated
// least-squares plane through its inliers, a height-over-the-plane code per pixel and an occupancy grid seen from above.
// Arithmetic contract (include/lwsnet_hip.h, lws_vdisparity): one IEEE operation per step (the build has no contraction and
// correctly rounded division and square root; no fma here), float32 per pixel, float64 for the plane, integers for every sum, so
// tests/ground_reference.py restates every output bit for bit in numpy.  Determinism: what crosses lanes or workgroups is an
// integer add or an integer max (LDS and global atomics, wave sums), whose order cannot show.
//   k_vdisparity     one workgroup per row: the row's histogram in LDS, equal bins of a wave joined by ballots before the LDS atomic
//   k_ground_clear   the workspace words of the call
//   k_hough          one workgroup per horizon row yh and 64 bottom bins qB, its four waves sharing the rows below yh; the winner
//                    by one packed 64-bit atomic max per workgroup
//   k_ground_seed    one thread per image: the winner as the plane of pass 0
//   k_fit_accum      one workgroup per row: the inliers' five row sums by wave sums, the nine sums by 64-bit atomic adds
//   k_fit_solve      one thread per image: the 2 x 2 normal equations in float64
//   k_classify       one thread per quad: height and code; the six counts by packed wave sums and 64-bit atomic adds
//   k_bev_clear, k_bev_scatter   one thread per quad: atomic add / unsigned atomic max per cell, equal cells of a quad and of a wave's lanes
//                    joined first
// 0 bytes of scratch.
#include "lws_geomkit.h"
#include "lws_opkit.h"

namespace lws {

namespace {

using namespace geomkit;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBins = 4096;              // a row's histogram in LDS: 16 KB
constexpr int kMaxSub = 16;
constexpr int kMaxDim = 16384;              // lws_ground_fit: H, W; every sum stays below 2^62
constexpr int kMinHorizon = -65536;         // 2 * qB * (y - yh) + den fits an int32
constexpr int kMaxCandidates = 1 << 22;
constexpr int kMaxTolBins = 8;
constexpr int kMaxIters = 8;
constexpr int kMaxGrid = 4096;
// the 64-bit words of an image in the workspace of lws_ground_fit
constexpr int kWsWords = 16;
constexpr int kBest = 0;                    // (score << 32) | ~candidate
constexpr int kSums = 1;                    // n, Sx, Sy, SQ, Sxx, Sxy, Syy, SxQ, SyQ
constexpr int kPlane = 10;                  // a, b, c of the current pass: float64, in 1/256 px
constexpr int kStatus = 13;
constexpr int kOk = 0, kNoGround = 1, kDegenerate = 2;

typedef unsigned long long u64;

// The bin of a pixel lws_vdisparity counts, -1 for any other.  The compare against the bin count is on the float: a huge product
// is never converted.
__device__ __forceinline__ int bin_of(float d, bool ok, float min_disp, float fsub, float fbins)
{
    const float t = floorf(d * fsub);
    return ok && __builtin_isfinite(d) && d >= min_disp && t < fbins ? (int)t : -1;
}

// u16(v) of lws_depth_maps, as the float32 it is before the conversion
__device__ __forceinline__ float u16f(float v) { return fminf(fmaxf(rintf(v * 256.0f), 0.0f), 65535.0f); }

// grid (H, B), 256 threads.
__global__ __launch_bounds__(kThreads) void k_vdisparity(const float *__restrict__ disp, const uint8_t *__restrict__ mask, int H, int W,
                                                        float min_disp, int sub, int nbins, uint32_t *__restrict__ hist)
{
    __shared__ unsigned s_h[kMaxBins];
    const int y = blockIdx.x, b = blockIdx.y, t = threadIdx.x, lane = t & 63;
    for (int i = t; i < nbins; i += kThreads) s_h[i] = 0u;
    __syncthreads();
    const int64_t row = ((int64_t)b * H + y) * W;
    const float *dp = disp + row;
    const uint8_t *mk = mask ? mask + row : nullptr;
    const bool vd = aligned(dp, 16), vm = aligned(mk, 4);
    const float fsub = (float)sub, fbins = (float)nbins;
    const int nq = (W + 3) >> 2;
    for (int q0 = 0; q0 < nq; q0 += kThreads) {             // (every thread of a wave takes every trip: the ballots below)
        const int q = q0 + t;
        float d[4];
        bool ok[4];
        if (q < nq) {
            load_quad(dp, 4 * q, W, vd, d);
            load_ok(mk, 4 * q, W, vm, ok);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) d[i] = 0.0f, ok[i] = false;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int bin = bin_of(d[i], ok[i], min_disp, fsub, fbins);
            const u64 any = __ballot(bin >= 0);
            if (any == 0) continue;                         // wave-uniform
            const int b0 = __shfl(bin, __ffsll((long long)any) - 1, 64);
            const u64 same = __ballot(bin == b0);           // a road row: most of the wave
            if (bin == b0) {
                if (lane == __ffsll((long long)same) - 1) atomicAdd(&s_h[b0], (unsigned)__popcll(same));
            } else if (bin >= 0) {
                atomicAdd(&s_h[bin], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t *o = hist + ((int64_t)b * H + y) * nbins;
    for (int i = t; i < nbins; i += kThreads) o[i] = s_h[i];
}

// grid (ceil(n / 256)): n 64-bit words
__global__ __launch_bounds__(kThreads) void k_ground_clear(u64 *__restrict__ w, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) w[i] = 0ull;
}

// The bin the line (yh, qB) expects in row y > yh; den = H - 1 - yh > 0.  Non-negative values below 2^31.
__device__ __forceinline__ int line_bin(int qb, int dy, int den) { return (int)((unsigned)(2 * qb * dy + den) / (unsigned)(2 * den)); }

// grid (nyh, ceil(nqb / 64), B), 256 threads: the candidates (yh_lo + blockIdx.x, qb_lo + 64 blockIdx.y + lane); wave w takes the rows
// y0 + w, y0 + w + 4, ..  The histogram (about 1 MB at KITTI size) stays in L2 and the lanes of a wave read neighbouring bins, so
// the rows are read where they lie; four short chains of dependent loads instead of one long one.
__global__ __launch_bounds__(kThreads) void k_hough(const uint32_t *__restrict__ hist, int H, int nbins, int yh_lo, int qb_lo, int qb_hi,
                                                   int nyh, int tol_bins, u64 *__restrict__ ws)
{
    __shared__ unsigned s_p[kWaves][64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.z;
    const int yh = yh_lo + (int)blockIdx.x, den = H - 1 - yh;
    const int qb = qb_lo + (int)blockIdx.y * 64 + lane;
    const bool active = qb <= qb_hi;
    const uint32_t *hb = hist + (int64_t)b * H * nbins;
    unsigned score = 0;
    if (active) {
        for (int y = max(yh + 1, 0) + wave; y < H; y += kWaves) {
            const int k = line_bin(qb, y - yh, den);
            const int k0 = max(k - tol_bins, 0), k1 = min(k + tol_bins, nbins - 1);
            const uint32_t *r = hb + (int64_t)y * nbins;
            for (int j = k0; j <= k1; ++j) score += r[j];
        }
    }
    s_p[wave][lane] = score;
    __syncthreads();
    if (wave != 0) return;
    score = (s_p[0][lane] + s_p[1][lane]) + (s_p[2][lane] + s_p[3][lane]);
    // the highest score, then the smaller qB, then the smaller yh: the candidates are numbered in that order
    const unsigned cand = (unsigned)(qb - qb_lo) * (unsigned)nyh + blockIdx.x;
    u64 best = active ? ((u64)score << 32) | (u64)(~cand) : 0ull;
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = __shfl_down(best, o, 64);
        best = other > best ? other : best;
    }
    if (lane == 0 && best != 0ull) atomicMax(ws + (int64_t)b * kWsWords + kBest, best);
}

__device__ __forceinline__ void store_plane(float *__restrict__ p, float a, float b, float c, float e)
{
    p[0] = a, p[1] = b, p[2] = c, p[3] = e;
}

// grid (B), 64 threads; thread 0: the winner -> info, the plane of pass 0 and the status -> the workspace.
__global__ __launch_bounds__(64) void k_ground_seed(u64 *__restrict__ ws, int H, int sub, int nyh, int yh_lo, int qb_lo, int min_score,
                                                   float *__restrict__ plane, int32_t *__restrict__ info)
{
    if (threadIdx.x != 0) return;
    const int b = blockIdx.x;
    u64 *w = ws + (int64_t)b * kWsWords;
    const u64 best = w[kBest];
    const unsigned score = (unsigned)(best >> 32), cand = ~(unsigned)best;
    const int qb = qb_lo + (int)(cand / (unsigned)nyh), yh = yh_lo + (int)(cand % (unsigned)nyh);
    const int status = (long long)score < (long long)min_score ? kNoGround : kOk;
    const int den = H - 1 - yh;
    const double pb = (256.0 * (double)qb) / ((double)sub * (double)den);
    const double pc = (-pb) * (double)yh + 128.0 / (double)sub;
    w[kPlane] = (u64)__double_as_longlong(0.0), w[kPlane + 1] = (u64)__double_as_longlong(pb), w[kPlane + 2] = (u64)__double_as_longlong(pc);
    w[kStatus] = (u64)status;
    int32_t *o = info + 8 * (int64_t)b;
    o[0] = status, o[1] = yh, o[2] = qb, o[3] = (int32_t)score, o[4] = 0, o[5] = 0, o[6] = 0, o[7] = 0;
    const float nan = __builtin_nanf("");
    store_plane(plane + 4 * (int64_t)b, nan, nan, nan, nan);
}

// grid (H, B), 256 threads: the inliers of row y against the workspace's plane.
__global__ __launch_bounds__(kThreads) void k_fit_accum(const float *__restrict__ disp, const uint8_t *__restrict__ mask, int H, int W,
                                                       float min_disp, int sub, int nbins, double tol256, u64 *__restrict__ ws)
{
    __shared__ long long s_s[5][kWaves];
    const int y = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    u64 *w = ws + (int64_t)b * kWsWords;
    if (w[kStatus] != 0ull) return;                         // (uniform) no ground, or degenerate in an earlier pass
    const double pa = __longlong_as_double((long long)w[kPlane]), pb = __longlong_as_double((long long)w[kPlane + 1]),
                 pc = __longlong_as_double((long long)w[kPlane + 2]);
    const double by = pb * (double)y;
    const int64_t row = ((int64_t)b * H + y) * W;
    const float *dp = disp + row;
    const uint8_t *mk = mask ? mask + row : nullptr;
    const bool vd = aligned(dp, 16), vm = aligned(mk, 4);
    const float fsub = (float)sub, fbins = (float)nbins;
    const int nq = (W + 3) >> 2;
    long long s[5] = {0, 0, 0, 0, 0};                       // n, Sx, SQ, Sxx, SxQ of the row
    for (int q = t; q < nq; q += kThreads) {
        float d[4];
        bool ok[4];
        load_quad(dp, 4 * q, W, vd, d);
        load_ok(mk, 4 * q, W, vm, ok);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (bin_of(d[i], ok[i], min_disp, fsub, fbins) < 0) continue;
            const int x = 4 * q + i;
            const float qf = u16f(d[i]);
            const double r = fabs((double)qf - ((pa * (double)x + by) + pc));
            if (!(r <= tol256)) continue;
            const int Q = (int)qf;
            s[0] += 1, s[1] += x, s[2] += Q, s[3] += x * x, s[4] += x * Q;
        }
    }
    wave_sum_n(s);
    if ((t & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 5; ++j) s_s[j][t >> 6] = s[j];
    }
    __syncthreads();
    if (t >= 9) return;
    long long r[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) r[j] = sum4(s_s[j][0], s_s[j][1], s_s[j][2], s_s[j][3]);
    if (r[0] == 0) return;
    // n, Sx, Sy, SQ, Sxx, Sxy, Syy, SxQ, SyQ: the moments in y are the row's sums times y, exactly
    const long long yy = y;
    const long long v[9] = {r[0], r[1], yy * r[0], r[2], r[3], yy * r[1], yy * yy * r[0], r[4], yy * r[2]};
    atomicAdd(w + kSums + t, (u64)v[t]);
}

// grid (B), 64 threads; thread 0: the plane of the pass's sums -> the workspace, plane and info; clears the sums.
__global__ __launch_bounds__(64) void k_fit_solve(u64 *__restrict__ ws, float *__restrict__ plane, int32_t *__restrict__ info)
{
    if (threadIdx.x != 0) return;
    const int b = blockIdx.x;
    u64 *w = ws + (int64_t)b * kWsWords;
    if (w[kStatus] != 0ull) return;
    long long s[9];
    for (int j = 0; j < 9; ++j) s[j] = (long long)w[kSums + j], w[kSums + j] = 0ull;
    const long long n = s[0];
    info[8 * (int64_t)b + 4] = (int32_t)n;
    bool good = n >= 3;
    double a = 0.0, bb = 0.0, c = 0.0;
    if (good) {
        const double fn = (double)n;
        const double mx = (double)s[1] / fn, my = (double)s[2] / fn, mq = (double)s[3] / fn;
        const double cxx = (double)s[4] / fn - mx * mx;
        const double cxy = (double)s[5] / fn - mx * my;
        const double cyy = (double)s[6] / fn - my * my;
        const double cxq = (double)s[7] / fn - mx * mq;
        const double cyq = (double)s[8] / fn - my * mq;
        const double det = cxx * cyy - cxy * cxy;
        good = det > 0.0;
        if (good) {
            a = (cxq * cyy - cyq * cxy) / det;
            bb = (cyq * cxx - cxq * cxy) / det;
            c = (mq - a * mx) - bb * my;
            good = __builtin_isfinite(a) && __builtin_isfinite(bb) && __builtin_isfinite(c);
        }
    }
    float *p = plane + 4 * (int64_t)b;
    if (!good) {
        const float nan = __builtin_nanf("");
        w[kStatus] = (u64)kDegenerate;
        info[8 * (int64_t)b] = kDegenerate;
        store_plane(p, nan, nan, nan, nan);
        return;
    }
    w[kPlane] = (u64)__double_as_longlong(a), w[kPlane + 1] = (u64)__double_as_longlong(bb), w[kPlane + 2] = (u64)__double_as_longlong(c);
    store_plane(p, (float)(a / 256.0), (float)(bb / 256.0), (float)(c / 256.0), 0.0f);
}

// grid (ceil(H * nq / 256), B): one thread per quad of a row.
__global__ __launch_bounds__(kThreads) void k_classify(const float *__restrict__ disp, const uint8_t *__restrict__ mask,
                                                      const float *__restrict__ cam, const float *__restrict__ plane, int H, int W, int nq,
                                                      float min_disp, float max_depth, float ground_tol, float max_height,
                                                      float *__restrict__ height, uint8_t *__restrict__ codes, u64 *__restrict__ counts)
{
    __shared__ int s_c[6][kWaves];
    const int g = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y, t = threadIdx.x;
    unsigned packed[2] = {0u, 0u};                          // codes 0..2 and 3..5 of the thread's pixels, 10 bits each
    if (g < H * nq) {
        const int y = g / nq, x = 4 * (g - y * nq);
        const int64_t row = ((int64_t)b * H + y) * W;
        const float *dp = disp + row;
        const uint8_t *mk = mask ? mask + row : nullptr;
        float d[4];
        bool ok[4];
        load_quad(dp, x, W, aligned(dp, 16), d);
        load_ok(mk, x, W, aligned(mk, 4), ok);
        const Cam c = load_cam(cam, b);
        const float pa = plane[4 * (int64_t)b], pb = plane[4 * (int64_t)b + 1], pc = plane[4 * (int64_t)b + 2];
        const float nx = pa * c.fx, ny = pb * c.fy, nz = (pa * c.cx + pb * c.cy) + pc;
        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
        const bool plane_ok = __builtin_isfinite(pa) && __builtin_isfinite(pb) && __builtin_isfinite(pc);
        const float by = pb * (float)y;
        float ho[4];
        uint8_t co[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float z;
            const bool v = valid_z(d[i], ok[i], c.fb, min_disp, max_depth, z);
            const float dpl = (pa * (float)(x + i) + by) + pc;
            const float h = ((d[i] - dpl) * z) / len;
            const int code = !v ? 0 : !(plane_ok && __builtin_isfinite(h)) ? 5 : fabsf(h) <= ground_tol ? 1 : h < 0.0f ? 4 : h <= max_height ? 2 : 3;
            co[i] = (uint8_t)code;
            ho[i] = code == 0 || code == 5 ? 0.0f : h;
            if (x + i < W) packed[code / 3] += 1u << (10 * (code % 3));
        }
        const bool full = x + 4 <= W;
        if (height) {
            float *p = height + row;
            if (full && aligned(p + x, 16)) {
                *reinterpret_cast<float4 *>(p + x) = make_float4(ho[0], ho[1], ho[2], ho[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (x + i < W) p[x + i] = ho[i];
            }
        }
        if (codes) {
            uint8_t *p = codes + row;
            if (full && aligned(p + x, 4)) {
                *reinterpret_cast<uchar4 *>(p + x) = make_uchar4(co[0], co[1], co[2], co[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (x + i < W) p[x + i] = co[i];
            }
        }
    }
    if (!counts) return;                                    // (uniform)
    wave_sum_n(packed);                                     // at most 256 per field
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s_c[k][t >> 6] = (int)((packed[k / 3] >> (10 * (k % 3))) & 1023u);
    }
    __syncthreads();
    if (t < 6) {
        const int n = sum4(s_c[t][0], s_c[t][1], s_c[t][2], s_c[t][3]);
        if (n) atomicAdd(counts + 6 * (int64_t)b + t, (u64)n);
    }
}

// grid (ceil(n / 256)): n 32-bit words of each grid that is given
__global__ __launch_bounds__(kThreads) void k_bev_clear(uint32_t *__restrict__ count, uint32_t *__restrict__ hmax, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if (count) count[i] = 0u;
    if (hmax) hmax[i] = 0u;                                 // +0.0f
}

// grid (ceil(H * nq / 256), B): one thread per quad of a row.
__global__ __launch_bounds__(kThreads) void k_bev_scatter(const float *__restrict__ disp, const float *__restrict__ cam,
                                                         const uint8_t *__restrict__ codes, const float *__restrict__ height, int H, int W,
                                                         int nq, float min_disp, float max_depth, unsigned code_bits, float x_min, float cell,
                                                         int Gx, int Gz, uint32_t *__restrict__ count, uint32_t *__restrict__ hmax)
{
    const int g = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y, lane = threadIdx.x & 63;
    int at[4] = {-1, -1, -1, -1};                           // the pixels' cells in the image's grid, -1: takes no part
    unsigned hb[4] = {0u, 0u, 0u, 0u};
    if (g < H * nq) {
        const int y = g / nq, x = 4 * (g - y * nq);
        const int64_t row = ((int64_t)b * H + y) * W;
        const float *dp = disp + row;
        const float *hp = height ? height + row : nullptr;
        const uint8_t *cp = codes + row;
        float d[4], h[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        load_quad(dp, x, W, aligned(dp, 16), d);
        if (hp) load_quad(hp, x, W, aligned(hp, 16), h);
        unsigned cd[4];
        if (x + 4 <= W && aligned(cp + x, 4)) {
            const uchar4 v = *reinterpret_cast<const uchar4 *>(cp + x);
            cd[0] = v.x, cd[1] = v.y, cd[2] = v.z, cd[3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) cd[i] = x + i < W ? cp[x + i] : 0xffu;
        }
        const Cam c = load_cam(cam, b);
        const float fgx = (float)Gx, fgz = (float)Gz;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float z;
            const bool v = valid_z(d[i], true, c.fb, min_disp, max_depth, z);
            if (!(v && cd[i] < 6u && ((code_bits >> cd[i]) & 1u))) continue;
            const float X = (((float)(x + i) - c.cx) * z) / c.fx;
            const float u = (X - x_min) / cell, w = z / cell;
            if (!(u >= 0.0f && u < fgx && w >= 0.0f && w < fgz)) continue;  // compares on the floats: a huge or NaN coordinate is never converted
            at[i] = (int)floorf(w) * Gx + (int)floorf(u);
            hb[i] = __float_as_uint(h[i]);
        }
    }
    // A fronto-parallel obstacle puts long row segments into few cells, and atomics on one address queue up.  So a thread first joins
    // the runs of equal cells among its quad's pixels (the entry stays on the run's last pixel), then per pixel slot the lanes of the
    // wave that share a cell add and take the maximum once, cell after cell.  Sums and unsigned maxima: the grouping cannot show.
    unsigned n[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) n[i] = at[i] >= 0 ? 1u : 0u;
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        if (at[i] >= 0 && at[i] == at[i - 1]) n[i] += n[i - 1], hb[i] = max(hb[i], hb[i - 1]), at[i - 1] = -1;
    }
    uint32_t *cnt = count ? count + (int64_t)b * Gz * Gx : nullptr, *top = hmax ? hmax + (int64_t)b * Gz * Gx : nullptr;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        u64 left = __ballot(at[i] >= 0);
        while (left != 0) {                                 // (wave-uniform) one trip per distinct cell of the slot
            const int first = __ffsll((long long)left) - 1;
            const int a0 = __shfl(at[i], first, 64);
            const bool mine = at[i] == a0;
            unsigned cn = mine ? n[i] : 0u, m = mine ? hb[i] : 0u;
            for (int o = 32; o > 0; o >>= 1) {
                cn += (unsigned)__shfl_xor((int)cn, o, 64);
                m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
            }
            if (lane == first) {
                if (cnt) atomicAdd(cnt + a0, cn);
                if (top) atomicMax(top + a0, m);
            }
            left &= ~__ballot(mine);
        }
    }
}

int check_hist_args(const char *who, const float *disp, int B, int H, int W, float min_disp, int sub, int nbins)
{
    LWS_CHECK_ARG(disp, "%s: disp is null", who);
    LWS_CHECK_RC(check_image_shape(who, B, H, W, 31));
    LWS_CHECK_ARG(finite_pos(min_disp), "%s: min_disp must be finite and > 0, got %g", who, (double)min_disp);
    LWS_CHECK_ARG(sub >= 1 && sub <= kMaxSub, "%s: sub %d outside 1..%d", who, sub, kMaxSub);
    LWS_CHECK_ARG(nbins >= 1 && nbins <= kMaxBins && nbins <= 256 * sub, "%s: nbins %d outside 1..min(%d, 256 * sub = %d)", who, nbins,
                  kMaxBins, 256 * sub);
    LWS_CHECK_ARG(aligned(disp, 4), "%s: disp is not 4-byte aligned", who);
    return LWS_OK;
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int lws_vdisparity(const float *disp, const uint8_t *mask, int B, int H, int W, float min_disp, int sub, int nbins, uint32_t *hist,
                   void *stream)
{
    LWS_CHECK_RC(check_hist_args("vdisparity", disp, B, H, W, min_disp, sub, nbins));
    LWS_CHECK_ARG(hist, "vdisparity: hist is null");
    LWS_CHECK_ARG(aligned(hist, 4), "vdisparity: hist is not 4-byte aligned");
    const int64_t px = (int64_t)B * H * W;
    const Buf bufs[] = {{hist, 4 * (int64_t)B * H * nbins, "hist"}, {disp, 4 * px, "disp"}, {mask, px, "mask"}};
    LWS_CHECK_RC(check_no_overlap("vdisparity", bufs, 3, 1));
    hipLaunchKernelGGL(k_vdisparity, dim3(H, B), dim3(kThreads), 0, (hipStream_t)stream, disp, mask, H, W, min_disp, sub, nbins, hist);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

int64_t lws_ground_workspace(int B, int H, int nbins)
{
    LWS_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && nbins >= 1 && nbins <= kMaxBins, "ground_workspace: bad shape B=%d H=%d nbins=%d", B, H,
                  nbins);
    return round256((int64_t)B * kWsWords * (int64_t)sizeof(u64));
}

int lws_ground_fit(const float *disp, const uint8_t *mask, const uint32_t *hist, int B, int H, int W, float min_disp, int sub, int nbins,
                   int yh_lo, int yh_hi, int qb_lo, int qb_hi, int tol_bins, int min_score, float tol0, float tol, int iters,
                   void *workspace, float *plane, int32_t *info, void *stream)
{
    LWS_CHECK_RC(check_hist_args("ground_fit", disp, B, H, W, min_disp, sub, nbins));
    LWS_CHECK_ARG(H <= kMaxDim && W <= kMaxDim, "ground_fit: H=%d W=%d exceed %d (the 64-bit sums)", H, W, kMaxDim);
    LWS_CHECK_ARG(hist && workspace && plane && info, "ground_fit: hist, workspace, plane and info must not be null");
    LWS_CHECK_ARG(aligned(hist, 4) && aligned(plane, 4) && aligned(info, 4) && aligned(workspace, 8),
                  "ground_fit: hist / plane / info must be 4-byte, workspace 8-byte aligned");
    LWS_CHECK_ARG(yh_lo >= kMinHorizon && yh_lo <= yh_hi && yh_hi <= H - 2, "ground_fit: yh range %d..%d outside %d..H - 2 = %d", yh_lo,
                  yh_hi, kMinHorizon, H - 2);
    LWS_CHECK_ARG(qb_lo >= 1 && qb_lo <= qb_hi && qb_hi < nbins, "ground_fit: qB range %d..%d outside 1..nbins - 1 = %d", qb_lo, qb_hi,
                  nbins - 1);
    const int64_t nyh = (int64_t)yh_hi - yh_lo + 1, nqb = (int64_t)qb_hi - qb_lo + 1;
    LWS_CHECK_ARG(nyh * nqb <= kMaxCandidates, "ground_fit: %lld x %lld candidates exceed %d", (long long)nyh, (long long)nqb,
                  kMaxCandidates);
    LWS_CHECK_ARG(tol_bins >= 0 && tol_bins <= kMaxTolBins, "ground_fit: tol_bins %d outside 0..%d", tol_bins, kMaxTolBins);
    LWS_CHECK_ARG(min_score >= 0, "ground_fit: min_score %d < 0", min_score);
    LWS_CHECK_ARG(finite_nonneg(tol0) && finite_nonneg(tol), "ground_fit: tol0 and tol must be finite and >= 0, got %g and %g", (double)tol0,
                  (double)tol);
    LWS_CHECK_ARG(iters >= 0 && iters <= kMaxIters, "ground_fit: iters %d outside 0..%d", iters, kMaxIters);
    const int64_t px = (int64_t)B * H * W;
    const Buf bufs[] = {{workspace, round256((int64_t)B * kWsWords * 8), "workspace"}, {plane, 16 * (int64_t)B, "plane"},
                        {info, 32 * (int64_t)B, "info"}, {disp, 4 * px, "disp"}, {mask, px, "mask"},
                        {hist, 4 * (int64_t)B * H * nbins, "hist"}};
    LWS_CHECK_RC(check_no_overlap("ground_fit", bufs, 6, 3));
    u64 *ws = static_cast<u64 *>(workspace);
    hipStream_t st = (hipStream_t)stream;
    const int64_t words = (int64_t)B * kWsWords;
    hipLaunchKernelGGL(k_ground_clear, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, ws, words);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_hough, dim3((unsigned)nyh, (unsigned)((nqb + 63) / 64), B), dim3(kThreads), 0, st, hist, H, nbins,
                       yh_lo, qb_lo, qb_hi, (int)nyh, tol_bins, ws);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ground_seed, dim3(B), dim3(64), 0, st, ws, H, sub, (int)nyh, yh_lo, qb_lo, min_score, plane, info);
    LWS_LAUNCH_CHECK();
    for (int p = 0; p <= iters; ++p) {                      // a fixed list: iters is no convergence test
        const double tol256 = (double)(p == 0 ? tol0 : tol) * 256.0;
        hipLaunchKernelGGL(k_fit_accum, dim3(H, B), dim3(kThreads), 0, st, disp, mask, H, W, min_disp, sub, nbins, tol256, ws);
        LWS_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_fit_solve, dim3(B), dim3(64), 0, st, ws, plane, info);
        LWS_LAUNCH_CHECK();
    }
    return LWS_OK;
}

int lws_ground_classify(const float *disp, const uint8_t *mask, const float *cam, const float *plane, int B, int H, int W, float min_disp,
                        float max_depth, float ground_tol, float max_height, float *height, uint8_t *codes, int64_t *counts, void *stream)
{
    LWS_CHECK_RC(check_geometry_args("ground_classify", disp, B, H, W, min_disp, max_depth));
    LWS_CHECK_ARG(cam && plane, "ground_classify: cam and plane must not be null");
    LWS_CHECK_ARG(height || codes, "ground_classify: no output requested (height and codes are both null)");
    LWS_CHECK_ARG(aligned(cam, 4) && aligned(plane, 4) && aligned(height, 4) && aligned(counts, 8),
                  "ground_classify: cam / plane / height must be 4-byte, counts 8-byte aligned");
    LWS_CHECK_ARG(finite_nonneg(ground_tol) && finite_nonneg(max_height) && ground_tol <= max_height,
                  "ground_classify: need finite 0 <= ground_tol <= max_height, got %g and %g", (double)ground_tol, (double)max_height);
    const int64_t px = (int64_t)B * H * W;
    const Buf bufs[] = {{height, 4 * px, "height"}, {codes, px, "codes"}, {counts, 48 * (int64_t)B, "counts"}, {disp, 4 * px, "disp"},
                        {mask, px, "mask"}, {cam, 20 * (int64_t)B, "cam"}, {plane, 16 * (int64_t)B, "plane"}};
    LWS_CHECK_RC(check_no_overlap("ground_classify", bufs, 7, 3));
    hipStream_t st = (hipStream_t)stream;
    if (counts) {
        const int64_t words = 6 * (int64_t)B;
        hipLaunchKernelGGL(k_ground_clear, dim3((unsigned)((words + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                           reinterpret_cast<u64 *>(counts), words);
        LWS_LAUNCH_CHECK();
    }
    const int nq = (W + 3) / 4;
    const int64_t n = (int64_t)H * nq;
    hipLaunchKernelGGL(k_classify, dim3((unsigned)((n + kThreads - 1) / kThreads), B), dim3(kThreads), 0, st, disp, mask, cam, plane, H, W, nq,
                       min_disp, max_depth, ground_tol, max_height, height, codes, reinterpret_cast<u64 *>(counts));
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

int lws_bev_grid(const float *disp, const float *cam, const uint8_t *codes, const float *height, int B, int H, int W, float min_disp,
                 float max_depth, int code_bits, float x_min, float cell, int Gx, int Gz, uint32_t *count, float *hmax, void *stream)
{
    LWS_CHECK_RC(check_geometry_args("bev_grid", disp, B, H, W, min_disp, max_depth));
    LWS_CHECK_ARG(cam && codes, "bev_grid: cam and codes must not be null");
    LWS_CHECK_ARG(count || hmax, "bev_grid: no output requested (count and hmax are both null)");
    LWS_CHECK_ARG(!hmax || height, "bev_grid: hmax needs height");
    LWS_CHECK_ARG(aligned(cam, 4) && aligned(height, 4) && aligned(count, 4) && aligned(hmax, 4),
                  "bev_grid: cam / height / count / hmax must be 4-byte aligned");
    LWS_CHECK_ARG(code_bits >= 0 && code_bits < 64, "bev_grid: code_bits %d outside 0..63", code_bits);
    LWS_CHECK_ARG(!hmax || (code_bits & 0x33) == 0,
                  "bev_grid: code_bits %d selects a code other than 2 and 3, whose heights are not positive; hmax cannot be requested", code_bits);
    LWS_CHECK_ARG(x_min >= -3.4028234663852886e38f && x_min <= 3.4028234663852886e38f, "bev_grid: x_min must be finite, got %g", (double)x_min);
    LWS_CHECK_ARG(finite_pos(cell), "bev_grid: cell must be finite and > 0, got %g", (double)cell);
    LWS_CHECK_ARG(Gx >= 1 && Gx <= kMaxGrid && Gz >= 1 && Gz <= kMaxGrid, "bev_grid: grid Gx=%d Gz=%d outside 1..%d", Gx, Gz, kMaxGrid);
    const int64_t px = (int64_t)B * H * W, cells = (int64_t)B * Gz * Gx;
    const Buf bufs[] = {{count, 4 * cells, "count"}, {hmax, 4 * cells, "hmax"}, {disp, 4 * px, "disp"}, {cam, 20 * (int64_t)B, "cam"},
                        {codes, px, "codes"}, {height, 4 * px, "height"}};
    LWS_CHECK_RC(check_no_overlap("bev_grid", bufs, 6, 2));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_bev_clear, dim3((unsigned)((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, count,
                       reinterpret_cast<uint32_t *>(hmax), cells);
    LWS_LAUNCH_CHECK();
    const int nq = (W + 3) / 4;
    const int64_t n = (int64_t)H * nq;
    hipLaunchKernelGGL(k_bev_scatter, dim3((unsigned)((n + kThreads - 1) / kThreads), B), dim3(kThreads), 0, st, disp, cam, codes, height, H, W,
                       nq, min_disp, max_depth, (unsigned)code_bits, x_min, cell, Gx, Gz, count, reinterpret_cast<uint32_t *>(hmax));
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // extern "C"
