// Photometric reprojection error of disparity maps (Godard et al.): the right image is warped into the left view with the map and
// compared with the left image by L1 and a 3 x 3 SSIM term.  A score that needs no ground truth: a correct map reproduces the
// left image.  Contract: include/lwsnet_hip.h, lws_photometric; tests/photometric_reference.py restates every output bit for bit.
//
// Launches (a fixed list: two kernels, nothing is read back, so the call is two nodes of a captured graph):
//   k_photo_zero    sums[nmaps][B][4] = 0
//   k_photometric   one workgroup of 256 threads per 16 x 64 tile of one image and map
// sums is cleared by a kernel, as lws_wmedian_filter clears its counts, not by hipMemsetAsync: a captured memset node of the HIP
// runtime this was developed on fills its destination with stale kernel-argument words from the second replay on, once other
// kernels have run in between (the first replay is right); a kernel node replays correctly every time.
//
// k_photometric stages the tile and its halo of one pixel (18 x 66) in LDS: per pixel the warped colour as three floats and one
// word bb << 16 | gg << 8 | rr, the left pixel, with the warpable flag in bit 24 (a pixel outside the image: 0).  The two right
// taps of a pixel are gathered from global memory as bytes: 6 contiguous bytes when i1 = i0 + 1, and with a smooth map neighbouring lanes
// read neighbouring bytes (the argument of k_rectify_pair's gather).  Nothing assumes an aligned row: the pitch is 3 W bytes.  The
// staging thread of an interior pixel also stores its warped colour.
// Compute: wave w owns the tile's rows 4w .. 4w + 3, lane l its column l.  A thread walks down the six halo rows its strip
// touches, forms the horizontal sums of the five quantities per channel once per row (the contract sums horizontally first for
// this) and keeps the last three rows' sums in registers; every LDS read of a wave is 64 consecutive words of one row
// (conflict-free), every store one run of a row.
// The four sums of a tile are integers below 2^30 (1024 pixels of at most 2^20 each): 32-bit wave sums by shuffles, the four
// waves through LDS, then one 64-bit integer atomic per workgroup and counter into the cleared sums.  Integer adds, so their order
// cannot show: an image gives the same bytes in any batch, at any position, on every run.  No float atomics, no workspace, 0
// bytes of scratch.
#include "lws_common.h"
#include "lws_opkit.h"

namespace lws {

namespace {

using namespace opkit;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTH = 16, kTW = 64;                           // the output tile
constexpr int kStrip = kTH / kWaves;                        // 4 rows per wave
constexpr int kPitch = kTW + 2, kRows = kTH + 2, kHalo = kPitch * kRows;
constexpr unsigned kFlag = 1u << 24;
constexpr float kC1 = 6.5025f, kC2 = 58.5225f;              // (0.01 * 255)^2, (0.03 * 255)^2
static_assert(kTW == 64 && kTH % kWaves == 0, "a wave owns one row of the tile at a time");

struct PhotoMaps {                                          // the nmaps maps of one call, by value in the kernel arguments
    const float *disp[4];
    const uint8_t *mask[4];
    float *err[4];
    uint8_t *scored[4], *warped[4];
};

// The horizontal sums of one halo row at the columns c - 1, c, c + 1: per channel {x, y, x*x, y*y, x*y}, x the left and y the
// warped value; the flags of the three pixels and-ed.
struct RowSums {
    float v[15];
    bool ok;
};

__device__ __forceinline__ void quantities(unsigned l, float w0, float w1, float w2, float (&q)[15])
{
    const float x[3] = {(float)(l & 255u), (float)((l >> 8) & 255u), (float)((l >> 16) & 255u)}, y[3] = {w0, w1, w2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        q[5 * c] = x[c];
        q[5 * c + 1] = y[c];
        q[5 * c + 2] = x[c] * x[c];
        q[5 * c + 3] = y[c] * y[c];
        q[5 * c + 4] = x[c] * y[c];
    }
}

__device__ __forceinline__ RowSums row_sums(const unsigned *sl, const float *sw, int at)
{
    float a[15], b[15], c[15];
    const unsigned l0 = sl[at], l1 = sl[at + 1], l2 = sl[at + 2];
    quantities(l0, sw[at], sw[kHalo + at], sw[2 * kHalo + at], a);
    quantities(l1, sw[at + 1], sw[kHalo + at + 1], sw[2 * kHalo + at + 1], b);
    quantities(l2, sw[at + 2], sw[kHalo + at + 2], sw[2 * kHalo + at + 2], c);
    RowSums r;
#pragma unroll
    for (int j = 0; j < 15; ++j) r.v[j] = (a[j] + b[j]) + c[j];
    r.ok = (l0 & l1 & l2 & kFlag) != 0;
    return r;
}

// n words of sums = 0
__global__ void k_photo_zero(unsigned long long *__restrict__ sums, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sums[i] = 0;
}

// grid (ntx * nty, B * nmaps), 256 threads; blockIdx.y = s * B + b.  LDS: 18 x 66 x (3 floats + 1 word) = 18.6 KiB.
__global__ __launch_bounds__(kThreads) void k_photometric(PhotoMaps m, const uint8_t *__restrict__ left, const uint8_t *__restrict__ right,
                                                         const uint8_t *__restrict__ rvalid, int B, int H, int W, int ntx, float alpha,
                                                         unsigned long long *__restrict__ sums)
{
    __shared__ float s_w[3 * kHalo];
    __shared__ unsigned s_l[kHalo];
    __shared__ unsigned s_n[kWaves][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int s = blockIdx.y / B, b = blockIdx.y - s * B;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * kTH, x0 = tx * kTW;
    const int64_t img = (int64_t)b * H * W;
    const float *disp = m.disp[s];
    const uint8_t *mask = m.mask[s];
    float *err = m.err[s];
    uint8_t *scored = m.scored[s], *warped = m.warped[s];
    const float wmax = (float)(W - 1);

    // ---- stage the halo: warp every pixel of it that lies inside the image ----
    for (int i = t; i < kHalo; i += kThreads) {
        const int ry = i / kPitch, rx = i - ry * kPitch;
        const int y = y0 - 1 + ry, x = x0 - 1 + rx;
        float w[3] = {0.0f, 0.0f, 0.0f};
        unsigned l = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int64_t row = img + (int64_t)y * W, p = row + x;
            const float d = disp[p];
            const float tt = (float)x - d;
            bool ok = !__builtin_isnan(d) && tt >= 0.0f && tt <= wmax;
            const uint8_t *lp = left + 3 * p;
            l = (unsigned)lp[0] | ((unsigned)lp[1] << 8) | ((unsigned)lp[2] << 16);
            if (ok) {
                const float fl = floorf(tt);
                const int i0 = (int)fl, i1 = i0 + 1 < W ? i0 + 1 : W - 1;
                if (rvalid) ok = rvalid[row + i0] == 1 && rvalid[row + i1] == 1;
                if (ok) {
                    const float a = tt - fl;
                    const uint8_t *r0 = right + 3 * (row + i0), *r1 = right + 3 * (row + i1);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float v0 = (float)r0[c], v1 = (float)r1[c];
                        w[c] = v0 + a * (v1 - v0);
                    }
                    l |= kFlag;
                }
            }
            if (warped && ry >= 1 && ry <= kTH && rx >= 1 && rx <= kTW) {      // an unwarpable pixel: w = 0
                uint8_t *wp = warped + 3 * p;
                wp[0] = (uint8_t)rintf(w[0]);
                wp[1] = (uint8_t)rintf(w[1]);
                wp[2] = (uint8_t)rintf(w[2]);
            }
        }
        s_w[i] = w[0];
        s_w[kHalo + i] = w[1];
        s_w[2 * kHalo + i] = w[2];
        s_l[i] = l;
    }
    __syncthreads();

    // ---- the strip: halo rows 4 wave .. 4 wave + 5 at the halo columns lane .. lane + 2 ----
    const int x = x0 + lane;
    const float beta = 1.0f - alpha;
    unsigned n[4] = {0u, 0u, 0u, 0u};                       // count, sum q(pe), sum q(l1), sum q(ds)
    RowSums r0 = row_sums(s_l, s_w, (kStrip * wave) * kPitch + lane);
    RowSums r1 = row_sums(s_l, s_w, (kStrip * wave + 1) * kPitch + lane);
#pragma unroll
    for (int k = 0; k < kStrip; ++k) {
        const int ly = kStrip * wave + k, y = y0 + ly;
        const RowSums r2 = row_sums(s_l, s_w, (ly + 2) * kPitch + lane);
        const int at = (ly + 1) * kPitch + lane + 1;        // the pixel itself in the halo
        const unsigned l = s_l[at];
        const float lc[3] = {(float)(l & 255u), (float)((l >> 8) & 255u), (float)((l >> 16) & 255u)};
        const float wc[3] = {s_w[at], s_w[kHalo + at], s_w[2 * kHalo + at]};
        const float l1 = (((fabsf(lc[0] - wc[0]) + fabsf(lc[1] - wc[1])) + fabsf(lc[2] - wc[2])) / 3.0f) / 255.0f;
        float dsc[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float S[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) S[j] = (r0.v[5 * c + j] + r1.v[5 * c + j]) + r2.v[5 * c + j];
            const float mx = S[0] / 9.0f, my = S[1] / 9.0f;
            const float vx = S[2] / 9.0f - mx * mx, vy = S[3] / 9.0f - my * my, cxy = S[4] / 9.0f - mx * my;
            const float num = ((2.0f * mx) * my + kC1) * (2.0f * cxy + kC2);
            const float den = ((mx * mx + my * my) + kC1) * ((vx + vy) + kC2);
            dsc[c] = fminf(fmaxf((1.0f - num / den) * 0.5f, 0.0f), 1.0f);
        }
        const float ds = ((dsc[0] + dsc[1]) + dsc[2]) / 3.0f;
        const float pe = alpha * ds + beta * l1;
        if (y < H && x < W) {
            const int64_t p = img + (int64_t)y * W + x;
            const bool sc = r0.ok && r1.ok && r2.ok && (mask ? mask[p] == 1 : true);
            if (err) err[p] = sc ? pe : 0.0f;
            if (scored) scored[p] = sc ? 1 : 0;
            if (sc) {
                n[0] += 1u;
                n[1] += (unsigned)(int)rintf(pe * 1048576.0f);
                n[2] += (unsigned)(int)rintf(l1 * 1048576.0f);
                n[3] += (unsigned)(int)rintf(ds * 1048576.0f);
            }
        }
        r0 = r1;
        r1 = r2;
    }

    wave_sum_n(n);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s_n[wave][j] = n[j];
    }
    __syncthreads();
    if (t < 4) {
        const unsigned v = sum4(s_n[0][t], s_n[1][t], s_n[2][t], s_n[3][t]);
        if (v) atomicAdd(sums + 4 * (int64_t)blockIdx.y + t, (unsigned long long)v);
    }
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int lws_photometric(const float *const disp[4], int nmaps, const uint8_t *left, const uint8_t *right, const uint8_t *const mask[4],
                    const uint8_t *rvalid, int B, int H, int W, float alpha, float *const err[4], uint8_t *const scored[4],
                    uint8_t *const warped[4], int64_t *sums, void *stream)
{
    LWS_CHECK_ARG(disp && left && right && sums, "photometric: disp, left, right and sums must not be null");
    LWS_CHECK_ARG(nmaps >= 1 && nmaps <= 4, "photometric: nmaps %d outside 1..4", nmaps);
    LWS_CHECK_ARG(alpha >= 0.0f && alpha <= 1.0f, "photometric: alpha must be in [0, 1], got %g", (double)alpha);     // (false for NaN)
    LWS_CHECK_RC(check_image_shape("photometric", B, H, W, 31));
    LWS_CHECK_ARG((int64_t)B * nmaps <= 65535, "photometric: B * nmaps = %d * %d exceeds 65535", B, nmaps);
    static const char *const names[5][4] = {{"err[0]", "err[1]", "err[2]", "err[3]"},
                                            {"scored[0]", "scored[1]", "scored[2]", "scored[3]"},
                                            {"warped[0]", "warped[1]", "warped[2]", "warped[3]"},
                                            {"disp[0]", "disp[1]", "disp[2]", "disp[3]"},
                                            {"mask[0]", "mask[1]", "mask[2]", "mask[3]"}};
    const int64_t px = (int64_t)B * H * W;
    PhotoMaps m = {};
    Buf bufs[24];
    int n = 0;
    for (int s = 0; s < nmaps; ++s) {
        LWS_CHECK_ARG(disp[s], "photometric: disp[%d] is null", s);
        m.disp[s] = disp[s];
        m.mask[s] = mask ? mask[s] : nullptr;
        m.err[s] = err ? err[s] : nullptr;
        m.scored[s] = scored ? scored[s] : nullptr;
        m.warped[s] = warped ? warped[s] : nullptr;
        LWS_CHECK_ARG(aligned(m.disp[s], 4) && aligned(m.err[s], 4), "photometric: disp[%d] / err[%d] must be 4-byte aligned", s, s);
    }
    LWS_CHECK_ARG(aligned(sums, 8), "photometric: sums must be 8-byte aligned");
    // the written buffers first: each against every buffer behind it; the inputs may overlap one another as they like
    for (int s = 0; s < nmaps; ++s) bufs[n++] = Buf{m.err[s], 4 * px, names[0][s]};
    for (int s = 0; s < nmaps; ++s) bufs[n++] = Buf{m.scored[s], px, names[1][s]};
    for (int s = 0; s < nmaps; ++s) bufs[n++] = Buf{m.warped[s], 3 * px, names[2][s]};
    const int64_t sums_bytes = (int64_t)nmaps * B * 4 * (int64_t)sizeof(int64_t);
    bufs[n++] = Buf{sums, sums_bytes, "sums"};
    const int n_written = n;
    for (int s = 0; s < nmaps; ++s) bufs[n++] = Buf{m.disp[s], 4 * px, names[3][s]};
    for (int s = 0; s < nmaps; ++s) bufs[n++] = Buf{m.mask[s], px, names[4][s]};
    bufs[n++] = Buf{left, 3 * px, "left"};
    bufs[n++] = Buf{right, 3 * px, "right"};
    bufs[n++] = Buf{rvalid, px, "rvalid"};
    LWS_CHECK_RC(check_no_overlap("photometric", bufs, n, n_written));

    hipStream_t st = (hipStream_t)stream;
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(sums);
    const int n_sums = 4 * B * nmaps;
    hipLaunchKernelGGL(k_photo_zero, dim3(cdiv(n_sums, kThreads)), dim3(kThreads), 0, st, cnt, n_sums);
    LWS_LAUNCH_CHECK();
    const int ntx = (W + kTW - 1) / kTW, nty = (H + kTH - 1) / kTH;
    hipLaunchKernelGGL(k_photometric, dim3((unsigned)((int64_t)ntx * nty), (unsigned)(B * nmaps)), dim3(kThreads), 0, st, m, left, right,
                       rvalid, B, H, W, ntx, alpha, cnt);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // extern "C"
