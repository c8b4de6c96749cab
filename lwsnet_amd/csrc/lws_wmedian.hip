// Edge-aware weighted median filter of a disparity map: per pixel the lower weighted median of the valid disparities in a
// (2r + 1)^2 window, the integer weights looked up by the colour distance to the centre pixel in the left image.  Contract:
// include/lwsnet_hip.h, lws_wmedian_filter; tests/wmedian_reference.py restates every output bit for bit.
//
// Launches (a fixed list: it depends on the argument `counts`, never on the data; nothing is read back):
//   k_wm_zero     (counts != NULL) counts[B][2] = 0
//   k_wm_filter   one workgroup of 256 threads per 16 x 64 tile of one image, templated on the radius R and on GUIDED (rgb given)
//
// k_wm_filter stages the tile and its halo of R pixels in LDS -- the disparities with every non-candidate (invalid pixel, pixel
// outside the image) replaced by a NaN, the guide as one 32-bit word 0x00bbggrr per pixel -- and the weight table as 766 uint16.
// Thread t owns column t % 64 of the tile and the rows t / 64 + 4k, k < 4: every LDS read of a wave is 64 consecutive words of
// one row (ds_read_b32 banks per 32 lanes: conflict-free), every store of a wave one 256-byte run of a row.  Per pixel:
//   gather   the n = (2R + 1)^2 window values d_j and weights w_j into registers (both loops unrolled, so the arrays never leave the
//            register file); w_j = wlut[v_sad_u8(guide_p, guide_j)], or 1 without a guide, forced to 0 where d_j is the NaN marker:
//            T = sum w_j, n(p) = #{w_j > 0}
//   count    for every window position i (row loop rolled, column loop unrolled; v_i re-read from LDS): le_i = sum_j w_j [d_j <= v_i]
//            -- a compare, a select and an add per step, branch-free; the answer is min{v_i : 2 le_i >= T}.  A NaN v_i compares
//            false everywhere (le = 0 < T), a weight-0 value can only tie with or exceed a weighted value with the same le, so
//            neither changes the minimum.  Float compares and integer sums only: no order of visiting can show.
// Cost: n^2 steps per pixel (2401 at R = 3), about 3 VALU instructions each with a guide and 2 without; the staging moves 8
// bytes per pixel once, so the kernel is bound by the vector ALU, not by memory or LDS.  Bisecting on the bit pattern instead
// takes 31 passes of n steps with a loop-carried dependency -- 1519 steps at R = 3, no cheaper at R <= 2 (775 against 625, 279
// against 81) -- so the counting form is the one shipped.  Rows are staged with scalar loads: the halo starts R pixels left of the
// tile, W is arbitrary, and the loads are ~1 % of the kernel's work.
// The counts are summed per wave by shuffles, per workgroup in LDS, and added to counts[b] with one 64-bit integer atomic per
// workgroup and counter: integer adds, so their order cannot show.  0 bytes of scratch.
#include "lws_common.h"
#include "lws_opkit.h"

namespace lws {

namespace {

using namespace opkit;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTH = 16, kTW = 64;                           // the output tile
constexpr int kRowsPerThread = kTH / kWaves;                // 4
constexpr int kLut = 766;                                   // s = |dr| + |dg| + |db| in 0 .. 765
static_assert(kTW == 64 && kTH % kWaves == 0, "a wave owns one row of the tile at a time");

__device__ __forceinline__ bool wm_valid(float d, bool ok) { return ok && __builtin_isfinite(d) && d > 0.0f; }

// grid (1, B): counts[b][0..1] = 0
__global__ void k_wm_zero(int64_t *__restrict__ counts)
{
    if (threadIdx.x < 2) counts[2 * (int64_t)blockIdx.y + threadIdx.x] = 0;
}

// grid (ntx * nty, B), 256 threads.  LDS at R = 3: 22 x 70 floats + 22 x 70 words + 766 uint16 = 13.9 KiB.
template <int R, bool GUIDED>
__global__ __launch_bounds__(kThreads) void k_wm_filter(const float *__restrict__ disp, const uint8_t *__restrict__ mask,
                                                       const uint8_t *__restrict__ rgb, const uint16_t *__restrict__ wlut, int H, int W,
                                                       int ntx, int fill_min, float *__restrict__ out,
                                                       unsigned long long *__restrict__ counts)
{
    constexpr int D = 2 * R + 1, N = D * D;
    constexpr int kPitch = kTW + 2 * R, kRows = kTH + 2 * R, kHalo = kPitch * kRows;
    __shared__ float s_d[kHalo];
    __shared__ unsigned s_g[GUIDED ? kHalo : 1];
    __shared__ uint16_t s_w[GUIDED ? kLut + 2 : 2];
    __shared__ int s_n[kWaves][2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.y;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * kTH, x0 = tx * kTW;
    const int64_t img = (int64_t)b * H * W;
    const float nan = __builtin_nanf("");

    for (int i = t; i < kHalo; i += kThreads) {
        const int ry = i / kPitch, rx = i - ry * kPitch;
        const int y = y0 - R + ry, x = x0 - R + rx;
        float d = nan;
        unsigned g = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int64_t p = img + (int64_t)y * W + x;
            const float v = disp[p];
            d = wm_valid(v, mask ? mask[p] == 1 : true) ? v : nan;
            if (GUIDED) g = (unsigned)rgb[3 * p] | ((unsigned)rgb[3 * p + 1] << 8) | ((unsigned)rgb[3 * p + 2] << 16);
        }
        s_d[i] = d;
        if (GUIDED) s_g[i] = g;
    }
    if (GUIDED)
        for (int i = t; i < kLut; i += kThreads) s_w[i] = wlut[i];
    __syncthreads();

    int n_changed = 0, n_filled = 0;
    const int x = x0 + lane;
#pragma unroll 1
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int ly = wave + kWaves * k, y = y0 + ly;
        if (y >= H || x >= W) continue;
        const float *win = s_d + ly * kPitch + lane;        // the window's top-left corner; the centre is win[R * kPitch + R]
        float d[N];
        int w[N];
        int T = 0, n = 0;
#pragma unroll
        for (int dy = 0; dy < D; ++dy)
#pragma unroll
            for (int dx = 0; dx < D; ++dx) {
                const int j = dy * D + dx;
                d[j] = win[dy * kPitch + dx];
                if (GUIDED) {
                    const unsigned *gw = s_g + ly * kPitch + lane;
                    const unsigned s = __builtin_amdgcn_sad_u8(gw[R * kPitch + R], gw[dy * kPitch + dx], 0u);
                    w[j] = __builtin_isnan(d[j]) ? 0 : (int)s_w[s];
                } else {
                    w[j] = __builtin_isnan(d[j]) ? 0 : 1;   // (only T and n see it: a NaN d_j never passes the compare below)
                }
                T += w[j];
                n += w[j] > 0 ? 1 : 0;
            }
        const float inf = __builtin_inff();
        float m = inf;
#pragma unroll 1
        for (int iy = 0; iy < D; ++iy) {
#pragma unroll
            for (int ix = 0; ix < D; ++ix) {
                const float v = win[iy * kPitch + ix];
                int le = 0;
#pragma unroll
                for (int j = 0; j < N; ++j) le += d[j] <= v ? (GUIDED ? w[j] : 1) : 0;
                const float c = 2 * le >= T ? v : inf;      // a NaN v: le = 0, and T > 0 wherever m is used
                m = c < m ? c : m;
            }
        }
        const float dp = d[R * D + R];
        const bool valid = !__builtin_isnan(dp);
        const bool fill = !valid && fill_min > 0 && n >= fill_min;
        const float o = valid ? (T == 0 ? dp : m) : (fill ? m : 0.0f);
        out[img + (int64_t)y * W + x] = o;
        n_changed += valid && __float_as_uint(o) != __float_as_uint(dp) ? 1 : 0;
        n_filled += fill ? 1 : 0;
    }
    if (counts) {                                           // (uniform)
        int n[2] = {n_changed, n_filled};
        wave_sum_n(n);
        if (lane == 0) s_n[wave][0] = n[0], s_n[wave][1] = n[1];
        __syncthreads();
        if (t < 2) {
            const int v = sum4(s_n[0][t], s_n[1][t], s_n[2][t], s_n[3][t]);
            if (v) atomicAdd(counts + 2 * (int64_t)b + t, (unsigned long long)v);
        }
    }
}

template <int R>
void launch(bool guided, dim3 grid, hipStream_t st, const float *disp, const uint8_t *mask, const uint8_t *rgb, const uint16_t *wlut,
            int H, int W, int ntx, int fill_min, float *out, unsigned long long *counts)
{
    if (guided)
        hipLaunchKernelGGL((k_wm_filter<R, true>), grid, dim3(kThreads), 0, st, disp, mask, rgb, wlut, H, W, ntx, fill_min, out, counts);
    else
        hipLaunchKernelGGL((k_wm_filter<R, false>), grid, dim3(kThreads), 0, st, disp, mask, rgb, wlut, H, W, ntx, fill_min, out, counts);
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int lws_wmedian_filter(const float *disp, const uint8_t *mask, const uint8_t *rgb, const uint16_t *wlut, int B, int H, int W, int radius,
                       int fill_min, float *out, int64_t *counts, void *stream)
{
    LWS_CHECK_RC(check_image_shape("wmedian_filter", B, H, W, 31));
    LWS_CHECK_ARG(disp && out, "wmedian_filter: disp and out must not be null");
    LWS_CHECK_ARG(radius >= 1 && radius <= 3, "wmedian_filter: radius must be 1, 2 or 3, got %d", radius);
    LWS_CHECK_ARG(fill_min >= 0, "wmedian_filter: fill_min must be >= 0, got %d", fill_min);
    LWS_CHECK_ARG(!rgb || wlut, "wmedian_filter: rgb needs wlut (766 uint16 weights in device memory)");
    LWS_CHECK_ARG(aligned(disp, 4) && aligned(out, 4) && aligned(counts, 8) && (!rgb || aligned(wlut, 2)),
                  "wmedian_filter: disp / out must be 4-byte, counts 8-byte, wlut 2-byte aligned");
    const int64_t px = (int64_t)B * H * W;
    // out and counts are written; an overlap of either with anything else is an error (a neighbourhood of disp is read, so out may
    // not be disp either).  wlut is ignored without rgb.
    const Buf bufs[] = {{out, 4 * px, "out"}, {counts, 16 * (int64_t)B, "counts"}, {disp, 4 * px, "disp"},
                        {mask, px, "mask"},   {rgb, 3 * px, "rgb"},                {rgb ? wlut : nullptr, 2 * kLut, "wlut"}};
    LWS_CHECK_RC(check_no_overlap("wmedian_filter", bufs, 6, 2));

    hipStream_t st = (hipStream_t)stream;
    if (counts) {
        hipLaunchKernelGGL(k_wm_zero, dim3(1, B), dim3(64), 0, st, counts);
        LWS_LAUNCH_CHECK();
    }
    const int ntx = (W + kTW - 1) / kTW, nty = (H + kTH - 1) / kTH;
    const dim3 grid((unsigned)((int64_t)ntx * nty), B);
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counts);
    if (radius == 1)
        launch<1>(rgb != nullptr, grid, st, disp, mask, rgb, wlut, H, W, ntx, fill_min, out, cnt);
    else if (radius == 2)
        launch<2>(rgb != nullptr, grid, st, disp, mask, rgb, wlut, H, W, ntx, fill_min, out, cnt);
    else
        launch<3>(rgb != nullptr, grid, st, disp, mask, rgb, wlut, H, W, ntx, fill_min, out, cnt);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // extern "C"
