// Per-pixel confidence and disparity sigma of a stage's soft-argmin (HBM-bound, float32, -ffp-contract=off).
//
// Arithmetic contract (include/lwsnet_hip.h, lws_softargmin_conf): the softmax over the D hypotheses is k_softargmin's -- both call the
// same functions of lws_device_math.h; `peak` is its mass within one hypothesis step of the regressed value, `sig` its standard
// deviation, and the full-resolution maps are k_upsample_add's resize of the two.  One IEEE float32 operation per step.
#include "lws_common.h"
#include "lws_device_math.h"
#include "lws_opkit.h"

namespace lws {

// d, peak and sig of one low-resolution pixel: the shared softmax and expectation, then the moment pass over the same p_k.  DT =
// compile-time D: the p_k stay in registers, so the moment pass divides nothing again.  DT = 0: the generic fallback re-reads the
// costs through L1 and recomputes e_k (a pure function of its input, so the same bits).
template <int DT>
__device__ __forceinline__ void conf_pixel(const float *c, int64_t plane, int D, float start, float &d, float &peak, float &sig)
{
    float acc, pk = 0.0f, var = 0.0f;
    if constexpr (DT > 0) {
        float v[DT];
        acc = softargmin_regs<DT>(c, plane, start, v);
#pragma unroll
        for (int k = 0; k < DT; ++k) {
            const float t = (start + (float)k) - acc;
            if (fabsf(t) <= 1.0f) pk = pk + v[k];
            var = var + v[k] * (t * t);
        }
    } else {
        float m, S;
        softmax_max_sum(c, plane, D, m, S);
        acc = 0.0f;
        for (int k = 0; k < D; ++k) {
            const float p = lws_expf(-c[(int64_t)k * plane] - m) / S;
            acc = acc + p * (start + (float)k);
        }
        for (int k = 0; k < D; ++k) {
            const float p = lws_expf(-c[(int64_t)k * plane] - m) / S;
            const float t = (start + (float)k) - acc;
            if (fabsf(t) <= 1.0f) pk = pk + p;
            var = var + p * (t * t);
        }
    }
    d = acc;
    peak = pk;
    sig = sqrtf(var);
}

// A workgroup computes peak and sig of a TY x TX low-resolution tile plus its one-pixel ring into LDS (threads 0 .. HY*HX-1, one
// pixel each), then writes the full-resolution conf / sigma pixels the tile determines.
//   exact (H % h == 0 and W % w == 0): those are the (TY*s) x (TX*s) block under the tile, whose taps lie in tile + ring
//     (k_softargmin_upsample's map; aligned rows of whole cache lines).
//   otherwise (H or W = 8k-1): a full-resolution pixel belongs to the tile that holds its upper-left tap (y0, x0) -- src_index is
//     monotone, so every pixel has exactly one owner and its other taps (y0 + 1, x0 + 1 at most) are in the ring.  The workgroup
//     walks a candidate range that is one pixel wider than the exact pre-image of the tile and skips what it does not own.
// No atomics, no workspace: a pixel's bytes depend on its image's costs alone.
template <int DT, int TY, int TX>
__global__ __launch_bounds__(256) void k_softargmin_conf(const float *__restrict__ cost, float *__restrict__ disp_low,
                                                         float *__restrict__ peak_low, float *__restrict__ sigma_low,
                                                         float *__restrict__ conf, float *__restrict__ sigma, int D, int h, int w,
                                                         int H, int W, float start, float mul_a, float mul_b, float ioff, int exact)
{
    constexpr int HY = TY + 2, HX = TX + 2;
    __shared__ float sPeak[HY * HX], sSig[HY * HX];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int ly0 = blockIdx.y * TY, lx0 = blockIdx.x * TX;
    const int64_t plane = (int64_t)h * w;
    if (tid < HY * HX) {
        const int hy = tid / HX, hx = tid - hy * HX;
        const int y = ly0 + hy - 1, x = lx0 + hx - 1;
        float d = 0.0f, pk = 0.0f, sg = 0.0f;
        if (y >= 0 && y < h && x >= 0 && x < w) {
            conf_pixel<DT>(cost + (int64_t)b * D * plane + (int64_t)y * w + x, plane, D, start, d, pk, sg);
            if (hy >= 1 && hy <= TY && hx >= 1 && hx <= TX) {
                const int64_t o = (int64_t)b * plane + (int64_t)y * w + x;
                if (disp_low != nullptr) disp_low[o] = d;
                if (peak_low != nullptr) peak_low[o] = pk;
                if (sigma_low != nullptr) sigma_low[o] = sg;
            }
        }
        sPeak[tid] = pk;
        sSig[tid] = sg;
    }
    __syncthreads();
    if (conf == nullptr && sigma == nullptr) return;
    int ya, yb, xa, xb;        // candidate rows [ya, yb) and columns [xa, xb)
    if (exact) {
        const int sy = H / h, sx = W / w;
        ya = ly0 * sy;
        yb = ya + TY * sy;
        xa = lx0 * sx;
        xb = xa + TX * sx;
    } else {
        // src(y) in [ly0, ly0 + TY)  <=>  y in [(ly0 + off) H/h - off, (ly0 + TY + off) H/h - off), off in {0, 0.5}: bracketed in
        // integers with one pixel of slack; the first tile also owns what src_index clamps to 0, the last what it clamps to h - 1
        ya = (int)(((int64_t)ly0 * H) / h) - 1;
        yb = ly0 + TY >= h ? H : (int)(((int64_t)(2 * (ly0 + TY) + 1) * H + 2 * h - 1) / (2 * h)) + 1;
        xa = (int)(((int64_t)lx0 * W) / w) - 1;
        xb = lx0 + TX >= w ? W : (int)(((int64_t)(2 * (lx0 + TX) + 1) * W + 2 * w - 1) / (2 * w)) + 1;
        ya = ya < 0 ? 0 : ya;
        xa = xa < 0 ? 0 : xa;
    }
    yb = yb < H ? yb : H;
    xb = xb < W ? xb : W;
    const int oh = yb - ya, ow = xb - xa;
    if (oh <= 0 || ow <= 0) return;
    const float rh = (float)h / (float)H, rw = (float)w / (float)W;
    for (int i = tid; i < oh * ow; i += 256) {
        const int oy = i / ow, ox = i - oy * ow;
        const int y = ya + oy, x = xa + ox;
        int y0, y1, x0, x1;
        float hy0, hy1, wx0, wx1;
        src_index(y, rh, h, y0, y1, hy0, hy1, ioff);
        src_index(x, rw, w, x0, x1, wx0, wx1, ioff);
        if (!exact && (y0 < ly0 || y0 >= ly0 + TY || x0 < lx0 || x0 >= lx0 + TX)) continue;
        const int i00 = (y0 - ly0 + 1) * HX + (x0 - lx0 + 1), i01 = (y0 - ly0 + 1) * HX + (x1 - lx0 + 1);
        const int i10 = (y1 - ly0 + 1) * HX + (x0 - lx0 + 1), i11 = (y1 - ly0 + 1) * HX + (x1 - lx0 + 1);
        const int64_t o = ((int64_t)b * H + y) * W + x;
        if (conf != nullptr) {
            conf[o] = bilinear_blend(sPeak[i00], sPeak[i01], sPeak[i10], sPeak[i11], wx0, wx1, hy0, hy1);
        }
        if (sigma != nullptr) {
            sigma[o] = bilinear_blend(scaled_tap(sSig[i00], mul_a, mul_b), scaled_tap(sSig[i01], mul_a, mul_b),
                                      scaled_tap(sSig[i10], mul_a, mul_b), scaled_tap(sSig[i11], mul_a, mul_b), wx0, wx1, hy0, hy1);
        }
    }
}

int launch_softargmin_conf(const float *cost, float *disp_low, float *peak_low, float *sigma_low, float *conf, float *sigma, int B,
                           int D, int h, int w, int H, int W, float start, hipStream_t st, float ioff)
{
    const bool small = softargmin_small_tile(h, w, B);
    dim3 grid(cdiv(w, small ? 4 : 8), cdiv(h, small ? 2 : 4), B), block(256);
    const float mul_a = (float)H, mul_b = 1.0f / (float)h;
    const int exact = (H % h == 0 && W % w == 0) ? 1 : 0;
    dispatch_dt(D, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (small)
            hipLaunchKernelGGL((k_softargmin_conf<DT, 2, 4>), grid, block, 0, st, cost, disp_low, peak_low, sigma_low, conf, sigma, D, h,
                               w, H, W, start, mul_a, mul_b, ioff, exact);
        else
            hipLaunchKernelGGL((k_softargmin_conf<DT, 4, 8>), grid, block, 0, st, cost, disp_low, peak_low, sigma_low, conf, sigma, D, h,
                               w, H, W, start, mul_a, mul_b, ioff, exact);
    });
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // namespace lws

using namespace lws;

extern "C" int lws_softargmin_conf(const float *cost, int B, int D, int h, int w, float start, int H, int W, float *disp_low,
                                   float *peak_low, float *sigma_low, float *conf, float *sigma, void *stream)
{
    LWS_CHECK_ARG(cost, "softargmin_conf: null cost");
    LWS_CHECK_ARG(disp_low || peak_low || sigma_low || conf || sigma, "softargmin_conf: every output is null");
    LWS_CHECK_ARG(opkit::shape_ok(B, h, w) && D >= 1, "softargmin_conf: bad shape B=%d D=%d h=%d w=%d", B, D, h, w);
    // (float)H and the source coordinates are exact up to 2^24; the tile grid's y extent is h / 2 at most
    LWS_CHECK_ARG(H >= h && W >= w && H <= (1 << 24) && W <= (1 << 24) && h <= 2 * 65535,
                  "softargmin_conf: bad full-resolution size %dx%d for a %dx%d map", H, W, h, w);
    // a workgroup indexes the pixels under its tile with an int
    LWS_CHECK_ARG(H / h <= 1024 && W / w <= 1024, "softargmin_conf: upsampling factor above 1024 (%dx%d from %dx%d)", H, W, h, w);
    return launch_softargmin_conf(cost, disp_low, peak_low, sigma_low, conf, sigma, B, D, h, w, H, W, start, (hipStream_t)stream, 0.5f);
}
