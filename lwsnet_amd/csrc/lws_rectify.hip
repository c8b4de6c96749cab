// Undistortion + rectification of a raw stereo pair, fused with the network's input transform: what cv2.initUndistortRectifyMap +
// cv2.remap (INTER_LINEAR, BORDER_CONSTANT) + ToTensor + Normalize do in front of LWSNet.forward, as one launch.
// Arithmetic contract (include/lwsnet_hip.h, lws_rectify_pair): one IEEE float32 operation per step (the build has no contraction
// and correctly rounded division; no fmaf here), a 5-bit fixed-point bilinear blend in integers, so tests/rectify_reference.py
// restates every output bit for bit in numpy.  Exact bits, NOT OpenCV's: OpenCV rounds a float weight table to int16.
// Shape of the kernel: a gather bound by memory traffic (per pixel and camera 3 + 12 + 1 bytes written, four taps of 3 bytes read;
// the ~40 float operations and two divisions of the map are nothing beside it), so the map is recomputed per pixel and never stored
// unless asked for.  A workgroup is kTH rows of kTW = 64 consecutive pixels, one wave per row: the float planes, the valid bytes and
// the map are written as whole coalesced row segments, and neighbouring lanes read neighbouring source bytes of the same two source
// rows, which the next wave (the next output row) reads again from the vector cache.  The source rows are NOT staged in LDS: which
// source rectangle a tile needs depends on the distortion record, so a staged form would need a data-dependent extent and a gather
// path behind it anyway.  The 3-byte rect pixels ARE packed through LDS: a lane-per-pixel store would be three byte stores at a
// stride of 3, the packed row segment is 48 aligned dword stores (plus up to 3 head and 3 tail bytes on a misaligned row).
// Determinism: no atomics, no data-dependent loop, every pixel a pure function of its image and record.  0 bytes of scratch.
#include "lws_common.h"
#include "lws_opkit.h"

namespace lws {

namespace {

using namespace opkit;
constexpr int kTW = 64;                 // tile width: one wave = 64 consecutive pixels of a row
constexpr int kTH = 4;                  // tile height: one wave per row
constexpr int kThreads = kTW * kTH;
constexpr int kParams = 18;             // floats per record: iR[9], fx, fy, cx, cy, k1, k2, p1, p2, k3

struct RectifyArgs {
    const uint8_t *raw[2];
    uint8_t *rect[2];
    float *input[2];
    uint8_t *valid[2];
    float *map[2];
    float mean[3], std[3];
};

// grid (tiles, 2 cameras, B), kThreads threads
__global__ __launch_bounds__(kThreads) void k_rectify_pair(const RectifyArgs a, const float *__restrict__ params, int Hs, int Ws, int H,
                                                          int W, int x0, int y0, int border, int ntx)
{
    __shared__ uint32_t s_px[kTH][kTW * 3 / 4 + 1];         // one packed row segment per wave, shifted by the row's byte alignment
    const int c = blockIdx.y, b = blockIdx.z;
    const uint8_t *const raw = c ? a.raw[1] : a.raw[0];     // (selects, not a runtime index: the argument block stays in SGPRs)
    uint8_t *const rect = c ? a.rect[1] : a.rect[0];
    float *const input = c ? a.input[1] : a.input[0];
    uint8_t *const valid = c ? a.valid[1] : a.valid[0];
    float *const map = c ? a.map[1] : a.map[0];
    if (!rect && !input && !valid && !map) return;          // (uniform) nothing asked of this camera
    const int lane = threadIdx.x & (kTW - 1), wave = threadIdx.x / kTW;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int u0 = tx * kTW, u = u0 + lane, v = ty * kTH + wave;
    const bool in = u < W && v < H;

    const float *p = params + ((int64_t)b * 2 + c) * kParams;
    const float xr = (float)(u + x0), yr = (float)(v + y0);
    const float X = p[0] * xr + p[1] * yr + p[2];
    const float Y = p[3] * xr + p[4] * yr + p[5];
    const float Wc = p[6] * xr + p[7] * yr + p[8];
    const float fx = p[9], fy = p[10], cx = p[11], cy = p[12], k1 = p[13], k2 = p[14], p1 = p[15], p2 = p[16], k3 = p[17];
    const float x = X / Wc, y = Y / Wc;
    const float x2 = x * x, y2 = y * y;
    const float r2 = x2 + y2;
    const float t = (2.0f * x) * y;
    const float kr = 1.0f + ((k3 * r2 + k2) * r2 + k1) * r2;
    const float xd = (x * kr + p1 * t) + p2 * (r2 + 2.0f * x2);
    const float yd = (y * kr + p1 * (r2 + 2.0f * y2)) + p2 * t;
    const float sx = fx * xd + cx, sy = fy * yd + cy;
    const bool ok = fabsf(sx) <= 32768.0f && fabsf(sy) <= 32768.0f;             // (false for NaN)
    const int qx = ok ? (int)rintf(sx * 32.0f) : 0, qy = ok ? (int)rintf(sy * 32.0f) : 0;
    const int X0 = qx >> 5, ax = qx & 31, Y0 = qy >> 5, ay = qy & 31;
    const bool inx0 = X0 >= 0 && X0 < Ws, inx1 = X0 + 1 >= 0 && X0 + 1 < Ws;
    const bool iny0 = Y0 >= 0 && Y0 < Hs, iny1 = Y0 + 1 >= 0 && Y0 + 1 < Hs;
    const bool live = in && ok;                                                 // no tap is read for a pixel outside the window
    const uint8_t *src = raw + ((int64_t)b * Hs * Ws + (int64_t)Y0 * Ws + X0) * 3;
    const int64_t down = (int64_t)Ws * 3;
    const int w00 = (32 - ax) * (32 - ay), w01 = ax * (32 - ay), w10 = (32 - ax) * ay, w11 = ax * ay;
    int px[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int t00 = live && iny0 && inx0 ? (int)src[ch] : border;
        const int t01 = live && iny0 && inx1 ? (int)src[3 + ch] : border;
        const int t10 = live && iny1 && inx0 ? (int)src[down + ch] : border;
        const int t11 = live && iny1 && inx1 ? (int)src[down + 3 + ch] : border;
        px[ch] = (w00 * t00 + w01 * t01 + w10 * t10 + w11 * t11 + 512) >> 10;  // !ok: the weights sum to 1024, every tap = border
    }
    const int64_t plane = (int64_t)H * W, pix = (int64_t)v * W + u;
    if (in) {
        if (input) {
            float *o = input + (int64_t)b * 3 * plane + pix;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[ch * plane] = (((float)px[ch] / 255.0f) - a.mean[ch]) / a.std[ch];
        }
        if (valid) valid[(int64_t)b * plane + pix] = ok && X0 >= 0 && X0 <= Ws - 2 && Y0 >= 0 && Y0 <= Hs - 2 ? 1 : 0;
        if (map) {
            float *o = map + ((int64_t)b * plane + pix) * 2;
            o[0] = sx, o[1] = sy;
        }
    }
    if (!rect) return;                                      // (uniform)
    // The wave's row segment [u0, u0 + cnt) as bytes g[0 .. 3 cnt): up to 3 head bytes, aligned dwords, up to 3 tail bytes.  The
    // bytes sit in LDS at the offset g & 3, so that a global dword is an aligned LDS dword.
    const int cnt = v < H ? min(kTW, W - u0) : 0;           // (wave-uniform; > 0 for every row of the window: u0 < W)
    uint8_t *g = rect + ((int64_t)b * plane + (int64_t)v * W + u0) * 3;
    const int shift = (int)((uintptr_t)g & 3);
    uint8_t *s = reinterpret_cast<uint8_t *>(s_px[wave]);
    if (lane < cnt) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) s[shift + 3 * lane + ch] = (uint8_t)px[ch];
    }
    __syncthreads();
    const int nbytes = 3 * cnt;
    const int head = min((4 - shift) & 3, nbytes);
    const int ndw = (nbytes - head) >> 2, tail = nbytes - head - 4 * ndw;
    if (lane < head) g[lane] = s[shift + lane];
    if (lane < ndw) *reinterpret_cast<uint32_t *>(g + head + 4 * lane) = s_px[wave][((shift + head) >> 2) + lane];
    if (lane < tail) g[head + 4 * ndw + lane] = s[shift + head + 4 * ndw + lane];
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int lws_rectify_pair(const uint8_t *const raw[2], const float *params, int B, int Hs, int Ws, int H, int W, int x0, int y0, int border,
                     const float *mean, const float *std, uint8_t *const rect[2], float *const input[2], uint8_t *const valid[2],
                     float *const map[2], void *stream)
{
    LWS_CHECK_ARG(B >= 1 && B <= 32767, "rectify_pair: B = %d must be in 1 .. 32767", B);
    LWS_CHECK_ARG(Hs >= 1 && Ws >= 1 && Hs <= 16384 && Ws <= 16384, "rectify_pair: raw size %dx%d must be in 1 .. 16384", Hs, Ws);
    LWS_CHECK_ARG(H >= 1 && W >= 1 && x0 >= 0 && y0 >= 0 && (int64_t)x0 + W <= 32768 && (int64_t)y0 + H <= 32768,
                  "rectify_pair: window %dx%d at x0 = %d, y0 = %d must lie in 0 .. 32768", H, W, x0, y0);
    LWS_CHECK_ARG((int64_t)Hs * Ws < ((int64_t)1 << 31) && (int64_t)H * W < ((int64_t)1 << 31), "rectify_pair: Hs*Ws and H*W must be < 2^31");
    LWS_CHECK_ARG(raw && raw[0] && raw[1], "rectify_pair: raw and both of its elements must not be null");
    LWS_CHECK_ARG(params, "rectify_pair: params is null");
    LWS_CHECK_ARG(border >= 0 && border <= 255, "rectify_pair: border must be in 0 .. 255, got %d", border);
    RectifyArgs a = {};
    bool any = false, any_input = false;
    for (int c = 0; c < 2; ++c) {
        a.raw[c] = raw[c];
        a.rect[c] = rect ? rect[c] : nullptr;
        a.input[c] = input ? input[c] : nullptr;
        a.valid[c] = valid ? valid[c] : nullptr;
        a.map[c] = map ? map[c] : nullptr;
        any = any || a.rect[c] || a.input[c] || a.valid[c] || a.map[c];
        any_input = any_input || a.input[c];
    }
    LWS_CHECK_ARG(any, "rectify_pair: no output requested (every element of rect, input, valid and map is null)");
    for (int ch = 0; ch < 3; ++ch) a.mean[ch] = 0.0f, a.std[ch] = 1.0f;
    if (any_input) {
        LWS_CHECK_ARG(mean && std, "rectify_pair: an input is requested but mean or std is null");
        for (int ch = 0; ch < 3; ++ch) {
            LWS_CHECK_ARG(std[ch] != 0.0f, "rectify_pair: std[%d] is zero", ch);
            a.mean[ch] = mean[ch], a.std[ch] = std[ch];
        }
    }
    LWS_CHECK_ARG(aligned(params, 4) && aligned(a.input[0], 4) && aligned(a.input[1], 4) && aligned(a.map[0], 4) && aligned(a.map[1], 4),
                  "rectify_pair: params, input and map must be 4-byte aligned");
    // the eight outputs are written; an overlap of any of them with any other buffer is an error
    const int64_t src = (int64_t)B * Hs * Ws, px = (int64_t)B * H * W;
    const Buf bufs[] = {{a.rect[0], 3 * px, "rect[0]"},   {a.rect[1], 3 * px, "rect[1]"},   {a.input[0], 12 * px, "input[0]"},
                        {a.input[1], 12 * px, "input[1]"}, {a.valid[0], px, "valid[0]"},     {a.valid[1], px, "valid[1]"},
                        {a.map[0], 8 * px, "map[0]"},     {a.map[1], 8 * px, "map[1]"},     {raw[0], 3 * src, "raw[0]"},
                        {raw[1], 3 * src, "raw[1]"},      {params, (int64_t)B * 2 * kParams * 4, "params"}};
    LWS_CHECK_RC(check_no_overlap("rectify_pair", bufs, 11, 8));

    const int ntx = cdiv(W, kTW), nty = cdiv(H, kTH);
    hipLaunchKernelGGL(k_rectify_pair, dim3((unsigned)((int64_t)ntx * nty), 2, B), dim3(kThreads), 0, (hipStream_t)stream, a, params, Hs,
                       Ws, H, W, x0, y0, border, ntx);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // extern "C"
