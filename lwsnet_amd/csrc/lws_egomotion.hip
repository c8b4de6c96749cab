// Ego-motion by dense direct alignment of two consecutive left images with the previous frame's disparity: grey pyramids, and per
// Gauss-Newton step one per-pixel kernel (warp, four-tap sample of the image and of its central differences, the 6-vector Jacobian,
// 29 sums in double) and one small kernel per image that adds the workgroups' partial sums in a fixed order, solves the 6 x 6 system
// by Cholesky and composes M <- exp(delta) . M.  Contract: include/lwsnet_egomotion.h; one IEEE float32 operation per per-pixel step
// (the build has no contraction and correctly rounded division), so tests/egomotion_reference.py restates terms, resid and the
// pyramids bit for bit; the sums and the update are double and agree with it to rounding.
//
// Launches of lws_egomotion (a list fixed by levels and iters, never by the data; nothing is read back):
//   k_ego_grey     both level-0 grey images (grid z = 0 reference, 1 current) and the start M of every image
//   k_ego_down     per level 1 .. levels - 1: the two grey images and the reference disparity of that level from the level below
//   k_ego_normal   per step: one workgroup per 1024 pixels of an image; its 29 sums go to the workspace
//   k_ego_solve    per step: one workgroup per image: the partials added, the update, the trace entry
//   k_ego_normal, k_ego_solve once more at level 0 for the final M: resid, info, status bit 3 and the pose block
// lws_ego_normal is one k_ego_normal and one k_ego_solve that only adds.  A level without pixels (H or W below 2^level) launches no
// k_ego_normal; its k_ego_solve sees n = 0.
// Determinism: no atomics; per thread, per wave (shuffles), per workgroup ((w0 + w1) + (w2 + w3)), then the partials in the order
// of their workgroups; a workgroup works on one image.  The small matrices of the update live in LDS: 0 bytes of scratch.
#include "lwsnet_egomotion.h"

#include "lws_motionkit.h"

namespace lws {

namespace {

using namespace motionkit;
constexpr int kSums = 29;
constexpr int kTrace = 48;
constexpr int kMaxLevels = 8;

// Where the pieces of the workspace lie.  Doubles first: state [B][16], partials [B][tiles of level 0][29]; then three float
// pyramids (reference grey, current grey, reference disparity), level l of each an array [B][H_l][W_l] at cum[l] * B floats.
struct Layout {
    int Hl[kMaxLevels], Wl[kMaxLevels];
    int64_t cum[kMaxLevels + 1];                            // pixels of one image in the levels below l
    int64_t tiles0, state, partials, pyr[3], total;         // byte offsets, total bytes
};

Layout layout_of(int B, int H, int W, int levels)
{
    Layout L{};
    int64_t c = 0;
    for (int l = 0; l < levels; ++l) {
        L.Hl[l] = H >> l, L.Wl[l] = W >> l;
        L.cum[l] = c;
        c += (int64_t)L.Hl[l] * L.Wl[l];
    }
    L.cum[levels] = c;
    L.tiles0 = ((int64_t)H * W + kTile - 1) / kTile;
    L.state = 0;
    L.partials = L.state + 8 * (int64_t)kState * B;
    L.pyr[0] = L.partials + 8 * (int64_t)kSums * B * L.tiles0;
    L.pyr[1] = L.pyr[0] + 4 * c * B;
    L.pyr[2] = L.pyr[1] + 4 * c * B;
    L.total = (L.pyr[2] + 4 * c * B + 15) & ~(int64_t)15;
    return L;
}

// grid (ceil(H * W / 256), B, 2): z = 0 the reference image, 1 the current one; the first workgroup of an image also writes its
// start state.
__global__ __launch_bounds__(kThreads) void k_ego_grey(const uint8_t *__restrict__ rgb_ref, const uint8_t *__restrict__ rgb_cur,
                                                       const float *__restrict__ init, int64_t npix, float *__restrict__ g_ref,
                                                       float *__restrict__ g_cur, double *__restrict__ state)
{
    const int b = blockIdx.y, t = threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.z == 0 && t < kState) start_state(init, b, t, state);
    const int64_t p = (int64_t)blockIdx.x * kThreads + t;
    if (p >= npix) return;
    const uint8_t *s = (blockIdx.z ? rgb_cur : rgb_ref) + 3 * ((int64_t)b * npix + p);
    (blockIdx.z ? g_cur : g_ref)[(int64_t)b * npix + p] = grey_rule(s);
}

struct DownArgs {
    const float *src[3];                                    // reference grey, current grey, reference disparity: [B][Hs][Ws]
    float *dst[3];                                          // [B][Hs / 2][Ws / 2]
    const uint8_t *mask;                                    // of the source disparity (level 0 only), or NULL
    int Hs, Ws;
    float min_disp, max_jump;
};

// grid (ceil((Hs / 2) * (Ws / 2) / 256), B, 3): z = 0, 1 the grey images, 2 the disparity
__global__ __launch_bounds__(kThreads) void k_ego_down(DownArgs a)
{
    const int b = blockIdx.y, which = blockIdx.z;
    const int Hd = a.Hs >> 1, Wd = a.Ws >> 1;
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= (int64_t)Hd * Wd) return;
    const int y = (int)(p / Wd), x = (int)(p - (int64_t)y * Wd);
    const int64_t s00 = (int64_t)b * a.Hs * a.Ws + (int64_t)(2 * y) * a.Ws + 2 * x;
    const float *src = a.src[which] + s00;
    const float t00 = src[0], t01 = src[1], t10 = src[a.Ws], t11 = src[a.Ws + 1];
    const float mean = ((t00 + t01) + (t10 + t11)) * 0.25f;
    float out = mean;
    if (which == 2) {
        const uint8_t *m = a.mask ? a.mask + s00 : nullptr;
        bool ok = !m || (m[0] == 1 && m[1] == 1 && m[a.Ws] == 1 && m[a.Ws + 1] == 1);
        ok = ok && __builtin_isfinite(t00) && t00 >= a.min_disp && __builtin_isfinite(t01) && t01 >= a.min_disp &&
             __builtin_isfinite(t10) && t10 >= a.min_disp && __builtin_isfinite(t11) && t11 >= a.min_disp;
        out = ok && jump4(t00, t01, t10, t11) <= a.max_jump ? mean : 0.0f;
    }
    a.dst[which][(int64_t)b * Hd * Wd + p] = out;
}

struct NormalArgs {
    const float *grey_ref, *disp;
    const uint8_t *mask;
    const float *grey_cur, *cam;
    const double *M;                                        // image b's 12 doubles at M + m_stride * b
    int m_stride, H, W;
    float scale, min_disp, huber;                           // scale = 2^-level
    double *partials;                                       // [B][tiles][29]
    float *terms, *resid;
};

// grid (ceil(H * W / 1024), B): thread t takes the pixels tile * 1024 + k * 256 + t, k = 0 .. 3
__global__ __launch_bounds__(kThreads) void k_ego_normal(NormalArgs a)
{
    __shared__ double s_w[kThreads / 64][kSums];
    const int b = blockIdx.y, t = threadIdx.x, H = a.H, W = a.W;
    const int64_t npix = (int64_t)H * W, img = (int64_t)b * npix;
    const Cam c0 = load_cam(a.cam, b);                      // the full-resolution camera; c: this level's
    const Cam c = level_cam(c0, a.scale);
    float Mf[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) Mf[i] = (float)a.M[(int64_t)a.m_stride * b + i];
    const bool big = W >= 4 && H >= 4;
    const float *I = a.grey_cur + img;
    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int k = 0; k < kPerThread; ++k) {
        const int64_t p = (int64_t)blockIdx.x * kTile + k * kThreads + t;
        if (p >= npix) break;
        const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
        const float d = a.disp[img + p];
        bool use = (!a.mask || a.mask[img + p] == 1) && __builtin_isfinite(d) && d >= a.min_disp;
        float r = 0.0f, w = 0.0f, J[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (use) {
            const float z = c.fb / d;
            const float X = back_x(c, x, z), Y = back_y(c, y, z);
            const float Qx = row_dot(Mf, 0, X, Y, z), Qy = row_dot(Mf, 1, X, Y, z), Qz = row_dot(Mf, 2, X, Y, z);
            float u, v;
            const bool inside = project(c, Qx, Qy, Qz, H, W, 1, u, v);      // margin 1: the taps' central differences lie inside
            use = Qz > 0.0f && big && inside;
            if (use) {
                use = photo_term(I, H, W, c, Qx, Qy, Qz, u, v, a.grey_ref[img + p], a.huber, r, w, J);
                if (use) {
                    const double dw = (double)w, dr = (double)r;
                    add_normal(acc, dw, dr, J);
                    acc[27] += (dw * dr) * dr;
                    acc[28] += 1.0;
                }
            }
        }
        if (a.terms) {
            float *tp = a.terms + 8 * (img + p);
            tp[0] = r, tp[1] = w;
#pragma unroll
            for (int i = 0; i < 6; ++i) tp[2 + i] = J[i];
        }
        if (a.resid) a.resid[img + p] = r;
    }
    block_sum_n(acc, s_w);
    if (t < kSums) a.partials[((int64_t)b * gridDim.x + blockIdx.x) * kSums + t] = block_total(s_w, t);
}

struct SolveArgs {
    const double *partials;                                 // [B][tiles][29]
    int tiles, mode, min_pixels;
    double damping;
    double *state;                                          // [B][16] (kModeStep, kModeFinal)
    double *sums;                                           // [B][29] (kModeSums)
    double *trace;                                          // this step's entry of image 0, or NULL (kModeStep)
    int64_t trace_stride;                                   // doubles between two images' entries
    float *pose;                                            // kModeFinal
    int32_t *status;
    double *info;
};

// grid (B): the partials of image b added in a fixed order; then thread 0, in double: the update of M (kModeStep) or the outputs of
// the call (kModeFinal).  The 6 x 6 system lives in LDS so that no index of it needs scratch.
__global__ __launch_bounds__(kThreads) void k_ego_solve(SolveArgs a)
{
    __shared__ double s_w[kThreads / 64][kSums];
    __shared__ double s_s[kSums];
    __shared__ SolveLds s_m;
    const int b = blockIdx.x, t = threadIdx.x;
    double acc[kSums];
    add_partials(a.partials + (int64_t)b * a.tiles * kSums, a.tiles, acc);
    block_sum_n(acc, s_w);
    if (t < kSums) {
        const double v = block_total(s_w, t);
        s_s[t] = v;
        if (a.mode == kModeSums) a.sums[(int64_t)b * kSums + t] = v;
    }
    if (a.mode == kModeSums) return;                        // (uniform)
    __syncthreads();
    if (t != 0) return;
    double *st = a.state + (int64_t)kState * b;
    const double n = s_s[28];
    for (int i = 0; i < 12; ++i) s_m.M[i] = st[i];
    if (a.mode == kModeFinal) {
        int status = (int)st[14];
        if (n < (double)a.min_pixels) status |= kCodeFinalFew;
        a.status[b] = status;
        double *info = a.info + 4 * (int64_t)b;
        info[0] = n, info[1] = n > 0.0 ? sqrt(s_s[27] / n) : 0.0, info[2] = st[12], info[3] = st[13];
        write_pose(s_m.M, a.pose + kPoseFloats * (int64_t)b);
        return;
    }
    int code = 0;
    for (int i = 0; i < 6; ++i) s_m.d[i] = 0.0;
    if (n < (double)a.min_pixels) {
        code = kCodeFew;
    } else {
        bool finite = true;
        for (int k = 0; k < kSums; ++k) finite = finite && __builtin_isfinite(s_s[k]);
        if (!finite) code = kCodeNonFinite;
    }
    if (code == 0) code = gauss_newton_step(s_s, a.damping, s_m, st);
    st[14] = (double)((int)st[14] | code);
    if (a.trace) {
        double *tr = a.trace + a.trace_stride * b;
        for (int i = 0; i < 12; ++i) tr[i] = s_m.M[i];
        for (int k = 0; k < kSums; ++k) tr[12 + k] = s_s[k];
        for (int i = 0; i < 6; ++i) tr[41 + i] = s_m.d[i];
        tr[47] = (double)code;
    }
}

int check_levels(const char *who, int levels)
{
    LWS_CHECK_ARG(levels >= 1 && levels <= kMaxLevels, "%s: levels %d outside 1..%d", who, levels, kMaxLevels);
    return LWS_OK;
}

int launch_normal(const NormalArgs &n, int B, hipStream_t st)
{
    const int64_t npix = (int64_t)n.H * n.W;
    if (npix == 0) return LWS_OK;
    hipLaunchKernelGGL(k_ego_normal, dim3((unsigned)((npix + kTile - 1) / kTile), B), dim3(kThreads), 0, st, n);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int64_t lws_egomotion_workspace(int B, int H, int W, int levels)
{
    const char *who = "egomotion_workspace";
    LWS_CHECK_RC(check_view_shape(who, B, H, W));
    LWS_CHECK_RC(check_levels(who, levels));
    return layout_of(B, H, W, levels).total;
}

int lws_ego_normal(const float *grey_ref, const float *disp_ref, const uint8_t *mask, const float *grey_cur, const float *cam,
                   const double *M, int B, int H, int W, int level, float min_disp, float huber, void *workspace, double *sums,
                   float *terms, void *stream)
{
    const char *who = "ego_normal";
    LWS_CHECK_ARG(grey_ref && disp_ref && grey_cur && cam && M, "%s: grey_ref, disp_ref, grey_cur, cam and M must not be null", who);
    LWS_CHECK_ARG(workspace && sums, "%s: workspace and sums must not be null", who);
    LWS_CHECK_RC(check_view_shape(who, B, H, W));
    LWS_CHECK_ARG(level >= 0 && level < kMaxLevels, "%s: level %d outside 0..%d", who, level, kMaxLevels - 1);
    LWS_CHECK_ARG(aligned(grey_ref, 4) && aligned(disp_ref, 4) && aligned(grey_cur, 4) && aligned(cam, 4) && aligned(terms, 4) &&
                      aligned(M, 8) && aligned(sums, 8) && aligned(workspace, 8),
                  "%s: grey_ref / disp_ref / grey_cur / cam / terms must be 4-byte, M / sums / workspace 8-byte aligned", who);
    LWS_CHECK_ARG(finite_pos(min_disp), "%s: min_disp must be finite and > 0, got %g", who, (double)min_disp);
    LWS_CHECK_ARG(finite_pos(huber), "%s: huber must be finite and > 0, got %g", who, (double)huber);
    const Layout L = layout_of(B, H, W, 1);
    const int64_t px = (int64_t)B * H * W;
    const Buf bufs[] = {{sums, 8 * (int64_t)kSums * B, "sums"}, {terms, 32 * px, "terms"}, {workspace, L.total, "workspace"},
                        {grey_ref, 4 * px, "grey_ref"}, {disp_ref, 4 * px, "disp_ref"}, {mask, px, "mask"}, {grey_cur, 4 * px, "grey_cur"},
                        {cam, 20 * (int64_t)B, "cam"}, {M, 96 * (int64_t)B, "M"}};
    LWS_CHECK_RC(check_no_overlap(who, bufs, 9, 3));

    char *ws = static_cast<char *>(workspace);
    double *partials = reinterpret_cast<double *>(ws + L.partials);
    hipStream_t st = (hipStream_t)stream;
    const NormalArgs n = {grey_ref, disp_ref, mask, grey_cur, cam, M, 12, H, W, ldexpf(1.0f, -level), min_disp, huber, partials, terms, nullptr};
    LWS_CHECK_RC(launch_normal(n, B, st));
    SolveArgs s{};
    s.partials = partials, s.tiles = (int)L.tiles0, s.mode = kModeSums, s.sums = sums;
    hipLaunchKernelGGL(k_ego_solve, dim3(B), dim3(kThreads), 0, st, s);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

int lws_egomotion(const uint8_t *rgb_ref, const float *disp_ref, const uint8_t *mask, const uint8_t *rgb_cur, const float *cam,
                  const float *init, int B, int H, int W, int levels, int iters, float min_disp, float max_jump, float huber,
                  float damping, int min_pixels, void *workspace, float *pose, int32_t *status, double *info, double *trace,
                  float *resid, void *stream)
{
    const char *who = "egomotion";
    LWS_CHECK_ARG(rgb_ref && disp_ref && rgb_cur && cam, "%s: rgb_ref, disp_ref, rgb_cur and cam must not be null", who);
    LWS_CHECK_ARG(workspace && pose && status && info, "%s: workspace, pose, status and info must not be null", who);
    LWS_CHECK_RC(check_view_shape(who, B, H, W));
    LWS_CHECK_RC(check_levels(who, levels));
    LWS_CHECK_ARG(iters >= 1 && iters <= 64, "%s: iters %d outside 1..64", who, iters);
    LWS_CHECK_ARG(aligned(disp_ref, 4) && aligned(cam, 4) && aligned(init, 4) && aligned(pose, 4) && aligned(status, 4) && aligned(resid, 4) &&
                      aligned(info, 8) && aligned(trace, 8) && aligned(workspace, 8),
                  "%s: disp_ref / cam / init / pose / status / resid must be 4-byte, info / trace / workspace 8-byte aligned", who);
    LWS_CHECK_ARG(finite_pos(min_disp), "%s: min_disp must be finite and > 0, got %g", who, (double)min_disp);
    LWS_CHECK_ARG(max_jump >= 0.0f, "%s: max_jump must be >= 0 (+inf allowed), got %g", who, (double)max_jump);      // (false for NaN)
    LWS_CHECK_ARG(finite_pos(huber), "%s: huber must be finite and > 0, got %g", who, (double)huber);
    LWS_CHECK_ARG(finite_nonneg(damping), "%s: damping must be finite and >= 0, got %g", who, (double)damping);
    LWS_CHECK_ARG(min_pixels >= 1, "%s: min_pixels %d < 1", who, min_pixels);
    const Layout L = layout_of(B, H, W, levels);
    const int steps = levels * iters;
    const int64_t px = (int64_t)B * H * W;
    const Buf bufs[] = {{pose, 96 * (int64_t)B, "pose"}, {status, 4 * (int64_t)B, "status"}, {info, 32 * (int64_t)B, "info"},
                        {trace, 8 * (int64_t)kTrace * steps * B, "trace"}, {resid, 4 * px, "resid"}, {workspace, L.total, "workspace"},
                        {rgb_ref, 3 * px, "rgb_ref"}, {disp_ref, 4 * px, "disp_ref"}, {mask, px, "mask"}, {rgb_cur, 3 * px, "rgb_cur"},
                        {cam, 20 * (int64_t)B, "cam"}, {init, 48 * (int64_t)B, "init"}};
    LWS_CHECK_RC(check_no_overlap(who, bufs, 12, 6));

    char *ws = static_cast<char *>(workspace);
    double *state = reinterpret_cast<double *>(ws + L.state), *partials = reinterpret_cast<double *>(ws + L.partials);
    float *pyr[3] = {reinterpret_cast<float *>(ws + L.pyr[0]), reinterpret_cast<float *>(ws + L.pyr[1]), reinterpret_cast<float *>(ws + L.pyr[2])};
    hipStream_t st = (hipStream_t)stream;
    const int64_t npix = (int64_t)H * W;
    hipLaunchKernelGGL(k_ego_grey, dim3((unsigned)((npix + kThreads - 1) / kThreads), B, 2), dim3(kThreads), 0, st, rgb_ref, rgb_cur, init, npix,
                       pyr[0], pyr[1], state);
    LWS_LAUNCH_CHECK();
    for (int l = 1; l < levels; ++l) {
        const int64_t nd = (int64_t)L.Hl[l] * L.Wl[l];
        if (nd == 0) break;                                 // no pixels at this level, nor above it
        DownArgs d{};
        for (int k = 0; k < 3; ++k) {
            d.src[k] = pyr[k] + L.cum[l - 1] * B;
            d.dst[k] = pyr[k] + L.cum[l] * B;
        }
        if (l == 1) d.src[2] = disp_ref, d.mask = mask;
        d.Hs = L.Hl[l - 1], d.Ws = L.Wl[l - 1], d.min_disp = min_disp, d.max_jump = max_jump;
        hipLaunchKernelGGL(k_ego_down, dim3((unsigned)((nd + kThreads - 1) / kThreads), B, 3), dim3(kThreads), 0, st, d);
        LWS_LAUNCH_CHECK();
    }
    for (int s = 0; s <= steps; ++s) {                      // the last round is the final linearisation at level 0
        const bool final = s == steps;
        const int l = final ? 0 : levels - 1 - s / iters;
        NormalArgs n = {pyr[0] + L.cum[l] * B, l == 0 ? disp_ref : pyr[2] + L.cum[l] * B, l == 0 ? mask : nullptr, pyr[1] + L.cum[l] * B, cam,
                        state, kState, L.Hl[l], L.Wl[l], ldexpf(1.0f, -l), min_disp, huber, partials, nullptr, final ? resid : nullptr};
        LWS_CHECK_RC(launch_normal(n, B, st));
        SolveArgs v{};
        v.partials = partials, v.tiles = (int)(((int64_t)L.Hl[l] * L.Wl[l] + kTile - 1) / kTile);
        v.mode = final ? kModeFinal : kModeStep, v.min_pixels = min_pixels, v.damping = (double)damping, v.state = state;
        v.trace = trace && !final ? trace + (int64_t)kTrace * s : nullptr, v.trace_stride = (int64_t)kTrace * steps;
        v.pose = pose, v.status = status, v.info = info;
        hipLaunchKernelGGL(k_ego_solve, dim3(B), dim3(kThreads), 0, st, v);
        LWS_LAUNCH_CHECK();
    }
    return LWS_OK;
}

}  // extern "C"
