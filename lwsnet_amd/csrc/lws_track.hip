// Tracking the camera against the TSDF model: per Gauss-Newton step one fused per-pixel kernel -- a reference pixel is carried
// through M once, and both its photometric term (four taps of the current image and of its central differences) and its
// point-to-plane term against the current frame's depth (one tap) are formed from that one projection and added into 32 sums in
// double -- and one small kernel per image that adds the workgroups' partial sums in a fixed order and does the update.
// Contract: include/lwsnet_track.h; one IEEE float32 operation per per-pixel step, so tests/track_reference.py restates terms and
// resid bit for bit; the sums and the update are double and agree with it to rounding.  What it shares with lws_egomotion.hip is
// stated once in lws_motionkit.h.
//
// Launches of lws_track (a list fixed by iters, never by the data; nothing is read back):
//   k_track_grey     both grey images (grid z = 0 reference, 1 current) and the start M of every image
//   k_track_normal   per step: one workgroup per 1024 pixels of an image; its 32 sums go to the workspace
//   k_track_solve    per step: one workgroup per image: the partials added, the update, the trace entry
//   k_track_normal, k_track_solve once more for the final M: resid, info, status bits 3 and 5 and the pose block
// lws_track_normal is one k_track_normal and one k_track_solve that only adds.
// Determinism: no atomics; per thread, per wave (shuffles), per workgroup ((w0 + w1) + (w2 + w3)), then the partials in the order
// of their workgroups; a workgroup works on one image.  0 bytes of scratch.
#include "lwsnet_track.h"

#include "lws_motionkit.h"

namespace lws {

namespace {

using namespace motionkit;
constexpr int kSums = 32;                                   // 21 + 6, e_p, n_p, e_g, n_g, one spare
constexpr int kTrace = 51;
constexpr int kInfo = 6;
constexpr int kCodeNoModel = 32;                            // the final linearisation has n_g < min_pixels

// Where the pieces of the workspace lie.  Doubles first: state [B][16], partials [B][tiles][32]; then the two grey images [B][H][W].
struct Layout {
    int64_t tiles, state, partials, grey[2], total;         // byte offsets, total bytes
};

Layout layout_of(int B, int H, int W)
{
    Layout L{};
    const int64_t npix = (int64_t)H * W;
    L.tiles = (npix + kTile - 1) / kTile;
    L.state = 0;
    L.partials = L.state + 8 * (int64_t)kState * B;
    L.grey[0] = L.partials + 8 * (int64_t)kSums * B * L.tiles;
    L.grey[1] = L.grey[0] + 4 * npix * B;
    L.total = (L.grey[1] + 4 * npix * B + 15) & ~(int64_t)15;
    return L;
}

// grid (ceil(H * W / 256), B, 2): z = 0 the reference image, 1 the current one; the first workgroup of an image also writes its
// start state.
__global__ __launch_bounds__(kThreads) void k_track_grey(const uint8_t *__restrict__ rgb_ref, const uint8_t *__restrict__ rgb_cur,
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

struct NormalArgs {
    const float *grey_ref, *disp_ref, *normals;             // normals: NULL where the geometric term is off (no normals, or lambda_g = 0)
    const uint8_t *mask_ref;
    const float *grey_cur, *disp_cur, *sigma_cur;
    const uint8_t *mask_cur;
    const float *cam;
    const double *M;                                        // image b's 12 doubles at M + m_stride * b
    int m_stride, H, W;
    float min_disp, huber_p, huber_g, gate_g, sigma0, sigma_min;
    double kp, kg;                                          // the terms' weights in the sums
    double *partials;                                       // [B][tiles][32]
    float *terms, *resid;
};

// The point-to-plane term of a reference pixel whose point Q projects to (u, v), 0 <= u <= W - 1, 0 <= v <= H - 1, and whose model
// normal is n.  False, with r, w, J untouched, where the term is off.
__device__ __forceinline__ bool plane_term(const NormalArgs &a, int64_t img, const Cam &c, const float *__restrict__ Mf, float Qx, float Qy,
                                           float Qz, float u, float v, float nx, float ny, float nz, float &r, float &w, float (&J)[6])
{
    const int iu = (int)rintf(u), iv = (int)rintf(v);       // 0 <= iu <= W - 1, 0 <= iv <= H - 1
    const int64_t q = img + (int64_t)iv * a.W + iu;
    const float dc = a.disp_cur[q];
    if (!((!a.mask_cur || a.mask_cur[q] == 1) && __builtin_isfinite(dc) && dc >= a.min_disp)) return false;
    const float s = a.sigma_cur ? a.sigma_cur[q] : a.sigma0;
    if (!(s >= 0.0f && __builtin_isfinite(s))) return false;
    const float zc = c.fb / dc;
    const float Px = back_x(c, iu, zc), Py = back_y(c, iv, zc);
    const float mx = rot_dot(Mf, 0, nx, ny, nz), my = rot_dot(Mf, 1, nx, ny, nz), mz = rot_dot(Mf, 2, nx, ny, nz);
    const float sg = fmaxf(s, a.sigma_min);
    const float sz = sg * ((Qz * Qz) / c.fb);               // the model's depth, not the tap's: a weight must not follow the noise it weighs
    const float ex = Qx - Px, ey = Qy - Py, ez = Qz - zc;
    const float rr = ((ex * mx + ey * my) + ez * mz) / sz;
    const float ar = fabsf(rr);
    if (!(ar <= a.gate_g)) return false;
    const float ww = ar <= a.huber_g ? 1.0f : a.huber_g / ar;
    const float cx = Py * mz - zc * my, cy = zc * mx - Px * mz, cz = Px * my - Py * mx;
    const float j0 = mx / sz, j1 = my / sz, j2 = mz / sz, j3 = cx / sz, j4 = cy / sz, j5 = cz / sz;
    const bool use = __builtin_isfinite(rr) && __builtin_isfinite(j0) && __builtin_isfinite(j1) && __builtin_isfinite(j2) &&
                     __builtin_isfinite(j3) && __builtin_isfinite(j4) && __builtin_isfinite(j5);
    if (use) r = rr, w = ww, J[0] = j0, J[1] = j1, J[2] = j2, J[3] = j3, J[4] = j4, J[5] = j5;
    return use;
}

// grid (ceil(H * W / 1024), B): thread t takes the pixels tile * 1024 + k * 256 + t, k = 0 .. 3
__global__ __launch_bounds__(kThreads) void k_track_normal(NormalArgs a)
{
    __shared__ double s_w[kThreads / 64][kSums];
    const int b = blockIdx.y, t = threadIdx.x, H = a.H, W = a.W;
    const int64_t npix = (int64_t)H * W, img = (int64_t)b * npix;
    const Cam c = level_cam(load_cam(a.cam, b), 1.0f);      // lws_ego_normal's camera at level 0
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
        const float d = a.disp_ref[img + p];
        const bool use = (!a.mask_ref || a.mask_ref[img + p] == 1) && __builtin_isfinite(d) && d >= a.min_disp;
        float rp = 0.0f, wp = 0.0f, Jp[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        float rg = 0.0f, wg = 0.0f, Jg[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (use) {
            const float z = c.fb / d;
            const float X = back_x(c, x, z), Y = back_y(c, y, z);
            const float Qx = row_dot(Mf, 0, X, Y, z), Qy = row_dot(Mf, 1, X, Y, z), Qz = row_dot(Mf, 2, X, Y, z);
            if (Qz > 0.0f) {
                float u, v;
                const bool in1 = project(c, Qx, Qy, Qz, H, W, 1, u, v);     // margin 1: the taps' central differences lie inside
                if (big && in1 && photo_term(I, H, W, c, Qx, Qy, Qz, u, v, a.grey_ref[img + p], a.huber_p, rp, wp, Jp)) {
                    const double kw = a.kp * (double)wp, dr = (double)rp;
                    add_normal(acc, kw, dr, Jp);
                    acc[27] += (kw * dr) * dr;
                    acc[28] += 1.0;
                }
                if (a.normals && u >= 0.0f && u <= (float)(W - 1) && v >= 0.0f && v <= (float)(H - 1)) {
                    const float *np = a.normals + 3 * img + p;
                    const float nx = np[0], ny = np[npix], nz = np[2 * npix];
                    const bool has = __builtin_isfinite(nx) && __builtin_isfinite(ny) && __builtin_isfinite(nz) &&
                                     !(nx == 0.0f && ny == 0.0f && nz == 0.0f);
                    if (has && plane_term(a, img, c, Mf, Qx, Qy, Qz, u, v, nx, ny, nz, rg, wg, Jg)) {
                        const double kw = a.kg * (double)wg, dr = (double)rg;
                        add_normal(acc, kw, dr, Jg);
                        acc[29] += (kw * dr) * dr;
                        acc[30] += 1.0;
                    }
                }
            }
        }
        if (a.terms) {
            float4 *tp = reinterpret_cast<float4 *>(a.terms + 16 * (img + p));       // 64 bytes per pixel; the base is 4-byte aligned only
            float *ts = a.terms + 16 * (img + p);
            if (aligned(a.terms, 16)) {
                tp[0] = make_float4(rp, wp, Jp[0], Jp[1]), tp[1] = make_float4(Jp[2], Jp[3], Jp[4], Jp[5]);
                tp[2] = make_float4(rg, wg, Jg[0], Jg[1]), tp[3] = make_float4(Jg[2], Jg[3], Jg[4], Jg[5]);
            } else {
                ts[0] = rp, ts[1] = wp, ts[8] = rg, ts[9] = wg;
#pragma unroll
                for (int i = 0; i < 6; ++i) ts[2 + i] = Jp[i], ts[10 + i] = Jg[i];
            }
        }
        if (a.resid) a.resid[2 * img + p] = rp, a.resid[2 * img + npix + p] = rg;
    }
    block_sum_n(acc, s_w);
    if (t < kSums) a.partials[((int64_t)b * gridDim.x + blockIdx.x) * kSums + t] = block_total(s_w, t);
}

struct SolveArgs {
    const double *partials;                                 // [B][tiles][32]
    int tiles, mode, min_pixels;
    double damping, kp, kg;
    double *state;                                          // [B][16] (kModeStep, kModeFinal)
    double *sums;                                           // [B][32] (kModeSums)
    double *trace;                                          // this step's entry of image 0, or NULL (kModeStep)
    int64_t trace_stride;                                   // doubles between two images' entries
    float *pose;                                            // kModeFinal
    int32_t *status;
    double *info;
};

// grid (B): the partials of image b added in a fixed order; then thread 0, in double: the update of M (kModeStep) or the outputs of
// the call (kModeFinal)
__global__ __launch_bounds__(kThreads) void k_track_solve(SolveArgs a)
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
    const double np = s_s[28], ng = s_s[30], n = np + ng;
    for (int i = 0; i < 12; ++i) s_m.M[i] = st[i];
    if (a.mode == kModeFinal) {
        int status = (int)st[14];
        if (n < (double)a.min_pixels) status |= kCodeFinalFew;
        if (ng < (double)a.min_pixels) status |= kCodeNoModel;
        a.status[b] = status;
        double *info = a.info + kInfo * (int64_t)b;
        info[0] = np, info[1] = np > 0.0 ? sqrt(s_s[27] / (a.kp * np)) : 0.0;
        info[2] = ng, info[3] = ng > 0.0 ? sqrt(s_s[29] / (a.kg * ng)) : 0.0;
        info[4] = st[12], info[5] = st[13];
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
        for (int i = 0; i < 6; ++i) tr[44 + i] = s_m.d[i];
        tr[50] = (double)code;
    }
}

struct Scalars {
    float min_disp, huber_p, sigma_p, huber_g, gate_g, sigma0, sigma_min, lambda_g;
};

int check_scalars(const char *who, const Scalars &s)
{
    LWS_CHECK_ARG(finite_pos(s.min_disp), "%s: min_disp must be finite and > 0, got %g", who, (double)s.min_disp);
    LWS_CHECK_ARG(finite_pos(s.huber_p), "%s: huber_p must be finite and > 0, got %g", who, (double)s.huber_p);
    LWS_CHECK_ARG(finite_pos(s.sigma_p), "%s: sigma_p must be finite and > 0, got %g", who, (double)s.sigma_p);
    LWS_CHECK_ARG(finite_pos(s.huber_g), "%s: huber_g must be finite and > 0, got %g", who, (double)s.huber_g);
    LWS_CHECK_ARG(s.gate_g >= s.huber_g, "%s: gate_g must be >= huber_g (+inf allowed), got %g < %g", who, (double)s.gate_g, (double)s.huber_g);   // (false for NaN)
    LWS_CHECK_ARG(finite_nonneg(s.sigma0), "%s: sigma0 must be finite and >= 0, got %g", who, (double)s.sigma0);
    LWS_CHECK_ARG(finite_pos(s.sigma_min), "%s: sigma_min must be finite and > 0, got %g", who, (double)s.sigma_min);
    LWS_CHECK_ARG(finite_nonneg(s.lambda_g), "%s: lambda_g must be finite and >= 0, got %g", who, (double)s.lambda_g);
    return LWS_OK;
}

struct Maps {
    const float *disp_ref, *normals_ref;
    const uint8_t *mask_ref;
    const float *disp_cur, *sigma_cur;
    const uint8_t *mask_cur;
    const float *cam;
};

NormalArgs normal_args(const float *grey_ref, const float *grey_cur, const Maps &m, const double *M, int m_stride, int H, int W, const Scalars &s,
                       double *partials, float *terms, float *resid)
{
    NormalArgs n{};
    n.grey_ref = grey_ref, n.disp_ref = m.disp_ref, n.normals = s.lambda_g > 0.0f ? m.normals_ref : nullptr, n.mask_ref = m.mask_ref;
    n.grey_cur = grey_cur, n.disp_cur = m.disp_cur, n.sigma_cur = m.sigma_cur, n.mask_cur = m.mask_cur, n.cam = m.cam;
    n.M = M, n.m_stride = m_stride, n.H = H, n.W = W;
    n.min_disp = s.min_disp, n.huber_p = s.huber_p, n.huber_g = s.huber_g, n.gate_g = s.gate_g, n.sigma0 = s.sigma0, n.sigma_min = s.sigma_min;
    n.kp = 1.0 / ((double)s.sigma_p * (double)s.sigma_p), n.kg = (double)s.lambda_g;
    n.partials = partials, n.terms = terms, n.resid = resid;
    return n;
}

int launch_round(const NormalArgs &n, SolveArgs &v, int B, const Layout &L, hipStream_t st)
{
    hipLaunchKernelGGL(k_track_normal, dim3((unsigned)L.tiles, B), dim3(kThreads), 0, st, n);
    LWS_LAUNCH_CHECK();
    v.partials = n.partials, v.tiles = (int)L.tiles, v.kp = n.kp, v.kg = n.kg;
    hipLaunchKernelGGL(k_track_solve, dim3(B), dim3(kThreads), 0, st, v);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int64_t lws_track_workspace(int B, int H, int W)
{
    LWS_CHECK_RC(check_view_shape("track_workspace", B, H, W));
    return layout_of(B, H, W).total;
}

int lws_track_normal(const float *grey_ref, const float *disp_ref, const float *normals_ref, const uint8_t *mask_ref,
                     const float *grey_cur, const float *disp_cur, const float *sigma_cur, const uint8_t *mask_cur, const float *cam,
                     const double *M, int B, int H, int W, float min_disp, float huber_p, float sigma_p, float huber_g, float gate_g,
                     float sigma0, float sigma_min, float lambda_g, void *workspace, double *sums, float *terms, void *stream)
{
    const char *who = "track_normal";
    LWS_CHECK_ARG(grey_ref && disp_ref && grey_cur && disp_cur && cam && M, "%s: grey_ref, disp_ref, grey_cur, disp_cur, cam and M must not be null", who);
    LWS_CHECK_ARG(workspace && sums, "%s: workspace and sums must not be null", who);
    LWS_CHECK_RC(check_view_shape(who, B, H, W));
    LWS_CHECK_ARG(aligned(grey_ref, 4) && aligned(disp_ref, 4) && aligned(normals_ref, 4) && aligned(grey_cur, 4) && aligned(disp_cur, 4) &&
                      aligned(sigma_cur, 4) && aligned(cam, 4) && aligned(terms, 4) && aligned(M, 8) && aligned(sums, 8) && aligned(workspace, 8),
                  "%s: grey_ref / disp_ref / normals_ref / grey_cur / disp_cur / sigma_cur / cam / terms must be 4-byte, M / sums / workspace 8-byte aligned", who);
    const Scalars sc = {min_disp, huber_p, sigma_p, huber_g, gate_g, sigma0, sigma_min, lambda_g};
    LWS_CHECK_RC(check_scalars(who, sc));
    const Layout L = layout_of(B, H, W);
    const int64_t px = (int64_t)B * H * W;
    const Buf bufs[] = {{sums, 8 * (int64_t)kSums * B, "sums"}, {terms, 64 * px, "terms"}, {workspace, L.total, "workspace"},
                        {grey_ref, 4 * px, "grey_ref"}, {disp_ref, 4 * px, "disp_ref"}, {normals_ref, 12 * px, "normals_ref"}, {mask_ref, px, "mask_ref"},
                        {grey_cur, 4 * px, "grey_cur"}, {disp_cur, 4 * px, "disp_cur"}, {sigma_cur, 4 * px, "sigma_cur"}, {mask_cur, px, "mask_cur"},
                        {cam, 20 * (int64_t)B, "cam"}, {M, 96 * (int64_t)B, "M"}};
    LWS_CHECK_RC(check_no_overlap(who, bufs, 13, 3));

    char *ws = static_cast<char *>(workspace);
    const Maps maps = {disp_ref, normals_ref, mask_ref, disp_cur, sigma_cur, mask_cur, cam};
    const NormalArgs n = normal_args(grey_ref, grey_cur, maps, M, 12, H, W, sc, reinterpret_cast<double *>(ws + L.partials), terms, nullptr);
    SolveArgs s{};
    s.mode = kModeSums, s.sums = sums;
    return launch_round(n, s, B, L, (hipStream_t)stream);
}

int lws_track(const uint8_t *rgb_ref, const float *disp_ref, const float *normals_ref, const uint8_t *mask_ref, const uint8_t *rgb_cur,
              const float *disp_cur, const float *sigma_cur, const uint8_t *mask_cur, const float *cam, const float *init, int B, int H,
              int W, int iters, float min_disp, float huber_p, float sigma_p, float huber_g, float gate_g, float sigma0,
              float sigma_min, float lambda_g, float damping, int min_pixels, void *workspace, float *pose, int32_t *status,
              double *info, double *trace, float *resid, void *stream)
{
    const char *who = "track";
    LWS_CHECK_ARG(rgb_ref && disp_ref && rgb_cur && disp_cur && cam, "%s: rgb_ref, disp_ref, rgb_cur, disp_cur and cam must not be null", who);
    LWS_CHECK_ARG(workspace && pose && status && info, "%s: workspace, pose, status and info must not be null", who);
    LWS_CHECK_RC(check_view_shape(who, B, H, W));
    LWS_CHECK_ARG(iters >= 1 && iters <= 64, "%s: iters %d outside 1..64", who, iters);
    LWS_CHECK_ARG(aligned(disp_ref, 4) && aligned(normals_ref, 4) && aligned(disp_cur, 4) && aligned(sigma_cur, 4) && aligned(cam, 4) &&
                      aligned(init, 4) && aligned(pose, 4) && aligned(status, 4) && aligned(resid, 4) && aligned(info, 8) && aligned(trace, 8) &&
                      aligned(workspace, 8),
                  "%s: disp_ref / normals_ref / disp_cur / sigma_cur / cam / init / pose / status / resid must be 4-byte, info / trace / workspace 8-byte aligned", who);
    const Scalars sc = {min_disp, huber_p, sigma_p, huber_g, gate_g, sigma0, sigma_min, lambda_g};
    LWS_CHECK_RC(check_scalars(who, sc));
    LWS_CHECK_ARG(finite_nonneg(damping), "%s: damping must be finite and >= 0, got %g", who, (double)damping);
    LWS_CHECK_ARG(min_pixels >= 1, "%s: min_pixels %d < 1", who, min_pixels);
    const Layout L = layout_of(B, H, W);
    const int64_t px = (int64_t)B * H * W;
    const Buf bufs[] = {{pose, 96 * (int64_t)B, "pose"}, {status, 4 * (int64_t)B, "status"}, {info, 8 * (int64_t)kInfo * B, "info"},
                        {trace, 8 * (int64_t)kTrace * iters * B, "trace"}, {resid, 8 * px, "resid"}, {workspace, L.total, "workspace"},
                        {rgb_ref, 3 * px, "rgb_ref"}, {disp_ref, 4 * px, "disp_ref"}, {normals_ref, 12 * px, "normals_ref"}, {mask_ref, px, "mask_ref"},
                        {rgb_cur, 3 * px, "rgb_cur"}, {disp_cur, 4 * px, "disp_cur"}, {sigma_cur, 4 * px, "sigma_cur"}, {mask_cur, px, "mask_cur"},
                        {cam, 20 * (int64_t)B, "cam"}, {init, 48 * (int64_t)B, "init"}};
    LWS_CHECK_RC(check_no_overlap(who, bufs, 16, 6));

    char *ws = static_cast<char *>(workspace);
    double *state = reinterpret_cast<double *>(ws + L.state), *partials = reinterpret_cast<double *>(ws + L.partials);
    float *g_ref = reinterpret_cast<float *>(ws + L.grey[0]), *g_cur = reinterpret_cast<float *>(ws + L.grey[1]);
    hipStream_t st = (hipStream_t)stream;
    const int64_t npix = (int64_t)H * W;
    hipLaunchKernelGGL(k_track_grey, dim3((unsigned)((npix + kThreads - 1) / kThreads), B, 2), dim3(kThreads), 0, st, rgb_ref, rgb_cur, init, npix,
                       g_ref, g_cur, state);
    LWS_LAUNCH_CHECK();
    const Maps maps = {disp_ref, normals_ref, mask_ref, disp_cur, sigma_cur, mask_cur, cam};
    for (int s = 0; s <= iters; ++s) {                      // the last round is the final linearisation
        const bool final = s == iters;
        const NormalArgs n = normal_args(g_ref, g_cur, maps, state, kState, H, W, sc, partials, nullptr, final ? resid : nullptr);
        SolveArgs v{};
        v.mode = final ? kModeFinal : kModeStep, v.min_pixels = min_pixels, v.damping = (double)damping, v.state = state;
        v.trace = trace && !final ? trace + (int64_t)kTrace * s : nullptr, v.trace_stride = (int64_t)kTrace * iters;
        v.pose = pose, v.status = status, v.info = info;
        LWS_CHECK_RC(launch_round(n, v, B, L, st));
    }
    return LWS_OK;
}

}  // extern "C"
