// Temporal fusion of disparity maps over a sequence with known poses: a per-pixel Kalman step on disparity.  The previous state is
// gathered at the place the current pixel's point had in the previous left camera (four taps), carried along its ray into the
// current one, gated against the measurement and fused; optionally the previous state is splatted forward through a z-buffer and
// the pixels without a measurement hold what lands on them.  Contract: include/lwsnet_temporal.h, lws_temporal_step; one IEEE
// float32 operation per step (the build has no contraction and correctly rounded division), so tests/temporal_reference.py
// restates every output bit for bit in numpy.
//
// Launches (a fixed list: it depends on the arguments, never on the data; nothing is read back):
//   k_tp_zero    (counts without a hold pass) counts[B][5] = 0 -- a kernel, as k_wm_zero: see lws_photometric.hip on memset nodes
//   k_tp_fuse    one thread per quad of a row: state and code; with a hold pass it also clears counts and writes Zbuf = 0 at its
//                code-0 pixels, which is all the clearing the call needs.  The 12 gathers of a pixel (four taps of Dp, Vp, Ap)
//                follow a smooth motion field, so the lanes of a wave read neighbouring words of at most a few rows out of L2.
//   k_tp_splat   (hold) one thread per previous pixel: the target's code is read first and the 64-bit max is issued only where it
//                is 0 -- on a map of which the checks kept 90 % nine atomics in ten never leave the CU
//   k_tp_hold    (hold) one thread per quad: a code-0 pixel with a non-empty word takes the state of the source the word names
// The per-code counts are taken by the last kernel of the list: per thread in two packed words, per wave by shuffles, per
// workgroup through LDS (opkit::block_sum_n), then one 64-bit integer atomic per workgroup and non-zero counter.
// Determinism: what crosses threads is the integer max of the z-buffer words (agent scope, relaxed; the word holds the key of dn
// and the source index, so the winner is a function of the inputs) and the integer adds of the counts; a workgroup works on one
// image, so an image gives the same bytes in any batch, at any position, on every run.  0 bytes of scratch.
#include "lws_geomkit.h"
#include "lws_rowkit.h"

namespace lws {

namespace {

using namespace geomkit;
using u64 = unsigned long long;
constexpr int kThreads = 256;
using rowkit::store_codes;
using rowkit::store_quad;

struct TpArgs {                                             // by value in the kernel arguments
    const float *meas, *sigma;
    const uint8_t *mask;
    const float *cam, *pose, *Dp, *Vp;
    const uint16_t *Ap;
    int H, W, nq;
    float sigma0, min_disp, sigma_min, gate, q, max_jump, q_hold, max_var;
    float *D, *V;
    uint16_t *A;
    uint8_t *code;
    u64 *zbuf, *counts;
};

__device__ __forceinline__ void store_ages(uint16_t *p, int x, int W, const unsigned a[4])
{
    if (x + 4 <= W && aligned(p + x, 8)) {
        *reinterpret_cast<ushort4 *>(p + x) = make_ushort4((uint16_t)a[0], (uint16_t)a[1], (uint16_t)a[2], (uint16_t)a[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i < W) p[x + i] = (uint16_t)a[i];
    }
}

// The workgroup's pixels per code, packed[k / 3] holding code k in bits 10 (k % 3) .. (at most 4 per thread, 256 per wave), added
// to counts[b][0..4].  Called by all kThreads threads.
__device__ __forceinline__ void add_counts(unsigned (&packed)[2], u64 *__restrict__ counts, int b)
{
    __shared__ unsigned s_p[kThreads / 64][2];
    const int t = threadIdx.x;
    block_sum_n(packed, s_p);
    if (t < 5) {
        unsigned n = 0;                                     // (a wave's field is at most 256; four of them may need an 11th bit)
        for (int w = 0; w < kThreads / 64; ++w) n += (s_p[w][t / 3] >> (10 * (t % 3))) & 1023u;
        if (n) __hip_atomic_fetch_add(counts + 5 * (int64_t)b + t, (u64)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// grid (1, B): counts[b][0..4] = 0
__global__ void k_tp_zero(u64 *__restrict__ counts)
{
    if (threadIdx.x < 5) counts[5 * (int64_t)blockIdx.y + threadIdx.x] = 0;
}

// grid (ceil(H * nq / 256), B): one thread per quad of a row.  HOLD: a hold pass follows (a.zbuf is given, a previous state too).
template <bool HOLD>
__global__ __launch_bounds__(kThreads) void k_tp_fuse(TpArgs a)
{
    const int g = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int H = a.H, W = a.W;
    const int64_t img = (int64_t)b * H * W;
    if (HOLD && a.counts && blockIdx.x == 0 && t < 5) a.counts[5 * (int64_t)b + t] = 0;     // k_tp_hold adds to them
    unsigned packed[2] = {0u, 0u};
    if (g < H * a.nq) {
        const int y = g / a.nq, x = 4 * (g - y * a.nq);
        const int64_t row = img + (int64_t)y * W;
        const float *mp = a.meas + row;
        const float *sp = a.sigma ? a.sigma + row : nullptr;
        const uint8_t *mk = a.mask ? a.mask + row : nullptr;
        float m[4], s[4];
        bool ok[4];
        load_quad(mp, x, W, aligned(mp, 16), m);
        if (sp) {
            load_quad(sp, x, W, aligned(sp, 16), s);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) s[i] = a.sigma0;
        }
        load_ok(mk, x, W, aligned(mk, 4), ok);
        const Cam c = load_cam(a.cam, b);
        const bool prev = a.Dp != nullptr;
        const float *p0 = pose_of(a.pose, b), *p1 = inverse_of(a.pose, b);
        const float *Dp = a.Dp + img, *Vp = a.Vp + img;
        const uint16_t *Ap = a.Ap + img;
        const float gg = a.gate * a.gate;
        float Do[4], Vo[4];
        unsigned Ao[4];
        int co[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool valid = ok[i] && __builtin_isfinite(m[i]) && m[i] >= a.min_disp && s[i] >= 0.0f && __builtin_isfinite(s[i]);
            const float sg = fmaxf(s[i], a.sigma_min), r = sg * sg;
            bool assoc = false, pass = false;
            float Df = 0.0f, Vf = 0.0f;
            unsigned Af = 0u;
            if (valid && prev) {
                const float z = c.fb / m[i];
                const float X = back_x(c, x + i, z), Y = back_y(c, y, z);
                const float Qx = row_dot(p1, 0, X, Y, z), Qy = row_dot(p1, 1, X, Y, z), Qz = row_dot(p1, 2, X, Y, z);
                float u, v;
                if (Qz > 0.0f && project(c, Qx, Qy, Qz, H, W, 0, u, v)) {
                    const float dexp = c.fb / Qz;
                    const int i0 = (int)floorf(u), i1 = min(i0 + 1, W - 1), j0 = (int)floorf(v), j1 = min(j0 + 1, H - 1);
                    const float fa = u - (float)i0, fb_ = v - (float)j0;
                    const int t00 = j0 * W + i0, t01 = j0 * W + i1, t10 = j1 * W + i0, t11 = j1 * W + i1;
                    const unsigned a00 = Ap[t00], a01 = Ap[t01], a10 = Ap[t10], a11 = Ap[t11];
                    if (a00 > 0u && a01 > 0u && a10 > 0u && a11 > 0u) {
                        const float d00 = Dp[t00], d01 = Dp[t01], d10 = Dp[t10], d11 = Dp[t11];
                        if (jump4(d00, d01, d10, d11) <= a.max_jump) {
                            const float ds = blend4(d00, d01, d10, d11, fa, fb_);
                            const float vs = blend4(Vp[t00], Vp[t01], Vp[t10], Vp[t11], fa, fb_);
                            const unsigned ag = min(min(a00, a01), min(a10, a11));
                            const float k = dexp / ds;
                            const float Zn = row_dot(p0, 2, Qx * k, Qy * k, Qz * k);
                            if (Zn > 0.0f) {
                                assoc = true;
                                const float dpred = c.fb / Zn;
                                const float gr = dpred / ds, g2 = gr * gr, vpred = vs * (g2 * g2) + a.q;
                                const float innov = m[i] - dpred, S = vpred + r;
                                pass = innov * innov <= gg * S;
                                const float K = vpred / S;
                                Df = dpred + K * innov, Vf = vpred - K * vpred, Af = min(ag + 1u, 65535u);
                            }
                        }
                    }
                }
            }
            co[i] = !valid ? 0 : pass ? 2 : assoc ? 3 : 1;
            Do[i] = !valid ? 0.0f : pass ? Df : m[i];
            Vo[i] = !valid ? 0.0f : pass ? Vf : r;
            Ao[i] = !valid ? 0u : pass ? Af : 1u;
            if (x + i < W) packed[co[i] / 3] += 1u << (10 * (co[i] % 3));
        }
        store_quad(a.D + row, x, W, aligned(a.D + row, 16), Do[0], Do[1], Do[2], Do[3]);
        store_quad(a.V + row, x, W, aligned(a.V + row, 16), Vo[0], Vo[1], Vo[2], Vo[3]);
        store_ages(a.A + row, x, W, Ao);
        store_codes(a.code + row, x, W, aligned(a.code + row, 4), co);
        if (HOLD) {
            u64 *zb = a.zbuf + row;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < W && co[i] == 0) zb[x + i] = 0ull;
        }
    }
    if (HOLD || !a.counts) return;                          // (uniform)
    add_counts(packed, a.counts, b);
}

// grid (ceil(H * W / 256), B): one thread per previous pixel.
__global__ __launch_bounds__(kThreads) void k_tp_splat(TpArgs a)
{
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int b = blockIdx.y, H = a.H, W = a.W;
    if (s >= (int64_t)H * W) return;
    const int64_t img = (int64_t)b * H * W;
    if (a.Ap[img + s] == 0) return;
    const int y = (int)(s / W), x = (int)(s - (int64_t)y * W);
    const Cam c = load_cam(a.cam, b);
    const float *p0 = pose_of(a.pose, b);
    const float d = a.Dp[img + s];
    const float z = c.fb / d;
    const float X = back_x(c, x, z), Y = back_y(c, y, z);
    const float Px = row_dot(p0, 0, X, Y, z), Py = row_dot(p0, 1, X, Y, z), Pz = row_dot(p0, 2, X, Y, z);
    float u, v;
    if (!(Pz > 0.0f && project(c, Px, Py, Pz, H, W, 0, u, v))) return;
    const float dn = c.fb / Pz;
    const int64_t tgt = img + (int64_t)((int)rintf(v)) * W + (int)rintf(u);     // in the image: 0 <= u <= W - 1, 0 <= v <= H - 1
    if (a.code[tgt] != 0) return;
    __hip_atomic_fetch_max(a.zbuf + tgt, ((u64)key_of(dn) << 32) | (u64)(unsigned)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (ceil(H * nq / 256), B): one thread per quad of a row; the last kernel of a call with a hold pass, so it takes the counts.
__global__ __launch_bounds__(kThreads) void k_tp_hold(TpArgs a)
{
    const int g = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
    const int H = a.H, W = a.W;
    const int64_t img = (int64_t)b * H * W;
    unsigned packed[2] = {0u, 0u};
    if (g < H * a.nq) {
        const int y = g / a.nq, x = 4 * (g - y * a.nq);
        const int64_t row = img + (int64_t)y * W;
        uint8_t *cp = a.code + row;
        unsigned cw;
        if (x + 4 <= W && aligned(cp + x, 4)) {
            cw = *reinterpret_cast<const unsigned *>(cp + x);
        } else {
            cw = 0x01010101u;                               // beyond the row: not a code 0, and not counted
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < W) cw = (cw & ~(0xffu << (8 * i))) | ((unsigned)cp[x + i] << (8 * i));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (x + i >= W) break;
            int code = (int)((cw >> (8 * i)) & 0xffu);
            if (code == 0) {
                const u64 w = a.zbuf[row + x + i];
                if (w != 0ull) {
                    const int64_t s = img + (int64_t)(unsigned)(w & 0xffffffffull);
                    const float dn = unkey((unsigned)(w >> 32));
                    const float gr = dn / a.Dp[s], g2 = gr * gr;
                    const float vh = (a.Vp[s] * (g2 * g2) + a.q) + a.q_hold;
                    if (dn >= a.min_disp && vh <= a.max_var) {
                        a.D[row + x + i] = dn;
                        a.V[row + x + i] = vh;
                        a.A[row + x + i] = a.Ap[s];
                        cp[x + i] = (uint8_t)4;
                        code = 4;
                    }
                }
            }
            packed[code / 3] += 1u << (10 * (code % 3));
        }
    }
    if (!a.counts) return;                                  // (uniform)
    add_counts(packed, a.counts, b);
}

int check_shape(const char *who, int B, int H, int W, int hold)
{
    LWS_CHECK_RC(check_view_shape(who, B, H, W));
    LWS_CHECK_ARG(hold == 0 || hold == 1, "%s: hold %d (0 = off, 1 = hold what was seen before)", who, hold);
    return LWS_OK;
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int64_t lws_temporal_workspace(int B, int H, int W, int hold)
{
    LWS_CHECK_RC(check_shape("temporal_workspace", B, H, W, hold));
    return hold ? (int64_t)B * H * W * (int64_t)sizeof(u64) : 0;
}

int lws_temporal_step(const float *meas, const float *sigma, const uint8_t *mask, const float *cam, const float *pose, const float *Dp,
                      const float *Vp, const uint16_t *Ap, int B, int H, int W, float sigma0, float min_disp, float sigma_min, float gate,
                      float q, float max_jump, int hold, float q_hold, float max_var, void *workspace, float *D, float *V, uint16_t *A,
                      uint8_t *code, int64_t *counts, void *stream)
{
    const char *who = "temporal_step";
    LWS_CHECK_ARG(meas && cam, "%s: meas and cam must not be null", who);
    LWS_CHECK_ARG(D && V && A && code, "%s: D, V, A and code must not be null", who);
    const bool prev = Dp || Vp || Ap;
    LWS_CHECK_ARG(!prev || (Dp && Vp && Ap), "%s: Dp, Vp and Ap must be given together (all three null: the first frame)", who);
    LWS_CHECK_ARG(!prev || pose, "%s: a previous state needs pose", who);
    LWS_CHECK_RC(check_shape(who, B, H, W, hold));
    LWS_CHECK_ARG(!hold || workspace, "%s: hold needs a workspace (lws_temporal_workspace)", who);
    LWS_CHECK_ARG(aligned(meas, 4) && aligned(sigma, 4) && aligned(cam, 4) && aligned(pose, 4) && aligned(Dp, 4) && aligned(Vp, 4) &&
                      aligned(D, 4) && aligned(V, 4) && aligned(Ap, 2) && aligned(A, 2) && aligned(counts, 8) && aligned(workspace, 8),
                  "%s: meas / sigma / cam / pose / Dp / Vp / D / V must be 4-byte, Ap / A 2-byte, counts / workspace 8-byte aligned", who);
    LWS_CHECK_ARG(sigma || finite_nonneg(sigma0), "%s: sigma0 must be finite and >= 0 where sigma is null, got %g", who, (double)sigma0);
    LWS_CHECK_ARG(finite_pos(min_disp), "%s: min_disp must be finite and > 0, got %g", who, (double)min_disp);
    LWS_CHECK_ARG(finite_pos(sigma_min), "%s: sigma_min must be finite and > 0, got %g", who, (double)sigma_min);
    LWS_CHECK_ARG(finite_pos(gate), "%s: gate must be finite and > 0, got %g", who, (double)gate);
    LWS_CHECK_ARG(finite_nonneg(q), "%s: q must be finite and >= 0, got %g", who, (double)q);
    LWS_CHECK_ARG(max_jump >= 0.0f, "%s: max_jump must be >= 0 (+inf allowed), got %g", who, (double)max_jump);      // (false for NaN)
    LWS_CHECK_ARG(finite_nonneg(q_hold), "%s: q_hold must be finite and >= 0, got %g", who, (double)q_hold);
    LWS_CHECK_ARG(max_var > 0.0f, "%s: max_var must be > 0 (+inf allowed), got %g", who, (double)max_var);           // (false for NaN)
    const int64_t px = (int64_t)B * H * W;
    const Buf bufs[] = {{D, 4 * px, "D"}, {V, 4 * px, "V"}, {A, 2 * px, "A"}, {code, px, "code"}, {counts, 40 * (int64_t)B, "counts"},
                        {hold ? workspace : nullptr, 8 * px, "workspace"}, {meas, 4 * px, "meas"}, {sigma, 4 * px, "sigma"}, {mask, px, "mask"},
                        {cam, 20 * (int64_t)B, "cam"}, {prev ? pose : nullptr, 96 * (int64_t)B, "pose"}, {Dp, 4 * px, "Dp"}, {Vp, 4 * px, "Vp"},
                        {Ap, 2 * px, "Ap"}};
    LWS_CHECK_RC(check_no_overlap(who, bufs, 14, 6));

    const bool hold_pass = hold && prev;
    TpArgs a = {meas, sigma, mask, cam, pose, Dp, Vp, Ap, H, W, (W + 3) / 4, sigma0, min_disp, sigma_min, gate, q, max_jump, q_hold, max_var,
                D, V, A, code, hold_pass ? static_cast<u64 *>(workspace) : nullptr, reinterpret_cast<u64 *>(counts)};
    hipStream_t st = (hipStream_t)stream;
    const dim3 quads((unsigned)(((int64_t)H * a.nq + kThreads - 1) / kThreads), B);
    if (!hold_pass) {
        if (counts) {
            hipLaunchKernelGGL(k_tp_zero, dim3(1, B), dim3(64), 0, st, a.counts);
            LWS_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_tp_fuse<false>, quads, dim3(kThreads), 0, st, a);
        LWS_LAUNCH_CHECK();
        return LWS_OK;
    }
    hipLaunchKernelGGL(k_tp_fuse<true>, quads, dim3(kThreads), 0, st, a);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tp_splat, dim3((unsigned)(((int64_t)H * W + kThreads - 1) / kThreads), B), dim3(kThreads), 0, st, a);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tp_hold, quads, dim3(kThreads), 0, st, a);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // extern "C"
