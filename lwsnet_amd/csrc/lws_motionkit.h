// What the two direct pose estimators share (lws_egomotion.hip: frame to frame, photometric; lws_track.hip: frame to model,
// photometric + point-to-plane): the grey rule, the four-tap photometric pixel, the 27 products of a term's normal equations, the
// workgroup sums and the adding of the partials, the Gauss-Newton update (Cholesky, exp, compose) with its codes, and the pose
// block.  Each is stated here once; the contracts are include/lwsnet_egomotion.h and include/lwsnet_track.h.  The per-pixel
// functions are the float32 operations they show in the order they show them; the update is double.
#pragma once
#include "lws_geomkit.h"

namespace lws::motionkit {

using namespace geomkit;

constexpr int kThreads = 256;
constexpr int kPerThread = 4;                               // pixels of a thread in a normal kernel
constexpr int kTile = kThreads * kPerThread;                // pixels of a workgroup
constexpr int kState = 16;                                  // doubles per image: M[12], |delta| of the last step taken, steps taken, status
constexpr double kSeriesBelow = 0.05;
constexpr double kMinStep2 = 0x1p-46;
enum { kCodeFew = 1, kCodeSingular = 2, kCodeNonFinite = 4, kCodeFinalFew = 8, kCodeSmall = 16 };
enum { kModeSums = 0, kModeStep = 1, kModeFinal = 2 };

// The camera of pyramid level l from the full-resolution one, scale = 2^-l (level 0 goes through the same operations)
__device__ __forceinline__ Cam level_cam(const Cam &c0, float scale)
{
    return Cam{c0.fx * scale, c0.fy * scale, (c0.cx + 0.5f) * scale - 0.5f, (c0.cy + 0.5f) * scale - 0.5f, c0.fb};
}

// g = (float)(77 R + 150 G + 29 B) / 256.0f of the pixel at s
__device__ __forceinline__ float grey_rule(const uint8_t *__restrict__ s)
{
    const int sum = 77 * (int)s[0] + 150 * (int)s[1] + 29 * (int)s[2];
    return (float)sum / 256.0f;
}

// the start state of image b: init's 12 floats or the identity, then zeros; threads t < kState of one workgroup
__device__ __forceinline__ void start_state(const float *__restrict__ init, int b, int t, double *__restrict__ state)
{
    double v = 0.0;
    if (t < 12) v = init ? (double)init[12 * (int64_t)b + t] : (t == 0 || t == 5 || t == 10 ? 1.0 : 0.0);
    state[kState * (int64_t)b + t] = v;
}

// the four taps (j0, i0) .. (j0 + 1, i0 + 1) of f blended with the weights a (across) and b (down)
template <typename Fn>
__device__ __forceinline__ float blend(Fn f, int j0, int i0, float a, float b)
{
    return blend4(f(j0, i0), f(j0, i0 + 1), f(j0 + 1, i0), f(j0 + 1, i0 + 1), a, b);
}

// The photometric term of a reference pixel of grey level gref whose point Q projects to (u, v), 1 <= u <= W - 2, 1 <= v <= H - 2,
// W, H >= 4, in the image I [H][W] (lws_ego_normal's rule from i0 on).  False, with r, w, J untouched, where a value is not finite.
__device__ __forceinline__ bool photo_term(const float *__restrict__ I, int H, int W, const Cam &c, float Qx, float Qy, float Qz, float u,
                                           float v, float gref, float huber, float &r, float &w, float (&J)[6])
{
    const int i0 = min((int)floorf(u), W - 3), j0 = min((int)floorf(v), H - 3);      // 1 <= i0 <= W - 3, 1 <= j0 <= H - 3
    const float fa = u - (float)i0, fbl = v - (float)j0;
    const float Ic = blend([&](int j, int i) { return I[(int64_t)j * W + i]; }, j0, i0, fa, fbl);
    const float gx = blend([&](int j, int i) { return 0.5f * (I[(int64_t)j * W + i + 1] - I[(int64_t)j * W + i - 1]); }, j0, i0, fa, fbl);
    const float gy = blend([&](int j, int i) { return 0.5f * (I[(int64_t)(j + 1) * W + i] - I[(int64_t)(j - 1) * W + i]); }, j0, i0, fa, fbl);
    const float rr = Ic - gref;
    const float ar = fabsf(rr);
    const float ww = ar <= huber ? 1.0f : huber / ar;
    const float ju = (gx * c.fx) / Qz, jv = (gy * c.fy) / Qz;
    const float jz = -((ju * Qx + jv * Qy) / Qz);
    const float j3 = jz * Qy - jv * Qz, j4 = ju * Qz - jz * Qx, j5 = jv * Qx - ju * Qy;
    const bool use = __builtin_isfinite(rr) && __builtin_isfinite(gx) && __builtin_isfinite(gy) && __builtin_isfinite(ju) &&
                     __builtin_isfinite(jv) && __builtin_isfinite(jz) && __builtin_isfinite(j3) && __builtin_isfinite(j4) &&
                     __builtin_isfinite(j5);
    if (use) r = rr, w = ww, J[0] = ju, J[1] = jv, J[2] = jz, J[3] = j3, J[4] = j4, J[5] = j5;
    return use;
}

// One term's 27 products added to acc: wJ_i = dw * J_i;  H_ij += wJ_i * J_j (00 01 .. 05 11 .. 55);  b_i += wJ_i * dr
__device__ __forceinline__ void add_normal(double *acc, double dw, double dr, const float (&J)[6])
{
    int n = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double wj = dw * (double)J[i];
#pragma unroll
        for (int j = i; j < 6; ++j) acc[n++] += wj * (double)J[j];
        acc[21 + i] += wj * dr;
    }
}

// thread t's share of an image's partials part[tiles][N]: those of the workgroups t, t + 256, .. in that order
template <int N>
__device__ __forceinline__ void add_partials(const double *__restrict__ part, int tiles, double (&acc)[N])
{
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    for (int j = threadIdx.x; j < tiles; j += kThreads) {
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] += part[(int64_t)j * N + k];
    }
}

// The small matrices of the update live in LDS so that no index of them needs scratch
struct SolveLds {
    double A[6][6], L[6][6], y[6], d[6], E[12], M[12], N[12];
};

// One Gauss-Newton update by one thread, in double: s = the 21 + 6 sums, m.M the motion.  A = H + damping * diag(H), Cholesky,
// delta = -(A^-1 b) to m.d, and where the step is taken st[0 .. 12) <- exp(delta) . M, st[12] = |delta|, st[13] += 1.  Returns the
// code: 0, kCodeSingular, kCodeNonFinite (m.d zeroed) or kCodeSmall (m.d kept).  m.d is zero on entry.
__device__ __forceinline__ int gauss_newton_step(const double *s, double damping, SolveLds &m, double *__restrict__ st)
{
    int code = 0;
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) m.A[i][j] = m.A[j][i] = s[k++];
    for (int i = 0; i < 6; ++i) m.A[i][i] = m.A[i][i] + damping * m.A[i][i];
    for (int j = 0; j < 6 && code == 0; ++j) {              // A = L L^T, column by column
        double a = 0.0;
        for (int q = 0; q < j; ++q) a += m.L[j][q] * m.L[j][q];
        const double p = m.A[j][j] - a;
        if (!(p > 0.0)) {
            code = kCodeSingular;
            break;
        }
        const double root = sqrt(p);
        m.L[j][j] = root;
        for (int i = j + 1; i < 6; ++i) {
            double s2 = 0.0;
            for (int q = 0; q < j; ++q) s2 += m.L[i][q] * m.L[j][q];
            m.L[i][j] = (m.A[i][j] - s2) / root;
        }
    }
    if (code != 0) return code;
    for (int i = 0; i < 6; ++i) {                           // L y = -b
        double a = 0.0;
        for (int q = 0; q < i; ++q) a += m.L[i][q] * m.y[q];
        m.y[i] = (-s[21 + i] - a) / m.L[i][i];
    }
    for (int i = 5; i >= 0; --i) {                          // L^T delta = y
        double a = 0.0;
        for (int q = i + 1; q < 6; ++q) a += m.L[q][i] * m.d[q];
        m.d[i] = (m.y[i] - a) / m.L[i][i];
    }
    const double dd = ((((m.d[0] * m.d[0] + m.d[1] * m.d[1]) + m.d[2] * m.d[2]) + m.d[3] * m.d[3]) + m.d[4] * m.d[4]) + m.d[5] * m.d[5];
    if (!__builtin_isfinite(dd)) {
        for (int i = 0; i < 6; ++i) m.d[i] = 0.0;
        return kCodeNonFinite;
    }
    if (dd < kMinStep2) return kCodeSmall;
    const double ox = m.d[3], oy = m.d[4], oz = m.d[5];
    const double t2 = (ox * ox + oy * oy) + oz * oz, th = sqrt(t2);
    double A, Bc, C;
    if (th < kSeriesBelow) {
        A = 1.0 - t2 * (1.0 / 6.0 - t2 * (1.0 / 120.0 - t2 * (1.0 / 5040.0)));
        Bc = 0.5 - t2 * (1.0 / 24.0 - t2 * (1.0 / 720.0 - t2 * (1.0 / 40320.0)));
        C = 1.0 / 6.0 - t2 * (1.0 / 120.0 - t2 * (1.0 / 5040.0 - t2 * (1.0 / 362880.0)));
    } else {
        const double sn = sin(th), cs = cos(th);
        A = sn / th, Bc = (1.0 - cs) / t2, C = (th - sn) / (t2 * th);
    }
    // K = [om]x and K^2 = om om^T - t2 I, written out; rows of R = I + A K + B K^2 and V = I + B K + C K^2
    const double K[9] = {0.0, -oz, oy, oz, 0.0, -ox, -oy, ox, 0.0};
    const double K2[9] = {ox * ox - t2, ox * oy, ox * oz, ox * oy, oy * oy - t2, oy * oz, ox * oz, oy * oz, oz * oz - t2};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double tv = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double id = i == j ? 1.0 : 0.0;
            m.E[4 * i + j] = (id + A * K[3 * i + j]) + Bc * K2[3 * i + j];
            tv += ((id + Bc * K[3 * i + j]) + C * K2[3 * i + j]) * m.d[j];
        }
        m.E[4 * i + 3] = tv;
    }
    bool finite = true;
    for (int i = 0; i < 3; ++i) {                           // N = E . M
        for (int j = 0; j < 4; ++j) {
            double a = (m.E[4 * i] * m.M[j] + m.E[4 * i + 1] * m.M[4 + j]) + m.E[4 * i + 2] * m.M[8 + j];
            if (j == 3) a += m.E[4 * i + 3];
            m.N[4 * i + j] = a;
            finite = finite && __builtin_isfinite(a);
        }
    }
    if (!finite) {
        for (int i = 0; i < 6; ++i) m.d[i] = 0.0;
        return kCodeNonFinite;
    }
    for (int i = 0; i < 12; ++i) st[i] = m.N[i];
    st[12] = sqrt(dd);
    st[13] = st[13] + 1.0;
    return 0;
}

// The pose block of M: its float32 rounding and, 12 floats on, that of its inverse formed in double
__device__ __forceinline__ void write_pose(const double *M, float *__restrict__ po)
{
    float *pi = po + kPoseInverse;
    for (int i = 0; i < 12; ++i) po[i] = (float)M[i];
    for (int i = 0; i < 3; ++i) {                           // the inverse: R^T, 0 - R^T t (so that a zero t gives +0, not -0)
        for (int j = 0; j < 3; ++j) pi[4 * i + j] = (float)M[4 * j + i];
        pi[4 * i + 3] = (float)(0.0 - ((M[i] * M[3] + M[4 + i] * M[7]) + M[8 + i] * M[11]));
    }
}

}  // namespace lws::motionkit
