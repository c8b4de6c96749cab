// A TSDF volume seen through an integer offset, written to a second volume: the shift of a volume that follows the camera, the boxes
// cut out of it before they are shifted away, a resize.  Contract: include/lwsnet_tsdf_window.h; the rule moves bits and compares
// Wt with zero, so tests/tsdf_window_reference.py restates it in a few lines of numpy.
//
// Launches (a fixed list: it depends on the arguments, never on the data; nothing is read back):
//   k_tw_zero     (counts given) counts[0] = counts[1] = 0 -- a kernel, as k_ts_zero of lws_tsdf.hip
//   k_tw_window   one thread per four voxels along x of the DESTINATION, as the integrate sweep, so that every store is a whole
//                 16-byte word wherever the destination allows it; at most kMaxBlocks workgroups stride over the quads.  The source
//                 quad begins at x + sx: it is loaded as 16-byte words where it lies inside its row and is aligned, and voxel by
//                 voxel otherwise.  Wt, T and C of a quad are loaded together, before the first use, live or not: the plain form.
//                 Loading T and C only behind the test of Wt was measured too and is no faster at the aligned shift.
//                 12 bytes in and 12 bytes out a voxel with colour.
// Determinism: a voxel belongs to one thread; what crosses threads is the integer add of `counts`.  0 bytes of scratch.
#include "lws_tsdfkit.h"
#include "lwsnet_tsdf_window.h"

namespace lws {

namespace {

using namespace tsdfkit;                                    // kMaxGrid, aligned, Buf, check_no_overlap
using namespace packkit;                                    // kThreads, kWaves
using u64 = unsigned long long;

constexpr int kMaxShift = 4096;
constexpr int kMaxBlocks = 2048;                            // 256 CUs x 8 workgroups: the rest of the quads is strided over

struct WinArgs {                                            // by value in the kernel arguments
    const float *T, *Wt;
    const unsigned *C;                                      // one word {r, g, b, a} per voxel
    int Gx, Gy, Gz, sx, sy, sz;
    float *T2, *Wt2;
    unsigned *C2;
    int Dx, Dy, Dz, nq;                                     // nq: the quads of a destination row
    u64 *counts;
};

// grid (1): counts[0] = counts[1] = 0
__global__ void k_tw_zero(u64 *__restrict__ counts)
{
    if (threadIdx.x < 2) counts[threadIdx.x] = 0;
}

// grid (min(ceil(Dz * Dy * nq / 256), kMaxBlocks)): a thread takes the quads q, q + the grid's threads, ...  COLOUR: C and C2 are given.
template <bool COLOUR>
__global__ __launch_bounds__(kThreads) void k_tw_window(WinArgs a)
{
    __shared__ int s_n[2][kWaves];
    const int64_t quads = (int64_t)a.Dz * a.Dy * a.nq, stride = (int64_t)gridDim.x * kThreads;
    int n_live = 0, n_all = 0;                              // < 2^31: the destination holds fewer voxels
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < quads; q += stride) {
        const int64_t row = q / a.nq;
        const int x = 4 * (int)(q - row * a.nq);
        const int iz = (int)(row / a.Dy), iy = (int)(row - (int64_t)iz * a.Dy);
        const int n = min(4, a.Dx - x);                     // the quad's voxels: x .. x + n - 1 < Dx
        const int jx = x + a.sx, jy = iy + a.sy, jz = iz + a.sz;
        const bool row_in = jy >= 0 && jy < a.Gy && jz >= 0 && jz < a.Gz;
        float To[4] = {0.0f, 0.0f, 0.0f, 0.0f}, Wo[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        unsigned Co[4] = {0u, 0u, 0u, 0u};
        unsigned live = 0u;                                 // bit i: voxel x + i is live
        if (row_in && jx + n > 0 && jx < a.Gx) {            // some voxel of the quad has its source inside
            const int64_t src = ((int64_t)jz * a.Gy + jy) * a.Gx + jx;      // (jx < 0: before the row's first voxel; only sp[i] with 0 <= jx + i < Gx is read)
            const float *Tp = a.T + src, *Wp = a.Wt + src;
            const unsigned *Cp = COLOUR ? a.C + src : nullptr;
            const bool inside = n == 4 && jx >= 0 && jx + 4 <= a.Gx;
            // all three loads are issued before the first use: one trip to memory a quad, whatever its voxels turn out to be
            if (inside && aligned(Wp, 16)) {
                const float4 wv = *reinterpret_cast<const float4 *>(Wp);
                Wo[0] = wv.x, Wo[1] = wv.y, Wo[2] = wv.z, Wo[3] = wv.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < n && jx + i >= 0 && jx + i < a.Gx) Wo[i] = Wp[i];
            }
            if (inside && aligned(Tp, 16)) {
                const float4 tv = *reinterpret_cast<const float4 *>(Tp);
                To[0] = tv.x, To[1] = tv.y, To[2] = tv.z, To[3] = tv.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < n && jx + i >= 0 && jx + i < a.Gx) To[i] = Tp[i];
            }
            if (COLOUR) {
                if (inside && aligned(Cp, 16)) {
                    const uint4 cv = *reinterpret_cast<const uint4 *>(Cp);
                    Co[0] = cv.x, Co[1] = cv.y, Co[2] = cv.z, Co[3] = cv.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (i < n && jx + i >= 0 && jx + i < a.Gx) Co[i] = Cp[i];
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool in = i < n && jx + i >= 0 && jx + i < a.Gx;
                if (in && !(Wo[i] == 0.0f)) live |= 1u << i;
                else To[i] = 0.0f, Wo[i] = 0.0f, Co[i] = 0u;        // (-0.0 is dead and leaves as +0.0; what T and C held there is dropped)
            }
        }
        const int64_t dst = row * a.Dx + x;
        float *T2p = a.T2 + dst, *W2p = a.Wt2 + dst;
        unsigned *C2p = COLOUR ? a.C2 + dst : nullptr;
        if (n == 4 && aligned(T2p, 16)) {
            *reinterpret_cast<float4 *>(T2p) = make_float4(To[0], To[1], To[2], To[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < n) T2p[i] = To[i];
        }
        if (n == 4 && aligned(W2p, 16)) {
            *reinterpret_cast<float4 *>(W2p) = make_float4(Wo[0], Wo[1], Wo[2], Wo[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < n) W2p[i] = Wo[i];
        }
        if (COLOUR) {
            if (n == 4 && aligned(C2p, 16)) {
                *reinterpret_cast<uint4 *>(C2p) = make_uint4(Co[0], Co[1], Co[2], Co[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < n) C2p[i] = Co[i];
            }
        }
        n_live += __builtin_popcount(live);
        n_all += n;
    }
    if (a.counts) {                                         // (uniform) every thread of the workgroup is here: the loop has no barrier
        const int live = block_sum(n_live, s_n[0]), all = block_sum(n_all, s_n[1]);
        if (threadIdx.x == 0) {
            if (live) __hip_atomic_fetch_add(a.counts, (u64)live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (all - live) __hip_atomic_fetch_add(a.counts + 1, (u64)(all - live), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

int check_dims(const char *who, const char *what, int X, int Y, int Z)
{
    LWS_CHECK_ARG(X >= 2 && X <= kMaxGrid && Y >= 2 && Y <= kMaxGrid && Z >= 2 && Z <= kMaxGrid, "%s: bad %s volume %dx%dx%d (each in 2..%d)", who,
                  what, X, Y, Z, kMaxGrid);
    LWS_CHECK_ARG((int64_t)X * Y * Z < ((int64_t)1 << 31), "%s: the %s volume %dx%dx%d must hold fewer than 2^31 voxels", who, what, X, Y, Z);
    return LWS_OK;
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int lws_tsdf_window(const float *T, const float *Wt, const uint8_t *C, int Gx, int Gy, int Gz, int sx, int sy, int sz, float *T2, float *Wt2,
                    uint8_t *C2, int Dx, int Dy, int Dz, int64_t *counts, void *stream)
{
    const char *who = "tsdf_window";
    LWS_CHECK_ARG(T && Wt && T2 && Wt2, "%s: T, Wt, T2 and Wt2 must not be null", who);
    LWS_CHECK_ARG((C != nullptr) == (C2 != nullptr), "%s: C and C2 must be given together (both null: no colour)", who);
    LWS_CHECK_RC(check_dims(who, "source", Gx, Gy, Gz));
    LWS_CHECK_RC(check_dims(who, "destination", Dx, Dy, Dz));
    LWS_CHECK_ARG(sx >= -kMaxShift && sx <= kMaxShift && sy >= -kMaxShift && sy <= kMaxShift && sz >= -kMaxShift && sz <= kMaxShift,
                  "%s: bad shift (%d, %d, %d) (each in -%d..%d)", who, sx, sy, sz, kMaxShift, kMaxShift);
    LWS_CHECK_ARG(aligned(T, 4) && aligned(Wt, 4) && aligned(C, 4) && aligned(T2, 4) && aligned(Wt2, 4) && aligned(C2, 4) && aligned(counts, 8),
                  "%s: T / Wt / C / T2 / Wt2 / C2 must be 4-byte, counts 8-byte aligned", who);
    const int64_t vox = (int64_t)Gx * Gy * Gz, vox2 = (int64_t)Dx * Dy * Dz;
    const Buf bufs[] = {{T2, 4 * vox2, "T2"}, {Wt2, 4 * vox2, "Wt2"}, {C2, 4 * vox2, "C2"}, {counts, 16, "counts"}, {T, 4 * vox, "T"},
                        {Wt, 4 * vox, "Wt"}, {C, 4 * vox, "C"}};
    LWS_CHECK_RC(check_no_overlap(who, bufs, 7, 4));

    const int nq = (Dx + 3) / 4;
    const WinArgs a = {T, Wt, reinterpret_cast<const unsigned *>(C), Gx, Gy, Gz, sx, sy, sz, T2, Wt2, reinterpret_cast<unsigned *>(C2), Dx, Dy, Dz, nq,
                       reinterpret_cast<u64 *>(counts)};
    hipStream_t st = (hipStream_t)stream;
    if (counts) {
        hipLaunchKernelGGL(k_tw_zero, dim3(1), dim3(64), 0, st, a.counts);
        LWS_LAUNCH_CHECK();
    }
    const int64_t blocks = ((int64_t)Dz * Dy * nq + kThreads - 1) / kThreads;
    const dim3 grid((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks));
    if (C)
        hipLaunchKernelGGL(k_tw_window<true>, grid, dim3(kThreads), 0, st, a);
    else
        hipLaunchKernelGGL(k_tw_window<false>, grid, dim3(kThreads), 0, st, a);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // extern "C"
