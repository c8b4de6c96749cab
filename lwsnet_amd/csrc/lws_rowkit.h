// The row toolkit of the kernels shaped "one workgroup of kThreads threads per image row, thread t owns the quads t, t + 256, ...
// (pixels 4q .. 4q + 3)": k_lr_check (lws_lrcheck.hip), k_occ_check (lws_occlusion.hip) and k_sp_apply (lws_speckle.hip).  Each of
// them is its own arithmetic (the codes of a quad) between these pieces: the quad load, the code store, the "keep d where the code
// is 1" store, the kept flags of a thread's quads, the row totals, and the background fill of a row: pixels to trust keep their
// value, every other pixel takes the smaller of the values at the nearest trusted pixel on its left and on its right (the left one
// on a tie), one side's value if only that side has one, 0.0f if the row has none.
// No pointer a caller may alias with an output is __restrict__ here: out may be disp, mask_out may be mask, out[s] may be dL[s].
#ifndef LWS_ROWKIT_H
#define LWS_ROWKIT_H
#include "lws_opkit.h"

namespace lws {

namespace rowkit {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxW = 8192;                                 // a row of floats + two int per quad: 48 KiB of LDS at most
constexpr int kNone = 0x7fffffff;                           // "no trusted pixel to the right"
using opkit::aligned;

// Stage `n` floats of a row into LDS: float4 where the row is 16-byte aligned, scalar for a misaligned row and the tail.
__device__ __forceinline__ void stage_row(float *__restrict__ dst, const float *__restrict__ src, int W, int nq)
{
    const bool vec = aligned(src, 16);
    for (int q = threadIdx.x; q < nq; q += kThreads) {
        const int x = 4 * q;
        if (vec && x + 4 <= W) {
            *reinterpret_cast<float4 *>(dst + x) = *reinterpret_cast<const float4 *>(src + x);
        } else {
            for (int i = 0; i < 4 && x + i < W; ++i) dst[x + i] = src[x + i];
        }
    }
}

// The quad at x of a row (global memory or LDS): one float4 where `vec` (the row is 16-byte aligned) and the quad is whole,
// scalar otherwise, with `pad` for the columns >= W.  The condition is spelt as one compare so that the compiler lays the float4
// load out first: behind the scalar loads it waits for vmcnt(0), that is for the stores of the thread's previous quad.
__device__ __forceinline__ void load_quad(const float *p, int x, int W, bool vec, float pad, float d[4])
{
    if (x + 4 <= (vec ? W : 0)) {
        const float4 v = *reinterpret_cast<const float4 *>(p + x);
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = x + i < W ? p[x + i] : pad;
    }
}

__device__ __forceinline__ void store_quad(float *p, int x, int W, bool vec, float v0, float v1, float v2, float v3)
{
    if (vec && x + 4 <= W) {
        *reinterpret_cast<float4 *>(p + x) = make_float4(v0, v1, v2, v3);
    } else {
        const float v[4] = {v0, v1, v2, v3};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i < W) p[x + i] = v[i];
    }
}

// The four codes of the quad at x: one uchar4 where `vec` (the row is 4-byte aligned) and the quad is whole, scalar otherwise.
__device__ __forceinline__ void store_codes(uint8_t *p, int x, int W, bool vec, const int c[4])
{
    if (vec && x + 4 <= W) {
        *reinterpret_cast<uchar4 *>(p + x) = make_uchar4((uint8_t)c[0], (uint8_t)c[1], (uint8_t)c[2], (uint8_t)c[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i < W) p[x + i] = (uint8_t)c[i];
    }
}

// The output without a fill: d where the code is 1, 0.0f elsewhere.
__device__ __forceinline__ void store_kept(float *p, int x, int W, bool vec, const int c[4], const float d[4])
{
    store_quad(p, x, W, vec, c[0] == 1 ? d[0] : 0.0f, c[1] == 1 ? d[1] : 0.0f, c[2] == 1 ? d[2] : 0.0f, c[3] == 1 ? d[3] : 0.0f);
}

// The last / first trusted pixel of the quad at x whose flags are ok[0..3] (-1 / kNone if it has none)
__device__ __forceinline__ void quad_last_first(const bool ok[4], int x, int &last, int &first)
{
    int l = -1, f = kNone;                                  // (registers: last and first may be words of LDS)
#pragma unroll
    for (int i = 0; i < 4; ++i) l = ok[i] ? x + i : l;
#pragma unroll
    for (int i = 3; i >= 0; --i) f = ok[i] ? x + i : f;
    last = l, first = f;
}

// The kept (code == 1: "trusted") pixels of a thread's quads: their number, and bit 4k + i of `bits` for pixel i of its k-th quad.
// The word holds the 32 flags of 8 quads, which is every quad of a thread while W <= kMaxW.  Its readers (last_first, fill_row)
// run only under that bound, which the entry points check; k_sp_apply without a fill takes any W and reads `count` alone, so
// there the flags of a ninth quad wrap onto the first's (the shift is masked to stay defined) and are never looked at.
struct KeptFlags {
    static_assert(kMaxW == 4 * 8 * kThreads, "8 quads per thread at kMaxW: the 32 flags of KeptFlags::bits");
    unsigned bits = 0;
    int count = 0;

    // the thread's k-th quad, whose codes are c; hands back the flags ok[i] = (c[i] == 1) it recorded
    __device__ __forceinline__ void add(int k, const int c[4], bool ok[4])
    {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ok[i] = c[i] == 1;
            count += ok[i] ? 1 : 0;
            bits |= (ok[i] ? 1u : 0u) << ((4 * k + i) & 31);
        }
    }
    __device__ __forceinline__ void add(int k, const int c[4])
    {
        bool ok[4];
        add(k, c, ok);
    }

    // the last / first kept pixel of the thread's k-th quad, which lies at x, for a kernel that needs them after its quad loop
    __device__ __forceinline__ void last_first(int k, int x, int &last, int &first) const
    {
        const unsigned cb = bits >> (4 * k);
        const bool ok[4] = {(cb & 1u) != 0, (cb & 2u) != 0, (cb & 4u) != 0, (cb & 8u) != 0};
        quad_last_first(ok, x, last, first);
    }
};

// The row totals of N per-thread counters, in the fixed order wave shuffle -> one slot per wave and counter -> (w0 + w1) + (w2 + w3).
// wave_sums leaves the waves' sums in slots[kWaves * N] (the caller's LDS); behind a __syncthreads() row_total(slots, j) is the
// row's j-th total in every thread.
template <int N>
__device__ __forceinline__ void wave_sums(const int (&n)[N], int *slots)
{
    int v[N];
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = n[j];
    opkit::wave_sum_n(v);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int j = 0; j < N; ++j) slots[(threadIdx.x >> 6) * N + j] = v[j];
}

template <int N>
__device__ __forceinline__ int row_total(const int *slots, int j)
{
    static_assert(kWaves == 4, "the fixed order of the sum");
    return opkit::sum4(slots[j], slots[N + j], slots[2 * N + j], slots[3 * N + j]);
}

// Called by all kThreads threads once s_row holds the row's values and s_last[q] / s_first[q] the last / first trusted pixel
// of every quad; a __syncthreads() of the caller's lies between the writes of s_last / s_first and the call (s_row may still be
// being staged: it is read behind the two barriers in here).  s_wl, s_wf: kWaves ints of LDS each.  Writes the filled row to out.
__device__ __forceinline__ void fill_row(const float *__restrict__ s_row, int *__restrict__ s_last, int *__restrict__ s_first,
                                         int *__restrict__ s_wl, int *__restrict__ s_wf, unsigned bits, int nq, int W,
                                         float *__restrict__ out, bool vout)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // inclusive max-scan of last (left to right), inclusive min-scan of first (right to left) over the quads: each thread a
    // contiguous chunk of quads, the chunks' aggregates across the wave by shuffles, across waves through LDS
    const int per = (nq + kThreads - 1) / kThreads;
    const int q0 = min(t * per, nq), q1 = min(q0 + per, nq);
    int agg_l = -1, agg_f = kNone;
    for (int j = q0; j < q1; ++j) {
        agg_l = max(agg_l, s_last[j]);
        agg_f = min(agg_f, s_first[j]);
    }
    int inc_l = agg_l, inc_f = agg_f;
    for (int o = 1; o < 64; o <<= 1) {
        const int vl = __shfl_up(inc_l, o, 64), vf = __shfl_down(inc_f, o, 64);
        inc_l = lane >= o ? max(inc_l, vl) : inc_l;
        inc_f = lane + o < 64 ? min(inc_f, vf) : inc_f;
    }
    if (lane == 63) s_wl[wave] = inc_l;
    if (lane == 0) s_wf[wave] = inc_f;
    int exc_l = __shfl_up(inc_l, 1, 64), exc_f = __shfl_down(inc_f, 1, 64);
    exc_l = lane == 0 ? -1 : exc_l;
    exc_f = lane == 63 ? kNone : exc_f;
    __syncthreads();
    for (int w = 0; w < kWaves; ++w) {
        exc_l = w < wave ? max(exc_l, s_wl[w]) : exc_l;
        exc_f = w > wave ? min(exc_f, s_wf[w]) : exc_f;
    }
    for (int j = q0; j < q1; ++j) {
        exc_l = max(exc_l, s_last[j]);
        s_last[j] = exc_l;
    }
    for (int j = q1 - 1; j >= q0; --j) {
        exc_f = min(exc_f, s_first[j]);
        s_first[j] = exc_f;
    }
    __syncthreads();

    // trusted pixels keep d, the others min(d at the nearest trusted pixel on the left, on the right); one side only: that side's
    // value; neither: 0.  Ties keep the left value.
    for (int k = 0, q = t; q < nq; ++k, q += kThreads) {
        const int x = 4 * q;
        const unsigned cb = bits >> (4 * k);
        int prev = q > 0 ? s_last[q - 1] : -1;
        int nxt[4];
        int n = q + 1 < nq ? s_first[q + 1] : kNone;
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            n = (cb >> i) & 1 ? x + i : n;
            nxt[i] = n;
        }
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if ((cb >> i) & 1) {
                prev = x + i;
                v[i] = s_row[x + i];
            } else {
                const float vl = prev >= 0 ? s_row[prev] : 0.0f;
                const float vr = nxt[i] != kNone ? s_row[nxt[i]] : 0.0f;
                v[i] = prev >= 0 ? (nxt[i] != kNone ? (vr < vl ? vr : vl) : vl) : (nxt[i] != kNone ? vr : 0.0f);
            }
        }
        store_quad(out, x, W, vout, v[0], v[1], v[2], v[3]);
    }
}

}  // namespace rowkit

}  // namespace lws

#endif  // LWS_ROWKIT_H
