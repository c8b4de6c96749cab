// The background fill of a row, shared by k_lr_check (lws_lrcheck.hip) and k_sp_apply (lws_speckle.hip): pixels to trust keep
// their value, every other pixel takes the smaller of the values at the nearest trusted pixel on its left and on its right (the
// left one on a tie), one side's value if only that side has one, 0.0f if the row has none.  One workgroup of kFillThreads threads
// owns the row; thread t owns the quads t, t + 256, ... (pixels 4q .. 4q + 3), so W <= kFillMaxW gives at most 8 quads per thread
// and the "trusted" flags of its pixels fit in one 32-bit word (bit 4k + i for pixel i of its k-th quad).
#ifndef LWS_ROWFILL_H
#define LWS_ROWFILL_H
#include "lws_common.h"

namespace lws {

namespace rowfill {

constexpr int kFillThreads = 256;
constexpr int kFillWaves = kFillThreads / 64;
constexpr int kFillMaxW = 8192;                             // a row of floats + two int per quad: 48 KiB of LDS at most
constexpr int kNone = 0x7fffffff;                           // "no trusted pixel to the right"

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// Stage `n` floats of a row into LDS: float4 where the row is 16-byte aligned, scalar for a misaligned row and the tail.
__device__ __forceinline__ void stage_row(float *__restrict__ dst, const float *__restrict__ src, int W, int nq)
{
    const bool vec = aligned16(src);
    for (int q = threadIdx.x; q < nq; q += kFillThreads) {
        const int x = 4 * q;
        if (vec && x + 4 <= W) {
            *reinterpret_cast<float4 *>(dst + x) = *reinterpret_cast<const float4 *>(src + x);
        } else {
            for (int i = 0; i < 4 && x + i < W; ++i) dst[x + i] = src[x + i];
        }
    }
}

__device__ __forceinline__ void store_quad(float *__restrict__ p, int x, int W, bool vec, float v0, float v1, float v2, float v3)
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

// The last / first trusted pixel of the quad at x whose flags are ok[0..3] (-1 / kNone if it has none)
__device__ __forceinline__ void quad_last_first(const bool ok[4], int x, int &last, int &first)
{
    last = -1, first = kNone;
#pragma unroll
    for (int i = 0; i < 4; ++i) last = ok[i] ? x + i : last;
#pragma unroll
    for (int i = 3; i >= 0; --i) first = ok[i] ? x + i : first;
}

// Called by all kFillThreads threads once s_row holds the row's values and s_last[q] / s_first[q] the last / first trusted pixel
// of every quad; a __syncthreads() of the caller's lies between the writes of s_last / s_first and the call (s_row may still be
// being staged: it is read behind the two barriers in here).  s_wl, s_wf: kFillWaves ints of LDS each.  Writes the filled row to out.
__device__ __forceinline__ void fill_row(const float *__restrict__ s_row, int *__restrict__ s_last, int *__restrict__ s_first,
                                         int *__restrict__ s_wl, int *__restrict__ s_wf, unsigned bits, int nq, int W,
                                         float *__restrict__ out, bool vout)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // inclusive max-scan of last (left to right), inclusive min-scan of first (right to left) over the quads: each thread a
    // contiguous chunk of quads, the chunks' aggregates across the wave by shuffles, across waves through LDS
    const int per = (nq + kFillThreads - 1) / kFillThreads;
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
    for (int w = 0; w < kFillWaves; ++w) {
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
    for (int k = 0, q = t; q < nq; ++k, q += kFillThreads) {
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

}  // namespace rowfill

}  // namespace lws

#endif  // LWS_ROWFILL_H
