// The pieces of the count -> scan -> ranked-scatter kernels, which pack records in a fixed order without an atomic: lws_point_cloud
// (lws_geometry.hip), lws_surface_mesh (lws_mesh.hip), lws_tsdf_points (lws_tsdf.hip) and the numbering of lws_objects and
// lws_movers (lws_cclkit.h).  The count is opkit::block_sum; here are the exclusive scan of one value per thread, the scan of an array by
// one workgroup, and the rank of a thread's set bits from wave ballots.  All of it is integer arithmetic in thread order, for
// workgroups of 256 threads; s_w is always kWaves words of the caller's LDS.
#pragma once
#include "lws_opkit.h"

namespace lws::packkit {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// Behind a barrier that follows the waves writing their totals to s_w: `part`, a thread's place among its own wave's, becomes its
// place in the sequence: plus `carry` (uniform: everything before this workgroup-wide round) plus the earlier waves' totals.
// carry gains the round's total.
template <typename T>
__device__ __forceinline__ T add_earlier_waves(T part, const T *s_w, T &carry)
{
    const int wave = threadIdx.x >> 6;
    T before = carry, total = carry;
    for (int w = 0; w < kWaves; ++w) {
        before += w < wave ? s_w[w] : 0;
        total += s_w[w];
    }
    carry = total;
    return before + part;
}

// carry + the exclusive scan of `mine` over the workgroup's threads in thread order; carry gains the workgroup's total.  Every
// thread calls it; one barrier inside, and the caller synchronises before s_w is written again.
template <typename T>
__device__ __forceinline__ T block_scan(T mine, T *s_w, T &carry)
{
    const int lane = threadIdx.x & 63;
    T inc = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(inc, o, 64);
        inc += lane >= o ? u : 0;
    }
    if (lane == 63) s_w[threadIdx.x >> 6] = inc;
    __syncthreads();
    return add_earlier_waves(inc - mine, s_w, carry);
}

// r[0 .. n) -> its exclusive scan, in place, by one workgroup in chunks of 256; returns the total (in every thread)
template <typename T>
__device__ __forceinline__ T row_scan(T *__restrict__ r, int n, T *s_w)
{
    const unsigned count = n > 0 ? n : 0;                   // (unsigned: y0 + 255 does not wrap for an n just below 2^31)
    T carry = 0;                                            // uniform: the sum of the chunks before
    for (unsigned y0 = 0; y0 < count; y0 += kThreads) {
        const unsigned y = y0 + threadIdx.x;
        const T at = block_scan<T>(y < count ? r[y] : 0, s_w, carry);
        if (y < count) r[y] = at;
        __syncthreads();                                    // s_w is rewritten by the next chunk
    }
    return carry;
}

// The rank of a thread's first set bit among the set bits of its wave's threads in thread order (N bit slots per thread: one
// ballot per slot); wave_n = the wave's set bits.  A thread's later bits follow its first.
template <int N>
__device__ __forceinline__ int wave_rank(unsigned bits, int &wave_n)
{
    const unsigned long long below = (1ull << (threadIdx.x & 63)) - 1ull;
    int rank = 0;
    wave_n = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const unsigned long long m = __ballot((bits >> i) & 1u);
        rank += __popcll(m & below);
        wave_n += __popcll(m);
    }
    return rank;
}

// ... among those of the workgroup's threads, plus carry, which gains the workgroup's set bits.  Barriers as block_scan.
template <int N>
__device__ __forceinline__ int block_rank(unsigned bits, int *s_w, int &carry)
{
    int wave_n;
    const int rank = wave_rank<N>(bits, wave_n);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = wave_n;
    __syncthreads();
    return add_earlier_waves(rank, s_w, carry);
}

}  // namespace lws::packkit
