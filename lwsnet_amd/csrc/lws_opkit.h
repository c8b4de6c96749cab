// The toolkit of the post-network ops (lws_metrics, lws_lrcheck, lws_occlusion, lws_geometry, lws_mesh, lws_ground, lws_stixels,
// lws_objects, lws_temporal, lws_egomotion, lws_tsdf, lws_speckle, lws_wmedian, lws_rectify, lws_confidence, lws_sparsification,
// lws_photometric; lws_rowkit.h, lws_geomkit.h and lws_packkit.h build on it).  An op is its own arithmetic and its own limits
// between these pieces.  Host half: the argument checks their entry points share, under the caller's name `who`, so that a text is
// written once.  Device half: the 64-lane sum, the four-wave combine in its fixed order, the workgroup's sum made of the two, the
// monotone key of a float, and the ground-truth contract of the evaluation kernels.
// The translation units of the forward (feature2d, refine, conv3d, volume, regress, forward, params, api, pool) do not include this header.
#pragma once
#include "lws_common.h"

namespace lws::opkit {

// a check function's result handed on: LWS_CHECK_ARG one level up
#define LWS_CHECK_RC(call)                \
    do {                                  \
        const int rc_ = (call);           \
        if (rc_ != LWS_OK) return rc_;    \
    } while (0)

// ---- host half ----
__host__ __device__ __forceinline__ bool aligned(const void *p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }   // n = 2^k

// a part of a workspace, in bytes: the next part starts 256-byte aligned
constexpr int64_t round256(int64_t n) { return (n + 255) / 256 * 256; }

// true when the byte ranges [a, a + na) and [b, b + nb) intersect (a null pointer is no range)
static inline bool overlap(const void *a, int64_t na, const void *b, int64_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

struct Buf { const void *p; int64_t bytes; const char *name; };

// Rejects the overlapping pairs of bufs[0 .. n): each of the n_written leading entries (the buffers a call writes) against every
// entry behind it, reported as "<who>: <the later name> and <the earlier name> overlap".  same[0 .. n_same): index pairs {i, j},
// i < j, that may be one and the same pointer (an in-place call); they may still not overlap in part.
static inline int check_no_overlap(const char *who, const Buf *bufs, int n, int n_written, const int (*same)[2] = nullptr, int n_same = 0)
{
    for (int i = 0; i < n_written; ++i)
        for (int j = i + 1; j < n; ++j) {
            const Buf &a = bufs[i], &b = bufs[j];
            bool same_ok = false;
            for (int k = 0; k < n_same; ++k) same_ok = same_ok || (same[k][0] == i && same[k][1] == j && a.p == b.p);
            LWS_CHECK_ARG(same_ok || !overlap(a.p, a.bytes, b.p, b.bytes), "%s: %s and %s overlap", who, b.name, a.name);
        }
    return LWS_OK;
}

static inline bool shape_ok(int B, int H, int W) { return B >= 1 && B <= 65535 && H >= 1 && W >= 1; }   // B: a grid's y or z extent

// pixel_bits > 0: H * W < 2^pixel_bits as well (an image indexed with an int: 31)
static inline int check_image_shape(const char *who, int B, int H, int W, int pixel_bits)
{
    LWS_CHECK_ARG(shape_ok(B, H, W), "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    LWS_CHECK_ARG(pixel_bits <= 0 || (int64_t)H * W < ((int64_t)1 << pixel_bits), "%s: H*W = %dx%d must be < 2^%d", who, H, W, pixel_bits);
    return LWS_OK;
}

constexpr float kFloatMax = 3.4028234663852886e38f;
static inline bool finite_nonneg(float x) { return x >= 0.0f && x <= kFloatMax; }   // (false for NaN)
static inline bool finite_pos(float x) { return x > 0.0f && x <= kFloatMax; }
static inline bool finite_any(float x) { return x >= -kFloatMax && x <= kFloatMax; }

static inline int check_fill(const char *who, int fill)
{
    LWS_CHECK_ARG(fill == 0 || fill == 1, "%s: fill %d (0 = zero, 1 = background fill)", who, fill);
    return LWS_OK;
}

// The argument checks lws_lr_check and lws_occlusion_check share; `why` is the parenthesis that says what the caller keeps in LDS,
// so that W <= max_w.  dRm: NULL for a check without right-view maps.
static inline int check_row_check_args(const char *who, const char *why, int max_w, const float *const dL[4], const float *const dRm[4],
                                       int nmaps, int B, int H, int W, float tau, int fill, float *const out[4], uint8_t *const mask[4])
{
    LWS_CHECK_ARG(nmaps >= 1 && nmaps <= 4, "%s: nmaps %d outside 1..4", who, nmaps);
    LWS_CHECK_RC(check_image_shape(who, B, H, W, 0));
    LWS_CHECK_ARG(W <= max_w, "%s: W=%d exceeds %d %s", who, W, max_w, why);
    LWS_CHECK_ARG(finite_nonneg(tau), "%s: tau must be finite and >= 0, got %g", who, (double)tau);
    LWS_CHECK_RC(check_fill(who, fill));
    for (int s = 0; s < nmaps; ++s)
        LWS_CHECK_ARG(dL[s] && (!dRm || dRm[s]) && out[s] && mask[s], "%s: map %d has a null pointer", who, s);
    return LWS_OK;
}

// The ground truth of the evaluation kernels (lws_stage_metrics, lws_sparsification): gt [B,Hg,W] against the rows
// row_offset .. Hp - 1 of [B,Hp,W] maps.  rows == NULL: the workspace query, which knows the ground truth's size only.
constexpr int64_t kMaxPixels = (int64_t)1 << 40;            // blocks per image stay far below the grid limit
struct GtRows { int Hp, row_offset; float maxdisp; int mode; };
static inline int check_gt_args(const char *who, int B, int Hg, int W, const GtRows *rows)
{
    if (!rows) {
        LWS_CHECK_ARG(shape_ok(B, Hg, W), "%s: bad shape B=%d %dx%d", who, B, Hg, W);
    } else {
        LWS_CHECK_ARG(shape_ok(B, Hg, W), "%s: bad shape B=%d Hg=%d W=%d", who, B, Hg, W);
        LWS_CHECK_ARG(rows->row_offset >= 0, "%s: row_offset %d < 0", who, rows->row_offset);
        LWS_CHECK_ARG(rows->Hp == Hg + rows->row_offset, "%s: Hp=%d must be Hg + row_offset = %d + %d", who, rows->Hp, Hg, rows->row_offset);
        LWS_CHECK_ARG(rows->mode == 0 || rows->mode == 1, "%s: mode %d (0 = KITTI 3-px, 1 = EPE)", who, rows->mode);
        LWS_CHECK_ARG(rows->maxdisp > 0.0f, "%s: maxdisp must be > 0, got %g", who, (double)rows->maxdisp);      // (false for NaN)
    }
    LWS_CHECK_ARG((int64_t)Hg * W <= kMaxPixels, "%s: %dx%d is too large", who, Hg, W);
    return LWS_OK;
}

// ---- device half ----
// The sum over the 64 lanes of a wave: lane 0 holds it (the other lanes a partial sum).  For a float type this IS the order of the
// additions: o = 32, 16, .., 1, lane l adding lane l + o's value.
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// N sums side by side through the same tree
template <typename T, int N>
__device__ __forceinline__ void wave_sum_n(T (&v)[N])
{
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] += __shfl_down(v[j], o, 64);
}

// The sums of the four waves of a 256-thread workgroup, in the one fixed order
template <typename T>
__device__ __forceinline__ T sum4(const T &w0, const T &w1, const T &w2, const T &w3) { return (w0 + w1) + (w2 + w3); }

// The sum of v over the 256 threads of a workgroup in that fixed order: wave_sum, one word per wave in s[0 .. 4) (the caller's LDS),
// a barrier, sum4.  Every thread calls it and every thread holds the result; the caller synchronises before s is written again.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T *s)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return sum4(s[0], s[1], s[2], s[3]);
}

// N sums side by side: the waves' sums to s[wave][j] and a barrier; sum j is then block_total(s, j) in every thread
// (rowkit::wave_sums / row_total are this layout for int, with the barrier left to the row kernel, which has one anyway)
template <typename T, int N>
__device__ __forceinline__ void block_sum_n(T (&v)[N], T (*s)[N])
{
    wave_sum_n(v);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) s[threadIdx.x >> 6][j] = v[j];
    }
    __syncthreads();
}
template <typename T, int N>
__device__ __forceinline__ T block_total(const T (*s)[N], int j) { return sum4(s[0][j], s[1][j], s[2][j], s[3][j]); }

// The order-preserving word of a float: unsigned compare of keys == float compare of values (-0.0 below +0.0).  0 is no float's
// key but a NaN's (bits 0xffffffff), and NaNs are never keyed, so a caller may let 0 mean "empty".
__device__ __forceinline__ unsigned key_of(float d)
{
    const unsigned u = __float_as_uint(d);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// One pixel against its ground truth g, the reference's float32 numpy: valid = the mask of the mode (0 = KITTI: 0 < g < md,
// 1 = EPE: g < md), e = |p - g|, bad = valid & e > 3 & e / g > 0.05.  One IEEE float32 operation each; the ordered compares are
// false on NaN, so a NaN or +inf g is never valid and a NaN p is never bad.
struct GtPixel { bool valid, bad; float e; };
__device__ __forceinline__ GtPixel gt_pixel(float p, float g, float md, int mode)
{
    const bool valid = (mode == 0 ? g > 0.0f : true) && g < md;
    const float e = fabsf(p - g);
    return GtPixel{valid, valid && e > 3.0f && e / g > 0.05f, e};
}

// The quad at pixel i of an image of npix pixels, of its ground truth g and of N maps m[s]: one float4 each where `vec` (every base
// is 16-byte aligned) and the quad is whole; scalar otherwise (a misaligned image, or the last, partial quad before the
// image's end), where a missing pixel has gt = NaN, which no mode counts as valid, and the maps' value 0.  i < npix.
template <int N>
__device__ __forceinline__ void load_gt_quad(const float *g, const float *const (&m)[N], int64_t i, int64_t npix, bool vec,
                                             float4 &gq, float4 (&mq)[N])
{
    if (i + 4 <= (vec ? npix : 0)) {                        // one compare, as rowkit::load_quad: the float4 loads are laid out first
        gq = *reinterpret_cast<const float4 *>(g + i);
#pragma unroll
        for (int s = 0; s < N; ++s) mq[s] = *reinterpret_cast<const float4 *>(m[s] + i);
    } else {
        const float nan = __builtin_nanf("");
        gq = make_float4(g[i], i + 1 < npix ? g[i + 1] : nan, i + 2 < npix ? g[i + 2] : nan, i + 3 < npix ? g[i + 3] : nan);
#pragma unroll
        for (int s = 0; s < N; ++s)
            mq[s] = make_float4(m[s][i], i + 1 < npix ? m[s][i + 1] : 0.0f, i + 2 < npix ? m[s][i + 2] : 0.0f,
                                i + 3 < npix ? m[s][i + 3] : 0.0f);
    }
}

}  // namespace lws::opkit
