// One-forward occlusion check of the stage maps: the left-view disparities are splatted into the right view with a z-buffer (the
// nearest surface wins), and a left pixel is occluded when something nearer landed where it lands.  No second network: the
// alternative to the left-right check (lws_lrcheck.hip) for callers who only want occlusion masks; it finds no mismatches.
// Arithmetic contract (include/lwsnet_hip.h, lws_occlusion_check): one IEEE float32 operation per step (the build has no
// contraction), so tests/occ_reference.py restates every output bit for bit in numpy.  Determinism: the only atomics are unsigned
// integer max on LDS words of the workgroup's own row, whose order cannot show; a workgroup owns one row of one image and map, so
// an image gives the same bits in any batch.  0 bytes of scratch; the row and its z-buffer live in LDS.
#include "lws_common.h"
#include "lws_rowfill.h"

namespace lws {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxW = rowfill::kFillMaxW;                   // dL row + z-buffer row: 64 KiB of LDS at most
constexpr int kTailWords = 3 * kWaves;                      // the fill's two per-wave aggregates and the kept counts
static_assert(kThreads == rowfill::kFillThreads, "k_occ_check runs rowfill::fill_row");
using rowfill::aligned16;
using rowfill::stage_row;
using rowfill::store_quad;

struct OccMaps {                                            // the nmaps stage maps of one call, by value in the kernel arguments
    const float *dl[4];
    float *out[4];
    uint8_t *mask[4];
    float *right[4];
};

// The order-preserving word of a float: unsigned compare of keys == float compare of values (-0.0 below +0.0).  0 is no float's
// key but a NaN's (bits 0xffffffff), and NaNs are never keyed: 0 means "empty".
__device__ __forceinline__ unsigned key_of(float d)
{
    const unsigned u = __float_as_uint(d);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ float unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// words of LDS behind the staged row: the z-buffer (4 nq), which the fill's index arrays (2 nq) and the kTailWords reuse
__host__ __device__ constexpr int z_words(int nq) { return 4 * nq > 2 * nq + kTailWords ? 4 * nq : 2 * nq + kTailWords; }

// grid (H, B, nmaps), 256 threads: one workgroup per row.  Thread t owns the quads t, t + 256, ... (pixels 4q .. 4q + 3) of the
// row; W <= 8192 gives at most 8 quads, so the code == 1 flags of its pixels fit in one 32-bit word (bit 4k + i).
// LDS (dynamic): row[4 nq] floats (dL), then z_words(nq) words: Z[4 nq] through the splat and the test; once every thread is
// done with Z, last[nq], first[nq], wl[kWaves], wf[kWaves], kept[kWaves] in the same space.
__global__ __launch_bounds__(kThreads) void k_occ_check(OccMaps m, int H, int W, float tau, int fill, int *__restrict__ row_kept)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int y = blockIdx.x, b = blockIdx.y, s = blockIdx.z, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nq = (W + 3) >> 2;
    float *s_row = lds;
    unsigned *s_z = reinterpret_cast<unsigned *>(lds + 4 * nq);
    int *s_last = reinterpret_cast<int *>(s_z), *s_first = s_last + nq, *s_wl = s_first + nq, *s_wf = s_wl + kWaves, *s_kept = s_wf + kWaves;
    const int64_t row = ((int64_t)b * H + y) * W;
    const float *dl = m.dl[s] + row;
    float *out = m.out[s] + row, *rt = m.right[s] ? m.right[s] + row : nullptr;
    uint8_t *mk = m.mask[s] + row;
    const bool vout = aligned16(out), vrt = aligned16(rt), vmk = ((uintptr_t)mk & 3) == 0;
    const float wmax = (float)(W - 1);

    stage_row(s_row, dl, W, nq);                            // out may be dl: every load of the row is done before any store
    for (int q = t; q < nq; q += kThreads) *reinterpret_cast<uint4 *>(s_z + 4 * q) = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();

    // ---- pass 1: splat every in-view pixel's key onto the one or two columns its target x - d touches ----
    for (int q = t; q < nq; q += kThreads) {
        const int x0 = 4 * q;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int x = x0 + i;
            if (x >= W) break;
            const float d = s_row[x];
            const float tx = (float)x - d;
            if (__builtin_isnan(d) || !(tx >= 0.0f && tx <= wmax)) continue;
            const float fl = floorf(tx);
            const int j = (int)fl;
            const unsigned k = key_of(d);
            atomicMax(&s_z[j], k);
            if (ceilf(tx) != fl) atomicMax(&s_z[j + 1], k);  // j + 1 <= W - 1 since tx <= W - 1 is not an integer here
        }
    }
    __syncthreads();

    // ---- pass 2: codes, mask, right, out (no fill), kept count ----
    unsigned bits = 0;
    int kept = 0;
    for (int k = 0, q = t; q < nq; ++k, q += kThreads) {
        const int x0 = 4 * q;
        float d[4];
        int c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int x = x0 + i;
            d[i] = x < W ? s_row[x] : __builtin_nanf("");   // beyond the row: code 0, never kept
            const float tx = (float)x - d[i];
            if (__builtin_isnan(d[i])) {
                c[i] = 0;
            } else if (!(tx >= 0.0f && tx <= wmax)) {
                c[i] = 2;
            } else {
                const float z = unkey(s_z[(int)rintf(tx)]); // non-empty: x itself splatted there
                c[i] = z - d[i] <= tau ? 1 : 0;
            }
            kept += c[i] == 1 ? 1 : 0;
            bits |= (c[i] == 1 ? 1u : 0u) << (4 * k + i);
        }
        if (vmk && x0 + 4 <= W) {
            *reinterpret_cast<uchar4 *>(mk + x0) = make_uchar4((uint8_t)c[0], (uint8_t)c[1], (uint8_t)c[2], (uint8_t)c[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + i < W) mk[x0 + i] = (uint8_t)c[i];
        }
        if (rt) {                                           // the right view's own map; Z beyond the row stays empty
            const uint4 z = *reinterpret_cast<const uint4 *>(s_z + x0);
            store_quad(rt, x0, W, vrt, z.x ? unkey(z.x) : 0.0f, z.y ? unkey(z.y) : 0.0f, z.z ? unkey(z.z) : 0.0f, z.w ? unkey(z.w) : 0.0f);
        }
        if (!fill) store_quad(out, x0, W, vout, c[0] == 1 ? d[0] : 0.0f, c[1] == 1 ? d[1] : 0.0f, c[2] == 1 ? d[2] : 0.0f,
                              c[3] == 1 ? d[3] : 0.0f);
    }
    if (!fill && !row_kept) return;                         // launch-uniform

    if (row_kept)
        for (int o = 32; o > 0; o >>= 1) kept += __shfl_down(kept, o, 64);
    __syncthreads();                                        // every read of Z is done: its space is reused from here on
    if (row_kept && lane == 0) s_kept[wave] = kept;
    if (fill) {
        for (int k = 0, q = t; q < nq; ++k, q += kThreads) {
            const unsigned cb = bits >> (4 * k);
            const bool ok[4] = {(cb & 1u) != 0, (cb & 2u) != 0, (cb & 4u) != 0, (cb & 8u) != 0};
            int last, first;
            rowfill::quad_last_first(ok, 4 * q, last, first);
            s_last[q] = last;
            s_first[q] = first;
        }
    }
    __syncthreads();
    // the row fill (lws_rowfill.h): scans of last / first over the quads, then code-1 pixels keep d and the others take the
    // background value of their row
    if (fill) rowfill::fill_row(s_row, s_last, s_first, s_wl, s_wf, bits, nq, W, out, vout);
    if (row_kept && t == 0) row_kept[((int64_t)s * gridDim.y + b) * H + y] = (s_kept[0] + s_kept[1]) + (s_kept[2] + s_kept[3]);
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int lws_occlusion_check(const float *const dL[4], int nmaps, int B, int H, int W, float tau, int fill, float *const out[4],
                        uint8_t *const mask[4], float *const right[4], int32_t *row_kept, void *stream)
{
    LWS_CHECK_ARG(dL && out && mask, "occlusion_check: null pointer");
    LWS_CHECK_ARG(nmaps >= 1 && nmaps <= 4, "occlusion_check: nmaps %d outside 1..4", nmaps);
    LWS_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "occlusion_check: bad shape B=%d H=%d W=%d", B, H, W);
    LWS_CHECK_ARG(W <= kMaxW, "occlusion_check: W=%d exceeds %d (the row and its z-buffer are held in LDS)", W, kMaxW);
    LWS_CHECK_ARG(tau >= 0.0f && tau <= 3.4028234663852886e38f, "occlusion_check: tau must be finite and >= 0, got %g", (double)tau);
    LWS_CHECK_ARG(fill == 0 || fill == 1, "occlusion_check: fill %d (0 = zero, 1 = background fill)", fill);
    OccMaps m = {};
    for (int s = 0; s < nmaps; ++s) {
        LWS_CHECK_ARG(dL[s] && out[s] && mask[s], "occlusion_check: map %d has a null pointer", s);
        m.dl[s] = dL[s];
        m.out[s] = out[s];
        m.mask[s] = mask[s];
        m.right[s] = right ? right[s] : nullptr;
    }
    const int nq = (W + 3) / 4;
    const size_t lds = ((size_t)4 * nq + z_words(nq)) * sizeof(float);
    hipLaunchKernelGGL(k_occ_check, dim3(H, B, nmaps), dim3(kThreads), lds, (hipStream_t)stream, m, H, W, tau, fill, row_kept);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // extern "C"
