// One-forward occlusion check of the stage maps: the left-view disparities are splatted into the right view with a z-buffer (the
// nearest surface wins), and a left pixel is occluded when something nearer landed where it lands.  No second network: the
// alternative to the left-right check (lws_lrcheck.hip) for callers who only want occlusion masks; it finds no mismatches.
// Arithmetic contract (include/lwsnet_hip.h, lws_occlusion_check): one IEEE float32 operation per step (the build has no
// contraction), so tests/occ_reference.py restates every output bit for bit in numpy.  Determinism: the only atomics are unsigned
// integer max on LDS words of the workgroup's own row, whose order cannot show; a workgroup owns one row of one image and map, so
// an image gives the same bits in any batch.  0 bytes of scratch; the row and its z-buffer live in LDS.
#include "lws_common.h"
#include "lws_rowkit.h"

namespace lws {

namespace {

using namespace rowkit;                                     // kThreads, kWaves, kMaxW: dL row + z-buffer row, 64 KiB of LDS at most
using opkit::key_of;                                        // 0 is no splatted value's key: an empty z-buffer word
using opkit::unkey;
constexpr int kTailWords = 3 * kWaves;                      // the fill's two per-wave aggregates and the kept counts

struct OccMaps {                                            // the nmaps stage maps of one call, by value in the kernel arguments
    const float *dl[4];
    float *out[4];
    uint8_t *mask[4];
    float *right[4];
};

// words of LDS behind the staged row: the z-buffer (4 nq), which the fill's index arrays (2 nq) and the kTailWords reuse
__host__ __device__ constexpr int z_words(int nq) { return 4 * nq > 2 * nq + kTailWords ? 4 * nq : 2 * nq + kTailWords; }

// grid (H, B, nmaps), 256 threads: one workgroup per row, thread t owns the quads t, t + 256, ... of it (lws_rowkit.h).
// LDS (dynamic): row[4 nq] floats (dL), then z_words(nq) words: Z[4 nq] through the splat and the test; once every thread is
// done with Z, last[nq], first[nq], wl[kWaves], wf[kWaves], kept[kWaves] in the same space.
__global__ __launch_bounds__(kThreads) void k_occ_check(OccMaps m, int H, int W, float tau, int fill, int *__restrict__ row_kept)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int y = blockIdx.x, b = blockIdx.y, s = blockIdx.z, t = threadIdx.x;
    const int nq = (W + 3) >> 2;
    float *s_row = lds;
    unsigned *s_z = reinterpret_cast<unsigned *>(lds + 4 * nq);
    int *s_last = reinterpret_cast<int *>(s_z), *s_first = s_last + nq, *s_wl = s_first + nq, *s_wf = s_wl + kWaves, *s_kept = s_wf + kWaves;
    const int64_t row = ((int64_t)b * H + y) * W;
    const float *dl = m.dl[s] + row;
    float *out = m.out[s] + row, *rt = m.right[s] ? m.right[s] + row : nullptr;
    uint8_t *mk = m.mask[s] + row;
    const bool vout = aligned(out, 16), vrt = aligned(rt, 16), vmk = aligned(mk, 4);
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
    KeptFlags kept;
    for (int k = 0, q = t; q < nq; ++k, q += kThreads) {
        const int x0 = 4 * q;
        float d[4];
        int c[4];
        load_quad(s_row, x0, W, true, __builtin_nanf(""), d);       // the staged row; NaN beyond it: code 0, never kept
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float tx = (float)(x0 + i) - d[i];
            if (__builtin_isnan(d[i])) {
                c[i] = 0;
            } else if (!(tx >= 0.0f && tx <= wmax)) {
                c[i] = 2;
            } else {
                const float z = unkey(s_z[(int)rintf(tx)]); // non-empty: x itself splatted there
                c[i] = z - d[i] <= tau ? 1 : 0;
            }
        }
        kept.add(k, c);
        store_codes(mk, x0, W, vmk, c);
        if (rt) {                                           // the right view's own map; Z beyond the row stays empty
            const uint4 z = *reinterpret_cast<const uint4 *>(s_z + x0);
            store_quad(rt, x0, W, vrt, z.x ? unkey(z.x) : 0.0f, z.y ? unkey(z.y) : 0.0f, z.z ? unkey(z.z) : 0.0f, z.w ? unkey(z.w) : 0.0f);
        }
        if (!fill) store_kept(out, x0, W, vout, c, d);
    }
    if (!fill && !row_kept) return;                         // launch-uniform

    __syncthreads();                                        // every read of Z is done: its space is reused from here on
    if (row_kept) wave_sums<1>({kept.count}, s_kept);
    if (fill)
        for (int k = 0, q = t; q < nq; ++k, q += kThreads) kept.last_first(k, 4 * q, s_last[q], s_first[q]);
    __syncthreads();
    // the row fill: scans of last / first over the quads, then code-1 pixels keep d and the others take the background value of
    // their row
    if (fill) fill_row(s_row, s_last, s_first, s_wl, s_wf, kept.bits, nq, W, out, vout);
    if (row_kept && t == 0) row_kept[((int64_t)s * gridDim.y + b) * H + y] = row_total<1>(s_kept, 0);
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int lws_occlusion_check(const float *const dL[4], int nmaps, int B, int H, int W, float tau, int fill, float *const out[4],
                        uint8_t *const mask[4], float *const right[4], int32_t *row_kept, void *stream)
{
    LWS_CHECK_ARG(dL && out && mask, "occlusion_check: null pointer");
    LWS_CHECK_RC(opkit::check_row_check_args("occlusion_check", "(the row and its z-buffer are held in LDS)", kMaxW, dL, nullptr, nmaps, B, H, W,
                                             tau, fill, out, mask));
    OccMaps m = {};
    for (int s = 0; s < nmaps; ++s) {
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
