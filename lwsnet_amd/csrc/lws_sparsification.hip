// Sparsification histograms: how well an uncertainty map (sigma, or 1 - conf) ranks the pixels of a stage map by their error
// (Ilg et al. 2018).  For every map s, image b and valid ground-truth pixel, {1, bad, q} is added to two 1026-bin histograms: one
// indexed by the uncertainty u (the ranking under test), one by the error e itself (the oracle ranking); q is e in 1/1024 px.  The
// host turns the cumulative sums over ascending bins into the two sparsification curves (lwsnet_amd/metrics.py).
// Arithmetic contract (include/lwsnet_hip.h): valid, bad and e are gt_pixel() of lws_opkit.h; every step is one IEEE float32
// operation (the build has correctly rounded division and no contraction); the bin of a value is a function of its bits.
// Determinism: every sum is an integer.  A workgroup owns 2 x 1026 private bins in LDS ({count | bad << 32} and the q sum, one
// 64-bit word each), adds to them with LDS integer atomics and flushes its non-zero bins with 64-bit integer global atomics into
// the histogram the call has cleared: the order of integer additions cannot show, so an image gives the same bytes in any batch,
// at any position, under any partition into workgroups, on every run.
// The hot bin: a sharply peaked pixel has conf >= 1, so u <= 0 and most of a real image lands in bin 0 (and a good map puts the
// oracle's pixels into few bins too).  Lanes that add to one LDS word serialise, so the lanes that share the bin of the wave's
// first valid lane add once per wave when there are at least kAggMin of them: the counts are popcounts of ballots, q is one
// 64-bit wave sum.  The other lanes add on their own.
#include "lws_common.h"
#include "lws_opkit.h"

namespace lws {

namespace {

using namespace opkit;                                      // wave_sum, gt_pixel, load_gt_quad, overlap and the ground-truth checks
constexpr int kBins = LWS_SPARS_BINS;
constexpr int kThreads = 512;
constexpr int kMaxSteps = 8;                                // quads per thread: at most 16384 pixels per workgroup
constexpr int kAggMin = 16;                                 // lanes on one bin from which one wave-level add replaces theirs

typedef unsigned long long u64;

// Bin 0: v < 2^-24 (negatives and both zeros included); bins 1..1024: 32 logarithmic bins per octave over [2^-24, 2^8), every
// such v a normal float, 3296 = (127 - 24) << 5; bin 1025: v >= 256 or NaN.
__device__ __forceinline__ int spars_bin(float v)
{
    if (!(v < 256.0f)) return kBins - 1;
    if (v < 0x1p-24f) return 0;
    return 1 + (int)((__float_as_uint(v) >> 18) - 3296u);
}

// One pixel per lane into one ranking's bins, the whole wave converged.  cb: count | bad << 32 (a workgroup has fewer than 2^32
// pixels, so the halves never carry), qs: the q sum.
__device__ __forceinline__ void add_pixel(u64 *cb, u64 *qs, bool valid, int bin, bool bad, u64 q, int lane)
{
    const u64 act = __ballot(valid);
    if (act == 0) return;
    const int lbin = __shfl(bin, __ffsll((long long)act) - 1, 64);
    const bool same = valid && bin == lbin;
    const u64 m = __ballot(same);
    bool own = valid;
    if (__popcll(m) >= kAggMin) {                           // wave-uniform
        const u64 nbad = (u64)__popcll(__ballot(same && bad));
        const u64 qsum = wave_sum<u64>(same ? q : 0);
        if (lane == 0) {
            atomicAdd(&cb[lbin], (u64)__popcll(m) | (nbad << 32));
            if (qsum != 0) atomicAdd(&qs[lbin], qsum);
        }
        own = valid && !same;
    }
    if (own) {
        atomicAdd(&cb[bin], 1ull | ((u64)(bad ? 1 : 0) << 32));
        if (q != 0) atomicAdd(&qs[bin], q);
    }
}

__device__ __forceinline__ void pixel(u64 *cb, u64 *qs, float p, float uin, float g, float md, int mode, int kind, int lane)
{
    const GtPixel x = gt_pixel(p, g, md, mode);
    const bool valid = x.valid, bad = x.bad;
    const float e = x.e;
    const float ec = e < 65536.0f ? e : 65536.0f;                           // fminf(e, 65536.0f): a NaN e is the worst error
    const u64 q = (u64)(long long)rintf(ec * 1024.0f);                      // 1/1024 px; the scaling is exact
    const float u = kind == 0 ? uin : 1.0f - uin;
    add_pixel(cb, qs, valid, spars_bin(u), bad, q, lane);
    add_pixel(cb + kBins, qs + kBins, valid, spars_bin(e), bad, q, lane);
}

struct Maps {
    const float *pred[4], *unc[4];
};

// grid (blocks per image, B, nmaps), 512 threads; a workgroup owns 2048 * steps pixels of image b in map s and flushes once.
// pred[s] + b * pred_img + pred_off is image b's first ground-truth row of map s.
__global__ __launch_bounds__(kThreads) void k_sparsification(Maps maps, int kind, const float *__restrict__ gt, int64_t npix,
                                                             int64_t pred_img, int64_t pred_off, int steps, float md, int mode,
                                                             u64 *__restrict__ hist)
{
    __shared__ u64 s_cb[2 * kBins], s_q[2 * kBins];
    const int b = blockIdx.y, B = gridDim.y, s = blockIdx.z, t = threadIdx.x, lane = t & 63;
    const float *g = gt + (int64_t)b * npix;
    const float *const pu[2] = {maps.pred[s] + b * pred_img + pred_off, maps.unc[s] + b * pred_img + pred_off};
    const bool vec = ((((uintptr_t)g) | ((uintptr_t)pu[0]) | ((uintptr_t)pu[1])) & 15) == 0;   // image-uniform
    const int64_t first = (int64_t)blockIdx.x * steps * kThreads * 4;
    for (int j = t; j < 2 * kBins; j += kThreads) {
        s_cb[j] = 0;
        s_q[j] = 0;
    }
    __syncthreads();
    for (int k = 0; k < steps; ++k) {                       // every lane takes every step: the wave stays converged
        const int64_t i = first + 4 * ((int64_t)k * kThreads + t);
        const float nan = __builtin_nanf("");               // a quad beyond the image: gt = NaN, no pixel of it is valid
        float4 gq = make_float4(nan, nan, nan, nan), q[2] = {make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
        if (i < npix) load_gt_quad(g, pu, i, npix, vec, gq, q);
        pixel(s_cb, s_q, q[0].x, q[1].x, gq.x, md, mode, kind, lane);
        pixel(s_cb, s_q, q[0].y, q[1].y, gq.y, md, mode, kind, lane);
        pixel(s_cb, s_q, q[0].z, q[1].z, gq.z, md, mode, kind, lane);
        pixel(s_cb, s_q, q[0].w, q[1].w, gq.w, md, mode, kind, lane);
    }
    __syncthreads();
    u64 *h = hist + ((int64_t)s * B + b) * (2 * kBins * 3);
    for (int j = t; j < 2 * kBins; j += kThreads) {         // flush the non-zero bins
        const u64 cb = s_cb[j], q = s_q[j];
        if (cb != 0) {
            atomicAdd(&h[3 * j], cb & 0xffffffffull);
            if (cb >> 32) atomicAdd(&h[3 * j + 1], cb >> 32);
            if (q != 0) atomicAdd(&h[3 * j + 2], q);
        }
    }
}

// Quads per thread.  A workgroup's flush costs up to 3 global atomics per bin whatever it has counted, so a workgroup takes as many
// pixels as still leave a workgroup for every compute unit of a 256-unit device.  Any value gives the same histogram.
int steps_for(int64_t npix, int B, int nmaps)
{
    int steps = kMaxSteps;
    while (steps > 1 && ((npix + 4 * kThreads * steps - 1) / (4 * kThreads * steps)) * B * nmaps < 256) steps >>= 1;
    return steps;
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int lws_sparsification(const float *const pred[4], const float *const unc[4], int nmaps, int kind, int B, int Hp, int W, int row_offset,
                       const float *gt, int Hg, float maxdisp, int mode, int64_t *hist, void *stream)
{
    LWS_CHECK_ARG(pred && unc && gt && hist, "sparsification: null pointer");
    LWS_CHECK_ARG(nmaps >= 1 && nmaps <= 4, "sparsification: nmaps %d outside 1..4", nmaps);
    for (int s = 0; s < nmaps; ++s) LWS_CHECK_ARG(pred[s] && unc[s], "sparsification: pred[%d] or unc[%d] is null", s, s);
    LWS_CHECK_ARG(kind == 0 || kind == 1, "sparsification: kind %d (0 = sigma, 1 = conf)", kind);
    const GtRows rows = {Hp, row_offset, maxdisp, mode};
    LWS_CHECK_RC(check_gt_args("sparsification", B, Hg, W, &rows));
    const int64_t npix = (int64_t)Hg * W;
    const int64_t hist_bytes = (int64_t)nmaps * B * 2 * kBins * 3 * (int64_t)sizeof(int64_t);
    const int64_t map_bytes = (int64_t)B * Hp * W * 4;
    // (not opkit's table: the written buffer is named first here, and pred and unc may overlap each other as they like)
    LWS_CHECK_ARG(!overlap(hist, hist_bytes, gt, (int64_t)B * npix * 4), "sparsification: hist and gt overlap");
    Maps maps = {};
    for (int s = 0; s < nmaps; ++s) {
        LWS_CHECK_ARG(!overlap(hist, hist_bytes, pred[s], map_bytes), "sparsification: hist and pred[%d] overlap", s);
        LWS_CHECK_ARG(!overlap(hist, hist_bytes, unc[s], map_bytes), "sparsification: hist and unc[%d] overlap", s);
        maps.pred[s] = pred[s];
        maps.unc[s] = unc[s];
    }
    hipStream_t st = (hipStream_t)stream;
    LWS_HIP(hipMemsetAsync(hist, 0, (size_t)hist_bytes, st));
    const int steps = steps_for(npix, B, nmaps);
    const int64_t nblk = (npix + (int64_t)4 * kThreads * steps - 1) / ((int64_t)4 * kThreads * steps);
    hipLaunchKernelGGL(k_sparsification, dim3((unsigned)nblk, B, nmaps), dim3(kThreads), 0, st, maps, kind, gt, npix, (int64_t)Hp * W,
                       (int64_t)row_offset * W, steps, maxdisp, mode, reinterpret_cast<u64 *>(hist));
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // extern "C"
