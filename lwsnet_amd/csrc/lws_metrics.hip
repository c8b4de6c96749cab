// Per-stage evaluation metrics of the reference's two test loops, reduced on the device so that only 4 x B x 3 numbers leave it:
// the KITTI 3-pixel error of the reference's finetune.py:212-219 (error_estimating, mode 0) and the SceneFlow EPE of
// train.py:180,189-190 (mode 1).  For every stage map s and image b: valid = #mask, bad = #(mask & e > 3 & e / g > 0.05),
// abs_sum = sum over the mask of e, e = |pred - gt|.
// Arithmetic contract: the reference's float32 numpy -- e, the division and the compares are one IEEE float32 operation each
// (the build has correctly rounded division, no contraction), the constants are 3.0f, 0.05f and (float)maxdisp.  Ordered compares
// are false on NaN, so a NaN or +inf ground truth is never valid and a NaN prediction is never bad (but makes abs_sum NaN).
// Determinism: no float atomics.  Every pixel belongs to a fixed quad, every quad to a fixed (workgroup, thread, step); each thread
// adds its pixels' e (exact in fp64) in that order, the workgroup and the second launch combine in fixed trees.  Which pixels a
// workgroup owns depends on the image's geometry only, and the float4 and the scalar loads feed the same order, so an image gives the
// same bits in any batch, at any alignment (tests/test_gpu_evaluate.py).
#include "lws_common.h"
#include "lws_opkit.h"

namespace lws {

namespace {

using namespace opkit;                                      // wave_sum, sum4, gt_pixel, load_gt_quad and the ground-truth checks
constexpr int kThreads = 256;
constexpr int kSteps = 4;                                   // quads per thread
constexpr int kQuadsPerBlock = kThreads * kSteps;           // 1024 quads = 4096 pixels per workgroup
constexpr int kWaves = kThreads / 64;

struct Partial {                                            // one (image, workgroup, stage) of the workspace
    long long valid, bad;
    double abs_sum;
};

int64_t blocks_per_image(int64_t npix) { return (npix + 4 * kQuadsPerBlock - 1) / (4 * kQuadsPerBlock); }

struct Acc {
    int valid = 0, bad = 0;
    double sum = 0.0;
};

__device__ __forceinline__ void pixel(Acc &a, float p, float g, float md, int mode)
{
    const GtPixel x = gt_pixel(p, g, md, mode);
    a.valid += x.valid ? 1 : 0;
    a.bad += x.bad ? 1 : 0;
    if (x.valid) a.sum += (double)x.e;                      // NaN e of a valid pixel propagates, as np.mean does
}

// grid (blocks_per_image, B), 256 threads.  pred[s] + b * pred_img + pred_off is image b's first ground-truth row of stage s.
__global__ __launch_bounds__(kThreads) void k_stage_metrics(const float *__restrict__ p0, const float *__restrict__ p1,
                                                            const float *__restrict__ p2, const float *__restrict__ p3,
                                                            const float *__restrict__ gt, int64_t npix, int64_t pred_img,
                                                            int64_t pred_off, float md, int mode, Partial *__restrict__ part)
{
    const int b = blockIdx.y, t = threadIdx.x;
    const float *g = gt + (int64_t)b * npix;
    const float *const ps[4] = {p0 + b * pred_img + pred_off, p1 + b * pred_img + pred_off, p2 + b * pred_img + pred_off,
                                p3 + b * pred_img + pred_off};
    uintptr_t bits = (uintptr_t)g;
#pragma unroll
    for (int s = 0; s < 4; ++s) bits |= (uintptr_t)ps[s];
    const bool vec = (bits & 15) == 0;                      // image-uniform: float4 loads for every full quad
    Acc acc[4];
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
        const int64_t i = 4 * ((int64_t)blockIdx.x * kQuadsPerBlock + k * kThreads + t);
        if (i >= npix) break;
        float4 gq, pq[4];
        load_gt_quad(g, ps, i, npix, vec, gq, pq);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            pixel(acc[s], pq[s].x, gq.x, md, mode);
            pixel(acc[s], pq[s].y, gq.y, md, mode);
            pixel(acc[s], pq[s].z, gq.z, md, mode);
            pixel(acc[s], pq[s].w, gq.w, md, mode);
        }
    }
    __shared__ int s_cnt[kWaves][4][2];
    __shared__ double s_sum[kWaves][4];
    const int wave = t >> 6, lane = t & 63;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int v = wave_sum(acc[s].valid), bd = wave_sum(acc[s].bad);
        const double sm = wave_sum(acc[s].sum);
        if (lane == 0) {
            s_cnt[wave][s][0] = v;
            s_cnt[wave][s][1] = bd;
            s_sum[wave][s] = sm;
        }
    }
    __syncthreads();
    if (t < 4) {
        Partial o;
        o.valid = sum4<long long>(s_cnt[0][t][0], s_cnt[1][t][0], s_cnt[2][t][0], s_cnt[3][t][0]);
        o.bad = sum4<long long>(s_cnt[0][t][1], s_cnt[1][t][1], s_cnt[2][t][1], s_cnt[3][t][1]);
        o.abs_sum = sum4(s_sum[0][t], s_sum[1][t], s_sum[2][t], s_sum[3][t]);
        part[((int64_t)b * gridDim.x + blockIdx.x) * 4 + t] = o;
    }
}

// grid (4, B), 256 threads: stage s of image b sums its workgroups' partials, thread t the ones at t, t + 256, ..., then a fixed tree.
__global__ __launch_bounds__(kThreads) void k_stage_metrics_sum(const Partial *__restrict__ part, int nblk, int B,
                                                                long long *__restrict__ counts, double *__restrict__ abs_sum)
{
    const int s = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    long long v = 0, bd = 0;
    double sm = 0.0;
    for (int j = t; j < nblk; j += kThreads) {
        const Partial q = part[((int64_t)b * nblk + j) * 4 + s];
        v += q.valid;
        bd += q.bad;
        sm += q.abs_sum;
    }
    v = wave_sum(v);
    bd = wave_sum(bd);
    sm = wave_sum(sm);
    __shared__ long long s_cnt[kWaves][2];
    __shared__ double s_sum[kWaves];
    const int wave = t >> 6;
    if ((t & 63) == 0) {
        s_cnt[wave][0] = v;
        s_cnt[wave][1] = bd;
        s_sum[wave] = sm;
    }
    __syncthreads();
    if (t == 0) {
        const int64_t o = (int64_t)s * B + b;
        counts[2 * o] = sum4(s_cnt[0][0], s_cnt[1][0], s_cnt[2][0], s_cnt[3][0]);
        counts[2 * o + 1] = sum4(s_cnt[0][1], s_cnt[1][1], s_cnt[2][1], s_cnt[3][1]);
        abs_sum[o] = sum4(s_sum[0], s_sum[1], s_sum[2], s_sum[3]);
    }
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int64_t lws_stage_metrics_workspace(int B, int Hg, int Wg)
{
    LWS_CHECK_RC(check_gt_args("stage_metrics_workspace", B, Hg, Wg, nullptr));
    return (int64_t)B * blocks_per_image((int64_t)Hg * Wg) * 4 * (int64_t)sizeof(Partial);
}

int lws_stage_metrics(const float *const pred[4], int B, int Hp, int W, int row_offset, const float *gt, int Hg, float maxdisp,
                      int mode, void *workspace, int64_t *counts, double *abs_sum, void *stream)
{
    LWS_CHECK_ARG(pred && gt && workspace && counts && abs_sum, "stage_metrics: null pointer");
    for (int s = 0; s < 4; ++s) LWS_CHECK_ARG(pred[s], "stage_metrics: pred[%d] is null", s);
    const GtRows rows = {Hp, row_offset, maxdisp, mode};
    LWS_CHECK_RC(check_gt_args("stage_metrics", B, Hg, W, &rows));
    const int64_t npix = (int64_t)Hg * W;
    const int64_t nblk = blocks_per_image(npix);
    Partial *part = static_cast<Partial *>(workspace);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_stage_metrics, dim3((unsigned)nblk, B), dim3(kThreads), 0, st, pred[0], pred[1], pred[2], pred[3], gt, npix,
                       (int64_t)Hp * W, (int64_t)row_offset * W, maxdisp, mode, part);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_stage_metrics_sum, dim3(4, B), dim3(kThreads), 0, st, part, (int)nblk, B, reinterpret_cast<long long *>(counts),
                       abs_sum);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // extern "C"
