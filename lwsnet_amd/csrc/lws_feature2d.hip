// Feature extractor of LWSNet, float32, -ffp-contract=off.
//
//   /root/reference/models/submodules.py:5-33 (convbn/deconvbn), :35-109 (hourglass),
//   :113-188 (feature_extraction)                               -> k_conv2d_nchw, k_conv2d_pair, k_conv2d_pair_mfma
//
// Arithmetic contract (oracle/lws_oracle.c lwso_conv2d / lwso_deconv2d_s2 / lwso_bn_add_relu): every convolution
// output is ONE fmaf chain from 0, taps (kh,kw) outer ascending, input channel inner ascending; zero padding
// (fmaf(0, w, acc) == acc, so padded taps may be fed as zeros); BatchNorm(eval) = fmaf(x, s, t); then the residual
// add; then ReLU.
//
// Layout: planar NCHW maps with 3..16 channels (the volume kernels read the outputs plane by plane, coalesced
// along W).
#include "lws_common.h"
#include "lws_device_math.h"

namespace lws {

LWS_DEFINE_STAMPS(feature2d)

// =============================================================================================
// Feature extractor: 3x3 convolution / stride-2 transposed convolution on NCHW planes (3..16 channels).
// Workgroup = an 8 x 8 output tile of one image, ALL output channels: the input region the tile needs (all CIN
// planes, zero outside the image) is staged once in LDS with every global load in flight; wave w then computes
// output channels [w*COUT/4, (w+1)*COUT/4) for the 64 pixels (one pixel per lane), so the weights
// ([tap][wave][cin][COUT/4]) are wave-uniform and come through the scalar cache.
// Epilogue: BatchNorm (optional) -> + residual (optional) -> ReLU (optional).
// =============================================================================================
template <int CIN, int COUT, bool TRANSPOSED>
__global__ __launch_bounds__(256) void k_conv2d_nchw(const float *__restrict__ in, const float *__restrict__ in2, int n1,
                                                     const float *__restrict__ wgt,
                                                     const float *__restrict__ bn_s, const float *__restrict__ bn_t,
                                                     const float *__restrict__ res, float *__restrict__ out, int H,
                                                     int W, int Ho, int Wo, int stride, int pad, int dil, int relu,
                                                     int RH, int RW, int RWp)
{
    // images [0, n1) come from `in`, images [n1, N) from `in2` (left and right inputs of the first layer are two
    // separate caller tensors); the output batch is contiguous
    constexpr int CPT = COUT / 4;
    extern __shared__ float sIn[];   // [CIN][RH][RWp]
    const int b = blockIdx.z;
    const int tid = threadIdx.x, tx = tid & 7, ty = (tid >> 3) & 7;
    const int wave_id = __builtin_amdgcn_readfirstlane(tid >> 6);   // SGPR: the weight addresses below become scalar loads
    const int co0 = wave_id * CPT;
    const int ox0 = blockIdx.x * 8, oy0 = blockIdx.y * 8;
    const int ry0 = TRANSPOSED ? ((oy0 - 1) >> 1) : oy0 * stride - pad;
    const int rx0 = TRANSPOSED ? ((ox0 - 1) >> 1) : ox0 * stride - pad;
    const int plane = H * W, oplane = Ho * Wo;
    const float *inb = b < n1 ? in + (int64_t)b * CIN * plane : in2 + (int64_t)(b - n1) * CIN * plane;
    LWS_STAMPK(7, 0);
    // region positions are decoded once per thread (<= 2 positions: RH*RW <= 19*19), then all CIN planes of a
    // position are loaded back to back (unconditional clamped loads, masked afterwards)
    const int rsz = RH * RW;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int r = tid + 256 * k;
        if (r < rsz) {
            const int ry = r / RW, rx = r - ry * RW;
            const int gy = ry0 + ry, gx = rx0 + rx;
            const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
            const float *src = inb + (ok ? gy * W + gx : 0);
            float v[CIN];
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) v[ci] = src[ci * plane];
            float *dst = sIn + ry * RWp + rx;
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) dst[ci * RH * RWp] = ok ? v[ci] : 0.0f;
        }
    }
    __syncthreads();
    LWS_STAMPK(7, 1);
    const int ox = ox0 + tx, oy = oy0 + ty;
    if (ox >= Wo || oy >= Ho) return;
    float acc[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) acc[c] = 0.0f;
    const int cstride = RH * RWp;
#pragma unroll 3
    for (int tap = 0; tap < 9; ++tap) {
        const int kh = tap / 3, kw = tap - kh * 3;
        int ly, lx;
        bool ok = true;
        if (TRANSPOSED) {          // oy = 2*iy - 1 + kh  (k3, s2, p1, output_padding 1)
            const int t_y = oy + 1 - kh, t_x = ox + 1 - kw;
            ok = t_y >= 0 && !(t_y & 1) && (t_y >> 1) < H && t_x >= 0 && !(t_x & 1) && (t_x >> 1) < W;
            ly = (t_y >> 1) - ry0;
            lx = (t_x >> 1) - rx0;
        } else {
            ly = ty * stride + kh * dil;
            lx = tx * stride + kw * dil;
        }
        const float *p = sIn + (ok ? ly * RWp + lx : 0);
        // weights are packed [tap][wave][cin][CPT]: the CIN*CPT values a wave needs for one tap are contiguous, so they
        // arrive in a few wide scalar loads (one 8-byte s_load per (tap, cin) made this loop latency-bound)
        const float *w = wgt + (tap * 4 + wave_id) * CIN * CPT;
        float v[CIN];
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) v[ci] = ok ? p[ci * cstride] : 0.0f;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
            for (int c = 0; c < CPT; ++c) acc[c] = fmaf(v[ci], w[ci * CPT + c], acc[c]);
    }
    LWS_STAMPK(7, 2);
    const int64_t o = ((int64_t)b * COUT + co0) * oplane + oy * Wo + ox;
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
        float v = acc[c];
        if (bn_s != nullptr) v = fmaf(v, bn_s[co0 + c], bn_t[co0 + c]);
        if (res != nullptr) v = v + res[o + (int64_t)c * oplane];
        if (relu) v = fmaxf(v, 0.0f);
        out[o + (int64_t)c * oplane] = v;
    }
    LWS_STAMPK(7, 3);
}

template <int CIN, int COUT, bool TR>
static int conv2d_launch(const Conv2dLayer &l, const float *in, const float *in2, int n1, const float *res, float *out,
                         int N, int H, int W, int Ho, int Wo, hipStream_t st)
{
    const int RH = TR ? 6 : 7 * l.stride + 2 * l.dil + 1, RW = RH;
    const int RWp = RW | 1;                                       // odd row stride
    const size_t lds = (size_t)CIN * RH * RWp * sizeof(float);
    dim3 grid(cdiv(Wo, 8), cdiv(Ho, 8), N), block(256);
    hipLaunchKernelGGL((k_conv2d_nchw<CIN, COUT, TR>), grid, block, lds, st, in, in2, n1, l.w, l.bn_s, l.bn_t, res, out, H,
                       W, Ho, Wo, l.stride, l.pad, l.dil, l.relu ? 1 : 0, RH, RW, RWp);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

// N images [N,cin,H,W] -> [N,cout,Ho,Wo]; if in2 != nullptr the first n1 images are read from `in`, the rest from `in2`
int launch_conv2d_nchw(const Conv2dLayer &l, const float *in, const float *res, float *out, int N, int H, int W,
                       hipStream_t st, const float *in2, int n1)
{
    if (in2 == nullptr) {
        in2 = in;
        n1 = N;
    }
    int Ho, Wo;
    if (l.transposed) {
        Ho = 2 * H;
        Wo = 2 * W;
    } else {
        Ho = (H + 2 * l.pad - 2 * l.dil - 1) / l.stride + 1;
        Wo = (W + 2 * l.pad - 2 * l.dil - 1) / l.stride + 1;
    }
#define LWS_C2D(CI, CO, TR)                                   \
    if (l.cin == CI && l.cout == CO && l.transposed == TR)    \
        return conv2d_launch<CI, CO, TR>(l, in, in2, n1, res, out, N, H, W, Ho, Wo, st);
    LWS_C2D(3, 4, false) LWS_C2D(4, 8, false) LWS_C2D(8, 4, false) LWS_C2D(8, 16, false) LWS_C2D(16, 16, false)
    LWS_C2D(16, 16, true) LWS_C2D(16, 8, true) LWS_C2D(8, 8, false)
#undef LWS_C2D
    set_error("conv2d_nchw: unsupported layer cin=%d cout=%d", l.cin, l.cout);
    return LWS_ERR_INVALID;
}

// =============================================================================================
// Two chained feature-extractor layers in one launch: A (3x3, stride SA, dilation DA = pad, BN, ReLU?) followed by B
// (3x3, stride 1, dilation DB = pad, BN?, + residual?, ReLU?).  The workgroup owns an 8 x 8 tile of B's output; A is
// evaluated on the MR x MR region B needs (MR = 8 + 2 DB; its values outside A's output map are B's zero padding) and
// kept in LDS, so the intermediate map never goes to HBM and one launch disappears.  Every layer keeps its own
// arithmetic (same fma chains), so the result is bit-identical to running the two kernels back to back.
//
// These layers hold a few hundred fmas per pixel: they are latency-bound (LDS reads, scalar weight loads), so
// the kernel is organised for parallelism, not reuse.  All geometry is compile time.  NW waves per workgroup:
//   phase 1  every thread loads ceil(CIN RH^2 / NT) input values, all in flight at once;
//   phase 2  the MR^2 pixels of A are spread over WGA waves and its CM output channels over GA = NW / WGA groups of
//            waves, so the whole region is ONE pass (weights [tap][GA][CIN][CM/GA], wave-uniform -> scalar loads);
//   phase 3  wave = COUT/NW output channels of B for the 64 tile pixels (weights [tap][NW][CM][COUT/NW]).
// NW = 4 for the 1/2-resolution pairs (4 workgroups per CU), NW = 16 for the 1/4 and 1/8 pairs, whose grids have
// fewer workgroups than the chip has CUs.
// =============================================================================================
template <int CIN, int CM, int COUT, int SA, int DA, int DB, int NW>
struct PairCfg {
    static constexpr int NT = 64 * NW;
    static constexpr int MR = 8 + 2 * DB, MRp = MR | 1;
    static constexpr int RH = (MR - 1) * SA + 2 * DA + 1;
    // stride-2 layers read every other column: the input rows are stored de-interleaved by column parity (even
    // columns, then odd columns) so that consecutive lanes hit consecutive LDS banks instead of every second one
    static constexpr int HALF = (RH + 1) / 2, RWp = (SA == 2 ? 2 * HALF : RH) | 1;
    __host__ __device__ static constexpr int col(int rx) { return SA == 2 ? (rx & 1) * HALF + (rx >> 1) : rx; }
    static constexpr int WGA_ = (MR * MR + 63) / 64;                                  // waves needed for one pass over A's region
    static constexpr int WGA = WGA_ <= 1 ? 1 : WGA_ <= 2 ? 2 : WGA_ <= 4 ? 4 : WGA_ <= 8 ? 8 : 16;
    static constexpr int GA = NW / WGA, CPA = CM / GA, CPB = COUT / NW;
    static constexpr int ITEMS = CIN * RH * RH, SITER = (ITEMS + NT - 1) / NT;
    static constexpr int LDS_FLOATS = CIN * RH * RWp + CM * MR * MRp;
    static_assert(WGA <= NW && NW % WGA == 0 && CM % GA == 0 && COUT % NW == 0 && CPA >= 1 && CPB >= 1, "bad pair geometry");
    static_assert(WGA * 64 >= MR * MR, "phase 2 must be one pass");
};

template <int CIN, int CM, int COUT, int SA, int DA, int DB, int NW>
__global__ __launch_bounds__(64 * NW) void k_conv2d_pair(const float *__restrict__ in, const float *__restrict__ in2, int n1,
                                                         const float *__restrict__ wA, const float *__restrict__ sA_,
                                                         const float *__restrict__ tA_, int reluA,
                                                         const float *__restrict__ wB, const float *__restrict__ sB_,
                                                         const float *__restrict__ tB_, const float *__restrict__ res,
                                                         int reluB, float *__restrict__ out, int H, int W, int HA, int WA)
{
    using Cfg = PairCfg<CIN, CM, COUT, SA, DA, DB, NW>;
    constexpr int NT = Cfg::NT, MR = Cfg::MR, MRp = Cfg::MRp, RH = Cfg::RH, RWp = Cfg::RWp, WGA = Cfg::WGA, GA = Cfg::GA,
                  CPA = Cfg::CPA, CPB = Cfg::CPB, SITER = Cfg::SITER, RSZ = RH * RH;
    extern __shared__ float smem[];
    float *sIn = smem;                       // [CIN][RH][RWp]
    float *sMid = smem + CIN * RH * RWp;     // [CM][MR][MRp]
    const int b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ox0 = blockIdx.x * 8, oy0 = blockIdx.y * 8;
    const int my0 = oy0 - DB, mx0 = ox0 - DB;                     // origin of the intermediate region (A-output coords)
    const int iy0 = my0 * SA - DA, ix0 = mx0 * SA - DA;           // pad == dilation for every layer of the extractor
    const int plane = H * W;
    const float *inb = b < n1 ? in + (int64_t)b * CIN * plane : in2 + (int64_t)(b - n1) * CIN * plane;
    [[maybe_unused]] constexpr int STAMP_ID = 13 + (CIN == 3 ? 0 : CM == 4 ? 1 : CIN == 8 ? 2 : 3);   // diagnostic builds only
    LWS_STAMPK(STAMP_ID, 0);
    // phase 1: input region, item = (channel, region pixel); unconditional clamped loads, masked afterwards
    {
        float v[SITER];
        bool okv[SITER];
#pragma unroll
        for (int i = 0; i < SITER; ++i) {
            const int it = tid + i * NT;
            const int ci = it / RSZ, r = it - ci * RSZ;
            const int ry = r / RH, rx = r - ry * RH;
            const int gy = iy0 + ry, gx = ix0 + rx;
            okv[i] = it < Cfg::ITEMS && gy >= 0 && gy < H && gx >= 0 && gx < W;
            v[i] = inb[okv[i] ? ci * plane + gy * W + gx : 0];
        }
#pragma unroll
        for (int i = 0; i < SITER; ++i) {
            const int it = tid + i * NT;
            const int ci = it / RSZ, r = it - ci * RSZ;
            const int ry = r / RH, rx = r - ry * RH;
            if (it < Cfg::ITEMS) sIn[(ci * RH + ry) * RWp + Cfg::col(rx)] = okv[i] ? v[i] : 0.0f;
        }
    }
    __syncthreads();
    LWS_STAMPK(STAMP_ID, 1);
    // phase 2: layer A on the MR x MR region
    {
        const int ga = wave / WGA;
        const int coA = ga * CPA;
        const int p = (wave - ga * WGA) * 64 + lane;
        if (p < MR * MR) {
            const int my = p / MR, mx = p - my * MR;
            const int ay = my0 + my, ax = mx0 + mx;
            const bool valid = ay >= 0 && ay < HA && ax >= 0 && ax < WA;
            float acc[CPA];
#pragma unroll
            for (int c = 0; c < CPA; ++c) acc[c] = 0.0f;
#pragma unroll 3
            for (int tap = 0; tap < 9; ++tap) {
                const int kh = tap / 3, kw = tap - kh * 3;
                const float *pp = sIn + (my * SA + kh * DA) * RWp + Cfg::col(mx * SA + kw * DA);
                const float *w = wA + (tap * GA + ga) * CIN * CPA;
                float v[CIN];
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci) v[ci] = pp[ci * RH * RWp];
#pragma unroll
                for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
                    for (int c = 0; c < CPA; ++c) acc[c] = fmaf(v[ci], w[ci * CPA + c], acc[c]);
            }
#pragma unroll
            for (int c = 0; c < CPA; ++c) {
                float v = fmaf(acc[c], sA_[coA + c], tA_[coA + c]);
                if (reluA) v = fmaxf(v, 0.0f);
                sMid[((coA + c) * MR + my) * MRp + mx] = valid ? v : 0.0f;
            }
        }
    }
    __syncthreads();
    LWS_STAMPK(STAMP_ID, 2);
    // phase 3: layer B on the 8 x 8 tile; wave = output-channel group of B, lane = pixel
    const int tx = lane & 7, ty = lane >> 3;
    const int ox = ox0 + tx, oy = oy0 + ty;
    if (ox >= WA || oy >= HA) return;
    const int coB = wave * CPB;
    const int oplane = HA * WA;
    const int64_t o = ((int64_t)b * COUT + coB) * oplane + oy * WA + ox;
    float rv[CPB];
#pragma unroll
    for (int c = 0; c < CPB; ++c) rv[c] = res != nullptr ? res[o + (int64_t)c * oplane] : 0.0f;   // in flight under the taps
    float acc[CPB];
#pragma unroll
    for (int c = 0; c < CPB; ++c) acc[c] = 0.0f;
#pragma unroll 3
    for (int tap = 0; tap < 9; ++tap) {
        const int kh = tap / 3, kw = tap - kh * 3;
        const float *pp = sMid + (ty + kh * DB) * MRp + tx + kw * DB;
        const float *w = wB + (tap * NW + wave) * CM * CPB;
        float v[CM];
#pragma unroll
        for (int ci = 0; ci < CM; ++ci) v[ci] = pp[ci * MR * MRp];
#pragma unroll
        for (int ci = 0; ci < CM; ++ci)
#pragma unroll
            for (int c = 0; c < CPB; ++c) acc[c] = fmaf(v[ci], w[ci * CPB + c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < CPB; ++c) {
        float v = acc[c];
        if (sB_ != nullptr) v = fmaf(v, sB_[coB + c], tB_[coB + c]);
        if (res != nullptr) v = v + rv[c];
        if (reluB) v = fmaxf(v, 0.0f);
        out[o + (int64_t)c * oplane] = v;
    }
    LWS_STAMPK(STAMP_ID, 3);
}

template <int CIN, int CM, int COUT, int SA, int DA, int DB, int NW>
static int conv2d_pair_launch(const Conv2dLayer &a, const Conv2dLayer &b, const float *in, const float *in2, int n1,
                              const float *res, float *out, int N, int H, int W, int HA, int WA, hipStream_t st)
{
    using Cfg = PairCfg<CIN, CM, COUT, SA, DA, DB, NW>;
    if (a.w_pair == nullptr || b.w_pair == nullptr || a.pair_groups != Cfg::GA || b.pair_groups != NW) {
        set_error("conv2d_pair: weights are not packed for this pair geometry");
        return LWS_ERR_STATE;
    }
    const size_t lds = (size_t)Cfg::LDS_FLOATS * sizeof(float);
    if (lds > 48 * 1024)
        if (const int rc = allow_dyn_lds<&k_conv2d_pair<CIN, CM, COUT, SA, DA, DB, NW>>((int)lds)) return rc;
    dim3 grid(cdiv(WA, 8), cdiv(HA, 8), N), block(Cfg::NT);
    hipLaunchKernelGGL((k_conv2d_pair<CIN, CM, COUT, SA, DA, DB, NW>), grid, block, lds, st, in, in2, n1, a.w_pair, a.bn_s,
                       a.bn_t, a.relu ? 1 : 0, b.w_pair, b.bn_s, b.bn_t, res, b.relu ? 1 : 0, out, H, W, HA, WA);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

// =============================================================================================
// The two 16-channel pairs (conv1+conv2 at 1/4, conv3+conv4 at 1/8 resolution: stride-2 3x3 CIN -> 16, then 3x3
// 16 -> 16) on fp32 MFMA: with 16 output channels a layer is exactly one 16-row MFMA tile, Out^T[cout, pixel] =
// sum_{tap, cin} W[cout, (tap, cin)] X[(tap, cin), pixel], K = 4 input channels of one tap per instruction, taps outer
// and channels ascending -- the same fma chain as the VALU kernel, so the results are bit-identical.  The LDS images
// are the planar ones of k_conv2d_pair (lane (n, g) reads channel 4j+g of pixel n with one ds_read_b32 at
// lane base + compile-time offset); the 9 x CIN/4 A fragments of a layer (one VGPR each) are loaded up front.
// 8 waves stage the input region; wave w < 7 owns pixels 16w .. 16w+15 of layer A's 10 x 10 region, waves 0..3 the
// 8 x 8 output tile (the layers are latency-bound: the short dependent MFMA chains matter, not the idle waves;
// 16-wave workgroups were no faster at batch 1 and are starved of LDS by the side stream's kernels at batch 8).
// =============================================================================================
template <int CIN>
struct PairMfmaCfg {
    static constexpr int NT = 512, MR = 10, MRp = 11, RH = 21, HALF = 11, RWp = 23;
    static constexpr int JA = CIN / 4, JB = 4;                       // K groups per tap of layer A / layer B
    static constexpr int PIN = RH * RWp, PMID = MR * MRp;            // plane strides
    static constexpr int ITEMS = CIN * RH * RH, SITER = (ITEMS + NT - 1) / NT;
    static constexpr int LDS_FLOATS = CIN * PIN + 16 * PMID;
    __host__ __device__ static constexpr int col(int rx) { return (rx & 1) * HALF + (rx >> 1); }
};

template <int CIN>
__global__ __launch_bounds__(512) void k_conv2d_pair_mfma(const float *__restrict__ in, const float *__restrict__ in2, int n1,
                                                          const float *__restrict__ wA,   // [tap][lane][JA] A fragments
                                                          const float *__restrict__ sA_, const float *__restrict__ tA_,
                                                          int reluA,
                                                          const float *__restrict__ wB,   // [tap][lane][4]
                                                          const float *__restrict__ sB_, const float *__restrict__ tB_,
                                                          int reluB, float *__restrict__ out, int H, int W, int HA, int WA)
{
    using Cfg = PairMfmaCfg<CIN>;
    constexpr int NT = Cfg::NT, MR = Cfg::MR, MRp = Cfg::MRp, RH = Cfg::RH, RWp = Cfg::RWp, JA = Cfg::JA, JB = Cfg::JB,
                  PIN = Cfg::PIN, PMID = Cfg::PMID, SITER = Cfg::SITER, RSZ = RH * RH;
    extern __shared__ float smem[];
    float *sIn = smem;                  // [CIN][RH][RWp], columns de-interleaved by parity
    float *sMid = smem + CIN * PIN;     // [16][MR][MRp]
    const int b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, g = lane >> 4;
    const int ox0 = blockIdx.x * 8, oy0 = blockIdx.y * 8;
    const int my0 = oy0 - 1, mx0 = ox0 - 1;
    const int iy0 = my0 * 2 - 1, ix0 = mx0 * 2 - 1;
    const int plane = H * W;
    const float *inb = b < n1 ? in + (int64_t)b * CIN * plane : in2 + (int64_t)(b - n1) * CIN * plane;
    [[maybe_unused]] constexpr int STAMP_ID = CIN == 8 ? 15 : 16;
    LWS_STAMPK(STAMP_ID, 0);
    {
        float v[SITER];
        bool okv[SITER];
#pragma unroll
        for (int i = 0; i < SITER; ++i) {
            const int it = tid + i * NT;
            const int ci = it / RSZ, r = it - ci * RSZ;
            const int ry = r / RH, rx = r - ry * RH;
            const int gy = iy0 + ry, gx = ix0 + rx;
            okv[i] = it < Cfg::ITEMS && gy >= 0 && gy < H && gx >= 0 && gx < W;
            v[i] = inb[okv[i] ? ci * plane + gy * W + gx : 0];
        }
        // A fragments and BatchNorm parameters of both layers, for the waves that compute (in flight with the input loads)
        float fa[9][JA], fb[9][JB];
        float4 bsA = make_float4(0.f, 0.f, 0.f, 0.f), btA = bsA, bsB = bsA, btB = bsA;
        if (wave * 16 < MR * MR) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int j = 0; j < JA; ++j) fa[tap][j] = wA[(tap * 64 + lane) * JA + j];
            bsA = *reinterpret_cast<const float4 *>(sA_ + 4 * g);
            btA = *reinterpret_cast<const float4 *>(tA_ + 4 * g);
        }
        if (wave < 4) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int j = 0; j < JB; ++j) fb[tap][j] = wB[(tap * 64 + lane) * JB + j];
            if (sB_ != nullptr) {
                bsB = *reinterpret_cast<const float4 *>(sB_ + 4 * g);
                btB = *reinterpret_cast<const float4 *>(tB_ + 4 * g);
            }
        }
#pragma unroll
        for (int i = 0; i < SITER; ++i) {
            const int it = tid + i * NT;
            const int ci = it / RSZ, r = it - ci * RSZ;
            const int ry = r / RH, rx = r - ry * RH;
            if (it < Cfg::ITEMS) sIn[ci * PIN + ry * RWp + Cfg::col(rx)] = okv[i] ? v[i] : 0.0f;
        }
        __syncthreads();
        LWS_STAMPK(STAMP_ID, 1);
        // layer A: wave = 16-pixel tile of the 10 x 10 region
        if (wave * 16 < MR * MR) {
            const int p = wave * 16 + n, pc = p < MR * MR ? p : MR * MR - 1;
            const int my = pc / MR, mx = pc - my * MR;
            const float *bp = sIn + g * PIN + (my * 2) * RWp + mx;
            floatx4 acc = (floatx4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
                for (int j = 0; j < JA; ++j)
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[tap][j], bp[(4 * j) * PIN + kh * RWp + Cfg::col(kw)], acc, 0, 0, 0);
            }
            const int ay = my0 + my, ax = mx0 + mx;
            const bool valid = ay >= 0 && ay < HA && ax >= 0 && ax < WA;
            if (p < MR * MR) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int co = 4 * g + e;
                    float r = fmaf(acc[e], f4c(bsA, e), f4c(btA, e));
                    if (reluA) r = fmaxf(r, 0.0f);
                    sMid[co * PMID + my * MRp + mx] = valid ? r : 0.0f;
                }
            }
        }
        __syncthreads();
        LWS_STAMPK(STAMP_ID, 2);
        // layer B: waves 0..3 = the four 16-pixel tiles of the 8 x 8 output tile
        if (wave < 4) {
            const int p = wave * 16 + n;
            const int ty = p >> 3, tx = p & 7;
            const float *bp = sMid + g * PMID + ty * MRp + tx;
            floatx4 acc = (floatx4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
                for (int j = 0; j < JB; ++j)
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[tap][j], bp[(4 * j) * PMID + kh * MRp + kw], acc, 0, 0, 0);
            }
            const int ox = ox0 + tx, oy = oy0 + ty;
            if (ox < WA && oy < HA) {
                const int oplane = HA * WA;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int co = 4 * g + e;
                    float r = acc[e];
                    if (sB_ != nullptr) r = fmaf(r, f4c(bsB, e), f4c(btB, e));
                    if (reluB) r = fmaxf(r, 0.0f);
                    out[((int64_t)b * 16 + co) * oplane + oy * WA + ox] = r;
                }
            }
        }
        LWS_STAMPK(STAMP_ID, 3);
    }
}

// [cout=16][cin][3][3] -> A fragments [tap][lane][cin/4]: lane (m, g) holds W[m][4j+g][tap] for j = 0..cin/4-1
void pack_pair_mfma(const float *w, int cin, float *out)
{
    const int J = cin / 4;
    for (int tap = 0; tap < 9; ++tap)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < J; ++j) {
                const int m = lane & 15, g = lane >> 4;
                out[((size_t)tap * 64 + lane) * J + j] = w[((size_t)m * cin + 4 * j + g) * 9 + tap];
            }
}

template <int CIN>
static int conv2d_pair_mfma_launch(const Conv2dLayer &a, const Conv2dLayer &b, const float *in, const float *in2, int n1,
                                   float *out, int N, int H, int W, int HA, int WA, hipStream_t st)
{
    using Cfg = PairMfmaCfg<CIN>;
    const size_t lds = (size_t)Cfg::LDS_FLOATS * sizeof(float);
    dim3 grid(cdiv(WA, 8), cdiv(HA, 8), N), block(Cfg::NT);
    LWS_LAUNCH_STOP((k_conv2d_pair_mfma<CIN>), grid, block, lds, st, in, in2, n1, a.w_mfma, a.bn_s, a.bn_t, a.relu ? 1 : 0,
                    b.w_mfma, b.bn_s, b.bn_t, b.relu ? 1 : 0, out, H, W, HA, WA);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

// Output-channel groups the pair kernel wants for layer i of the feature extractor (0..7: A, B, A, B, ...); the host
// packs w_pair as [tap][groups][cin][cout/groups].
int conv2d_pair_groups(int layer)
{
    static const int g[8] = {PairCfg<3, 4, 8, 2, 2, 4, 4>::GA,     4,  PairCfg<8, 4, 8, 1, 2, 2, 4>::GA,      4,
                             PairCfg<8, 16, 16, 2, 1, 1, 16>::GA, 16, PairCfg<16, 16, 16, 2, 1, 1, 16>::GA, 16};
    return layer >= 0 && layer < 8 ? g[layer] : 0;
}

// layer a (conv, BN) then layer b (conv stride 1, pad == dil) on N images [N,a.cin,H,W] -> [N,b.cout,HA,WA]
int launch_conv2d_pair(const Conv2dLayer &a, const Conv2dLayer &b, const float *in, const float *res, float *out, int N,
                       int H, int W, hipStream_t st, const float *in2, int n1)
{
    if (a.transposed || b.transposed || b.stride != 1 || b.pad != b.dil || a.pad != a.dil || a.bn_s == nullptr ||
        b.cin != a.cout) {
        set_error("conv2d_pair: unsupported layer pair");
        return LWS_ERR_INVALID;
    }
    if (in2 == nullptr) {
        in2 = in;
        n1 = N;
    }
    const int HA = (H + 2 * a.pad - 2 * a.dil - 1) / a.stride + 1, WA = (W + 2 * a.pad - 2 * a.dil - 1) / a.stride + 1;
    if (a.cout == 16 && b.cout == 16 && a.stride == 2 && a.dil == 1 && b.dil == 1 && res == nullptr &&
        a.w_mfma != nullptr && b.w_mfma != nullptr && (a.cin == 8 || a.cin == 16)) {
        if (a.cin == 8) return conv2d_pair_mfma_launch<8>(a, b, in, in2, n1, out, N, H, W, HA, WA, st);
        return conv2d_pair_mfma_launch<16>(a, b, in, in2, n1, out, N, H, W, HA, WA, st);
    }
#define LWS_C2P(CI, CMID, CO, SA, DA, DB, NW)                                                             \
    if (a.cin == CI && a.cout == CMID && b.cout == CO && a.stride == SA && a.dil == DA && b.dil == DB)    \
        return conv2d_pair_launch<CI, CMID, CO, SA, DA, DB, NW>(a, b, in, in2, n1, res, out, N, H, W, HA, WA, st);
    LWS_C2P(3, 4, 8, 2, 2, 4, 4) LWS_C2P(8, 4, 8, 1, 2, 2, 4) LWS_C2P(8, 16, 16, 2, 1, 1, 16) LWS_C2P(16, 16, 16, 2, 1, 1, 16)
#undef LWS_C2P
    set_error("conv2d_pair: unsupported pair %d -> %d -> %d (stride %d, dilations %d, %d)", a.cin, a.cout, b.cout, a.stride,
              a.dil, b.dil);
    return LWS_ERR_INVALID;
}

}  // namespace lws
