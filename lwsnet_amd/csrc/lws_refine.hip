// Refinement of LWSNet, float32, -ffp-contract=off.
//
//   /root/reference/models/submodules.py:223-327, models/models.py:158-162
//                                   -> k_ref_first, k_ref_dws, k_ref_conv64, k_ref_conv64x, k_ref_last, k_ref_dws_last
//
// Arithmetic contract (oracle/lws_oracle.c lwso_conv2d / lwso_bn_add_relu): every convolution output is ONE fmaf
// chain from 0, taps (kh,kw) outer ascending, input channel inner ascending; zero padding (fmaf(0, w, acc) == acc,
// so padded taps may be fed as zeros); BatchNorm(eval) = fmaf(x, s, t); then the residual add; then ReLU.
//
// Layout: channels-last [B,H,W,32] maps: one pixel = one 128-byte line, so dilated taps (dilation 2..16) and the
// strided "phase grid" tiles below always move whole cache lines.
#include "lws_common.h"
#include "lws_device_math.h"

namespace lws {

LWS_DEFINE_STAMPS(refine)

// =============================================================================================
// Refinement, first convolution: NCHW image (3 ch) or disparity (1 ch) -> channels-last [B,H,W,32], 3x3 pad 1,
// no BatchNorm (submodules.py:284-291).  4 threads per pixel, 8 output channels each: a wave stores 16 whole lines.
// =============================================================================================
template <int CIN>
__global__ __launch_bounds__(256) void k_ref_first(const float *__restrict__ in, const float *__restrict__ wgt,   // [tap][ci][32]
                                                   float *__restrict__ out, int H, int W)
{
    __shared__ __attribute__((aligned(16))) float sW[9 * CIN * 32];
    for (int i = threadIdx.x; i < 9 * CIN * 32; i += 256) sW[i] = wgt[i];
    __syncthreads();
    const int64_t plane = (int64_t)H * W;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t pix = idx >> 2;
    const int grp = (int)(idx & 3), b = blockIdx.y;
    if (pix >= plane) return;
    const int y = (int)(pix / W), x = (int)(pix % W);
    const float *inb = in + (int64_t)b * CIN * plane;
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.0f;
#pragma unroll 3
    for (int tap = 0; tap < 9; ++tap) {
        const int kh = tap / 3, kw = tap - kh * 3;
        const int iy = y + kh - 1, ix = x + kw - 1;
        const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
            const float ld = inb[ok ? (int64_t)ci * plane + (int64_t)iy * W + ix : 0];
            const float v = ok ? ld : 0.0f;
            const float4 w0 = *reinterpret_cast<const float4 *>(&sW[(tap * CIN + ci) * 32 + grp * 8]);
            const float4 w1 = *reinterpret_cast<const float4 *>(&sW[(tap * CIN + ci) * 32 + grp * 8 + 4]);
            acc[0] = fmaf(v, w0.x, acc[0]);
            acc[1] = fmaf(v, w0.y, acc[1]);
            acc[2] = fmaf(v, w0.z, acc[2]);
            acc[3] = fmaf(v, w0.w, acc[3]);
            acc[4] = fmaf(v, w1.x, acc[4]);
            acc[5] = fmaf(v, w1.y, acc[5]);
            acc[6] = fmaf(v, w1.z, acc[6]);
            acc[7] = fmaf(v, w1.w, acc[7]);
        }
    }
    float4 *o = reinterpret_cast<float4 *>(out + ((int64_t)b * plane + pix) * 32 + grp * 8);
    o[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    o[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// =============================================================================================
// Phase-grid tiles for dilated 3x3 layers.  With dilation d the taps of pixel (y,x) are (y +- d, x +- d): pixels
// of the same phase (y mod d, x mod d) form an ordinary dense 3x3 problem on a grid subsampled by d.  A
// workgroup owns RT_Y x RT_X pixels of ONE phase inside an image block of (RT_Y*d) x (RT_X*d) pixels, so its halo
// is (RT_Y+2) x (RT_X+2) pixels for every dilation (1.56x read amplification instead of 9 re-reads), and every
// pixel it touches is a whole 128-byte line of the channels-last map.
// =============================================================================================
constexpr int RT_Y = 8, RT_X = 16;                // k_ref_dws tile: 8 rows of 16 pixels (one MFMA N-tile per row)
constexpr int RH_Y = RT_Y + 2, RH_X = RT_X + 2;   // halo tile
constexpr int RVS = 32;                           // LDS pixel stride in dwords: 32 channels, no padding ...

// ... instead the eight 16-byte channel groups of pixel p are XOR-swizzled with (p & 7): ds_read_b128 of 8
// consecutive pixels at the same group then covers all 64 banks, and the LDS image stays 128 B per pixel
// (k_ref_dws fits 4 workgroups per CU, k_ref_conv64 5).
__device__ __forceinline__ int swz(int p, int grp) { return p * RVS + ((grp ^ (p & 7)) << 2); }

struct RefTile {
    int b, Y0, X0;
};

// Block -> tile: dispatch order, the dilation phase fastest (consecutive blocks own the phases of one image block).  Measured
// r03 and removed: XCD-contiguous runs of that list, and the phase slowest inside an XCD's run -- 66.0 vs 69.3 / 67.2 us per
// k_ref_dws launch at 8 x 256x512 (profiles/r03/experiments/rbench_b8_ref_order.txt): the halo re-reads already hit L2 / the
// Infinity Cache (tools/micro/copybw.hip: a phase-grid copy costs the same with and without the halo).
__device__ __forceinline__ RefTile ref_tile(int dil, int nbx, int nby)
{
    int bid = blockIdx.x;
    const int d2 = dil * dil;
    const int phase = bid % d2;
    bid /= d2;
    const int bx = bid % nbx;
    bid /= nbx;
    const int by = bid % nby;
    RefTile t;
    t.b = bid / nby;
    t.Y0 = by * RT_Y * dil + phase / dil;
    t.X0 = bx * RT_X * dil + phase % dil;
    return t;
}

// Staging of a dense 32-channel halo tile of HY x HX pixels that starts PAD pixels before the tile origin (Y0, X0): item = (halo
// pixel hp, 4-channel group c4), hp = (tid >> 3) + 32 i.  Unconditional clamped loads, all in flight; okv[i] = the item exists
// and lies in the image.
constexpr int halo32_iters(int npx) { return (npx * 8 + 255) / 256; }
template <int HY, int HX, int PAD>
__device__ __forceinline__ void halo32_loads(const float *inb, int Y0, int X0, int H, int W, int tid,
                                             float4 (&c)[halo32_iters(HY * HX)], bool (&okv)[halo32_iters(HY * HX)])
{
    const int c4 = tid & 7;
#pragma unroll
    for (int i = 0; i < halo32_iters(HY * HX); ++i) {
        const int hp = (tid >> 3) + 32 * i;
        const int hy = hp / HX, hx = hp - hy * HX;
        const int gy = Y0 + (hy - PAD), gx = X0 + (hx - PAD);
        okv[i] = hp < HY * HX && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const int off = okv[i] ? (gy * W + gx) * 32 + c4 * 4 : 0;      // one image < 2^31 floats
        c[i] = *reinterpret_cast<const float4 *>(inb + off);
    }
}

// Per-thread weights of a depthwise-separable block: the pointwise A fragments and this thread's depthwise taps (its channel
// group c4 is fixed)
__device__ __forceinline__ void dws_weights(const float4 *pwpk, const float *dw, int lane, int c4, float4 (&aw)[2][2], float4 (&wd)[9])
{
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) aw[q][mt] = pwpk[(q * 2 + mt) * 64 + lane];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) wd[tap] = *reinterpret_cast<const float4 *>(dw + tap * 32 + c4 * 4);
}

// Pointwise 32 -> 32 on fp32 MFMA: Out^T[cout, pixel] = W[cout, cin] * X[cin, pixel] for NTW N-tiles of 16 pixels (bv[r][q]: the
// B operand of tile r, channels 16q ..) x both output-channel tiles, K = 32 = 8 MFMAs per accumulator, channels ascending
template <int NTW>
__device__ __forceinline__ void pointwise32_mfma(const float4 (&aw)[2][2], const float4 (&bv)[NTW][2], floatx4 (&acc)[NTW][2])
{
#pragma unroll
    for (int r = 0; r < NTW; ++r)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) acc[r][mt] = (floatx4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < NTW; ++r)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    acc[r][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(aw[q][mt], j), f4c(bv[r][q], j), acc[r][mt], 0, 0, 0);
}

// Output store of a phase-grid tile (refinement2[0], both forms): this wave's R tile rows from row0 on, both output-channel
// tiles; lane (n, g) holds channels 16mt + 4g .. +3 of pixel (row, n).  outb: the image's map [H,W,32].
template <int R>
__device__ __forceinline__ void store_tile_rows(float *outb, const RefTile t, int row0, const floatx4 (&acc)[R][2], int H, int W,
                                                int dil, int n, int g, int wt)
{
    const int gx = t.X0 + n * dil;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int gy = t.Y0 + (row0 + r) * dil;
        if (gy < H && gx < W) {
            float *o = outb + ((int64_t)gy * W + gx) * 32;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                store_act4(o + mt * 16 + 4 * g, make_float4(acc[r][mt][0], acc[r][mt][1], acc[r][mt][2], acc[r][mt][3]), wt);
        }
    }
}

// =============================================================================================
// Depthwise-separable block (submodules.py:238-261): BatchNorm(32) -> ReLU -> depthwise 3x3 (dilated) ->
// pointwise 1x1 (32 -> 32), all in one kernel:
//   1. stage the halo tile with BN+ReLU applied (out-of-image pixels are literal zeros = the conv padding);
//   2. depthwise on VALU: one thread = (pixel, 4 channels), 9 float4 taps from LDS, result written to a second
//      LDS image in MFMA B-operand order (4x4-transposed inside each 16-channel group, see lws_conv3d.hip);
//   3. pointwise on fp32 MFMA: Out^T[cout, pixel] = W[cout, cin] * X[cin, pixel], K = 32 = 8 MFMAs per tile;
//   4. store the raw result (the next block applies its own BatchNorm while staging).
// =============================================================================================
// LDS images of k_ref_dws are planar by 4-channel group: sA[c4][halo pixel] and sB[4q+g][tile pixel] as float4, so
// that every depthwise tap and every transposed write is base + compile-time offset (no per-tap address VALU);
// plane strides of 186 / 130 float4 put the 8 planes of one pixel 40 / 8 dwords apart mod 64: conflict-free b128.
constexpr int DWS_SA = 186, DWS_SB = 130;

// FIRST = CIN > 0 fuses the CIN -> 32 convolution in front of the block (refinement1_disp[0] with CIN = 1, refinement1_left[0]
// with CIN = 3, submodules.py:282-300: 3x3, pad 1, no BN/ReLU) into the staging: `in` is then the [B,CIN,H,W] image and wf the
// convolution's MFMA A fragments (pack_first_mfma); every halo pixel's 32 channels are recomputed from a dense
// (RH_Y-1)*dil+3 x (RH_X-1)*dil+3 window of every input plane held in LDS (aliased onto sB, which is not live yet) with the same
// fmaf chain as k_ref_first -- taps ascending, input channel inner (first_conv_mfma).  Requires dil = 2.  The 32-channel map the
// separate launch would write and this block read back (128 B per pixel each way) never exists.
// (Round 4 built the CIN = 1 form on packed FMA, round 6 the CIN = 3 form likewise: neutral; on MFMA both pay -- profiles/NOTES.md.)
constexpr int DWS_FD = 2, DWS_FR = (RH_Y - 1) * DWS_FD + 3, DWS_FC = (RH_X - 1) * DWS_FD + 3;
static_assert(DWS_FR * DWS_FC <= 1024 && 3 * DWS_FR * DWS_FC <= 8 * DWS_SB * 4, "first-conv window must fit 4 loads/thread/plane and sB");

// The fused CIN -> 32 convolution on fp32 MFMA: Out^T[cout, halo pixel] = W[cout, k] X[k, pixel] with k = 3 tap + ci (taps
// ascending, input channel inner: k_ref_first's chain, which v_mfma_f32_16x16x4_f32 reproduces k by k), K = 9 CIN padded to a
// multiple of 4 with zero weights (fmaf(x, 0, acc) == acc).  The 180 halo pixels are 12 N-tiles of 16, three per wave; lane
// (n, g) of MFMA j supplies window value k = 4 j + g of pixel n -- one ds_read_b32 at a per-lane offset, shared by the two
// output-channel tiles -- and ends up with channels 16 mt + 4 g .. + 3 of pixel n: exactly one float4 slot of sA.
template <int CIN>
__device__ __forceinline__ void first_conv_mfma(const float *sImg, const float *__restrict__ wfrag,   // [mt][j][lane]
                                                const float *__restrict__ bn_s, const float *__restrict__ bn_t, float4 *sA,
                                                int Y0, int X0, int H, int W, int lane, int wave)
{
    constexpr int WIN = DWS_FR * DWS_FC, K = 9 * CIN, J = (K + 3) / 4, NPX = RH_Y * RH_X, NTW = 3;
    static_assert(4 * NTW * 16 >= NPX, "three N-tiles per wave must cover the halo tile");
    const int n = lane & 15, g = lane >> 4;
    float a[2][J];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int j = 0; j < J; ++j) a[mt][j] = wfrag[(mt * J + j) * 64 + lane];
    int koff[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k = 4 * j + g, tap = k / CIN, ci = k - tap * CIN, kh = tap / 3, kw = tap - kh * 3;
        koff[j] = k < K ? ci * WIN + kh * DWS_FC + kw : 0;
    }
    float4 s4[2], t4[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        s4[mt] = *reinterpret_cast<const float4 *>(bn_s + (mt * 4 + g) * 4);
        t4[mt] = *reinterpret_cast<const float4 *>(bn_t + (mt * 4 + g) * 4);
    }
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        const int hp = (wave * NTW + nt) * 16 + n;
        const int hy = hp / RH_X, hx = hp - hy * RH_X;
        const float *sp = sImg + (hp < NPX ? (hy * DWS_FD) * DWS_FC + hx * DWS_FD : 0);
        floatx4 acc[2] = {(floatx4){0.f, 0.f, 0.f, 0.f}, (floatx4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const float b = sp[koff[j]];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][j], b, acc[mt], 0, 0, 0);
        }
        const int gy = Y0 + (hy - 1) * DWS_FD, gx = X0 + (hx - 1) * DWS_FD;
        const bool ok = hp < NPX && gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            float4 v = bn_relu4(make_float4(acc[mt][0], acc[mt][1], acc[mt][2], acc[mt][3]), s4[mt], t4[mt]);
            if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (hp < NPX) sA[(mt * 4 + g) * DWS_SA + hp] = v;
        }
    }
}

template <int FIRST>
__global__ __launch_bounds__(256, 4) void k_ref_dws(const float *__restrict__ in, const float *__restrict__ wf,
                                                 const float *__restrict__ bn_s,
                                                 const float *__restrict__ bn_t, const float *dw,   // [tap][32]
                                                 const float4 *pwpk,                              // [q][mt][lane]
                                                 float *__restrict__ out, int H, int W, int dil, int nbx, int nby, int wt,
                                                 const float *__restrict__ plow, int ph, int pw, float *__restrict__ pmat,
                                                 float ioff)
{
    // (FIRST == 1 only) plow != nullptr: the disparity map has not been materialised -- it is evaluated on demand as
    // upsample(plow [ph,pw]) + in (DeferredMap) and this workgroup writes its own tile pixels of it to pmat (the
    // phase-grid tiles of all workgroups partition the image, so the map is written exactly once)
    __shared__ float4 sA[8 * DWS_SA];
    __shared__ float4 sB[8 * DWS_SB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RefTile t = ref_tile(dil, nbx, nby);
    LWS_STAMPK(5, 0);

    const int c4 = tid & 7;
    const float4 s4 = *reinterpret_cast<const float4 *>(bn_s + c4 * 4);
    const float4 t4 = *reinterpret_cast<const float4 *>(bn_t + c4 * 4);

    // 1. stage: item = (halo pixel hp, 4-channel group c4); hp = (tid >> 3) + 32 i.  Unconditional clamped loads first.
    //    (The FIRST == 0 loads are halo32_loads with a dilation, and the store below is store_tile_rows with a 32-bit pixel index;
    //    both keep their own lines, which hold this kernel's machine code where it was -- profiles/NOTES.md, "Refinement file pass".)
    constexpr int NPX = RH_Y * RH_X, SITER = (NPX * 8 + 255) / 256;
    float4 c[SITER];
    bool okv[SITER];
    if (FIRST == 3) {
        // three input planes: the windows go to sImg[ci][DWS_FR * DWS_FC], all loads of a thread in flight together
        float *sImg = reinterpret_cast<float *>(sB);
        constexpr int WIN = DWS_FR * DWS_FC, NLD = (3 * WIN + 255) / 256;
        const float *inb = in + (int64_t)t.b * 3 * H * W;
        const int gy0 = t.Y0 - DWS_FD - 1, gx0 = t.X0 - DWS_FD - 1;
        float iv[NLD];
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int r3 = tid + 256 * k;
            const int ci = r3 / WIN, r = r3 - ci * WIN;
            const int ry = r / DWS_FC, rx = r - ry * DWS_FC;
            const int gy = gy0 + ry, gx = gx0 + rx;
            const bool ok = r3 < 3 * WIN && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const float ld = inb[ok ? (int64_t)ci * H * W + (int64_t)gy * W + gx : 0];
            iv[k] = ok ? ld : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < NLD; ++k)
            if (tid + 256 * k < 3 * WIN) sImg[tid + 256 * k] = iv[k];
        __syncthreads();
        first_conv_mfma<3>(sImg, wf, bn_s, bn_t, sA, t.Y0, t.X0, H, W, lane, wave);
        __syncthreads();          // sImg (= sB) is dead from here; sA is complete
    } else if (FIRST == 1) {
        float *sImg = reinterpret_cast<float *>(sB);
        DeferredMap dm{plow != nullptr ? plow + (int64_t)t.b * ph * pw : nullptr, in + (int64_t)t.b * H * W, ph, pw,
                       (float)H, 1.0f / (float)(ph > 0 ? ph : 1)};
        dm.off = ioff;
        const int gy0 = t.Y0 - DWS_FD - 1, gx0 = t.X0 - DWS_FD - 1;
        float iv[4];
        bool iok[4];
        int iys[4], ixs[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = tid + 256 * k;
            const int ry = r / DWS_FC, rx = r - ry * DWS_FC;
            const int gy = gy0 + ry, gx = gx0 + rx;
            iok[k] = r < DWS_FR * DWS_FC && gy >= 0 && gy < H && gx >= 0 && gx < W;
            iys[k] = iok[k] ? gy : 0;
            ixs[k] = iok[k] ? gx : 0;
        }
        deferred_at_n<4>(dm, iys, ixs, H, W, iv);       // all loads of the four points in flight together
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (tid + 256 * k < DWS_FR * DWS_FC) sImg[tid + 256 * k] = iok[k] ? iv[k] : 0.0f;
        __syncthreads();
        if (pmat != nullptr && tid < RT_Y * RT_X) {
            const int ty = tid / RT_X, tx = tid - ty * RT_X;
            const int gy = t.Y0 + ty * DWS_FD, gx = t.X0 + tx * DWS_FD;
            if (gy < H && gx < W)
                pmat[(int64_t)t.b * H * W + (int64_t)gy * W + gx] = sImg[((ty + 1) * DWS_FD + 1) * DWS_FC + (tx + 1) * DWS_FD + 1];
        }
        first_conv_mfma<1>(sImg, wf, bn_s, bn_t, sA, t.Y0, t.X0, H, W, lane, wave);
        __syncthreads();          // sImg (= sB) is dead from here; sA is complete
    } else {
        const float *inb = in + (int64_t)t.b * H * W * 32;
#pragma unroll
        for (int i = 0; i < SITER; ++i) {
            const int hp = (tid >> 3) + 32 * i;
            const int hy = hp / RH_X, hx = hp - hy * RH_X;
            const int gy = t.Y0 + (hy - 1) * dil, gx = t.X0 + (hx - 1) * dil;
            okv[i] = hp < NPX && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const int off = okv[i] ? (gy * W + gx) * 32 + c4 * 4 : 0;      // one image < 2^31 floats
            c[i] = *reinterpret_cast<const float4 *>(inb + off);
        }
    }
    float4 aw[2][2], wd[9];
    dws_weights(pwpk, dw, lane, c4, aw, wd);
    if (FIRST == 0) {
#pragma unroll
        for (int i = 0; i < SITER; ++i) {
            const int hp = (tid >> 3) + 32 * i;
            float4 v = bn_relu4(c[i], s4, t4);
            if (!okv[i]) v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (hp < NPX) sA[c4 * DWS_SA + hp] = v;
        }
        __syncthreads();
    }
    LWS_STAMPK(5, 1);

    // 2. depthwise: thread = (4-channel group c4, column x, row group rg): the four tile pixels (4 rg + j, x), j = 0..3.  The six
    //    halo rows those pixels read are walked ONCE (round 5): row rr feeds pixel j as its tap row kh = rr - j, so every pixel
    //    still receives its taps (kh, kw) ascending -- the chain of the contract -- from 18 ds_read_b128 per thread instead of
    //    the 36 of one-pixel-at-a-time (the phase is LDS-bandwidth-bound: four workgroups per CU, 2.9 k cycles each, r05 stamps)
    {
        const int q = c4 >> 2, a_ = c4 & 3;
        const int x = (tid >> 3) & 15, rg = tid >> 7;
        const float4 *src = sA + c4 * DWS_SA + (4 * rg) * RH_X + x;
        float4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) {
            const float4 t0 = src[rr * RH_X], t1 = src[rr * RH_X + 1], t2 = src[rr * RH_X + 2];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kh = rr - j;
                if (kh >= 0 && kh < 3) {
                    fma4(acc[j], t0, wd[kh * 3 + 0]);        // four channels: two v_pk_fma_f32
                    fma4(acc[j], t1, wd[kh * 3 + 1]);
                    fma4(acc[j], t2, wd[kh * 3 + 2]);
                }
            }
        }
        // channel 16q + 4a_ + e -> plane 4q + e, element a_ (the 4x4 transpose the MFMA B operand wants)
        float *dst = reinterpret_cast<float *>(sB + (4 * q) * DWS_SB + (4 * rg) * RT_X + x) + a_;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dst[(0 * DWS_SB + RT_X * j) * 4] = acc[j].x;
            dst[(1 * DWS_SB + RT_X * j) * 4] = acc[j].y;
            dst[(2 * DWS_SB + RT_X * j) * 4] = acc[j].z;
            dst[(3 * DWS_SB + RT_X * j) * 4] = acc[j].w;
        }
    }
    __syncthreads();
    LWS_STAMPK(5, 2);

    // 3. pointwise MFMA: wave handles tile rows 2*wave, 2*wave+1 x both output-channel tiles
    const int n = lane & 15, g = lane >> 4;
    floatx4 acc[2][2];
    float4 bv[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int q = 0; q < 2; ++q) bv[r][q] = sB[(4 * q + g) * DWS_SB + (2 * wave + r) * RT_X + n];
    pointwise32_mfma(aw, bv, acc);

    LWS_STAMPK(5, 3);
    // 4. store: lane (n, g) holds channels 16mt + 4g .. +3 of pixel (row, n)
    float *outb = out + (int64_t)t.b * H * W * 32;
    const int gx = t.X0 + n * dil;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int gy = t.Y0 + (2 * wave + r) * dil;
        if (gy < H && gx < W) {
            float *o = outb + (gy * W + gx) * 32;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                store_act4(o + mt * 16 + 4 * g, make_float4(acc[r][mt][0], acc[r][mt][1], acc[r][mt][2], acc[r][mt][3]), wt);
        }
    }
}

// =============================================================================================
// refinement2[0] (submodules.py:304-309): BatchNorm(64) -> ReLU -> Conv 3x3 dilation 8, 64 -> 32, on the
// concatenation [refined_left, refined_disp] (models.py:160) -- the concat is never materialised: the two
// channels-last maps are staged side by side.  fp32-MFMA implicit GEMM, K = 9 taps x 64 channels = 144 MFMAs per
// accumulator; weights streamed from L2 in fragment order one step ahead (same scheme as k_conv3d_mid16).
// =============================================================================================
constexpr int C64X_VSB = 208;                        // split-bf16 form: LDS pixel stride in bytes, 3 variants x 64 B + 16 B
constexpr int C64X_STEP_U4 = 2 * 3 * 64;             // ... and uint4 per (tap, tensor) step of its packed weights

// Both forms: the RT_Y x RT_X tile of k_ref_dws, NW waves of RW rows each; staging item = (tensor, halo pixel, 16-channel
// group) = 64 bytes of the concat, it = 2 (tensor * NPX + halo pixel) + group
struct Conv64Cfg {
    static constexpr int NW = 4, NT = 64 * NW, RW = RT_Y / NW, NPX = RH_Y * RH_X;
    static constexpr int ITEMS = 2 * NPX * 2, SITER = (ITEMS + NT - 1) / NT;
    static constexpr int LDS_BYTES = 2 * NPX * C64X_VSB;      // k_ref_conv64x only
    static_assert(RW == 2, "sub-steps j < RW of k_ref_conv64's step prefetch the fragments, the other two the weights");
};

// Staging loads of the concat [inL, inD], both forms: unconditional, clamped loads first (see k_ref_dws)
__device__ __forceinline__ void conv64_stage_loads(const float *__restrict__ inL, const float *__restrict__ inD, const RefTile t,
                                                   int H, int W, int dil, int tid, float4 (&c)[Conv64Cfg::SITER][4],
                                                   bool (&okv)[Conv64Cfg::SITER])
{
    using Cfg = Conv64Cfg;
#pragma unroll
    for (int i = 0; i < Cfg::SITER; ++i) {
        const int it = tid + i * Cfg::NT;
        const int q = it & 1, hp = (it >> 1) % Cfg::NPX, ten = (it >> 1) / Cfg::NPX;
        const int hy = hp / RH_X, hx = hp % RH_X;
        const int gy = t.Y0 + (hy - 1) * dil, gx = t.X0 + (hx - 1) * dil;
        okv[i] = it < Cfg::ITEMS && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const float *base = (ten == 1 && it < Cfg::ITEMS ? inD : inL) + (int64_t)t.b * H * W * 32;
        const float4 *src = reinterpret_cast<const float4 *>(base + (okv[i] ? ((int64_t)gy * W + gx) * 32 + q * 16 : 0));
#pragma unroll
        for (int k = 0; k < 4; ++k) c[i][k] = src[k];
    }
}

__global__ __launch_bounds__(Conv64Cfg::NT) void k_ref_conv64(const float *__restrict__ inL, const float *__restrict__ inD,
                                                              const float *__restrict__ bn_s, const float *__restrict__ bn_t,   // [64]
                                                              const float4 *__restrict__ wpk,   // [tap][qq][mt][lane]
                                                              float *__restrict__ out, int H, int W, int dil, int nbx, int nby, int wt)
{
    using Cfg = Conv64Cfg;
    constexpr int NPX = Cfg::NPX, RW = Cfg::RW, NT = Cfg::NT, SITER = Cfg::SITER;
    __shared__ __attribute__((aligned(16))) float sA[2 * NPX * RVS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RefTile t = ref_tile(dil, nbx, nby);
    const int n = lane & 15, g = lane >> 4;
    LWS_STAMPK(6, 0);

    // stage: BN + ReLU of the loaded items (zeros outside the image), into the two LDS images
    {
        float4 c[SITER][4];
        bool okv[SITER];
        conv64_stage_loads(inL, inD, t, H, W, dil, tid, c, okv);
#pragma unroll
        for (int i = 0; i < SITER; ++i) {
            const int it = tid + i * NT;
            if (it < Cfg::ITEMS) {
                const int q = it & 1, hp = (it >> 1) % NPX, ten = (it >> 1) / NPX;
                const float4 *sp = reinterpret_cast<const float4 *>(bn_s + ten * 32 + q * 16);
                const float4 *tp = reinterpret_cast<const float4 *>(bn_t + ten * 32 + q * 16);
                float4 a[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 v = c[i][k], sc = sp[k], tt = tp[k];
                    a[k] = make_float4(bn_relu2(v.x, sc.x, tt.x), bn_relu2(v.y, sc.y, tt.y), bn_relu2(v.z, sc.z, tt.z),
                                       bn_relu2(v.w, sc.w, tt.w));
                    if (!okv[i]) a[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                float *img = sA + ten * NPX * RVS;      // 4x4 transpose inside the 16-channel group, swizzled groups
                *reinterpret_cast<float4 *>(&img[swz(hp, 4 * q + 0)]) = make_float4(a[0].x, a[1].x, a[2].x, a[3].x);
                *reinterpret_cast<float4 *>(&img[swz(hp, 4 * q + 1)]) = make_float4(a[0].y, a[1].y, a[2].y, a[3].y);
                *reinterpret_cast<float4 *>(&img[swz(hp, 4 * q + 2)]) = make_float4(a[0].z, a[1].z, a[2].z, a[3].z);
                *reinterpret_cast<float4 *>(&img[swz(hp, 4 * q + 3)]) = make_float4(a[0].w, a[1].w, a[2].w, a[3].w);
            }
        }
    }
    // weights [tap][qq][mt][lane] (+ one all-zero tap so the next-tap prefetch needs no bounds check)
    const float4 *wp = wpk + lane;
    float4 wbuf[2][4][2];                           // ping-pong over taps (copied once per tap: 8 v_mov per 32 MFMAs)
#pragma unroll
    for (int qq = 0; qq < 4; ++qq)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) wbuf[0][qq][mt] = wp[(qq * 2 + mt) * 64];
    __syncthreads();
    LWS_STAMPK(6, 1);

    floatx4 acc[RW][2];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) acc[r][mt] = (floatx4){0.f, 0.f, 0.f, 0.f};
    // step = (tap, qq): qq = 2*tensor + 16-channel group -> input channels 16*qq .. 16*qq+15 of the concat
    auto frag = [&](int r, int tap, int qq) {
        const int hp = (RW * wave + r + tap / 3) * RH_X + n + tap % 3;
        return *reinterpret_cast<const float4 *>(&sA[(qq >> 1) * NPX * RVS + swz(hp, 4 * (qq & 1) + g)]);
    };
    // 4 steps per tap (even): activation fragments ping-pong by step parity; prefetches are issued in fenced slices
    // between the MFMA groups of the current step (see k_conv3d_mid16)
    float4 bbuf[2][RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) bbuf[0][r] = frag(r, 0, 0);
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const int tn = tap < 8 ? tap + 1 : 8;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            float4 *bc = bbuf[qq & 1], *bn = bbuf[(qq & 1) ^ 1];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int r = 0; r < RW; ++r)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
                        acc[r][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(wbuf[0][qq][mt], j), f4c(bc[r], j), acc[r][mt], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (j < RW) bn[j] = qq < 3 ? frag(j, tap, qq + 1) : frag(j, tn, 0);
                else {             // next tap's 8 weight fragments: one per (qq, j in {2,3})
                    const int l = qq * 2 + (j - RW);
                    wbuf[1][l >> 1][l & 1] = wp[(((tap + 1) * 4 + (l >> 1)) * 2 + (l & 1)) * 64];
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) wbuf[0][qq][mt] = wbuf[1][qq][mt];
    }
    LWS_STAMPK(6, 2);
    store_tile_rows(out + (int64_t)t.b * H * W * 32, t, RW * wave, acc, H, W, dil, n, g, wt);
    LWS_STAMPK(6, 3);
}

// =============================================================================================
// refinement2[0], split-bf16 form (k_ref_conv64x; option "split_bf16" bit 2, NOT the default and never what bench.py's
// headline measures: like k_conv3d_mid16x it is not bit-exact against the oracle chain, see lws_conv3d.hip).
// Same tile and interface as k_ref_conv64.  The BN + ReLU'd halo pixels are split into hi / mid / lo bf16 while they are
// staged ([tensor][halo pixel][variant][32 channels] bf16, 208-byte pixel stride); one step = (tap, tensor) contracts 32
// input channels with six v_mfma_f32_16x16x32_bf16 per accumulator, smallest cross terms first.  Weights are pre-split on
// the host into A fragments [step][mt][variant][lane][8] (pack_conv64_bf16x3) and streamed two steps ahead through a
// three-slot register ring; activation fragments are double-buffered by step parity.
// =============================================================================================
__global__ __launch_bounds__(Conv64Cfg::NT) void k_ref_conv64x(const float *__restrict__ inL, const float *__restrict__ inD,
                                                               const float *__restrict__ bn_s, const float *__restrict__ bn_t,   // [64]
                                                               const uint4 *__restrict__ wpk,   // [20][2][3][64] x 8 bf16
                                                               float *__restrict__ out, int H, int W, int dil, int nbx, int nby, int wt)
{
    using Cfg = Conv64Cfg;
    constexpr int NPX = Cfg::NPX, RW = Cfg::RW, NT = Cfg::NT, SITER = Cfg::SITER, VSB = C64X_VSB;
    extern __shared__ __attribute__((aligned(16))) float lds64x[];
    unsigned char *ldsb = reinterpret_cast<unsigned char *>(lds64x);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RefTile t = ref_tile(dil, nbx, nby);
    const int n = lane & 15, g = lane >> 4;
    LWS_STAMPK(21, 0);

    // stage: item = (tensor, halo pixel, 16-channel group) = 64 B of float32 -> BN + ReLU -> 3 x 32 B of bf16
    {
        float4 c[SITER][4];
        bool okv[SITER];
        conv64_stage_loads(inL, inD, t, H, W, dil, tid, c, okv);
#pragma unroll
        for (int i = 0; i < SITER; ++i) {
            const int it = tid + i * NT;
            if (it < Cfg::ITEMS) {
                const int q = it & 1, pix = it >> 1, ten = pix / NPX;     // pix = ten * NPX + hp: the images are back to back
                const float4 *sp = reinterpret_cast<const float4 *>(bn_s + ten * 32 + q * 16);
                const float4 *tp = reinterpret_cast<const float4 *>(bn_t + ten * 32 + q * 16);
                uint32_t pk[3][8];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 v = c[i][k], sc = sp[k], tt = tp[k];
                    float xs[4] = {bn_relu2(v.x, sc.x, tt.x), bn_relu2(v.y, sc.y, tt.y), bn_relu2(v.z, sc.z, tt.z),
                                   bn_relu2(v.w, sc.w, tt.w)};
#pragma unroll
                    for (int e = 0; e < 4; e += 2)
                        split_bf16x3_pair(okv[i] ? xs[e] : 0.f, okv[i] ? xs[e + 1] : 0.f, pk[0][2 * k + e / 2],
                                          pk[1][2 * k + e / 2], pk[2][2 * k + e / 2]);
                }
#pragma unroll
                for (int v3 = 0; v3 < 3; ++v3) {
                    uint4 *dst = reinterpret_cast<uint4 *>(ldsb + pix * VSB + v3 * 64 + q * 32);
                    dst[0] = make_uint4(pk[v3][0], pk[v3][1], pk[v3][2], pk[v3][3]);
                    dst[1] = make_uint4(pk[v3][4], pk[v3][5], pk[v3][6], pk[v3][7]);
                }
            }
        }
    }
    const uint4 *wp = wpk + lane;
    uint4 wa[3][2][3];                              // ring over steps: step s lives in slot s % 3 (6 steps per kh iteration)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int v3 = 0; v3 < 3; ++v3) {
            wa[0][mt][v3] = wp[(mt * 3 + v3) * 64];
            wa[1][mt][v3] = wp[C64X_STEP_U4 + (mt * 3 + v3) * 64];
        }
    __syncthreads();
    LWS_STAMPK(21, 1);

    floatx4 acc[RW][2];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) acc[r][mt] = (floatx4){0.f, 0.f, 0.f, 0.f};
    const unsigned char *rptr[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) rptr[r] = ldsb + ((RW * wave + r) * RH_X + n) * VSB + g * 16;
    uint4 bb[2][RW][3];                             // double-buffered by step parity; the step loop is fully unrolled
    auto load_b_row = [&](uint4 (&dst)[RW][3], int r, int off) {
#pragma unroll
        for (int v3 = 0; v3 < 3; ++v3) dst[r][v3] = *reinterpret_cast<const uint4 *>(rptr[r] + off + v3 * 64);
    };
#pragma unroll
    for (int r = 0; r < RW; ++r) load_b_row(bb[0], r, 0);

    // step = 2 tap + tensor.  One step = 6 terms x (RW x 2 accumulators); the prefetches ride in the MFMA gaps one at a time
    // (see k_conv3d_mid16x): the next step's fragments, then the weights of step + 2 into the ring slot of step - 1
    static_assert(2 * (3 * RW + 6) <= 6 * RW * 2, "one prefetch behind every second MFMA");
#pragma unroll
    for (int s = 0; s < 18; ++s) {
        const int cb = s & 1, nb = cb ^ 1;
        const int sn = s < 17 ? s + 1 : 17;                              // (clamped: the last prefetch is unused)
        const int off_n = (((sn >> 1) / 3) * RH_X + (sn >> 1) % 3) * VSB + (sn & 1) * NPX * VSB;
        auto prefetch = [&](int k) {                                     // as in k_conv3d_mid16x: one load per call
            if (k < 3 * RW)
                bb[nb][k / 3][k % 3] = *reinterpret_cast<const uint4 *>(rptr[k / 3] + off_n + (k % 3) * 64);
            else if (k < 3 * RW + 6)
                wa[(s + 2) % 3][(k - 3 * RW) / 3][(k - 3 * RW) % 3] = wp[(size_t)(s + 2) * C64X_STEP_U4 + (k - 3 * RW) * 64];
        };
#pragma unroll
        for (int T = 0; T < 6; ++T)
#pragma unroll
            for (int r = 0; r < RW; ++r)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    acc[r][mt] = mfma_split_bf16_term(acc[r][mt], wa[s % 3][mt], bb[cb][r], T);
                    const int m = (T * RW + r) * 2 + mt;                 // one prefetch behind every second MFMA
                    if (m % 2 == 0 && m / 2 < 3 * RW + 6) {
                        __builtin_amdgcn_sched_barrier(0);
                        prefetch(m / 2);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
    }
    LWS_STAMPK(21, 2);
    store_tile_rows(out + (int64_t)t.b * H * W * 32, t, RW * wave, acc, H, W, dil, n, g, wt);
    LWS_STAMPK(21, 3);
}

// =============================================================================================
// refinement2[5] + skip (submodules.py:318-325, models.py:161-162): Conv 3x3 pad 1, 32 -> 1, plus pred3.
// =============================================================================================
constexpr int LAST_TY = 8, LAST_TX = 32, LAST_HY = LAST_TY + 2, LAST_HX = LAST_TX + 2, LAST_NPX = LAST_HY * LAST_HX;
constexpr int LAST_PS = 346;     // plane stride in float4 (>= 340)

__global__ __launch_bounds__(256) void k_ref_last(const float *__restrict__ in, const float *__restrict__ wgt,   // [tap][32]
                                                  const float *__restrict__ pred3, float *__restrict__ out, int H, int W)
{
    // Workgroup = 8 x 32 output pixels, one per thread; the 10 x 34 halo tile is staged in LDS planar by 4-channel
    // group (a wave's ds_read_b128 of 64 neighbouring pixels in one plane is 1 KiB contiguous: conflict-free).
    __shared__ float4 sA[8 * LAST_PS];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int x0 = blockIdx.x * LAST_TX, y0 = blockIdx.y * LAST_TY;
    const float *inb = in + (int64_t)b * H * W * 32;
    LWS_STAMPK(9, 0);
    constexpr int ITEMS = LAST_NPX * 8, SITER = (ITEMS + 255) / 256;
    const int c4 = tid & 7;
    float4 c[SITER];
    bool okv[SITER];
    halo32_loads<LAST_HY, LAST_HX, 1>(inb, y0, x0, H, W, tid, c, okv);
#pragma unroll
    for (int i = 0; i < SITER; ++i) {
        const int hp = (tid >> 3) + 32 * i;
        if (hp < LAST_NPX) sA[c4 * LAST_PS + hp] = okv[i] ? c[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    LWS_STAMPK(9, 1);
    const int tx = tid & 31, ty = tid >> 5;
    const int x = x0 + tx, y = y0 + ty;
    const bool live = x < W && y < H;
    const int64_t o = ((int64_t)b * H + (live ? y : 0)) * W + (live ? x : 0);
    const float skip = pred3[o];                      // issued now: its latency hides behind the 288 fmas
    float acc = 0.0f;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const float4 *p = sA + (ty + kh) * LAST_HX + tx + kw;
            const float *w = wgt + (kh * 3 + kw) * 32;
#pragma unroll
            for (int g8 = 0; g8 < 8; ++g8) {
                const float4 a = p[g8 * LAST_PS];
                acc = fmaf(a.x, w[g8 * 4 + 0], acc);
                acc = fmaf(a.y, w[g8 * 4 + 1], acc);
                acc = fmaf(a.z, w[g8 * 4 + 2], acc);
                acc = fmaf(a.w, w[g8 * 4 + 3], acc);
            }
        }
    LWS_STAMPK(9, 2);
    if (live) out[o] = acc + skip;
    LWS_STAMPK(9, 3);
}

// =============================================================================================
// refinement2[4] (the last depthwise-separable block, dilation 1) + refinement2[5] + skip in ONE launch (round 5; VERDICT r4
// item 4: "k_ref_last inside the last k_ref_dws").  A workgroup owns RT_Y x RT_X output pixels of pred4; it needs the block's
// 32-channel output on the (RT_Y+2) x (RT_X+2) ring around them, which it computes itself from a (RT_Y+4) x (RT_X+4) input
// tile -- the same per-value chains as k_ref_dws (depthwise: taps ascending; pointwise: channels ascending on fp32 MFMA) and
// k_ref_last (taps outer, channels ascending, then + pred3), so the bits are those of the two launches.  What it saves: one
// launch on the chain and the write + read of one [B,H,W,32] map; what it pays: 1.41x of the block's arithmetic (the ring)
// and half the occupancy (56 KB of LDS).  Ring pixels outside the image are literal zeros: the padding of refinement2[5].
// =============================================================================================
constexpr int FL_IY = RT_Y + 4, FL_IX = RT_X + 4, FL_NIN = FL_IY * FL_IX;     // input tile 12 x 20
constexpr int FL_MY = RT_Y + 2, FL_MX = RT_X + 2, FL_NM = FL_MY * FL_MX;      // block-output ring tile 10 x 18 = 180 pixels
constexpr int FL_NT = (FL_NM + 15) / 16;                                      // 12 MFMA N-tiles (192 columns, 12 unused)
constexpr int FL_SA = 242, FL_SB = 194, FL_SC = 186;                          // plane strides in float4: 8 / 8 / 40 dwords mod 64
static_assert(FL_SA >= FL_NIN && FL_SB >= FL_NT * 16 && FL_SC >= FL_NM && FL_SC <= FL_SA, "k_ref_dws_last LDS planes");
static_assert(FL_NT % 4 == 0, "N-tiles split evenly over 4 waves");

__global__ __launch_bounds__(256, 2) void k_ref_dws_last(const float *__restrict__ in, const float *__restrict__ bn_s,
                                                         const float *__restrict__ bn_t, const float *dw,   // [tap][32]
                                                         const float4 *pwpk,                              // [q][mt][lane]
                                                         const float *__restrict__ wlast,                 // [tap][32]
                                                         const float *__restrict__ pred3, float *__restrict__ out, int H,
                                                         int W, int nbx, int nby)
{
    __shared__ float4 sA[8 * FL_SA];       // BN+ReLU'd input tile, planar by 4-channel group; later (sC) the block's output ring
    __shared__ float4 sB[8 * FL_SB];       // depthwise result in MFMA B-operand order
    float4 *sC = sA;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const RefTile t = ref_tile(1, nbx, nby);
    const int c4 = tid & 7;
    const float4 s4 = *reinterpret_cast<const float4 *>(bn_s + c4 * 4);
    const float4 t4 = *reinterpret_cast<const float4 *>(bn_t + c4 * 4);
    const float *inb = in + (int64_t)t.b * H * W * 32;

    // 1. stage the input tile (item = (pixel, 4-channel group); unconditional clamped loads, all in flight)
    constexpr int SITER = (FL_NIN * 8 + 255) / 256;
    float4 c[SITER];
    bool okv[SITER];
    halo32_loads<FL_IY, FL_IX, 2>(inb, t.Y0, t.X0, H, W, tid, c, okv);
    float4 aw[2][2], wd[9];
    dws_weights(pwpk, dw, lane, c4, aw, wd);
#pragma unroll
    for (int i = 0; i < SITER; ++i) {
        const int hp = (tid >> 3) + 32 * i;
        float4 v = bn_relu4(c[i], s4, t4);
        if (!okv[i]) v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (hp < FL_NIN) sA[c4 * FL_SA + hp] = v;
    }
    __syncthreads();

    // 2. depthwise on the ring tile: pixel p = (tid >> 3) + 32 i
    {
        const int q = c4 >> 2, a_ = c4 & 3;
        constexpr int DITER = (FL_NM * 8 + 255) / 256;
#pragma unroll
        for (int i = 0; i < DITER; ++i) {
            const int p = (tid >> 3) + 32 * i;
            if (p < FL_NM) {
                const int my = p / FL_MX, mx = p - my * FL_MX;
                const float4 *src = sA + c4 * FL_SA + my * FL_IX + mx;
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) fma4(acc, src[kh * FL_IX + kw], wd[kh * 3 + kw]);
                float *dst = reinterpret_cast<float *>(sB + (4 * q) * FL_SB + p) + a_;
                dst[(0 * FL_SB) * 4] = acc.x;
                dst[(1 * FL_SB) * 4] = acc.y;
                dst[(2 * FL_SB) * 4] = acc.z;
                dst[(3 * FL_SB) * 4] = acc.w;
            }
        }
    }
    __syncthreads();          // sB complete; sA is dead (sC may be written)

    // 3. pointwise on fp32 MFMA: wave w owns N-tiles 3w .. 3w+2 (16 ring pixels each) x both output-channel tiles
    {
        constexpr int NTW = FL_NT / 4;
        const int n = lane & 15, g = lane >> 4;
        floatx4 acc[NTW][2];
        float4 bv[NTW][2];
#pragma unroll
        for (int r = 0; r < NTW; ++r)
#pragma unroll
            for (int q = 0; q < 2; ++q) bv[r][q] = sB[(4 * q + g) * FL_SB + (wave * NTW + r) * 16 + n];
        pointwise32_mfma(aw, bv, acc);
        // lane (n, g) holds channels 16 mt + 4 g .. + 3 of ring pixel p -> plane 4 mt + g of sC; zeros outside the image
#pragma unroll
        for (int r = 0; r < NTW; ++r) {
            const int p = (wave * NTW + r) * 16 + n;
            if (p < FL_NM) {
                const int my = p / FL_MX, mx = p - my * FL_MX;
                const int gy = t.Y0 + my - 1, gx = t.X0 + mx - 1;
                const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    sC[(4 * mt + g) * FL_SC + p] = ok ? make_float4(acc[r][mt][0], acc[r][mt][1], acc[r][mt][2], acc[r][mt][3])
                                                      : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
    __syncthreads();

    // 4. refinement2[5] + pred3: one thread per output pixel (k_ref_last's chain)
    if (tid < RT_Y * RT_X) {
        const int ty = tid >> 4, tx = tid & 15;
        const int y = t.Y0 + ty, x = t.X0 + tx;
        const bool live = y < H && x < W;
        const int64_t o = ((int64_t)t.b * H + (live ? y : 0)) * W + (live ? x : 0);
        const float skip = pred3[o];
        float acc = 0.0f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const float4 *p = sC + (ty + kh) * FL_MX + tx + kw;
                const float *w = wlast + (kh * 3 + kw) * 32;
#pragma unroll
                for (int g8 = 0; g8 < 8; ++g8) {
                    const float4 a = p[g8 * FL_SC];
                    acc = fmaf(a.x, w[g8 * 4 + 0], acc);
                    acc = fmaf(a.y, w[g8 * 4 + 1], acc);
                    acc = fmaf(a.z, w[g8 * 4 + 2], acc);
                    acc = fmaf(a.w, w[g8 * 4 + 3], acc);
                }
            }
        if (live) out[o] = acc + skip;
    }
}

// =============================================================================================
// host side
// =============================================================================================
int launch_ref_first(const float *in, int cin, const float *w, float *out, int B, int H, int W, hipStream_t st)
{
    dim3 grid((unsigned)(((int64_t)H * W * 4 + 255) / 256), B), block(256);
    if (cin == 3) hipLaunchKernelGGL(k_ref_first<3>, grid, block, 0, st, in, w, out, H, W);
    else if (cin == 1) hipLaunchKernelGGL(k_ref_first<1>, grid, block, 0, st, in, w, out, H, W);
    else {
        set_error("ref_first: unsupported cin %d", cin);
        return LWS_ERR_INVALID;
    }
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

// Launch geometry of the phase-grid kernels (ref_tile): image blocks of (RT_Y * dil) x (RT_X * dil) pixels, dil * dil phases
// of each, B images.
struct RefGrid {
    int nbx, nby;
    dim3 grid;
};
static RefGrid ref_grid(int B, int H, int W, int dil)
{
    const int nbx = cdiv(W, RT_X * dil), nby = cdiv(H, RT_Y * dil);
    return {nbx, nby, dim3(nbx * nby * dil * dil * B)};
}

// One k_ref_dws launch.  kernel: k_ref_dws<FIRST>; wfrag: the fused first convolution's fragments (FIRST != 0); def: the
// deferred disparity map a FIRST == 1 block reads and writes out, or nullptr.
static void ref_dws_launch(decltype(&k_ref_dws<0>) kernel, const RefDws &l, const float *in, const float *wfrag, float *out, int B,
                           int H, int W, hipStream_t st, float ioff, const StageMap *def = nullptr)
{
    const RefGrid g = ref_grid(B, H, W, l.dil);
    hipLaunchKernelGGL(kernel, g.grid, dim3(256), 0, st, in, wfrag, l.bn_s, l.bn_t, l.dw, reinterpret_cast<const float4 *>(l.pw), out,
                       H, W, l.dil, g.nbx, g.nby, use_wt_stores((size_t)B * H * W * 128), def ? def->low : nullptr, def ? def->h : 0,
                       def ? def->w : 0, def ? def->mem : nullptr, ioff);
}

int launch_ref_dws(const RefDws &l, const float *in, float *out, int B, int H, int W, hipStream_t st)
{
    ref_dws_launch(k_ref_dws<0>, l, in, nullptr, out, B, H, W, st, 0.5f);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

// CIN -> 32 first convolution + the first depthwise-separable block in one launch (refinement1_disp: cin = 1, on a map that may
// be deferred; refinement1_left: cin = 3)
bool ref_first_dws_can_fuse(const RefDws &l, int cin) { return (cin == 1 || cin == 3) && l.dil == DWS_FD; }

// A fragments of the fused first convolution for first_conv_mfma: [mt][j][lane], lane (m, g) -> W[16 mt + m][k = 4 j + g],
// k = cin * tap + ci (zero beyond 9 cin); w is the Conv2D weight [32][cin][3][3]
int packed_first_mfma_floats(int cin) { return 2 * ((9 * cin + 3) / 4) * 64; }
void pack_first_mfma(const float *w, int cin, float *out)
{
    const int K = 9 * cin, J = (K + 3) / 4;
    for (int mt = 0; mt < 2; ++mt)
        for (int j = 0; j < J; ++j)
            for (int lane = 0; lane < 64; ++lane) {
                const int m = lane & 15, g = lane >> 4, k = 4 * j + g, tap = k / cin, ci = k % cin;
                out[(mt * J + j) * 64 + lane] = k < K ? w[((16 * mt + m) * cin + ci) * 9 + tap] : 0.0f;
            }
}

int launch_ref_first_dws(const RefDws &l, StageMap &in, int cin, const float *wfrag, float *out, int B, int H, int W,
                         hipStream_t st, float ioff)
{
    if (!ref_first_dws_can_fuse(l, cin)) {
        set_error("ref_first_dws: cin %d / dilation %d unsupported", cin, l.dil);
        return LWS_ERR_INVALID;
    }
    if (cin != 1 && !in.written) {
        set_error("ref_first_dws: only the one-channel (disparity) input can be a deferred map");
        return LWS_ERR_INVALID;
    }
    const int rc = check_stage_map(in, false, "ref_first_dws");
    if (rc) return rc;
    const bool def = !in.written;      // (the kernel writes a deferred map out: its tiles partition the image)
    const float *img = def ? in.prev->mem : in.mem;
    ref_dws_launch(cin == 3 ? k_ref_dws<3> : k_ref_dws<1>, l, img, wfrag, out, B, H, W, st, ioff, def ? &in : nullptr);
    LWS_LAUNCH_CHECK();
    in.written = true;
    return LWS_OK;
}

int launch_ref_conv64(const RefConv64 &l, const float *inL, const float *inD, float *out, int B, int H, int W,
                      hipStream_t st)
{
    const int dil = 8, wt = use_wt_stores((size_t)B * H * W * 128);
    using Cfg = Conv64Cfg;                        // both forms: 8-row tiles, 4 waves x 2 rows
    const RefGrid g = ref_grid(B, H, W, dil);
    if (l.form == 1) {
        // split-bf16 form: 73 KB of LDS (2 workgroups per CU)
        if (const int rc = allow_dyn_lds<&k_ref_conv64x>(Cfg::LDS_BYTES)) return rc;
        hipLaunchKernelGGL(k_ref_conv64x, g.grid, dim3(Cfg::NT), Cfg::LDS_BYTES, st, inL, inD, l.bn_s, l.bn_t,
                           reinterpret_cast<const uint4 *>(l.wx), out, H, W, dil, g.nbx, g.nby, wt);
    } else {
        // 46 KB LDS (3 workgroups per CU): 50.5 / 349 us at B = 1 / 8 (r01, 256x512; the floor is 31 / 246 us of fp32 MFMA
        // issue).  Measured and dropped: 4-row tiles x 4 waves 54.3 / 390 us, 4-row x 2 waves 66.2 / 403 us, 2-row x 1 wave
        // 53.8 / 408 us.
        hipLaunchKernelGGL(k_ref_conv64, g.grid, dim3(Cfg::NT), 0, st, inL, inD, l.bn_s, l.bn_t,
                           reinterpret_cast<const float4 *>(l.w), out, H, W, dil, g.nbx, g.nby, wt);
    }
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

// refinement2[4] (dilation 1) + refinement2[5] + pred3 in one launch (k_ref_dws_last)
bool ref_dws_last_can_fuse(const RefDws &l) { return l.dil == 1; }

int launch_ref_dws_last(const RefDws &l, const float *in, const float *wlast, const float *pred3, float *out, int B, int H, int W,
                        hipStream_t st)
{
    if (!ref_dws_last_can_fuse(l)) {
        set_error("ref_dws_last: dilation %d unsupported", l.dil);
        return LWS_ERR_INVALID;
    }
    const RefGrid g = ref_grid(B, H, W, 1);
    hipLaunchKernelGGL(k_ref_dws_last, g.grid, dim3(256), 0, st, in, l.bn_s, l.bn_t, l.dw, reinterpret_cast<const float4 *>(l.pw),
                       wlast, pred3, out, H, W, g.nbx, g.nby);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

int launch_ref_last(const float *in, const float *w, const float *pred3, float *out, int B, int H, int W, hipStream_t st)
{
    dim3 grid(cdiv(W, LAST_TX), cdiv(H, LAST_TY), B), block(256);
    hipLaunchKernelGGL(k_ref_last, grid, block, 0, st, in, w, pred3, out, H, W);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

// [cout=32][cin][kh][kw] with cin in 16-channel groups -> A fragments [tap][qq][mt][lane][j]
void pack_conv2d_mfma(const float *w, int cin, int ktaps, float *out)
{
    const int Q = cin / 16;
    for (int tap = 0; tap < ktaps; ++tap)
        for (int q = 0; q < Q; ++q)
            for (int mt = 0; mt < 2; ++mt)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j) {
                        const int m = lane & 15, g = lane >> 4;
                        const int co = 16 * mt + m, ci = 16 * q + 4 * j + g;
                        out[((((size_t)tap * Q + q) * 2 + mt) * 64 + lane) * 4 + j] = w[((size_t)co * cin + ci) * ktaps + tap];
                    }
}

// k_ref_conv64x: lane l of (step = 2 tap + tensor, mt, variant) holds W[16 mt + (l & 15)][32 tensor + 8 (l >> 4) + j][tap],
// j = 0..7, as bf16 bits; 18 steps + two all-zero steps (the two-steps-ahead prefetch needs no bounds check)
size_t packed_conv64x_floats() { return (size_t)20 * 2 * 3 * 64 * 4; }
void pack_conv64_bf16x3(const float *w, float *out)
{
    uint16_t *ox = reinterpret_cast<uint16_t *>(out);
    for (int step = 0; step < 20; ++step)
        for (int mt = 0; mt < 2; ++mt)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int tap = step >> 1, co = 16 * mt + (lane & 15), ci = 32 * (step & 1) + 8 * (lane >> 4) + j;
                    uint32_t v[3] = {0, 0, 0};
                    if (step < 18) split_bf16x3(w[((size_t)co * 64 + ci) * 9 + tap], v[0], v[1], v[2]);
                    for (int t = 0; t < 3; ++t) ox[((((size_t)step * 2 + mt) * 3 + t) * 64 + lane) * 8 + j] = (uint16_t)v[t];
                }
}

}  // namespace lws
