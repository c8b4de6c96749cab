// What lws_stixels.hip and lws_objects.hip share: the limits of a strip and of its histogram, the items a strip is read as, and
// take(p) of lws_stixels (include/lwsnet_hip.h), so that "a pixel that takes part" and its bin are written once.
#pragma once
#include "lws_geomkit.h"

namespace lws::takekit {

using namespace geomkit;

constexpr int kMaxBins = 4096;              // the strip's histogram in LDS: 16 KB
constexpr int kMaxSub = 16;
constexpr int kMaxDim = 16384;              // H: 64 rows per thread in the walk, r[y] in 16 KB; H, W: SQ stays below 2^36
constexpr int kMaxWidth = 64;               // r[y] <= 64 fits a byte

// u16(v) of lws_depth_maps, as the float32 it is before the conversion
__device__ __forceinline__ float u16f(float v) { return fminf(fmaxf(rintf(v * 256.0f), 0.0f), 65535.0f); }

// One item of a strip: the columns xs .. xs + 3 of the strip's row (dp, cp, hp point at the strip's first column; ws: its
// width).  Beyond the strip a disparity is NaN (never valid) and a code 0xff.
struct Item {
    float d[4];
    unsigned code[4];
};

__device__ __forceinline__ Item load_item(const float *__restrict__ dp, const uint8_t *__restrict__ cp, int xs, int ws)
{
    Item it;
    load_quad(dp, xs, ws, aligned(dp, 16), it.d);
    if (xs + 4 <= ws && aligned(cp + xs, 4)) {
        const uchar4 v = *reinterpret_cast<const uchar4 *>(cp + xs);
        it.code[0] = v.x, it.code[1] = v.y, it.code[2] = v.z, it.code[3] = v.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) it.code[i] = xs + i < ws ? cp[xs + i] : 0xffu;
    }
    return it;
}

struct Rule {
    float fb, min_disp, max_depth, fsub, fbins;
    unsigned code_bits;
};

// take(p) of lws_stixels: the pixel's bin, -1 when it takes no part.  The compare against the bin count is on the float.
__device__ __forceinline__ int bin_of(float d, unsigned code, const Rule &r)
{
    float z;
    const bool v = valid_z(d, true, r.fb, r.min_disp, r.max_depth, z);
    const float t = floorf(d * r.fsub);
    return v && code < 6u && ((r.code_bits >> code) & 1u) && t < r.fbins ? (int)t : -1;
}

}  // namespace lws::takekit
