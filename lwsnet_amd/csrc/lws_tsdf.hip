// Volumetric fusion of a sequence: a truncated signed distance volume that frames are integrated into with their poses, ray-cast
// back into a camera and extracted as oriented, coloured points.  Contract: include/lwsnet_tsdf.h; one IEEE float32 operation per
// step (the build has no contraction and correctly rounded division and square root), so tests/tsdf_reference.py restates every
// output bit for bit in numpy.
//
// Launches (fixed lists: they depend on the arguments, never on the data; nothing is read back):
//   lws_tsdf_integrate   k_ts_zero (updated given) updated[B] = 0 -- a kernel, as k_tp_zero: see lws_photometric.hip on memset nodes
//                        k_ts_integrate  one thread per four voxels along x, the frame loop inside with the quad's state in registers.
//                        A wave covers 256 consecutive voxels of a row: their projections are neighbouring pixels of a few image
//                        rows, so the one-tap gathers of disp, sigma, mask, normals and rgb come out of L2.  The volume is touched
//                        only where a frame takes a voxel: the quad is loaded at its first take and stored once after the last
//                        frame, as 16-byte words where it is whole and aligned.  Outside every frustum a quad costs the three
//                        row products and a compare per frame and no traffic.  No cull of rows or tiles: a conservative bound on
//                        the projection of a row would have to hold under float32 rounding of u and v, which was not shown.
//   lws_tsdf_raycast     k_ts_raycast  one thread per pixel; a step gathers the eight taps of Wt and, where all are known, of T.
//                        Neighbouring rays walk neighbouring cells, so a wave's taps share cache lines.
//   lws_tsdf_points      k_ts_count, k_ts_scan, k_ts_scatter: lws_point_cloud's form (lws_packkit.h) with an x-row of the volume in
//                        the place of an image row, 64-bit offsets (a volume has up to 3 * 2^31 edges) and a capacity.  The same
//                        three launches (tsdfkit::launch_points) give lws_tsdf_mesh (lws_tsdf_mesh.hip) its vertices.
// Determinism: a voxel, a pixel and a record belong to one thread; what crosses threads is the integer add of `updated` and the
// ballots of the scatter.  0 bytes of scratch.
#include "lws_tsdfkit.h"

namespace lws {

namespace {

using namespace tsdfkit;                                    // Vol, observed, edge_bits, voxel_normal
using namespace packkit;                                    // kThreads, kWaves
using u64 = unsigned long long;

// ---- integrate ----
struct IntArgs {                                            // by value in the kernel arguments
    const float *disp, *sigma;
    const uint8_t *mask;
    const float *normals;
    const uint8_t *rgb;
    const float *cam, *pose;
    int B, H, W;
    float *T, *Wt;
    unsigned *C;                                            // one word {r, g, b, a} per voxel
    int Gx, Gy, Gz, nq;
    float ox, oy, oz, vs, sigma0, min_disp, max_depth, mu0, mu_d, sigma_min;
    int wmode;
    float w_max;
    u64 *updated;
};

__device__ __forceinline__ unsigned sat8(float x) { return (unsigned)fminf(fmaxf(x, 0.0f), 255.0f); }

// grid (B): updated[b] = 0
__global__ void k_ts_zero(u64 *__restrict__ updated)
{
    if (threadIdx.x == 0) updated[blockIdx.x] = 0;
}

// grid (ceil(Gz * Gy * nq / 256)): one thread per quad of an x-row.  COLOUR: C and rgb are given.
template <bool COLOUR>
__global__ __launch_bounds__(kThreads) void k_ts_integrate(IntArgs a)
{
    __shared__ int s_n[2][kWaves];
    const int t = threadIdx.x;
    const int64_t q_all = (int64_t)blockIdx.x * kThreads + t;
    const bool active = q_all < (int64_t)a.Gz * a.Gy * a.nq;     // an idle thread stays for the barriers and touches nothing
    const int64_t q = active ? q_all : 0;
    const int64_t row = q / a.nq;
    const int x = 4 * (int)(q - row * a.nq);
    const int iz = (int)(row / a.Gy), iy = (int)(row - (int64_t)iz * a.Gy);
    const int64_t base = row * a.Gx + x;
    float *Tp = a.T + base, *Wp = a.Wt + base;
    unsigned *Cp = COLOUR ? a.C + base : nullptr;
    const bool whole = x + 4 <= a.Gx;
    const bool vec = whole && aligned(Tp, 16) && aligned(Wp, 16), vecc = whole && aligned(Cp, 16);
    const float yw = a.oy + (float)iy * a.vs, zw = a.oz + (float)iz * a.vs;
    const int H = a.H, W = a.W;
    const int64_t plane = (int64_t)H * W;
    float To[4] = {0.0f, 0.0f, 0.0f, 0.0f}, Wo[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned Co[4] = {0u, 0u, 0u, 0u};
    unsigned touched = 0u;                                  // bit i: voxel x + i was taken by some frame
    for (int b = 0; b < a.B; ++b) {
        int n_taken = 0;
        if (active) {
            const Cam c = load_cam(a.cam, b);
            const float *p0 = pose_of(a.pose, b);
            const int64_t img = (int64_t)b * plane;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (x + i >= a.Gx) continue;
                const float xw = a.ox + (float)(x + i) * a.vs;
                const float Px = row_dot(p0, 0, xw, yw, zw), Py = row_dot(p0, 1, xw, yw, zw), Pz = row_dot(p0, 2, xw, yw, zw);
                float u, v;
                if (!(Pz > 0.0f && project(c, Px, Py, Pz, H, W, 0, u, v))) continue;
                const int iu = (int)rintf(u), iv = (int)rintf(v);       // in the image: 0 <= u <= W - 1, 0 <= v <= H - 1
                const int64_t px = img + (int64_t)iv * W + iu;
                const float d = a.disp[px];
                const bool ok = !a.mask || a.mask[px] == 1;
                float z;
                bool valid = valid_z(d, ok, c.fb, a.min_disp, a.max_depth, z);
                const float s = a.sigma ? a.sigma[px] : a.sigma0;
                valid = valid && s >= 0.0f && __builtin_isfinite(s);
                if (!valid) continue;
                const float sg = fmaxf(s, a.sigma_min);
                float sdf = z - Pz;
                if (a.normals) {
                    const float *np = a.normals + 3 * img + (int64_t)iv * W + iu;
                    const float nx = np[0], ny = np[plane], nz = np[2 * plane];
                    if (nx != 0.0f || ny != 0.0f || nz != 0.0f) {
                        const float X = back_x(c, iu, z), Y = back_y(c, iv, z);
                        sdf = -(((X - Px) * nx + (Y - Py) * ny) + (z - Pz) * nz);
                    }
                }
                const float zz = (z * z) / c.fb;
                const float mu = fmaxf(a.mu0, a.mu_d * zz);
                const float sz = sg * zz;
                const float w = a.wmode == 0 ? 1.0f : 1.0f / (sz * sz);
                if (!(sdf >= -mu && __builtin_isfinite(w) && w > 0.0f)) continue;
                if (!touched) {                             // the quad's first take: its state comes in
                    if (vec) {
                        const float4 tv = *reinterpret_cast<const float4 *>(Tp), wv = *reinterpret_cast<const float4 *>(Wp);
                        To[0] = tv.x, To[1] = tv.y, To[2] = tv.z, To[3] = tv.w;
                        Wo[0] = wv.x, Wo[1] = wv.y, Wo[2] = wv.z, Wo[3] = wv.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (x + j < a.Gx) To[j] = Tp[j], Wo[j] = Wp[j];
                    }
                    if (COLOUR) {
                        if (vecc) {
                            const uint4 cv = *reinterpret_cast<const uint4 *>(Cp);
                            Co[0] = cv.x, Co[1] = cv.y, Co[2] = cv.z, Co[3] = cv.w;
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (x + j < a.Gx) Co[j] = Cp[j];
                        }
                    }
                }
                touched |= 1u << i;
                ++n_taken;
                const float tt = fminf(sdf, mu), Wn = Wo[i] + w;
                const bool seen = Wo[i] > 0.0f;
                if (COLOUR) {
                    if (sdf <= mu) {
                        const uint8_t *cp = a.rgb + 3 * px;
                        const bool blend = seen && (Co[i] >> 24) == 255u;
                        unsigned word = 255u << 24;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const unsigned cn = cp[k], co = (Co[i] >> (8 * k)) & 255u;
                            const unsigned m = blend ? sat8(rintf(((float)co * Wo[i] + (float)cn * w) / Wn)) : cn;
                            word |= m << (8 * k);
                        }
                        Co[i] = word;
                    } else if (!seen) {
                        Co[i] = 0u;
                    }
                }
                To[i] = seen ? (To[i] * Wo[i] + tt * w) / Wn : tt;
                Wo[i] = fminf(Wn, a.w_max);
            }
        }
        if (a.updated) {                                    // (uniform)
            const int total = block_sum(n_taken, s_n[b & 1]);   // one barrier per frame: the next frame writes the other half of s_n
            if (t == 0 && total) __hip_atomic_fetch_add(a.updated + b, (u64)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (!touched) return;
    if (vec) {
        *reinterpret_cast<float4 *>(Tp) = make_float4(To[0], To[1], To[2], To[3]);
        *reinterpret_cast<float4 *>(Wp) = make_float4(Wo[0], Wo[1], Wo[2], Wo[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((touched >> j) & 1u) Tp[j] = To[j], Wp[j] = Wo[j];
    }
    if (COLOUR) {
        if (vecc) {
            *reinterpret_cast<uint4 *>(Cp) = make_uint4(Co[0], Co[1], Co[2], Co[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((touched >> j) & 1u) Cp[j] = Co[j];
        }
    }
}

// ---- raycast ----
struct Sample { bool inside, known; float f, wf; };

// sample(P) of the header; f is computed only where known, wf only where inside and WANT_W
template <bool WANT_W>
__device__ __forceinline__ Sample sample(const Vol &v, float px, float py, float pz)
{
    Sample s = {false, false, 0.0f, 0.0f};
    const float gx = (px - v.ox) / v.vs, gy = (py - v.oy) / v.vs, gz = (pz - v.oz) / v.vs;
    s.inside = gx >= 0.0f && gx < (float)(v.Gx - 1) && gy >= 0.0f && gy < (float)(v.Gy - 1) && gz >= 0.0f && gz < (float)(v.Gz - 1);
    if (!s.inside) return s;
    const int ix = (int)floorf(gx), iy = (int)floorf(gy), iz = (int)floorf(gz);       // 0 <= i0 <= G - 2: both taps are inside
    const float ax = gx - (float)ix, ay = gy - (float)iy, az = gz - (float)iz;
    const int i000 = (iz * v.Gy + iy) * v.Gx + ix, sy = v.Gx, sz = v.Gy * v.Gx;          // Gx * Gy * Gz < 2^31
    const int o[8] = {i000, i000 + 1, i000 + sy, i000 + sy + 1, i000 + sz, i000 + sz + 1, i000 + sz + sy, i000 + sz + sy + 1};
    float w[8];
    bool known = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        w[k] = v.Wt[o[k]];
        known = known && observed(w[k], v.w_min);
    }
    s.known = known;
    if (WANT_W) s.wf = lerp(blend4(w[0], w[1], w[2], w[3], ax, ay), blend4(w[4], w[5], w[6], w[7], ax, ay), az);
    if (known) {
        float f[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = v.T[o[k]];
        s.f = lerp(blend4(f[0], f[1], f[2], f[3], ax, ay), blend4(f[4], f[5], f[6], f[7], ax, ay), az);
    }
    return s;
}

// grid (ceil(H * W / 256), B): one thread per pixel.
__global__ __launch_bounds__(kThreads) void k_ts_raycast(Vol v, const float *__restrict__ cam, const float *__restrict__ pose, int H, int W,
                                                        float z_near, float step, int nsteps, float *__restrict__ disp,
                                                        float *__restrict__ weight, float *__restrict__ normals)
{
    const int64_t plane = (int64_t)H * W, s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (s >= plane) return;
    const int y = (int)(s / W), x = (int)(s - (int64_t)y * W);
    const Cam c = load_cam(cam, b);
    const float *p0 = pose_of(pose, b), *p1 = inverse_of(pose, b);
    const float xn = ((float)x - c.cx) / c.fx, yn = ((float)y - c.cy) / c.fy;
    bool pk = false, hit = false;
    float fp = 0.0f, zp = 0.0f, zs = 0.0f;
    for (int k = 0; k < nsteps; ++k) {
        const float zc = z_near + (float)k * step;
        const float X = xn * zc, Y = yn * zc;
        const Sample sm = sample<false>(v, row_dot(p1, 0, X, Y, zc), row_dot(p1, 1, X, Y, zc), row_dot(p1, 2, X, Y, zc));
        if (sm.known && pk) {
            if (fp > 0.0f && sm.f <= 0.0f) {
                zs = zp + (fp / (fp - sm.f)) * (zc - zp);
                hit = true;
                break;
            }
            if (fp <= 0.0f && sm.f > 0.0f) break;
        }
        pk = sm.known, fp = sm.f, zp = zc;
    }
    float d = 0.0f, wf = 0.0f, n[3] = {0.0f, 0.0f, 0.0f};
    if (hit) {
        d = c.fb / zs;
        if (weight || normals) {
            const float X = xn * zs, Y = yn * zs;
            const float hx = row_dot(p1, 0, X, Y, zs), hy = row_dot(p1, 1, X, Y, zs), hz = row_dot(p1, 2, X, Y, zs);
            if (weight) {
                const Sample h = sample<true>(v, hx, hy, hz);
                wf = h.inside ? h.wf : 0.0f;
            }
            if (normals) {
                const Sample xp = sample<false>(v, hx + v.vs, hy, hz), xm = sample<false>(v, hx - v.vs, hy, hz);
                const Sample yp = sample<false>(v, hx, hy + v.vs, hz), ym = sample<false>(v, hx, hy - v.vs, hz);
                const Sample zq = sample<false>(v, hx, hy, hz + v.vs), zm = sample<false>(v, hx, hy, hz - v.vs);
                if (xp.known && xm.known && yp.known && ym.known && zq.known && zm.known) {
                    const float gx = xp.f - xm.f, gy = yp.f - ym.f, gz = zq.f - zm.f;
                    normalise(rot_dot(p0, 0, gx, gy, gz), rot_dot(p0, 1, gx, gy, gz), rot_dot(p0, 2, gx, gy, gz), n);
                }
            }
        }
    }
    const int64_t o = (int64_t)b * plane + s;
    disp[o] = d;
    if (weight) weight[o] = wf;
    if (normals) {
        float *np = normals + 3 * (int64_t)b * plane + s;
        np[0] = n[0], np[plane] = n[1], np[2 * plane] = n[2];
    }
}

// ---- points ----
// grid (Gy, Gz), 256 threads: the crossings of each x-row -> row_count[iz * Gy + iy].
__global__ __launch_bounds__(kThreads) void k_ts_count(Vol v, int64_t *__restrict__ row_count)
{
    __shared__ int s_n[kWaves];
    const int iy = blockIdx.x, iz = blockIdx.y, t = threadIdx.x;
    int n = 0;
    for (int ix = t; ix < v.Gx; ix += kThreads) {
        float Ta, Tb[3];
        n += __builtin_popcount(edge_bits(v, ix, iy, iz, Ta, Tb));
    }
    n = block_sum(n, s_n);
    if (t == 0) row_count[(int64_t)iz * v.Gy + iy] = n;
}

// grid (1), 256 threads: row_count[0 .. R) -> its exclusive scan, in place (packkit::row_scan with 64-bit sums); counts[0] = the total.
__global__ __launch_bounds__(kThreads) void k_ts_scan(int64_t *__restrict__ r, int R, int64_t *__restrict__ counts)
{
    __shared__ int64_t s_w[kWaves];
    const int64_t total = row_scan(r, R, s_w);
    if (threadIdx.x == 0) counts[0] = total;
}

// grid (Gy, Gz), 256 threads: the crossings of the x-row in the order (ix, axis) to the records row_off[iz * Gy + iy] ..; a chunk
// is 256 voxels, the rank of (voxel, axis) in it the crossings of the chunk's earlier voxels (packkit::block_rank, one bit slot per
// axis) plus the crossings of the voxel on its earlier axes.
__global__ __launch_bounds__(kThreads) void k_ts_scatter(Vol v, const unsigned *__restrict__ C, const int64_t *__restrict__ row_off,
                                                        int64_t max_points, uint4 *__restrict__ points, float4 *__restrict__ vnormals)
{
    __shared__ int s_w[kWaves];
    const int iy = blockIdx.x, iz = blockIdx.y, t = threadIdx.x;
    const int64_t first = row_off[(int64_t)iz * v.Gy + iy];
    if (first >= max_points) return;                        // (uniform) nothing of this row fits
    const float yw = v.oy + (float)iy * v.vs, zw = v.oz + (float)iz * v.vs;
    int carry = 0;                                          // uniform: the crossings of the earlier chunks
    for (int x0 = 0; x0 < v.Gx; x0 += kThreads) {
        const int ix = x0 + t;
        float Ta = 0.0f, Tb[3] = {0.0f, 0.0f, 0.0f};
        const unsigned bits = ix < v.Gx ? edge_bits(v, ix, iy, iz, Ta, Tb) : 0u;
        int rank = block_rank<3>(bits, s_w, carry);
        if (bits) {
            const float xw = v.ox + (float)ix * v.vs;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                if (!((bits >> e) & 1u)) continue;
                const int64_t rec = first + rank;
                ++rank;
                if (rec >= max_points) continue;
                const float s = Ta / (Ta - Tb[e]);
                const float along = s * v.vs;
                const float X = e == 0 ? xw + along : xw, Y = e == 1 ? yw + along : yw, Z = e == 2 ? zw + along : zw;
                const bool near_a = s <= 0.5f;
                const int jx = ix + (e == 0 && !near_a), jy = iy + (e == 1 && !near_a), jz = iz + (e == 2 && !near_a);
                const unsigned col = C ? C[(jz * v.Gy + jy) * v.Gx + jx] : 0xffffffffu;
                points[rec] = make_uint4(__float_as_uint(X), __float_as_uint(Y), __float_as_uint(Z), col);
                if (vnormals) {
                    float n[3];
                    voxel_normal(v, jx, jy, jz, n);
                    vnormals[rec] = make_float4(n[0], n[1], n[2], 0.0f);
                }
            }
        }
        __syncthreads();                                    // s_w is rewritten by the next chunk
    }
}

// ---- host ----
int check_views(const char *who, const float *cam, const float *pose, int B, int H, int W)
{
    LWS_CHECK_ARG(cam && pose, "%s: cam and pose must not be null", who);
    LWS_CHECK_RC(check_view_shape(who, B, H, W));
    LWS_CHECK_ARG(aligned(cam, 4) && aligned(pose, 4), "%s: cam / pose must be 4-byte aligned", who);
    return LWS_OK;
}

}  // namespace

int tsdfkit::check_volume(const char *who, const float *T, const float *Wt, int Gx, int Gy, int Gz, float ox, float oy, float oz, float vs)
{
    LWS_CHECK_ARG(T && Wt, "%s: T and Wt must not be null", who);
    LWS_CHECK_ARG(Gx >= 2 && Gx <= kMaxGrid && Gy >= 2 && Gy <= kMaxGrid && Gz >= 2 && Gz <= kMaxGrid,
                  "%s: bad volume Gx=%d Gy=%d Gz=%d (each in 2..%d)", who, Gx, Gy, Gz, kMaxGrid);
    LWS_CHECK_ARG((int64_t)Gx * Gy * Gz < ((int64_t)1 << 31), "%s: Gx*Gy*Gz = %dx%dx%d must be < 2^31", who, Gx, Gy, Gz);
    LWS_CHECK_ARG(finite_any(ox) && finite_any(oy) && finite_any(oz), "%s: the origin (%g, %g, %g) must be finite", who, (double)ox, (double)oy,
                  (double)oz);
    LWS_CHECK_ARG(finite_pos(vs), "%s: vs must be finite and > 0, got %g", who, (double)vs);
    LWS_CHECK_ARG(aligned(T, 4) && aligned(Wt, 4), "%s: T / Wt must be 4-byte aligned", who);
    return LWS_OK;
}

int tsdfkit::launch_points(const Vol &v, const uint8_t *C, int64_t max_points, int64_t *rows, void *points, float *vnormals, int64_t *counts,
                           hipStream_t st)
{
    hipLaunchKernelGGL(k_ts_count, dim3(v.Gy, v.Gz), dim3(kThreads), 0, st, v, rows);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ts_scan, dim3(1), dim3(kThreads), 0, st, rows, v.Gy * v.Gz, counts);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ts_scatter, dim3(v.Gy, v.Gz), dim3(kThreads), 0, st, v, reinterpret_cast<const unsigned *>(C), rows, max_points,
                       static_cast<uint4 *>(points), reinterpret_cast<float4 *>(vnormals));
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // namespace lws

using namespace lws;

extern "C" {

int lws_tsdf_integrate(const float *disp, const float *sigma, const uint8_t *mask, const float *normals, const uint8_t *rgb,
                       const float *cam, const float *pose, int B, int H, int W, float *T, float *Wt, uint8_t *C, int Gx, int Gy, int Gz,
                       float ox, float oy, float oz, float vs, float sigma0, float min_disp, float max_depth, float mu0, float mu_d,
                       float sigma_min, int wmode, float w_max, int64_t *updated, void *stream)
{
    const char *who = "tsdf_integrate";
    LWS_CHECK_ARG(disp, "%s: disp is null", who);
    LWS_CHECK_RC(check_views(who, cam, pose, B, H, W));
    LWS_CHECK_RC(check_volume(who, T, Wt, Gx, Gy, Gz, ox, oy, oz, vs));
    LWS_CHECK_ARG((rgb != nullptr) == (C != nullptr), "%s: rgb and C must be given together (rgb colours C; both null: no colour)", who);
    LWS_CHECK_ARG(aligned(disp, 4) && aligned(sigma, 4) && aligned(normals, 4) && aligned(C, 4) && aligned(updated, 8),
                  "%s: disp / sigma / normals / C must be 4-byte, updated 8-byte aligned", who);
    LWS_CHECK_ARG(finite_pos(min_disp), "%s: min_disp must be finite and > 0, got %g", who, (double)min_disp);
    LWS_CHECK_ARG(max_depth > 0.0f, "%s: max_depth must be > 0 (+inf allowed), got %g", who, (double)max_depth);           // (false for NaN)
    LWS_CHECK_ARG(finite_pos(mu0), "%s: mu0 must be finite and > 0, got %g", who, (double)mu0);
    LWS_CHECK_ARG(finite_nonneg(mu_d), "%s: mu_d must be finite and >= 0, got %g", who, (double)mu_d);
    LWS_CHECK_ARG(sigma || finite_nonneg(sigma0), "%s: sigma0 must be finite and >= 0 where sigma is null, got %g", who, (double)sigma0);
    LWS_CHECK_ARG(finite_pos(sigma_min), "%s: sigma_min must be finite and > 0, got %g", who, (double)sigma_min);
    LWS_CHECK_ARG(wmode == 0 || wmode == 1, "%s: wmode %d (0 = unit weights, 1 = 1 / sigma_z^2)", who, wmode);
    LWS_CHECK_ARG(w_max > 0.0f, "%s: w_max must be > 0 (+inf allowed), got %g", who, (double)w_max);                       // (false for NaN)
    const int64_t px = (int64_t)B * H * W, vox = (int64_t)Gx * Gy * Gz;
    const Buf bufs[] = {{T, 4 * vox, "T"}, {Wt, 4 * vox, "Wt"}, {C, 4 * vox, "C"}, {updated, 8 * (int64_t)B, "updated"}, {disp, 4 * px, "disp"},
                        {sigma, 4 * px, "sigma"}, {mask, px, "mask"}, {normals, 12 * px, "normals"}, {rgb, 3 * px, "rgb"},
                        {cam, 20 * (int64_t)B, "cam"}, {pose, 96 * (int64_t)B, "pose"}};
    LWS_CHECK_RC(check_no_overlap(who, bufs, 11, 4));

    const int nq = (Gx + 3) / 4;
    IntArgs a = {disp, sigma, mask, normals, rgb, cam, pose, B, H, W, T, Wt, reinterpret_cast<unsigned *>(C), Gx, Gy, Gz, nq, ox, oy, oz, vs,
                 sigma0, min_disp, max_depth, mu0, mu_d, sigma_min, wmode, w_max, reinterpret_cast<u64 *>(updated)};
    hipStream_t st = (hipStream_t)stream;
    if (updated) {
        hipLaunchKernelGGL(k_ts_zero, dim3(B), dim3(64), 0, st, a.updated);
        LWS_LAUNCH_CHECK();
    }
    const dim3 grid((unsigned)(((int64_t)Gz * Gy * nq + kThreads - 1) / kThreads));
    if (C)
        hipLaunchKernelGGL(k_ts_integrate<true>, grid, dim3(kThreads), 0, st, a);
    else
        hipLaunchKernelGGL(k_ts_integrate<false>, grid, dim3(kThreads), 0, st, a);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

int lws_tsdf_raycast(const float *T, const float *Wt, int Gx, int Gy, int Gz, float ox, float oy, float oz, float vs, const float *cam,
                     const float *pose, int B, int H, int W, float z_near, float step, int nsteps, float w_min, float *disp, float *weight,
                     float *normals, void *stream)
{
    const char *who = "tsdf_raycast";
    LWS_CHECK_RC(check_volume(who, T, Wt, Gx, Gy, Gz, ox, oy, oz, vs));
    LWS_CHECK_RC(check_views(who, cam, pose, B, H, W));
    LWS_CHECK_ARG(disp, "%s: disp is null", who);
    LWS_CHECK_ARG(aligned(disp, 4) && aligned(weight, 4) && aligned(normals, 4), "%s: disp / weight / normals must be 4-byte aligned", who);
    LWS_CHECK_ARG(finite_pos(z_near), "%s: z_near must be finite and > 0, got %g", who, (double)z_near);
    LWS_CHECK_ARG(finite_pos(step), "%s: step must be finite and > 0, got %g", who, (double)step);
    LWS_CHECK_ARG(nsteps >= 2 && nsteps <= 65535, "%s: nsteps %d outside 2..65535", who, nsteps);
    LWS_CHECK_ARG(finite_nonneg(w_min), "%s: w_min must be finite and >= 0, got %g", who, (double)w_min);
    const int64_t px = (int64_t)B * H * W, vox = (int64_t)Gx * Gy * Gz;
    const Buf bufs[] = {{disp, 4 * px, "disp"}, {weight, 4 * px, "weight"}, {normals, 12 * px, "normals"}, {T, 4 * vox, "T"}, {Wt, 4 * vox, "Wt"},
                        {cam, 20 * (int64_t)B, "cam"}, {pose, 96 * (int64_t)B, "pose"}};
    LWS_CHECK_RC(check_no_overlap(who, bufs, 7, 3));

    const Vol v = {T, Wt, Gx, Gy, Gz, ox, oy, oz, vs, w_min};
    hipLaunchKernelGGL(k_ts_raycast, dim3((unsigned)(((int64_t)H * W + kThreads - 1) / kThreads), B), dim3(kThreads), 0, (hipStream_t)stream, v,
                       cam, pose, H, W, z_near, step, nsteps, disp, weight, normals);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

int64_t lws_tsdf_points_workspace(int Gy, int Gz)
{
    LWS_CHECK_ARG(Gy >= 2 && Gy <= kMaxGrid && Gz >= 2 && Gz <= kMaxGrid, "tsdf_points_workspace: bad volume Gy=%d Gz=%d (each in 2..%d)", Gy,
                  Gz, kMaxGrid);
    return ((int64_t)Gy * Gz * (int64_t)sizeof(int64_t) + 255) / 256 * 256;
}

int lws_tsdf_points(const float *T, const float *Wt, const uint8_t *C, int Gx, int Gy, int Gz, float ox, float oy, float oz, float vs,
                    float w_min, int64_t max_points, void *workspace, void *points, float *vnormals, int64_t *counts, void *stream)
{
    const char *who = "tsdf_points";
    LWS_CHECK_RC(check_volume(who, T, Wt, Gx, Gy, Gz, ox, oy, oz, vs));
    LWS_CHECK_ARG(workspace && points && counts, "%s: workspace, points and counts must not be null", who);
    LWS_CHECK_ARG(finite_nonneg(w_min), "%s: w_min must be finite and >= 0, got %g", who, (double)w_min);
    LWS_CHECK_ARG(max_points >= 1 && max_points < ((int64_t)1 << 31), "%s: max_points %lld outside 1 .. 2^31 - 1", who, (long long)max_points);
    LWS_CHECK_ARG(aligned(C, 4) && aligned(workspace, 8) && aligned(points, 16) && aligned(vnormals, 16) && aligned(counts, 8),
                  "%s: C must be 4-byte, workspace / counts 8-byte, points / vnormals 16-byte aligned", who);
    const int64_t vox = (int64_t)Gx * Gy * Gz;
    const Buf bufs[] = {{workspace, lws_tsdf_points_workspace(Gy, Gz), "workspace"}, {points, 16 * max_points, "points"},
                        {vnormals, 16 * max_points, "vnormals"}, {counts, 8, "counts"}, {T, 4 * vox, "T"}, {Wt, 4 * vox, "Wt"}, {C, 4 * vox, "C"}};
    LWS_CHECK_RC(check_no_overlap(who, bufs, 7, 4));

    const Vol v = {T, Wt, Gx, Gy, Gz, ox, oy, oz, vs, w_min};
    return launch_points(v, C, max_points, static_cast<int64_t *>(workspace), points, vnormals, counts, (hipStream_t)stream);
}

}  // extern "C"
