// Moving objects between two consecutive frames: per current pixel the evidence against a rigid scene under the given camera motion
// (geometric: the one-tap projective association of lws_tsdf_integrate and lws_track, widened to a window; photometric: the blend
// of lws_ego_normal), the connected components of the candidate pixels (4-neighbours joined iff |dp - dq| <= max_diff, the rule of
// lws_speckle_filter), and per component of at least min_pixels pixels -- a mover -- its box, its members per evidence code and
// its disparity, numbered in raster order as lws_objects numbers its objects.  Contract: include/lwsnet_movers.h; restated bit for
// bit by tests/movers_reference.py.  One IEEE operation per step (no fma), float32 per pixel, integers for every sum, float64 only
// for the mean disparity.
//
// Launches (a fixed list: it never depends on the data; nothing is read back):
//   k_mv_evidence  one workgroup per 4 rows x 64 columns, a wave's pixels 64 consecutive ones of a row, so that its taps in the
//                  previous frame and the four blend taps fall in the few lines around the row the motion maps it to; the codes and
//                  the workgroup's pixels per code
//   k_mv_tile      one workgroup per 32 x 64 tile: union-find of the tile's candidates in LDS; parent[p] = the raster index of p's
//                  tile-local root (-1: no candidate), and the record of every tile-local root set to "nothing yet"
//   k_mv_border    one thread per pair of pixels across a tile edge: unions of the tile-local roots, agent-scope atomics
//   k_mv_flatten   one thread per pixel: parent[p] = the global root (no union runs here, so the roots stand still)
//   k_mv_pixels    one thread per pixel: every candidate into its root's record; the lanes of a wave that share its first root are
//                  combined first, one lane adds for them
//   k_mv_count     the numbering, as the three-launch scan of lws_point_cloud over the pixels in raster order: the movers' roots
//   k_mv_scan      per block of 2048 pixels, a per-image exclusive scan of the blocks' counts with info and the empty slots, and
//   k_mv_write     the ranked write of rows / vals and of the number into the root's record
//   k_mv_flags     one thread per pixel: is it a member of a mover (a byte), and its label
//   k_mv_grow_x    the flags dilated along the row by `grow`
//   k_mv_apply     ... and along the column: mask_out, and its pixels of code 4 added to info[7]
// A record is 12 words: the head of lws_cclkit.h {n, x_min, x_max, y_min, y_max, the mover's number (-1: none), SQ (two words)}, then
// n2, n3, n4 and an unused word.
// lws_cclkit.h holds the steps this labeller shares with lws_speckle.hip and lws_objects.hip -- the union-find, the tile geometry,
// the tile-edge pairs, the flatten, the wave merge, the record's head, the numbering -- and the invariant, termination, memory-scope
// and determinism arguments they rest on.  The words shared inside a launch here: parent[] in k_mv_border and k_mv_flatten, the
// records in k_mv_pixels, info[7] in k_mv_apply.  0 bytes of scratch.
#include "lwsnet_movers.h"

#include "lws_cclkit.h"
#include "lws_motionkit.h"
#include "lws_packkit.h"
#include "lws_takekit.h"

namespace lws {

namespace {

using namespace geomkit;
using namespace cclkit;
using namespace packkit;                    // kThreads, kWaves, block_scan
using motionkit::blend;
using motionkit::grey_rule;
using takekit::u16f;
constexpr int kEH = 4, kEW = 64;            // the pixels of a workgroup of k_mv_evidence: a wave is one row segment
constexpr int kMaxMovers = 65536;
constexpr int kMaxRadius = 2, kMaxGrow = 8;
constexpr int kRec = 12;                    // words per record
enum { R_N2 = kHeadWords, R_N3, R_N4 };
enum { kUntested = 0, kStatic = 1, kAppeared = 2, kUncovered = 3, kChanged = 4 };
constexpr int kMoverCode = 4;               // mask_out's code of a mover's pixel

struct Gates {
    float min_disp, sigma0, sigma_min, gate_g, gate_p;
    int radius;
};

struct Frame {                              // one image of a frame's maps
    const uint8_t *rgb;
    const float *disp, *sigma;
    const uint8_t *mask;
};

__device__ __forceinline__ bool finite_from(float v, float lo) { return __builtin_isfinite(v) && v >= lo; }

// The evidence code of the current pixel (x, y): include/lwsnet_movers.h, "Evidence", step for step
__device__ __forceinline__ int evidence_code(const Frame &prev, const Frame &cur, const Cam &c, const float *__restrict__ M, int H, int W,
                                             int x, int y, const Gates &g)
{
    const int64_t p = (int64_t)y * W + x;
    const float d = cur.disp[p];
    bool use = (!cur.mask || cur.mask[p] == 1) && finite_from(d, g.min_disp);
    const float z = c.fb / d;
    const float X = back_x(c, x, z), Y = back_y(c, y, z);
    const float Qx = row_dot(M, 0, X, Y, z), Qy = row_dot(M, 1, X, Y, z), Qz = row_dot(M, 2, X, Y, z);
    use = use && Qz > 0.0f;
    float u, v;
    use = project(c, Qx, Qy, Qz, H, W, 0, u, v) && use;
    const float sc = cur.sigma ? cur.sigma[p] : g.sigma0;
    use = use && finite_from(sc, 0.0f);
    if (!use) return kUntested;
    const int iu = (int)rintf(u), iv = (int)rintf(v);
    const float dq = c.fb / Qz;
    const float sc2 = sc * sc;
    bool have = false;
    float rg = 0.0f;
    for (int j = -g.radius; j <= g.radius; ++j) {
        const int ty = iv + j;
        if (ty < 0 || ty >= H) continue;
        for (int i = -g.radius; i <= g.radius; ++i) {
            const int tx = iu + i;
            if (tx < 0 || tx >= W) continue;
            const int64_t t = (int64_t)ty * W + tx;
            if (prev.mask && prev.mask[t] != 1) continue;
            const float dp = prev.disp[t];
            const float sp = prev.sigma ? prev.sigma[t] : g.sigma0;
            if (!finite_from(dp, g.min_disp) || !finite_from(sp, 0.0f)) continue;
            const float s = sqrtf(sc2 + sp * sp);
            const float sg = fmaxf(s, g.sigma_min);
            const float r = (dp - dq) / sg;
            if (__builtin_isnan(r)) continue;
            if (!have || fabsf(r) < fabsf(rg)) rg = r, have = true;
        }
    }
    if (!have) return kUntested;
    if (rg < -g.gate_g) return kAppeared;
    if (rg > g.gate_g) return kUncovered;
    if (W >= 4 && H >= 4 && u >= 1.0f && u <= (float)(W - 2) && v >= 1.0f && v <= (float)(H - 2)) {
        const int i0 = min((int)floorf(u), W - 3), j0 = min((int)floorf(v), H - 3);
        const float fa = u - (float)i0, fbl = v - (float)j0;
        const float Ip = blend([&](int j, int i) { return grey_rule(prev.rgb + 3 * ((int64_t)j * W + i)); }, j0, i0, fa, fbl);
        const float rp = grey_rule(cur.rgb + 3 * p) - Ip;
        if (fabsf(rp) > g.gate_p) return kChanged;
    }
    return kStatic;
}

// grid (nbx * nby, B), 256 threads: wave w of workgroup (bx, by) is the pixels 64 bx .. 64 bx + 63 of row 4 by + w.
// part[b][workgroup][4]: its pixels of code 1, 2, 3, 4.
__global__ __launch_bounds__(kThreads) void k_mv_evidence(const uint8_t *__restrict__ rgb_prev, const float *__restrict__ disp_prev,
                                                         const float *__restrict__ sigma_prev, const uint8_t *__restrict__ mask_prev,
                                                         const uint8_t *__restrict__ rgb_cur, const float *__restrict__ disp_cur,
                                                         const float *__restrict__ sigma_cur, const uint8_t *__restrict__ mask_cur,
                                                         const float *__restrict__ cam, const float *__restrict__ pose, int H, int W, int nbx,
                                                         Gates g, uint8_t *__restrict__ evidence, int *__restrict__ part)
{
    __shared__ int s_n[kWaves][4];
    const int t = threadIdx.x, b = blockIdx.y;
    const int by = blockIdx.x / nbx, bx = blockIdx.x - by * nbx;
    const int x = bx * kEW + (t & 63), y = by * kEH + (t >> 6);
    const int64_t img = (int64_t)b * H * W;
    int code = kUntested;
    if (x < W && y < H) {
        const Frame prev = {rgb_prev + 3 * img, disp_prev + img, sigma_prev ? sigma_prev + img : nullptr, mask_prev ? mask_prev + img : nullptr};
        const Frame cur = {rgb_cur + 3 * img, disp_cur + img, sigma_cur ? sigma_cur + img : nullptr, mask_cur ? mask_cur + img : nullptr};
        code = evidence_code(prev, cur, load_cam(cam, b), inverse_of(pose, b), H, W, x, y, g);
        evidence[img + (int64_t)y * W + x] = (uint8_t)code;
    }
    int n[4] = {code == kStatic, code == kAppeared, code == kUncovered, code == kChanged};
    block_sum_n(n, s_n);
    if (t < 4) part[4 * ((int64_t)b * gridDim.x + blockIdx.x) + t] = block_total(s_n, t);
}

// The record of a root that holds nothing yet
__device__ __forceinline__ void rec_init(int *r)
{
    Head::init(r);
    reinterpret_cast<int4 *>(r)[2] = make_int4(0, 0, 0, 0);
}

// grid (ntx * nty, B), 256 threads: tile (tx, ty) of image b, 8 pixels per thread, a wave a row of the tile.  LDS 16 KiB: s_d (the
// disparity of a candidate, NaN elsewhere and outside the image) and s_par, indexed l as in lws_cclkit.h.
__global__ __launch_bounds__(kThreads) void k_mv_tile(const float *__restrict__ disp, const uint8_t *__restrict__ evidence, int H, int W,
                                                     int ntx, unsigned cand_bits, float max_diff, int *__restrict__ parent,
                                                     int *__restrict__ rec)
{
    __shared__ float s_d[kTile];
    __shared__ int s_par[kTile];
    const int t = threadIdx.x, b = blockIdx.y;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int y0 = ty * kTileRows, x0 = tx * kTileCols;
    const int64_t img = (int64_t)b * H * W;

    for (int l = t; l < kTile; l += kThreads) {
        const int y = y0 + l / kTileCols, x = x0 + (l & (kTileCols - 1));
        float d = __builtin_nanf("");
        if (y < H && x < W) {
            const int64_t p = img + (int64_t)y * W + x;
            if ((cand_bits >> evidence[p]) & 1u) d = disp[p];
        }
        s_d[l] = d;
        s_par[l] = l;
    }
    __syncthreads();
    for (int l = t; l < kTile; l += kThreads)
        join_right_below(s_d, s_par, l, (l & (kTileCols - 1)) + 1 < kTileCols, l / kTileCols + 1 < kTileRows, max_diff);
    __syncthreads();
    for (int l = t; l < kTile; l += kThreads) {
        const int y = y0 + l / kTileCols, x = x0 + (l & (kTileCols - 1));
        if (y >= H || x >= W) continue;
        const int64_t p = img + (int64_t)y * W + x;
        int gp = -1;
        if (!__builtin_isnan(s_d[l])) {
            const int r = lds_find(s_par, l);
            gp = tile_to_index(r, y0, x0, W);
            if (r == l) rec_init(rec + p * kRec);
        }
        parent[p] = gp;
    }
}

// grid (ceil(n / 256), B), n = (nty - 1) * W + (ntx - 1) * H: one thread per pair of pixels across a tile edge (lws_cclkit.h)
__global__ __launch_bounds__(kThreads) void k_mv_border(const float *__restrict__ disp, int H, int W, int nty, int ntx, float max_diff,
                                                       int *__restrict__ parent)
{
    unite_tile_edges(disp, H, W, nty, ntx, max_diff, parent);
}

// grid (ceil(HW / 256), B): one thread per pixel; afterwards parent[p] is the component's first pixel (lws_cclkit.h)
__global__ __launch_bounds__(kThreads) void k_mv_flatten(int HW, int *__restrict__ parent) { flatten_elements(HW, parent); }

// What a set of member pixels adds to a record
struct Acc {
    Head h;
    int n2, n3, n4;

    static __device__ __forceinline__ Acc none() { return Acc{Head::none(), 0, 0, 0}; }
    __device__ __forceinline__ void merge(const Acc &b) { h.merge(b.h), n2 += b.n2, n3 += b.n3, n4 += b.n4; }
    __device__ __forceinline__ Acc lane_xor(int o) const { return Acc{h.lane_xor(o), __shfl_xor(n2, o, 64), __shfl_xor(n3, o, 64), __shfl_xor(n4, o, 64)}; }
    // into the record of root `root` of the image's records: integer atomics only
    __device__ __forceinline__ void add_to(int *rec, int root) const
    {
        int *r = rec + (int64_t)root * kRec;
        h.add_to(r);
        if (n2) a_add(r + R_N2, n2);
        if (n3) a_add(r + R_N3, n3);
        if (n4) a_add(r + R_N4, n4);
    }
};

// grid (ceil(HW / 256), B): one thread per pixel, whole waves (cclkit::wave_add shuffles): every candidate into its root's record.
// A wave inside one mover costs one set of atomics.
__global__ __launch_bounds__(kThreads) void k_mv_pixels(const float *__restrict__ disp, const uint8_t *__restrict__ evidence, int HW, int W,
                                                       const int *__restrict__ parent, int *__restrict__ rec)
{
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t img = (int64_t)blockIdx.y * HW;
    int root = -1;
    Acc a = Acc::none();
    if (g < HW) {
        const int p = (int)g;
        root = parent[img + p];
        if (root >= 0) {
            const int y = p / W, x = p - y * W, code = evidence[img + p];
            a = Acc{Head::pixel(x, y, (u64)(int)u16f(disp[img + p])), code == kAppeared, code == kUncovered, code == kChanged};
        }
    }
    wave_add(a, root, rec + img * kRec);
}

// The numbering (lws_cclkit.h) over the pixels in raster order; a kept root is a mover's.
// grid (nblk, B), 256 threads: cnt[b][blk] = {movers' roots, components} of the block.
__global__ __launch_bounds__(kThreads) void k_mv_count(const int *__restrict__ parent, const int *__restrict__ rec, int HW, int min_pixels,
                                                      int *__restrict__ cnt)
{
    __shared__ int s_n[kWaves][2];
    const int blk = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const Kept k = kept_roots<kRec>(parent + (int64_t)b * HW, rec + (int64_t)b * HW * kRec, ((int64_t)blk * kThreads + t) * kPer, HW, min_pixels);
    int sums[2] = {(int)__popc(k.bits), k.roots};
    block_sum_n(sums, s_n);
    if (t < 2) cnt[2 * ((int64_t)b * gridDim.x + blk) + t] = block_total(s_n, t);
}

// grid (B), 256 threads: cnt[b][blk][0] becomes the movers before the block; the slots of rows / vals past the movers; and info,
// with info[7] = 0 for k_mv_apply to add to.  part: k_mv_evidence's counts, npart workgroups per image.
__global__ __launch_bounds__(kThreads) void k_mv_scan(int *__restrict__ cnt, int nblk, const int *__restrict__ part, int npart, int max_movers,
                                                     int32_t *__restrict__ rows, float *__restrict__ vals, int32_t *__restrict__ info)
{
    __shared__ int s_w[kWaves];
    __shared__ int s_n[kWaves][5];
    const int b = blockIdx.x, t = threadIdx.x;
    int *c = cnt + 2 * (int64_t)b * nblk;
    const int *e = part + 4 * (int64_t)b * npart;
    int sums[5] = {0, 0, 0, 0, 0};                          // components, then the pixels of evidence 1 .. 4
    const int movers = scan_blocks(c, 2, nblk, s_w, [&](int i) { sums[0] += c[2 * i + 1]; });
    for (int i = t; i < npart; i += kThreads)
        for (int j = 0; j < 4; ++j) sums[1 + j] += e[4 * (int64_t)i + j];
    clear_slots<2>(rows + (int64_t)b * max_movers * 8, vals + (int64_t)b * max_movers * 2, movers, max_movers);
    block_sum_n(sums, s_n);
    if (t == 0) {
        int32_t *o = info + 8 * (int64_t)b;
        const int n1 = block_total(s_n, 1), n2 = block_total(s_n, 2), n3 = block_total(s_n, 3), n4 = block_total(s_n, 4);
        o[0] = (n1 + n2) + (n3 + n4), o[1] = n1, o[2] = n2, o[3] = n3, o[4] = n4;
        o[5] = block_total(s_n, 0), o[6] = movers, o[7] = 0;
    }
}

// grid (nblk, B), 256 threads: below max_movers a mover's slot of rows / vals is written and its record gets the number for
// k_mv_flags.  Every other root's record holds -1 since k_mv_tile.
__global__ __launch_bounds__(kThreads) void k_mv_write(const int *__restrict__ parent, int *__restrict__ rec, const float *__restrict__ cam,
                                                      const int *__restrict__ cnt, int HW, int min_pixels, int max_movers,
                                                      int32_t *__restrict__ rows, float *__restrict__ vals)
{
    __shared__ int s_w[kWaves];
    const int blk = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    int *r_img = rec + (int64_t)b * HW * kRec;
    int32_t *orow = rows + (int64_t)b * max_movers * 8;
    float *oval = vals + (int64_t)b * max_movers * 2;
    const float fb = load_cam(cam, b).fb;
    const int64_t cb = ((int64_t)blk * kThreads + t) * kPer;
    const unsigned keep = kept_roots<kRec>(parent + (int64_t)b * HW, r_img, cb, HW, min_pixels).bits;
    for_each_kept(keep, cnt[2 * ((int64_t)b * gridDim.x + blk)], s_w, [&](int i, int j) {
        if (j >= max_movers) return;
        int *r = r_img + (cb + i) * kRec;
        const Head h = Head::load(r);
        const float d = h.mean_disp();
        const int ri[8] = {h.n, h.x0, h.x1, h.y0, h.y1, r[R_N2], r[R_N3], r[R_N4]};
        const float vf[2] = {d, fb / d};
        store_slot(orow, oval, j, ri, vf);
        r[H_NUM] = j;
    });
}

// grid (ceil(HW / 256), B): one thread per pixel: flag[p] = 1 iff p is a member of a mover, capped or not; labels (if given) = the
// mover's number below the cap, -1 for every other pixel.
__global__ __launch_bounds__(kThreads) void k_mv_flags(int HW, const int *__restrict__ parent, const int *__restrict__ rec, int min_pixels,
                                                      uint8_t *__restrict__ flag, int32_t *__restrict__ labels)
{
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= HW) return;
    const int64_t img = (int64_t)blockIdx.y * HW;
    const int root = parent[img + g];
    const int *r = rec + (img + (root < 0 ? 0 : root)) * kRec;
    const bool mover = root >= 0 && r[H_N] >= min_pixels;
    flag[img + g] = mover ? 1 : 0;
    if (labels) labels[img + g] = mover ? r[H_NUM] : -1;
}

// grid (ceil(HW / 256), B): out[y, x] = 1 iff in[y, x - grow .. x + grow] holds a 1 inside the row
__global__ __launch_bounds__(kThreads) void k_mv_grow_x(int HW, int W, int grow, const uint8_t *__restrict__ in, uint8_t *__restrict__ out)
{
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= HW) return;
    const int64_t img = (int64_t)blockIdx.y * HW;
    const int p = (int)g, x = p % W;
    const int lo = max(x - grow, 0), hi = min(x + grow, W - 1);
    int any = 0;
    for (int i = lo; i <= hi; ++i) any |= in[img + p - x + i];
    out[img + p] = (uint8_t)any;
}

// grid (ceil(HW / 256), B), 256 threads: a pixel with a 1 of `in` within `grow` rows in its column is a mover's (code 4); every other
// pixel keeps mask's code, or without a mask gets 1 iff its disparity is finite and > 0.  mask_out may be mask (no __restrict__ on
// them): a thread reads its own pixel before it writes it.  The workgroup's pixels of code 4 are added to info[7] (k_mv_scan
// zeroed it): an integer atomic.
__global__ __launch_bounds__(kThreads) void k_mv_apply(int HW, int W, int grow, const uint8_t *__restrict__ in, const float *__restrict__ disp,
                                                      const uint8_t *mask, uint8_t *mask_out, int32_t *__restrict__ info)
{
    __shared__ int s_n[kWaves];
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t img = (int64_t)blockIdx.y * HW;
    int any = 0;
    if (g < HW) {
        const int p = (int)g, y = p / W, H = HW / W;
        const int lo = max(y - grow, 0), hi = min(y + grow, H - 1);
        for (int j = lo; j <= hi; ++j) any |= in[img + p + (int64_t)(j - y) * W];
        const float d = disp[img + p];
        const int keep = mask ? mask[img + p] : (__builtin_isfinite(d) && d > 0.0f ? 1 : 0);
        mask_out[img + p] = (uint8_t)(any ? kMoverCode : keep);
    }
    const int n = block_sum(any, s_n);
    if (threadIdx.x == 0 && n > 0) a_add(info + 8 * (int64_t)blockIdx.y + 7, n);
}

struct Layout {                             // the parts of the workspace, in bytes from its start
    int64_t parent, rec, flag, flag_x, part, cnt, end;
    int nbx, nby, nblk;
};

Layout layout_of(int B, int H, int W)
{
    Layout l;
    const int64_t px = (int64_t)B * H * W;
    l.nbx = (W + kEW - 1) / kEW, l.nby = (H + kEH - 1) / kEH;
    l.nblk = (int)(((int64_t)H * W + kBlock - 1) / kBlock);
    l.parent = 0;
    l.rec = l.parent + round256(px * (int64_t)sizeof(int));
    l.flag = l.rec + round256(px * kRec * (int64_t)sizeof(int));
    l.flag_x = l.flag + round256(px);
    l.part = l.flag_x + round256(px);
    l.cnt = l.part + round256(4 * (int64_t)B * l.nbx * l.nby * (int64_t)sizeof(int));
    l.end = l.cnt + round256(2 * (int64_t)B * l.nblk * (int64_t)sizeof(int));
    return l;
}

int check_size(const char *who, int B, int H, int W, int max_movers)
{
    LWS_CHECK_RC(check_view_shape(who, B, H, W));
    LWS_CHECK_ARG(max_movers >= 1 && max_movers <= kMaxMovers, "%s: max_movers %d outside 1..%d", who, max_movers, kMaxMovers);
    return LWS_OK;
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int64_t lws_movers_workspace(int B, int H, int W, int max_movers)
{
    LWS_CHECK_RC(check_size("movers_workspace", B, H, W, max_movers));
    return layout_of(B, H, W).end;
}

int lws_movers(const uint8_t *rgb_prev, const float *disp_prev, const float *sigma_prev, const uint8_t *mask_prev, const uint8_t *rgb_cur,
               const float *disp_cur, const float *sigma_cur, const uint8_t *mask_cur, const float *cam, const float *pose, int B, int H,
               int W, float min_disp, float sigma0, float sigma_min, float gate_g, float gate_p, int radius, int cand_bits, float max_diff,
               int min_pixels, int grow, int max_movers, void *workspace, uint8_t *evidence, uint8_t *mask_out, int32_t *labels,
               int32_t *rows, float *vals, int32_t *info, void *stream)
{
    LWS_CHECK_RC(check_size("movers", B, H, W, max_movers));
    LWS_CHECK_ARG(rgb_prev && disp_prev && rgb_cur && disp_cur && cam && pose, "movers: rgb_prev, disp_prev, rgb_cur, disp_cur, cam and pose must not be null");
    LWS_CHECK_ARG(workspace && evidence && mask_out && rows && vals && info, "movers: workspace, evidence, mask_out, rows, vals and info must not be null");
    LWS_CHECK_ARG(aligned(disp_prev, 4) && aligned(sigma_prev, 4) && aligned(disp_cur, 4) && aligned(sigma_cur, 4) && aligned(cam, 4) &&
                      aligned(pose, 4) && aligned(labels, 4) && aligned(rows, 4) && aligned(vals, 4) && aligned(info, 4) && aligned(workspace, 16),
                  "movers: disp / sigma / cam / pose / labels / rows / vals / info must be 4-byte, workspace 16-byte aligned");
    LWS_CHECK_ARG(finite_pos(min_disp), "movers: min_disp must be finite and > 0, got %g", (double)min_disp);
    LWS_CHECK_ARG(finite_nonneg(sigma0), "movers: sigma0 must be finite and >= 0, got %g", (double)sigma0);
    LWS_CHECK_ARG(finite_pos(sigma_min), "movers: sigma_min must be finite and > 0, got %g", (double)sigma_min);
    LWS_CHECK_ARG(finite_pos(gate_g), "movers: gate_g must be finite and > 0, got %g", (double)gate_g);
    LWS_CHECK_ARG(gate_p > 0.0f, "movers: gate_p must be > 0 (+inf: no photometric test), got %g", (double)gate_p);       // (false for NaN)
    LWS_CHECK_ARG(radius >= 0 && radius <= kMaxRadius, "movers: radius %d outside 0..%d", radius, kMaxRadius);
    LWS_CHECK_ARG(cand_bits >= 0 && cand_bits < 32 && !(cand_bits & 3), "movers: cand_bits %d outside 0..31 or with bit 0 or 1 set (untested and static pixels are no candidates)", cand_bits);
    LWS_CHECK_ARG(max_diff >= 0.0f, "movers: max_diff must be >= 0 (+inf allowed), got %g", (double)max_diff);
    LWS_CHECK_ARG(min_pixels >= 1, "movers: min_pixels %d < 1", min_pixels);
    LWS_CHECK_ARG(grow >= 0 && grow <= kMaxGrow, "movers: grow %d outside 0..%d", grow, kMaxGrow);
    const int64_t px = (int64_t)B * H * W;
    const Layout l = layout_of(B, H, W);
    // mask_out may be mask_cur itself (a thread reads its pixel before it writes it, and the evidence is taken before); any other
    // overlap between an input, an output and the workspace is an error: every pair is checked
    const Buf bufs[] = {{workspace, l.end, "workspace"}, {evidence, px, "evidence"}, {mask_out, px, "mask_out"}, {labels, 4 * px, "labels"},
                        {rows, 32 * (int64_t)B * max_movers, "rows"}, {vals, 8 * (int64_t)B * max_movers, "vals"}, {info, 32 * (int64_t)B, "info"},
                        {mask_cur, px, "mask_cur"}, {rgb_prev, 3 * px, "rgb_prev"}, {disp_prev, 4 * px, "disp_prev"},
                        {sigma_prev, 4 * px, "sigma_prev"}, {mask_prev, px, "mask_prev"}, {rgb_cur, 3 * px, "rgb_cur"},
                        {disp_cur, 4 * px, "disp_cur"}, {sigma_cur, 4 * px, "sigma_cur"}, {cam, 20 * (int64_t)B, "cam"},
                        {pose, 96 * (int64_t)B, "pose"}};
    const int in_place[][2] = {{2, 7}};                     // mask_out / mask_cur
    LWS_CHECK_RC(check_no_overlap("movers", bufs, 17, 7, in_place, 1));

    char *ws = static_cast<char *>(workspace);
    int *parent = reinterpret_cast<int *>(ws + l.parent), *rec = reinterpret_cast<int *>(ws + l.rec);
    uint8_t *flag = reinterpret_cast<uint8_t *>(ws + l.flag), *flag_x = reinterpret_cast<uint8_t *>(ws + l.flag_x);
    int *part = reinterpret_cast<int *>(ws + l.part), *cnt = reinterpret_cast<int *>(ws + l.cnt);
    const int HW = H * W, npart = l.nbx * l.nby;
    const int ntx = (W + kTileCols - 1) / kTileCols, nty = (H + kTileRows - 1) / kTileRows;
    const int64_t pairs = (int64_t)(nty - 1) * W + (int64_t)(ntx - 1) * H;
    const unsigned per_pixel = (unsigned)(((int64_t)HW + kThreads - 1) / kThreads);
    const Gates g = {min_disp, sigma0, sigma_min, gate_g, gate_p, radius};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mv_evidence, dim3((unsigned)npart, B), dim3(kThreads), 0, st, rgb_prev, disp_prev, sigma_prev, mask_prev, rgb_cur, disp_cur,
                       sigma_cur, mask_cur, cam, pose, H, W, l.nbx, g, evidence, part);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mv_tile, dim3((unsigned)(ntx * nty), B), dim3(kThreads), 0, st, disp_cur, evidence, H, W, ntx, (unsigned)cand_bits, max_diff,
                       parent, rec);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mv_border, dim3((unsigned)(pairs > 0 ? (pairs + kThreads - 1) / kThreads : 1), B), dim3(kThreads), 0, st, disp_cur, H, W,
                       nty, ntx, max_diff, parent);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mv_flatten, dim3(per_pixel, B), dim3(kThreads), 0, st, HW, parent);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mv_pixels, dim3(per_pixel, B), dim3(kThreads), 0, st, disp_cur, evidence, HW, W, parent, rec);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mv_count, dim3(l.nblk, B), dim3(kThreads), 0, st, parent, rec, HW, min_pixels, cnt);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mv_scan, dim3(B), dim3(kThreads), 0, st, cnt, l.nblk, part, npart, max_movers, rows, vals, info);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mv_write, dim3(l.nblk, B), dim3(kThreads), 0, st, parent, rec, cam, cnt, HW, min_pixels, max_movers, rows, vals);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mv_flags, dim3(per_pixel, B), dim3(kThreads), 0, st, HW, parent, rec, min_pixels, flag, labels);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mv_grow_x, dim3(per_pixel, B), dim3(kThreads), 0, st, HW, W, grow, flag, flag_x);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mv_apply, dim3(per_pixel, B), dim3(kThreads), 0, st, HW, W, grow, flag_x, disp_cur, mask_cur, mask_out, info);
    LWS_LAUNCH_CHECK();
    return LWS_OK;
}

}  // extern "C"
