// Obstacle objects: the connected components (8-neighbours) of the occupied cells of the u-disparity image, each pixel mapped back
// to its cell's component, and per component the pixel box, the bins, the mean disparity and the box in camera coordinates.
// Contract: include/lwsnet_objects.h, lws_objects; restated bit for bit by tests/object_reference.py.  One IEEE operation per step (no
// fma), float32 per pixel, integers for every sum, float64 only for the mean disparity.
//
// The cells of an image are indexed c = (nbins - 1 - k) * S + s: row kr = nbins - 1 - k (nearest first), column s.  c is the
// union-find index, so that "parent <= self" (lws_cclkit.h) makes a component's root its smallest c: the numbering key.
// Launches (a fixed list: it depends on the argument `labels`, never on the data; nothing is read back):
//   k_ob_tile     one workgroup per tile of 32 rows x 64 columns of cells: union-find of the tile's occupied cells in LDS with the
//                 four forward joins of the 8-neighbourhood; parent[c] = the index of c's tile-local root (-1: not occupied), and
//                 the record of every occupied cell set to "nothing yet"
//   k_ob_border   one thread per cell on a tile's first row or first column: unions with its neighbours across the edge
//   k_ob_flatten  one thread per cell: parent[c] = the global root (no union runs here, so the roots stand still)
//   k_ob_pixels   one workgroup per strip and image (the loop of k_stixels): every member pixel into its cell's record; the lanes
//                 of a wave that hit the same cell are combined first, one lane adds for them
//   k_ob_cells    one thread per cell: the record of an occupied cell that is not a root into its root's record
//   k_ob_count    the numbering, as the three-launch scan of lws_point_cloud over the cells in c order: the kept roots per block
//   k_ob_scan     of 2048 cells, a per-image exclusive scan of the blocks' counts with info and the empty slots, and the ranked
//   k_ob_write    write of rows / vals and of the number into the root's record
//   k_ob_labels   (labels != NULL) one workgroup per strip and image: the object's number per pixel
// A record is 16 words: the head of lws_cclkit.h {n, x_min, x_max, y_min, y_max, the object's number (-1: none), SQ (two words)}, the
// ordered keys of X_min, X_max, Y_min, Y_max, Z_min, Z_max, the largest row kr, the other cells.
// lws_cclkit.h holds the steps this labeller shares with lws_speckle.hip and lws_movers.hip -- the union-find, the tile geometry, the
// flatten, the wave merge, the record's head, the numbering -- and the invariant, termination, memory-scope and determinism arguments
// they rest on (the floats cross lanes and workgroups as ordered keys: integers too).  The words shared inside a launch here:
// parent[] in k_ob_border and k_ob_flatten, the records in k_ob_pixels and k_ob_cells.  0 bytes of scratch.
#include "lwsnet_objects.h"

#include "lws_cclkit.h"
#include "lws_geomkit.h"
#include "lws_packkit.h"
#include "lws_takekit.h"

namespace lws {

namespace {

using namespace geomkit;
using namespace takekit;                    // the limits, Item / load_item, Rule / bin_of, u16f
using namespace cclkit;
using namespace packkit;                    // kThreads, kWaves, block_scan
constexpr int kTK = 32, kTS = 64;           // the tile of k_ob_tile: rows (bins) x columns (strips); tests/test_objects_cpu.py reads this line
static_assert(kTK == kTileRows && kTS == kTileCols, "the cell tile is the labellers' tile (lws_cclkit.h)");
constexpr int kMaxCells = 1 << 22;          // S * nbins: the workspace stays below 286 MB per image
constexpr int kMaxObjects = 65536;
constexpr int kRec = 16;                    // words per record
enum { R_KEY = kHeadWords, R_KR = 14, R_CELLS = 15 };

// What a set of member pixels adds to a record.  key[]: X_min, X_max, Y_min, Y_max, Z_min, Z_max as opkit::key_of words (no NaN comes here)
struct Acc {
    Head h;
    u32 key[6];

    static __device__ __forceinline__ Acc none() { return Acc{Head::none(), {~0u, 0u, ~0u, 0u, ~0u, 0u}}; }
    __device__ __forceinline__ void merge(const Acc &b)
    {
        h.merge(b.h);
#pragma unroll
        for (int i = 0; i < 6; i += 2) key[i] = min(key[i], b.key[i]), key[i + 1] = max(key[i + 1], b.key[i + 1]);
    }
    __device__ __forceinline__ Acc lane_xor(int o) const
    {
        Acc v = {h.lane_xor(o), {}};
#pragma unroll
        for (int i = 0; i < 6; ++i) v.key[i] = __shfl_xor(key[i], o, 64);
        return v;
    }
    // into the record of cell `cell` of the image's records: integer atomics only
    __device__ __forceinline__ void add_to(u32 *rec, int cell) const
    {
        u32 *r = rec + (int64_t)cell * kRec;
        h.add_to(reinterpret_cast<int *>(r));
#pragma unroll
        for (int i = 0; i < 6; i += 2) a_min(r + R_KEY + i, key[i]), a_max(r + R_KEY + i + 1, key[i + 1]);
    }
};

// The record of a cell in row kr that holds nothing yet
__device__ __forceinline__ void rec_init(u32 *r, int kr)
{
    Head::init(reinterpret_cast<int *>(r));
    int4 *q = reinterpret_cast<int4 *>(r);
    q[2] = make_int4(-1, 0, -1, 0);
    q[3] = make_int4(-1, 0, kr, 0);
}

// grid (ntk * nts, B), 256 threads: the tile (tk, ts) of image b, 8 cells per thread.  LDS 16 KiB: s_occ, s_par, indexed
// l as in lws_cclkit.h, which grows with c.  udisp is read with the bins along the threads.
__global__ __launch_bounds__(kThreads) void k_ob_tile(const uint32_t *__restrict__ udisp, int S, int nbins, int nts, unsigned min_count,
                                                     int *__restrict__ parent, u32 *__restrict__ rec)
{
    __shared__ int s_occ[kTile];
    __shared__ int s_par[kTile];
    const int t = threadIdx.x, b = blockIdx.y;
    const int tk = blockIdx.x / nts, ts = blockIdx.x - tk * nts;
    const int kr0 = tk * kTK, s0 = ts * kTS;
    const int64_t cells = (int64_t)b * S * nbins;
    const uint32_t *u = udisp + cells;

    for (int i = t; i < kTile; i += kThreads) {
        const int lk = i & (kTK - 1), ls = i / kTK;
        const int kr = kr0 + lk, s = s0 + ls, l = lk * kTS + ls;
        s_occ[l] = kr < nbins && s < S && u[(int64_t)s * nbins + (nbins - 1 - kr)] >= min_count;
        s_par[l] = l;
    }
    __syncthreads();
    // the four forward joins of the 8-neighbourhood: right, down-left, down, down-right
    for (int l = t; l < kTile; l += kThreads) {
        if (!s_occ[l]) continue;
        const int lk = l / kTS, ls = l & (kTS - 1);
        if (ls + 1 < kTS && s_occ[l + 1]) lds_unite(s_par, l, l + 1);
        if (lk + 1 < kTK) {
            if (ls > 0 && s_occ[l + kTS - 1]) lds_unite(s_par, l, l + kTS - 1);
            if (s_occ[l + kTS]) lds_unite(s_par, l, l + kTS);
            if (ls + 1 < kTS && s_occ[l + kTS + 1]) lds_unite(s_par, l, l + kTS + 1);
        }
    }
    __syncthreads();
    for (int l = t; l < kTile; l += kThreads) {
        const int lk = l / kTS, ls = l & (kTS - 1), kr = kr0 + lk, s = s0 + ls;
        if (kr >= nbins || s >= S) continue;
        const int c = kr * S + s;
        int p = -1;
        if (s_occ[l]) {
            p = tile_to_index(lds_find(s_par, l), kr0, s0, S);
            rec_init(rec + (cells + c) * kRec, kr);
        }
        parent[cells + c] = p;
    }
}

// grid (ceil(n / 256), B), n = (ntk - 1) * S + (nts - 1) * nbins: thread g < (ntk - 1) * S is the cell (kr, s) on the first row of
// a tile row, joined with (kr - 1, s - 1 .. s + 1); the others the cell (kr, s) on the first column of a tile column, joined with
// (kr - 1 .. kr + 1, s - 1).  Together: every pair of neighbours in different tiles (some twice, which a union does not mind).
// parent[] is shared between workgroups here (g_find, g_unite); the sign of a parent word never changes (lws_cclkit.h).
__global__ __launch_bounds__(kThreads) void k_ob_border(int S, int nbins, int ntk, int nts, int *__restrict__ parent)
{
    const int g = blockIdx.x * kThreads + threadIdx.x;
    const int nh = (ntk - 1) * S, nv = (nts - 1) * nbins;
    if (g >= nh + nv) return;
    int *par = parent + (int64_t)blockIdx.y * S * nbins;
    int kr, s, dk, ds;                                      // the three neighbours: (kr - 1 + dk * j, s - 1 + ds * j), j = 0, 1, 2
    if (g < nh) {
        const int e = g / S;
        s = g - e * S, kr = (e + 1) * kTK, dk = 0, ds = 1;  // (kr - 1, s - 1 + j)
    } else {
        const int v = g - nh, e = v / nbins;
        kr = v - e * nbins, s = (e + 1) * kTS, dk = 1, ds = 0;      // (kr - 1 + j, s - 1)
    }
    const int q = kr * S + s;
    if (ld_agent(par + q) < 0) return;
    for (int j = 0; j < 3; ++j) {
        const int nk = kr - 1 + dk * j, ns = s - 1 + ds * j;
        if (nk < 0 || nk >= nbins || ns < 0 || ns >= S) continue;
        const int p = nk * S + ns;
        if (ld_agent(par + p) >= 0) g_unite(par, p, q);
    }
}

// grid (ceil(N / 256), B): one thread per cell; afterwards parent[c] is the component's smallest c (lws_cclkit.h)
__global__ __launch_bounds__(kThreads) void k_ob_flatten(int N, int *__restrict__ parent) { flatten_elements(N, parent); }

// The occupied bins of strip s as a bit mask in LDS (s_occ: kMaxBins / 32 words); a barrier before it is read
__device__ __forceinline__ void stage_occupied(const uint32_t *__restrict__ u, int nbins, unsigned min_count, u32 *s_occ)
{
    for (int w = threadIdx.x; w < (nbins + 31) / 32; w += kThreads) {
        u32 bits = 0u;
        for (int i = 0; i < 32 && 32 * w + i < nbins; ++i) bits |= (u32)(u[32 * w + i] >= min_count) << i;
        s_occ[w] = bits;
    }
}

// grid (S, B), 256 threads: the strip blockIdx.x of image blockIdx.y, read as k_stixels reads it.  A member pixel -- it takes part
// and its cell (s, q) is occupied -- goes into its cell's record: the runs of equal bins of an item first, then the lanes of the
// wave with the same cell (cclkit::wave_add).  A cell belongs to one strip, hence to this workgroup alone.
__global__ __launch_bounds__(kThreads) void k_ob_pixels(const float *__restrict__ disp, const float *__restrict__ cam,
                                                       const uint8_t *__restrict__ codes, const uint32_t *__restrict__ udisp, int H, int W,
                                                       float min_disp, float max_depth, unsigned code_bits, int width, int sub, int nbins,
                                                       unsigned min_count, u32 *__restrict__ rec)
{
    __shared__ u32 s_occ[kMaxBins / 32];
    const int s = blockIdx.x, b = blockIdx.y, S = gridDim.x, t = threadIdx.x;
    const int x0 = s * width, x1 = min(x0 + width, W) - 1, ws = x1 - x0 + 1;
    const int nc = (ws + 3) >> 2, items = H * nc;
    const int64_t base = (int64_t)b * H * W + x0;
    const Cam c = load_cam(cam, b);
    const Rule rule = {c.fb, min_disp, max_depth, (float)sub, (float)nbins, code_bits};
    u32 *r_img = rec + (int64_t)b * S * nbins * kRec;

    stage_occupied(udisp + ((int64_t)b * S + s) * nbins, nbins, min_count, s_occ);
    __syncthreads();
    for (int i0 = 0; i0 < items; i0 += kThreads) {          // (whole waves go round: wave_add shuffles)
        const int i = i0 + t;
        Acc a[4] = {Acc::none(), Acc::none(), Acc::none(), Acc::none()};
        int cell[4] = {-1, -1, -1, -1};
        if (i < items) {
            const int y = i / nc, xs = 4 * (i - y * nc);
            const int64_t at = base + (int64_t)y * W;
            const Item it = load_item(disp + at, codes + at, xs, ws);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = bin_of(it.d[j], it.code[j], rule);
                if (q < 0 || !((s_occ[q >> 5] >> (q & 31)) & 1u)) continue;
                const int x = x0 + xs + j;
                const float z = c.fb / it.d[j];
                const float X = back_x(c, x, z), Y = back_y(c, y, z);
                const u32 kx = key_of(X), ky = key_of(Y), kz = key_of(z);
                a[j] = Acc{Head::pixel(x, y, (u64)(int)u16f(it.d[j])), {kx, kx, ky, ky, kz, kz}};
                cell[j] = (nbins - 1 - q) * S + s;
            }
            // a fronto-parallel obstacle puts its pixels into few bins: the runs of equal cells of an item go on as one
#pragma unroll
            for (int j = 1; j < 4; ++j)
                if (cell[j] >= 0 && cell[j] == cell[j - 1]) a[j].merge(a[j - 1]), cell[j - 1] = -1;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) wave_add(a[j], cell[j], r_img);
    }
}

// grid (ceil(N / 256), B): one thread per cell; an occupied cell that is not its component's root hands its record, itself as a
// cell and its row to the root's.  Only roots' records are written here (atomics), only the others' are read (plain loads).
__global__ __launch_bounds__(kThreads) void k_ob_cells(int N, const int *__restrict__ parent, u32 *__restrict__ rec)
{
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= N) return;
    const int64_t cells = (int64_t)blockIdx.y * N;
    const int p = parent[cells + c];
    if (p < 0 || p == c) return;
    const u32 *m = rec + (cells + c) * kRec;
    u32 *r = rec + (cells + p) * kRec;
    Acc a = {Head::load(reinterpret_cast<const int *>(m)), {}};
#pragma unroll
    for (int i = 0; i < 6; ++i) a.key[i] = m[R_KEY + i];
    a.add_to(rec + cells * kRec, p);
    a_add(r + R_CELLS, 1u);
    a_max(reinterpret_cast<int *>(r) + R_KR, (int)m[R_KR]);
}

// The numbering (lws_cclkit.h) over the cells in c order.
// grid (nblk, B), 256 threads: cnt[b][blk] = {kept roots, occupied cells, components, member pixels of the kept roots} of the block.
__global__ __launch_bounds__(kThreads) void k_ob_count(const int *__restrict__ parent, const u32 *__restrict__ rec, int N, int min_pixels,
                                                      int *__restrict__ cnt)
{
    __shared__ int s_n[kWaves][4];
    const int blk = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const Kept k = kept_roots<kRec>(parent + (int64_t)b * N, rec + (int64_t)b * N * kRec, (blk * kThreads + t) * kPer, N, min_pixels);
    int sums[4] = {(int)__popc(k.bits), k.in_sets, k.roots, k.members};
    block_sum_n(sums, s_n);
    if (t < 4) cnt[4 * ((int64_t)b * gridDim.x + blk) + t] = block_total(s_n, t);
}

// grid (B), 256 threads: cnt[b][blk][0] becomes the kept roots before the block; info; and the slots of rows / vals past the kept
// components.
__global__ __launch_bounds__(kThreads) void k_ob_scan(int *__restrict__ cnt, int nblk, int max_objects, int32_t *__restrict__ rows,
                                                     float *__restrict__ vals, int32_t *__restrict__ info)
{
    __shared__ int s_w[kWaves];
    __shared__ int s_n[kWaves][3];
    const int b = blockIdx.x;
    int *c = cnt + 4 * (int64_t)b * nblk;
    int sums[3] = {0, 0, 0};
    const int kept = scan_blocks(c, 4, nblk, s_w, [&](int i) {
        for (int j = 0; j < 3; ++j) sums[j] += c[4 * i + 1 + j];
    });
    clear_slots<8>(rows + (int64_t)b * max_objects * 8, vals + (int64_t)b * max_objects * 8, kept, max_objects);
    block_sum_n(sums, s_n);
    if (threadIdx.x == 0) {
        int32_t *o = info + 4 * (int64_t)b;
        o[0] = block_total(s_n, 0), o[1] = block_total(s_n, 1), o[2] = kept, o[3] = block_total(s_n, 2);
    }
}

// grid (nblk, B), 256 threads: below max_objects a kept root's slot of rows / vals is written, and its record gets the number
// for k_ob_labels.  Every other root's record holds -1 since k_ob_tile.
__global__ __launch_bounds__(kThreads) void k_ob_write(const int *__restrict__ parent, u32 *__restrict__ rec, const float *__restrict__ cam,
                                                      const int *__restrict__ cnt, int S, int nbins, int min_pixels, int max_objects,
                                                      int32_t *__restrict__ rows, float *__restrict__ vals)
{
    __shared__ int s_w[kWaves];
    const int blk = blockIdx.x, b = blockIdx.y, t = threadIdx.x, N = S * nbins;
    u32 *r_img = rec + (int64_t)b * N * kRec;
    int32_t *orow = rows + (int64_t)b * max_objects * 8;
    float *oval = vals + (int64_t)b * max_objects * 8;
    const float fb = load_cam(cam, b).fb;
    const int cb = (blk * kThreads + t) * kPer;
    const unsigned keep = kept_roots<kRec>(parent + (int64_t)b * N, r_img, cb, N, min_pixels).bits;
    for_each_kept(keep, cnt[4 * ((int64_t)b * gridDim.x + blk)], s_w, [&](int i, int j) {
        if (j >= max_objects) return;
        u32 *r = r_img + (int64_t)(cb + i) * kRec;
        const Head h = Head::load(reinterpret_cast<const int *>(r));
        const int k_max = nbins - 1 - (cb + i) / S, k_min = nbins - 1 - (int)r[R_KR];
        const float d = h.mean_disp();
        const int ri[8] = {h.n, h.x0, h.x1, h.y0, h.y1, k_min, k_max, (int)r[R_CELLS] + 1};
        const float vf[8] = {d, fb / d, unkey(r[R_KEY]), unkey(r[R_KEY + 1]), unkey(r[R_KEY + 2]), unkey(r[R_KEY + 3]),
                             unkey(r[R_KEY + 4]), unkey(r[R_KEY + 5])};
        store_slot(orow, oval, j, ri, vf);
        r[H_NUM] = (u32)j;
    });
}

// grid (S, B), 256 threads: the strip blockIdx.x of image blockIdx.y.  The number of each bin's component in LDS (16 KB), then the
// strip's pixels: the number of a member of a kept component below max_objects, -1 for every other pixel.
__global__ __launch_bounds__(kThreads) void k_ob_labels(const float *__restrict__ disp, const float *__restrict__ cam,
                                                       const uint8_t *__restrict__ codes, int H, int W, float min_disp, float max_depth,
                                                       unsigned code_bits, int width, int sub, int nbins, const int *__restrict__ parent,
                                                       const u32 *__restrict__ rec, int32_t *__restrict__ labels)
{
    __shared__ int s_lab[kMaxBins];
    const int s = blockIdx.x, b = blockIdx.y, S = gridDim.x, t = threadIdx.x;
    const int x0 = s * width, x1 = min(x0 + width, W) - 1, ws = x1 - x0 + 1;
    const int nc = (ws + 3) >> 2, items = H * nc;
    const int64_t base = (int64_t)b * H * W + x0, cells = (int64_t)b * S * nbins;
    const Rule rule = {load_cam(cam, b).fb, min_disp, max_depth, (float)sub, (float)nbins, code_bits};

    for (int k = t; k < nbins; k += kThreads) {
        const int p = parent[cells + (int64_t)(nbins - 1 - k) * S + s];
        s_lab[k] = p < 0 ? -1 : (int)rec[(cells + p) * kRec + H_NUM];
    }
    __syncthreads();
    for (int i = t; i < items; i += kThreads) {
        const int y = i / nc, xs = 4 * (i - y * nc);
        const int64_t at = base + (int64_t)y * W;
        const Item it = load_item(disp + at, codes + at, xs, ws);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (xs + j >= ws) continue;
            const int q = bin_of(it.d[j], it.code[j], rule);
            labels[at + xs + j] = q < 0 ? -1 : s_lab[q];
        }
    }
}

// The checks lws_objects_workspace and lws_objects share; S: the strips
int check_grid(const char *who, int B, int W, int width, int nbins, int &S)
{
    LWS_CHECK_ARG(B >= 1 && B <= 65535 && W >= 1 && W <= kMaxDim, "%s: bad shape B=%d W=%d (W <= %d)", who, B, W, kMaxDim);
    LWS_CHECK_ARG(width >= 1 && width <= kMaxWidth, "%s: width %d outside 1..%d", who, width, kMaxWidth);
    LWS_CHECK_ARG(nbins >= 1 && nbins <= kMaxBins, "%s: nbins %d outside 1..%d", who, nbins, kMaxBins);
    S = (W + width - 1) / width;
    LWS_CHECK_ARG((int64_t)S * nbins <= kMaxCells, "%s: S * nbins = %d * %d exceeds %d cells (the workspace would pass 286 MB per image)", who, S,
                  nbins, kMaxCells);
    return LWS_OK;
}

}  // namespace

}  // namespace lws

using namespace lws;

extern "C" {

int64_t lws_objects_workspace(int B, int W, int width, int nbins)
{
    int S;
    LWS_CHECK_RC(check_grid("objects_workspace", B, W, width, nbins, S));
    const int64_t cells = (int64_t)B * S * nbins;
    const int64_t nblk = ((int64_t)S * nbins + kBlock - 1) / kBlock;
    return round256(cells * (int64_t)sizeof(int)) + round256(cells * kRec * (int64_t)sizeof(u32)) + round256(4 * B * nblk * (int64_t)sizeof(int));
}

int lws_objects(const float *disp, const float *cam, const uint8_t *codes, const uint32_t *udisp, int B, int H, int W, float min_disp,
                float max_depth, int code_bits, int width, int sub, int nbins, int min_count, int min_pixels, int max_objects,
                void *workspace, int32_t *rows, float *vals, int32_t *labels, int32_t *info, void *stream)
{
    LWS_CHECK_RC(check_geometry_args("objects", disp, B, H, W, min_disp, max_depth));
    LWS_CHECK_ARG(H <= kMaxDim && W <= kMaxDim, "objects: H=%d W=%d exceed %d (the 64-bit sums)", H, W, kMaxDim);
    LWS_CHECK_ARG(cam && codes && udisp, "objects: cam, codes and udisp must not be null");
    LWS_CHECK_ARG(workspace && rows && vals && info, "objects: workspace, rows, vals and info must not be null");
    LWS_CHECK_ARG(aligned(cam, 4) && aligned(udisp, 4) && aligned(rows, 4) && aligned(vals, 4) && aligned(labels, 4) && aligned(info, 4) &&
                      aligned(workspace, 16),
                  "objects: cam / udisp / rows / vals / labels / info must be 4-byte, workspace 16-byte aligned");
    LWS_CHECK_ARG(code_bits >= 0 && code_bits < 64, "objects: code_bits %d outside 0..63", code_bits);
    LWS_CHECK_ARG(sub >= 1 && sub <= kMaxSub, "objects: sub %d outside 1..%d", sub, kMaxSub);
    int S;
    LWS_CHECK_RC(check_grid("objects", B, W, width, nbins, S));
    LWS_CHECK_ARG(nbins <= 256 * sub, "objects: nbins %d outside 1..min(%d, 256 * sub = %d)", nbins, kMaxBins, 256 * sub);
    LWS_CHECK_ARG(min_count >= 1, "objects: min_count %d < 1", min_count);
    LWS_CHECK_ARG(min_pixels >= 1, "objects: min_pixels %d < 1", min_pixels);
    LWS_CHECK_ARG(max_objects >= 1 && max_objects <= kMaxObjects, "objects: max_objects %d outside 1..%d", max_objects, kMaxObjects);
    const int N = S * nbins;
    const int64_t px = (int64_t)B * H * W, cells = (int64_t)B * N, slots = 32 * (int64_t)B * max_objects;
    const int64_t ws = lws_objects_workspace(B, W, width, nbins);
    const Buf bufs[] = {{workspace, ws, "workspace"}, {rows, slots, "rows"}, {vals, slots, "vals"}, {labels, 4 * px, "labels"},
                        {info, 16 * (int64_t)B, "info"}, {disp, 4 * px, "disp"}, {cam, 20 * (int64_t)B, "cam"}, {codes, px, "codes"},
                        {udisp, 4 * cells, "udisp"}};
    LWS_CHECK_RC(check_no_overlap("objects", bufs, 9, 5));

    int *parent = static_cast<int *>(workspace);
    u32 *rec = reinterpret_cast<u32 *>(static_cast<char *>(workspace) + round256(cells * (int64_t)sizeof(int)));
    int *cnt = reinterpret_cast<int *>(reinterpret_cast<char *>(rec) + round256(cells * kRec * (int64_t)sizeof(u32)));
    const int nblk = (N + kBlock - 1) / kBlock;
    const int ntk = (nbins + kTK - 1) / kTK, nts = (S + kTS - 1) / kTS;
    const int pairs = (ntk - 1) * S + (nts - 1) * nbins;
    const unsigned per_cell = (unsigned)((N + kThreads - 1) / kThreads);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ob_tile, dim3((unsigned)(ntk * nts), B), dim3(kThreads), 0, st, udisp, S, nbins, nts, (unsigned)min_count, parent, rec);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ob_border, dim3((unsigned)(pairs > 0 ? (pairs + kThreads - 1) / kThreads : 1), B), dim3(kThreads), 0, st, S, nbins, ntk,
                       nts, parent);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ob_flatten, dim3(per_cell, B), dim3(kThreads), 0, st, N, parent);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ob_pixels, dim3(S, B), dim3(kThreads), 0, st, disp, cam, codes, udisp, H, W, min_disp, max_depth, (unsigned)code_bits,
                       width, sub, nbins, (unsigned)min_count, rec);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ob_cells, dim3(per_cell, B), dim3(kThreads), 0, st, N, parent, rec);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ob_count, dim3(nblk, B), dim3(kThreads), 0, st, parent, rec, N, min_pixels, cnt);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ob_scan, dim3(B), dim3(kThreads), 0, st, cnt, nblk, max_objects, rows, vals, info);
    LWS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ob_write, dim3(nblk, B), dim3(kThreads), 0, st, parent, rec, cam, cnt, S, nbins, min_pixels, max_objects, rows, vals);
    LWS_LAUNCH_CHECK();
    if (labels) {
        hipLaunchKernelGGL(k_ob_labels, dim3(S, B), dim3(kThreads), 0, st, disp, cam, codes, H, W, min_disp, max_depth, (unsigned)code_bits,
                           width, sub, nbins, parent, rec, labels);
        LWS_LAUNCH_CHECK();
    }
    return LWS_OK;
}

}  // extern "C"
