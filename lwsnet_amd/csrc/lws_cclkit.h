// The shared steps of the connected-component labellers (lws_speckle.hip: the pixels of a disparity map; lws_objects.hip: the cells
// of a u-disparity image; lws_movers.hip: the candidate pixels between two frames).  One scheme: union-find of a 32 x 64 tile in
// LDS, unions across the tile edges in global memory, a flatten to the global root, per-component records filled through integer
// atomics with the lanes of a wave that share a root combined first, and a count / scan / ranked-write numbering of the kept roots.
// Every argument the loops rest on is stated here, once:
// - The invariant: parent[i] <= i in the index order of the caller, always (a root is the FIRST element of its set, a union hangs
//   the later root under the earlier one with an atomic min).  A find walk therefore strictly decreases and ends after at most i
//   steps whatever other workgroups do meanwhile; no loop waits for another thread's progress.
// - Sharing: a word shared between workgroups inside a launch (parent[] in the edge and flatten launches, the records while they
//   are filled) is touched through relaxed agent-scope atomics only; each word stands for itself, there is no payload to publish
//   behind it.  Everything else crosses between workgroups at kernel boundaries.
// - Determinism: what crosses lanes or workgroups is an integer add, min or max, whose order cannot show.
#pragma once
#include <climits>

#include "lws_common.h"
#include "lws_packkit.h"

namespace lws::cclkit {

typedef unsigned long long u64;
typedef unsigned u32;

// ---- the relaxed agent-scope atomics ----
__device__ __forceinline__ int ld_agent(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ void a_add(T *p, T v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ void a_min(T *p, T v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ void a_max(T *p, T v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- union-find in LDS (one tile) ----
// par[i] <= i: the walk strictly decreases, so it ends.
__device__ __forceinline__ int lds_find(const volatile int *par, int i)
{
    for (int n = par[i]; n != i; n = par[i]) i = n;
    return i;
}

// Every round ends the call or strictly lowers max(a, b) (the atomic min hangs the later root a under the earlier one b; when
// another thread re-parented a first, its old parent `o` < a takes a's place and the union goes on as (o, b)), so the loop ends.
__device__ __forceinline__ void lds_unite(int *par, int a, int b)
{
    for (;;) {
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int o = atomicMin(&par[a], b);
        if (o == a) return;
        a = o;
    }
}

// ---- union-find in global memory across workgroups ----
// par[i] <= i, and a parent only ever decreases: the walk strictly decreases, so it ends (after at most i steps).
__device__ __forceinline__ int g_find(const int *par, int i)
{
    for (int n = ld_agent(par + i); n != i; n = ld_agent(par + i)) i = n;
    return i;
}

// As lds_unite: every round returns or strictly lowers max(a, b); it never waits for another workgroup.
__device__ __forceinline__ void g_unite(int *par, int a, int b)
{
    for (;;) {
        a = g_find(par, a);
        b = g_find(par, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int o = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (o == a) return;
        a = o;                                              // a had been hung under o < a meanwhile: o and b are still to be joined
    }
}

// ---- the tile: 32 rows x 64 columns, indexed l = 64 * (row in the tile) + (column in the tile), which grows with the caller's index ----
constexpr int kTileRows = 32, kTileCols = 64;
constexpr int kTile = kTileRows * kTileCols;

// The caller's index of the tile-local element l of the tile at (r0, c0), in rows of `stride` elements
__device__ __forceinline__ int tile_to_index(int l, int r0, int c0, int stride) { return (r0 + l / kTileCols) * stride + c0 + (l & (kTileCols - 1)); }

// joined iff |a - b| <= max_diff; an element that is in no set is staged as NaN, which joins nothing
__device__ __forceinline__ bool joined(float a, float b, float max_diff) { return fabsf(a - b) <= max_diff; }

// The joins of the 4-neighbourhood, to the right and below, of the cell l of a tile staged in LDS (s_d: values, s_par: parents).
// right / below: the cell has that neighbour inside the tile.  The caller says so from its own row and column: a quad-staged
// tile knows three of four `right` at compile time, and k_sp_tile keeps the machine code it had with the loop written out.
__device__ __forceinline__ void join_right_below(const float *s_d, int *s_par, int l, bool right, bool below, float max_diff)
{
    const float d = s_d[l];
    if (right && joined(d, s_d[l + 1], max_diff)) lds_unite(s_par, l, l + 1);
    if (below && joined(d, s_d[l + kTileCols], max_diff)) lds_unite(s_par, l, l + kTileCols);
}

// ---- the tile edges of a raster image: the whole body of k_sp_border and k_mv_border ----
// grid (ceil(n / 256), B), n = (nty - 1) * W + (ntx - 1) * H: thread g < (nty - 1) * W is the pair (y - 1, x), (y, x) on the top
// edge of a tile row, the others the pair (y, x - 1), (y, x) on the left edge of a tile column.  parent[] is shared between
// workgroups here (g_find, g_unite).  The sign of a parent word (-1: in no set) never changes, so it may be tested beforehand.
__device__ __forceinline__ void unite_tile_edges(const float *__restrict__ disp, int H, int W, int nty, int ntx, float max_diff,
                                                 int *__restrict__ parent)
{
    const int64_t g = (int64_t)blockIdx.x * packkit::kThreads + threadIdx.x;
    const int64_t nh = (int64_t)(nty - 1) * W, nv = (int64_t)(ntx - 1) * H;
    if (g >= nh + nv) return;
    const int64_t img = (int64_t)blockIdx.y * H * W;
    int p, q;
    if (g < nh) {
        const int e = (int)(g / W), x = (int)(g - (int64_t)e * W), y = (e + 1) * kTileRows;
        q = y * W + x;
        p = q - W;
    } else {
        const int64_t v = g - nh;
        const int e = (int)(v / H), y = (int)(v - (int64_t)e * H), x = (e + 1) * kTileCols;
        q = y * W + x;
        p = q - 1;
    }
    int *par = parent + img;
    if (ld_agent(par + p) < 0 || ld_agent(par + q) < 0) return;
    if (joined(disp[img + p], disp[img + q], max_diff)) g_unite(par, p, q);
}

// ---- the flatten ----
// i finds its root, points at it and returns it.  Only for a launch in which no union runs, so that a root stays a root; the
// atomic min keeps the invariant (r <= par[i]).  Afterwards par[i] is the first element of i's component.
__device__ __forceinline__ int point_at_root(int *par, int i)
{
    const int r = g_find(par, i);
    if (r != i) a_min(par + i, r);
    return r;
}

// grid (ceil(n / 256), B): one thread per element of image blockIdx.y, every element of a set: the whole body of k_ob_flatten and
// k_mv_flatten
__device__ __forceinline__ void flatten_elements(int n, int *__restrict__ parent)
{
    const int64_t g = (int64_t)blockIdx.x * packkit::kThreads + threadIdx.x;
    if (g >= n) return;
    int *par = parent + (int64_t)blockIdx.y * n;
    if (ld_agent(par + (int)g) >= 0) point_at_root(par, (int)g);
}

// ---- the head of a component's record: 8 words {n, x_min, x_max, y_min, y_max, the component's number (-1: none), SQ (two words)} ----
enum { H_N = 0, H_X0, H_X1, H_Y0, H_Y1, H_NUM, H_SQ, kHeadWords = 8 };

// What a set of member pixels adds to a head (and, as `load`, a head itself)
struct Head {
    int n, x0, x1, y0, y1;
    u64 sq;

    static __device__ __forceinline__ Head none() { return Head{0, INT_MAX, -1, INT_MAX, -1, 0ull}; }
    static __device__ __forceinline__ Head pixel(int x, int y, u64 q) { return Head{1, x, x, y, y, q}; }
    static __device__ __forceinline__ Head load(const int *r) { return Head{r[H_N], r[H_X0], r[H_X1], r[H_Y0], r[H_Y1], *reinterpret_cast<const u64 *>(r + H_SQ)}; }
    // the head of a record that holds nothing yet
    static __device__ __forceinline__ void init(int *r)
    {
        int4 *q = reinterpret_cast<int4 *>(r);
        q[0] = make_int4(0, INT_MAX, -1, INT_MAX);
        q[1] = make_int4(-1, -1, 0, 0);
    }
    __device__ __forceinline__ void merge(const Head &b)
    {
        n += b.n, sq += b.sq;
        x0 = min(x0, b.x0), x1 = max(x1, b.x1), y0 = min(y0, b.y0), y1 = max(y1, b.y1);
    }
    __device__ __forceinline__ Head lane_xor(int o) const
    {
        return Head{__shfl_xor(n, o, 64), __shfl_xor(x0, o, 64), __shfl_xor(x1, o, 64), __shfl_xor(y0, o, 64), __shfl_xor(y1, o, 64), __shfl_xor(sq, o, 64)};
    }
    __device__ __forceinline__ void add_to(int *r) const    // integer atomics only
    {
        a_add(r + H_N, n);
        a_min(r + H_X0, x0), a_max(r + H_X1, x1), a_min(r + H_Y0, y0), a_max(r + H_Y1, y1);
        a_add(reinterpret_cast<u64 *>(r + H_SQ), sq);
    }
    // SQ sums the disparities as u16f words of 1 / 256: the one float step of a labeller
    __device__ __forceinline__ float mean_disp() const { return (float)(((double)sq / (double)n) / 256.0); }
};

// ---- the wave merge ----
// The lanes of the wave that share the key of its first lane with one (>= 0) are merged through a butterfly and that lane adds the
// result to the key's record; every other lane with a key adds for itself.  A wave inside one component costs one set of atomics;
// a wave over scattered keys meets no contention to begin with, and pays no butterfly when its first key is one lane's alone.
// Every lane of the wave must call (key < 0: nothing to add).  A supplies none() (the identity), merge(b), lane_xor(o) (the
// value of lane ^ o) and add_to(rec, key).
template <typename A, typename W>
__device__ __forceinline__ void wave_add(const A &a, int key, W *__restrict__ rec)
{
    const int lane = threadIdx.x & 63;
    const u64 pend = __ballot(key >= 0);
    if (pend == 0) return;                                  // (wave-uniform)
    const int lead = __ffsll((long long)pend) - 1;
    const int k0 = __shfl(key, lead, 64);
    const bool mine = key == k0;
    A r = mine ? a : A::none();                             // (the other lanes: the identity in the butterfly)
    if (__popcll(__ballot(mine)) > 1) {                     // (wave-uniform)
        for (int o = 32; o > 0; o >>= 1) r.merge(r.lane_xor(o));
    }
    if (lane == lead) r.add_to(rec, k0);
    else if (key >= 0 && !mine) a.add_to(rec, key);
}

// ---- the numbering of the kept roots: the three-launch scan of lws_point_cloud over the elements in index order, in blocks of
// 2048 elements (8 consecutive ones per thread): per-block counts, a per-image exclusive scan of them, a ranked write ----
constexpr int kPer = 8;                                     // elements per thread
constexpr int kBlock = packkit::kThreads * kPer;            // ... and per workgroup

// The eight consecutive elements cb .. cb + 7 of a thread, of the n of an image: bit i of `bits` is set iff element cb + i is a
// kept root (its component's root, n >= min_pixels); the elements in a set, the roots and the member pixels of the kept roots
// among them.  r_img: the image's records of kWords words.
struct Kept {
    unsigned bits;
    int in_sets, roots, members;
};

template <int kWords, typename W>
__device__ __forceinline__ Kept kept_roots(const int *__restrict__ par, const W *__restrict__ r_img, int64_t cb, int n, int min_pixels)
{
    Kept k = {0u, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        const int64_t c = cb + i;
        const int p = c < n ? par[c] : -1;
        k.in_sets += p >= 0, k.roots += p == (int)c;
        if (p != (int)c) continue;
        const int m = (int)r_img[c * kWords + H_N];
        if (m >= min_pixels) k.bits |= 1u << i, k.members += m;
    }
    return k;
}

// One workgroup: c[stride * i], the kept roots of block i < nblk of an image, becomes the kept roots before the block (an exclusive
// scan, 256 blocks a round); side(i) lets the caller add block i's other counts on the way.  Returns the image's kept roots.
template <typename F>
__device__ __forceinline__ int scan_blocks(int *__restrict__ c, int stride, int nblk, int *s_w, F &&side)
{
    int before = 0;
    for (int i0 = 0; i0 < nblk; i0 += packkit::kThreads) {
        const int i = i0 + threadIdx.x;
        const int at = packkit::block_scan(i < nblk ? c[stride * i] : 0, s_w, before);
        if (i < nblk) {
            c[stride * i] = at;
            side(i);
        }
        __syncthreads();                                    // s_w is rewritten by the next round
    }
    return before;
}

// A slot of the outputs: 8 ints of rows and NV floats of vals; and the slots from..max - 1 past the kept components, which the
// ranked write does not touch, by one workgroup
template <int NV>
__device__ __forceinline__ void store_slot(int32_t *__restrict__ rows, float *__restrict__ vals, int j, const int (&r)[8], const float (&v)[NV])
{
#pragma unroll
    for (int i = 0; i < 8; ++i) rows[8 * (int64_t)j + i] = r[i];
#pragma unroll
    for (int i = 0; i < NV; ++i) vals[NV * (int64_t)j + i] = v[i];
}

template <int NV>
__device__ __forceinline__ void clear_slots(int32_t *__restrict__ rows, float *__restrict__ vals, int from, int max)
{
    const int none[8] = {0, -1, -1, -1, -1, -1, -1, 0};
    const float zero[NV] = {};
    for (int j = min(from, max) + threadIdx.x; j < max; j += packkit::kThreads) store_slot<NV>(rows, vals, j, none, zero);
}

// The ranked walk: a kept root's number j is the kept roots before its block (`before`, the scanned count) plus those before it
// inside the block; f(i, j) for every set bit i of keep, in order.  Every thread of the workgroup calls (one barrier inside).
template <typename F>
__device__ __forceinline__ void for_each_kept(unsigned keep, int before, int *s_w, F &&f)
{
    int j = packkit::block_scan((int)__popc(keep), s_w, before);
    for (int i = 0; i < kPer; ++i) {
        if (!((keep >> i) & 1u)) continue;
        f(i, j);
        ++j;
    }
}

}  // namespace lws::cclkit
