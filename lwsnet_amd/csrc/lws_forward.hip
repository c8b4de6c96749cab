// Running the network: the workspace layout, the built-in profiler's event pairs, the launch plan of LWSNet.forward
// (models/models.py:106-164 of the reference) and the entry points that execute it on a handle.
#include <algorithm>
#include <chrono>

#include "lws_common.h"

namespace lws {

struct WsLayout {
    size_t act_a, act_b, cost_raw, cost_out, low[3], total;   // float offsets (hot path); low[s]: stage s low-res disparity
    // 2D networks: feature-extractor maps for N = 2B images, refinement ping-pong maps
    size_t fe_o, fe_o2, fe_pre, fe_f8, fe_f4, fe_o3, fe_cls, fe_f2;
    size_t r_a, r_b, r_c;
    size_t total_all;
};

// Feature-map sizes: the stem convolution (submodules.py:118-125: k3 s2 dil2 pad2) gives ceil(H/2); the hourglass halves
// twice more (check_size guarantees ceil(H/2) % 4 == 0).  H = 8k-1 is therefore as legal as H = 8k.
static inline int half_up(int v) { return (v + 1) / 2; }

// src_index's offset for every resize of the path (lws_device_math.h): lws_config.interp_align_mode
static inline float ioff_of(const lws_ctx *h) { return h->cfg.interp_align_mode == 1 ? 0.0f : 0.5f; }

// Stage s at input size H x W: D hypotheses from `start` on, over a map of hh x ww
struct StageDims {
    int D, hh, ww;
    float start;
};
static StageDims stage_dims(const lws_ctx *h, int s, int H, int W)
{
    const int div = 4 >> s, m = h->cfg.maxdisplist[s];
    return {s == 0 ? m : 2 * m - 1, half_up(H) / div, half_up(W) / div, s == 0 ? 0.0f : (float)(-m + 1)};
}

static WsLayout ws_layout(const lws_ctx *h, int B, int H, int W)
{
    size_t max_act = 0, max_cost = 0;
    for (int s = 0; s < 3; ++s) {
        const StageDims d = stage_dims(h, s, H, W);
        size_t vox = (size_t)B * d.D * d.hh * d.ww;
        max_cost = std::max(max_cost, vox);
        max_act = std::max(max_act, vox * (size_t)h->stage[s].c3);
    }
    auto al = [](size_t n) { return (n + 63) & ~(size_t)63; };
    WsLayout L;
    L.act_a = 0;
    L.act_b = L.act_a + al(max_act);
    L.cost_raw = L.act_b + al(max_act);
    L.cost_out = L.cost_raw + al(max_cost);
    L.low[0] = L.cost_out + al(max_cost);
    const int H2 = half_up(H), W2 = half_up(W);
    const size_t N = 2 * (size_t)B, p2 = (size_t)H2 * W2, p4 = (size_t)(H2 / 2) * (W2 / 2), p8 = (size_t)(H2 / 4) * (W2 / 4);
    L.low[1] = L.low[0] + al((size_t)B * p8);
    L.low[2] = L.low[1] + al((size_t)B * p4);
    L.total = L.low[2] + al((size_t)B * p2);
    size_t o = L.total;
    auto take = [&](size_t n) { size_t r = o; o += al(n); return r; };
    L.fe_o = take(N * 8 * p2);
    L.fe_o2 = take(N * 8 * p2);
    L.fe_pre = take(N * 16 * p4);
    L.fe_f8 = take(N * 16 * p8);
    L.fe_f4 = take(N * 16 * p4);
    L.fe_o3 = take(N * 8 * p2);
    L.fe_cls = take(N * 8 * p2);
    L.fe_f2 = take(N * 8 * p2);
    L.r_a = take((size_t)B * H * W * 32);
    L.r_b = take((size_t)B * H * W * 32);
    L.r_c = take((size_t)B * H * W * 32);
    L.total_all = o;
    return L;
}

static int ensure_ws(lws_ctx *h, size_t floats)
{
    const size_t bytes = floats * sizeof(float);
    if (h->ws_bytes >= bytes) return LWS_OK;
    if (h->ws) LWS_HIP(hipFree(h->ws));
    h->ws = nullptr;
    h->ws_bytes = 0;
    LWS_HIP(hipMalloc(&h->ws, bytes));
    h->ws_bytes = bytes;
    return LWS_OK;
}

// the hourglass skip-adds (submodules.py:103,182) need ceil(H/2), ceil(W/2) divisible by 4
static inline bool size_ok(int H, int W) { return H > 0 && W > 0 && half_up(H) % 4 == 0 && half_up(W) % 4 == 0; }

static int check_size(const lws_ctx *h, int B, int H, int W)
{
    LWS_CHECK_ARG(B >= 1, "batch must be >= 1 (got %d)", B);
    // size_ok; models.py:72 needs w/8 >= D1
    LWS_CHECK_ARG(size_ok(H, W),
                  "unsupported input size %dx%d: ceil(H/2) and ceil(W/2) must be divisible by 4", H, W);
    LWS_CHECK_ARG(half_up(W) / 4 >= h->cfg.maxdisplist[0],
                  "unsupported input size %dx%d: the 1/8 map is %d wide, must be >= maxdisplist[0] = %d", H, W,
                  half_up(W) / 4, h->cfg.maxdisplist[0]);
    return LWS_OK;
}

// ---- built-in profiler: one hipEvent pair per launch on the launch stream ---------------------
static const size_t kMaxProfRecords = 65536;

static hipEvent_t prof_event(lws_ctx *h)
{
    if (!h->evt_pool.empty()) {
        hipEvent_t e = h->evt_pool.back();
        h->evt_pool.pop_back();
        return e;
    }
    // timing events never publish data to the host: no system-scope fence when they complete
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return nullptr;
    return e;
}

// stamped: the launch inside the scope takes t0() / t1() and its kernel stamps them with its own begin / end
// (hipExtLaunchKernelGGL), instead of the scope recording them around the launch
struct ProfScope {
    lws_ctx *h;
    hipStream_t st;
    lws_prof_rec rec;
    bool live, stamped;
    ProfScope(lws_ctx *h_, int kc, hipStream_t st_, bool stamped_ = false) : h(h_), st(st_), live(false), stamped(stamped_)
    {
        if (!((h->prof_mask >> kc) & 1u) || h->prof.size() >= kMaxProfRecords) return;
        rec.kc = kc;
        rec.t0 = prof_event(h);
        rec.t1 = prof_event(h);
        if (!rec.t0 || !rec.t1) return;
        live = stamped || hipEventRecord(rec.t0, st) == hipSuccess;
    }
    hipEvent_t t0() const { return live && stamped ? rec.t0 : nullptr; }
    hipEvent_t t1() const { return live && stamped ? rec.t1 : nullptr; }
    ~ProfScope()
    {
        if (!live) return;
        if (stamped || hipEventRecord(rec.t1, st) == hipSuccess) h->prof.push_back(rec);
    }
};

void prof_clear(lws_ctx *h)
{
    for (lws_prof_rec &r : h->prof) {
        h->evt_pool.push_back(r.t0);
        h->evt_pool.push_back(r.t1);
    }
    h->prof.clear();
}

// lws_debug_delay_side's kernel: ONE wave that holds its stream for `ticks` ticks of the 100 MHz counter (clock_pair's wall
// clock), asleep between two reads.  It stores nothing.  One s_sleep 127 is 127 x 64 = 8128 shader cycles: 3.4 us at the 2.4 GHz
// peak clock, 3.9 us at the 2.1 GHz the kernels here hold, more at any lower clock.  The loop is bounded by `cap` = us / 2 + 2
// sleeps, so a counter that did not advance ends it after at least 1.7 x the request, about 2 x at 2.1 GHz (0.5 s for the largest
// request, 250 ms) -- and the cap can never cut a delay short while the counter runs.
__global__ void __launch_bounds__(64) k_debug_delay(unsigned long long ticks, int cap)
{
    unsigned long long shader, t0, t;
    clock_pair(shader, t0);
    for (int i = 0; i < cap; ++i) {
        clock_pair(shader, t);
        if (t - t0 >= ticks) break;
        __builtin_amdgcn_s_sleep(127);
    }
}

// The head of side segment `bit` (LWS_DELAY_*): lws_debug_delay_side's kernel on the side stream when that segment is selected.
// Off (every handle no test has touched) this is the one branch.  Callers pass the side stream of a multi-stream plan only.
static inline int delay_side(const lws_ctx *h, int bit, hipStream_t side)
{
    if (!(h->opt.delay_segments & bit)) return LWS_OK;
    hipLaunchKernelGGL(k_debug_delay, dim3(1), dim3(64), 0, side, (unsigned long long)h->opt.delay_us * 100ull, h->opt.delay_us / 2 + 2);
    LWS_HIP(hipGetLastError());
    return LWS_OK;
}

// low != nullptr: the soft-argmin is wanted too; *fused tells the caller whether it was done here.  fork: see Fork
static int conv3d_stack(lws_ctx *h, int stage, const float *cost_in, float *cost_out, float *act_a, float *act_b,
                        int B, int D, int hh, int ww, hipStream_t st, float *low = nullptr, float start = 0.f,
                        bool *fused = nullptr, bool first_done = false, const Fork &fork = Fork())
{
    const Stage3d &s = h->stage[stage];
    int rc = LWS_OK;
    if (!first_done) {     // (first_done: act_a already holds the first layer's output, see launch_shift_first)
        ProfScope p(h, LWS_KC_CONV3D_FIRST, st);
        rc = launch_conv3d_first(s, cost_in, act_a, B, D, hh, ww, st);
    }
    if (rc) return rc;
    float *src = act_a, *dst = act_b;
    for (int j = 1; j <= h->cfg.layers_3d; ++j) {
        StopArm stop(j == fork.after ? fork : Fork(), st);
        {
            // dominant kernel (mid16): timed by its own begin / end timestamps, not by events around the launch
            const bool own = s.c3 != 8;
            ProfScope p(h, own ? LWS_KC_CONV3D_MID16 : LWS_KC_CONV3D_MID8, st, own);
            rc = launch_conv3d_mid(s, j, src, dst, B, D, hh, ww, st, p.t0(), p.t1());
            if (own && rc) p.live = false;      // (nothing has stamped the events)
        }
        LWS_HIP(stop.finish(rc));
        if (rc) return rc;
        std::swap(src, dst);
    }
    {
        ProfScope p(h, LWS_KC_CONV3D_LAST, st);
        StopArm stop(fork.after == 0 ? fork : Fork(), st);
        if (low != nullptr && conv3d_last_can_fuse(s, D)) {
            *fused = true;
            rc = launch_conv3d_last_softargmin(s, src, cost_in, nullptr, low, start, B, D, hh, ww, st);
        } else {
            if (fused) *fused = false;
            rc = launch_conv3d_last(s, src, cost_in, cost_out, B, D, hh, ww, st);
        }
        LWS_HIP(stop.finish(rc));
    }
    return rc;
}


// One launch of the 2D networks (feature extractor, refinement) on stream `st`, timed as kernel class kc; returns on error
#define LWS_TIMED(kc, call)            \
    {                                  \
        ProfScope p_(h, kc, st);       \
        rc = (call);                   \
    }                                  \
    if (rc) return rc;

// feature_extraction.forward (submodules.py:176-188) up to the 1/8 map f8, on N = nA + nB images read from two tensors (left
// batch, right batch) as ONE batch.  Stage 1 needs nothing else: lws_forward runs feature_tail (conv5, conv6, classif1 -> f4, f2)
// on a side stream later, beside the volume stages.  fork (optional): complete once f8 / pre are
static int feature_head(lws_ctx *h, const float *imgA, const float *imgB, int nA, int nB, int H, int W, const WsLayout &L,
                        float *f8, hipStream_t st, const Fork &fork = Fork())
{
    const Net2d &n = h->net2d;
    const int N = nA + nB, H2 = half_up(H), W2 = half_up(W), H4 = H2 / 2, W4 = W2 / 2;
    float *ws = h->ws;
    float *o = ws + L.fe_o, *o2 = ws + L.fe_o2, *pre = ws + L.fe_pre;
    const float *img2 = nB > 0 ? imgB : nullptr;
    int rc;
    // dres0, dres1, hourglass conv1..conv4: consecutive layers run pairwise in one launch (k_conv2d_pair /
    // k_conv2d_pair_mfma, the same fma chains as one kernel per layer)
    LWS_TIMED(LWS_KC_FEATURE2D, launch_conv2d_pair(n.fe[0], n.fe[1], imgA, nullptr, o, N, H, W, st, img2, nA));    // dres0
    LWS_TIMED(LWS_KC_FEATURE2D, launch_conv2d_pair(n.fe[2], n.fe[3], o, o, o2, N, H2, W2, st));                     // dres1 + o (:179)
    LWS_TIMED(LWS_KC_FEATURE2D, launch_conv2d_pair(n.fe[4], n.fe[5], o2, nullptr, pre, N, H2, W2, st));             // conv1, conv2 -> pre
    {
        StopArm stop(fork, st);
        ProfScope p_(h, LWS_KC_FEATURE2D, st);
        rc = launch_conv2d_pair(n.fe[6], n.fe[7], pre, nullptr, f8, N, H4, W4, st);                  // conv3, conv4 -> f8
        LWS_HIP(stop.finish(rc));
    }
    return rc;
}

// conv5 (-> f4), conv6, classif1 (-> f2), submodules.py:103-107,182-186.  ev (optional): ev[1] recorded after f4,
// ev[2] after f2, on st.  part: bit 0 = conv5 (f4), bit 1 = conv6 + classif1 (f2).
static int feature_tail(lws_ctx *h, int N, int H, int W, const WsLayout &L, float *f8, float *f4, float *f2,
                        hipStream_t st, hipEvent_t *ev, int part)
{
    const Net2d &n = h->net2d;
    const int H2 = half_up(H), W2 = half_up(W), H4 = H2 / 2, W4 = W2 / 2, H8 = H2 / 4, W8 = W2 / 4;
    float *ws = h->ws;
    float *o2 = ws + L.fe_o2, *pre = ws + L.fe_pre, *o3 = ws + L.fe_o3, *cls = ws + L.fe_cls;
    int rc;
    if (part & 1) {
        LWS_TIMED(LWS_KC_FEATURE2D, launch_conv2d_nchw(n.fe[8], f8, pre, f4, N, H8, W8, st));          // relu(conv5 + pre) (:103)
        if (ev != nullptr) LWS_HIP(hipEventRecord(ev[1], st));
    }
    if (part & 2) {
        LWS_TIMED(LWS_KC_FEATURE2D, launch_conv2d_nchw(n.fe[9], f4, o2, o3, N, H4, W4, st));           // conv6 + output (:106,:182)
        LWS_TIMED(LWS_KC_FEATURE2D, launch_conv2d_nchw(n.fe[10], o3, nullptr, cls, N, H2, W2, st));    // classif1.0
        LWS_TIMED(LWS_KC_FEATURE2D, launch_conv2d_nchw(n.fe[11], cls, nullptr, f2, N, H2, W2, st));    // classif1.2 -> f2
        if (ev != nullptr) LWS_HIP(hipEventRecord(ev[2], st));
    }
    return LWS_OK;
}

// The refinement maps are [B,H,W,32] float32 = 128 B per pixel (134 MB at 8 x 256x512) and every block reads one and writes
// another.  A chunk of pairs runs its whole layer chain before the next chunk starts, sized so that one map of the chunk is
// at most `ref_chunk_mb` MB: the three maps a block chain touches then stay in the 256 MiB Infinity Cache between a block's
// write and the next block's read (MI355X_MICROARCH.md: a table stays resident while it plus everything moved between two
// uses fits in ~256 MiB).  0 = one chunk.  Pairs are independent, so chunking cannot change a bit.
static int refine_chunk(const lws_ctx *h, int B, int H, int W)
{
    if (h->opt.ref_chunk_mb <= 0) return B;
    const double map_mb = (double)H * W * 128.0 / 1e6;
    int c = (int)((double)h->opt.ref_chunk_mb / map_mb);
    c = c < 1 ? 1 : c;
    return c < B ? c : B;
}

// refinement1_left(left) (models.py:158): depends on the left image only -> result in r_a.  Each chunk keeps its slice of r_a;
// the scratch map r_c is the SAME memory for every chunk (it stays cache-resident)
static int refine_left(lws_ctx *h, const float *left, int B, int H, int W, const WsLayout &L, hipStream_t st)
{
    const Net2d &n = h->net2d;
    const int CH = refine_chunk(h, B, H, W);
    float *rc_ = h->ws + L.r_c;
    int rc;
    for (int b0 = 0; b0 < B; b0 += CH) {
        const int nb = std::min(CH, B - b0);
        float *ra = h->ws + L.r_a + (size_t)b0 * H * W * 32;
        StageMap img{const_cast<float *>(left) + (size_t)b0 * 3 * H * W, true};
        if ((h->opt.fuse_first & 2) && ref_first_dws_can_fuse(n.r1[0][0], 3)) {
            // the 3 -> 32 convolution is recomputed inside the first block's staging: one launch less, and the 32-channel map
            // it would write (and the block read back) never exists
            LWS_TIMED(LWS_KC_REF_DWS, launch_ref_first_dws(n.r1[0][0], img, 3, n.r1_first_mfma[0], rc_, nb, H, W, st));
        } else {
            LWS_TIMED(LWS_KC_REF_FIRST, launch_ref_first(img.mem, 3, n.r1_first[0], ra, nb, H, W, st));
            LWS_TIMED(LWS_KC_REF_DWS, launch_ref_dws(n.r1[0][0], ra, rc_, nb, H, W, st));
        }
        LWS_TIMED(LWS_KC_REF_DWS, launch_ref_dws(n.r1[0][1], rc_, ra, nb, H, W, st));
        LWS_TIMED(LWS_KC_REF_DWS, launch_ref_dws(n.r1[0][2], ra, rc_, nb, H, W, st));
        LWS_TIMED(LWS_KC_REF_DWS, launch_ref_dws(n.r1[0][3], rc_, ra, nb, H, W, st));
    }
    return LWS_OK;
}

// One chunk of refine_rest: pairs b0 .. b0 + n - 1 on stream st, its scratch maps from pair `scratch` on.  after_disp
// (optional): recorded once the chunk's refinement1_disp branch is done.
struct RefChunk {
    int b0, n, scratch;
    hipStream_t st;
    hipEvent_t after_disp;
};

static int refine_rest_chunk(lws_ctx *h, const StageMap &pred3, const RefChunk &c, int H, int W, const WsLayout &L,
                             float *pred4, bool fuse_last)
{
    const Net2d &n = h->net2d;
    const int B = c.n;
    hipStream_t st = c.st;
    const size_t po = (size_t)c.b0 * H * W;
    StageMap p3 = pred3;          // this chunk's pairs (a deferred map is one chunk)
    p3.mem += po;
    pred4 += po;
    // r_a: this chunk's slice (refinement1_left's result); r_b, r_c: the same memory for every chunk
    float *ra = h->ws + L.r_a + po * 32, *rb = h->ws + L.r_b + (size_t)c.scratch * H * W * 32,
          *rc_ = h->ws + L.r_c + (size_t)c.scratch * H * W * 32;
    int rc;
    if ((h->opt.fuse_first & 1) && ref_first_dws_can_fuse(n.r1[1][0], 1)) {
        // refinement1_disp: the 1 -> 32 convolution is recomputed inside the first block's staging (one launch less); a deferred
        // pred3 is evaluated there and written out
        LWS_TIMED(LWS_KC_REF_DWS, launch_ref_first_dws(n.r1[1][0], p3, 1, n.r1_first_mfma[1], rc_, B, H, W, st, ioff_of(h)));
    } else {
        LWS_TIMED(LWS_KC_REF_FIRST, launch_ref_first(p3.mem, 1, n.r1_first[1], rb, B, H, W, st));
        LWS_TIMED(LWS_KC_REF_DWS, launch_ref_dws(n.r1[1][0], rb, rc_, B, H, W, st));
    }
    // refinement1_disp blocks 2..4 (dil 4, 8, 16; block 1 ran above): rc_ -> ... -> rb
    LWS_TIMED(LWS_KC_REF_DWS, launch_ref_dws(n.r1[1][1], rc_, rb, B, H, W, st));
    LWS_TIMED(LWS_KC_REF_DWS, launch_ref_dws(n.r1[1][2], rb, rc_, B, H, W, st));
    LWS_TIMED(LWS_KC_REF_DWS, launch_ref_dws(n.r1[1][3], rc_, rb, B, H, W, st));
    if (c.after_disp != nullptr) LWS_HIP(hipEventRecord(c.after_disp, st));
    LWS_TIMED(LWS_KC_REF_CONV64, launch_ref_conv64(n.r2_first, ra, rb, rc_, B, H, W, st));
    LWS_TIMED(LWS_KC_REF_DWS, launch_ref_dws(n.r2[0], rc_, ra, B, H, W, st));
    LWS_TIMED(LWS_KC_REF_DWS, launch_ref_dws(n.r2[1], ra, rc_, B, H, W, st));
    LWS_TIMED(LWS_KC_REF_DWS, launch_ref_dws(n.r2[2], rc_, ra, B, H, W, st));
    // refinement2[4] + refinement2[5] + pred3: one launch (k_ref_dws_last) or two (refine_rest decides)
    if (fuse_last && ref_dws_last_can_fuse(n.r2[3])) {
        LWS_TIMED(LWS_KC_REF_LAST, launch_ref_dws_last(n.r2[3], ra, n.r2_last, p3.mem, pred4, B, H, W, st));
        return LWS_OK;
    }
    LWS_TIMED(LWS_KC_REF_DWS, launch_ref_dws(n.r2[3], ra, rc_, B, H, W, st));
    LWS_TIMED(LWS_KC_REF_LAST, launch_ref_last(rc_, n.r2_last, p3.mem, pred4, B, H, W, st));
    return LWS_OK;
}
#undef LWS_TIMED

// models.py:159-162: refinement1_disp(pred3), refinement2(concat), + pred3.  Needs refine_left's result in r_a.
static int refine_rest(lws_ctx *h, const StageMap &pred3, int B, int H, int W, const WsLayout &L, float *pred4, hipStream_t st)
{
    const int CH = pred3.written ? refine_chunk(h, B, H, W) : B;      // (a deferred map: batches <= 2, one chunk)
    // Option "ref_pipe": chunks alternate between the caller's stream and the side stream (idle by now), each starting once the
    // previous chunk has finished its disparity branch, so that one chunk's memory-bound blocks run beside the other's MFMA-bound
    // 64 -> 32 convolution; odd chunks use the second half of the (batch-sized) scratch maps.  Two chunks only add their
    // collisions, hence the automatic setting wants at least four.
    // refinement2[4] + refinement2[5] + pred3 in one launch (k_ref_dws_last): option "fuse_ref_last"; automatic = batch 1 only
    // (the fused launch takes as long as the two it replaces, so all it buys is one dispatch gap).
    // Numbers for both: profiles/NOTES.md, "refinement launch plan".
    const bool fuse_last = h->opt.fuse_ref_last >= 0 ? h->opt.fuse_ref_last != 0 : B <= 1;
    const int nchunks = (B + CH - 1) / CH;
    const int want = h->opt.ref_pipe >= 0 ? h->opt.ref_pipe : (nchunks >= 4 ? 1 : 0);
    const bool pipe = want != 0 && h->side != nullptr && h->opt.side_streams != 0 && nchunks >= 2 && 2 * CH <= B;
    if (pipe) {
        LWS_HIP(hipEventRecord(h->ev_fork, st));
        LWS_HIP(hipStreamWaitEvent(h->side, h->ev_fork, 0));
    }
    int k = 0;
    for (int b0 = 0; b0 < B; b0 += CH, ++k) {
        const RefChunk c{b0, std::min(CH, B - b0), pipe ? (k & 1) * CH : 0, (pipe && (k & 1)) ? h->side : st,
                         pipe ? h->ev_feat[k & 1] : nullptr};
        if (pipe && k > 0) LWS_HIP(hipStreamWaitEvent(c.st, h->ev_feat[(k - 1) & 1], 0));
        if (pipe && (k & 1)) {
            const int rc = delay_side(h, LWS_DELAY_CHUNKS, c.st);
            if (rc) return rc;
        }
        const int rc = refine_rest_chunk(h, pred3, c, H, W, L, pred4, fuse_last);
        if (rc) return rc;
    }
    if (pipe) {
        LWS_HIP(hipEventRecord(h->ev_join, h->side));
        LWS_HIP(hipStreamWaitEvent(st, h->ev_join, 0));
    }
    return LWS_OK;
}

// Deferred maps (StageMap): where the caller lets map[s] wait for its consumer (keep), the fused last Conv3D layer + soft-argmin
// leaves the low-resolution disparity and no launch on the critical chain materialises the map.  Stage 1's map is read by stage
// 2's warp kernel (the four taps it needs) and written out by stage 3's, which evaluates it beside the deferred stage-2 map
// (two-level DeferredMap); stage 3's map is written out by the refinement's first block.  Batches <= 2 only (two launches fewer
// on a batch-1 chain; from batch 4 up the heavier consumers cost more than the launches, so large batches keep the separate
// k_upsample_add launches), and only at exact 2x geometry: with odd H or W the four taps of a stage-3 pixel are not the 2x2
// block it owns.  Stage 1: the fused last layer only pays when its map can leave the chain; otherwise the
// k_softargmin_upsample launch does soft-argmin AND upsample in one kernel.
static bool defers(const lws_ctx *h, int s, int B, int H, int W, bool keep)
{
    return keep && h->opt.defer_upsample != 0 && B <= 2 && H % 2 == 0 && W % 2 == 0 && (s > 0 || h->opt.fuse_last1 != 0);
}

// Stage s of LWSNet.forward up to its Conv3D stack (models.py:119-138; fork: see Fork).  fused: the stack's last layer did the
// soft-argmin too (into low[s]).  keep_cost (lws_forward_conf): the last layer never fuses, so the filtered cost is in L.cost_out.
static int stage_volume(lws_ctx *h, int s, const StageDims &d, const float *featL, const float *featR, int B, int H, int W,
                        StageMap map[3], const WsLayout &L, hipStream_t st, bool defer, bool &fused, const Fork &fork = Fork(),
                        bool keep_cost = false)
{
    static const int feat_c[3] = {16, 16, 8};   // feature_extraction outputs, submodules.py:101,104,186
    float *act_a = h->ws + L.act_a, *act_b = h->ws + L.act_b, *raw = h->ws + L.cost_raw, *cost = h->ws + L.cost_out;
    float *low = h->ws + L.low[s];
    const int D = d.D, hh = d.hh, ww = d.ww;
    int rc;
    bool first_done = false;
    if (s == 0 && shift_first_can_fuse(h->stage[0], feat_c[0])) {
        // stage-1 volume and the first Conv3D layer in one launch (the raw volume is still written: skip input)
        ProfScope p(h, LWS_KC_CONV3D_FIRST, st);
        rc = launch_shift_first(h->stage[0], featL, featR, raw, act_a, B, feat_c[0], D, hh, ww, st,
                                h->cfg.feature_fp16 != 0);                                                          // :131
        first_done = true;
    } else if (s == 0) {
        ProfScope p(h, LWS_KC_VOLUME_SHIFT, st);
        rc = launch_volume_l1_shift(featL, featR, raw, B, feat_c[0], hh, ww, D, st, h->cfg.feature_fp16 != 0);         // :131
    } else {
        ProfScope p(h, LWS_KC_VOLUME_WARP, st);
        rc = launch_volume_l1_warp(featL, featR, map[s - 1], raw, nullptr, B, feat_c[s], hh, ww, H, W, h->cfg.maxdisplist[s],
                                   st, h->cfg.feature_fp16 != 0, h->opt.warp_form, ioff_of(h));                       // :119-127
    }
    if (rc) return rc;
    fused = false;
    return conv3d_stack(h, s, raw, cost, act_a, act_b, B, D, hh, ww, st, (!keep_cost && (s > 0 || defer)) ? low : nullptr, d.start, &fused,
                        first_done, fork);                                                                          // :136-138
}

// Materialises a deferred map with one k_upsample_add (models.py:145-148,153-156); the map before it is in memory
static int write_out(lws_ctx *h, StageMap &m, int B, int H, int W, hipStream_t st)
{
    if (m.written) return LWS_OK;
    ProfScope p(h, LWS_KC_UPSAMPLE, st);
    const int rc = launch_upsample_add(m.low, m.prev != nullptr ? m.prev->mem : nullptr, m.mem, B, m.h, m.w, H, W, st, ioff_of(h));
    m.written = rc == LWS_OK;
    return rc;
}

// The map of stage s, after stage_volume: left deferred, or computed into memory (models.py:142-156).  A map before it that
// is still unwritten is materialised first.
static int stage_map(lws_ctx *h, int s, const StageDims &d, int B, int H, int W, StageMap map[3], const WsLayout &L,
                     hipStream_t st, bool defer, bool fused)
{
    const int D = d.D, hh = d.hh, ww = d.ww;
    const float start = d.start;
    float *cost = h->ws + L.cost_out, *low = h->ws + L.low[s];
    StageMap &m = map[s];
    m.low = low;
    m.h = hh;
    m.w = ww;
    m.prev = s > 0 ? &map[s - 1] : nullptr;
    if (fused && defer) return LWS_OK;
    int rc;
    if (m.prev != nullptr) {
        rc = write_out(h, *m.prev, B, H, W, st);
        if (rc) return rc;
    }
    if (!fused && H % hh == 0 && W % ww == 0) {
        // soft-argmin + rescale + upsample (+ previous stage) in one launch                                     :142-148
        ProfScope p(h, LWS_KC_SOFTARGMIN, st);
        rc = launch_softargmin_upsample(cost, m.prev != nullptr ? m.prev->mem : nullptr, m.mem, nullptr, B, D, hh, ww, H, W,
                                        start, st, ioff_of(h));
        m.written = rc == LWS_OK;
        return rc;
    }
    if (!fused) {
        // H or W = 8k-1: the resize ratio is not an integer, which the fused kernel's tile -> block map needs
        ProfScope p(h, LWS_KC_SOFTARGMIN, st);
        rc = launch_softargmin(cost, low, B, D, hh, ww, start, st);
        if (rc) return rc;
    }
    return write_out(h, m, B, H, W, st);                                                                          // :145-156
}

// The preamble of the entry points that run the network: the handle's device is current, lws_finalize has run (with every 2D
// tensor set: need_2d; the error `state_msg` otherwise), the workspace holds `floats`, and no stop event is armed on this thread.
static int begin_call(lws_ctx *h, const char *what, bool need_2d, const char *state_msg, size_t floats)
{
    LWS_CHECK_DEVICE(h, what);
    if (!h->finalized || (need_2d && !h->have_2d)) {
        set_error("%s", state_msg);
        return LWS_ERR_STATE;
    }
    const int rc = ensure_ws(h, floats);
    if (rc) return rc;
    (void)stop_event_take();
    return LWS_OK;
}

// side stream and cross-stream events of lws_forward: created by lws_reserve (which promises that later calls allocate
// nothing) or, for callers that never reserve, on the first forward.  (A CU-masked side stream was built, measured and removed
// in round 5: profiles/NOTES.md, "CU masks".)
static int ensure_streams(lws_ctx *h)
{
    if (h->side) return LWS_OK;
    const unsigned ef = hipEventDisableTiming | hipEventDisableSystemFence;
    LWS_HIP(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
    LWS_HIP(hipEventCreateWithFlags(&h->ev_fork, ef));
    LWS_HIP(hipEventCreateWithFlags(&h->ev_join, ef));
    for (int i = 0; i < 3; ++i) LWS_HIP(hipEventCreateWithFlags(&h->ev_feat[i], ef));
    LWS_HIP(hipEventCreateWithFlags(&h->ev_fork2, ef));
    return LWS_OK;
}

// A join of lws_forward: everything queued on `st` from here on runs after `ev` (recorded on the side stream) is complete.
// hipStreamWaitEvent on an event that is NOT complete when the host calls it puts a wait on st's queue, which costs the chain
// 5 to 7 us even when the event has long completed by the time the queue reaches it; on an event that IS complete the runtime
// queues nothing (tools/micro/event_cost.hip; profiles/NOTES.md, "host-resolved joins").  host: poll the event first.  Once the
// host has seen it complete, every later launch on st is ordered behind the side work and nothing is queued at all.  The poll is
// bounded by option "host_join_budget_us"; when that runs out (or is 0) the wait is queued as before, so the budget decides
// where the host spends its time and never what is computed -- and `host` is cleared: the caller's stream is backed up, the
// forward's later joins would run out as well, so they queue at once and one forward spins for one budget at the most.
// Never under hipGraph capture (the caller passes host = false): an event query is illegal there, and a captured graph needs
// the wait as an edge.
static int host_join(lws_ctx *h, int which, hipEvent_t ev, hipStream_t st, bool &host)
{
    lws_join_stat &js = h->join_stat[which];
    if (host && h->opt.host_join_budget_us > 0) {
        typedef std::chrono::steady_clock clk;
        const clk::time_point t0 = clk::now(), t_end = t0 + std::chrono::microseconds(h->opt.host_join_budget_us);
        clk::time_point t = t0;
        hipError_t e;
        do {
            e = hipEventQuery(ev);
            t = clk::now();
        } while (e == hipErrorNotReady && t < t_end);
        const int64_t ns = std::chrono::duration_cast<std::chrono::nanoseconds>(t - t0).count();
        js.wait_ns += ns;
        js.max_ns = std::max(js.max_ns, ns);
        if (e == hipSuccess) {
            ++js.host;
            return LWS_OK;
        }
        if (e != hipErrorNotReady) {
            set_error("hipEventQuery failed at join %d of the forward: %s", which, hipGetErrorString(e));
            return LWS_ERR_HIP;
        }
        host = false;
    }
    ++js.queued;
    LWS_HIP(hipStreamWaitEvent(st, ev, 0));
    return LWS_OK;
}

// Which handle ran the latest forward on this thread (automatic "host_joins"): a thread that feeds several handles in turn
// (bench.py --streams N) must not be held at a join of one while the others have nothing queued.  Compared, never
// dereferenced: a handle destroyed since, or a new one at its address, costs at most one forward on the other plan.
static thread_local const lws_ctx *tl_last_forward = nullptr;

}  // namespace lws

using namespace lws;

extern "C" {

int lws_reserve(lws_handle h, int B, int H, int W)
{
    LWS_CHECK_ARG(h, "lws_reserve: null handle");
    int rc = check_size(h, B, H, W);
    if (rc) return rc;
    LWS_CHECK_DEVICE(h, "lws_reserve");
    if (h->opt.side_streams != 0) {      // (single-stream plans never fork)
        rc = ensure_streams(h);
        if (rc) return rc;
    }
    return ensure_ws(h, ws_layout(h, B, H, W).total_all);
}

int lws_conv3d_stack(lws_handle h, int stage, const float *cost_in, float *cost_out, int B, int D, int hh, int ww,
                     void *stream)
{
    LWS_CHECK_ARG(h && cost_in && cost_out && cost_in != cost_out, "conv3d_stack: bad pointer");
    LWS_CHECK_ARG(stage >= 0 && stage < 3, "conv3d_stack: stage must be 0..2 (got %d)", stage);
    LWS_CHECK_ARG(B >= 1 && D >= 1 && hh >= 1 && ww >= 1, "conv3d_stack: bad shape");
    const size_t act = ((size_t)B * D * hh * ww * h->stage[stage].c3 + 63) & ~(size_t)63;
    const int rc = begin_call(h, "lws_conv3d_stack", false, "conv3d_stack: lws_finalize has not been called", 2 * act);
    if (rc) return rc;
    return conv3d_stack(h, stage, cost_in, cost_out, h->ws, h->ws + act, B, D, hh, ww, (hipStream_t)stream);
}

int lws_disparity_stages(lws_handle h, const float *const featsL[3], const float *const featsR[3], int B, int H,
                         int W, float *const pred_out[3], void *stream)
{
    LWS_CHECK_ARG(h && featsL && featsR && pred_out, "disparity_stages: null pointer");
    for (int s = 0; s < 3; ++s)
        LWS_CHECK_ARG(featsL[s] && featsR[s] && pred_out[s], "disparity_stages: null tensor for stage %d", s);
    int rc = check_size(h, B, H, W);
    if (rc) return rc;
    const WsLayout L = ws_layout(h, B, H, W);
    rc = begin_call(h, "lws_disparity_stages", false, "disparity_stages: lws_finalize has not been called", L.total);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    StageMap map[3] = {{pred_out[0]}, {pred_out[1]}, {pred_out[2]}};
    for (int s = 0; s < 3; ++s) {
        // only stage 2's map may wait for its consumer (stage 3's warp kernel writes it out): the caller reads all three
        const bool defer = defers(h, s, B, H, W, s == 1);
        const StageDims d = stage_dims(h, s, H, W);
        bool fused;
        rc = stage_volume(h, s, d, featsL[s], featsR[s], B, H, W, map, L, st, defer, fused);
        if (rc) return rc;
        rc = stage_map(h, s, d, B, H, W, map, L, st, defer, fused);
        if (rc) return rc;
    }
    return LWS_OK;
}

int lws_feature_extraction(lws_handle h, const float *img, int N, int H, int W, float *f8, float *f4, float *f2,
                           void *stream)
{
    LWS_CHECK_ARG(h && img && f8 && f4 && f2, "feature_extraction: null pointer");
    LWS_CHECK_ARG(N >= 1 && size_ok(H, W),
                  "feature_extraction: unsupported size N=%d %dx%d (ceil(H/2), ceil(W/2) divisible by 4)", N, H, W);
    // workspace is planned per pair: N images = ceil(N/2) pairs
    const WsLayout L = ws_layout(h, (N + 1) / 2, H, W);
    int rc = begin_call(h, "lws_feature_extraction", true,
                        "feature_extraction: the 2D network tensors were not all set before lws_finalize", L.total_all);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = feature_head(h, img, nullptr, N, 0, H, W, L, f8, st);
    if (rc) return rc;
    return feature_tail(h, N, H, W, L, f8, f4, f2, st, nullptr, 3);
}

int lws_refine(lws_handle h, const float *left, const float *pred3, int B, int H, int W, float *pred4, void *stream)
{
    LWS_CHECK_ARG(h && left && pred3 && pred4, "refine: null pointer");
    LWS_CHECK_ARG(B >= 1 && H > 0 && W > 0, "refine: unsupported size B=%d %dx%d", B, H, W);
    const WsLayout L = ws_layout(h, B, H, W);
    int rc = begin_call(h, "lws_refine", true, "refine: the 2D network tensors were not all set before lws_finalize",
                        L.total_all);
    if (rc) return rc;
    rc = refine_left(h, left, B, H, W, L, (hipStream_t)stream);
    if (rc) return rc;
    const StageMap p3{const_cast<float *>(pred3), true};      // (a written map is only read)
    return refine_rest(h, p3, B, H, W, L, pred4, (hipStream_t)stream);
}

}  // extern "C"

// What lws_forward_conf adds to the forward: conf[s] / sigma[s] (either may be null) receive stage s's confidence and sigma maps
struct ConfOut {
    float *const *conf;
    float *const *sigma;
};

// LWSNet.forward on a handle (lws_forward; arguments checked by the caller).  co != nullptr (lws_forward_conf): the plan that
// keeps every stage's filtered cost -- no stage defers its map and no last Conv3D layer fuses the soft-argmin (low = nullptr
// in conv3d_stack), so stage_map runs the soft-argmin from L.cost_out -- plus one k_softargmin_conf launch per stage.
static int run_forward(lws_ctx *h, const char *what, const float *left, const float *right, int B, int H, int W,
                       float *const pred_out[4], const ConfOut *co, hipStream_t st)
{
    const WsLayout L = ws_layout(h, B, H, W);
    int rc = begin_call(h, what, true, "forward: set_state_dict/lws_finalize must be called with the full state dict first",
                        L.total_all);
    if (rc) return rc;
    // Under hipGraph capture (tools/graph_pipeline.py; lws_reserve first, so that nothing allocates) the forks must be capture-
    // time records -- hipEventRecord on the capturing stream, which is what pulls the side stream into the graph; an event bound
    // to a kernel's completion signal is not one -- and nothing is profiled (timing events cannot be read back from a graph).
    bool capturing = false;
    if (st != nullptr) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        LWS_HIP(hipStreamIsCapturing(st, &cs));
        capturing = cs != hipStreamCaptureStatusNone;
    }
    // profiler sampling (lws_profile_sample): only every n-th forward call records events
    struct MaskGuard {
        lws_ctx *h;
        ~MaskGuard() { h->prof_mask = h->prof_mask_cfg; }
    } mask_guard{h};
    h->prof_mask = (!capturing && (h->prof_every <= 1 || h->prof_calls++ % (unsigned)h->prof_every == 0)) ? h->prof_mask_cfg : 0u;
    // Two independent branches run on the handle-owned side stream (speed only): the tail of the feature extractor and
    // refinement1_left, which depends on the left image only.  Option "side_streams" = 0 keeps everything on the caller's
    // stream: no forks, joins or event bubbles -- the plan lws_pool uses, where the kernels of OTHER forwards fill the CUs.
    // The plan (what was measured against what: profiles/NOTES.md, "launch plan of lws_forward"):
    //   caller's stream: feature head -> stage 1 -> stage 2 -> stage 3 -> refinement1_disp, refinement2
    //   fork 1, behind the feature head:                    conv5 (-> the 1/4 map of stage 2)
    //   fork 2, behind stage 1's last middle Conv3D layer:  conv6 + classif1 (-> the 1/2 map of stage 3), refinement1_left
    //   joins: the 1/4 map before stage 2, the 1/2 map before stage 3, refinement1_left before the refinement (host_join:
    //   at batch 1 the host resolves them, option "host_joins").
    // refinement1_left is HBM-bound work beside stages 2 and 3, whose MFMA kernels keep their weights in registers and do not
    // mind; beside stage 1 it would slow k_conv3d_mid16, which streams its weights from L2.
    const bool multi = h->opt.side_streams != 0;
    if (multi) {
        rc = ensure_streams(h);
        if (rc) return rc;
    }
    hipStream_t side = multi ? h->side : st;
    const bool ext = multi && !capturing;       // forks ride on their producer kernel's completion signal (StopArm)
    // automatic: batch 1 only -- from batch 2 up a queued wait is under 0.3 % of the step and blocking the caller buys nothing --
    // and only when this thread's previous forward ran on this same handle (one handle, one stream: the host has nothing else
    // to issue while it waits; rotating handles measured 2,374 against 2,612 pairs/s with the host held at the joins)
    const bool same_handle = tl_last_forward == h;
    tl_last_forward = h;
    bool hj = !capturing && (h->opt.host_joins >= 0 ? h->opt.host_joins != 0 : B == 1 && same_handle);
    float *f8 = h->ws + L.fe_f8, *f4 = h->ws + L.fe_f4, *f2 = h->ws + L.fe_f2;
    rc = feature_head(h, left, right, B, B, H, W, L, f8, st, Fork{multi ? h->ev_feat[0] : nullptr, 0, ext});   // models.py:110-111
    if (rc) return rc;
    const size_t n2 = (size_t)B * 8 * half_up(H) * half_up(W), n4 = n2 / 2, n8 = n2 / 8;   // 8 / 16 / 16 channels
    const float *fl[3] = {f8, f4, f2};
    const float *fr[3] = {f8 + n8, f4 + n4, f2 + n2};
    if (multi) {
        LWS_HIP(hipStreamWaitEvent(side, h->ev_feat[0], 0));
        rc = delay_side(h, LWS_DELAY_F4, side);
        if (rc) return rc;
    }
    rc = feature_tail(h, 2 * B, H, W, L, f8, f4, f2, side, multi ? h->ev_feat : nullptr, 1);          // conv5 -> f4
    if (rc) return rc;
    // where the second fork sits: option "fork2_after" (k = behind stage 1's k-th middle layer, 0 = behind its last layer,
    // -1 = automatic: the last middle layer, which leaves every k_conv3d_mid16 launch undisturbed)
    const int L3 = h->cfg.layers_3d;
    int fork2 = h->opt.fork2_after;
    if (fork2 < 0) fork2 = L3;
    if (fork2 > L3) fork2 = 0;
    // stage 3's map may wait for the refinement when its first block computes the 1 -> 32 convolution itself
    const bool ref_evaluates = (h->opt.fuse_first & 1) && ref_first_dws_can_fuse(h->net2d.r1[1][0], 1);
    StageMap map[3] = {{pred_out[0]}, {pred_out[1]}, {pred_out[2]}};
    for (int s = 0; s < 3; ++s) {                                                                   // :115-156
        if (multi && s > 0) {                                                     // joins: f4 before stage 2, f2 before stage 3
            rc = host_join(h, s - 1, h->ev_feat[s], st, hj);
            if (rc) return rc;
        }
        const bool defer = co == nullptr && defers(h, s, B, H, W, s < 2 || ref_evaluates);
        const StageDims d = stage_dims(h, s, H, W);
        bool fused;
        rc = stage_volume(h, s, d, fl[s], fr[s], B, H, W, map, L, st, defer, fused,
                          Fork{multi && s == 0 ? h->ev_fork2 : nullptr, fork2, ext}, co != nullptr);
        if (rc) return rc;
        if (s == 0) {
            // fork 2: the side branch starts once the event is complete (bound or recorded by conv3d_stack)
            if (multi) {
                LWS_HIP(hipStreamWaitEvent(side, h->ev_fork2, 0));
                rc = delay_side(h, LWS_DELAY_F2, side);
                if (rc) return rc;
            }
            rc = feature_tail(h, 2 * B, H, W, L, f8, f4, f2, side, multi ? h->ev_feat : nullptr, 2);  // conv6, classif1 -> f2
            if (rc) return rc;
            if (multi) {
                rc = delay_side(h, LWS_DELAY_LEFT, side);
                if (rc) return rc;
            }
            rc = refine_left(h, left, B, H, W, L, side);                                               // models.py:158
            if (rc) return rc;
            if (multi) LWS_HIP(hipEventRecord(h->ev_join, side));
        }
        rc = stage_map(h, s, d, B, H, W, map, L, st, defer, fused);
        if (rc) return rc;
        float *conf = co != nullptr && co->conf != nullptr ? co->conf[s] : nullptr;
        float *sigma = co != nullptr && co->sigma != nullptr ? co->sigma[s] : nullptr;
        if (conf != nullptr || sigma != nullptr) {
            // Lifetime of the filtered cost: L.cost_out is ONE buffer for the three stages (ws_layout), written by this stage's
            // last Conv3D layer and overwritten by the next stage's.  Both, and this launch between them, are on the chain
            // stream st, and the side stream's branches (feature tail, refinement1_left) never touch it.
            ProfScope p(h, LWS_KC_CONFIDENCE, st);
            rc = launch_softargmin_conf(h->ws + L.cost_out, nullptr, nullptr, nullptr, conf, sigma, B, d.D, d.hh, d.ww, H, W,
                                        d.start, st, ioff_of(h));
            if (rc) return rc;
        }
    }
    if (multi) {
        rc = host_join(h, 2, h->ev_join, st, hj);
        if (rc) return rc;
    }
    return refine_rest(h, map[2], B, H, W, L, pred_out[3], st);                                        // :159-162
}

extern "C" {

int lws_forward(lws_handle h, const float *left, const float *right, int B, int H, int W, float *const pred_out[4],
                void *stream)
{
    LWS_CHECK_ARG(h && left && right && pred_out, "forward: null pointer");
    for (int s = 0; s < 4; ++s) LWS_CHECK_ARG(pred_out[s], "forward: null output for stage %d", s + 1);
    const int rc = check_size(h, B, H, W);
    if (rc) return rc;
    return run_forward(h, "lws_forward", left, right, B, H, W, pred_out, nullptr, (hipStream_t)stream);
}

int lws_forward_conf(lws_handle h, const float *left, const float *right, int B, int H, int W, float *const pred_out[4],
                     float *const conf_out[3], float *const sigma_out[3], void *stream)
{
    LWS_CHECK_ARG(h && left && right && pred_out, "forward_conf: null pointer");
    for (int s = 0; s < 4; ++s) LWS_CHECK_ARG(pred_out[s], "forward_conf: null output for stage %d", s + 1);
    LWS_CHECK_ARG(B <= 65535, "forward_conf: batch %d above 65535", B);
    const int rc = check_size(h, B, H, W);
    if (rc) return rc;
    const ConfOut co{conf_out, sigma_out};
    return run_forward(h, "lws_forward_conf", left, right, B, H, W, pred_out, &co, (hipStream_t)stream);
}

}  // extern "C"
