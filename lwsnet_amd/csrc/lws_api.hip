// C ABI of the library (include/lwsnet_hip.h): the error string, handle life cycle, options, profiler and clock read-out,
// and the stateless per-kernel entry points.  State dict -> device slab: lws_params.hip; workspace and the launch plan of
// lws_forward: lws_forward.hip.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "lws_common.h"

namespace lws {

static thread_local char g_err[512] = "";
thread_local hipEvent_t tl_stop_event = nullptr;

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static constexpr int kClockWgs = 64;      // workgroups of a stamped k_conv3d_mid16 launch that leave their clocks

// Every entry point that touches the GPU through a handle requires the calling thread's current HIP device to be the
// handle's (recorded by lws_create, or set with lws_set_option("device")): its parameter slab, workspace, streams and
// events live there, and a launch from another device would run on foreign pointers.  Checked, never switched: a C
// library that silently changes the caller's current device is worse than one that refuses.
int check_device(const lws_ctx *h, const char *what)
{
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) {
        (void)hipGetLastError();
        cur = -1;
    }
    if (cur != h->device) {
        set_error("%s: the handle belongs to HIP device %d but the calling thread's current device is %d "
                  "(hipSetDevice(%d) first; -1 = no device)", what, h->device, cur, h->device);
        return LWS_ERR_INVALID;
    }
    return LWS_OK;
}

// copies the per-handle options into the per-layer structs the launchers read
void apply_options(lws_ctx *h)
{
    for (int i = 0; i < 3; ++i) {
        h->stage[i].mid16_split = (h->opt.split_bf16 & 1) != 0;
        h->stage[i].mid8_split = (h->opt.split_bf16 & 2) != 0;
        h->stage[i].mid8_balance = h->mid8_balance;
        h->stage[i].cu_count = h->cu_count;
    }
    h->net2d.r2_first.form = (h->opt.split_bf16 & 4) ? 1 : 0;
}

}  // namespace lws

using namespace lws;

extern "C" {

int lws_abi_version(void) { return LWS_ABI_VERSION; }

const char *lws_last_error(void) { return g_err; }

int lws_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int lws_create(const lws_config *cfg, lws_handle *out)
{
    LWS_CHECK_ARG(cfg != nullptr && out != nullptr, "lws_create: null argument");
    LWS_CHECK_ARG(cfg->layers_3d >= 1 && cfg->layers_3d <= 16, "layers_3d must be in 1..16 (got %d)", cfg->layers_3d);
    LWS_CHECK_ARG(cfg->maxdisplist[0] >= 1 && cfg->maxdisplist[0] <= 64, "maxdisplist[0] must be in 1..64 (got %d)",
                  cfg->maxdisplist[0]);
    for (int i = 1; i < 3; ++i)
        LWS_CHECK_ARG(cfg->maxdisplist[i] >= 1 && 2 * cfg->maxdisplist[i] - 1 <= 64,
                      "maxdisplist[%d] must be in 1..32 (got %d)", i, cfg->maxdisplist[i]);
    for (int i = 0; i < 3; ++i) {
        const int c3 = cfg->channels_3d * cfg->growth_rate[i];
        LWS_CHECK_ARG(c3 == 8 || c3 == 16 || c3 == 32,
                      "stage %d: channels_3d*growth_rate = %d is not supported by the gfx950 kernels (8, 16, 32)", i, c3);
    }
    LWS_CHECK_ARG(cfg->feature_fp16 == 0 || cfg->feature_fp16 == 1, "feature_fp16 must be 0 or 1 (got %d)", cfg->feature_fp16);
    LWS_CHECK_ARG(cfg->interp_align_mode == 0 || cfg->interp_align_mode == 1, "interp_align_mode must be 0 or 1 (got %d)",
                  cfg->interp_align_mode);
    lws_ctx *h = new (std::nothrow) lws_ctx();
    if (!h) {
        set_error("out of host memory");
        return LWS_ERR_NOMEM;
    }
    h->cfg = *cfg;
    h->spec = build_spec(*cfg);
    for (int i = 0; i < 3; ++i) h->stage[i].c3 = cfg->channels_3d * cfg->growth_rate[i];
    if (hipGetDevice(&h->device) != hipSuccess) h->device = -1;   // no GPU: host-side calls still work
    (void)hipGetLastError();
    *out = h;
    return LWS_OK;
}

static int *option_slot(lws_ctx *h, const char *name)
{
    struct { const char *name; int *slot; } tab[] = {{"fuse_first", &h->opt.fuse_first},
                                                     {"defer_upsample", &h->opt.defer_upsample},
                                                     {"side_streams", &h->opt.side_streams},
                                                     {"split_bf16", &h->opt.split_bf16},
                                                     {"ref_chunk_mb", &h->opt.ref_chunk_mb},
                                                     {"ref_pipe", &h->opt.ref_pipe},
                                                     {"warp_form", &h->opt.warp_form},
                                                     {"fuse_last1", &h->opt.fuse_last1},
                                                     {"fork2_after", &h->opt.fork2_after},
                                                     {"fuse_ref_last", &h->opt.fuse_ref_last},
                                                     {"host_joins", &h->opt.host_joins},
                                                     {"host_join_budget_us", &h->opt.host_join_budget_us},
                                                     {"device", &h->device}};
    for (auto &e : tab)
        if (strcmp(e.name, name) == 0) return e.slot;
    return nullptr;
}

int lws_set_option(lws_handle h, const char *name, int value)
{
    LWS_CHECK_ARG(h && name, "lws_set_option: null argument");
    int *slot = option_slot(h, name);
    LWS_CHECK_ARG(slot != nullptr, "lws_set_option: unknown option '%s'", name);
    if (strcmp(name, "split_bf16") == 0)
        // the opt-in numerics mode: a bit per MFMA convolution that has a split-bf16 form (NOT bit-exact); 7 = all of them
        LWS_CHECK_ARG(value >= 0 && value <= 7, "lws_set_option: split_bf16 is a bit mask in 0..7 (got %d)", value);
    else if (strcmp(name, "fuse_first") == 0)
        LWS_CHECK_ARG(value >= 0 && value <= 3, "lws_set_option: fuse_first is a bit mask in 0..3 (got %d)", value);
    else if (strcmp(name, "ref_pipe") == 0 || strcmp(name, "fuse_ref_last") == 0 || strcmp(name, "host_joins") == 0)
        LWS_CHECK_ARG(value >= -1 && value <= 1, "lws_set_option: %s is out of range (got %d)", name, value);
    else if (strcmp(name, "host_join_budget_us") == 0)
        LWS_CHECK_ARG(value >= 0 && value <= 1000000, "lws_set_option: host_join_budget_us must be in 0..1000000 (got %d)", value);
    else if (strcmp(name, "ref_chunk_mb") == 0)
        LWS_CHECK_ARG(value >= 0 && value <= 4096, "lws_set_option: ref_chunk_mb must be in 0..4096 (got %d)", value);
    else if (strcmp(name, "device") == 0) {
        LWS_CHECK_ARG(value >= 0, "lws_set_option: device must be >= 0 (got %d)", value);
        LWS_CHECK_ARG(h->params == nullptr && h->ws == nullptr && h->side == nullptr,
                      "lws_set_option: the device of a handle can only be changed before lws_finalize / lws_reserve "
                      "have allocated on device %d", h->device);
    }
    else if (strcmp(name, "fork2_after") == 0)
        LWS_CHECK_ARG(value >= -1 && value <= 16, "lws_set_option: fork2_after must be in -1..16 (got %d)", value);
    else
        LWS_CHECK_ARG(value == 0 || value == 1, "lws_set_option: %s must be 0 or 1 (got %d)", name, value);
    *slot = value;
    apply_options(h);
    return LWS_OK;
}

int lws_get_option(lws_handle h, const char *name, int *value)
{
    LWS_CHECK_ARG(h && name && value, "lws_get_option: null argument");
    int *slot = option_slot(h, name);
    LWS_CHECK_ARG(slot != nullptr, "lws_get_option: unknown option '%s'", name);
    *value = *slot;
    return LWS_OK;
}

int lws_profile_enable(lws_handle h, int class_mask)
{
    LWS_CHECK_ARG(h, "lws_profile_enable: null handle");
    prof_clear(h);
    h->prof_mask = h->prof_mask_cfg = (unsigned)class_mask;
    h->prof_every = 1;
    h->prof_calls = 0;
    return LWS_OK;
}

int lws_profile_sample(lws_handle h, int every_n)
{
    LWS_CHECK_ARG(h && every_n >= 1, "lws_profile_sample: every_n must be >= 1");
    h->prof_every = every_n;
    h->prof_calls = 0;
    return LWS_OK;
}

int lws_profile_read(lws_handle h, double *total_ms, int64_t *launches)
{
    LWS_CHECK_ARG(h && total_ms && launches, "lws_profile_read: null argument");
    LWS_CHECK_DEVICE(h, "lws_profile_read");
    for (int i = 0; i < LWS_KC_COUNT; ++i) {
        total_ms[i] = 0.0;
        launches[i] = 0;
    }
    for (lws_prof_rec &r : h->prof) {
        LWS_HIP(hipEventSynchronize(r.t1));
        float ms = 0.f;
        LWS_HIP(hipEventElapsedTime(&ms, r.t0, r.t1));
        total_ms[r.kc] += ms;
        launches[r.kc] += 1;
    }
    return LWS_OK;
}

int lws_profile_read_class(lws_handle h, int kernel_class, float *ms_out, int capacity, int *count)
{
    LWS_CHECK_ARG(h && count && (ms_out || capacity == 0) && capacity >= 0, "lws_profile_read_class: bad argument");
    LWS_CHECK_ARG(kernel_class >= 0 && kernel_class < LWS_KC_COUNT, "lws_profile_read_class: unknown kernel class %d", kernel_class);
    LWS_CHECK_DEVICE(h, "lws_profile_read_class");
    int n = 0;
    for (lws_prof_rec &r : h->prof) {
        if (r.kc != kernel_class) continue;
        if (n < capacity) {
            LWS_HIP(hipEventSynchronize(r.t1));
            float ms = 0.f;
            LWS_HIP(hipEventElapsedTime(&ms, r.t0, r.t1));
            ms_out[n] = ms;
        }
        ++n;
    }
    *count = n;
    return LWS_OK;
}

int lws_join_stats(lws_handle h, int64_t *out, int reset)
{
    LWS_CHECK_ARG(h, "lws_join_stats: null handle");
    for (int i = 0; i < 3 && out != nullptr; ++i) {
        const lws_join_stat &j = h->join_stat[i];
        out[4 * i] = j.host;
        out[4 * i + 1] = j.queued;
        out[4 * i + 2] = j.wait_ns;
        out[4 * i + 3] = j.max_ns;
    }
    if (reset)
        for (lws_join_stat &j : h->join_stat) j = lws_join_stat();
    return LWS_OK;
}

int lws_clock_stamp(lws_handle h, int enable)
{
    LWS_CHECK_ARG(h, "lws_clock_stamp: null handle");
    LWS_CHECK_DEVICE(h, "lws_clock_stamp");
    if (enable) {
        if (h->stage[0].c3 == 8) {
            set_error("lws_clock_stamp: stage 1 of this model has C3 = 8: no k_conv3d_mid16 launch to stamp");
            return LWS_ERR_STATE;
        }
        if (!h->clk_buf) LWS_HIP(hipMalloc(&h->clk_buf, kClockWgs * 4 * sizeof(unsigned long long)));
        LWS_HIP(hipMemset(h->clk_buf, 0, kClockWgs * 4 * sizeof(unsigned long long)));
    }
    h->stage[0].clk = enable ? h->clk_buf : nullptr;
    return LWS_OK;
}

int lws_clock_read(lws_handle h, double *ghz)
{
    LWS_CHECK_ARG(h && ghz, "lws_clock_read: null argument");
    LWS_CHECK_DEVICE(h, "lws_clock_read");
    if (!h->clk_buf) {
        set_error("lws_clock_read: lws_clock_stamp(h, 1) was never called");
        return LWS_ERR_STATE;
    }
    unsigned long long host[kClockWgs * 4];
    LWS_HIP(hipDeviceSynchronize());
    LWS_HIP(hipMemcpy(host, h->clk_buf, sizeof(host), hipMemcpyDeviceToHost));
    std::vector<double> v;
    for (int i = 0; i < kClockWgs; ++i) {
        const unsigned long long c0 = host[4 * i], r0 = host[4 * i + 1], c1 = host[4 * i + 2], r1 = host[4 * i + 3];
        if (r1 > r0 && c1 > c0) v.push_back((double)(c1 - c0) / (double)(r1 - r0) * 0.1);      // shader cycles per 10 ns tick -> GHz
    }
    if (v.empty()) {
        set_error("lws_clock_read: no stamped k_conv3d_mid16 launch since lws_clock_stamp(h, 1)");
        return LWS_ERR_STATE;
    }
    std::sort(v.begin(), v.end());
    *ghz = v[v.size() / 2];
    return LWS_OK;
}

int lws_debug_fill_workspace(lws_handle h, uint32_t word, void *stream)
{
    LWS_CHECK_ARG(h, "lws_debug_fill_workspace: null handle");
    LWS_CHECK_DEVICE(h, "lws_debug_fill_workspace");
    if (!h->ws || h->ws_bytes == 0) {
        set_error("lws_debug_fill_workspace: the handle has no workspace yet (lws_reserve first)");
        return LWS_ERR_STATE;
    }
    // (the slab is a whole number of floats: ensure_ws)
    LWS_HIP(hipMemsetD32Async((hipDeviceptr_t)h->ws, (int)word, h->ws_bytes / sizeof(uint32_t), (hipStream_t)stream));
    return LWS_OK;
}

int lws_debug_delay_side(lws_handle h, int segments, int microseconds)
{
    LWS_CHECK_ARG(h, "lws_debug_delay_side: null handle");
    LWS_CHECK_ARG(segments >= 0 && (segments & ~LWS_DELAY_ALL) == 0, "lws_debug_delay_side: unknown segment bits 0x%x (known: 0x%x)",
                  segments, LWS_DELAY_ALL);
    LWS_CHECK_ARG(microseconds >= 0 && microseconds <= 250000, "lws_debug_delay_side: microseconds must be in 0..250000 (got %d)",
                  microseconds);
    const bool on = segments != 0 && microseconds != 0;
    h->opt.delay_segments = on ? segments : 0;
    h->opt.delay_us = on ? microseconds : 0;
    return LWS_OK;
}

const char *lws_kernel_class_name(int kc)
{
    static const char *names[LWS_KC_COUNT] = {"volume_l1_shift", "volume_l1_warp", "conv3d_first", "conv3d_mid16",
                                              "conv3d_mid8",     "conv3d_last",    "softargmin",   "upsample_add",
                                              "feature_conv2d",  "ref_first",      "ref_dws",      "ref_conv64",
                                              "ref_last",        "softargmin_conf"};
    return kc >= 0 && kc < LWS_KC_COUNT ? names[kc] : "?";
}

int lws_destroy(lws_handle h)
{
    if (!h) return LWS_OK;
    prof_clear(h);
    for (hipEvent_t e : h->evt_pool) (void)hipEventDestroy(e);
    if (h->side) {
        (void)hipStreamSynchronize(h->side);
        (void)hipStreamDestroy(h->side);
        (void)hipEventDestroy(h->ev_fork);
        (void)hipEventDestroy(h->ev_join);
        for (int i = 0; i < 3; ++i) (void)hipEventDestroy(h->ev_feat[i]);
        if (h->ev_fork2) (void)hipEventDestroy(h->ev_fork2);
    }
    if (h->clk_buf) (void)hipFree(h->clk_buf);
    if (h->params && h->owns_params) (void)hipFree(h->params);
    if (h->ws) (void)hipFree(h->ws);
    delete h;
    return LWS_OK;
}

int lws_volume_l1_shift(const float *L, const float *R, float *cost, int B, int C, int h, int w, int D, void *stream)
{
    LWS_CHECK_ARG(L && R && cost, "volume_l1_shift: null pointer");
    LWS_CHECK_ARG(B >= 1 && h >= 1 && w >= 1 && D >= 1 && D <= 64, "volume_l1_shift: bad shape B=%d h=%d w=%d D=%d", B, h, w, D);
    // models.py:72: feat_l[:, :, :, i:] - feat_r[:, :, :, :-i] needs at least one column for every i < D
    LWS_CHECK_ARG(w >= D, "volume_l1_shift: width %d must be >= number of hypotheses %d", w, D);
    return launch_volume_l1_shift(L, R, cost, B, C, h, w, D, (hipStream_t)stream);
}

int lws_volume_l1_warp(const float *L, const float *R, const float *prev_disp, float *cost, float *wflow_out, int B,
                       int C, int h, int w, int H, int W, int m, void *stream)
{
    LWS_CHECK_ARG(L && R && prev_disp && cost, "volume_l1_warp: null pointer");
    LWS_CHECK_ARG(B >= 1 && h >= 1 && w >= 1 && H >= h && W >= w && m >= 1 && 2 * m - 1 <= 64,
                  "volume_l1_warp: bad shape B=%d h=%d w=%d H=%d W=%d m=%d", B, h, w, H, W, m);
    StageMap prev{const_cast<float *>(prev_disp), true};      // (a written map is only read)
    return launch_volume_l1_warp(L, R, prev, cost, wflow_out, B, C, h, w, H, W, m, (hipStream_t)stream);
}

int lws_softargmin(const float *cost, float *disp_low, int B, int D, int h, int w, float start, void *stream)
{
    LWS_CHECK_ARG(cost && disp_low, "softargmin: null pointer");
    LWS_CHECK_ARG(B >= 1 && D >= 1 && h >= 1 && w >= 1, "softargmin: bad shape");
    return launch_softargmin(cost, disp_low, B, D, h, w, start, (hipStream_t)stream);
}

int lws_upsample_add(const float *disp_low, const float *prev, float *out, int B, int h, int w, int H, int W,
                     void *stream)
{
    LWS_CHECK_ARG(disp_low && out, "upsample_add: null pointer");
    LWS_CHECK_ARG(B >= 1 && h >= 1 && w >= 1 && H >= h && W >= w, "upsample_add: bad shape");
    return launch_upsample_add(disp_low, prev, out, B, h, w, H, W, (hipStream_t)stream);
}

}  // extern "C"
