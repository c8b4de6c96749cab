// From a state dict to the device slab: the state-dict contract (build_spec), lws_set_tensor, BatchNorm folding and
// lws_finalize, which packs every tensor for the kernel that reads it (the pack_* helpers live beside those kernels).
#include <math.h>
#include <string.h>

#include "lws_common.h"

namespace lws {

// ---- the state-dict contract (mirrors lwsnet_amd/weights.py:state_dict_spec) -------------------
typedef std::map<std::string, std::vector<int64_t>> Spec;

static void spec_bn(Spec &sp, const std::string &p, int c)
{
    for (const char *s : {".weight", ".bias", "._mean", "._variance"}) sp[p + s] = {c};
}

// The feature extractor in execution order.  Keys: weight feature_extraction.<name> + (bn ? ".0.weight" : ".weight"),
// BatchNorm(cout) feature_extraction.<name>.1; shape [cout][cin][3][3], transposed (tr) [cin][cout][3][3].
static const struct { const char *name; int cin, cout, stride, pad, dil; bool tr, bn, relu; } kFeLayers[12] = {
    {"dres0.0", 3, 4, 2, 2, 2, false, true, true},         {"dres0.2", 4, 8, 1, 4, 4, false, true, true},
    {"dres1.0", 8, 4, 1, 2, 2, false, true, true},         {"dres1.2", 4, 8, 1, 2, 2, false, true, false},
    {"dres2.conv1.0", 8, 16, 2, 1, 1, false, true, true},  {"dres2.conv2.0", 16, 16, 1, 1, 1, false, true, true},
    {"dres2.conv3.0", 16, 16, 2, 1, 1, false, true, true}, {"dres2.conv4.0", 16, 16, 1, 1, 1, false, true, true},
    {"dres2.conv5", 16, 16, 2, 1, 1, true, true, true},    {"dres2.conv6", 16, 8, 2, 1, 1, true, true, false},
    {"classif1.0", 8, 8, 1, 1, 1, false, true, true},      {"classif1.2", 8, 8, 1, 1, 1, false, false, false}};

static std::string fe_name(int i) { return std::string("feature_extraction.") + kFeLayers[i].name; }
static std::string fe_weight_key(int i) { return fe_name(i) + (kFeLayers[i].bn ? ".0.weight" : ".weight"); }

// Layer j of the Conv3D stack of stage i: BatchNorm3D <name>.0, Conv3D <name>.2.weight
static const char kVolumePost[] = "volume_postprocess.";
static std::string vp_name(int i, int j) { return kVolumePost + std::to_string(i) + "." + std::to_string(j); }

// Block k (1..4) of a refinement network: BatchNorm(32) -> ReLU -> depthwise 3x3 -> pointwise 32 -> 32
struct DwsKeys { std::string bn, dw, pw; };
static DwsKeys dws_keys(const std::string &net, int k)
{
    const std::string p = net + "." + std::to_string(k);
    return {p + ".0", p + ".2.weight", p + ".3.weight"};
}
static const char *const kRef1[2] = {"refinement1_left", "refinement1_disp"};

Spec build_spec(const lws_config &cfg)
{
    Spec sp;
    for (int i = 0; i < 12; ++i) {
        const auto &d = kFeLayers[i];
        sp[fe_weight_key(i)] = d.tr ? std::vector<int64_t>{d.cin, d.cout, 3, 3} : std::vector<int64_t>{d.cout, d.cin, 3, 3};
        if (d.bn) spec_bn(sp, fe_name(i) + ".1", d.cout);
    }
    for (int i = 0; i < 3; ++i) {
        const int c3 = cfg.channels_3d * cfg.growth_rate[i];
        for (int j = 0; j < cfg.layers_3d + 2; ++j) {
            const int ci = j == 0 ? 1 : c3, co = j == cfg.layers_3d + 1 ? 1 : c3;
            spec_bn(sp, vp_name(i, j) + ".0", ci);
            sp[vp_name(i, j) + ".2.weight"] = {co, ci, 3, 3, 3};
        }
    }
    for (const std::string net : {kRef1[0], kRef1[1], "refinement2"})
        for (int k = 1; k <= 4; ++k) {
            const DwsKeys d = dws_keys(net, k);
            spec_bn(sp, d.bn, 32);
            sp[d.dw] = {32, 1, 3, 3};
            sp[d.pw] = {32, 32, 1, 1};
        }
    sp[std::string(kRef1[0]) + ".0.weight"] = {32, 3, 3, 3};
    sp[std::string(kRef1[1]) + ".0.weight"] = {32, 1, 3, 3};
    spec_bn(sp, "refinement2.0.0", 64);
    sp["refinement2.0.2.weight"] = {32, 64, 3, 3};
    sp["refinement2.5.weight"] = {1, 32, 3, 3};
    return sp;
}

// Eval BatchNorm as y = fmaf(x, s, t): s = gamma / sqrt(var + eps), t = beta - mean*s, float32 steps
// (the same sequence as lwsnet_amd/weights.py:bn_scale_shift; this file is built with -ffp-contract=off).
static void fold_bn(const lws_ctx *h, const std::string &p, std::vector<float> &s, std::vector<float> &t)
{
    const std::vector<float> &g = h->host.at(p + ".weight"), &b = h->host.at(p + ".bias"),
                             &m = h->host.at(p + "._mean"), &v = h->host.at(p + "._variance");
    s.resize(g.size());
    t.resize(g.size());
    for (size_t i = 0; i < g.size(); ++i) {
        float sd = sqrtf(v[i] + 1e-5f);
        s[i] = g[i] / sd;
        float ms = m[i] * s[i];
        t[i] = b[i] - ms;
    }
}

// ---- the parameter slab -------------------------------------------------------------------------
// One host vector that becomes one device allocation.  Every entry starts on a 64-float boundary (zero padding between);
// the device address is unknown while the slab grows, so put() notes which pointer wants which offset and bind() sets
// them all once the slab is uploaded.  The pointers must stay where they are between the two.
struct SlabBuilder {
    std::vector<float> slab;
    std::vector<std::pair<float **, size_t>> refs;
    void align() { slab.resize((slab.size() + 63) & ~(size_t)63, 0.0f); }
    void put(const std::vector<float> &v, float *&dst)
    {
        align();
        refs.push_back({&dst, slab.size()});
        slab.insert(slab.end(), v.begin(), v.end());
    }
    void put_bn(const lws_ctx *h, const std::string &p, float *&s_dst, float *&t_dst)
    {
        std::vector<float> s, t;
        fold_bn(h, p, s, t);
        put(s, s_dst);
        put(t, t_dst);
    }
    void bind(float *base)
    {
        for (const auto &r : refs) *r.first = base + r.second;
    }
};

// The Conv3D stacks, per stage and layer: w, [w_mfma], bn_s, bn_t
static void pack_net3d(lws_ctx *h, SlabBuilder &sb)
{
    const int L = h->cfg.layers_3d + 2;
    for (int i = 0; i < 3; ++i) {
        const int c3 = h->stage[i].c3;
        h->stage[i].layers.assign(L, Conv3dLayer());      // (sized first: put() keeps addresses into it)
        for (int j = 0; j < L; ++j) {
            Conv3dLayer &l = h->stage[i].layers[j];
            l.cin = j == 0 ? 1 : c3;
            l.cout = j == L - 1 ? 1 : c3;
            const std::vector<float> &w = h->host.at(vp_name(i, j) + ".2.weight");
            if (j == 0) {
                sb.put(w, l.w);                                                 // [c3][27]
                std::vector<float> wf(c3 == 8 ? 9 * 64 : (size_t)(c3 / 16) * 7 * 64);      // + MFMA A fragments
                if (c3 == 8)
                    pack_first8_weights(w.data(), wf.data());
                else
                    pack_first16_weights(w.data(), c3, wf.data());
                sb.put(wf, l.w_mfma);
            } else if (j == L - 1) {
                std::vector<float> wt((size_t)27 * c3);                         // [27][c3]
                for (int ci = 0; ci < c3; ++ci)
                    for (int tap = 0; tap < 27; ++tap) wt[(size_t)tap * c3 + ci] = w[(size_t)ci * 27 + tap];
                sb.put(wt, l.w);
            } else {
                std::vector<float> wp(packed_mid_weight_floats(c3));
                pack_mid_weights(w.data(), c3, wp.data());
                sb.put(wp, l.w);
            }
            sb.put_bn(h, vp_name(i, j) + ".0", l.bn_s, l.bn_t);
        }
    }
}

static void pack_dws(const lws_ctx *h, SlabBuilder &sb, const DwsKeys &k, int dil, RefDws &r)
{
    r.dil = dil;
    sb.put_bn(h, k.bn, r.bn_s, r.bn_t);
    const std::vector<float> &dw = h->host.at(k.dw);      // [32][1][3][3]
    std::vector<float> dwt(9 * 32);
    for (int c = 0; c < 32; ++c)
        for (int tap = 0; tap < 9; ++tap) dwt[tap * 32 + c] = dw[c * 9 + tap];
    sb.put(dwt, r.dw);
    std::vector<float> pw(2 * 2 * 64 * 4);
    pack_conv2d_mfma(h->host.at(k.pw).data(), 32, 1, pw.data());   // [32][32][1][1]
    sb.put(pw, r.pw);
}

// The 2D networks: feature extractor (per layer w, [w_pair], [w_mfma], [bn_s, bn_t]), refinement1_left / _disp, refinement2
static void pack_net2d(lws_ctx *h, SlabBuilder &sb)
{
    Net2d &n = h->net2d;
    n = Net2d();
    for (int i = 0; i < 12; ++i) {
        const auto &d = kFeLayers[i];
        Conv2dLayer &l = n.fe[i];
        l.cin = d.cin; l.cout = d.cout; l.stride = d.stride; l.pad = d.pad; l.dil = d.dil;
        l.transposed = d.tr; l.relu = d.relu;
        // Conv2D [cout][cin][3][3] / Conv2DTranspose [cin][cout][3][3]  ->  [tap][wave][cin][cout/4]
        const std::vector<float> &w = h->host.at(fe_weight_key(i));
        const int cpt = d.cout / 4;
        std::vector<float> wt((size_t)9 * d.cin * d.cout);
        for (int co = 0; co < d.cout; ++co)
            for (int ci = 0; ci < d.cin; ++ci)
                for (int tap = 0; tap < 9; ++tap)
                    wt[(((size_t)tap * 4 + co / cpt) * d.cin + ci) * cpt + co % cpt] =
                        d.tr ? w[((size_t)ci * d.cout + co) * 9 + tap] : w[((size_t)co * d.cin + ci) * 9 + tap];
        sb.put(wt, l.w);
        const int G = l.pair_groups = conv2d_pair_groups(i);      // second copy in the group count the pair kernel uses
        if (G > 0) {                                  // (layers 0..7: none of them transposed)
            const int cpg = d.cout / G;
            std::vector<float> wq((size_t)9 * d.cin * d.cout);
            for (int co = 0; co < d.cout; ++co)
                for (int ci = 0; ci < d.cin; ++ci)
                    for (int tap = 0; tap < 9; ++tap)
                        wq[(((size_t)tap * G + co / cpg) * d.cin + ci) * cpg + co % cpg] = w[((size_t)co * d.cin + ci) * 9 + tap];
            sb.put(wq, l.w_pair);
        }
        if (i >= 4 && i <= 7) {                       // conv1..conv4: 16 output channels -> MFMA A fragments
            std::vector<float> wf((size_t)9 * 64 * (d.cin / 4));
            pack_pair_mfma(w.data(), d.cin, wf.data());
            sb.put(wf, l.w_mfma);
        }
        if (d.bn) sb.put_bn(h, fe_name(i) + ".1", l.bn_s, l.bn_t);
    }
    for (int k = 0; k < 2; ++k) {
        const int cin = k == 0 ? 3 : 1;
        const std::vector<float> &w = h->host.at(std::string(kRef1[k]) + ".0.weight");   // [32][cin][3][3]
        std::vector<float> wt(9 * cin * 32);
        for (int co = 0; co < 32; ++co)
            for (int ci = 0; ci < cin; ++ci)
                for (int tap = 0; tap < 9; ++tap) wt[(tap * cin + ci) * 32 + co] = w[(co * cin + ci) * 9 + tap];
        sb.put(wt, n.r1_first[k]);
        std::vector<float> wf(packed_first_mfma_floats(cin));
        pack_first_mfma(w.data(), cin, wf.data());
        sb.put(wf, n.r1_first_mfma[k]);
        for (int b = 0; b < 4; ++b) pack_dws(h, sb, dws_keys(kRef1[k], b + 1), 2 << b, n.r1[k][b]);   // dilation 2,4,8,16 (submodules.py:298)
    }
    {
        sb.put_bn(h, "refinement2.0.0", n.r2_first.bn_s, n.r2_first.bn_t);
        const std::vector<float> &w = h->host.at("refinement2.0.2.weight");   // [32][64][3][3]
        std::vector<float> wp(10 * 4 * 2 * 64 * 4, 0.0f);   // 9 taps + one all-zero tap (prefetch without bounds check)
        pack_conv2d_mfma(w.data(), 64, 9, wp.data());
        sb.put(wp, n.r2_first.w);
        std::vector<float> wx(packed_conv64x_floats(), 0.0f);
        pack_conv64_bf16x3(w.data(), wx.data());
        sb.put(wx, n.r2_first.wx);
    }
    for (int b = 0; b < 4; ++b) pack_dws(h, sb, dws_keys("refinement2", b + 1), 8 >> b, n.r2[b]);     // dilation 8,4,2,1 (submodules.py:316)
    {
        const std::vector<float> &w = h->host.at("refinement2.5.weight");   // [1][32][3][3]
        std::vector<float> wt(9 * 32);
        for (int ci = 0; ci < 32; ++ci)
            for (int tap = 0; tap < 9; ++tap) wt[tap * 32 + ci] = w[ci * 9 + tap];
        sb.put(wt, n.r2_last);
    }
}

}  // namespace lws

using namespace lws;

extern "C" {

int lws_set_tensor(lws_handle h, const char *key, const float *host, const int64_t *shape, int ndim)
{
    LWS_CHECK_ARG(h && key && host && shape && ndim >= 1 && ndim <= 5, "lws_set_tensor: bad argument");
    if (!h->owns_params) {
        set_error("lws_set_tensor: this handle is a clone and shares its source's parameters");
        return LWS_ERR_STATE;
    }
    auto it = h->spec.find(key);
    LWS_CHECK_ARG(it != h->spec.end(), "set_state_dict: unexpected key '%s'", key);
    std::vector<int64_t> shp(shape, shape + ndim);
    if (shp != it->second) {
        std::string want, got;
        for (int64_t d : it->second) want += std::to_string(d) + ",";
        for (int64_t d : shp) got += std::to_string(d) + ",";
        set_error("set_state_dict: shape mismatch for '%s': expected [%s] got [%s]", key, want.c_str(), got.c_str());
        return LWS_ERR_INVALID;
    }
    size_t n = 1;
    for (int64_t d : shp) n *= (size_t)d;
    h->host[key].assign(host, host + n);
    h->shapes[key] = shp;
    h->finalized = false;
    return LWS_OK;
}

int lws_finalize(lws_handle h)
{
    LWS_CHECK_ARG(h, "lws_finalize: null handle");
    if (!h->owns_params) {
        set_error("lws_finalize: this handle is a clone (lws_clone / lws_pool worker) and shares its source's parameters");
        return LWS_ERR_STATE;
    }
    LWS_CHECK_DEVICE(h, "lws_finalize");
    // every hot-path tensor must be present; the 2D networks are packed only when all of theirs are
    bool have_2d = true;
    for (const auto &kv : h->spec) {
        if (h->host.count(kv.first)) continue;
        if (kv.first.compare(0, strlen(kVolumePost), kVolumePost) == 0) {
            set_error("lws_finalize: state dict entry '%s' was never set", kv.first.c_str());
            return LWS_ERR_STATE;
        }
        have_2d = false;
    }
    // build one host slab, upload it, then point the layer structs into it
    h->finalized = false;
    h->have_2d = have_2d;
    SlabBuilder sb;
    pack_net3d(h, sb);
    if (have_2d) pack_net2d(h, sb);
    sb.align();
    if (h->params) LWS_HIP(hipFree(h->params));
    h->params = nullptr;
    LWS_HIP(hipMalloc(&h->params, sb.slab.size() * sizeof(float)));
    h->params_bytes = sb.slab.size() * sizeof(float);
    LWS_HIP(hipMemcpy(h->params, sb.slab.data(), h->params_bytes, hipMemcpyHostToDevice));
    sb.bind(h->params);
    {
        int ncu = 0;
        if (h->device >= 0 && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && ncu > 0)
            h->cu_count = ncu;
        (void)hipGetLastError();
    }
    apply_options(h);
    h->finalized = true;
    return LWS_OK;
}

}  // extern "C"
