"""The HIP network kernels under the parameter families of tests/param_families.py (run with -m gpu on an MI355X): BatchNorm
weights of both signs, exact zeros, variances over two decades -- what a trained checkpoint brings and the seeded generator
(positive scales within a factor 3 of 1) never does.  It is the fold (fold_bn), every fmaf(x, s, t) + ReLU epilogue, the MFMA
weight packers and the bf16 split of the weights that meet something new here.

Per op and for the whole forward every comparison is bit for bit against the C oracle under the same state dict, and per op also
on the float64 floor (tests/float64_floor.py) wherever tests/test_param_families_cpu.py floor-gates the C restatement.  The
split-bf16 kernels have no C restatement: the floor, with the project's own factors, is their whole check.  One model per
(family, constructor, feature_fp16), references computed once and shared."""
import ctypes

import numpy as np
import pytest

import float64_floor as FF
import guarded as G
import param_families as PF
import plan_matrix as pm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FAMILY = pytest.mark.parametrize("family", PF.FAMILIES)
SIZES = ((15, 191), (24, 200), (16, 192))         # both sides odd; partial tiles at every scale; every resize ratio an integer
BATCHES = (1, 2, 3)

_MODELS, _REF = {}, {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def cu(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def host(t):
    return t.detach().cpu().numpy()


def ref(key, fn):
    """References are computed once and shared; never modified."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def new_model(dev, family, constructor=None, fp16=False):
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args
    args, sd = FF.state_dict(constructor, True, family)
    args = default_args(args.maxdisplist, args.layers_3d, args.channels_3d, args.growth_rate, feature_fp16=fp16)
    return LWSNet(args, device=dev).set_state_dict(sd).eval()


def model(dev, family, constructor=None, fp16=False):
    key = (family, constructor, fp16)
    if key not in _MODELS:
        _MODELS[key] = new_model(dev, family, constructor, fp16)
    return _MODELS[key]


def family_cases(op, extra=()):
    cases = [(fam, p) for fam in PF.FAMILIES for o, p in PF.CASES + list(extra) if o == op]
    return pytest.mark.parametrize("family,params", cases, ids=[f"{fam}-{FF.case_id(op, p)}" for fam, p in cases])


def hold(family, op, c, got, want):
    """`got` (name -> array) is the C oracle's `want` bit for bit and finite, and on the float64 floor where the case is floor-gated."""
    for name in want:
        assert np.isfinite(want[name]).all(), name
        G.assert_bits(got[name], want[name], f"{family} {op} {c.id} {name}")
    if PF.floor_gated(family, op, c.params):
        FF.check(c, got, show=print)


# ------------------------------------------------------------------ per op
@family_cases("conv3d_stack", PF.GPU_ONLY_CASES)
def test_conv3d_stack(dev, hip_lib, family, params):
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    stage, _, constructor, calibrated = params
    with FF.under_family(family):
        c = FF.case("conv3d_stack", params)
        sd = FF.state_dict(constructor, calibrated)[1]
    want = ref((family, "conv3d_stack", params), lambda: {"cost_out": C.conv3d_stack(c.inputs["cost"], sd, stage)})
    got = ops.conv3d_stack(model(dev, family, constructor)._h, stage, cu(c.inputs["cost"], dev))
    hold(family, "conv3d_stack", c, {"cost_out": host(got)}, want)


@family_cases("feature_extraction")
def test_feature_extraction(dev, hip_lib, family, params):
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    with FF.under_family(family):
        c = FF.case("feature_extraction", params)
        sd = FF.state_dict()[1]
    want = ref((family, "feature_extraction", params), lambda: dict(zip(("f8", "f4", "f2"), C.feature_extraction(c.inputs["img"], sd))))
    got = ops.feature_extraction(model(dev, family)._h, cu(c.inputs["img"], dev))
    hold(family, "feature_extraction", c, dict(zip(("f8", "f4", "f2"), (host(t) for t in got))), want)


@pytest.mark.parametrize("fuse_first", [0, 3])
@pytest.mark.parametrize("fuse_ref_last", [0, 1])
@family_cases("refine")
def test_refine(dev, hip_lib, family, params, fuse_ref_last, fuse_first):
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    with FF.under_family(family):
        c = FF.case("refine", params)
        sd = FF.state_dict()[1]
    want = ref((family, "refine", params), lambda: {"pred4": C.refine(c.inputs["left"], c.inputs["pred3"], sd)})
    m = model(dev, family)
    m.set_option("fuse_ref_last", fuse_ref_last)
    m.set_option("fuse_first", fuse_first)
    try:
        got = host(ops.refine(m._h, cu(c.inputs["left"], dev), cu(c.inputs["pred3"], dev)))
    finally:
        m.set_option("fuse_ref_last", pm.OPTION_DEFAULTS["fuse_ref_last"])
        m.set_option("fuse_first", pm.OPTION_DEFAULTS["fuse_first"])
    hold(family, "refine", c, {"pred4": got}, want)


def stage_features(B, H, W, seed):
    rng = np.random.default_rng(seed)
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    shapes = [(B, 16, h2 // 4, w2 // 4), (B, 16, h2 // 2, w2 // 2), (B, 8, h2, w2)]
    return [[rng.standard_normal(s).astype(np.float32) for s in shapes] for _ in "LR"]


@FAMILY
def test_disparity_stages(dev, hip_lib, family):
    """The three volume stages from seeded feature maps at 24 x 200 (25 / 50 / 100 columns: partial tiles at every scale): batch 2,
    and sample 0 alone -- the batch-1 plan, whose stage 1 ends in the fused last-layer + soft-argmin kernel -- with that fusion
    on and off."""
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    H, W = 24, 200
    fl, fr = stage_features(2, H, W, 2420)
    sd = FF.state_dict(family=family)[1]
    want = ref((family, "stages"), lambda: C.disparity_stages(fl, fr, H, W, sd))
    assert all(np.isfinite(w).all() for w in want)
    m = model(dev, family)
    got = ops.disparity_stages(m._h, [cu(a, dev) for a in fl], [cu(a, dev) for a in fr], H, W)
    for s in range(3):
        G.assert_bits(got[s], want[s], f"{family} batch 2 pred{s + 1}")
    for fuse_last1 in (1, 0):
        m.set_option("fuse_last1", fuse_last1)
        try:
            got = ops.disparity_stages(m._h, [cu(a[:1], dev) for a in fl], [cu(a[:1], dev) for a in fr], H, W)
        finally:
            m.set_option("fuse_last1", pm.OPTION_DEFAULTS["fuse_last1"])
        for s in range(3):
            G.assert_bits(got[s], want[s][:1], f"{family} batch 1 fuse_last1={fuse_last1} pred{s + 1}")


# ------------------------------------------------------------------ the forward
def pairs(H, W):
    from lwsnet_amd.synth import make_batch
    return ref(("pairs", H, W), lambda: make_batch(max(BATCHES), H, W, 3000 + 7 * H + W))


def oracle_forward(family, fp16, H, W):
    """The C oracle's four stage maps of pairs 0 .. 2, pair by pair (the forward is per sample), concatenated."""
    from oracle import c_oracle as C

    def make():
        left, right = pairs(H, W)
        sd = FF.state_dict(family=family)[1]
        each = [C.forward(left[i:i + 1], right[i:i + 1], sd, feature_fp16=fp16) for i in range(max(BATCHES))]
        maps = [np.concatenate([e[s] for e in each]) for s in range(4)]
        assert all(np.isfinite(a).all() for a in maps)
        return maps
    return ref(("forward", family, fp16, H, W), make)


def assert_forward(got, want, B, what):
    bad = []
    for s in range(4):
        g, w = host(got[s]), want[s][:B]
        n = int((g.view(np.uint32) != w.view(np.uint32)).sum())
        if n:
            bad.append(f"{what} stage {s + 1}: {n}/{w.size} elements differ, max abs {np.abs(g - w).max():.3e}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("plan", [{}, pm.ALL_OFF_PLAN, {"side_streams": 0}], ids=pm.plan_id)
@FAMILY
def test_forward_under_a_plan(dev, hip_lib, family, plan):
    """lws_forward against C.forward at an odd, a ragged and an even size, batches 1, 2, 3, on a handle that carries the plan."""
    m = new_model(dev, family)
    for k, v in plan.items():
        m.set_option(k, v)
        assert m.get_option(k) == v
    for H, W in SIZES:
        assert pm.size_ok(H, W)
        left, right = pairs(H, W)
        want = oracle_forward(family, False, H, W)
        for B in BATCHES:
            assert_forward(m(left[:B], right[:B]), want, B, f"{family} plan {pm.plan_id(plan)} {H}x{W} B={B}")


@FAMILY
def test_forward_conf_holds_the_forwards_bits(dev, hip_lib, family):
    """lws_forward_conf: its four stage maps are the oracle's (hence the forward's) bits; conf and sigma are finite, conf in [0, 1]."""
    m = model(dev, family)
    for H, W in SIZES:
        left, right = pairs(H, W)
        want = oracle_forward(family, False, H, W)
        for B in BATCHES:
            r = m.forward_conf(left[:B], right[:B])
            assert_forward(r.preds, want, B, f"{family} forward_conf {H}x{W} B={B}")
            assert all(torch.equal(a, b) for a, b in zip(r.preds, m(left[:B], right[:B])))
            for c, s in zip(r.conf, r.sigma):
                assert bool(torch.isfinite(c).all()) and bool(torch.isfinite(s).all()) and bool((c >= 0).all()) and bool((c <= 1.0 + 1e-6).all())


@FAMILY
def test_forward_with_fp16_features(dev, hip_lib, family):
    """A model built with feature_fp16 against C.forward(..., feature_fp16=True)."""
    m = model(dev, family, fp16=True)
    for H, W in SIZES:
        left, right = pairs(H, W)
        want = oracle_forward(family, True, H, W)
        for B in BATCHES:
            assert_forward(m(left[:B], right[:B]), want, B, f"{family} feature_fp16 {H}x{W} B={B}")
    assert not np.array_equal(oracle_forward(family, True, 24, 200)[0], oracle_forward(family, False, 24, 200)[0])


# ------------------------------------------------------------------ split-bf16
SPLIT = [(1, "conv3d_stack", (0, (1, 9, 17, 33), None, True)), (1, "conv3d_stack", (0, (1, 24, 8, 32), None, True)),
         (2, "conv3d_stack", (2, (1, 4, 64, 256), None, True)), (4, "refine", (1, 33, 47))]


@pytest.mark.parametrize("mask,op,params", SPLIT, ids=[FF.split_id(op, mask, p) for mask, op, p in SPLIT])
@FAMILY
def test_split_bf16_under_a_family(dev, hip_lib, family, mask, op, params):
    """k_conv3d_mid16x (mask 1), k_conv3d_mid8x (mask 2, 256 tiles, stage 2's weights) and k_ref_conv64x (mask 4) on shapes of
    FF.SPLIT_TEETH: on the float32 floor at FF.MAX_FACTOR / FF.MEAN_FACTOR (whole tensor, ring, carrier removed), not the exact
    kernel's bits, and the exact kernel's bits -- the C oracle's -- with the option off again."""
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    assert params in FF.SPLIT_TEETH[op]
    with FF.under_family(family):
        c = FF.case(op, params)
        sd = FF.state_dict()[1]
    m = model(dev, family)
    if op == "conv3d_stack":
        x = cu(c.inputs["cost"], dev)
        want = ref((family, op, params), lambda: {"cost_out": C.conv3d_stack(c.inputs["cost"], sd, params[0])})

        def run():
            return {"cost_out": host(ops.conv3d_stack(m._h, params[0], x))}
    else:
        left, pred3 = cu(c.inputs["left"], dev), cu(c.inputs["pred3"], dev)
        want = ref((family, op, params), lambda: {"pred4": C.refine(c.inputs["left"], c.inputs["pred3"], sd)})

        def run():
            return {"pred4": host(ops.refine(m._h, left, pred3))}

    assert m.get_option("split_bf16") == 0
    exact = run()
    m.set_option("split_bf16", mask)
    try:
        got = run()
    finally:
        m.set_option("split_bf16", 0)
    after = run()
    (name,) = want
    G.assert_bits(exact[name], want[name], f"{family} exact {c.id}")
    G.assert_bits(after[name], want[name], f"{family} {c.id}: the exact form did not come back")
    FF.check(c, got, show=print)
    assert not np.array_equal(got[name], exact[name]), "the option did not select the split kernel"


# ------------------------------------------------------------------ swapping families on one handle
def test_swapping_families_on_one_handle(dev, hip_lib):
    """set_state_dict(seeded), forward, set_state_dict(all), forward, set_state_dict(seeded), forward at 15 x 191, batch 2: each
    forward is the C oracle's bits under the state dict then loaded (no folded BatchNorm scale and no packed weight goes stale),
    the third is the first.  Clones as include/lwsnet_hip.h documents them (lws_clone: the source "must not be re-finalized while
    clones exist; a clone refuses lws_set_tensor / lws_finalize"): a clone made before the swap refuses lws_finalize and is
    destroyed before the source is re-finalized; a clone made after it carries the new parameters."""
    from lwsnet_amd import _lib, ops
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args
    H, W, B = 15, 191, 2
    left, right = pairs(H, W)
    want = {family: oracle_forward(family, False, H, W) for family in (None, "all")}
    m = LWSNet(default_args(), device=dev).eval()
    l, r = cu(left[:B], dev), cu(right[:B], dev)

    def clone_forward(what, family):
        c = ctypes.c_void_p()
        _lib.check(hip_lib.lws_clone(m._h, ctypes.byref(c)), "lws_clone")
        try:
            assert hip_lib.lws_finalize(c) == _lib.LWS_ERR_STATE
            assert_forward(ops.forward(c, l, r), want[family], B, what)
            torch.cuda.synchronize()
        finally:
            hip_lib.lws_destroy(c)

    runs = []
    for step, family in enumerate((None, "all", None)):
        m.set_state_dict(FF.state_dict(family=family)[1])
        preds = m(l, r)
        assert_forward(preds, want[family], B, f"step {step}: the forward under the {family or 'seeded'} state dict")
        runs.append([host(p) for p in preds])
        clone_forward(f"step {step}: a clone made under the {family or 'seeded'} state dict", family)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(runs[0], runs[2]))
    assert all((a != b).any() for a, b in zip(runs[0], runs[1]))


# ------------------------------------------------------------------ the memory contract once more
@pytest.mark.parametrize("word", G.FLOAT_WORDS, ids=G.word_id)
def test_forward_memory_contract_under_all(dev, hip_lib, word):
    """lws_forward under `all` at 15 x 191, batch 1, between poisoned flanks, into poisoned outputs, over a poisoned workspace
    (tests/guarded.py), under a quiet NaN, +FLT_MAX and -FLT_MAX: behind a negative BatchNorm scale it is the OTHER sign of
    +-FLT_MAX that survives the ReLU, which is why guarded.py carries both."""
    from lwsnet_amd import _lib
    H, W = 15, 191
    left, right = pairs(H, W)
    want = oracle_forward("all", False, H, W)
    m = new_model(dev, "all")
    g = G.Guard(dev, word)
    lt, rt = g.place(left[:1], name="left"), g.place(right[:1], name="right")
    outs = [g.empty((1, 1, H, W), name=f"pred{s + 1}") for s in range(4)]
    with torch.cuda.device(dev):
        _lib.check(hip_lib.lws_reserve(m._h, 1, H, W), "lws_reserve")
        torch.cuda.synchronize()
        _lib.check(hip_lib.lws_debug_fill_workspace(m._h, ctypes.c_uint32(word), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "lws_debug_fill_workspace")
        got = m(lt, rt, out=outs)
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, outs)), "the guarded tensors themselves must reach lws_forward"
    for s in range(4):
        G.assert_bits(outs[s], want[s][:1], f"all, {G.word_id(word)}: stage {s + 1}")
    g.check()
