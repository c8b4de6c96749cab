"""The HIP path of every network op against the literal restatement in float64, by the yardstick of the literal restatement's own
float32 run: the cases, references, helper and factors of tests/test_float64_floor_cpu.py (tests/float64_floor.py), run through
lwsnet_amd.ops instead of the C restatement, and the distribution gates of the end-to-end stage maps on the model's forward.
HIP equals the C restatement bit for bit, so a failure here where the CPU test passes means that a bit-exact test is missing at
that shape.  References are computed once per case and shared (FF.case); never modified.

Two things the per-op entry points cannot be given, both by their own contract: lws_volume_l1_shift rejects a map narrower than
the number of hypotheses (the (2, 8, 4, 3), D = 5 case: the rejection is asserted instead), and lws_volume_l1_warp /
lws_upsample_add carry no handle and so resize under align mode 0 only -- align mode 1 is reached through a model built with
interp_align_mode = 1: stage 1 of lws_disparity_stages per op (`align1_stage1`), the warps in the end-to-end gates below.

The split-bf16 kernels (option "split_bf16": k_conv3d_mid16x, k_conv3d_mid8x, k_ref_conv64x) are NOT the C restatement's bits, so
here the tolerance does all the work: FF.SPLIT_CASES under the same gate with the same factors (the mode claims the float32
chain's accuracy, so it gets the float32 chain's gate), what tests/test_float64_floor_cpu.py (part D) shows a kernel that loses one of its
2^-16-order terms would miss; then the bits across batch sizes, calls and refinement chunks, and the end-to-end distributions."""
import numpy as np
import pytest

import float64_floor as FF

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_MODELS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def cu(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def host(t):
    return t.detach().cpu().numpy()


def model(dev, constructor=None, calibrated=True, align=0, fp16=False):
    """One model per (constructor setting, statistics, align mode, feature_fp16), shared by the cases that need it."""
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args
    key = (constructor, calibrated, align, fp16)
    if key not in _MODELS:
        args, sd = FF.state_dict(constructor, calibrated)
        args = default_args(args.maxdisplist, args.layers_3d, args.channels_3d, args.growth_rate, feature_fp16=fp16, interp_align_mode=align)
        _MODELS[key] = LWSNet(args, device=dev).set_state_dict(sd).eval()
    return _MODELS[key]


def ids(family, keep=lambda p: True):
    cases = [p for p in FF.CASES[family] if keep(p)]
    return pytest.mark.parametrize("params", cases, ids=[FF.case_id(family, p) for p in cases])


# ------------------------------------------------------------------ per op
@ids("feature_extraction")
def test_feature_extraction(dev, hip_lib, params):
    from lwsnet_amd import ops
    c = FF.case("feature_extraction", params)
    got = ops.feature_extraction(model(dev)._h, cu(c.inputs["img"], dev))
    FF.check(c, dict(zip(("f8", "f4", "f2"), (host(t) for t in got))), show=print)


@pytest.mark.parametrize("H,W", [(9, 17), (33, 47)])
def test_sizes_the_reference_cannot_run_are_rejected(dev, hip_lib, H, W):
    """ceil(H/2) not divisible by 4: the literal restatement raises (tests/test_float64_floor_cpu.py), and so do both entry points."""
    from lwsnet_amd import ops
    m = model(dev)
    with pytest.raises(ValueError, match="divisible by 4"):
        ops.feature_extraction(m._h, torch.zeros((1, 3, H, W), device=dev))
    z = np.zeros((1, 3, H, 255), np.float32)            # wide enough for 24 hypotheses: only the height is at fault
    with pytest.raises(ValueError, match="divisible by 4"):
        m(z, z)


@pytest.mark.parametrize("fuse_first", [0, None], ids=["fuse_first=0", "fuse_first=default"])
@pytest.mark.parametrize("fuse_ref_last", [0, 1])
@ids("refine")
def test_refine(dev, hip_lib, params, fuse_ref_last, fuse_first):
    from lwsnet_amd import ops
    c = FF.case("refine", params)
    m = model(dev)
    default_ff = m.get_option("fuse_first")
    m.set_option("fuse_ref_last", fuse_ref_last)
    m.set_option("fuse_first", default_ff if fuse_first is None else fuse_first)
    try:
        got = host(ops.refine(m._h, cu(c.inputs["left"], dev), cu(c.inputs["pred3"], dev)))
    finally:
        m.set_option("fuse_ref_last", -1)
        m.set_option("fuse_first", default_ff)
    FF.check(c, {"pred4": got}, show=print)


@ids("conv3d_stack")
def test_conv3d_stack(dev, hip_lib, params):
    from lwsnet_amd import ops
    stage, _, constructor, calibrated = params
    c = FF.case("conv3d_stack", params)
    got = ops.conv3d_stack(model(dev, constructor, calibrated)._h, stage, cu(c.inputs["cost"], dev))
    FF.check(c, {"cost_out": host(got)}, show=print)


@ids("volume_l1_shift")
def test_volume_l1_shift(dev, hip_lib, params):
    from lwsnet_amd import ops
    shape, D = params
    c = FF.case("volume_l1_shift", params)
    L, R = cu(c.inputs["L"], dev), cu(c.inputs["R"], dev)
    if shape[3] < D:                                    # models.py:72 has no column left for hypothesis i >= w: rejected by contract
        with pytest.raises(ValueError, match="must be >= number of hypotheses"):
            ops.volume_l1_shift(L, R, D)
        return
    FF.check(c, {"cost": host(ops.volume_l1_shift(L, R, D))}, show=print)


@ids("volume_l1_warp", lambda p: p[0] == 0)
def test_volume_l1_warp(dev, hip_lib, params):
    from lwsnet_amd import ops
    c = FF.case("volume_l1_warp", params)
    cost, wflow = ops.volume_l1_warp(cu(c.inputs["L"], dev), cu(c.inputs["R"], dev), cu(c.inputs["prev"], dev), c.meta["m"], return_wflow=True)
    FF.check(c, {"wflow": host(wflow), "cost": host(cost)}, show=print)


@ids("softargmin")
def test_softargmin(dev, hip_lib, params):
    from lwsnet_amd import ops
    c = FF.case("softargmin", params)
    FF.check(c, {"low": host(ops.softargmin(cu(c.inputs["cost"], dev), c.meta["start"]))}, show=print)


@ids("upsample_add", lambda p: p[0] == 0)
def test_upsample_add(dev, hip_lib, params):
    from lwsnet_amd import ops
    c = FF.case("upsample_add", params)
    prev = cu(c.inputs["prev"], dev) if "prev" in c.inputs else None
    FF.check(c, {"up": host(ops.upsample_add(cu(c.inputs["low"], dev), prev, c.meta["H"], c.meta["W"]))}, show=print)


@pytest.mark.parametrize("family", ["fp16_stage1", "align1_stage1"])
def test_stage1_through_a_configured_model(dev, hip_lib, family):
    """Stage 1 of lws_disparity_stages on a model built with feature_fp16 (the kernel rounds the float32 features it is given; the
    literal restatement is fed the features numpy rounded) or with interp_align_mode = 1 (the upsample under the other reading)."""
    from lwsnet_amd import ops
    (params,) = FF.CASES[family]
    c = FF.case(family, params)
    m = model(dev, align=c.meta["align_mode"], fp16=c.meta["feature_fp16"])
    fl, fr = ([cu(a, dev) for a in side] for side in FF.stage1_features(c))
    FF.check(c, {"pred1": host(ops.disparity_stages(m._h, fl, fr, c.meta["H"], c.meta["W"])[0])}, show=print)


# ------------------------------------------------------------------ per op, split-bf16
def split_ids(family, keep=lambda mask, p: True):
    cases = [(mask, p) for mask, p in FF.SPLIT_CASES[family] if keep(mask, p)]
    return pytest.mark.parametrize("mask,params", cases, ids=[FF.split_id(family, mask, p) for mask, p in cases])


def with_split(m, mask, fn):
    """fn() under option split_bf16 = mask, the option restored whatever happens."""
    m.set_option("split_bf16", mask)
    try:
        return fn()
    finally:
        m.set_option("split_bf16", 0)


@split_ids("conv3d_stack")
def test_conv3d_stack_split(dev, hip_lib, mask, params):
    """k_conv3d_mid16x (mask 1, stage 0) and k_conv3d_mid8x (mask 2, stages 1 and 2, from 256 tiles per sample) on the float32
    floor at FF.MAX_FACTOR / FF.MEAN_FACTOR, whole tensor and ring; on the large maps the bits differ from the exact kernel's (the
    split kernel really ran); the 240-tile sample stays on the exact kernel (the C restatement's bits with the option on); the
    exact form comes back bit for bit."""
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    stage, shape, _, _ = params
    c = FF.case("conv3d_stack", params)
    m, x = model(dev), cu(c.inputs["cost"], dev)
    assert m.get_option("split_bf16") == 0
    exact = host(ops.conv3d_stack(m._h, stage, x))
    got = with_split(m, mask, lambda: host(ops.conv3d_stack(m._h, stage, x)))
    after = host(ops.conv3d_stack(m._h, stage, x))
    FF.check(c, {"cost_out": got}, show=print)
    assert np.array_equal(after.view(np.uint32), exact.view(np.uint32)), "the exact form did not come back"
    runs_split = mask == 1 or FF.mid8x_tiles(shape) >= FF.MID8X_MIN_TILES
    if not runs_split:
        assert np.array_equal(got.view(np.uint32), C.conv3d_stack(c.inputs["cost"], FF.state_dict()[1], stage).view(np.uint32))
    elif shape in FF.SPLIT_LARGE["conv3d_stack"]:
        assert not np.array_equal(got, exact), "the option did not select the split kernel"


@split_ids("refine")
def test_refine_split(dev, hip_lib, mask, params):
    """k_ref_conv64x (mask 4) on the float32 floor at FF.MAX_FACTOR / FF.MEAN_FACTOR: whole tensor, ring, and both again with the
    150-px carrier removed; on the maps larger than the dilation-8 footprint the bits differ from the exact kernel's; the exact
    form comes back bit for bit."""
    from lwsnet_amd import ops
    c = FF.case("refine", params)
    m, left, pred3 = model(dev), cu(c.inputs["left"], dev), cu(c.inputs["pred3"], dev)
    assert m.get_option("split_bf16") == 0
    exact = host(ops.refine(m._h, left, pred3))
    got = with_split(m, mask, lambda: host(ops.refine(m._h, left, pred3)))
    after = host(ops.refine(m._h, left, pred3))
    FF.check(c, {"pred4": got}, show=print)
    assert np.array_equal(after.view(np.uint32), exact.view(np.uint32)), "the exact form did not come back"
    if params in FF.SPLIT_LARGE["refine"]:
        assert not np.array_equal(got, exact), "the option did not select the split kernel"


@pytest.mark.parametrize("family,mask,params", [("conv3d_stack", 1, (0, (2, 9, 30, 70), None, True)), ("conv3d_stack", 2, (1, (2, 9, 41, 353), None, True)),
                                                ("conv3d_stack", 2, (2, (2, 9, 41, 353), None, True)), ("refine", 4, (3, 5, 70)), ("refine", 4, (2, 17, 15)),
                                                ("refine", 4, (2, 63, 65))],
                         ids=lambda v: FF.case_id("", v) if isinstance(v, tuple) else str(v))
def test_split_bits_do_not_depend_on_the_batch_the_call_or_the_chunk(dev, hip_lib, family, mask, params):
    """In split mode too (launch_conv3d_mid's comment: the one mode whose candidate kernels differ in bits): sample b of a batch is
    the bits of the same sample run alone, a second call repeats the first, and the refinement under ref_chunk_mb = 1 is the
    refinement under 72 -- (2,63,65) is there for that: its [H,W,32] map is 0.52 MB a pair, so 1 MB really makes chunks of one pair
    (the two small maps fit one chunk either way)."""
    from lwsnet_amd import ops
    c = FF.case(family, params)
    m = model(dev)
    names = ["cost"] if family == "conv3d_stack" else ["left", "pred3"]

    def run(sel=slice(None)):
        args = [cu(c.inputs[n][sel], dev) for n in names]
        return host(ops.conv3d_stack(m._h, params[0], *args) if family == "conv3d_stack" else ops.refine(m._h, *args))

    def all_of_it():
        whole = run()
        out = {"whole": whole, "again": run(), "alone": [run(slice(b, b + 1)) for b in range(whole.shape[0])]}
        if family == "refine":
            m.set_option("ref_chunk_mb", 1)
            try:
                out["chunked"] = run()
            finally:
                m.set_option("ref_chunk_mb", 72)
        return out

    exact = run()
    out = with_split(m, mask, all_of_it)
    whole = out["whole"].view(np.uint32)
    assert np.array_equal(out["again"].view(np.uint32), whole), "a second call gave other bits"
    for b, alone in enumerate(out["alone"]):
        assert np.array_equal(alone.view(np.uint32), whole[b:b + 1]), f"sample {b} alone differs from sample {b} of the batch"
    if family == "refine":
        assert np.array_equal(out["chunked"].view(np.uint32), whole), "ref_chunk_mb = 1 differs from 72"
    else:
        assert not np.array_equal(out["whole"], exact), "the option did not select the split kernel"


# ------------------------------------------------------------------ end to end
def forward(dev, name, split_bf16=(0,)):
    """The fixture and the stage maps of one model's forward (under each mask of option split_bf16, if more than the default)."""
    from lwsnet_amd.models import LWSNet
    g, args, sd, _ = FF.ref_source_case(name)               # args carries the fixture's align mode
    m = LWSNet(args, device=dev).set_state_dict(sd).eval()
    preds = []
    for mask in split_bf16:
        m.set_option("split_bf16", mask)
        preds.append([host(p) for p in m(g["left"], g["right"])])
    return (g, *preds)


def show_e2e(name, s, st):
    print(f"{name:20s} stage {s + 1}: mean {st.mean_ratio:4.2f} median {st.median_ratio:4.2f} |bias| {st.bias_ratio:4.2f} of the float32 floor; "
          f"within 1e-3 px: {100 * st.within_1e3:6.2f} % (reference float32: {100 * st.floor_within_1e3:6.2f} %)")


@pytest.mark.parametrize("name", FF.E2E_SMOOTH)
def test_e2e_distributions_on_the_smooth_fixtures(dev, hip_lib, name):
    """tests/test_float64_floor_cpu.py's gates of the same name on the model's forward (e2e_align1_64x256: a model built with
    interp_align_mode = 1): mean within 1.3 x, median within 1.35 x, |mean signed error| within 0.3 x the reference's own float32."""
    g, pred = forward(dev, name)
    for s in range(4):
        show_e2e(name, s, FF.assert_e2e_distribution(pred[s], g[f"pred{s}"], g[f"pred64_{s}"], f"{name} stage {s + 1}", **FF.E2E_SMOOTH_GATES))


@pytest.mark.parametrize("name", FF.E2E_CHAOTIC)
def test_e2e_medians_on_the_chaotic_fixtures(dev, hip_lib, name):
    """Single samples of a chaotic map (white noise; uncalibrated BatchNorm statistics): the median alone is gated, at 1.75 x."""
    g, pred = forward(dev, name)
    for s in range(4):
        show_e2e(name, s, FF.assert_e2e_distribution(pred[s], g[f"pred{s}"], g[f"pred64_{s}"], f"{name} stage {s + 1}", **FF.E2E_CHAOTIC_GATES))


@pytest.mark.parametrize("name", FF.E2E_SMOOTH)
def test_e2e_distributions_split(dev, hip_lib, name):
    """The smooth fixtures through a model with split_bf16 = 7 under the gates of the exact build (FF.E2E_SMOOTH_GATES: mean 1.3,
    median 1.35, bias 0.3 x the reference's own float32).  At these sizes bits 1 and 4 are live (stage 3 has 96 tiles per sample:
    its 8 -> 8 layers stay exact), so stage 4 is not the exact build's bits.  The bias gate is the one that would catch a device
    split that truncates where it should round to nearest: every operand then errs to the same side."""
    g, exact, pred = forward(dev, name, split_bf16=(0, 7))
    for s in range(4):
        show_e2e(name + " split", s, FF.assert_e2e_distribution(pred[s], g[f"pred{s}"], g[f"pred64_{s}"], f"{name} split_bf16 = 7 stage {s + 1}",
                                                               **FF.E2E_SMOOTH_GATES))
    assert not np.array_equal(pred[3], exact[3]), "split_bf16 = 7 gave the exact build's stage 4"
