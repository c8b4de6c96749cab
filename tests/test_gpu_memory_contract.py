"""The memory contract of every C-ABI entry point ("memory contract"): a result depends neither on what the
activation workspace held before the call nor on the memory beside the caller's tensors, nothing is stored outside the outputs,
and every output element is written.  Each case calls the ABI through ctypes with guarded pointers (tests/guarded.py): inputs
between poisoned flanks, outputs between poisoned flanks with a poisoned interior, the handle's workspace poisoned through
lws_debug_fill_workspace (caller workspaces: poisoned in place) -- under a quiet NaN, +FLT_MAX and -FLT_MAX in turn -- then
compares bit for bit with the reference the entry point's own test uses (the C oracle, tests/lr_reference.py,
geometry_reference.py, speckle_reference.py, the numpy float32 metrics of test_gpu_evaluate.py) and ends with Guard.check().
The shapes are the smallest that still reach every tile path: ragged on every axis, a single voxel, more than one workgroup."""
import ctypes

import numpy as np
import pytest

import geometry_reference as GEO
import guarded as G
import lr_reference as LR
import speckle_inputs as SI
import speckle_reference as SR
from conftest import golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WORDS = pytest.mark.parametrize("word", G.FLOAT_WORDS, ids=G.word_id)
SKEWS = pytest.mark.parametrize("skew", [0, 1], ids=["aligned", "skewed"])
RESERVE = (3, 64, 256)          # the largest geometry any case of this file runs: no later call regrows the poisoned slab

_REF = {}


def ref(key, fn):
    """References are computed once per case and shared by its poison words / plans; never modified."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def new_model(dev):
    from lwsnet_amd import _lib
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    m = LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().lws_reserve(m._h, *RESERVE), "lws_reserve")
    return m


@pytest.fixture(scope="module")
def model(dev, hip_lib):
    return new_model(dev)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def arr(n, ts):
    return (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(rc, what):
    from lwsnet_amd import _lib
    _lib.check(rc, what)


def poison_workspace(lib, h, word):
    torch.cuda.synchronize()
    ok(lib.lws_debug_fill_workspace(h, ctypes.c_uint32(word), stream()), "lws_debug_fill_workspace")


# ------------------------------------------------------------------ the hook itself
def test_fill_workspace_needs_a_workspace(dev, hip_lib):
    from lwsnet_amd import _lib
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    m = LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()
    with torch.cuda.device(dev):
        assert hip_lib.lws_debug_fill_workspace(m._h, G.QNAN, stream()) == _lib.LWS_ERR_STATE
        assert hip_lib.lws_reserve(m._h, 1, 64, 256) == 0
        assert hip_lib.lws_debug_fill_workspace(m._h, G.QNAN, stream()) == 0
        assert hip_lib.lws_debug_fill_workspace(m._h, G.MINUS_MAX, None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ core path, per op
@WORDS
@SKEWS
@pytest.mark.parametrize("shape,D", [((3, 16, 5, 24), 24), ((1, 16, 9, 37), 24)])
def test_volume_l1_shift(dev, hip_lib, shape, D, skew, word):
    from oracle import c_oracle as C
    rng = np.random.default_rng(11)
    L = rng.standard_normal(shape).astype(np.float32)
    R = rng.standard_normal(shape).astype(np.float32)
    want = ref(("shift", shape, D), lambda: C.volume_l1_shift(L, R, D))
    B, Cc, h, w = shape
    g = G.Guard(dev, word, skew)
    l, r, cost = g.place(L, name="L"), g.place(R, name="R"), g.empty((B, D, h, w), name="cost")
    with torch.cuda.device(dev):
        ok(hip_lib.lws_volume_l1_shift(P(l), P(r), P(cost), B, Cc, h, w, D, stream()), "lws_volume_l1_shift")
    G.assert_bits(cost, want, "cost")
    g.check()


@WORDS
@pytest.mark.parametrize("with_wflow", [True, False], ids=["wflow", "no-wflow"])
@pytest.mark.parametrize("B,C,h,w,scale,m,wild", [(2, 8, 19, 65, 2, 1, 0), (1, 16, 1, 7, 4, 2, 0), (2, 8, 40, 300, 2, 5, 700.0)])
def test_volume_l1_warp(dev, hip_lib, B, C, h, w, scale, m, wild, with_wflow, word):
    """The wild case holds LDS-window segments and gather-fallback segments in one launch."""
    from oracle import c_oracle as C_
    from test_gpu_parity import _warp_case
    L, R, prev, H, W = _warp_case(np.random.default_rng(5), B, C, h, w, scale, wild)

    def reference():
        wf = C_.resize_bilinear(prev[:, 0], h, w, float(h), float(np.float32(1) / np.float32(H)))
        return wf, C_.volume_l1_warp(L, R, wf, m)

    want_wf, want = ref(("warp", B, C, h, w, scale, m, wild), reference)
    g = G.Guard(dev, word)
    l, r, p = g.place(L, name="L"), g.place(R, name="R"), g.place(prev, name="prev")
    cost = g.empty((B, 2 * m - 1, h, w), name="cost")
    wflow = g.empty((B, h, w), name="wflow") if with_wflow else None
    with torch.cuda.device(dev):
        ok(hip_lib.lws_volume_l1_warp(P(l), P(r), P(p), P(cost), P(wflow), B, C, h, w, H, W, m, stream()), "lws_volume_l1_warp")
    G.assert_bits(cost, want, "cost")
    if with_wflow:
        G.assert_bits(wflow, want_wf, "wflow")
    g.check()


def mid8_takes_the_big_tile(B, D, h, w, ncu):
    """launch_conv3d_mid's rule for the 8 -> 8 layers (lwsnet_amd/csrc/lws_conv3d.hip): the 3 x 8 x 32 tile once there are 192
    of them, unless at most four small (3 x 4 x 32) tiles per CU are the shorter schedule of the fullest CU."""
    def cdiv(a, b):
        return -(-a // b)
    big = cdiv(w, 32) * cdiv(h, 8) * cdiv(D, 3) * B
    small = cdiv(w, 32) * cdiv(h, 4) * cdiv(D, 3) * B
    ks, kl = cdiv(small, ncu), cdiv(big, ncu)
    small_wins = ks <= 4 and ks * 384 < kl * 768
    return big >= 192 and not small_wins


BIG_TILE_CASE = (4, 9, 41, 89)          # 216 big tiles, ragged on every axis; 396 small ones: two rounds on 256 CUs, no win
CONV3D_CASES = ([(s, shape) for shape in ((1, 1, 1, 1), (2, 1, 5, 1), (1, 4, 9, 31)) for s in (0, 1, 2)]
                + [(0, (1, 24, 10, 40)), (2, BIG_TILE_CASE)])


@WORDS
@pytest.mark.parametrize("stage,shape", CONV3D_CASES)
def test_conv3d_stack(dev, hip_lib, model, stage, shape, word):
    """(1, 24, 10, 40) at stage 0: the tile that spans D.  BIG_TILE_CASE: the 3 x 8 x 32 tile of k_conv3d_mid8q, ragged in d,
    y and x -- the test recomputes the launch rule with this device's CU count and insists that the case reaches that tile."""
    from oracle import c_oracle as C
    if shape == BIG_TILE_CASE:
        ncu = torch.cuda.get_device_properties(dev).multi_processor_count
        assert mid8_takes_the_big_tile(*shape, ncu), f"{shape} does not reach the 3 x 8 x 32 tile on {ncu} CUs: choose another shape"
        assert not mid8_takes_the_big_tile(1, 4, 9, 31, ncu)           # and the small tile is covered beside it
    c = (np.random.default_rng(stage + 1).random(shape) * 12.0).astype(np.float32)
    want = ref(("conv3d", stage, shape), lambda: C.conv3d_stack(c, model.state_dict(), stage))
    g = G.Guard(dev, word)
    cin, cout = g.place(c, name="cost_in"), g.empty(shape, name="cost_out")
    with torch.cuda.device(dev):
        poison_workspace(hip_lib, model._h, word)
        ok(hip_lib.lws_conv3d_stack(model._h, stage, P(cin), P(cout), *shape, stream()), "lws_conv3d_stack")
    G.assert_bits(cout, want, f"conv3d_stack stage {stage} {shape}")
    g.check()


@WORDS
@pytest.mark.parametrize("shape,start", [((2, 9, 3, 5), -4.0), ((1, 24, 2, 67), 0.0)])
def test_softargmin(dev, hip_lib, shape, start, word):
    from oracle import c_oracle as C
    c = (np.random.default_rng(3).random(shape) * 12.0).astype(np.float32)
    want = ref(("softargmin", shape), lambda: C.softargmin(c, start))
    B, D, h, w = shape
    g = G.Guard(dev, word)
    cost, low = g.place(c, name="cost"), g.empty((B, h, w), name="disp_low")
    with torch.cuda.device(dev):
        ok(hip_lib.lws_softargmin(P(cost), P(low), B, D, h, w, start, stream()), "lws_softargmin")
    G.assert_bits(low, want, "disp_low")
    g.check()


@WORDS
@pytest.mark.parametrize("with_prev", [True, False], ids=["prev", "no-prev"])
@pytest.mark.parametrize("B,h,w,H,W", [(2, 3, 5, 24, 40), (1, 8, 32, 63, 255)])
def test_upsample_add(dev, hip_lib, B, h, w, H, W, with_prev, word):
    from oracle import c_oracle as C
    rng = np.random.default_rng(4)
    low_np = (rng.random((B, h, w)) * 20.0).astype(np.float32)
    prev_np = (rng.random((B, 1, H, W)) * 150.0).astype(np.float32) if with_prev else None
    want = ref(("upsample", B, h, w, H, W, with_prev), lambda: C.upsample_add(low_np, prev_np, H, W))
    g = G.Guard(dev, word)
    low = g.place(low_np, name="disp_low")
    prev = g.place(prev_np, name="prev") if with_prev else None
    out = g.empty((B, 1, H, W), name="out")
    with torch.cuda.device(dev):
        ok(hip_lib.lws_upsample_add(P(low), P(prev), P(out), B, h, w, H, W, stream()), "lws_upsample_add")
    G.assert_bits(out, want, "out")
    g.check()


@WORDS
@pytest.mark.parametrize("N,H,W", [(3, 32, 48), (1, 63, 255)])
def test_feature_extraction(dev, hip_lib, model, N, H, W, word):
    from oracle import c_oracle as C
    x = np.random.default_rng(3).standard_normal((N, 3, H, W)).astype(np.float32)
    want = ref(("features", N, H, W), lambda: C.feature_extraction(x, model.state_dict()))
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    g = G.Guard(dev, word)
    img = g.place(x, name="img")
    f8 = g.empty((N, 16, h2 // 4, w2 // 4), name="f8")
    f4 = g.empty((N, 16, h2 // 2, w2 // 2), name="f4")
    f2 = g.empty((N, 8, h2, w2), name="f2")
    with torch.cuda.device(dev):
        poison_workspace(hip_lib, model._h, word)
        ok(hip_lib.lws_feature_extraction(model._h, P(img), N, H, W, P(f8), P(f4), P(f2), stream()), "lws_feature_extraction")
    for name, got, w_ in zip(("f8", "f4", "f2"), (f8, f4, f2), want):
        G.assert_bits(got, w_, name)
    g.check()


@WORDS
@pytest.mark.parametrize("fuse_first", [0, 3])
@pytest.mark.parametrize("fuse_ref_last", [0, 1])
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 17, 15), (1, 33, 47)])
def test_refine(dev, hip_lib, model, B, H, W, fuse_ref_last, fuse_first, word):
    from oracle import c_oracle as C
    rng = np.random.default_rng(9)
    left_np = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    pred3_np = (rng.random((B, 1, H, W)) * 150.0).astype(np.float32)
    want = ref(("refine", B, H, W), lambda: C.refine(left_np, pred3_np, model.state_dict()))
    g = G.Guard(dev, word)
    left, pred3, pred4 = g.place(left_np, name="left"), g.place(pred3_np, name="pred3"), g.empty((B, 1, H, W), name="pred4")
    default_ff = model.get_option("fuse_first")
    model.set_option("fuse_ref_last", fuse_ref_last)
    model.set_option("fuse_first", fuse_first)
    try:
        with torch.cuda.device(dev):
            poison_workspace(hip_lib, model._h, word)
            ok(hip_lib.lws_refine(model._h, P(left), P(pred3), B, H, W, P(pred4), stream()), "lws_refine")
        torch.cuda.synchronize()
    finally:
        model.set_option("fuse_ref_last", -1)
        model.set_option("fuse_first", default_ff)
    G.assert_bits(pred4, want, "pred4")
    g.check()


@WORDS
def test_disparity_stages(dev, hip_lib, model, word):
    from oracle import c_oracle as C
    gold = golden("e2e_64x256.npz")
    fl = [gold[f"featL{i}"] for i in range(3)]
    fr = [gold[f"featR{i}"] for i in range(3)]
    want = ref("stages", lambda: C.disparity_stages(fl, fr, 64, 256, model.state_dict()))
    g = G.Guard(dev, word)
    tl = [g.place(f, name=f"featL{i}") for i, f in enumerate(fl)]
    tr = [g.place(f, name=f"featR{i}") for i, f in enumerate(fr)]
    preds = [g.empty((1, 1, 64, 256), name=f"pred{s + 1}") for s in range(3)]
    with torch.cuda.device(dev):
        poison_workspace(hip_lib, model._h, word)
        ok(hip_lib.lws_disparity_stages(model._h, arr(3, tl), arr(3, tr), 1, 64, 256, arr(3, preds), stream()), "lws_disparity_stages")
    for s in range(3):
        G.assert_bits(preds[s], want[s], f"stage {s + 1}")
    g.check()


# ------------------------------------------------------------------ the whole forward, through out=
def guarded_forward(g, m, lib, word, left_np, right_np, tag=""):
    B, _, H, W = left_np.shape
    left, right = g.place(left_np, name=tag + "left"), g.place(right_np, name=tag + "right")
    outs = [g.empty((B, 1, H, W), name=f"{tag}pred{s + 1}") for s in range(4)]
    with torch.cuda.device(m.device):
        poison_workspace(lib, m._h, word)
        got = m(left, right, out=outs)
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, outs)), "the guarded tensors themselves must reach lws_forward"
    return outs


def forward_reference(m, B, H, W, seed):
    from lwsnet_amd.synth import make_batch
    from oracle import c_oracle as C
    left, right = make_batch(B, H, W, seed)
    return left, right, ref(("forward", B, H, W, seed), lambda: C.forward(left, right, m.state_dict()))


@WORDS
@pytest.mark.parametrize("side_streams", [0, 1])
@pytest.mark.parametrize("B,H,W", [(1, 64, 256), (3, 64, 256), (2, 63, 255)])
def test_forward(dev, hip_lib, model, B, H, W, side_streams, word):
    """B = 1: the fused / deferred plan (no launch materialises pred1, the consumers write the stage-2/3 maps); B = 3: the
    materialised plan; 63 x 255: ragged maps at every scale, non-integer resize ratios."""
    left, right, want = forward_reference(model, B, H, W, 61)
    g = G.Guard(dev, word)
    model.set_option("side_streams", side_streams)
    try:
        outs = guarded_forward(g, model, hip_lib, word, left, right)
    finally:
        model.set_option("side_streams", 1)
    for s in range(4):
        G.assert_bits(outs[s], want[s], f"stage {s + 1}")
    g.check()


@WORDS
def test_forward_shape_change_on_a_stale_slab(dev, hip_lib, word):
    """One handle, reserved once at 3 x 64 x 256: a batch-1 forward at 40 x 264, then a batch-3 forward at 64 x 256.  ws_layout
    carves the slab differently for each, so without the re-poisoning the second call would meet the first one's activations at
    other offsets; with it, poison everywhere.  Both equal the C oracle."""
    m = new_model(dev)
    g = G.Guard(dev, word)
    for B, H, W in ((1, 40, 264), (3, 64, 256)):
        left, right, want = forward_reference(m, B, H, W, 61 if (H, W) == (64, 256) else 5)
        outs = guarded_forward(g, m, hip_lib, word, left, right, tag=f"{B}x{H}x{W} ")
        for s in range(4):
            G.assert_bits(outs[s], want[s], f"B={B} {H}x{W} stage {s + 1}")
    g.check()


# ------------------------------------------------------------------ I/O kernels
@WORDS
def test_preprocess_rgb8_and_apply_lut8(dev, hip_lib, word):
    """Sizes that are no multiple of 4, bases at element (byte) alignment only."""
    from lwsnet_amd import imageio
    from lwsnet_amd.synth import IMAGENET_MEAN, IMAGENET_STD
    rng = np.random.default_rng(4)
    B, H, W = 2, 37, 53
    img = rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)
    img[0].reshape(-1)[:768] = np.repeat(np.arange(256, dtype=np.uint8), 3)
    want = np.stack([imageio.to_input(img[b]) for b in range(B)])
    g = G.Guard(dev, word, skew=1)
    rgb, out = g.place(img, plane=H * W * 3, name="rgb"), g.empty((B, 3, H, W), name="out")
    mean = (ctypes.c_float * 3)(*[float(v) for v in IMAGENET_MEAN])
    std = (ctypes.c_float * 3)(*[float(v) for v in IMAGENET_STD])
    with torch.cuda.device(dev):
        ok(hip_lib.lws_preprocess_rgb8(P(rgb), P(out), B, H, W, mean, std, stream()), "lws_preprocess_rgb8")
    G.assert_bits(out, want, "preprocess_rgb8")
    disp_np = (rng.random((61, 47)) * 300.0 - 20.0).astype(np.float32)
    disp_np[0, :8] = [0.0, -0.5, -1.0, 255.999, 256.0, 1e10, -3e9, 191.5]
    with np.errstate(invalid="ignore"):
        want_rgb = imageio.disparity_to_color(disp_np)
    disp, lut = g.place(disp_np, name="disp"), g.place(imageio.jet_lut(), name="lut")
    col = g.empty((61, 47, 3), np.uint8, plane=61 * 47 * 3, name="colour")
    with torch.cuda.device(dev):
        ok(hip_lib.lws_apply_lut8(P(disp), P(lut), P(col), ctypes.c_int64(disp_np.size), stream()), "lws_apply_lut8")
    G.assert_bits(col, want_rgb, "apply_lut8")
    g.check()


# ------------------------------------------------------------------ left-right check
@WORDS
@SKEWS
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (1, 8, 1)])
def test_lr_pairs(dev, hip_lib, B, H, W, skew, word):
    rng = np.random.default_rng(B * W)
    left_np = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    right_np = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    wl, wr = LR.lr_pairs(left_np, right_np)
    g = G.Guard(dev, word, skew)
    left, right = g.place(left_np, name="left"), g.place(right_np, name="right")
    l2, r2 = g.empty((2 * B, 3, H, W), name="left2"), g.empty((2 * B, 3, H, W), name="right2")
    with torch.cuda.device(dev):
        ok(hip_lib.lws_lr_pairs(P(left), P(right), P(l2), P(r2), B, H, W, stream()), "lws_lr_pairs")
    G.assert_bits(l2, wl, "left2")
    G.assert_bits(r2, wr, "right2")
    g.check()


@WORDS
@SKEWS
@pytest.mark.parametrize("optional", [True, False], ids=["right+row_kept", "no-optional"])
@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (1, 8, 1)])
def test_lr_check(dev, hip_lib, B, H, W, fill, optional, skew, word):
    """Skewed bases with W = 7: rows start at every alignment, the scalar row path runs beside the float4 path."""
    from test_gpu_lrcheck import maps
    n = 2
    stages = [maps(B, H, W, 10 * s + W) for s in range(n)]
    want = ref(("lr", B, H, W, fill), lambda: [LR.lr_check(stages[s][0], stages[s][1], 1.0, fill) for s in range(n)])
    g = G.Guard(dev, word, skew)
    dl = [g.place(stages[s][0], name=f"dL{s}") for s in range(n)]
    drm = [g.place(stages[s][1], name=f"dRm{s}") for s in range(n)]
    out = [g.empty((B, 1, H, W), name=f"out{s}") for s in range(n)]
    mask = [g.empty((B, 1, H, W), np.uint8, name=f"mask{s}") for s in range(n)]
    right = [g.empty((B, 1, H, W), name=f"right{s}") for s in range(n)] if optional else []
    kept = g.empty((n, B, H), np.int32, name="row_kept") if optional else None
    with torch.cuda.device(dev):
        ok(hip_lib.lws_lr_check(arr(4, dl), arr(4, drm), n, B, H, W, 1.0, fill, arr(4, out), arr(4, mask), arr(4, right), P(kept),
                                stream()), "lws_lr_check")
    for s in range(n):
        wo, wm, wr, wk = want[s]
        G.assert_bits(out[s], wo, f"out {s}")
        G.assert_bits(mask[s], wm, f"mask {s}")
        if optional:
            G.assert_bits(right[s], wr, f"right {s}")
            G.assert_bits(kept[s], wk, f"row_kept {s}")
    g.check()


# ------------------------------------------------------------------ metrics
@WORDS
@pytest.mark.parametrize("mode", [0, 1])
def test_stage_metrics(dev, hip_lib, mode, word):
    """Caller workspace poisoned with the float word.  counts: exact; abs_sum: the fp64 sum of exactly numpy's float32 terms in
    the kernel's fixed order -- the rtol of test_gpu_evaluate.check, which an unwritten (poisoned) entry cannot meet."""
    from test_gpu_evaluate import expected, make
    B, Hg, W, off = 2, 37, 61, 3
    preds_np, gt_np = make(B, Hg, W, off, seed=B * 1000 + Hg + W + off)
    want_c, want_s = ref(("metrics", mode), lambda: expected(preds_np, gt_np, off, 192, mode))
    nbytes = int(hip_lib.lws_stage_metrics_workspace(B, Hg, W))
    assert nbytes > 0
    g = G.Guard(dev, word)
    preds = [g.place(p, name=f"pred{s}") for s, p in enumerate(preds_np)]
    gt = g.place(gt_np, name="gt")
    work = g.empty((nbytes,), np.uint8, word=word, name="workspace")
    counts = g.empty((4, B, 2), np.int64, name="counts")
    sums = g.empty((4, B), np.float64, name="abs_sum")
    with torch.cuda.device(dev):
        ok(hip_lib.lws_stage_metrics(arr(4, preds), B, Hg + off, W, off, P(gt), Hg, 192.0, mode, P(work), P(counts), P(sums), stream()),
           "lws_stage_metrics")
    G.assert_bits(counts, want_c, "counts")
    assert np.isfinite(want_s).all()
    np.testing.assert_allclose(sums.cpu().numpy(), want_s, rtol=1e-9)
    g.check()


# ------------------------------------------------------------------ geometry
def geometry_case(B, H, W, seed):
    from test_gpu_geometry import cam_rows, cameras, maps
    d, mask, rgb = maps(B, H, W, seed)
    return d, mask, rgb, cam_rows(cameras(B))


@WORDS
@pytest.mark.parametrize("subset", range(1, 8), ids=lambda k: "+".join(n for i, n in enumerate(("depth", "depth16", "disp16")) if k >> i & 1))
def test_depth_maps(dev, hip_lib, subset, word):
    """Every subset of the three outputs (cam = NULL where only disp16 is asked for), element-aligned bases."""
    B, H, W = 2, 31, 133
    d_np, mask_np, _, rows = geometry_case(B, H, W, 5)
    want = ref("depth_maps", lambda: GEO.depth_maps(d_np, mask_np, rows, 1.0, 80.0))
    g = G.Guard(dev, word, skew=1)
    disp, mask = g.place(d_np, name="disp"), g.place(mask_np, word=G.MASK_WORD, name="mask")
    cam = g.place(rows, name="cam") if subset & 3 else None
    outs = [g.empty((B, 1, H, W), dt, name=n) if subset >> i & 1 else None
            for i, (n, dt) in enumerate((("depth", np.float32), ("depth16", np.uint16), ("disp16", np.uint16)))]
    with torch.cuda.device(dev):
        ok(hip_lib.lws_depth_maps(P(disp), P(mask), P(cam), B, H, W, 1.0, 80.0, P(outs[0]), P(outs[1]), P(outs[2]), stream()),
           "lws_depth_maps")
    for i, name in enumerate(("depth", "depth16", "disp16")):
        if outs[i] is not None:
            G.assert_bits(outs[i], want[i], name)
    g.check()


@WORDS
@pytest.mark.parametrize("with_mask_rgb", [True, False], ids=["mask+rgb", "plain"])
def test_point_cloud(dev, hip_lib, with_mask_rgb, word):
    """Caller workspace poisoned; the records past counts[b] are "left unwritten" (include/lwsnet_hip.h): they still hold the poison."""
    B, H, W = 2, 17, 133
    d_np, mask_np, rgb_np, rows = geometry_case(B, H, W, 8)
    m_np, c_np = (mask_np, rgb_np) if with_mask_rgb else (None, None)
    clouds, want_n = ref(("cloud", with_mask_rgb), lambda: GEO.point_cloud(d_np, m_np, c_np, rows, 1.0, 80.0))
    nbytes = int(hip_lib.lws_point_cloud_workspace(B, H))
    assert nbytes > 0
    g = G.Guard(dev, word)
    disp, cam = g.place(d_np, name="disp"), g.place(rows, name="cam")
    mask = g.place(m_np, word=G.MASK_WORD, name="mask") if with_mask_rgb else None
    rgb = g.place(c_np, plane=H * W * 3, name="rgb") if with_mask_rgb else None
    work = g.empty((nbytes,), np.uint8, align16=True, word=word, name="workspace")
    points = g.empty((B, H * W, 16), np.uint8, plane=H * W * 16, align16=True, word=word, name="points")
    counts = g.empty((B,), np.int64, name="counts")
    with torch.cuda.device(dev):
        ok(hip_lib.lws_point_cloud(P(disp), P(mask), P(rgb), P(cam), B, H, W, 1.0, 80.0, P(work), P(points), P(counts), stream()),
           "lws_point_cloud")
    G.assert_bits(counts, want_n, "counts")
    p = points.cpu().numpy()
    for b, rec in enumerate(clouds):
        k = len(rec)
        assert 0 < k < H * W, "the inputs should leave both records and room behind them"
        assert np.array_equal(p[b, :k].reshape(-1), rec.view(np.uint8).reshape(-1)), f"image {b}: points differ"
        rest = p[b, k:].reshape(-1).view(np.uint32)
        assert (rest == word).all(), f"image {b}: {int((rest != word).sum())} words past counts[b] were written"
    g.check()


# ------------------------------------------------------------------ speckle filter
def speckle_reference(kind, B, H, W, masked, fill):
    d = SI.make(kind, B, H, W, 3 * H + W)
    m = SI.random_mask(B, H, W, H + 7 * W) if masked else None
    lab = ref(("speckle-lab", kind, B, H, W, masked), lambda: SR.labelling(d, m, 0.5))
    return d, m, ref(("speckle", kind, B, H, W, masked, fill), lambda: SR.apply(d, m, lab, 50, fill))


@WORDS
@pytest.mark.parametrize("kind", ["plateaus", "serpentine", "checkerboard"])
@pytest.mark.parametrize("B,H,W", [(2, 63, 255), (1, 1, 300)])
def test_speckle_filter(dev, hip_lib, B, H, W, kind, word):
    """Caller workspace (16-byte aligned, as the header demands) poisoned before every call.  Four forms: every optional output
    present; mask, labels and counts NULL; in place out = disp; in place mask_out = mask."""
    nbytes = int(hip_lib.lws_speckle_workspace(B, H, W))
    assert nbytes > 0
    shape = (B, 1, H, W)

    def call(g, disp, mask, fill, out, mask_out, labels, counts):
        work = g.empty((nbytes,), np.uint8, align16=True, word=word, name="workspace")
        with torch.cuda.device(dev):
            ok(hip_lib.lws_speckle_filter(P(disp), P(mask), B, H, W, 0.5, 50, fill, P(work), P(out), P(mask_out), P(labels), P(counts),
                                          stream()), "lws_speckle_filter")

    # every optional output, out of place
    d_np, m_np, (wo, wm, wl, wc) = speckle_reference(kind, B, H, W, True, 1)
    g = G.Guard(dev, word)
    disp, mask = g.place(d_np, name="disp"), g.place(m_np, word=G.MASK_WORD, name="mask")
    out, mask_out = g.empty(shape, name="out"), g.empty(shape, np.uint8, name="mask_out")
    labels, counts = g.empty(shape, np.int32, name="labels"), g.empty((B, 3), np.int64, name="counts")
    call(g, disp, mask, 1, out, mask_out, labels, counts)
    for got, w_, what in ((out, wo, "out"), (mask_out, wm, "mask_out"), (labels, wl, "labels"), (counts, wc, "counts")):
        G.assert_bits(got, w_, what)
    G.assert_bits(disp, d_np, "disp is only read")
    G.assert_bits(mask, m_np, "mask is only read")
    g.check()
    # mask, labels, counts NULL
    d_np, _, (wo, wm, _, _) = speckle_reference(kind, B, H, W, False, 0)
    g = G.Guard(dev, word)
    disp, out, mask_out = g.place(d_np, name="disp"), g.empty(shape, name="out"), g.empty(shape, np.uint8, name="mask_out")
    call(g, disp, None, 0, out, mask_out, None, None)
    G.assert_bits(out, wo, "out (no optional argument)")
    G.assert_bits(mask_out, wm, "mask_out (no optional argument)")
    g.check()
    # in place: out = disp
    d_np, m_np, (wo, wm, wl, wc) = speckle_reference(kind, B, H, W, True, 1)
    g = G.Guard(dev, word)
    disp, mask = g.place(d_np, name="disp"), g.place(m_np, word=G.MASK_WORD, name="mask")
    mask_out, counts = g.empty(shape, np.uint8, name="mask_out"), g.empty((B, 3), np.int64, name="counts")
    call(g, disp, mask, 1, disp, mask_out, None, counts)
    G.assert_bits(disp, wo, "out = disp")
    G.assert_bits(mask_out, wm, "mask_out (out = disp)")
    G.assert_bits(counts, wc, "counts (out = disp)")
    g.check()
    # in place: mask_out = mask
    d_np, m_np, (wo, wm, wl, wc) = speckle_reference(kind, B, H, W, True, 0)
    g = G.Guard(dev, word)
    disp, mask = g.place(d_np, name="disp"), g.place(m_np, word=G.MASK_WORD, name="mask")
    out, labels = g.empty(shape, name="out"), g.empty(shape, np.int32, name="labels")
    call(g, disp, mask, 0, out, mask, labels, None)
    G.assert_bits(out, wo, "out (mask_out = mask)")
    G.assert_bits(mask, wm, "mask_out = mask")
    G.assert_bits(labels, wl, "labels (mask_out = mask)")
    g.check()
