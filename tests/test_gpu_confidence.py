"""lws_softargmin_conf and lws_forward_conf on the GPU against tests/confidence_reference.py: every comparison asks for zero differing
elements.  References are computed once per case and shared (never modified)."""
import ctypes
import itertools
import os
import shutil

import numpy as np
import pytest

import confidence_reference as CR
import guarded as G
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F = np.float32
START = {9: -4.0, 24: 0.0, 32: 0.0, 7: -3.0}
# (h, w) -> (H, W): ragged tiles at factor 8; factor 2; a non-integer ratio (pixels owned through their upper-left tap)
SHAPES = [((5, 11), (40, 88)), ((6, 9), (12, 18)), ((8, 32), (63, 255))]
NAMES = ("disp_low", "peak_low", "sigma_low", "conf", "sigma")

_REF = {}


def ref(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def op_case(B, D, hw, HW):
    def make():
        # costs from a peaked to a nearly flat softmax: the scale grows with the pixel index
        rng = np.random.default_rng(100 * D + B)
        scale = np.linspace(0.2, 14.0, hw[0] * hw[1], dtype=F).reshape(hw)
        cost = (rng.random((B, D) + hw).astype(F) * scale).astype(F)
        return cost, CR.softargmin_conf(cost, START[D], *HW)
    return ref(("op", B, D, hw, HW), make)


# ------------------------------------------------------------------ the per-op entry
@pytest.mark.parametrize("hw,HW", SHAPES, ids=["x8-ragged", "x2", "non-integer"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D", [9, 24, 32, 7])
def test_softargmin_conf_matches_the_reference(dev, hip_lib, D, B, hw, HW):
    """All five outputs, then every combination of NULL outputs: what is written never depends on what else is asked for."""
    from lwsnet_amd import _lib, ops
    cost_np, want = op_case(B, D, hw, HW)
    cost = cu(cost_np, dev)
    got = ops.softargmin_conf(cost, START[D], *HW)
    for name in NAMES:
        G.assert_bits(getattr(got, name), want[name], f"D={D} B={B} {hw}->{HW} {name}")
    G.assert_bits(ops.softargmin(cost, START[D]), want["disp_low"], "ops.softargmin")
    want_dev = {n: cu(want[n], dev).view(torch.int32) for n in NAMES}
    for on in itertools.product([False, True], repeat=5):
        if not any(on):
            continue
        part = ops.softargmin_conf(cost, START[D], *HW, **dict(zip(NAMES, on)))
        for name, flag in zip(NAMES, on):
            t = getattr(part, name)
            assert (t is not None) == flag
            if flag:
                assert torch.equal(t.view(torch.int32), want_dev[name]), f"outputs {on}: {name}"
    # an image gives the same bytes in any batch
    if B > 1:
        one = ops.softargmin_conf(cost[B - 1:], START[D], *HW)
        for name in NAMES:
            G.assert_bits(getattr(one, name), want[name][B - 1:], f"last image alone: {name}")
    with pytest.raises(ValueError):
        _lib.check(hip_lib.lws_softargmin_conf(P(cost), B, D, *hw, START[D], *HW, None, None, None, None, None, stream()))


def test_softargmin_conf_exact_cases(dev, hip_lib):
    from lwsnet_amd import ops
    for D, start, k in ((9, -4.0, 0), (24, 0.0, 17), (7, -3.0, 6)):
        cost = np.full((1, D, 5, 11), 1e4, F)
        cost[:, k] = 0.0
        r = ops.softargmin_conf(cu(cost, dev), start, 40, 88)
        assert torch.all(r.disp_low == start + k) and torch.all(r.peak_low == 1.0) and torch.all(r.sigma_low.view(torch.int32) == 0)
        assert torch.all(r.conf == 1.0) and torch.all(r.sigma.view(torch.int32) == 0)
    for D, start in ((9, -4.0), (7, -3.0), (33, 0.0)):
        cost = np.full((2, D, 6, 9), 2.5, F)
        r = ops.softargmin_conf(cu(cost, dev), start, 12, 18)
        p = F(1.0) / F(D)
        assert torch.all((r.disp_low - (start + (D - 1) // 2)).abs() < 1e-5)
        assert torch.all(r.peak_low == float((F(0.0) + p) + p + p))
        want = CR.softargmin_conf(cost, start, 12, 18)
        for name in NAMES:
            G.assert_bits(getattr(r, name), want[name], f"flat D={D} {name}")


# ------------------------------------------------------------------ the forward
def new_model(dev, mode=0):
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    return LWSNet(default_args(interp_align_mode=mode), device=dev).set_state_dict(make_state_dict(7)).eval()


def model_of(dev, mode):
    return ref(("model", mode), lambda: new_model(dev, mode))


def forward_case(dev, mode, B, H, W):
    """(left, right, conf reference [3], sigma reference [3]): the reference applied to the C oracle's filtered costs, computed from
    the features the library's own extractor gives (the extractor has its own bit-exact tests)."""
    def make():
        from lwsnet_amd import ops
        from lwsnet_amd.synth import make_batch
        from oracle import c_oracle as C, lws_oracle as O
        m = model_of(dev, mode)
        left, right = make_batch(B, H, W, 4100 + 10 * B + H)
        with torch.cuda.device(dev):
            feats = ops.feature_extraction(m._h, cu(np.concatenate([left, right]), dev))
        fl = [f[:B].cpu().numpy() for f in feats]
        fr = [f[B:].cpu().numpy() for f in feats]
        conf, sigma = [], []
        with O.variant(align_mode=mode):
            _, costs = C.disparity_stages(fl, fr, H, W, m.state_dict(), return_costs=True)
            for s, (_, cost) in enumerate(costs):
                start = 0.0 if s == 0 else float(-m.maxdisplist[s] + 1)
                _, peak, sig = CR.low_maps(cost, start)
                c, g = CR.full_maps(peak, sig, H, W)
                conf.append(c)
                sigma.append(g)
        return left, right, conf, sigma
    return ref(("forward", mode, B, H, W), make)


FORWARD_CASES = [(0, 1, 64, 256), (0, 2, 64, 256), (0, 3, 64, 256), (0, 1, 63, 255), (1, 1, 64, 256), (1, 1, 63, 255)]


@pytest.mark.parametrize("mode,B,H,W", FORWARD_CASES)
def test_forward_conf_matches_the_forward_and_the_reference(dev, hip_lib, mode, B, H, W):
    """preds are the bits of model(left, right) -- at B <= 2 that is the deferred / fused plan, at B = 3 the plan with fused last
    layers and upsample launches, neither of which lws_forward_conf runs -- and conf / sigma are the reference's bits."""
    m = model_of(dev, mode)
    left, right, conf, sigma = forward_case(dev, mode, B, H, W)
    want = [p.clone() for p in m(left, right)]
    res = m.forward_conf(left, right)
    assert len(res.preds) == 4 and len(res.conf) == 3 and len(res.sigma) == 3
    for s in range(4):
        assert torch.equal(res.preds[s].view(torch.int32), want[s].view(torch.int32)), f"pred{s + 1}"
    for s in range(3):
        G.assert_bits(res.conf[s], conf[s], f"conf stage {s + 1}")
        G.assert_bits(res.sigma[s], sigma[s], f"sigma stage {s + 1}")
    # and the plain forward is undisturbed afterwards
    again = m(left, right)
    assert all(torch.equal(a, b) for a, b in zip(again, want))


def test_forward_conf_null_outputs_and_profiler_class(dev, hip_lib):
    from lwsnet_amd import _lib, ops
    m = model_of(dev, 0)
    left, right, conf, sigma = forward_case(dev, 0, 1, 64, 256)
    l, r = cu(left, dev), cu(right, dev)
    want = m(l, r)
    with torch.cuda.device(dev):
        preds, c, s = ops.forward_conf(m._h, l, r, sigma=False)
        assert s is None
        preds2, c2, s2 = ops.forward_conf(m._h, l, r, conf=False)
        assert c2 is None
        # single NULL entries: stage 2's conf and stage 1's sigma are not wanted
        outs = [torch.empty((1, 1, 64, 256), device=dev) for _ in range(4)]
        cs = [torch.full((1, 1, 64, 256), -7.0, device=dev) for _ in range(3)]
        ss = [torch.full((1, 1, 64, 256), -7.0, device=dev) for _ in range(3)]
        a4 = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in outs])
        ac = (ctypes.c_void_p * 3)(cs[0].data_ptr(), None, cs[2].data_ptr())
        asg = (ctypes.c_void_p * 3)(None, ss[1].data_ptr(), ss[2].data_ptr())
        _lib.check(hip_lib.lws_profile_enable(m._h, (1 << _lib.LWS_KC_COUNT) - 1))
        try:
            _lib.check(hip_lib.lws_forward_conf(m._h, P(l), P(r), 1, 64, 256, a4, ac, asg, stream()), "lws_forward_conf")
            torch.cuda.synchronize()
            tot = (ctypes.c_double * _lib.LWS_KC_COUNT)()
            cnt = (ctypes.c_int64 * _lib.LWS_KC_COUNT)()
            _lib.check(hip_lib.lws_profile_read(m._h, tot, cnt))
        finally:
            _lib.check(hip_lib.lws_profile_enable(m._h, 0))
    names = [hip_lib.lws_kernel_class_name(k).decode() for k in range(_lib.LWS_KC_COUNT)]
    got = dict(zip(names, cnt))
    # the plan that keeps the costs: three unfused soft-argmin launches and three confidence launches
    assert got["softargmin_conf"] == 3 and got["softargmin"] == 3 and got["conv3d_last"] == 3
    for k in range(4):
        assert torch.equal(preds[k], want[k]) and torch.equal(preds2[k], want[k]) and torch.equal(outs[k], want[k])
    for k in range(3):
        G.assert_bits(c[k], conf[k], f"conf {k}")
        G.assert_bits(s2[k], sigma[k], f"sigma {k}")
    G.assert_bits(cs[0], conf[0], "conf 0")
    G.assert_bits(cs[2], conf[2], "conf 2")
    G.assert_bits(ss[1], sigma[1], "sigma 1")
    G.assert_bits(ss[2], sigma[2], "sigma 2")
    assert torch.all(cs[1] == -7.0) and torch.all(ss[0] == -7.0)


def test_forward_conf_after_a_larger_geometry(dev, hip_lib):
    """Stale workspace: a fresh handle runs 3 x 64x256 first; the smaller geometries that follow read none of what it left."""
    m = new_model(dev, 0)
    for B, H, W in ((3, 64, 256), (1, 63, 255), (1, 64, 256)):
        left, right, conf, sigma = forward_case(dev, 0, B, H, W)
        res = m.forward_conf(left, right)
        for s in range(3):
            G.assert_bits(res.conf[s], conf[s], f"{B}x{H}x{W} conf stage {s + 1}")
            G.assert_bits(res.sigma[s], sigma[s], f"{B}x{H}x{W} sigma stage {s + 1}")


def test_forward_conf_graph_capture(dev, hip_lib):
    """Captured after lws_reserve, replayed on new inputs: the bits of the eager call."""
    from lwsnet_amd import _lib
    m = new_model(dev, 0)
    for B in (1, 3):
        la, ra, conf_a, sigma_a = forward_case(dev, 0, B, 64, 256)
        eager = m.forward_conf(la, ra)
        want_preds = [p.clone() for p in eager.preds]
        # new inputs: the same pairs mirrored top to bottom
        lb, rb = np.ascontiguousarray(la[:, :, ::-1]), np.ascontiguousarray(ra[:, :, ::-1])
        eager_b = m.forward_conf(lb, rb)
        want_b = [[t.clone() for t in part] for part in eager_b]
        lt, rt = cu(la, dev), cu(ra, dev)
        with torch.cuda.device(dev):
            _lib.check(hip_lib.lws_reserve(m._h, B, 64, 256), "lws_reserve")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            res = m.forward_conf(lt, rt)
        for part in res:
            for t in part:
                t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for s in range(4):
            assert torch.equal(res.preds[s], want_preds[s]), f"B={B} replay pred{s + 1}"
        for s in range(3):
            G.assert_bits(res.conf[s], conf_a[s], f"B={B} replay conf stage {s + 1}")
            G.assert_bits(res.sigma[s], sigma_a[s], f"B={B} replay sigma stage {s + 1}")
        lt.copy_(cu(lb, dev))
        rt.copy_(cu(rb, dev))
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        for part, want in zip(res, want_b):
            for s, (a, b) in enumerate(zip(part, want)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"B={B} replay on new inputs, map {s}"


# ------------------------------------------------------------------ memory contract
WORDS = pytest.mark.parametrize("word", G.FLOAT_WORDS, ids=G.word_id)


@WORDS
@pytest.mark.parametrize("skew", [0, 1], ids=["aligned", "skewed"])
@pytest.mark.parametrize("B,D,hw,HW", [(3, 9, (5, 11), (40, 88)), (1, 7, (8, 32), (63, 255)), (1, 24, (6, 9), (12, 18))])
def test_softargmin_conf_under_guard_bands(dev, hip_lib, B, D, hw, HW, skew, word):
    from lwsnet_amd import _lib
    cost_np, want = op_case(B, D, hw, HW)
    g = G.Guard(dev, word, skew)
    cost = g.place(cost_np, name="cost")
    outs = [g.empty((B,) + hw, name=n) for n in NAMES[:3]] + [g.empty((B, 1) + HW, name=n) for n in NAMES[3:]]
    with torch.cuda.device(dev):
        _lib.check(hip_lib.lws_softargmin_conf(P(cost), B, D, *hw, START[D], *HW, *[P(t) for t in outs], stream()), "lws_softargmin_conf")
    for name, t in zip(NAMES, outs):
        G.assert_bits(t, want[name], name)
    g.check()


@WORDS
@pytest.mark.parametrize("B,H,W", [(2, 64, 256), (1, 63, 255)])
def test_forward_conf_under_guard_bands(dev, hip_lib, B, H, W, word):
    from lwsnet_amd import _lib
    m = ref("guard model", lambda: new_model(dev, 0))
    left_np, right_np, conf, sigma = forward_case(dev, 0, B, H, W)
    want = ref(("guard preds", B, H, W), lambda: [p.cpu().numpy() for p in model_of(dev, 0)(left_np, right_np)])
    with torch.cuda.device(dev):
        _lib.check(hip_lib.lws_reserve(m._h, 2, 64, 256), "lws_reserve")      # the largest geometry of this test: the slab never regrows
    g = G.Guard(dev, word)
    left, right = g.place(left_np, name="left"), g.place(right_np, name="right")
    preds = [g.empty((B, 1, H, W), name=f"pred{s + 1}") for s in range(4)]
    cs = [g.empty((B, 1, H, W), name=f"conf{s + 1}") for s in range(3)]
    ss = [g.empty((B, 1, H, W), name=f"sigma{s + 1}") for s in range(3)]
    arr = lambda n, ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])      # noqa: E731
    with torch.cuda.device(dev):
        torch.cuda.synchronize()
        _lib.check(hip_lib.lws_debug_fill_workspace(m._h, ctypes.c_uint32(word), stream()), "lws_debug_fill_workspace")
        _lib.check(hip_lib.lws_forward_conf(m._h, P(left), P(right), B, H, W, arr(4, preds), arr(3, cs), arr(3, ss), stream()),
                   "lws_forward_conf")
    torch.cuda.synchronize()
    for s in range(4):
        G.assert_bits(preds[s], want[s], f"pred{s + 1}")
    for s in range(3):
        G.assert_bits(cs[s], conf[s], f"conf stage {s + 1}")
        G.assert_bits(ss[s], sigma[s], f"sigma stage {s + 1}")
    g.check()


# ------------------------------------------------------------------ the CLI
def test_inference_cli_confidence(dev, hip_lib, tmp_path):
    from PIL import Image
    from lwsnet_amd import imageio as io, inference, ops
    from lwsnet_amd.geometry import Camera
    src = os.path.join(ROOT, "tests", "golden", "kitti_pair")
    for n in ("left_test.png", "right_test.png"):
        shutil.copy(os.path.join(src, n), tmp_path / n)
    lp, rp = str(tmp_path / "left_test.png"), str(tmp_path / "right_test.png")
    camera = ["721.5", "721.5", "609.5", "172.8", "0.54"]
    written = inference.main(["--left_img", lp, "--synthetic_weights", "--save_conf", "--conf_min", "0.5", "--save_ply", "--camera", *camera])
    assert [os.path.basename(p) for p in written] == ["1.png", "1.ply", "2.png", "2.ply", "3.png", "3_conf.png", "3_sigma.png", "3.ply",
                                                      "4.png", "4.ply"]
    assert all(os.path.isfile(p) for p in written)
    full = io.load_rgb(lp)
    left = io.crop_bottom_right(full)
    m = model_of(dev, 0)
    res = m.forward_conf(io.to_input(left)[None], io.to_input(io.crop_bottom_right(io.load_rgb(rp)))[None])
    conf3, sigma3 = res.conf[2].numpy()[0, 0].astype(np.float64), res.sigma[2].numpy()[0, 0].astype(np.float64)
    img = Image.open(tmp_path / "3_conf.png")
    assert img.mode == "L" and np.array_equal(np.asarray(img), np.rint(np.clip(conf3, 0.0, 1.0) * 255.0).astype(np.uint8))
    img = Image.open(tmp_path / "3_sigma.png")
    assert img.mode == "L" and np.array_equal(np.asarray(img), np.rint(np.minimum(sigma3, 8.0) * 255.0 / 8.0).astype(np.uint8))
    # the colour files are a plain run's
    for s in range(4):
        assert np.array_equal(np.asarray(Image.open(tmp_path / f"{s + 1}.png")), io.disparity_to_color(res.preds[s].numpy()[0, 0]))
    # the point clouds hold exactly the pixels ops.point_cloud keeps under the confidence mask of the map's stage
    cam = Camera(*[float(v) for v in camera]).crop_bottom_right(*full.shape[:2], io.CROP_H, io.CROP_W)
    rgb = torch.from_numpy(np.ascontiguousarray(left)[None]).to(dev)
    dropped = 0
    for s in range(4):
        mask = ops.confidence_codes(res.conf, res.sigma, min_conf=0.5, stages=(min(s, 2),))
        with torch.cuda.device(dev):
            _, counts = ops.point_cloud(res.preds[s].as_subclass(torch.Tensor), cam, mask, rgb, 1.0, float("inf"))
            _, unmasked = ops.point_cloud(res.preds[s].as_subclass(torch.Tensor), cam, None, rgb, 1.0, float("inf"))
        with open(tmp_path / f"{s + 1}.ply", "rb") as f:
            header = f.read(400).split(b"end_header")[0].decode()
        n = int([ln for ln in header.splitlines() if ln.startswith("element vertex")][0].split()[-1])
        assert n == int(counts[0]) and n <= int((mask == 1).sum())
        dropped += int(unmasked[0]) - n
    assert dropped > 0, "the threshold should drop something from this pair"
