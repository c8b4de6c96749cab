"""Finite activations over the whole float32 exponent range through the network kernels (run with -m gpu on an MI355X).

"HIP == C oracle, bit for bit" is a statement about the arithmetic, not about N(0,1) data.  It rests on the f32 MFMA and
v_pk_fma_f32 keeping subnormal inputs and results (MODE.denorm as hipcc sets it), on the polynomial exp and its cut, and on the
device's f32 -> f16 conversion agreeing with the oracle's in fp16's subnormal range and under its maximum.  Here every network op
meets inputs scaled far down (differences, products and sums subnormal) and far up, -0.0, ties, and the boundaries of lws_expf.
Every test is bit for bit against oracle.c_oracle (built without fast-math) on the same inputs, and asserts that the C result is
finite, so that no case passes as NaN == NaN.

What the soft-argmin cases can and cannot reach: lws_expf (lws_device_math.h) returns exactly 0 below -80 and 2^n * y above it with
n >= -115, so its smallest result is about 2^-116, a normal number, and p_k * t^2 >= e^-80 / D stays normal too -- there is no
subnormal e_k and no sqrtf of a subnormal variance to meet.  What is held instead is the cut at -80 to the ulp, every rint
boundary of the range reduction below -69, the dead band [-80, -110], exact ties, and the three register-resident depths.

lws_upsample_add and lws_volume_l1_warp carry no handle, so a chosen low map reaches them under align mode 0 only; align mode 1
is held through models built with it (tests/test_gpu_float64_floor.py, tests/test_gpu_plan_matrix.py).

OUT OF SCOPE: non-finite activations.  include/lwsnet_hip.h says "costs are assumed finite".  The packed MFMA weights carry
all-zero phantom taps that read a real in-tile address (pack_mid_weights, lws_conv3d.hip), so an infinite activation meets
0 x inf on the device and not in the oracle: a known, accepted difference."""
import numpy as np
import pytest

import confidence_reference as CR
import float64_floor as FF
import guarded as G
import plan_matrix as pm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F = np.float32
_MODELS, _REF = {}, {}
TINY32 = float(np.finfo(np.float32).tiny)           # 2^-126: below it float32 is subnormal


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


def pow2(e):
    return F(2.0) ** F(e)


def model(dev, name="seeded", fp16=False):
    """One model per state dict of `state` and feature_fp16."""
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args
    if (name, fp16) not in _MODELS:
        _MODELS[(name, fp16)] = LWSNet(default_args(feature_fp16=fp16), device=dev).set_state_dict(state(name)).eval()
    return _MODELS[(name, fp16)]


def state(name):
    """seeded: FF.state_dict().  tiny_weights, as the issue words it: every convolution weight x 2^-100, every BatchNorm weight
    x 2^100 (the running means stay, so each shift t = beta - mean * s is of order 2^97 and the activations ride on it: finite,
    and the convolution products are 2^-100 of their operands).  subnormal_weights: every Conv3D weight but each stack's last
    x 2^-120 -- so most of them ARE subnormal MFMA B operands, and so are the products and the early partial sums -- with the
    BatchNorm that follows undoing it: its weight x 2^120 and its running mean x 2^-120, the statistics of the scaled activation."""
    from lwsnet_amd.weights import default_args, state_dict_spec

    def make():
        args, sd = FF.state_dict()
        if name == "seeded":
            return sd
        out = {k: v.copy() for k, v in sd.items()}
        if name == "tiny_weights":
            for key, _, kind in state_dict_spec(args):
                if kind == "conv":
                    out[key] = out[key] * pow2(-100)
                elif kind == "bnweight":
                    out[key] = out[key] * pow2(100)
        else:
            assert name == "subnormal_weights", name
            last = default_args().layers_3d + 1
            for i in range(3):
                for j in range(last):
                    out[f"volume_postprocess.{i}.{j}.2.weight"] = out[f"volume_postprocess.{i}.{j}.2.weight"] * pow2(-120)
                    out[f"volume_postprocess.{i}.{j + 1}.0.weight"] = out[f"volume_postprocess.{i}.{j + 1}.0.weight"] * pow2(120)
                    out[f"volume_postprocess.{i}.{j + 1}.0._mean"] = out[f"volume_postprocess.{i}.{j + 1}.0._mean"] * pow2(-120)
        assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in out.values())
        return out
    return ref(("state", name), make)


def finite(want, what):
    for i, a in enumerate(want if isinstance(want, (list, tuple)) else [want]):
        assert np.isfinite(a).all(), f"{what}: output {i} of the C oracle is not finite"


def scalings(x, rng):
    """name -> x under the scalings of the volume tests, each with a planted -0.0.  x 2^-120 leaves N(0,1) values normal (only
    the differences of near-equal values are subnormal); x 2^-135 makes the values, every difference and every sum subnormal."""
    out = {"2^-120": x * pow2(-120), "2^-135": x * pow2(-135), "2^100": x * pow2(100),
           "2^U(-60,60)": (x * F(2.0) ** rng.uniform(-60, 60, x.shape).astype(F)).astype(F)}
    for a in out.values():
        a.reshape(-1)[::37] = F(-0.0)
    return out


# ------------------------------------------------------------------ the cost volumes
SCALES = ["2^-120", "2^-135", "2^100", "2^U(-60,60)"]


@pytest.mark.parametrize("scale", SCALES)
def test_volume_l1_shift(dev, hip_lib, scale):
    """(3,16,5,24), D = 24.  x 2^-135: the differences |l - r| and their 16-term sums are all subnormal."""
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    rng = np.random.default_rng(501)
    L, R = (scalings(rng.standard_normal((3, 16, 5, 24)).astype(F), rng)[scale] for _ in "LR")
    want = C.volume_l1_shift(L, R, 24)
    finite(want, scale)
    if scale == "2^-135":
        assert 0 < np.abs(want).max() < TINY32
    G.assert_bits(ops.volume_l1_shift(cu(L, dev), cu(R, dev), 24), want, f"volume_l1_shift {scale}")


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B,C_,h,w,s,m,wild", [(2, 8, 19, 65, 2, 1, 0), (1, 8, 12, 40, 2, 5, 60)])
def test_volume_l1_warp(dev, hip_lib, B, C_, h, w, s, m, wild, scale):
    """The previous map stays in pixels (it is an index); the features carry the scale through the bilinear blend and the sums."""
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    H, W = h * s - 1, w * s - 1
    rng = np.random.default_rng(502 + wild)
    L, R = (scalings(rng.standard_normal((B, C_, h, w)).astype(F), rng)[scale] for _ in "LR")
    prev = (rng.random((B, 1, H, W)) * (wild if wild else 30.0) - (wild / 2.0 if wild else 0.0)).astype(F)
    wflow = C.resize_bilinear(prev[:, 0], h, w, float(h), float(F(1) / F(H)))
    want = C.volume_l1_warp(L, R, wflow, m)
    finite([wflow, want], scale)
    cost, got_flow = ops.volume_l1_warp(cu(L, dev), cu(R, dev), cu(prev, dev), m, return_wflow=True)
    G.assert_bits(got_flow, wflow, "wflow")
    G.assert_bits(cost, want, f"volume_l1_warp {scale}")


# ------------------------------------------------------------------ the soft-argmin
def expf_boundaries():
    """Arguments x <= 0 of lws_expf (as positive cost differences -x) at its seams, each with the three float32 values either
    side: the cut at 80, and x * log2(e) = n + 1/2 for n = -116 .. -100, where rint changes n (x between 69 and 80.1)."""
    log2e = np.float64(F(1.44269504088896341))
    centres = [F(80.0)] + [F((n + 0.5) / log2e) for n in range(100, 116)]
    out = []
    for c in centres:
        lo = hi = c
        out.append(c)
        for _ in range(3):
            lo, hi = np.nextafter(lo, F(0)), np.nextafter(hi, F(200))
            out += [lo, hi]
    return np.array(out, F)


def softargmin_cost(D):
    """[1,D,4,64]: row 0 -- the minimum is 0 at a seeded hypothesis, so the exponent's argument is the planted value exactly: the
    seams of expf_boundaries in turn, the rest between 69 and 80 (alive, e_k from 1e-30 to 2e-35); row 1 -- the same with a sweep
    through the dead band [80, 110]; row 2 -- a seeded minimum in [0, 5), a second hypothesis within O(1) of it, the others from
    60 to 110 above; row 3 -- exact ties: two-way, D-way at a non-zero constant, two-way beside a dead band, and -0.0 against 0.0."""
    rng = np.random.default_rng(600 + D)
    seams = expf_boundaries()
    c = np.empty((1, D, 4, 64), F)
    i = 0
    for x in range(64):
        for y in (0, 1):
            v = rng.uniform(69.0, 80.0, D).astype(F)
            if y == 1:
                v[::2] = np.linspace(80.0, 110.0, 64 * D, dtype=F)[x * D:(x + 1) * D][::2]
            n = min(D - 1, 6)
            v[rng.permutation(D)[:n]] = np.take(seams, np.arange(i, i + n), mode="wrap")
            i += n
            v[rng.integers(D)] = F(0.0)
            c[0, :, y, x] = v
        lo = F(rng.uniform(0.0, 5.0))
        v = (lo + rng.uniform(60.0, 110.0, D)).astype(F)
        k = rng.permutation(D)[:2]
        v[k[0]], v[k[1]] = lo, lo + F(rng.uniform(0.0, 2.0))
        c[0, :, 2, x] = v
        v = rng.uniform(70.0, 110.0, D).astype(F)
        k = rng.permutation(D)[:2]
        if x % 4 == 0:
            v[k] = F(0.0)
        elif x % 4 == 1:
            v[:] = F(3.7)
        elif x % 4 == 2:
            v[:] = F(100.0 + x)
            v[k] = F(x)
        else:
            v[k[0]], v[k[1]] = F(-0.0), F(0.0)
        c[0, :, 3, x] = v
    return c


@pytest.mark.parametrize("D,start,HW", [(24, 0.0, (31, 509)), (9, -4.0, (8, 128)), (32, 0.0, (32, 512))])
def test_softargmin_at_the_seams_of_the_exponential(dev, hip_lib, D, start, HW):
    """lws_softargmin and the five outputs of lws_softargmin_conf (disp_low, peak_low, sigma_low, conf, sigma) on softargmin_cost,
    against the C oracle's soft-argmin and tests/confidence_reference.py (numpy float32 around the oracle's expf), bit for bit."""
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    cost = softargmin_cost(D)
    want = CR.softargmin_conf(cost, start, *HW)
    low = C.softargmin(cost, start)
    finite([low] + list(want.values()), f"D={D}")
    G.assert_bits(want["disp_low"], low, "the two references")
    e = C.expf(-expf_boundaries())
    assert (e == 0).any() and (e[e > 0] >= TINY32).all()            # the cut is inside the planted values; nothing subnormal comes out
    x = cu(cost, dev)
    G.assert_bits(ops.softargmin(x, start), low, f"softargmin D={D}")
    got = ops.softargmin_conf(x, start, *HW)
    for name in want:
        G.assert_bits(getattr(got, name), want[name], f"softargmin_conf D={D} {name}")


@pytest.mark.parametrize("scale", [4.0, 8.0, 16.0])
def test_fused_last_layer_softargmin(dev, hip_lib, scale):
    """The fused last-layer + soft-argmin kernel takes its costs from the stack, so they are steered through the features: seeded
    feature maps x 4, 8, 16 give raw costs whose spread across the hypotheses reaches 80 and beyond, on both sides of the cut.
    lws_disparity_stages at batch 1 with fuse_last1 = 1 and 0 against C.disparity_stages, all three maps."""
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    H, W = 24, 200
    rng = np.random.default_rng(700)
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    shapes = [(1, 16, h2 // 4, w2 // 4), (1, 16, h2 // 2, w2 // 2), (1, 8, h2, w2)]
    fl, fr = ([(rng.standard_normal(s) * scale).astype(F) for s in shapes] for _ in "LR")
    sd = state("seeded")
    want, costs = C.disparity_stages(fl, fr, H, W, sd, return_costs=True)
    finite(want, f"x{scale}")
    spread = costs[0][1].max(axis=1) - costs[0][1].min(axis=1)
    print(f"features x {scale}: stage-1 filtered cost spread per pixel {spread.min():.1f} .. {spread.max():.1f}")
    if scale >= 8.0:
        assert spread.max() > 80.0
    m = model(dev)
    for fuse_last1 in (1, 0):
        m.set_option("fuse_last1", fuse_last1)
        try:
            got = ops.disparity_stages(m._h, [cu(a, dev) for a in fl], [cu(a, dev) for a in fr], H, W)
        finally:
            m.set_option("fuse_last1", pm.OPTION_DEFAULTS["fuse_last1"])
        for s in range(3):
            G.assert_bits(got[s], want[s], f"features x {scale} fuse_last1={fuse_last1} pred{s + 1}")


# ------------------------------------------------------------------ the upsample
@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("e", [-140, 110])
def test_upsample_add(dev, hip_lib, e, with_prev):
    """(1,8,32) -> (63,255), no ratio an integer.  x 2^-140: the low map, its taps (t * H) / h and the blend are subnormal; prev,
    where given, is at the same scale so that the sum does not swallow them."""
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    rng = np.random.default_rng(800)
    low = (rng.random((1, 8, 32)) * 20.0).astype(F) * pow2(e)
    low.reshape(-1)[::29] = F(-0.0)
    prev = ((rng.random((1, 1, 63, 255)) * 150.0).astype(F) * pow2(e)) if with_prev else None
    want = C.upsample_add(low, prev, 63, 255)
    finite(want, f"2^{e}")
    if e < 0:
        assert 0 < np.abs(want).max() < TINY32
    got = ops.upsample_add(cu(low, dev), cu(prev, dev) if with_prev else None, 63, 255)
    G.assert_bits(got, want, f"upsample_add 2^{e} prev={with_prev}")


# ------------------------------------------------------------------ the Conv3D stacks
STACK_SHAPES = [(1, 9, 17, 33), (2, 9, 30, 70)]
# (state dict, exponent of the cost's scale, shape); x 2^-140 and subnormal_weights at the small shape only: the C oracle is slow
# on subnormal operands
STACK_CASES = ([(name, e, shape) for name, e in (("seeded", -110), ("tiny_weights", 0)) for shape in STACK_SHAPES]
               + [("seeded", -140, STACK_SHAPES[0]), ("subnormal_weights", 0, STACK_SHAPES[0])])


def stack_case(name, e, stage, shape):
    """(cost, the C oracle's cost_out): cost = U(0, 12) x 2^e under the state dict `name`."""
    from oracle import c_oracle as C

    def make():
        cost = (np.random.default_rng([900, stage, *shape]).random(shape) * 12.0).astype(F) * pow2(e)
        want = C.conv3d_stack(cost, state(name), stage)
        finite(want, f"{name} 2^{e} stage {stage} {shape}")
        return cost, want
    return ref(("stack", name, e, stage, shape), make)


@pytest.mark.parametrize("stage", [0, 1, 2])
@pytest.mark.parametrize("name,e,shape", STACK_CASES, ids=[f"{n}-cost2^{e}-{FF.case_id('', (s,))}" for n, e, s in STACK_CASES])
def test_conv3d_stack(dev, hip_lib, name, e, stage, shape):
    """Costs x 2^-110 (tiny but normal: the first layer's fmaf(x, s, t) keeps them beside t) and x 2^-140 (subnormal inputs of the
    first layer and of the skip connection) under the seeded weights; costs of O(1) under `tiny_weights` and `subnormal_weights`
    (see `state`): subnormal MFMA B operands, subnormal products and partial sums, normal results."""
    from lwsnet_amd import ops
    cost, want = stack_case(name, e, stage, shape)
    if name == "subnormal_weights":
        w = state(name)[f"volume_postprocess.{stage}.1.2.weight"]
        assert (np.abs(w[w != 0]) < TINY32).mean() > 0.1
    got = ops.conv3d_stack(model(dev, name)._h, stage, cu(cost, dev))
    G.assert_bits(got, want, f"conv3d_stack {name} cost x 2^{e} stage {stage} {shape}")
    assert not np.array_equal(want, cost), "the stack added nothing to its input: the case is blind"


@pytest.mark.parametrize("shape", STACK_SHAPES, ids=["1x9x17x33", "2x9x30x70"])
@pytest.mark.parametrize("name,e", [("seeded", -110), ("tiny_weights", 0)], ids=["seeded-cost2^-110", "tiny_weights"])
@pytest.mark.parametrize("mask,stage", [(1, 0), (2, 1), (2, 2)])
def test_conv3d_stack_split(dev, hip_lib, mask, stage, name, e, shape):
    """The same under option split_bf16.  Mask 1 runs k_conv3d_mid16x at stage 0: no C restatement has its bits, and
    tests/test_float64_floor_cpu.py shows the CPU emulation on the floor, not bit-equal to anything, so the device result is held
    to the float64 floor of the literal restatement on these inputs (FF.check, 3.0 / 2.5) and must differ from the exact kernel's.
    Mask 2 at these shapes (30 and 72 tiles per sample, under the 256 from which k_conv3d_mid8x runs) stays on the exact kernel:
    the C oracle's bits."""
    from lwsnet_amd import ops
    from oracle import lws_oracle as O
    cost, want = stack_case(name, e, stage, shape)
    m = model(dev, name)
    m.set_option("split_bf16", mask)
    try:
        got = host(ops.conv3d_stack(m._h, stage, cu(cost, dev)))
    finally:
        m.set_option("split_bf16", 0)
    assert np.isfinite(got).all()
    if mask == 2:
        assert FF.mid8x_tiles(shape) < FF.MID8X_MIN_TILES
        G.assert_bits(got, want, f"split_bf16 = 2 below 256 tiles: {name} stage {stage} {shape}")
        return

    def lit(t, dt):
        return (O.post_3dconvs(t(cost)[:, None], state(name), stage, dt) + t(cost)[:, None])[:, 0]

    refs = ref(("stack literal", name, e, stage, shape), lambda: FF.literal(lit))
    c = FF.Case("conv3d_stack", (stage, shape, name, e), {"cost": cost}, {"cost_out": refs[0]}, stacked=["cost_out"])
    FF.check(c, {"cost_out": got}, show=print)
    assert not np.array_equal(got, want), "the option did not select the split kernel"


# ------------------------------------------------------------------ fp16 features
def fp16_features(kind, B, H, W):
    """Stage features whose values fall (sub) in fp16's subnormal range 2^-24 .. 2^-14 with exact ties (k + 1/2) 2^-24 between two
    fp16 subnormals planted, (under) below 2^-25 -- they round to zero or to the least subnormal, with the tie 2^-25 itself and its
    two neighbours planted -- and (top) in (65472, 65520), the last rounding interval under overflow: nothing at or above 65520."""
    rng = np.random.default_rng({"sub": 1, "under": 2, "top": 3}[kind] + 1000)
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    shapes = [(B, 16, h2 // 4, w2 // 4), (B, 16, h2 // 2, w2 // 2), (B, 8, h2, w2)]
    feats = []
    for _ in "LR":
        side = []
        for s in shapes:
            # top: one sign per channel on both sides, so that |l - r| is the difference of two roundings (0 or 32) and not 131000
            sign = F([1.0, -1.0])[np.arange(s[1]) % 2].reshape(1, -1, 1, 1) if kind == "top" else rng.choice(F([-1.0, 1.0]), s)
            if kind == "sub":
                a = (F(2.0) ** rng.uniform(-24, -14, s).astype(F)).astype(F)
                ties = ((rng.integers(0, 1023, a.size // 3) + 0.5) * 2.0 ** -24).astype(F)
                a.reshape(-1)[::3][:ties.size] = ties
            elif kind == "under":
                a = (F(2.0) ** rng.uniform(-40, -25, s).astype(F)).astype(F)
                t = pow2(-25)
                a.reshape(-1)[::5] = np.resize(F([t, np.nextafter(t, F(1)), np.nextafter(t, F(0)), 1.5 * t, 0.0]), a.reshape(-1)[::5].size)
            else:
                a = rng.uniform(65472.5, 65519.5, s).astype(F)
                edge = F([65504.0, 65488.0, np.nextafter(F(65488.0), F(0)), np.nextafter(F(65488.0), F(1e9)), np.nextafter(F(65520.0), F(0))])
                a.reshape(-1)[::7] = np.resize(edge, a.reshape(-1)[::7].size)
                assert a.max() < 65520.0 and a.min() > 65472.0
            side.append((a * sign).astype(F))
        feats.append(side)
    return feats


@pytest.mark.parametrize("kind", ["sub", "under", "top"])
def test_fp16_features_at_the_ends_of_fp16(dev, hip_lib, kind):
    """lws_disparity_stages on a model built with feature_fp16 against C.disparity_stages(..., feature_fp16=True) at 24 x 200,
    batch 2 and sample 0 alone; the oracle's rounding is numpy's on exactly these values (nearest even, no infinity)."""
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    H, W = 24, 200
    fl, fr = fp16_features(kind, 2, H, W)
    for a in fl + fr:
        r = C.round_fp16(a)
        assert np.array_equal(r.view(np.uint32), FF.fp16_round(a).view(np.uint32)) and np.isfinite(r).all()
        if kind != "top":
            assert (r != a).any() and np.abs(r).max() <= 2.0 ** -14
    want = C.disparity_stages(fl, fr, H, W, state("seeded"), feature_fp16=True)
    finite(want, kind)
    exact = C.disparity_stages(fl, fr, H, W, state("seeded"))
    if kind != "under":             # (there every cost is within 2^-20 of zero either way)
        assert any(not np.array_equal(a, b) for a, b in zip(want, exact)), "the rounding moves nothing: the case is blind"
    m = model(dev, fp16=True)
    for B in (2, 1):
        got = ops.disparity_stages(m._h, [cu(a[:B], dev) for a in fl], [cu(a[:B], dev) for a in fr], H, W)
        for s in range(3):
            G.assert_bits(got[s], want[s][:B], f"feature_fp16 {kind} B={B} pred{s + 1}")


# ------------------------------------------------------------------ the 2D networks
@pytest.mark.parametrize("e", [-125, 20])
def test_feature_extraction(dev, hip_lib, e):
    """Image x 2^-125 (the first convolution's products and sums are subnormal) and x 2^20, at (2,31,39)."""
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    img = np.random.default_rng(1100).standard_normal((2, 3, 31, 39)).astype(F) * pow2(e)
    want = C.feature_extraction(img, state("seeded"))
    finite(want, f"2^{e}")
    got = ops.feature_extraction(model(dev)._h, cu(img, dev))
    for name, g, w in zip(("f8", "f4", "f2"), got, want):
        G.assert_bits(g, w, f"feature_extraction 2^{e} {name}")


@pytest.mark.parametrize("fuse_first", [0, 3])
@pytest.mark.parametrize("e", [-125, 20])
def test_refine(dev, hip_lib, e, fuse_first):
    """Image x 2^-125 and x 2^20 at (1,33,47); the disparity map stays in pixels."""
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    rng = np.random.default_rng(1200)
    left = rng.standard_normal((1, 3, 33, 47)).astype(F) * pow2(e)
    pred3 = (rng.random((1, 1, 33, 47)) * 150.0).astype(F)
    want = ref(("refine", e), lambda: C.refine(left, pred3, state("seeded")))
    finite(want, f"2^{e}")
    m = model(dev)
    m.set_option("fuse_first", fuse_first)
    try:
        got = ops.refine(m._h, cu(left, dev), cu(pred3, dev))
    finally:
        m.set_option("fuse_first", pm.OPTION_DEFAULTS["fuse_first"])
    G.assert_bits(got, want, f"refine 2^{e} fuse_first={fuse_first}")
