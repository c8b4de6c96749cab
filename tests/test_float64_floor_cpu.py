"""Every network op of the C restatement (oracle/lws_oracle.c through oracle/c_oracle.py: the bits the HIP kernels are held to)
against the literal restatement (oracle/lws_oracle.py) in float64, by the yardstick of the literal restatement's own float32 run
(tests/float64_floor.py), at the smallest shapes that reach every border rule.  Part A: the helper bites -- planted defects on
the literal float32 output itself, no HIP and no C library.  Part B: the C restatement per op.  Part C: the distributions of the
end-to-end stage maps on the committed reference-source fixtures.  Part D: the split-bf16 kernels' arithmetic restated, six terms
on the floor and five terms off it.  Run with -s for the ratio tables (tools/noise_budget.py
--per-op --e2e prints the same)."""
import os

import numpy as np
import pytest
import torch

import float64_floor as FF
from conftest import ROOT
from oracle import c_oracle as C
from oracle import lws_oracle as O

ALL_CASES = [(family, params) for family, cases in FF.CASES.items() for params in cases]
_ROWS = []          # (family, label, Ratios) of every gate part B has run: the table the last test prints


# ------------------------------------------------------------------ part A: the helper bites
def _refine():
    c = FF.case("refine", (2, 17, 15))
    r32, r64 = c.refs["pred4"]
    car = c.carrier["pred4"].astype(np.float64)
    return r32, r64, car


def _residual_gate(got, ring=True):
    """What FF.check does to refine's output: the gate with the 150-px carrier removed from all three."""
    r32, r64, car = _refine()
    return FF.assert_on_float32_floor(got.astype(np.float64) - car, r32.astype(np.float64) - car, r64 - car, "planted", ring=ring)


def _features():
    return FF.case("feature_extraction", (1, 15, 23))


def test_the_literal_float32_output_passes_against_itself():
    r32, r64, _ = _refine()
    assert FF.assert_on_float32_floor(r32, r32, r64, "refine") == FF.Ratios(1.0, 1.0, 1.0, 1.0)
    _residual_gate(r32)
    c = _features()
    for name, (a, b) in c.refs.items():
        r = FF.assert_on_float32_floor(a, a, b, name)
        assert r.max == 1.0 and r.mean == 1.0
        assert (r.ring_max is None) == (min(a.shape[2:]) < 3)               # f8 is 2 x 3 here: all ring, no gate of its own
    FF.check(c, {name: a for name, (a, _) in c.refs.items()})
    FF.check(FF.case("refine", (2, 17, 15)), {"pred4": r32})


def test_ring_mask():
    m = FF.ring_mask((2, 3, 4, 5))
    assert m.sum() == 2 * 3 * (4 * 5 - 2 * 3) and not m[:, :, 1:-1, 1:-1].any()
    s = FF.ring_mask((2, 3, 4, 5), stacked=True)
    assert s[:, 0].all() and s[:, 2].all() and s[:, 1].sum() == 2 * 14 and s.sum() == 2 * (2 * 20 + 14)
    assert FF.ring_mask((1, 2, 3, 4, 5)).sum() == 2 * (2 * 20 + 14)
    assert FF.ring_mask((2, 4, 5)).sum() == 2 * 14                           # [B,h,w]: no channel extent needed
    assert not FF.has_ring((1, 16, 2, 3)) and FF.has_ring((1, 16, 3, 3)) and not FF.has_ring((5,))


def test_every_element_scaled_by_2e_6_raises():
    """On the refine map (pred4 of 150 px: a defect of 3e-4 px) and on f8 and f2.  On f4 of this case the same defect measures 3.8 x
    (max) and 6.2 x (mean) the floor and still passes: its floor is 5e-7 of the scale at the maximum but 4e-8 in the mean, so
    `tiny` = 4.8e-7 of the scale is most of the mean gate there.  Twice the defect is caught on f4 too."""
    def scaled(a, k):
        return (a.astype(np.float64) * (1 + k)).astype(np.float32)

    r32, r64, _ = _refine()
    with pytest.raises(AssertionError, match="whole tensor.*off the float32 floor"):
        FF.assert_on_float32_floor(scaled(r32, 2e-6), r32, r64, "planted")
    refs = _features().refs
    for name, k in (("f8", 2e-6), ("f2", 2e-6), ("f4", 4e-6)):
        with pytest.raises(AssertionError, match="off the float32 floor"):
            FF.assert_on_float32_floor(scaled(refs[name][0], k), *refs[name], name)


def test_a_constant_on_the_last_column_is_caught_by_the_ring_gate():
    """2e-5 px on one column of a 17 x 15 map: 1/15 of the pixels, which the whole-tensor mean and maximum let through --
    the same two statistics over the 60-pixel ring of each plane do not."""
    r32, r64, car = _refine()
    got = r32.astype(np.float64)
    got[..., -1] += 2e-5
    res = (got - car, r32.astype(np.float64) - car, r64 - car)
    FF.assert_on_float32_floor(*res, "planted", ring=False)
    with pytest.raises(AssertionError, match=r"border ring.*\(on the border ring\)"):
        FF.assert_on_float32_floor(*res, "planted", ring=True)


def test_a_shift_by_one_pixel_raises():
    r32, _, _ = _refine()
    with pytest.raises(AssertionError, match="off the float32 floor"):
        _residual_gate(np.roll(r32, 1, axis=-1))
    for name, (a, b) in _features().refs.items():
        with pytest.raises(AssertionError, match="off the float32 floor"):
            FF.assert_on_float32_floor(np.roll(a, 1, axis=-1), a, b, name)


def test_one_zeroed_row_raises_and_is_located():
    r32, r64, _ = _refine()
    got = r32.copy()
    got[1, 0, 5, :] = 0.0
    with pytest.raises(AssertionError, match=r"worst element at flat index \d+ = \(1, 0, 5, \d+\)"):
        FF.assert_on_float32_floor(got, r32, r64, "planted")
    a, b = _features().refs["f2"]
    got = a.copy()
    got[0, :, 3, :] = 0.0
    with pytest.raises(AssertionError, match=r"= \(0, \d, 3, \d+\) \(off the border ring\)"):
        FF.assert_on_float32_floor(got, a, b, "planted")


def test_two_swapped_channels_of_f4_raise():
    a, b = _features().refs["f4"]
    got = a.copy()
    got[:, [3, 11]] = got[:, [11, 3]]
    with pytest.raises(AssertionError, match="off the float32 floor"):
        FF.assert_on_float32_floor(got, a, b, "f4")


def test_one_nan_raises():
    r32, r64, _ = _refine()
    got = r32.copy()
    got[1, 0, 9, 2] = np.nan
    with pytest.raises(AssertionError, match=r"1 element\(s\) are not finite .* = \(1, 0, 9, 2\)"):
        FF.assert_on_float32_floor(got, r32, r64, "planted")
    with pytest.raises(AssertionError, match="shapes differ"):
        FF.assert_on_float32_floor(r32[:, :, :-1], r32, r64, "planted")


def test_an_exact_floor_of_zero_does_not_divide_by_zero():
    """D = 1: the soft-argmin is `start` exactly in every precision, the floor 0 and `tiny` the whole gate."""
    ref64 = np.full((1, 3, 3), 2.0)
    ref32 = ref64.astype(np.float32)
    assert FF.assert_on_float32_floor(ref32, ref32, ref64, "exact") == FF.Ratios(0.0, 0.0, 0.0, 0.0)
    r = FF.assert_on_float32_floor(np.nextafter(ref32, np.float32(3)), ref32, ref64, "one ulp")
    assert r.max == float("inf")
    with pytest.raises(AssertionError, match="off the float32 floor"):
        FF.assert_on_float32_floor(ref32 + np.float32(1e-5), ref32, ref64, "planted")
    zero = np.zeros((1, 3, 3))
    FF.assert_on_float32_floor(zero.astype(np.float32), zero.astype(np.float32), zero, "all zero")


# ------------------------------------------------------------------ part B: the C restatement per op
@pytest.mark.parametrize("family,params", ALL_CASES, ids=[f"{f}-{FF.case_id(f, p)}" for f, p in ALL_CASES])
def test_c_restatement_on_the_float32_floor(family, params):
    c = FF.case(family, params)
    rows = FF.check(c, FF.C_RUNNERS[family](c), show=print)
    _ROWS.extend((family, label, r) for label, r in rows)


def test_few_cases_go_without_a_ring_gate_of_their_own():
    """At most two geometries per op have no output of 3 x 3 or more (there the whole tensor is ring, and the whole-tensor gate,
    which no case goes without, is the ring gate); a geometry run under every stage or both align modes counts once."""
    for family, cases in FF.CASES.items():
        without = {tuple(r64.shape for _, r64 in FF.case(family, p).refs.values()) for p in cases
                   if not any(FF.has_ring(r64.shape) for _, r64 in FF.case(family, p).refs.values())}
        assert len(without) <= 2, (family, without)


def test_one_weight_tap_off_by_a_thousandth_fails_part_b():
    """refinement2.5's first tap x 1.001 in the state dict given to the C restatement only: no end-to-end max-abs gate sees it
    (it moves stage 4 by ~1e-5 px under a floor of 3e-3); the per-op gate does."""
    c = FF.case("refine", (2, 17, 15))
    sd = dict(FF.state_dict()[1])
    w = sd["refinement2.5.weight"].copy()
    w[0, 0, 0, 0] *= np.float32(1.001)
    sd["refinement2.5.weight"] = w
    FF.check(c, {"pred4": C.refine(c.inputs["left"], c.inputs["pred3"], FF.state_dict()[1])})
    with pytest.raises(AssertionError, match="refine .* pred4 - carrier .*off the float32 floor"):
        FF.check(c, {"pred4": C.refine(c.inputs["left"], c.inputs["pred3"], sd)})


def test_the_fp16_rounding_is_numpys():
    x = FF.case("fp16_stage1", (2, 63, 255)).inputs["featL0"]
    x = np.concatenate([x.reshape(-1), np.float32([0.0, -0.0, 65504.0, 65520.0, 1e-8, 6e-8, 2.0 ** -14, 1.00048828125, -3.0e4, 7e4])])
    assert np.array_equal(C.round_fp16(x).view(np.uint32), FF.fp16_round(x).view(np.uint32))


@pytest.mark.parametrize("H,W", [(9, 17), (33, 47)])
def test_sizes_the_reference_cannot_run(H, W):
    """ceil(H/2) not divisible by 4: the hourglass skip-add of the reference (submodules.py:103) meets two sizes, the literal
    restatement raises as the reference would, and the HIP path rejects the same sizes by rule -- stated in the header and in
    lwsnet_amd.synth.check_size here, asserted on the device in tests/test_gpu_float64_floor.py."""
    from lwsnet_amd.synth import check_size
    x = torch.zeros((1, 3, H, W))
    with pytest.raises(RuntimeError):
        O.feature_extraction(x, FF.state_dict()[1])
    with pytest.raises(ValueError, match="divisible by 4"):
        check_size(H, W)
    header = open(os.path.join(ROOT, "include", "lwsnet_hip.h"), encoding="utf-8").read()
    assert "both must be divisible by 4" in header
    source = open(os.path.join(ROOT, "lwsnet_amd", "csrc", "lws_forward.hip"), encoding="utf-8").read()
    assert source.count("size_ok(H, W)") >= 2           # check_size (lws_forward, lws_disparity_stages, lws_reserve) and lws_feature_extraction


def test_zz_worst_ratios_per_op():
    """Prints the table of DESIGN.md section 2 from the gates part B has just run (under -s); nothing new is asserted here."""
    print(f"\n{'worst per op':19s} {'max':>5s} {'mean':>5s} {'ring max':>9s} {'ring mean':>10s}   (gates: {FF.MAX_FACTOR} / {FF.MEAN_FACTOR})")
    for family, r in FF.worst_per_family(_ROWS).items():
        print(f"{family:19s} {r.max:5.2f} {r.mean:5.2f} {r.ring_max:9.2f} {r.ring_mean:10.2f}")


# ------------------------------------------------------------------ part C: end-to-end distributions
_E2E = {}


def c_forward(name):
    if name not in _E2E:
        g, args, sd, align = FF.ref_source_case(name)
        with O.variant(align_mode=align):
            _E2E[name] = (g, C.forward(g["left"], g["right"], sd, tuple(args.maxdisplist)))
    return _E2E[name]


def show_e2e(name, s, st):
    print(f"{name:20s} stage {s + 1}: mean {st.mean_ratio:4.2f} median {st.median_ratio:4.2f} |bias| {st.bias_ratio:4.2f} of the float32 floor; "
          f"within 1e-3 px: {100 * st.within_1e3:6.2f} % (reference float32: {100 * st.floor_within_1e3:6.2f} %)")


@pytest.mark.parametrize("name", FF.E2E_SMOOTH)
def test_e2e_distributions_on_the_smooth_fixtures(name):
    """Per stage, against the reference source's float64 map: the mean of |C - fp64| within 1.3 x, the median within 1.35 x the
    reference source's own float32 statistic, and the mean of the SIGNED error within 0.3 x its mean |error| (measured: <= 1.13,
    <= 1.17, <= 0.14).  The max-abs gates beside this one admit ~6e-4 px of systematic error at stage 4; this admits ~1e-4."""
    g, got = c_forward(name)
    for s in range(4):
        st = FF.assert_e2e_distribution(got[s], g[f"pred{s}"], g[f"pred64_{s}"], f"{name} stage {s + 1}", **FF.E2E_SMOOTH_GATES)
        show_e2e(name, s, st)


def test_e2e_a_constant_offset_of_1e_4_px_fails():
    g, got = c_forward("e2e_64x256")
    args = (g["pred3"], g["pred64_3"], "e2e_64x256 stage 4")
    FF.assert_e2e_distribution(got[3], *args, **FF.E2E_SMOOTH_GATES)
    floor = float(np.abs(g["pred3"].astype(np.float64) - g["pred64_3"]).max())
    planted = (got[3].astype(np.float64) + 1e-4).astype(np.float32)
    assert float(np.abs(planted.astype(np.float64) - g["pred64_3"]).max()) <= 1.25 * floor + 1e-4        # today's max-abs gate lets it through
    with pytest.raises(AssertionError, match=r"\|mean\(build - fp64\)\|, the signed error, is 0\.[3-9]"):
        FF.assert_e2e_distribution(planted, *args, **FF.E2E_SMOOTH_GATES)


@pytest.mark.parametrize("name", FF.E2E_CHAOTIC)
def test_e2e_medians_on_the_chaotic_fixtures(name):
    """The white-noise pair and the uncalibrated-BatchNorm case are SINGLE SAMPLES OF A CHAOTIC MAP (warp -> soft-argmin
    multiplies a sub-ulp difference ~7 x per stage, on inputs without structure): their means ride on a heavy tail (measured up to
    1.35 and 1.59 with correct code), so only the median is gated, at 1.75 x (measured 1.14 and 1.42); the rest is printed."""
    g, got = c_forward(name)
    for s in range(4):
        st = FF.assert_e2e_distribution(got[s], g[f"pred{s}"], g[f"pred64_{s}"], f"{name} stage {s + 1}", **FF.E2E_CHAOTIC_GATES)
        show_e2e(name, s, st)


# ------------------------------------------------------------------ part D: the split-bf16 arithmetic, restated
# The arithmetic of the opt-in numerics mode (option "split_bf16": k_conv3d_mid16x, k_conv3d_mid8x, k_ref_conv64x) on the CPU
# (oracle.lws_oracle.split_conv behind VARIANT["split_bf16"]: each float32 operand as three bf16 values by round to nearest even,
# the six cross terms of mfma_split_bf16_term each one float32 convolution, summed in float32), held to the float32 floor on
# FF.SPLIT_CASES with the project's own factors -- and the same restatement with one of its three 2^-16-order terms left out, which
# must leave the floor where the map exceeds the contraction's footprint and yet stays inside the 2e-5 x scale of
# tests/test_gpu_parity.py::test_split_bf16_*_close_to_the_exact_chain: why the kernels are gated per op by
# tests/test_gpu_float64_floor.py::test_*_split.  No HIP here.
SPLIT = [(family, mask, params) for family, cases in FF.SPLIT_CASES.items() for mask, params in cases]
TEETH = [(f, m, p) for f, m, p in SPLIT if p in FF.SPLIT_TEETH[f]]
_EMU, _EXACT = {}, {}
_SIX, _FIVE = [], []        # (family, label, Ratios) of the gates run here: the table the last test prints


def split_ids(cases):
    return [f"{f}-{FF.split_id(f, m, p)}" for f, m, p in cases]


def emulation(family, mask, params, without=None):
    key = (family, mask, params, without)
    if key not in _EMU:
        _EMU[key] = FF.split_emulation(FF.case(family, params), mask, without)
    return _EMU[key]


# ------------------------------------------------------------------ the split itself
def bf16_rne(x):
    """float32 -> bf16 -> float32 by the bit arithmetic of f2bf_bits (lws_device_math.h), in numpy: round to nearest even."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def split_values():
    rng = np.random.default_rng(11)
    normals = rng.standard_normal(4096).astype(np.float32)
    relu = np.maximum(rng.standard_normal(512).astype(np.float32), 0.0)
    powers = np.float32(2.0) ** np.arange(-100, 101, dtype=np.float32)
    upper = rng.integers(0x0D80, 0x7200, 512).astype(np.uint32) << 16              # bf16 values of 8e-31 .. 2.5e30, even and odd
    ties = np.concatenate([upper | low for low in (0x7FFF, 0x8000, 0x8001)])       # one ulp below a tie, the tie, one ulp above
    ties = np.concatenate([ties, ties | 0x80000000]).astype(np.uint32).view(np.float32)
    wide = (np.float32(10.0) ** rng.uniform(-30, 30, 2048).astype(np.float32) * rng.choice(np.float32([-1, 1]), 2048)).astype(np.float32)
    ends = np.float32([0.0, -0.0, 1e-30, -1e-30, 1e30, -1e30, 1.0, -1.0, 1.00390625, 3.0e38])
    return np.concatenate([normals, relu, powers, -powers, ties, wide, ends])


def test_the_split_is_exact():
    """hi + mid + lo == x exactly in float32 (summed smallest first or largest first), each part is a bf16 value (its low 16 bits
    are zero), hi is the round-to-nearest-even bf16 of x by the device header's bit arithmetic, mid that of x - hi and lo that of
    x - hi - mid, and -0.0 / +0.0 keep their signs in hi: seeded normals, ReLU zeros, -0.0, powers of two, values on and one ulp
    either side of a bf16 rounding tie, and magnitudes from 1e-30 to 1e30 (below ~1e-33 the third part would be subnormal: no
    activation or weight of the network is)."""
    x = split_values()
    p = {k: v.numpy() for k, v in O.split_bf16x3(torch.from_numpy(x)).items()}
    for name, v in p.items():
        assert v.dtype == np.float32 and not (v.view(np.uint32) & 0xFFFF).any(), name
        assert np.isfinite(v).all(), name
    assert np.array_equal((p["hi"] + p["mid"]) + p["lo"], x)
    assert np.array_equal(p["hi"] + (p["mid"] + p["lo"]), x)
    assert np.array_equal(p["hi"].astype(np.float64) + p["mid"].astype(np.float64) + p["lo"].astype(np.float64), x.astype(np.float64))
    assert np.array_equal(p["hi"].view(np.uint32), bf16_rne(x).view(np.uint32))                      # the signs of the zeros too
    assert np.array_equal(p["mid"], bf16_rne(x - p["hi"]))
    assert np.array_equal(p["lo"], bf16_rne((x - p["hi"]) - p["mid"]))
    ties = x[(x.view(np.uint32) & 0xFFFF) == 0x8000]
    assert ties.size >= 1024
    up = bf16_rne(ties).view(np.uint32) >> 16
    assert not (up & 1).any()                                                                        # a tie goes to the even neighbour


def test_the_switch_is_a_mask_and_float64_ignores_it():
    """Bit 1 moves the 32 -> 32 layers only (stage 0), bit 2 the 8 -> 8 ones only (stages 1, 2), bit 4 refinement2.0.2 only; a
    float64 run is the same bits under every mask; the switch is restored on exit."""
    _, sd = FF.state_dict()
    c0, c1 = FF.case("conv3d_stack", (0, (1, 9, 17, 33), None, True)), FF.case("conv3d_stack", (1, (1, 9, 17, 33), None, True))
    r = FF.case("refine", (1, 33, 47))
    assert not np.array_equal(emulation("conv3d_stack", 1, c0.params)["cost_out"], c0.refs["cost_out"][0])
    assert not np.array_equal(FF.split_emulation(c1, 2)["cost_out"], c1.refs["cost_out"][0])
    assert not np.array_equal(emulation("refine", 4, r.params)["pred4"], r.refs["pred4"][0])
    assert np.array_equal(FF.split_emulation(c0, 6)["cost_out"], c0.refs["cost_out"][0])
    assert np.array_equal(FF.split_emulation(c1, 5)["cost_out"], c1.refs["cost_out"][0])
    assert np.array_equal(FF.split_emulation(r, 3)["pred4"], r.refs["pred4"][0])
    with torch.no_grad(), O.variant(split_bf16=7):
        cost = torch.as_tensor(c0.inputs["cost"], dtype=torch.float64)[:, None]
        got = (O.post_3dconvs(cost, sd, 0, torch.float64) + cost)[:, 0].numpy()
        got4 = O.refine(torch.as_tensor(r.inputs["left"], dtype=torch.float64), torch.as_tensor(r.inputs["pred3"], dtype=torch.float64), sd,
                        torch.float64).numpy()
    assert np.array_equal(got, c0.refs["cost_out"][1]) and np.array_equal(got4, r.refs["pred4"][1])
    assert "split_bf16" not in O.VARIANT and len(O.SPLIT_TERMS) == 6
    with FF.split_terms_without("mid*mid"):
        assert len(O.SPLIT_TERMS) == 5 and ("mid", "mid") not in O.SPLIT_TERMS
    assert len(O.SPLIT_TERMS) == 6


def test_the_split_cases_share_the_exact_cases_references():
    """A split case IS the exact case of the same parameters (one Case object, references computed once), and none is in CASES'
    own iteration unless the exact tests put it there."""
    for family, mask, params in SPLIT:
        assert FF.case(family, params) is FF.case(family, params)
    assert {p for _, p in FF.SPLIT_CASES["conv3d_stack"] if p[0] == 0} <= set(FF.CASES["conv3d_stack"])
    assert [p for _, p in FF.SPLIT_CASES["refine"]] == FF.CASES["refine"]
    assert "split" not in " ".join(FF.CASES) and set(FF.C_RUNNERS) == set(FF.CASES)
    assert [FF.mid8x_tiles(s) for s in FF.MID8X_SHAPES] == [288, 396, FF.MID8X_MIN_TILES, 240]


# ------------------------------------------------------------------ six terms pass, five do not
@pytest.mark.parametrize("family,mask,params", SPLIT, ids=split_ids(SPLIT))
def test_six_terms_are_on_the_float32_floor(family, mask, params):
    """Whole tensor, border ring and (refine) carrier removed, at FF.MAX_FACTOR / FF.MEAN_FACTOR."""
    c = FF.case(family, params)
    rows = FF.check(c, emulation(family, mask, params), show=print)
    _SIX.extend((family, label, r) for label, r in rows)


@pytest.mark.parametrize("without", FF.ORDER2_TERMS)
@pytest.mark.parametrize("family,mask,params", TEETH, ids=split_ids(TEETH))
def test_five_terms_leave_the_floor(family, mask, params, without):
    """With one 2^-16-order term left out FF.check raises on every case of FF.SPLIT_TEETH (measured 4.5 .. 13.3 x the floor against
    gates of 3.0 / 2.5), and the same output stays within the old per-op gate: for the stack max|got - C restatement| <= 2e-5 x
    max|C restatement| (measured <= 4.3e-6), for refine <= 2e-5 x max(residual, 1) + 2e-5 x 150 (measured <= 4.0e-4 against 3.9e-3).

    No teeth are asserted on the small maps -- stack (1,1,1,1), (2,1,5,1), (1,4,9,31) (7 .. 10 x there, raises, but not listed),
    refine (1,1,1), (1,2,3), (2,17,15), (3,5,70) (at most 3.1 x: most taps of the dilation-8 footprint are padding) -- nor on
    (1,4,60,256), which the device runs on the exact kernel.  DROPPED from the teeth list: the four 8 -> 8 shapes under STAGE 1's
    weights.  There a five-term form measures 3.3 .. 9.7 x the floor (max) and 3.8 .. 9.0 x (mean) and yet passes FF.check on
    (1,7,45,225) without lo*hi (4.11 / 4.07) and hi*lo (7.57 / 7.13), on (2,9,41,353) without lo*hi (3.86 / 4.03) and hi*lo (8.08 /
    7.40) and on (1,4,64,256) without any of the three (3.34 .. 7.70 / 4.98 .. 8.99): that stack's float32 floor is 1e-7 of the
    scale (max 1.3e-6 at scale 13.5), so `tiny` = 4 eps x scale = 6.5e-6 is most of the gate.  The same shapes under stage 2's
    weights (floor 4e-6) are on the list and raise at 9.5 .. 13.3 x."""
    c = FF.case(family, params)
    got = emulation(family, mask, params, without)
    rows = FF.check(c, got, max_factor=float("inf"), mean_factor=float("inf"))
    _FIVE.extend((family, label, r) for label, r in rows)
    for label, r in rows:
        print(f"without {without:8s} " + FF.format_row(c, label, r))
    with pytest.raises(AssertionError, match="off the float32 floor"):
        FF.check(c, got)
    if (family, params) not in _EXACT:
        _EXACT[family, params] = FF.C_RUNNERS[family](c)
    want = _EXACT[family, params]
    if family == "conv3d_stack":
        err, bound = float(np.abs(got["cost_out"] - want["cost_out"]).max()), 2e-5 * float(np.abs(want["cost_out"]).max())
    else:
        resid = float(np.abs(want["pred4"] - c.inputs["pred3"]).max())
        err, bound = float(np.abs(got["pred4"] - want["pred4"]).max()), 2e-5 * max(resid, 1.0) + 2e-5 * 150.0
    print(f"without {without:8s} the old gate: max|got - exact| = {err:.2e} <= {bound:.2e}")
    assert 0.0 < err <= bound                                    # the old gate is blind to it


def test_zz_worst_ratios_per_family():
    """Prints the CPU emulation's lines of DESIGN.md section 2 from the gates run above (under -s): the worst six-term and the
    smallest five-term ratio per family and column; nothing new is asserted."""
    print(f"\n{'CPU emulation':32s} {'max':>5s} {'mean':>5s} {'ring max':>9s} {'ring mean':>10s}   (gates: {FF.MAX_FACTOR} / {FF.MEAN_FACTOR})")
    for family, r in FF.worst_per_family(_SIX).items():
        print(f"{family + ', six terms, worst':32s} {r.max:5.2f} {r.mean:5.2f} {r.ring_max:9.2f} {r.ring_mean:10.2f}")
    for family in dict.fromkeys(f for f, _, _ in _FIVE):
        cols = [min(v for v in col if v is not None) for col in zip(*[r for f, _, r in _FIVE if f == family])]
        print(f"{family + ', five terms, smallest':32s} {cols[0]:5.2f} {cols[1]:5.2f} {cols[2]:9.2f} {cols[3]:10.2f}")
