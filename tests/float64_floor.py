"""The float32 noise floor of ONE network op as a yardstick (tests/test_float64_floor_cpu.py, tests/test_gpu_float64_floor.py,
tools/noise_budget.py --per-op).  One op is not chaotic: its float32 result sits a few 1e-7 of the tensor's scale from its
float64 result, whatever the summation order.  So a candidate (the C restatement, the HIP kernels) is held to

    e = |got - ref64|      against      f = |ref32 - ref64|

where ref32 / ref64 are the literal restatement (oracle/lws_oracle.py) in float32 / float64 on the same inputs: the maximum and
the mean of e may exceed those of f by a fixed factor only -- on the whole tensor and, again, on its border ring alone, where a
padding rule read wrongly is the whole signal and not 1/20 of the pixels.  The yardstick is the reference restatement's own
float32 run, never the code under test.

Also here, because the CPU test, the GPU test and the tool share them: the seeded inputs and literal references of every per-op
case (`case`, one per entry of `CASES`), the C restatement's runners (`C_RUNNERS`), and the distribution gates of the end-to-end
stage maps (`assert_e2e_distribution`) on the committed tests/golden/ref_source_*.npz fixtures; and the cases of the split-bf16
kernels (`SPLIT_CASES`: the same references, the same factors) with the CPU emulation of their arithmetic (`split_emulation`;
tests/test_float64_floor_cpu.py part D, tools/noise_budget.py --split).  Plain numpy / torch-CPU."""
import os
from collections import namedtuple

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
MAX_FACTOR, MEAN_FACTOR = 3.0, 2.5          # 1.79 / 1.68 were the worst of ~70 cases: about 1.5 x headroom over one seeded sample

Ratios = namedtuple("Ratios", ["max", "mean", "ring_max", "ring_mean"])      # ring_*: None where no ring gate applies


def ring_mask(shape, stacked=False):
    """True on the outermost row and column of every H x W plane (the last two extents); for a 5-D tensor, or a 4-D one that
    stacks D slices in its second extent (`stacked`: a cost volume [B,D,h,w]), also on the first and the last D slice."""
    m = np.zeros(shape, bool)
    m[..., 0, :] = m[..., -1, :] = True
    m[..., :, 0] = m[..., :, -1] = True
    if len(shape) == 5 or (stacked and len(shape) == 4):
        m[..., 0, :, :] = m[..., -1, :, :] = True
    return m


def has_ring(shape):
    """A ring gate of its own: both plane extents >= 3 (below that every element lies on the ring: the whole-tensor gate is it)."""
    return len(shape) >= 2 and shape[-1] >= 3 and shape[-2] >= 3


def _ratio(stat_e, stat_f):
    """stat(e) / stat(f); over an exact floor of 0 (D = 1, a 1 x 1 map: `tiny` is then the whole gate) 0 or inf."""
    return float(stat_e) / float(stat_f) if stat_f > 0 else (0.0 if stat_e == 0 else float("inf"))


def assert_on_float32_floor(got, ref32, ref64, what, max_factor=MAX_FACTOR, mean_factor=MEAN_FACTOR, ring=True, stacked=False):
    """max|got - ref64| <= max_factor * max|ref32 - ref64| + tiny and the same for the mean with mean_factor, tiny =
    4 * eps_fp32 * max|ref64| (an exact floor of 0 -- D = 1, a 1 x 1 map -- then asks for 4 ulp of the scale); with `ring`, and
    both plane extents >= 3, once more over the border ring alone (`ring_mask`).  Shapes must agree and `got` be finite wherever
    ref64 is.  Returns the measured Ratios, stat|got - ref64| / stat|ref32 - ref64| (inf over a floor of 0 that `got` misses)."""
    got, ref32, ref64 = np.asarray(got), np.asarray(ref32), np.asarray(ref64)
    assert ref64.dtype == np.float64, f"{what}: ref64 is {ref64.dtype}"
    assert got.shape == ref32.shape == ref64.shape, f"{what}: shapes differ: got {got.shape}, ref32 {ref32.shape}, ref64 {ref64.shape}"
    assert got.size > 0, f"{what}: empty"
    ok = np.isfinite(ref64)
    bad = ok & ~np.isfinite(got)
    if bad.any():
        first = int(np.flatnonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} element(s) are not finite where the float64 reference is, the first at flat index "
                             f"{first} = {tuple(int(v) for v in np.unravel_index(first, got.shape))}: {got.reshape(-1)[first]!r}")
    assert ok.any(), f"{what}: the float64 reference has no finite element"
    e = np.where(ok, np.abs(got.astype(np.float64) - ref64), 0.0)
    f = np.where(ok, np.abs(ref32.astype(np.float64) - ref64), 0.0)
    tiny = 4.0 * EPS32 * float(np.abs(ref64[ok]).max())
    rmask = ring_mask(got.shape, stacked) if got.ndim >= 2 else np.ones(got.shape, bool)
    worst = int(np.argmax(e))
    where = (f"worst element at flat index {worst} = {tuple(int(v) for v in np.unravel_index(worst, got.shape))} "
             f"({'on' if rmask.reshape(-1)[worst] else 'off'} the border ring): got {got.reshape(-1)[worst]!r}, "
             f"float32 reference {ref32.reshape(-1)[worst]!r}, float64 reference {ref64.reshape(-1)[worst]!r}")

    def gate(sel, region):
        n = int(sel.sum())
        e_max, f_max = float(e[sel].max()), float(f[sel].max())
        e_mean, f_mean = float(e[sel & ok].sum()) / n, float(f[sel & ok].sum()) / n
        r_max, r_mean = _ratio(e_max, f_max), _ratio(e_mean, f_mean)
        if not (e_max <= max_factor * f_max + tiny and e_mean <= mean_factor * f_mean + tiny):
            raise AssertionError(
                f"{what} ({region}, {n} elements): off the float32 floor: max|got - fp64| = {e_max:.3e} against a floor of {f_max:.3e} "
                f"(ratio {r_max:.2f}, gate {max_factor}), mean {e_mean:.3e} against {f_mean:.3e} (ratio {r_mean:.2f}, gate {mean_factor}); "
                f"tiny = {tiny:.1e}; {where}")
        return r_max, r_mean

    whole = gate(ok, "whole tensor")
    on_ring = (None, None)
    if ring and has_ring(got.shape) and (rmask & ok).any():
        on_ring = gate(rmask & ok, "border ring")
    return Ratios(*whole, *on_ring)


# ------------------------------------------------------------------------------------------------
# end to end: distributions of the stage maps
# ------------------------------------------------------------------------------------------------
E2E_SMOOTH = ["e2e_64x256", "e2e_d32_64x320", "e2e_odd_63x255", "e2e_align1_64x256"]
E2E_CHAOTIC = ["e2e_noise_64x256", "e2e_args_32x256"]
E2E_SMOOTH_GATES = dict(mean_factor=1.3, median_factor=1.35, bias_factor=0.3)        # measured <= 1.13 / 1.17 / 0.14
E2E_CHAOTIC_GATES = dict(mean_factor=None, median_factor=1.75, bias_factor=None)     # measured median 1.14 / 1.42

E2EStats = namedtuple("E2EStats", ["mean_ratio", "median_ratio", "bias_ratio", "within_1e3", "floor_within_1e3", "mean_err", "mean_floor"])


def assert_e2e_distribution(build, ref32, ref64, what, mean_factor=1.3, median_factor=1.35, bias_factor=0.3):
    """One stage map of a whole forward against the reference source's float64 run, by the yardstick of its float32 run:
    mean|build - fp64| <= mean_factor * mean|ref32 - fp64|, the same for the median, and |mean(build - fp64)| <= bias_factor *
    mean|ref32 - fp64| (a systematic offset does not average out; noise does).  A factor that is None is measured, not gated.
    Returns the E2EStats, with the fractions of pixels within 1e-3 px of the float64 map."""
    build, ref32, ref64 = np.asarray(build), np.asarray(ref32), np.asarray(ref64)
    assert ref64.dtype == np.float64 and build.shape == ref32.shape == ref64.shape, (what, build.shape, ref32.shape, ref64.shape, ref64.dtype)
    assert np.isfinite(build).all(), f"{what}: not finite"
    d = build.astype(np.float64) - ref64
    e, f = np.abs(d), np.abs(ref32.astype(np.float64) - ref64)
    st = E2EStats(e.mean() / f.mean(), float(np.median(e) / np.median(f)), abs(d.mean()) / f.mean(), float((e <= 1e-3).mean()),
                  float((f <= 1e-3).mean()), float(e.mean()), float(f.mean()))
    missed = [f"{name} is {value:.3f} x the reference's own float32 {of} (gate {factor})"
              for name, of, value, factor in (("the mean of |build - fp64|", "mean", st.mean_ratio, mean_factor),
                                              ("the median of |build - fp64|", "median", st.median_ratio, median_factor),
                                              ("|mean(build - fp64)|, the signed error,", "mean", st.bias_ratio, bias_factor))
              if factor is not None and not value <= factor]
    if missed:
        raise AssertionError(f"{what}: " + "; ".join(missed) + f"; mean floor {st.mean_floor:.3e} px")
    return st


def ref_source_case(name):
    """tests/golden/ref_source_<name>.npz (the reference's own source on a torch-CPU stand-in, float32 and float64 stage maps)
    with the constructor arguments, the state dict and the align mode it was made under."""
    from lwsnet_amd.weights import default_args, make_state_dict
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"ref_source_{name}.npz")
    with np.load(path) as z:
        g = {k: z[k] for k in z.files}
    align = int(g["align_mode"]) if "align_mode" in g else 0
    args = default_args(maxdisplist=tuple(int(v) for v in g["maxdisplist"]), layers_3d=int(g["layers_3d"]),
                        channels_3d=int(g["channels_3d"]), growth_rate=tuple(int(v) for v in g["growth_rate"]), interp_align_mode=align)
    return g, args, make_state_dict(int(g["seed"]), args, calibrated=bool(g["calibrated"])), align


# ------------------------------------------------------------------------------------------------
# per-op cases: seeded inputs and the literal restatement in float32 and float64
# ------------------------------------------------------------------------------------------------
# the constructor settings of tests/test_oracle_cpu.py::test_c_oracle_constructor_sweep_tracks_the_literal_oracle
CONSTRUCTORS = [((16, 2, 6), 2, 8, (4, 2, 1)), ((8, 1, 1), 1, 16, (1, 1, 1)), ((24, 5, 5), 1, 8, (4, 1, 1)), ((12, 4, 2), 3, 8, (2, 2, 2))]

CASES = {
    # N, H, W: f8 down to 1 x 1; odd sizes (ceil(H/2) rule of the stem); batch 3; wide; every resize ragged
    "feature_extraction": [(1, 7, 7), (1, 8, 8), (1, 15, 23), (3, 16, 40), (2, 31, 39), (1, 24, 200), (2, 63, 255)],
    # B, H, W: smaller than every dilation (1 .. 16) up to larger than all of them
    "refine": [(1, 1, 1), (1, 2, 3), (2, 17, 15), (1, 33, 47), (3, 5, 70), (1, 63, 255)],
    # stage, (B, D, h, w), constructor (None: the default) and whether its BatchNorm statistics are calibrated
    "conv3d_stack": ([(s, shape, None, True) for s in (0, 1, 2)
                      for shape in ((1, 1, 1, 1), (2, 1, 5, 1), (1, 4, 9, 31), (2, 9, 30, 70), (1, 24, 8, 32), (1, 32, 9, 48), (1, 9, 17, 33))]
                     + [(s, (2, CONSTRUCTORS[k][0][0] if s == 0 else 2 * CONSTRUCTORS[k][0][s] - 1, 7, 19), k, cal)
                        for k in range(len(CONSTRUCTORS)) for cal in (True, False) for s in (0, 1, 2)]),
    # (B, C, h, w), D
    "volume_l1_shift": [((3, 16, 5, 24), 24), ((1, 16, 9, 37), 24), ((2, 8, 4, 3), 5), ((1, 8, 1, 1), 1)],
    # align mode, B, C, h, w, scale, m, wild: the previous map is (h scale - 1) x (w scale - 1), so no resize ratio is an integer;
    # wild = 60: flows of +-15 px on a 40-wide map, taps off both borders
    "volume_l1_warp": [(am, *c) for am in (0, 1) for c in ((2, 8, 19, 65, 2, 1, 0), (1, 16, 1, 7, 4, 2, 0), (2, 8, 10, 33, 2, 5, 0),
                                                           (1, 16, 7, 21, 8, 5, 0), (1, 8, 12, 40, 2, 5, 60))],
    # (B, D, h, w), start; "extreme": rows 1 and 2 of a 4-row map are the rows of test_softargmin_extreme_costs
    "softargmin": [((2, 9, 3, 5), -4), ((1, 24, 2, 67), 0), ((1, 1, 3, 3), 0), ((1, 32, 2, 5), 0), ("extreme", 0)],
    # align mode, B, h, w, H, W, with prev
    "upsample_add": [(am, *c) for am in (0, 1) for c in ((2, 3, 5, 24, 40, True), (1, 8, 32, 63, 255, True), (1, 8, 32, 63, 255, False),
                                                         (1, 1, 1, 7, 9, True))],
    # B, H, W: stage 1 of the volume path (shift -> Conv3D stack -> soft-argmin -> upsample) from seeded feature maps ...
    "fp16_stage1": [(2, 63, 255)],          # ... rounded to fp16 (feature_fp16, BASELINE config 5)
    "align1_stage1": [(2, 63, 255)],        # ... under align mode 1: the one way to the HIP resize of that mode, which only a handle carries
}
FAMILY_SEED = {name: i + 1 for i, name in enumerate(CASES)}

# The split-bf16 kernels (option "split_bf16": 1 = k_conv3d_mid16x, 2 = k_conv3d_mid8x, 4 = k_ref_conv64x), a dict of their own:
# the C restatement has no split form, so nothing that iterates CASES may meet them.  family -> [(mask, params of `case`)]: the
# references are those of the exact cases (the same Case object where the parameters coincide) -- the mode claims the float32
# chain's accuracy, so its yardstick is the float32 chain's.
#   mask 1, stage 0 (C3 = 32; the tile is 3 x 4 x 16): the seven stage-0 shapes of CASES["conv3d_stack"]
#   mask 2, stages 1 and 2 (C3 = 8; the tile is 3 x 4 x 32 and the kernel runs from 256 tiles per sample), each shape under both
#           stages' weights: 288 tiles with every extent one past a tile edge and an odd width; batch 2 at 396 tiles; exactly 256
#           tiles; 240 tiles (stays on the exact kernel)
#   mask 4: the six shapes of CASES["refine"]
MID8X_SHAPES = ((1, 7, 45, 225), (2, 9, 41, 353), (1, 4, 64, 256), (1, 4, 60, 256))
SPLIT_CASES = {
    "conv3d_stack": ([(1, (0, shape, None, True)) for shape in ((1, 1, 1, 1), (2, 1, 5, 1), (1, 4, 9, 31), (2, 9, 30, 70), (1, 24, 8, 32),
                                                               (1, 32, 9, 48), (1, 9, 17, 33))]
                     + [(2, (stage, shape, None, True)) for stage in (1, 2) for shape in MID8X_SHAPES]),
    "refine": [(4, params) for params in CASES["refine"]],
}
# the shapes whose map exceeds the contraction's footprint and that run a split kernel: there the GPU tests assert that the
# result differs in bits from the exact kernel's ...
SPLIT_LARGE = {
    "conv3d_stack": [(2, 9, 30, 70), (1, 24, 8, 32), (1, 32, 9, 48), (1, 9, 17, 33), (1, 7, 45, 225), (2, 9, 41, 353), (1, 4, 64, 256)],
    "refine": [(1, 33, 47), (1, 63, 255)],
}
# ... and the cases on which a restatement that loses one 2^-16-order cross term leaves the floor (tests/test_float64_floor_cpu.py part D
# asserts it): those shapes, the 8 -> 8 ones under stage 2's weights only (under stage 1's the float32 floor is 1e-7 of the scale
# and `tiny` is most of the gate: see test_five_terms_leave_the_floor)
SPLIT_TEETH = {
    "conv3d_stack": [(0, shape, None, True) for shape in SPLIT_LARGE["conv3d_stack"][:4]]
                    + [(2, shape, None, True) for shape in SPLIT_LARGE["conv3d_stack"][4:]],
    "refine": list(SPLIT_LARGE["refine"]),
}
MID8X_MIN_TILES = 256        # launch_conv3d_mid (lws_conv3d.hip): k_conv3d_mid8x from this many 3 x 4 x 32 tiles per SAMPLE


def mid8x_tiles(shape):
    _, D, h, w = shape
    return -(-w // 32) * -(-h // 4) * -(-D // 3)


def split_id(family, mask, params):
    return f"mask{mask}-{case_id(family, params)}"


def case_id(family, params):
    def flat(v):
        return "x".join(flat(u) for u in v) if isinstance(v, (tuple, list)) else str(v)
    return "-".join(flat(v) for v in params)


class Case:
    """inputs: numpy float32 arrays by name; refs: output name -> (literal float32, literal float64); stacked: the outputs that
    are cost volumes [B,D,h,w]; carrier: output name -> an input it contains additively, gated again with the carrier removed."""

    def __init__(self, family, params, inputs, refs, stacked=(), carrier=None, meta=None):
        self.family, self.params, self.inputs, self.refs = family, params, inputs, refs
        self.stacked, self.carrier, self.meta = set(stacked), dict(carrier or {}), dict(meta or {})
        self.id = case_id(family, params)


_STATE = {}
_FAMILY = None          # the parameter family (tests/param_families.py) that `state_dict` and `case` are under: see `under_family`


class under_family:
    """with under_family("signed"): ... -- inside, `state_dict` gives the seeded state dict transformed by that parameter family
    (tests/param_families.py) and `case` builds and caches its cases under it, so that the builders, the C runners and the
    split emulation serve the families without a second copy.  The ids, seeds and inputs of a case do not depend on the family;
    None is the seeded family itself."""

    def __init__(self, family):
        self.family = family

    def __enter__(self):
        global _FAMILY
        self.saved, _FAMILY = _FAMILY, self.family
        return self

    def __exit__(self, *a):
        global _FAMILY
        _FAMILY = self.saved


def state_dict(constructor=None, calibrated=True, family=False):
    """(args, state dict): the default model's (seed 7) or CONSTRUCTORS[constructor]'s (seed 13); under `family` (default: the one
    of the enclosing `under_family`, else none) transformed by tests/param_families.py."""
    from lwsnet_amd.weights import default_args, make_state_dict
    family = _FAMILY if family is False else family
    key = (constructor, calibrated) if family is None else (constructor, calibrated, family)
    if key not in _STATE:
        if family is not None:
            import param_families
            args, sd = state_dict(constructor, calibrated, None)
            _STATE[key] = (args, param_families.apply(sd, args, family))
        elif constructor is None:
            args = default_args()
            _STATE[key] = (args, make_state_dict(7, args, calibrated=calibrated))
        else:
            mdl, l3, c3, gr = CONSTRUCTORS[constructor]
            args = default_args(maxdisplist=mdl, layers_3d=l3, channels_3d=c3, growth_rate=gr)
            _STATE[key] = (args, make_state_dict(13, args, calibrated=calibrated))
    return _STATE[key]


def _rng(family, params):
    def ints(v):
        if isinstance(v, (tuple, list)):
            return [i for u in v for i in ints(u)]
        if isinstance(v, str):
            return [sum(v.encode())]
        return [int(v) + 1000 if v is not None else 999]
    return np.random.default_rng([FAMILY_SEED[family]] + ints(params))


def literal(fn):
    """fn(T, dtype) -> tensor or tuple of tensors, run in float32 and float64 (T casts a numpy input); -> per output (ref32, ref64)."""
    outs = []
    with torch.no_grad():
        for dt in (torch.float32, torch.float64):
            r = fn(lambda a, dt=dt: torch.as_tensor(np.asarray(a), dtype=dt), dt)
            outs.append([t.numpy() for t in (r if isinstance(r, (tuple, list)) else (r,))])
    return list(zip(*outs))


def _feature_case(params):
    from oracle import lws_oracle as O
    N, H, W = params
    _, sd = state_dict()
    x = _rng("feature_extraction", params).standard_normal((N, 3, H, W)).astype(np.float32)
    refs = literal(lambda T, dt: O.feature_extraction(T(x), sd, dt))
    return Case("feature_extraction", params, {"img": x}, dict(zip(("f8", "f4", "f2"), refs)))


def _refine_case(params):
    from oracle import lws_oracle as O
    B, H, W = params
    _, sd = state_dict()
    rng = _rng("refine", params)
    left = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    pred3 = (rng.random((B, 1, H, W)) * 150.0).astype(np.float32)
    refs = literal(lambda T, dt: O.refine(T(left), T(pred3), sd, dt))
    return Case("refine", params, {"left": left, "pred3": pred3}, {"pred4": refs[0]}, carrier={"pred4": pred3})


def _conv3d_case(params):
    from oracle import lws_oracle as O
    stage, shape, constructor, calibrated = params
    _, sd = state_dict(constructor, calibrated)
    cost = (_rng("conv3d_stack", params).random(shape) * 12.0).astype(np.float32)
    refs = literal(lambda T, dt: (O.post_3dconvs(T(cost)[:, None], sd, stage, dt) + T(cost)[:, None])[:, 0])
    return Case("conv3d_stack", params, {"cost": cost}, {"cost_out": refs[0]}, stacked=["cost_out"])


def _shift_case(params):
    from oracle import lws_oracle as O
    shape, D = params
    rng = _rng("volume_l1_shift", params)
    L, R = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    refs = literal(lambda T, dt: O.build_volume_2d(T(L), T(R), D, dt))
    return Case("volume_l1_shift", params, {"L": L, "R": R}, {"cost": refs[0]}, stacked=["cost"])


def _warp_case(params):
    from oracle import lws_oracle as O
    am, B, C, h, w, scale, m, wild = params
    H, W = h * scale - 1, w * scale - 1
    rng = _rng("volume_l1_warp", params)
    L, R = rng.standard_normal((B, C, h, w)).astype(np.float32), rng.standard_normal((B, C, h, w)).astype(np.float32)
    prev = (rng.random((B, 1, H, W)) * (wild if wild else 30.0) - (wild / 2.0 if wild else 0.0)).astype(np.float32)

    def lit(T, dt):
        wflow = O._scale(O._interp(T(prev), [h, w]) * float(h), H, dt)                       # models.py:119-121
        return wflow[:, 0], O.build_volume_2d3(T(L), T(R), m, wflow, dt)                    # :123

    with O.variant(align_mode=am):
        refs = literal(lit)
    return Case("volume_l1_warp", params, {"L": L, "R": R, "prev": prev}, {"wflow": refs[0], "cost": refs[1]}, stacked=["cost"],
                meta={"align_mode": am, "H": H, "W": W, "m": m})


def softargmin_extreme_rows():
    """The two rows of tests/test_gpu_parity.py::test_softargmin_extreme_costs: exp underflow on all but one hypothesis; one-hot."""
    c = np.zeros((1, 24, 2, 64), np.float32)
    c[0, :, 0, :] = np.linspace(0, 300, 24, dtype=np.float32)[:, None]
    c[0, :, 1, :] = 1e4
    c[0, 7, 1, :] = -1e4
    return c


def _softargmin_case(params):
    from oracle import lws_oracle as O
    shape, start = params
    rng = _rng("softargmin", params)
    if shape == "extreme":
        cost = (rng.random((1, 24, 4, 64)) * 12.0).astype(np.float32)
        cost[:, :, 1:3, :] = softargmin_extreme_rows()
    else:
        cost = (rng.random(shape) * 12.0).astype(np.float32)
    D = cost.shape[1]
    refs = literal(lambda T, dt: O.disparity_regression(torch.softmax(-T(cost), 1), int(start), int(start) + D, dt)[:, 0])
    return Case("softargmin", params, {"cost": cost}, {"low": refs[0]}, meta={"start": float(start)})


def _upsample_case(params):
    from oracle import lws_oracle as O
    am, B, h, w, H, W, with_prev = params
    rng = _rng("upsample_add", params)
    low = (rng.random((B, h, w)) * 20.0).astype(np.float32)
    prev = (rng.random((B, 1, H, W)) * 150.0).astype(np.float32) if with_prev else None

    def lit(T, dt):
        up = O._interp(O._scale(T(low)[:, None] * float(H), h, dt), [H, W])                  # models.py:145-146
        return up + T(prev) if with_prev else up                                            # :148

    with O.variant(align_mode=am):
        refs = literal(lit)
    inputs = {"low": low, "prev": prev} if with_prev else {"low": low}
    return Case("upsample_add", params, inputs, {"up": refs[0]}, carrier={"up": prev} if with_prev else None,
                meta={"align_mode": am, "H": H, "W": W})


def fp16_round(x):
    """float32 -> nearest-even fp16 -> float32 by numpy: what the rounding of feature_fp16 is compared with exactly."""
    with np.errstate(over="ignore"):                     # beyond 65504 + half an ulp fp16 has infinity
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def _stage1_case(family, params):
    from oracle import lws_oracle as O
    B, H, W = params
    args, sd = state_dict()
    am, fp16 = (1, False) if family == "align1_stage1" else (0, True)
    rng = _rng(family, params)
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    shapes = [(B, 16, h2 // 4, w2 // 4), (B, 16, h2 // 2, w2 // 2), (B, 8, h2, w2)]
    inputs = {}
    for side in "LR":
        for i, s in enumerate(shapes):
            inputs[f"feat{side}{i}"] = rng.standard_normal(s).astype(np.float32)
    rl = [fp16_round(inputs[f"featL{i}"]) if fp16 else inputs[f"featL{i}"] for i in range(3)]
    rr = [fp16_round(inputs[f"featR{i}"]) if fp16 else inputs[f"featR{i}"] for i in range(3)]
    with O.variant(align_mode=am):
        refs = literal(lambda T, dt: O.disparity_stages([T(a) for a in rl], [T(a) for a in rr], H, W, sd, list(args.maxdisplist), dt)[0])
    return Case(family, params, inputs, {"pred1": refs[0]}, meta={"H": H, "W": W, "align_mode": am, "feature_fp16": fp16})


_BUILDERS = {"feature_extraction": _feature_case, "refine": _refine_case, "conv3d_stack": _conv3d_case, "volume_l1_shift": _shift_case,
             "volume_l1_warp": _warp_case, "softargmin": _softargmin_case, "upsample_add": _upsample_case, "fp16_stage1": lambda p: _stage1_case("fp16_stage1", p),
             "align1_stage1": lambda p: _stage1_case("align1_stage1", p)}
_CASE = {}


def case(family, params):
    """The Case of CASES[family]'s entry `params` (under the parameter family of the enclosing `under_family`, if any): built
    once, shared by every test that needs it, never modified."""
    key = (family, params) if _FAMILY is None else (family, params, _FAMILY)
    if key not in _CASE:
        _CASE[key] = _BUILDERS[family](params)
    return _CASE[key]


def check(c, outputs, show=None, max_factor=MAX_FACTOR, mean_factor=MEAN_FACTOR):
    """Every output of case `c` (name -> float32 array from the code under test) on the float32 floor, whole tensor and ring; an
    output with a carrier once more with the carrier subtracted from all three (the 150-px map a residual rides on would otherwise
    set the scale term).  Returns [(label, Ratios)]; `show` (print) gets one line per gate."""
    assert set(outputs) == set(c.refs), (c.id, sorted(outputs), sorted(c.refs))
    rows = []
    for name, (r32, r64) in c.refs.items():
        got = np.asarray(outputs[name])
        assert got.dtype == np.float32, f"{c.family} {c.id} {name}: {got.dtype}"
        todo = [(name, got, r32, r64)]
        if name in c.carrier:
            car = c.carrier[name].astype(np.float64)
            todo.append((f"{name} - carrier", got.astype(np.float64) - car, r32.astype(np.float64) - car, r64 - car))
        for label, g, a, b in todo:
            r = assert_on_float32_floor(g, a, b, f"{c.family} {c.id} {label}", max_factor, mean_factor, ring=True, stacked=name in c.stacked)
            rows.append((label, r))
            if show is not None:
                show(format_row(c, label, r))
    return rows


def format_row(c, label, r):
    def v(x):
        return "   -" if x is None else f"{x:4.2f}"
    return f"{c.family:19s} {c.id:28s} {label:18s} max {v(r.max)} mean {v(r.mean)} | ring max {v(r.ring_max)} mean {v(r.ring_mean)}"


# ------------------------------------------------------------------------------------------------
# the split-bf16 arithmetic, restated (oracle.lws_oracle.split_conv behind VARIANT["split_bf16"]); leaving a term out is test-side
# ------------------------------------------------------------------------------------------------
class split_terms_without:
    """with split_terms_without("mid*mid"): ... -- the restatement's split convolutions sum five terms, the named one ("weight
    part*input part") left out: the planted defect of the teeth checks.  None leaves the six."""

    def __init__(self, term):
        self.term = None if term is None else tuple(term.split("*"))

    def __enter__(self):
        from oracle import lws_oracle as O
        self.saved = O.SPLIT_TERMS
        if self.term is not None:
            assert self.term in O.SPLIT_TERMS, self.term
            O.SPLIT_TERMS = tuple(t for t in O.SPLIT_TERMS if t != self.term)
        return self

    def __exit__(self, *a):
        from oracle import lws_oracle as O
        O.SPLIT_TERMS = self.saved


ORDER2_TERMS = ("lo*hi", "hi*lo", "mid*mid")          # weight part * input part: the three cross terms of order 2^-16


def split_emulation(c, mask, without=None):
    """The outputs of case `c` from the literal restatement in float32 with its split convolutions on (`mask`), as `check` takes
    them; `without`: one term of ORDER2_TERMS left out."""
    from oracle import lws_oracle as O

    def T(a):
        return torch.as_tensor(np.asarray(a), dtype=torch.float32)

    _, sd = state_dict(*c.params[2:4]) if c.family == "conv3d_stack" else state_dict()
    with torch.no_grad(), O.variant(split_bf16=mask), split_terms_without(without):
        if c.family == "conv3d_stack":
            cost = T(c.inputs["cost"])[:, None]
            return {"cost_out": (O.post_3dconvs(cost, sd, c.params[0], torch.float32) + cost)[:, 0].numpy()}
        assert c.family == "refine", c.family
        return {"pred4": O.refine(T(c.inputs["left"]), T(c.inputs["pred3"]), sd, torch.float32).numpy()}


# ------------------------------------------------------------------------------------------------
# the C restatement, case by case
# ------------------------------------------------------------------------------------------------
def _c_warp(c):
    from oracle import c_oracle as C
    from oracle import lws_oracle as O
    am, B, _, h, w, _, m, _ = c.params
    with O.variant(align_mode=am):
        wflow = C.resize_bilinear(c.inputs["prev"][:, 0], h, w, float(h), float(np.float32(1) / np.float32(c.meta["H"])))
    return {"wflow": wflow, "cost": C.volume_l1_warp(c.inputs["L"], c.inputs["R"], wflow, m)}


def _c_upsample(c):
    from oracle import c_oracle as C
    from oracle import lws_oracle as O
    with O.variant(align_mode=c.meta["align_mode"]):
        return {"up": C.upsample_add(c.inputs["low"], c.inputs.get("prev"), c.meta["H"], c.meta["W"])}


def stage1_features(c):
    return ([c.inputs[f"feat{side}{i}"] for i in range(3)] for side in "LR")


def _c_stage1(c):
    from oracle import c_oracle as C
    from oracle import lws_oracle as O
    args, sd = state_dict()
    fl, fr = stage1_features(c)
    with O.variant(align_mode=c.meta["align_mode"]):
        return {"pred1": C.disparity_stages(fl, fr, c.meta["H"], c.meta["W"], sd, tuple(args.maxdisplist), feature_fp16=c.meta["feature_fp16"])[0]}


def _c_runners():
    from oracle import c_oracle as C
    return {
        "feature_extraction": lambda c: dict(zip(("f8", "f4", "f2"), C.feature_extraction(c.inputs["img"], state_dict()[1]))),
        "refine": lambda c: {"pred4": C.refine(c.inputs["left"], c.inputs["pred3"], state_dict()[1])},
        "conv3d_stack": lambda c: {"cost_out": C.conv3d_stack(c.inputs["cost"], state_dict(c.params[2], c.params[3])[1], c.params[0])},
        "volume_l1_shift": lambda c: {"cost": C.volume_l1_shift(c.inputs["L"], c.inputs["R"], c.params[1])},
        "volume_l1_warp": _c_warp,
        "softargmin": lambda c: {"low": C.softargmin(c.inputs["cost"], c.meta["start"])},
        "upsample_add": _c_upsample,
        "fp16_stage1": _c_stage1,
        "align1_stage1": _c_stage1,
    }


C_RUNNERS = _c_runners()


def worst_per_family(rows):
    """rows: [(family, label, Ratios)] -> family -> Ratios of the per-column maxima (the table of DESIGN.md section 2); a ratio
    over a floor of exactly 0 (inf: held by `tiny` alone) is left out."""
    out = {}
    for family, _, r in rows:
        cur = out.get(family, Ratios(0.0, 0.0, 0.0, 0.0))
        out[family] = Ratios(*[max(a, b if b is not None and np.isfinite(b) else 0.0) for a, b in zip(cur, r)])
    return out
