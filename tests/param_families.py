"""Parameter families beyond the seeded generator (tests/test_param_families_cpu.py, tests/test_gpu_param_families.py).

lwsnet_amd.weights.make_state_dict draws every BatchNorm weight from U(0.5, 1.5) and every running variance from U(0.5, 1.5)
(or takes the calibrated ones), so the scale s = gamma / sqrt(var + eps) of every folded BatchNorm the suite has met is positive
and within a factor 3 of 1.  A trained checkpoint has gammas of both signs, exact zeros from pruned channels and variances over
orders of magnitude.  The families here are TRANSFORMS of a seeded state dict (the seed-7 default model, CONSTRUCTORS[k] at seed
13), so the seeded generator, its calibration file and the goldens stay as they are:

  signed   every BatchNorm weight element x -1 with probability 1/2
  pruned   every BatchNorm weight element set to exactly 0.0 with probability 0.15
  spread   every running-variance element x 10 ** U(-1, 1)
  all      the three from one generator, in that order per tensor

Not a family, on purpose: running means far from the data (|mean| >> sqrt(var)).  The folded form fmaf(x, s, beta - mean * s)
cancels there by construction and is legitimately further from float64 than the literal (x - mean) * s + beta.

numpy only: importable where neither torch nor the HIP library is."""
import numpy as np

from lwsnet_amd.weights import state_dict_spec

FAMILIES = ("signed", "pruned", "spread", "all")
PRUNE_P = 0.15
SPREAD_DECADES = 1.0          # variance x 10 ** U(-SPREAD_DECADES, SPREAD_DECADES)


# The per-op cases held under every family, as (op, params of tests/float64_floor.py's `case`): the C restatement on the CPU
# (tests/test_param_families_cpu.py), the HIP kernels on the device (tests/test_gpu_param_families.py, which adds GPU_ONLY_CASES).
# One CONSTRUCTORS entry per stage at (2, D, 7, 19): D = maxdisplist[0] at stage 0, 2 * maxdisplist[stage] - 1 after it.
CASES = [("feature_extraction", (1, 15, 23)), ("feature_extraction", (2, 31, 39)),
         ("refine", (2, 17, 15)), ("refine", (1, 33, 47)),
         ("conv3d_stack", (0, (1, 24, 8, 32), None, True)), ("conv3d_stack", (1, (1, 9, 17, 33), None, True)),
         ("conv3d_stack", (2, (1, 9, 17, 33), None, True)),
         ("conv3d_stack", (0, (2, 16, 7, 19), 0, True)), ("conv3d_stack", (1, (2, 9, 7, 19), 2, True)),
         ("conv3d_stack", (2, (2, 3, 7, 19), 3, True))]
GPU_ONLY_CASES = [("conv3d_stack", (0, (2, 9, 30, 70), None, True))]

# A case is floor-gated only where the C restatement measures <= 0.8 x the project's factors (3.0 max / 2.5 mean) against the
# host's own torch float32 run, because that yardstick moves between hosts (one ratio went 1.00 -> 1.26).
# The cases above that line stay in the bit-exact lists and are NOT held to the floor:
#   all, feature_extraction (1,15,23): mean 2.19 on f8, a 2 x 3 map of 96 elements (max 2.00)
GATED_MAX, GATED_MEAN = 2.4, 2.0
NOT_FLOOR_GATED = {"signed": [], "pruned": [], "spread": [], "all": [("feature_extraction", (1, 15, 23))]}


def floor_gated(family, op, params):
    return (op, params) not in NOT_FLOOR_GATED[family]


def apply(sd, args, family, seed=99):
    """A new state dict: `sd` (untouched) with the family's transform applied to the tensors of state_dict_spec(args), in spec
    order, from np.random.default_rng(seed).  Every tensor is a fresh contiguous float32 array."""
    assert family in FAMILIES, family
    rng = np.random.default_rng(seed)
    out = {k: np.array(v, dtype=np.float32, copy=True) for k, v in sd.items()}
    for key, shape, kind in state_dict_spec(args):
        v = out[key]
        assert v.shape == tuple(shape), (key, v.shape, shape)
        if kind == "bnweight":
            if family in ("signed", "all"):
                v = np.where(rng.random(shape) < 0.5, -v, v)
            if family in ("pruned", "all"):
                v = np.where(rng.random(shape) < PRUNE_P, np.float32(0.0), v)
        elif kind == "bn_variance" and family in ("spread", "all"):
            v = v * (10.0 ** rng.uniform(-SPREAD_DECADES, SPREAD_DECADES, shape))
        out[key] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def bn_prefixes(args):
    """The prefix of every BatchNorm of the model, in spec order."""
    return [key[:-len(".weight")] for key, _, kind in state_dict_spec(args) if kind == "bnweight"]


def with_bn_weights(sd, args, fn):
    """A copy of `sd` whose BatchNorm weights are fn(key, weight): the planted state dicts of the teeth checks."""
    out = dict(sd)
    for key, _, kind in state_dict_spec(args):
        if kind == "bnweight":
            out[key] = np.ascontiguousarray(fn(key, sd[key]), dtype=np.float32)
    return out
