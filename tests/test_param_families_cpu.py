"""The C restatement (oracle/lws_oracle.c through oracle/c_oracle.py: the bits the HIP kernels are held to) under the parameter
families of tests/param_families.py -- BatchNorm weights of both signs, exact zeros, variances over two decades -- against the
literal restatement in float64 by the yardstick of its own float32 run (tests/float64_floor.py).  (a) every case of PF.CASES under
every family on the floor with the project's own factors, floor-gated only where it measures <= 0.8 x the factors here; (b) the
gate has teeth: a C restatement handed |gamma| for a signed gamma, or the unpruned gamma for a pruned one, leaves the floor on
every floor-gated case; (c) the fold itself, bit for bit between two restatements, zeros included.  No HIP here; run with -s for
the table of DESIGN.md section 2 ("Beyond the seeded weight family")."""
import numpy as np
import pytest

import float64_floor as FF
import param_families as PF
from lwsnet_amd import weights
from oracle import c_oracle as C

FAMILY_CASES = [(fam, op, params) for fam in PF.FAMILIES for op, params in PF.CASES]
GATED = [(fam, op, params) for fam, op, params in FAMILY_CASES if PF.floor_gated(fam, op, params)]
_ROWS = {}          # (family, op) -> [Ratios]: the table the last test prints


def ids(cases):
    return [f"{fam}-{op}-{FF.case_id(op, params)}" for fam, op, params in cases]


def c_run(c, sd):
    """The C restatement of case `c` under the state dict `sd` (FF.C_RUNNERS takes the case's own)."""
    if c.family == "feature_extraction":
        return dict(zip(("f8", "f4", "f2"), C.feature_extraction(c.inputs["img"], sd)))
    if c.family == "refine":
        return {"pred4": C.refine(c.inputs["left"], c.inputs["pred3"], sd)}
    assert c.family == "conv3d_stack", c.family
    return {"cost_out": C.conv3d_stack(c.inputs["cost"], sd, c.params[0])}


def case_state(op, params, family=False):
    """(args, state dict) that case (op, params) runs under."""
    return FF.state_dict(*params[2:4], family=family) if op == "conv3d_stack" else FF.state_dict(family=family)


def worst(rows):
    """(max ratio, mean ratio) over the whole-tensor and the ring gates of FF.check's rows."""
    return max(max(r.max, r.ring_max or 0.0) for _, r in rows), max(max(r.mean, r.ring_mean or 0.0) for _, r in rows)


# ------------------------------------------------------------------ the families themselves
def test_the_families_are_what_they_say():
    """`apply` leaves its input untouched, changes only the tensors its family names, and really reaches the values the seeded
    generator never gives: both signs, exact +0.0, variances over two decades; `all` is the three from one generator."""
    args, sd = FF.state_dict()
    before = {k: v.copy() for k, v in sd.items()}
    out = {fam: PF.apply(sd, args, fam) for fam in PF.FAMILIES}
    assert all(np.array_equal(sd[k], before[k]) for k in sd) and all(o is not sd for o in out.values())
    kinds = {key: kind for key, _, kind in weights.state_dict_spec(args)}
    gam = {fam: np.concatenate([o[k].reshape(-1) for k in o if kinds[k] == "bnweight"]) for fam, o in out.items()}
    var = {fam: np.concatenate([o[k].reshape(-1) for k in o if kinds[k] == "bn_variance"]) for fam, o in out.items()}
    g0 = np.concatenate([sd[k].reshape(-1) for k in sd if kinds[k] == "bnweight"])
    v0 = np.concatenate([sd[k].reshape(-1) for k in sd if kinds[k] == "bn_variance"])
    assert (g0 > 0).all()
    for fam, o in out.items():
        touched = {kinds[k] for k in o if not np.array_equal(o[k], sd[k])}
        assert touched == {"signed": {"bnweight"}, "pruned": {"bnweight"}, "spread": {"bn_variance"}, "all": {"bnweight", "bn_variance"}}[fam]
        assert all(v.dtype == np.float32 and v.flags["C_CONTIGUOUS"] and v.shape == sd[k].shape for k, v in o.items())
    assert np.array_equal(np.abs(gam["signed"]), g0) and 0.4 < (gam["signed"] < 0).mean() < 0.6
    zeros = gam["pruned"] == 0
    assert 0.10 < zeros.mean() < 0.20 and not np.signbit(gam["pruned"][zeros]).any() and np.array_equal(gam["pruned"][~zeros], g0[~zeros])
    ratio = var["spread"].astype(np.float64) / v0
    assert 0.1 * (1 - 1e-6) <= ratio.min() < 0.15 and 7.0 < ratio.max() <= 10.0 * (1 + 1e-6)
    assert (gam["all"] < 0).any() and (gam["all"] == 0).any() and (gam["all"] > 0).any() and not np.array_equal(var["all"], v0)
    assert np.array_equal(PF.apply(sd, args, "all")["refinement2.0.0.weight"], out["all"]["refinement2.0.0.weight"])      # seeded
    assert len(PF.bn_prefixes(args)) == sum(kind == "bnweight" for kind in kinds.values())


def test_the_family_key_moves_no_existing_case():
    """FF.state_dict's third key and FF.under_family: outside a family everything is what it was (same objects, same ids); inside,
    a case has the id, the seed and the inputs of the seeded one and other references; the family is restored on exit."""
    args, sd = FF.state_dict()
    seeded = FF.case("refine", (2, 17, 15))
    with FF.under_family("signed"):
        a2, sd2 = FF.state_dict()
        c = FF.case("refine", (2, 17, 15))
        assert FF.case("refine", (2, 17, 15)) is c and FF.state_dict(family=None)[1] is sd
        with FF.under_family(None):
            assert FF.state_dict()[1] is sd and FF.case("refine", (2, 17, 15)) is seeded
        assert FF.state_dict()[1] is sd2
    assert FF.state_dict()[1] is sd and FF.case("refine", (2, 17, 15)) is seeded and FF.state_dict(family="signed")[1] is sd2
    assert c is not seeded and c.id == seeded.id and all(np.array_equal(c.inputs[k], seeded.inputs[k]) for k in seeded.inputs)
    assert not np.array_equal(c.refs["pred4"][1], seeded.refs["pred4"][1])
    assert a2.maxdisplist == args.maxdisplist and np.array_equal(sd2["refinement2.5.weight"], sd["refinement2.5.weight"])
    assert all(FF.case_id(op, p) == FF.case(op, p).id for op, p in PF.CASES)
    assert all(p in FF.CASES[op] for op, p in PF.CASES + PF.GPU_ONLY_CASES)


# ------------------------------------------------------------------ (a) the floor under the families
@pytest.mark.parametrize("family,op,params", FAMILY_CASES, ids=ids(FAMILY_CASES))
def test_c_restatement_on_the_float32_floor_under_a_family(family, op, params):
    """FF.check with FF.MAX_FACTOR / FF.MEAN_FACTOR, whole tensor and ring, on every floor-gated case; a case listed in
    PF.NOT_FLOOR_GATED is measured and must be finite (FF.check asserts that whatever the factors)."""
    gated = PF.floor_gated(family, op, params)
    with FF.under_family(family):
        c = FF.case(op, params)
        got = FF.C_RUNNERS[op](c)
        rows = FF.check(c, got, show=print) if gated else FF.check(c, got, show=print, max_factor=float("inf"), mean_factor=float("inf"))
    _ROWS.setdefault((family, op), []).extend(rows)
    mx, mean = worst(rows)
    print(f"{family} {op} {c.id}: worst max {mx:.2f} mean {mean:.2f}" + ("" if gated else "   (not floor-gated)"))
    for name, a in got.items():
        assert np.isfinite(a).all(), name


def test_few_cases_go_without_the_floor_gate():
    """At most one case in five per family, and only cases of PF.CASES."""
    for family in PF.FAMILIES:
        out = PF.NOT_FLOOR_GATED[family]
        assert all(case in PF.CASES for case in out) and len(set(out)) == len(out)
        assert 5 * len(out) <= len(PF.CASES), (family, out)


# ------------------------------------------------------------------ (b) teeth
def planted_state(family, op, params):
    """What the teeth hand to the C restatement in place of the family's state dict: under `signed` the same with |gamma|, under
    `pruned` the zeros put back (which is the seeded state dict: the family touches nothing else)."""
    args, sd = case_state(op, params, family)
    if family == "signed":
        return PF.with_bn_weights(sd, args, lambda key, w: np.abs(w))
    assert family == "pruned", family
    seeded = case_state(op, params, None)[1]
    return PF.with_bn_weights(sd, args, lambda key, w: seeded[key])


TEETH = [(fam, op, params) for fam, op, params in GATED if fam in ("signed", "pruned")]


@pytest.mark.parametrize("family,op,params", TEETH, ids=ids(TEETH))
def test_a_fold_that_ignores_the_family_leaves_the_floor(family, op, params):
    """The literal references are built under the family; a C restatement run with |gamma| (signed) or the unpruned gamma (pruned)
    is what a fold or an epilogue that is right only for s > 0, or parameters gone stale across a swap, would compute: FF.check
    raises on every floor-gated case, and passes on the same case with the family's own state dict."""
    with FF.under_family(family):
        c = FF.case(op, params)
    true_sd, planted = case_state(op, params, family)[1], planted_state(family, op, params)
    FF.check(c, c_run(c, true_sd))
    with pytest.raises(AssertionError, match="off the float32 floor"):
        FF.check(c, c_run(c, planted))
    assert all(np.array_equal(true_sd[k], planted[k]) for k in true_sd if not k.endswith(".weight"))


# ------------------------------------------------------------------ (c) the fold
@pytest.mark.parametrize("family", PF.FAMILIES)
@pytest.mark.parametrize("constructor", [None, 0, 1, 2, 3])
def test_the_fold_is_the_same_bits_in_both_restatements(family, constructor):
    """C.bn_scale_shift (numpy float32 arrays) against lwsnet_amd.weights.bn_scale_shift (one channel at a time through float64,
    rounded per step): s and t bit for bit for every BatchNorm of the model; a pruned channel has s == +-0.0 and t == beta; s
    has gamma's sign; everything is finite."""
    args, sd = FF.state_dict(constructor, True, family)
    pruned = negative = 0
    for p in PF.bn_prefixes(args):
        s, t = C.bn_scale_shift(sd, p)
        s2, t2 = weights.bn_scale_shift(sd, p)
        assert s.dtype == t.dtype == s2.dtype == t2.dtype == np.float32
        assert np.array_equal(s.view(np.uint32), s2.view(np.uint32)) and np.array_equal(t.view(np.uint32), t2.view(np.uint32)), p
        assert np.isfinite(s).all() and np.isfinite(t).all()
        g, beta = sd[p + ".weight"], sd[p + ".bias"]
        zero = g == 0
        assert (s[zero] == 0).all() and np.array_equal(t[zero], beta[zero]) and (s[~zero] != 0).all(), p
        assert np.array_equal(np.sign(s), np.sign(g)), p
        pruned, negative = pruned + int(zero.sum()), negative + int((g < 0).sum())
    assert (pruned > 0) == (family in ("pruned", "all")) and (negative > 0) == (family in ("signed", "all"))


def test_zz_worst_ratios_per_family_and_op():
    """Prints the C-restatement rows of DESIGN.md section 2, "Beyond the seeded weight family" (under -s); nothing new is asserted."""
    print(f"\n{'family':8s} {'op':19s} {'max':>5s} {'mean':>5s}   (whole tensor and ring; gates {FF.MAX_FACTOR} / {FF.MEAN_FACTOR}, "
          f"floor-gated up to {PF.GATED_MAX} / {PF.GATED_MEAN})")
    for (family, op), rows in _ROWS.items():
        mx, mean = worst(rows)
        print(f"{family:8s} {op:19s} {mx:5.2f} {mean:5.2f}")
