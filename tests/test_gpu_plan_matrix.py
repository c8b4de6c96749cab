"""Every launch plan of lws_forward against the C oracle's bits at ragged sizes and batches (run with -m gpu on an MI355X).

include/lwsnet_hip.h promises that every option setting returns the same bits.  tests/test_gpu_parity.py checks that at 64x256,
where every plan takes the deferred-map side and the integer-ratio side of the host predicates; the ragged sizes run the default
plan only.  Here the two axes are crossed (tests/plan_matrix.py: 29 plans x 8 shapes x batches 1, 2, 3, 5 and 8), every cell
bit for bit against oracle.c_oracle.forward, and the library's own profiler (lws_profile_read) confirms per cell that the side
of each host predicate the matrix was built to reach is the side the library took (plan_matrix.expected_launches).

The oracle is computed once per (model configuration, shape, pair) and shared by all plans: about 50 single-pair forwards of
0.1 - 0.9 s each.  A batch of B uses pairs 0 .. B-1 of its shape, so the batches of one shape share them too.
"""
import contextlib
import ctypes
import time

import numpy as np
import pytest
import torch

import plan_matrix as pm
from lwsnet_amd.synth import make_batch
from lwsnet_amd.weights import default_args, make_state_dict

pytestmark = pytest.mark.gpu

# model configurations: constructor keywords, and how the C oracle is configured the same way
CONFIGS = {"default": {}, "fp16": {"feature_fp16": True}, "align1": {"interp_align_mode": 1}, "d32": {"maxdisplist": (32, 5, 5)}}

_INPUTS = {}            # (H, W) -> (left, right) numpy, pairs 0 .. 7
_DEV_INPUTS = {}        # (H, W) -> the same on the device
_ORACLE = {}            # (config, H, W, pair) -> the four stage maps [1,1,H,W] of that pair
_WANT = {}              # (config, H, W, B) -> the four stage maps [B,1,H,W] on the device
_STATS = {"oracle_s": 0.0, "oracle_calls": 0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield torch.device("cuda:0")
    print(f"\nplan matrix: C oracle {_STATS['oracle_calls']} single-pair forwards, {_STATS['oracle_s']:.1f} s in all")


@pytest.fixture(scope="module")
def sd():
    return make_state_dict(7)


def inputs(H, W, dev):
    if (H, W) not in _INPUTS:
        _INPUTS[(H, W)] = make_batch(8, H, W, 1000 + 7 * H + W)
        _DEV_INPUTS[(H, W)] = tuple(torch.as_tensor(a).to(dev) for a in _INPUTS[(H, W)])
    return _DEV_INPUTS[(H, W)]


def want_bits(config, H, W, B, dev, sd):
    """The oracle's four stage maps of pairs 0 .. B-1, on the device; each pair is computed once (the forward is per sample)."""
    from oracle import c_oracle as C, lws_oracle as O
    key = (config, H, W, B)
    if key not in _WANT:
        inputs(H, W, dev)
        left, right = _INPUTS[(H, W)]
        kw = CONFIGS[config]
        for i in range(B):
            if (config, H, W, i) not in _ORACLE:
                t0 = time.perf_counter()
                with O.variant(align_mode=1) if kw.get("interp_align_mode") == 1 else contextlib.nullcontext():
                    _ORACLE[(config, H, W, i)] = C.forward(left[i:i + 1], right[i:i + 1], sd, tuple(kw.get("maxdisplist", (24, 5, 5))),
                                                           feature_fp16=bool(kw.get("feature_fp16", False)))
                _STATS["oracle_s"] += time.perf_counter() - t0
                _STATS["oracle_calls"] += 1
        _WANT[key] = [torch.as_tensor(np.concatenate([_ORACLE[(config, H, W, i)][s] for i in range(B)])).to(dev) for s in range(4)]
    return _WANT[key]


@pytest.fixture(scope="module")
def matrix_oracle(dev, sd):
    """The oracle of the whole matrix, once, before the first plan (so that no plan's test carries its cost)."""
    for H, W in pm.WALK:
        for B in pm.BATCHES[(H, W)]:
            want_bits("default", H, W, B, dev, sd)


def new_model(dev, sd, plan, config="default"):
    from lwsnet_amd.models import LWSNet
    m = LWSNet(default_args(**CONFIGS[config]), device=dev).set_state_dict(sd).eval()
    for k, v in plan.items():
        m.set_option(k, v)
        assert m.get_option(k) == v
    return m


def diff_bits(got, want, what, bad):
    """Appends one line per (pair, stage) of `got` that is not `want` bit for bit."""
    for s in range(4):
        if torch.equal(got[s], want[s]):
            continue
        for i in range(want[s].shape[0]):
            g, w = got[s][i].cpu().numpy(), want[s][i].cpu().numpy()
            n = int((g != w).sum())
            if n:
                bad.append(f"{what} pair {i} stage {s + 1}: {n}/{w.size} elements differ, max abs {np.abs(g - w).max():.3e}")


def launch_counts(m, hip_lib, run):
    """The per-class launch counts of run() under the profiler, and what run() returned."""
    from lwsnet_amd import _lib
    tot = (ctypes.c_double * _lib.LWS_KC_COUNT)()
    cnt = (ctypes.c_int64 * _lib.LWS_KC_COUNT)()
    _lib.check(hip_lib.lws_profile_enable(m._h, -1))
    try:
        out = run()
        torch.cuda.synchronize()
        _lib.check(hip_lib.lws_profile_read(m._h, tot, cnt))
    finally:
        _lib.check(hip_lib.lws_profile_enable(m._h, 0))
    got = {hip_lib.lws_kernel_class_name(k).decode(): int(cnt[k]) for k in range(_lib.LWS_KC_COUNT)}
    got["volume_l1_shift+conv3d_first"] = got["volume_l1_shift"] + got["conv3d_first"]
    return {k: got[k] for k in pm.MODELLED_CLASSES}, out


def diff_counts(got, exp, what, bad):
    if any(got[k] != exp[k] for k in pm.MODELLED_CLASSES):
        delta = {k: (got[k], exp[k]) for k in pm.MODELLED_CLASSES if got[k] != exp[k]}
        sides = {k: exp[k] for k in ("defers", "integer_ratio", "fuse_ref_last", "nchunks", "pipe")}
        bad.append(f"{what}: launch counts (profiler, model) differ: {delta}; the model took {sides}")


def report(bad):
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:40])


# ------------------------------------------------------------------ a, b: every plan over the whole matrix
@pytest.mark.parametrize("plan", pm.PLANS, ids=pm.plan_id)
def test_plan_holds_the_oracles_bits_at_every_shape_and_batch(dev, hip_lib, sd, matrix_oracle, plan):
    """One handle carries the plan through the shapes in the order large, small, large (a workspace sized for the largest serves
    the smallest, stale; the geometry changes under a non-default plan).  Every cell -- batches 1, 2, 3, 5, and 8 at 15x191 --
    runs twice back to back and once more under the profiler: the four stage maps of all three runs are the C oracle's bits for
    every pair, and the profiler's per-class launch counts are those of plan_matrix.expected_launches, i.e. the cell took the
    side of defers() / the integer-ratio test / fuse_ref_last / the chunk count / the pipe that the matrix says it reaches."""
    m = new_model(dev, sd, plan)
    args = default_args()
    bad = []
    for H, W in pm.WALK:
        left, right = inputs(H, W, dev)
        for B in pm.BATCHES[(H, W)]:
            what = f"plan {pm.plan_id(plan)} {H}x{W} B={B}"
            want = want_bits("default", H, W, B, dev, sd)
            first = m(left[:B], right[:B])
            second = m(left[:B], right[:B])                       # back to back: no host synchronisation in between
            diff_bits(first, want, what, bad)
            if not all(torch.equal(a, b) for a, b in zip(first, second)):
                diff_bits(second, want, what + " (second run differs from the first)", bad)
            counts, profiled = launch_counts(m, hip_lib, lambda: m(left[:B], right[:B]))
            diff_counts(counts, pm.expected_launches(plan, args, B, H, W), what, bad)
            if not all(torch.equal(a, b) for a, b in zip(first, profiled)):
                diff_bits(profiled, want, what + " (profiled run differs from the unprofiled)", bad)
    report(bad)


# (lws_forward_conf under the plans is not covered here; tests/test_gpu_confidence.py runs it on the default plan)


# ------------------------------------------------------------------ d: the pool's clones carry the options
@pytest.mark.parametrize("side_streams", [False, True])
def test_pool_clones_carry_the_plan(dev, hip_lib, sd, side_streams):
    """lws_pool_create clones the handle with its options (include/lwsnet_hip.h: frozen at creation).  A non-default plan, an
    odd size with several tile rows, batch 2: three jobs in flight return the oracle's bits."""
    H, W, B = 63, 255, 2
    m = new_model(dev, sd, {"fuse_first": 0, "warp_form": 0, "fuse_ref_last": 1})
    left, right = inputs(H, W, dev)
    want3 = want_bits("default", H, W, 3, dev, sd)
    bad = []
    with m.pool(workers=3, side_streams=side_streams) as pool:
        jobs = [pool.submit(left[i:i + B], right[i:i + B]) for i in (0, 1, 0)]
        for j, (i, job) in enumerate(zip((0, 1, 0), jobs)):
            diff_bits(job.result(), [w[i:i + B] for w in want3], f"pool side_streams={side_streams} job {j} (pairs {i}..{i + 1}) {H}x{W} B={B}", bad)
    report(bad)


# ------------------------------------------------------------------ e: graph capture under a non-default plan
@pytest.mark.parametrize("plan", [{"fuse_last1": 0, "defer_upsample": 0}, {"ref_pipe": 1, "ref_chunk_mb": 1}], ids=pm.plan_id)
def test_graph_capture_under_a_plan(dev, hip_lib, sd, plan):
    """As tests/test_gpu_parity.py::test_graph_capture_replays_the_forward (lws_reserve first, captured on a non-default stream),
    under plans that launch what the default batch-2 plan defers, or that fork the refinement's chunks over two streams, at an
    odd height: the replay, and the replay on a second input set, are the oracle's bits."""
    from lwsnet_amd import _lib
    H, W, B = 23, 200, 2
    if "ref_pipe" in plan:
        e = pm.expected_launches(plan, default_args(), B, H, W)
        assert e["pipe"] and e["nchunks"] == 2                     # (the capture really holds the two-stream refinement)
    m = new_model(dev, sd, plan)
    left, right = inputs(H, W, dev)
    want3 = want_bits("default", H, W, 3, dev, sd)
    lt, rt = left[:B].clone(), right[:B].clone()
    _lib.check(_lib.load().lws_reserve(m._h, B, H, W), "lws_reserve")
    outs = [torch.empty((B, 1, H, W), device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                      # (captures on a side stream of its own)
        m(lt, rt, out=outs)
    for o in outs:
        o.zero_()
    bad = []
    g.replay()
    torch.cuda.synchronize()
    diff_bits(outs, [w[:B] for w in want3], f"graph replay plan {pm.plan_id(plan)} {H}x{W} B={B}", bad)
    lt.copy_(left[1:1 + B])
    rt.copy_(right[1:1 + B])
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    diff_bits(outs, [w[1:1 + B] for w in want3], f"graph replay on new inputs (pairs 1..2) plan {pm.plan_id(plan)} {H}x{W} B={B}", bad)
    diff_bits(m(lt, rt), [w[1:1 + B] for w in want3], f"eager after the capture plan {pm.plan_id(plan)} {H}x{W} B={B}", bad)
    report(bad)


# ------------------------------------------------------------------ f: constructor variants
VARIANT_PLANS = [{}, pm.ALL_OFF_PLAN, {"fuse_ref_last": 1}, {"warp_form": 0}]
VARIANT_SHAPES = {"fp16": ((15, 191), (24, 200)), "align1": ((15, 191), (24, 200)), "d32": ((16, 255), (16, 256))}


@pytest.mark.parametrize("plan", VARIANT_PLANS, ids=pm.plan_id)
@pytest.mark.parametrize("config", sorted(VARIANT_SHAPES))
def test_constructor_variants_under_a_plan(dev, hip_lib, sd, config, plan):
    """fp16 features, interp_align_mode = 1 and maxdisplist (32, 5, 5) (another stage-1 tile and soft-argmin span), each with the
    C oracle configured the same way, at an odd and an even ragged size, batches 1, 2, 3."""
    m = new_model(dev, sd, plan, config)
    bad = []
    for H, W in VARIANT_SHAPES[config]:
        assert pm.size_ok(H, W, default_args(**CONFIGS[config]).maxdisplist[0])
        left, right = inputs(H, W, dev)
        for B in (1, 2, 3):
            diff_bits(m(left[:B], right[:B]), want_bits(config, H, W, B, dev, sd), f"{config} plan {pm.plan_id(plan)} {H}x{W} B={B}", bad)
    report(bad)
