"""Host-resolved joins of lws_forward (options "host_joins" / "host_join_budget_us", include/lwsnet_hip.h): whichever way a join
is resolved -- the host polls the side stream's event and queues nothing, or a wait goes on the caller's queue -- the four stage
maps are the same bits, equal to the C oracle.  Shapes: 64x256 with maxdisplist [24, 5, 5], the smallest valid frame; the joins
exist at every size.  lws_join_stats says which way each join went, so the tests also hold the plan to what the header promises:
no polling with "host_joins" = 0, with a zero budget, with "side_streams" = 0 or under hipGraph capture."""
import ctypes

import numpy as np
import pytest
import torch

from lwsnet_amd import _lib
from lwsnet_amd.synth import make_batch
from lwsnet_amd.weights import default_args, make_state_dict

pytestmark = pytest.mark.gpu

H, W = 64, 256
RUN_AHEAD, ISOLATED = 20, 5
DEFAULT_BUDGET_US = 900


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, hip_lib):
    from lwsnet_amd.models import LWSNet
    return LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()


@pytest.fixture(scope="module")
def case(dev):
    """Two pairs and their C-oracle stage maps, computed once as one batch of two (pairs are independent): want[s][b]."""
    from oracle import c_oracle
    left, right = make_batch(2, H, W, 4100)
    want = c_oracle.forward(left, right, make_state_dict(7))
    lt, rt = (torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (left, right))
    return lt, rt, want


def stats(model, reset=True):
    """[join][host-resolved, queued, wait ns, longest wait ns] since the last reset"""
    out = (ctypes.c_int64 * 12)()
    _lib.check(_lib.load().lws_join_stats(model._h, out, 1 if reset else 0), "lws_join_stats")
    return np.array(out[:], dtype=np.int64).reshape(3, 4)


def restore(model):
    for name, v in (("host_joins", -1), ("host_join_budget_us", DEFAULT_BUDGET_US), ("side_streams", 1)):
        model.set_option(name, v)
    stats(model)


def run_both_ways(model, case):
    """RUN_AHEAD forwards without a synchronise in between (the host runs ahead of the device), then ISOLATED forwards with a
    synchronise after each; the two pairs alternate so that a stale map cannot pass.  Returns [(pair index, maps)]."""
    lt, rt, _ = case
    got = []
    for i in range(RUN_AHEAD):
        got.append((i & 1, model(lt[i & 1:(i & 1) + 1], rt[i & 1:(i & 1) + 1])))
    torch.cuda.synchronize()
    for i in range(ISOLATED):
        got.append((i & 1, model(lt[i & 1:(i & 1) + 1], rt[i & 1:(i & 1) + 1])))
        torch.cuda.synchronize()
    return got


@pytest.fixture(scope="module")
def queued_maps(model, case):
    """The stage maps of both pairs on today's plan, "host_joins" = 0 (every join a queued wait)."""
    lt, rt, _ = case
    try:
        model.set_option("host_joins", 0)
        maps = [[p.cpu().numpy() for p in model(lt[b:b + 1], rt[b:b + 1])] for b in range(2)]
    finally:
        restore(model)
    return maps


# (host_joins, host_join_budget_us); a budget of one second: the host path then cannot miss unless the device stalls for a second
PLANS = [(0, DEFAULT_BUDGET_US), (1, 1000000), (-1, DEFAULT_BUDGET_US), (1, 0)]


@pytest.mark.parametrize("host_joins,budget", PLANS, ids=["queued", "host", "automatic", "budget0"])
def test_forward_b1_same_bits_however_the_joins_resolve(model, case, queued_maps, host_joins, budget):
    _, _, want = case
    try:
        model.set_option("host_joins", host_joins)
        model.set_option("host_join_budget_us", budget)
        assert model.get_option("host_joins") == host_joins and model.get_option("host_join_budget_us") == budget
        stats(model)
        got = run_both_ways(model, case)
        st = stats(model)
    finally:
        restore(model)
    n = RUN_AHEAD + ISOLATED
    print(f"host_joins={host_joins} budget={budget}: [host, queued, wait ns, longest ns] per join = {st.tolist()}")
    assert (st[:, 0] + st[:, 1] == n).all(), st
    if host_joins == 0 or budget == 0:
        assert (st[:, 0] == 0).all() and (st[:, 2] == 0).all(), st       # never polled
    if host_joins == 1 and budget == 1000000:
        assert (st[:, 0] == n).all(), st                                  # nothing was queued
    for k, (b, maps) in enumerate(got):
        for s in range(4):
            a = maps[s].cpu().numpy()
            assert np.array_equal(a, queued_maps[b][s]), f"forward {k}, stage {s + 1}: differs from host_joins = 0"
            assert np.array_equal(a[0], want[s][b]), f"forward {k}, stage {s + 1}: differs from the C oracle"


def test_forward_b2_forced_on(model, case):
    """Batch 2 is outside the automatic range: -1 queues every join, 1 polls; both give the oracle's bits."""
    lt, rt, want = case
    try:
        stats(model)
        auto = [p.cpu().numpy() for p in model(lt, rt)]
        st_auto = stats(model)
        model.set_option("host_joins", 1)
        model.set_option("host_join_budget_us", 1000000)
        got = [[p.cpu().numpy() for p in model(lt, rt)] for _ in range(3)]
        st = stats(model)
    finally:
        restore(model)
    assert (st_auto[:, 0] == 0).all() and (st_auto[:, 1] == 1).all(), st_auto
    assert (st[:, 0] == 3).all() and (st[:, 1] == 0).all(), st
    for s in range(4):
        assert np.array_equal(auto[s], want[s]), f"automatic, stage {s + 1}"
        for maps in got:
            assert np.array_equal(maps[s], want[s]), f"host_joins = 1, stage {s + 1}"


def test_graph_capture_keeps_event_waits(model, case, dev):
    """An event query is illegal while a stream captures, so with "host_joins" = 1 the capture must succeed, count three queued
    joins and no poll, and the replayed maps must equal the eager ones."""
    lt, rt, want = case
    try:
        model.set_option("host_joins", 1)
        model.set_option("host_join_budget_us", 1000000)
        l1, r1 = lt[:1].clone(), rt[:1].clone()
        eager = [p.clone() for p in model(l1, r1)]
        _lib.check(_lib.load().lws_reserve(model._h, 1, H, W), "lws_reserve")
        outs = [torch.empty((1, 1, H, W), device=dev) for _ in range(4)]
        torch.cuda.synchronize()
        stats(model)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            model(l1, r1, out=outs)
        st = stats(model)
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for s in range(4):
            assert torch.equal(outs[s], eager[s]), f"replay, stage {s + 1}"
        l1.copy_(lt[1:2])
        r1.copy_(rt[1:2])
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        for s in range(4):
            assert np.array_equal(outs[s].cpu().numpy()[0], want[s][1]), f"replay on the other pair, stage {s + 1}"
        again = model(l1, r1)                     # the eager path polls again afterwards
        st_after = stats(model)
        for s in range(4):
            assert np.array_equal(again[s].cpu().numpy()[0], want[s][1]), f"eager after the capture, stage {s + 1}"
    finally:
        restore(model)
    assert (st[:, 0] == 0).all() and (st[:, 1] == 1).all() and (st[:, 2] == 0).all(), st
    assert (st_after[:, 0] == 1).all(), st_after


def test_single_stream_plan_has_nothing_to_join(model, case):
    lt, rt, want = case
    try:
        model.set_option("side_streams", 0)
        model.set_option("host_joins", 1)
        stats(model)
        got = [p.cpu().numpy() for p in model(lt[:1], rt[:1])]
        st = stats(model)
    finally:
        restore(model)
    assert (st == 0).all(), st
    for s in range(4):
        assert np.array_equal(got[s][0], want[s][0]), f"stage {s + 1}"


def test_automatic_never_holds_a_thread_that_rotates_handles(model, case, dev):
    """Automatic is on only when the thread's previous forward ran on the same handle: two handles in turn queue every join
    (include/lwsnet_hip.h), the same handle twice in a row polls again; the bits are the oracle's either way."""
    from lwsnet_amd import ops
    lib = _lib.load()
    lt, rt, want = case
    c = ctypes.c_void_p()
    out = (ctypes.c_int64 * 12)()
    try:
        with torch.cuda.device(dev):
            _lib.check(lib.lws_clone(model._h, ctypes.byref(c)), "lws_clone")
            stats(model)
            got = []
            for i in range(6):                                  # clone first: the model ran this thread's latest forward
                got.append(ops.forward(c, lt[:1], rt[:1]) if i % 2 == 0 else model(lt[:1], rt[:1]))
            st_rot = stats(model)
            # the same handle as the call before: polls.  Idle device and a budget of one second, so that how the joins resolve
            # does not depend on how much is still queued (an exhausted budget would queue the forward's later joins unpolled)
            torch.cuda.synchronize()
            model.set_option("host_join_budget_us", 1000000)
            got.append(model(lt[:1], rt[:1]))
            _lib.check(lib.lws_join_stats(model._h, out, 1), "lws_join_stats")
            torch.cuda.synchronize()
        st_same = np.array(out[:], dtype=np.int64).reshape(3, 4)
        for k, maps in enumerate(got):
            for s in range(4):
                assert np.array_equal(maps[s].cpu().numpy()[0], want[s][0]), f"forward {k}, stage {s + 1}"
    finally:
        restore(model)
        if c:
            torch.cuda.synchronize()
            lib.lws_destroy(c)
    assert (st_rot[:, 0] == 0).all() and (st_rot[:, 1] == 3).all() and (st_rot[:, 2] == 0).all(), st_rot
    assert (st_same[:, 0] == 1).all() and (st_same[:, 1] == 0).all() and (st_same[:, 2] > 0).all(), st_same


def test_clone_carries_both_options(model, dev):
    """lws_clone needs a finalized source, which needs a device: the host-side half is tests/test_host_joins_cpu.py."""
    lib = _lib.load()
    c = ctypes.c_void_p()
    v = ctypes.c_int(0)
    try:
        model.set_option("host_joins", 1)
        model.set_option("host_join_budget_us", 123)
        with torch.cuda.device(dev):
            _lib.check(lib.lws_clone(model._h, ctypes.byref(c)), "lws_clone")
        assert lib.lws_get_option(c, b"host_joins", ctypes.byref(v)) == 0 and v.value == 1
        assert lib.lws_get_option(c, b"host_join_budget_us", ctypes.byref(v)) == 0 and v.value == 123
    finally:
        restore(model)
        if c:
            lib.lws_destroy(c)
