"""The joins of lws_forward / lws_forward_conf, held under a LATE side branch (lws_debug_delay_side, include/lwsnet_hip.h).

tests/test_gpu_stream_order.py stalls the caller's stream, which holds the forks: a side branch that starts before its producer.  It
cannot hold the joins, the caller's stream waiting for the side branch, because the side stream is the handle's.  On an idle device
the side branch is done long before the caller's chain reaches its consumer, so a missing join, a misplaced record or a stage buffer
laid over one the side branch still uses gives the right bits by timing alone.  Here the library delays its own side stream by
STALL_MS at the head of one side segment (or of all of them), and every case follows one pattern:

  the handle's workspace and the outputs are filled with quiet NaN on the caller's stream; the forward runs with the segment
  delayed; all maps are compared bit for bit with the C oracle's (lws_forward_conf: the confidence and sigma maps with those of
  the single-stream plan, which has no join to miss).

A consumer that runs before its join reads the NaN, and so does a late side segment whose input a stage of the caller's chain has
overwritten.  Two more conditions keep a passing case honest: the device time between an event recorded on the caller's stream in
front of the forward and one behind it is at least half the delay (the delay really ran, and the caller's stream really waited for
it; the margin of stream_stall.assert_host_was_held), and where the joins are queued the event behind the forward is not complete
when the call returns.  Every case runs once per stream of stream_stall.caller_streams: a caller stream that shares a hardware queue
with the side stream is held behind the delay by accident.

Segments (LWS_DELAY_*): F4 = conv5, F2 = conv6 + classif1, LEFT = refinement1_left, CHUNKS = the refinement chunks "ref_pipe" puts on
the side stream.  Only the four-chunk plan has the last one; test_the_hook_itself shows that it delays nothing on the others.

profiles/NOTES.md ("stream ordering under a stalled device") says which case fails for which join when that join is removed."""
import contextlib
import ctypes

import pytest

import guarded as G
import stream_stall as SS
from test_gpu_stream_order import (H, PLANS, W, assert_all_bits, forward_call, host, maps_of, new_net, plan, poison_, poisoned, sp,  # noqa: F401
                                   still_poison, dev, net, oracle, pairs, streams)      # (the last five are fixtures)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from lwsnet_amd._lib import LWS_DELAY_ALL as ALL, LWS_DELAY_CHUNKS as CHUNKS, LWS_DELAY_F2 as F2, LWS_DELAY_F4 as F4, LWS_DELAY_LEFT as LEFT  # noqa: E402

DELAY_MS = SS.STALL_MS
SEGMENT_NAMES = {F4: "f4", F2: "f2", LEFT: "left", CHUNKS: "chunks"}
JOIN_BEHIND = {F4: 0, F2: 1, LEFT: 2}       # lws_join_stats' index of the first join behind a delayed segment


def set_delay(net, segments, ms=DELAY_MS):
    from lwsnet_amd import _lib
    _lib.call("lws_debug_delay_side", net._h, int(segments), int(ms * 1000))


@contextlib.contextmanager
def delayed(net, segments, ms=DELAY_MS):
    try:
        set_delay(net, segments, ms)
        yield
    finally:
        set_delay(net, 0, 0)


def segments_of(options):
    """The side segments a plan of PLANS has: the refinement chunks only where "ref_pipe" spreads four chunks over two streams."""
    return (F4, F2, LEFT, CHUNKS) if options.get("ref_pipe") == 1 else (F4, F2, LEFT)


def fill_workspace(net, stream):
    from lwsnet_amd import _lib
    _lib.call("lws_debug_fill_workspace", net._h, ctypes.c_uint32(G.QNAN), sp(stream))


class Run:
    """What one forward left: the maps (numpy), the device milliseconds between the events around it, the host seconds the call
    took, whether the event behind it was complete when the call returned."""


def run_forward(net, dev, lt, rt, stream, conf=False):
    """One forward of the pairs lt, rt on `stream` by the pattern of the module docstring (the delay is the caller's to set)."""
    B = lt.shape[0]
    outs = [poisoned((B, 1, H, W), torch.float32, dev) for _ in range(10 if conf else 4)]
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    r = Run()
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        fill_workspace(net, stream)
        for o in outs:
            poison_(o)
        t0.record(stream)
        _, r.seconds = SS.timed(forward_call, net, lt, rt, outs[:4], stream, *((outs[4:7], outs[7:]) if conf else ()))
        t1.record(stream)
        r.done_at_return = t1.query()
    stream.synchronize()
    r.ms = t0.elapsed_time(t1)
    r.maps = host(outs)
    return r


def assert_delay_ran(r, what, queued=True):
    print(f"{what}: {r.ms:.2f} ms on the device, {r.seconds * 1e3:.2f} ms in the call")
    assert r.ms >= 0.5 * DELAY_MS, f"{what}: {r.ms:.2f} ms between the events around a forward delayed by {DELAY_MS} ms: the caller's stream did not wait"
    if queued:
        assert not r.done_at_return, f"{what}: the forward was complete when the call returned, so no join was held to the delay"


# ================================================================== a. the hook itself
def test_the_hook_itself(dev, net, streams, pairs, oracle):
    """One delayed segment holds the forward between half the delay and MAX_STALL_MS.  Off, with "side_streams" = 0 (no side
    stream: nothing to queue, and no join counted) and for a segment the plan does not have (the refinement chunks of a plan that
    runs one chunk) the forward takes less than half the delay.  A refused call leaves the earlier setting."""
    from lwsnet_amd import _lib
    from test_gpu_host_joins import stats
    lib = _lib.load()
    lt, rt, _, _ = pairs
    want = maps_of(oracle, 0, 1)
    s = streams[0]
    with delayed(net, LEFT):
        for args in ((16, 1000), (-1, 1000), (ALL + 16, 1000), (LEFT, -1), (LEFT, 250001), (1 << 30, 0)):
            assert lib.lws_debug_delay_side(net._h, *args) == _lib.LWS_ERR_INVALID, args
            assert b"lws_debug_delay_side" in lib.lws_last_error()
        assert lib.lws_debug_delay_side(None, LEFT, 1000) == _lib.LWS_ERR_INVALID
        r = run_forward(net, dev, lt[:1], rt[:1], s)                # the refused calls changed nothing: still LEFT, DELAY_MS
        assert_all_bits(r.maps, want, "refinement1_left delayed")
        assert_delay_ran(r, "refinement1_left delayed")
        assert r.ms <= SS.MAX_STALL_MS, r.ms
        with plan(net, dict(side_streams=0)):
            stats(net)
            r = run_forward(net, dev, lt[:1], rt[:1], s)
            assert (stats(net) == 0).all()
        assert_all_bits(r.maps, want, "side_streams = 0")
        assert r.ms < 0.5 * DELAY_MS, f"side_streams = 0: {r.ms} ms"
    for segments, ms in ((0, 0), (LEFT, 0), (0, int(DELAY_MS))):      # each of the three spellings of "off"
        set_delay(net, ALL)
        set_delay(net, segments, ms)
        stats(net)
        r = run_forward(net, dev, lt[:1], rt[:1], s)
        st = stats(net)
        assert_all_bits(r.maps, want, f"off as ({segments}, {ms})")
        assert r.ms < 0.5 * DELAY_MS, f"off as ({segments}, {ms}): {r.ms} ms"
        assert (st[:, 0] + st[:, 1] == 1).all(), st.tolist()        # the joins are there as ever
    with delayed(net, CHUNKS):                                      # four pairs in one chunk: no chunk on the side stream
        r = run_forward(net, dev, lt[:4], rt[:4], s)
    assert_all_bits(r.maps, maps_of(oracle, 0, 4), "the chunks of a one-chunk plan")
    assert r.ms < 0.5 * DELAY_MS, f"the chunks of a one-chunk plan: {r.ms} ms"
    set_delay(net, ALL, SS.MAX_STALL_MS)                            # the largest request is accepted (and not run)
    set_delay(net, 0, 0)


# ================================================================== b, c. plans and segments; queued joins
CASES = [(pid, seg) for pid, (_, options) in PLANS.items() if options.get("side_streams", 1) != 0 for seg in (*segments_of(options), ALL)]


@pytest.mark.parametrize("plan_id,segments", CASES, ids=[f"{p}-{SEGMENT_NAMES.get(s, 'all')}" for p, s in CASES])
def test_forward_joins_wait_for_a_late_side_branch(dev, net, streams, pairs, oracle, plan_id, segments):
    """Every multi-stream plan of PLANS -- batches 1, 2 and 4, both "fork2_after" values, four refinement chunks over two streams,
    every way of resolving the joins -- with each single segment it has delayed, and with all of them.  Where the plan says how
    the joins resolve ("host_joins" = 0, or 1 with no budget), lws_join_stats must have every join queued and none polled."""
    from test_gpu_host_joins import stats
    B, options = PLANS[plan_id]
    lt, rt, _, _ = pairs
    want = maps_of(oracle, 0, B)
    assert segments == ALL or segments in segments_of(options)
    with plan(net, options), delayed(net, segments):
        for i, s in enumerate(streams):
            what = f"{plan_id}, segments {segments}, caller stream {i}"
            stats(net)
            r = run_forward(net, dev, lt[:B], rt[:B], s)
            st = stats(net)
            assert_all_bits(r.maps, want, what)
            assert_delay_ran(r, what)
            assert (st[:, 0] + st[:, 1] == 1).all(), (what, st.tolist())
            if "host_joins" in options:
                assert (st[:, 0] == 0).all() and (st[:, 1] == 1).all() and (st[:, 2] == 0).all(), (what, st.tolist())


# ================================================================== d. joins the host resolves
@pytest.mark.parametrize("segment", [F4, F2, LEFT], ids=["f4", "f2", "left"])
def test_host_resolved_joins_hold_the_host_for_the_delay(dev, net, streams, pairs, oracle, segment):
    """"host_joins" = 1 with a budget of one second: the host polls the first join behind the delayed segment until the segment
    has run -- the call takes at least half the delay, that join's longest poll too -- and no join is queued.  (The event the host
    polls is recorded again by every forward: a query that saw the previous forward's record would return at once.)"""
    from test_gpu_host_joins import stats
    lt, rt, _, _ = pairs
    want = maps_of(oracle, 0, 1)
    j = JOIN_BEHIND[segment]
    with plan(net, dict(host_joins=1, host_join_budget_us=1000000)), delayed(net, segment):
        for i, s in enumerate(streams):
            what = f"segment {segment}, caller stream {i}"
            stats(net)
            r = run_forward(net, dev, lt[:1], rt[:1], s)
            st = stats(net)
            assert_all_bits(r.maps, want, what)
            assert_delay_ran(r, what, queued=False)
            assert r.seconds * 1e3 >= 0.5 * DELAY_MS, f"{what}: the call returned after {r.seconds * 1e3:.2f} ms"
            assert (st[:, 0] == 1).all() and (st[:, 1] == 0).all(), (what, st.tolist())
            assert st[j, 3] >= 0.5 * DELAY_MS * 1e6, (what, st.tolist())


# ================================================================== e. the budget runs out
@pytest.mark.parametrize("segment", [F4, F2, LEFT], ids=["f4", "f2", "left"])
def test_one_forward_spins_for_one_budget_at_the_most(dev, net, streams, pairs, oracle, segment):
    """"host_joins" = 1 with the default budget, 900 us, far below the delay: the first join behind the delayed segment runs out of
    budget and is queued, and every later join of that forward is queued without polling.  The joins in front of the segment may go
    either way."""
    from test_gpu_host_joins import DEFAULT_BUDGET_US, stats
    lt, rt, _, _ = pairs
    want = maps_of(oracle, 0, 1)
    j = JOIN_BEHIND[segment]
    with plan(net, dict(host_joins=1, host_join_budget_us=DEFAULT_BUDGET_US)), delayed(net, segment):
        for i, s in enumerate(streams):
            what = f"segment {segment}, caller stream {i}"
            stats(net)
            r = run_forward(net, dev, lt[:1], rt[:1], s)
            st = stats(net)
            assert_all_bits(r.maps, want, what)
            assert_delay_ran(r, what)
            assert (st[:, 0] + st[:, 1] == 1).all(), (what, st.tolist())
            assert st[j, 0] == 0 and st[j, 1] == 1, (what, st.tolist())
            assert (st[j + 1:, 1] == 1).all() and (st[j + 1:, 2] == 0).all(), (what, st.tolist())
            assert st[:, 2].sum() < 0.5 * DELAY_MS * 1e6, (what, st.tolist())      # nowhere near the delay: the budget held


# ================================================================== f. two forwards back to back
@pytest.mark.parametrize("B", [1, 4])
def test_two_forwards_back_to_back_with_a_late_refinement1_left(dev, net, streams, pairs, oracle, B):
    """No synchronise between them, two different pair sets: the head and the forks of forward n + 1 must not touch what the late
    side branch of forward n still reads (o2, f4, the left image) or writes (o3, cls, f2, r_a, r_c)."""
    lt, rt, _, _ = pairs
    sets = [(lt[:B], rt[:B]), (lt[4:4 + B], rt[4:4 + B])]
    want = [maps_of(oracle, 0, B), maps_of(oracle, 4, B)]
    with delayed(net, LEFT):
        for i, s in enumerate(streams):
            outs = [[poisoned((B, 1, H, W), torch.float32, dev) for _ in range(4)] for _ in sets]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            with torch.cuda.device(dev), torch.cuda.stream(s):
                fill_workspace(net, s)
                for o in outs[0] + outs[1]:
                    poison_(o)
                ev[0].record(s)
                for k, (l, r) in enumerate(sets):
                    forward_call(net, l, r, outs[k], s)
                    ev[k + 1].record(s)
                assert not ev[2].query(), "both forwards were complete when the second call returned"
            s.synchronize()
            for k in range(2):
                what = f"B={B} caller stream {i} forward {'n' if k == 0 else 'n + 1'}"
                assert_all_bits(host(outs[k]), want[k], what)
                ms = ev[k].elapsed_time(ev[k + 1])
                assert ms >= 0.5 * DELAY_MS, f"{what}: {ms:.2f} ms on the device"


# ================================================================== g. lws_forward_conf
_CONF_WANT = {}


def conf_want(net, dev, pairs, oracle, B, stream):
    """The ten maps of the single-stream plan, once per batch; its stage maps are the C oracle's."""
    if B not in _CONF_WANT:
        lt, rt, _, _ = pairs
        with plan(net, dict(side_streams=0)):
            want = run_forward(net, dev, lt[:B], rt[:B], stream, conf=True).maps
        assert_all_bits(want[:4], maps_of(oracle, 0, B), "the single-stream forward_conf against the C oracle")
        assert not any(still_poison(w) for w in want[4:])
        _CONF_WANT[B] = want
    return _CONF_WANT[B]


@pytest.mark.parametrize("segments", [F4, F2, LEFT, ALL], ids=["f4", "f2", "left", "all"])
@pytest.mark.parametrize("B", [1, 4])
def test_forward_conf_joins_wait_for_a_late_side_branch(dev, net, streams, pairs, oracle, B, segments):
    """The plan that keeps every stage's filtered cost: no deferred map, so each stage has its own launches between the joins."""
    lt, rt, _, _ = pairs
    want = conf_want(net, dev, pairs, oracle, B, streams[0])
    with delayed(net, segments):
        for i, s in enumerate(streams):
            what = f"forward_conf B={B}, segments {segments}, caller stream {i}"
            r = run_forward(net, dev, lt[:B], rt[:B], s, conf=True)
            assert_all_bits(r.maps, want, what)
            assert_delay_ran(r, what)


# ================================================================== h. a captured graph
@pytest.mark.parametrize("B", [1, 3])
def test_captured_graph_carries_the_delay_and_its_joins(dev, hip_lib, streams, pairs, oracle, B):
    """Captured with F4, F2 and LEFT delayed, on other pairs than the ones replayed; the hook is switched off before the replays,
    which are late all the same: the delay kernels were captured like every other launch of the side branch, and the joins are the
    graph's edges.  Between replays the workspace is poisoned eagerly on the replay stream (forbidden only while capturing)."""
    lt, rt, _, _ = pairs
    m = new_net(dev, (B, H, W))
    want = maps_of(oracle, 0, B)
    left, right = lt[4:4 + B].clone(), rt[4:4 + B].clone()
    outs = [torch.empty((B, 1, H, W), device=dev) for _ in range(4)]
    assert_all_bits(host(m(left, right)), maps_of(oracle, 4, B), f"B={B}: the eager forward")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with delayed(m, F4 | F2 | LEFT):
        with torch.cuda.graph(g):
            m(left, right, out=outs)
    g.replay()                                                          # once calmly: the graph is instantiated and loaded
    torch.cuda.synchronize()
    left.copy_(lt[:B])
    right.copy_(rt[:B])
    for i, s in enumerate(streams):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            fill_workspace(m, s)
            for o in outs:
                poison_(o)
            t0.record(s)
            g.replay()
            t1.record(s)
            assert not t1.query(), "the replay was complete when it returned"
        s.synchronize()
        assert_all_bits(host(outs), want, f"B={B} replay on caller stream {i}")
        ms = t0.elapsed_time(t1)
        assert ms >= 0.5 * DELAY_MS, f"B={B} replay on caller stream {i}: {ms:.2f} ms on the device"


# ================================================================== i. lws_pool
def test_pool_workers_cloned_from_a_delayed_handle(dev, net, streams, pairs, oracle):
    """Three side-stream workers, created while the handle has F4, F2 and LEFT delayed: lws_clone copies the setting, and the
    workers' joins are queued ("host_joins" = 0 on every worker).  Eight jobs from a ring of three input buffers, each pair's maps
    expected at lws_pool_wait.  One worker runs at least three of the eight jobs, one behind the other, and each job holds that
    worker's side stream for three delays: the eight take at least nine delays, and half of that is asserted."""
    lt, rt, _, _ = pairs
    with delayed(net, F4 | F2 | LEFT):
        pool = net.pool(workers=3, side_streams=True)
    with pool:
        pool.reserve(1, H, W)
        for i, s in enumerate(streams):
            ring = [(poisoned((1, 3, H, W), torch.float32, dev), poisoned((1, 3, H, W), torch.float32, dev)) for _ in range(3)]
            outs = [[poisoned((1, 1, H, W), torch.float32, dev) for _ in range(4)] for _ in range(8)]
            jobs = []
            torch.cuda.synchronize()

            def eight_jobs():
                with torch.cuda.stream(s):
                    for t in range(8):
                        if t >= 3:
                            jobs[t - 3].result()                        # the header's rule for reusing a job's buffers
                        k = (t + i) % 8
                        ring[t % 3][0].copy_(lt[k:k + 1], non_blocking=True)
                        ring[t % 3][1].copy_(rt[k:k + 1], non_blocking=True)
                        jobs.append(pool.submit(*ring[t % 3], out=outs[t]))
                for t in range(8):
                    jobs[t].result()
                    assert_all_bits(host(outs[t]), maps_of(oracle, (t + i) % 8, 1), f"caller stream {i} ticket {t}")

            _, seconds = SS.timed(eight_jobs)
            assert seconds * 1e3 >= 0.5 * 9 * DELAY_MS, f"caller stream {i}: eight delayed jobs on three workers took {seconds * 1e3:.1f} ms"
