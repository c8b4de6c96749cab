"""tools/benchkit.py, the timing and report kit of the per-op benchmark tools (tools/*bench.py), without a GPU: its pure parts
against values restated from the formulas the tools carried before the kit, the window loop behind a fake event class, and a source
check that no tool states the method a second time."""
import ast
import glob
import importlib.util
import os
import sys

import pytest
import torch

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
_spec = importlib.util.spec_from_file_location("benchkit", os.path.join(TOOLS, "benchkit.py"))       # by path: tools/ stays off sys.path
benchkit = importlib.util.module_from_spec(_spec)
_PATH_BEFORE = list(sys.path)
_spec.loader.exec_module(benchkit)
_PATH_AFTER = list(sys.path)

BENCH_TOOLS = sorted(glob.glob(os.path.join(TOOLS, "*bench.py")))
MIB = 1 << 20


@pytest.mark.parametrize("windows,want", [([7.0], 7.0), ([1.0, 2.0, 3.0, 4.0, 5.0], 3.0), ([1.0, 1.5, 2.0, 4.0, 8.0, 9.0, 9.5], 4.0),
                                          ([1.0, 2.0, 3.0, 4.0], 3.0), ([1.0, 2.0], 2.0)])
def test_median_is_the_sample_at_half_the_length(windows, want):
    """out[len(out) // 2] of the sorted windows: a measured window; the upper middle one for an even count."""
    assert benchkit.median(windows) == want


@pytest.mark.parametrize("set_bytes,want", [(1, 512 * MIB), (512 * MIB, 2), (512 * MIB + 1, 2), (256 * MIB, 2), (128 * MIB, 4),
                                            (128 * MIB + 1, 4), (128 * MIB - 1, 5), (13 * 368 * 1232, 92)])
def test_n_sets_covers_512_mib_with_at_least_two_sets(set_bytes, want):
    """max(2, ceil(512 MiB / set_bytes)); 13 x 368 x 1232 = 5 893 888 bytes go 91.09 times into 536 870 912."""
    assert benchkit.n_sets(set_bytes) == want


def test_traffic_figures_and_their_rounding():
    """5 893 888 bytes in 2.5 us: 2.3575552 TB/s, / 6.29 = 0.37481..., the floor 5.893888 / 6.29 = 0.937025... us, 2.5 / 0.937025 = 2.66802."""
    assert benchkit.HBM_TBS == 6.29
    want = {"tb_per_s": 2.358, "fraction_of_hbm": 0.375, "hbm_floor_us": 0.94}
    got = benchkit.traffic(5893888, 2.5)
    assert got == want and list(got) == list(want)
    got = benchkit.traffic(5893888, 2.5, benchkit.TRAFFIC + ("over_floor",))
    assert got == {**want, "over_floor": 2.67} and list(got)[-1] == "over_floor"
    assert benchkit.traffic(5893888, 2.5, ("fraction_of_hbm", "hbm_floor_us")) == {"fraction_of_hbm": 0.375, "hbm_floor_us": 0.94}


def test_report_shapes_keep_the_keys_of_the_tools():
    us = [10.004, 10.006, 12.346, 20.0, 30.016]
    assert benchkit.per_call(us) == {"us_per_call": 12.35, "us_runs": [10.0, 10.01, 12.35, 20.0, 30.02]}
    line = benchkit.per_call(us, 5893888, benchkit.TRAFFIC + ("over_floor",))
    assert list(line) == ["us_per_call", "us_runs", "tb_per_s", "fraction_of_hbm", "hbm_floor_us", "over_floor"]
    assert line["tb_per_s"] == 0.477 and line["over_floor"] == 13.18       # of the unrounded median: 5.893888 / 12.346, 12.346 / 0.937025
    assert benchkit.summary(us) == {"us": 12.35, "min": 10.0, "max": 30.02}
    assert list(benchkit.summary(us, "_us")) == ["us", "min_us", "max_us"]
    assert benchkit.forward_ms("forward_lr_B", [1000.4, 2000.6, 3000.0]) == {"forward_lr_B_ms": 2.001, "forward_lr_B_ms_runs": [1.0, 2.001, 3.0]}


class FakeEvent:
    """Reads a clock in milliseconds that only the timed call advances."""
    now_ms = 0.0
    log = []

    def __init__(self, enable_timing=False):
        assert enable_timing
        self.t = None

    def record(self):
        self.t = FakeEvent.now_ms
        FakeEvent.log.append("record")

    def synchronize(self):
        assert self.t is not None
        FakeEvent.log.append("synchronize")

    def elapsed_time(self, end):
        return end.t - self.t


@pytest.mark.parametrize("patched", [False, True])
def test_window_loop_with_a_fake_event(monkeypatch, patched):
    """runs x iters calls; k is 0 .. iters - 1 inside every window (what the tools' own loops passed: `for k in range(iters)` per
    window); the windows come back sorted, in microseconds per call."""
    FakeEvent.now_ms, FakeEvent.log = 0.0, []
    runs, iters = 3, 4
    cost_ms = [0.3, 0.1, 0.2]                   # per call, by window
    seen = []

    def call(k):
        FakeEvent.now_ms += cost_ms[len(seen) // iters]
        seen.append(k)

    if patched:
        monkeypatch.setattr(torch.cuda, "Event", FakeEvent)
        got = benchkit.windows(call, iters, runs)
    else:
        got = benchkit.windows(call, iters, runs, event=FakeEvent)
    assert seen == list(range(iters)) * runs
    assert got == sorted(got) and got == pytest.approx([100.0, 200.0, 300.0])
    assert FakeEvent.log == ["record", "record", "synchronize"] * runs
    FakeEvent.now_ms, FakeEvent.log = 0.0, []
    seen.clear()
    assert len(benchkit.windows(call, 2, event=None if patched else FakeEvent)) == 5          # five windows unless told otherwise
    assert seen == [0, 1] * 5
    # device_sync: the whole device is waited for behind the end event's record, not the event
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: FakeEvent.log.append("device"))
    FakeEvent.now_ms, FakeEvent.log = 0.0, []
    seen.clear()
    assert benchkit.windows(call, iters, 1, event=FakeEvent, device_sync=True) == pytest.approx([300.0])
    assert FakeEvent.log == ["record", "record", "device"]


def test_warm_passes_the_running_index(monkeypatch):
    seen = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: seen.append("sync"))
    benchkit.warm(seen.append, 3)
    assert seen == [0, 1, 2, "sync"]


def test_loading_the_kit_leaves_tools_off_the_path():
    """The repository root is on the path of a test session already; loading the kit by its file adds nothing to it."""
    assert benchkit.ROOT in _PATH_BEFORE and _PATH_AFTER == _PATH_BEFORE and TOOLS not in _PATH_AFTER


def test_device_check_names_the_tool(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit) as e:
        benchkit.need_device(os.path.join(TOOLS, "gbench.py"))
    assert str(e.value) == "tools/gbench.py needs a HIP device"


def _names(tree):
    """Every identifier, attribute name and string constant of a module."""
    for node in ast.walk(tree):
        if isinstance(node, ast.Name):
            yield node.id
        elif isinstance(node, ast.Attribute):
            yield node.attr
        elif isinstance(node, ast.Constant) and isinstance(node.value, str):
            yield node.value
        elif isinstance(node, ast.alias):
            yield node.name
            yield node.asname


def test_the_tools_state_the_method_nowhere_else():
    assert len(BENCH_TOOLS) == 23 and os.path.isfile(os.path.join(TOOLS, "benchkit.py"))
    for path in BENCH_TOOLS:
        name = os.path.basename(path)
        with open(path) as f:
            src = f.read()
        compile(src, path, "exec")
        tree = ast.parse(src)
        defs = {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}
        assert not defs & {"timed", "n_sets"}, (name, defs)
        stored = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store)}
        assert "HBM_TBS" not in stored, name
        used = set(_names(tree))
        assert not used & {"Event", "lws_clock_read", "lws_profile_read", "lws_clock_stamp", "lws_profile_enable"}, (name, used)
        imports = {a.name for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom)) for a in n.names}
        assert "benchkit" in imports, name
        siblings = {n.module: {a.name for a in n.names} for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.module.endswith("bench")}
        assert not any(names & {"timed", "n_sets", "HBM_TBS"} for names in siblings.values()), (name, siblings)
