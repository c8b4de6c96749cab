"""tools/benchkit.py on a real device: the window loop, the shader-clock helper and the profiler helper of the per-op benchmark
tools.  Small on purpose: the model runs at batch 1 and 8 x 192, the smallest size the forward takes with the default arguments
(ceil(W / 2) / 4 >= 24); the tools themselves (368 x 1232, batch 8, tens of seconds each) are not run here."""
import ctypes
import importlib.util
import math
import os

import pytest
import torch

_spec = importlib.util.spec_from_file_location("benchkit", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "benchkit.py"))
benchkit = importlib.util.module_from_spec(_spec)       # by path: tools/ stays off sys.path
_spec.loader.exec_module(benchkit)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(hip_lib):
    return benchkit.seeded_model()


@pytest.fixture(scope="module")
def pair():
    from lwsnet_amd.synth import make_batch
    return make_batch(1, 8, 192, 3)[:2]


def test_window_loop_on_the_device():
    x = torch.zeros((1,), device=benchkit.DEV)
    torch.cuda.synchronize()
    us = benchkit.windows(lambda k: x.add_(1.0), 4, 3)
    assert len(us) == 3 and us == sorted(us) and all(math.isfinite(v) and v > 0.0 for v in us)
    assert float(x) == 12.0                                           # 3 windows of 4 calls, every one on the device


def test_clock_helper_leaves_stamping_off(model, pair):
    before = [p.clone() for p in model(*pair)]
    ghz = benchkit.clock_ghz(model, lambda: model(*pair))
    assert ghz is None or (ghz > 0.0 and ghz == round(ghz, 3))
    after = model(*pair)
    assert all(torch.equal(a, b) for a, b in zip(after, before))


def test_profiler_helper_counts_and_switches_off(model, pair, hip_lib):
    from lwsnet_amd import _lib
    classes = benchkit.profiled(model, lambda: model(*pair), 2)
    for name in ("conv3d_first", "conv3d_mid16", "conv3d_mid8", "conv3d_last"):
        total_ms, launches = classes[name]
        assert launches > 0 and launches % 2 == 0 and total_ms > 0.0, (name, classes)
    assert all(launches > 0 for _, launches in classes.values())
    with benchkit.profiler(model):
        model(*pair)
        torch.cuda.synchronize()
        each = benchkit.profile_each(model, "conv3d_mid8")
        assert len(each) == benchkit.profile_read(model)["conv3d_mid8"][1] == classes["conv3d_mid8"][1] // 2 and all(ms > 0.0 for ms in each)
    # off again: enabling and disabling both clear the records, so a forward after the helper leaves nothing to read
    model(*pair)
    torch.cuda.synchronize()
    tot = (ctypes.c_double * _lib.LWS_KC_COUNT)()
    cnt = (ctypes.c_int64 * _lib.LWS_KC_COUNT)()
    _lib.check(hip_lib.lws_profile_read(model._h, tot, cnt))
    assert sum(cnt) == 0
