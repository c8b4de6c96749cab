"""What the per-op benchmark tools (tools/*bench.py) share: the one statement of how they time and report.

    import benchkit                      # tools/ is sys.path[0] when a tool runs; importing puts the repository root on sys.path

A tool keeps its inputs, its call bodies, its byte counts and its output line; the method is here:
  - need_device, library, seeded_model: the device check, the (optionally rebuilt) C library and the seeded model (seed 7);
  - warm and windows: `n` warm-up calls and a synchronise, then `runs` windows of `iters` back-to-back calls on the current stream
    between two device events; median picks the reported window;
  - n_sets and HBM_TBS: how many distinct buffer sets a rotating tool needs to stream from HBM, and the rate it compares with;
  - per_call, traffic, summary, forward_ms: the figures of a JSON line and their rounding;
  - clock_ghz; profiler, profile_read, profile_each and profiled: the shader clock of one stamped forward; the library's built-in
    profiler around a block, its per-class totals and per-launch times, and the three as one loop;
  - ptr, stream, KITTI, device_batch: small helpers.
Development aid: the package, the tests' run-time path, bench.py and smoke() import none of this."""
import contextlib
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_TBS = 6.29          # MI355X, measured float4 copy rate
KITTI = (721.5377, 721.5377, 609.5593, 172.854, 0.54)          # fx, fy, cx, cy, baseline of the KITTI camera
DEV = torch.device("cuda:0")
TRAFFIC = ("tb_per_s", "fraction_of_hbm", "hbm_floor_us")      # what traffic() reports unless a tool names its own figures
PROFILE_RECORDS = 65536         # launches the built-in profiler keeps (include/lwsnet_hip.h)


def use_tests():
    """Puts tests/ on sys.path, for the tools that take their inputs from the tests' generators."""
    if os.path.join(ROOT, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests"))


def need_device(tool_file):
    if not torch.cuda.is_available():
        raise SystemExit(f"tools/{os.path.basename(tool_file)} needs a HIP device")


def library(build=False):
    """The loaded C library, rebuilt first where the tool asks for that."""
    from lwsnet_amd import _lib
    if build:
        from lwsnet_amd.build import build_library
        build_library()
    return _lib.load()


def seeded_model(build=False, opts=()):
    """LWSNet with default_args() and the weights of seed 7 on the device, in eval mode; `opts` are name=value launch-plan options."""
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    library(build)
    model = LWSNet(default_args(), device=DEV).set_state_dict(make_state_dict(7)).eval()
    for o in opts:
        name, value = o.split("=")
        model.set_option(name, int(value))
    return model


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_batch(B, H, W):
    """The left and right images of lwsnet_amd.synth.make_batch(B, H, W), resident on the device."""
    import numpy as np
    from lwsnet_amd.synth import make_batch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in make_batch(B, H, W)[:2])


def n_sets(set_bytes):
    """Distinct buffer sets to rotate over: 512 MiB together (twice the Infinity Cache), and at least two."""
    return max(2, -(-(512 << 20) // set_bytes))


def warm(call, n):
    for k in range(n):
        call(k)
    torch.cuda.synchronize()


def windows(call, iters, runs=5, event=None, device_sync=False):
    """`runs` windows of `iters` back-to-back call(k) on the current stream, each between two timing events (`event`:
    torch.cuda.Event unless given); k counts 0 .. iters - 1 inside every window, and a rotating tool picks its buffer set from it.
    The host waits on a window's end event, or with `device_sync` on the whole device, as wbench always did (profiles/NOTES.md).
    Returns the windows' microseconds per call, sorted; median() picks the one a tool reports (for an even `runs` the upper middle
    window, also where a tool once took numpy's median)."""
    event = event or torch.cuda.Event
    out = []
    for _ in range(runs):
        e0, e1 = event(enable_timing=True), event(enable_timing=True)
        e0.record()
        for k in range(iters):
            call(k)
        e1.record()
        torch.cuda.synchronize() if device_sync else e1.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / iters)
    out.sort()
    return out


def median(us):
    """The reported window of windows()'s sorted list: the sample at len // 2, a window that was measured.  For an odd number of
    windows (every default: 5, 7) this is numpy's median; for an even --runs it is the upper middle window, also in the tools that
    once took np.median (objectbench, egomotionbench, temporalbench, tsdfbench) and averaged the two middle windows there."""
    return us[len(us) // 2]


def traffic(set_bytes, us, figures=TRAFFIC):
    """What `set_bytes` moved in `us` microseconds is of the HBM rate, the time that rate would take, and `us` over that time:
    those of tb_per_s, fraction_of_hbm, hbm_floor_us and over_floor that the tool names, in its order."""
    floor_us = set_bytes / HBM_TBS / 1e6
    figure = {"tb_per_s": lambda: round(set_bytes / us / 1e6, 3), "fraction_of_hbm": lambda: round(set_bytes / us / 1e6 / HBM_TBS, 3),
              "hbm_floor_us": lambda: round(floor_us, 2), "over_floor": lambda: round(us / floor_us, 2)}
    return {name: figure[name]() for name in figures}


def per_call(us, set_bytes=None, figures=TRAFFIC):
    """The time fields of a rotating tool's line from windows()'s list, with traffic() of the median where bytes are given."""
    out = {"us_per_call": round(median(us), 2), "us_runs": [round(r, 2) for r in us]}
    if set_bytes is not None:
        out.update(traffic(set_bytes, median(us), figures))
    return out


def summary(us, suffix=""):
    """Median, fastest and slowest window of windows()'s list."""
    return {"us": round(median(us), 2), "min" + suffix: round(us[0], 2), "max" + suffix: round(us[-1], 2)}


def forward_ms(name, us):
    """A forward's windows in milliseconds: <name>_ms and <name>_ms_runs."""
    return {name + "_ms": round(median(us) / 1e3, 3), name + "_ms_runs": [round(r / 1e3, 3) for r in us]}


def clock_ghz(model, forward):
    """The shader clock the device held during one stamped forward() of `model` (lws_clock_read), in GHz to 3 places; None
    where the model cannot stamp.  Stamping is off again afterwards."""
    from lwsnet_amd import _lib
    lib = _lib.load()
    ghz = None
    if lib.lws_clock_stamp(model._h, 1) == _lib.LWS_OK:
        forward()
        v = ctypes.c_double(0.0)
        if lib.lws_clock_read(model._h, ctypes.byref(v)) == _lib.LWS_OK:
            ghz = round(v.value, 3)
        lib.lws_clock_stamp(model._h, 0)
    return ghz


@contextlib.contextmanager
def profiler(model):
    """The library's built-in profiler on every kernel class inside the block, off again (and its records cleared) behind it."""
    from lwsnet_amd import _lib
    lib = _lib.load()
    _lib.check(lib.lws_profile_enable(model._h, -1))
    try:
        yield
    finally:
        _lib.check(lib.lws_profile_enable(model._h, 0))


def profile_read(model):
    """{class name: (total_ms, launches)} of the kernel classes that launched under profiler(), in class order."""
    from lwsnet_amd import _lib
    lib = _lib.load()
    tot = (ctypes.c_double * _lib.LWS_KC_COUNT)()
    cnt = (ctypes.c_int64 * _lib.LWS_KC_COUNT)()
    _lib.check(lib.lws_profile_read(model._h, tot, cnt))
    return {lib.lws_kernel_class_name(kc).decode(): (tot[kc], cnt[kc]) for kc in range(_lib.LWS_KC_COUNT) if cnt[kc]}


def profile_each(model, name):
    """The launches of the kernel class called `name` under profiler(), one by one in launch order, in milliseconds."""
    from lwsnet_amd import _lib
    lib = _lib.load()
    kc = [lib.lws_kernel_class_name(k).decode() for k in range(_lib.LWS_KC_COUNT)].index(name)
    ms = (ctypes.c_float * PROFILE_RECORDS)()
    n = ctypes.c_int(0)
    _lib.check(lib.lws_profile_read_class(model._h, kc, ms, PROFILE_RECORDS, ctypes.byref(n)))
    return ms[:n.value]


def profiled(model, call, iters):
    """profile_read() of `iters` call() under profiler(), synchronised."""
    with profiler(model):
        for _ in range(iters):
            call()
        torch.cuda.synchronize()
        return profile_read(model)
