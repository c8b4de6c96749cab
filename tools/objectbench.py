#!/usr/bin/env python3
"""lws_objects beside lws_stixels, timed with device events (development aid, not the judged bench).

    python tools/objectbench.py [--iters N] [--runs R]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/objectbench.py --iters 50 --runs 1      # the k_ob_* kernels one by one

The map is stage 4 of the seeded model (seed 7) behind forward_occ at 1 x 368 x 1232; ops.ground gives its codes and heights and
ops.stixels(udisp=True) its histogram, all with their defaults (width 8, sub 4, 768 bins).  Then each of the two C calls alone, on
buffers allocated once: a warm-up, and R windows of N calls between two events; the median window, per call.  lws_stixels is the
yardstick: its kernel is what it was before lws_objects existed.  Prints one JSON line with the times, what the objects call found
and the shader clock the device held during the forward (lws_clock_read)."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(call, iters, runs):
    """The median over `runs` windows of `iters` calls between two device events, in microseconds per call, with min and max."""
    us = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            call()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1000.0 / iters)
    return {"us": round(float(np.median(us)), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/objectbench.py needs a HIP device")
    from lwsnet_amd import _lib, ops
    from lwsnet_amd.geometry import Camera, camera_rows
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.synth import make_pair
    from lwsnet_amd.weights import default_args, make_state_dict
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, H, W = 1, 368, 1232
    model = LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()
    left, right = (x[None] for x in make_pair(H, W, 0)[:2])
    cams = [Camera(721.5377, 721.5377, 609.5593, 172.854, 0.54)]
    res = model.forward_occ(left, right, tau=1.0, fill=False)
    ghz = None
    if lib.lws_clock_stamp(model._h, 1) == _lib.LWS_OK:
        model.forward_occ(left, right, tau=1.0, fill=False)
        v = ctypes.c_double(0.0)
        if lib.lws_clock_read(model._h, ctypes.byref(v)) == _lib.LWS_OK:
            ghz = round(v.value, 3)
        lib.lws_clock_stamp(model._h, 0)
    disp = res.disp[3].as_subclass(torch.Tensor).contiguous()
    g = ops.ground(disp, cams, res.mask[3])
    st = ops.stixels(disp, cams, g.codes, g.height, udisp=True)
    ob = ops.objects(disp, cams, g.codes, st.udisp)
    width, sub, nbins = 8, 4, st.udisp.shape[2]
    S = st.udisp.shape[1]
    cam = torch.from_numpy(camera_rows(cams, B)).to(dev)
    work = torch.empty((_lib.nbytes("lws_objects_workspace", B, W, width, nbins),), device=dev, dtype=torch.uint8)
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    inf = float("inf")

    def stixels():
        _lib.call("lws_stixels", P(disp), P(cam), P(g.codes), P(g.height), B, H, W, 1.0, inf, 1 << 2, width, sub, nbins, 1, 2 * width, width // 2, 2,
                  2, P(st.rows), P(st.vals), P(st.udisp), stream)

    def objects(labels=ob.labels):
        _lib.call("lws_objects", P(disp), P(cam), P(g.codes), P(st.udisp), B, H, W, 1.0, inf, 1 << 2, width, sub, nbins, width, 64, 256, P(work),
                  P(ob.rows), P(ob.vals), P(labels), P(ob.info), stream)

    line = {"tool": "objectbench", "geometry": f"{B}x{H}x{W}", "width": width, "sub": sub, "nbins": nbins, "strips": S, "iters": a.iters,
            "runs": a.runs, "clock_ghz": ghz, "info": ob.info[0].cpu().tolist(), "taking_pixels": int(st.udisp.sum())}
    for name, call in (("stixels", stixels), ("objects", objects), ("objects_without_labels", lambda: objects(None)), ("stixels_again", stixels)):
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        line[name] = timed(call, a.iters, a.runs)
    line["objects_over_stixels"] = round(line["objects"]["us"] / line["stixels"]["us"], 2)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
