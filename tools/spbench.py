#!/usr/bin/env python3
"""Device time of the speckle filter (development aid, not the judged bench).

    python tools/spbench.py [--iters N] [--forward_iters N] [--inputs KIND ...] [--no_mask]

For each geometry (1 x 368 x 1232, 8 x 256 x 512, 8 x 368 x 1232), mask on, labels and counts on, one JSON line per input
(plateaus with islands, constant, checkerboard, serpentine) and fill (0, 1):
  - us per lws_speckle_filter call and its launches (5 with counts: tile labelling, tile edges, flatten, apply, counts);
  - the byte floor: the compulsory bytes (4 read + 4 written per pixel for the maps, 1 + 1 for the codes, + 4 for the labels) at
    the measured 6.29 TB/s copy rate, the call's time over it, and the bytes the implementation moves (disp and mask are read
    by the tile and the apply kernels: + 5; the parent and size words are written by the tile kernel, read by the flatten and
    apply kernels: + 24 per pixel, more where find walks are long);
  - the forward of the same batch (synthetic weights) and the call's time over it.
The calls rotate over enough distinct buffer sets (> 256 MiB together) that every call streams from HBM rather than from the
Infinity Cache; hipEvents bracket a run of back-to-back calls on one stream, all launches of a call inside; the median of five runs
is reported."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_TBS = 6.29          # MI355X, measured float4 copy rate
FLOOR_BYTES = 4 + 4 + 1 + 1 + 4
MOVED_BYTES = FLOOR_BYTES + 4 + 1 + 24


def timed(call, iters, runs=5):
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(iters):
            call(k)
        e1.record()
        e1.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / iters)
    out.sort()
    return out[len(out) // 2], out


def bench_filter(lib, kind, B, H, W, fill, iters, dev, masked=True):
    import speckle_inputs as I
    from lwsnet_amd import _lib
    px = B * H * W
    ws = int(lib.lws_speckle_workspace(B, H, W))
    set_bytes = px * (4 + 1 + 4 + 1 + 4) + ws
    n = max(2, -(-(512 << 20) // set_bytes))
    base = torch.from_numpy(I.make(kind, B, H, W, 1)).to(dev)
    mask = torch.from_numpy(I.random_mask(B, H, W, 2)).to(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    sets = []
    for _ in range(n):
        ts = (base.clone(), mask.clone(), torch.empty((ws,), dtype=torch.uint8, device=dev), torch.empty_like(base), torch.empty_like(mask),
              torch.empty((B, 1, H, W), dtype=torch.int32, device=dev), torch.empty((B, 3), dtype=torch.int64, device=dev))
        sets.append((ts, [p(t) for t in ts]))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(k):
        d, m, w, o, mo, lab, cnt = sets[k % n][1]
        m = m if masked else None
        _lib.check(lib.lws_speckle_filter(d, m, B, H, W, 0.5, 50, fill, w, o, mo, lab, cnt, st), "lws_speckle_filter")

    for k in range(n + 2):
        call(k)
    torch.cuda.synchronize()
    us, runs = timed(call, iters)
    floor_us = FLOOR_BYTES * px / HBM_TBS / 1e6
    return {"kernel": "lws_speckle_filter", "input": kind, "geometry": f"{B}x{H}x{W}", "mask": masked, "fill": fill, "launches": 5,
            "buffer_sets": n, "us_per_call": round(us, 2), "us_runs": [round(r, 2) for r in runs], "byte_floor_us": round(floor_us, 2),
            "over_byte_floor": round(us / floor_us, 2), "floor_bytes_per_pixel": FLOOR_BYTES, "moved_bytes_per_pixel": MOVED_BYTES,
            "kept_removed": sets[0][0][6].cpu().numpy()[:, 1:].sum(axis=0).tolist()}


def bench_forward(model, B, H, W, iters):
    from lwsnet_amd.synth import make_batch
    left, right = (torch.from_numpy(np.ascontiguousarray(a)).to(model.device) for a in make_batch(B, H, W)[:2])
    for _ in range(3):
        model(left, right)
    torch.cuda.synchronize()
    us, runs = timed(lambda k: model(left, right), iters)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--forward_iters", type=int, default=10)
    ap.add_argument("--inputs", nargs="+", default=["plateaus", "constant", "checkerboard", "serpentine"])
    ap.add_argument("--no_mask", action="store_true", help="mask = NULL (the serpentine then is ONE component: the longest find walks)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/spbench.py needs a HIP device")
    from lwsnet_amd import _lib, build
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    build.build_library()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    model = LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()
    for B, H, W in ((1, 368, 1232), (8, 256, 512), (8, 368, 1232)):
        fwd_us = bench_forward(model, B, H, W, a.forward_iters)
        torch.cuda.empty_cache()
        for kind in a.inputs:
            for fill in (0, 1):
                line = bench_filter(lib, kind, B, H, W, fill, a.iters, dev, not a.no_mask)
                line["forward_ms"] = round(fwd_us / 1e3, 3)
                line["over_forward"] = round(line["us_per_call"] / fwd_us, 4)
                print(json.dumps(line), flush=True)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
