#!/usr/bin/env python3
"""Device time of lws_stage_metrics (both launches) at the evaluation geometries (development aid, not the judged bench).

    python tools/mbench.py [--iters N]

KITTI: 8 x 368 x 1232, row offset 0; SceneFlow: 8 x 544 x 960 maps against 540 ground-truth rows, row offset 4.  The kernel reads
20 bytes per ground-truth pixel (gt + four stage maps).  Calls rotate over enough distinct buffer sets (> 256 MiB together) that
every call streams from HBM rather than from the Infinity Cache; hipEvents bracket a run of back-to-back calls on one stream.
Prints one JSON line per geometry: us per call and the fraction of the measured 6.29 TB/s HBM rate."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_TBS = 6.29          # MI355X, measured float4 copy rate


def bench(lib, B, Hg, W, off, iters, dev):
    from lwsnet_amd import _lib
    Hp = Hg + off
    set_bytes = 20 * B * Hg * W
    n_sets = max(2, -(-(512 << 20) // set_bytes))
    g = torch.Generator(device=dev).manual_seed(0)
    sets = []
    for _ in range(n_sets):
        gt = torch.rand((B, Hg, W), device=dev, generator=g) * 200
        preds = [gt.new_zeros((B, 1, Hp, W)) for _ in range(4)]
        for p in preds:
            p[:, 0, off:] = gt + torch.randn((B, Hg, W), device=dev, generator=g) * 3
        sets.append((gt, preds, (ctypes.c_void_p * 4)(*[p.data_ptr() for p in preds])))
    work = torch.empty((int(lib.lws_stage_metrics_workspace(B, Hg, W)),), dtype=torch.uint8, device=dev)
    counts = torch.empty((4, B, 2), dtype=torch.int64, device=dev)
    sums = torch.empty((4, B), dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(k):
        gt, _, arr = sets[k % n_sets]
        _lib.check(lib.lws_stage_metrics(arr, B, Hp, W, off, ctypes.c_void_p(gt.data_ptr()), Hg, 192.0, 0,
                                         ctypes.c_void_p(work.data_ptr()), ctypes.c_void_p(counts.data_ptr()),
                                         ctypes.c_void_p(sums.data_ptr()), st), "lws_stage_metrics")

    for k in range(2 * n_sets):                         # warm-up: code objects, every buffer touched
        call(k)
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(iters):
            call(k)
        e1.record()
        e1.synchronize()
        runs.append(1e3 * e0.elapsed_time(e1) / iters)
    runs.sort()
    us = runs[len(runs) // 2]
    return {"geometry": f"{B}x{Hg}x{W}", "row_offset": off, "bytes": set_bytes, "buffer_sets": n_sets, "us_per_call": round(us, 2),
            "us_runs": [round(r, 2) for r in runs], "tb_per_s": round(set_bytes / us / 1e6, 3),
            "fraction_of_hbm": round(set_bytes / us / 1e6 / HBM_TBS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mbench.py needs a HIP device")
    from lwsnet_amd import _lib, build
    build.build_library()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    for B, Hg, W, off in ((8, 368, 1232, 0), (8, 540, 960, 4)):
        print(json.dumps(bench(lib, B, Hg, W, off, a.iters, dev)), flush=True)


if __name__ == "__main__":
    main()
