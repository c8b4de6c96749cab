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

import benchkit
import torch


def bench(lib, B, Hg, W, off, iters, dev):
    from lwsnet_amd import _lib
    Hp = Hg + off
    set_bytes = 20 * B * Hg * W
    n_sets = benchkit.n_sets(set_bytes)
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
    P, st = benchkit.ptr, benchkit.stream()

    def call(k):
        gt, _, arr = sets[k % n_sets]
        _lib.check(lib.lws_stage_metrics(arr, B, Hp, W, off, P(gt), Hg, 192.0, 0, P(work), P(counts), P(sums), st), "lws_stage_metrics")

    benchkit.warm(call, 2 * n_sets)                     # code objects, every buffer touched
    return {"geometry": f"{B}x{Hg}x{W}", "row_offset": off, "bytes": set_bytes, "buffer_sets": n_sets,
            **benchkit.per_call(benchkit.windows(call, iters), set_bytes, ("tb_per_s", "fraction_of_hbm"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    lib, dev = benchkit.library(build=True), benchkit.DEV
    for B, Hg, W, off in ((8, 368, 1232, 0), (8, 540, 960, 4)):
        print(json.dumps(bench(lib, B, Hg, W, off, a.iters, dev)), flush=True)


if __name__ == "__main__":
    main()
