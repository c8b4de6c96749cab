#!/usr/bin/env python3
"""Device time of the sparsification histograms beside the stage metrics (development aid, not the judged bench).

    python tools/sparsbench.py [--geometry B H W] [--iters N]

One JSON line for one geometry (default 8 x 368 x 1232), from one process:
  - "stage_metrics": lws_stage_metrics on a batch (4 stage maps + the ground truth read: 5 maps);
  - "sparsification": lws_sparsification with 4 maps (2 * 4 + 1 = 9 maps read) on the same batch, for each input:
      "random_sigma"  unc log-uniform over 2^-30..2^10, kind 0: every bin of the ranking is in use;
      "random_conf"   unc uniform over [-0.1, 1.1], kind 1;
      "bin0"          unc = 0, kind 0: every pixel of the ranking in bin 0, the contention case;
    with us per call, the fraction of the measured 6.29 TB/s HBM rate, and "over_stage_metrics", the ratio of the two times.
    9 / 5 = 1.8 is what the traffic alone would give.
The stage maps and the ground truth are what make() of tests/test_gpu_evaluate.py builds (gt in [-15, 215), errors of a few
pixels).  The calls rotate over enough distinct buffer sets (> 512 MiB together) that every call streams from HBM rather than from
the Infinity Cache; hipEvents bracket a run of back-to-back calls on one stream, the median of five runs is reported."""
import argparse
import ctypes
import json

import benchkit
import torch

INPUTS = (("random_sigma", 0), ("random_conf", 1), ("bin0", 0))


def make_set(B, H, W, dev, g):
    """One batch on the device: gt, four stage maps and, per input, four uncertainty maps."""
    gt = torch.rand((B, H, W), device=dev, generator=g) * 230 - 15
    preds = [(gt + torch.randn((B, H, W), device=dev, generator=g) * (4 * (s + 1))).reshape(B, 1, H, W) for s in range(4)]
    unc = {"random_sigma": [torch.exp2(torch.rand((B, 1, H, W), device=dev, generator=g) * 40 - 30) for _ in range(4)],
           "random_conf": [torch.rand((B, 1, H, W), device=dev, generator=g) * 1.2 - 0.1 for _ in range(4)],
           "bin0": [torch.zeros((B, 1, H, W), device=dev) for _ in range(4)]}
    return gt, preds, unc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", type=int, nargs=3, default=(8, 368, 1232), metavar=("B", "H", "W"))
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    from lwsnet_amd import _lib
    lib, dev = benchkit.library(build=True), benchkit.DEV
    B, H, W = a.geometry
    map_bytes = 4 * B * H * W
    n = benchkit.n_sets(5 * map_bytes)                               # the smaller call's reads alone exceed the Infinity Cache
    g = torch.Generator(device=dev).manual_seed(0)
    sets = [make_set(B, H, W, dev, g) for _ in range(n)]
    arr = ctypes.c_void_p * 4
    P, st = benchkit.ptr, benchkit.stream()
    work = torch.empty((int(lib.lws_stage_metrics_workspace(B, H, W)),), device=dev, dtype=torch.uint8)
    counts = torch.empty((4, B, 2), device=dev, dtype=torch.int64)
    sums = torch.empty((4, B), device=dev, dtype=torch.float64)
    hist = torch.empty((4, B, 2, _lib.LWS_SPARS_BINS, 3), device=dev, dtype=torch.int64)
    pred_arrs = [arr(*[t.data_ptr() for t in s[1]]) for s in sets]
    unc_arrs = {name: [arr(*[t.data_ptr() for t in s[2][name]]) for s in sets] for name, _ in INPUTS}

    def metrics_call(k):
        _lib.check(lib.lws_stage_metrics(pred_arrs[k % n], B, H, W, 0, P(sets[k % n][0]), H, 192.0, 0, P(work), P(counts), P(sums), st),
                   "lws_stage_metrics")

    def spars_call(name, kind):
        def call(k):
            _lib.check(lib.lws_sparsification(pred_arrs[k % n], unc_arrs[name][k % n], 4, kind, B, H, W, 0, P(sets[k % n][0]), H, 192.0, 0,
                                              P(hist), st), "lws_sparsification")
        return call

    def run(call, nbytes):
        benchkit.warm(call, 2 * n)
        return {"bytes": nbytes, **benchkit.per_call(benchkit.windows(call, a.iters), nbytes, ("fraction_of_hbm", "hbm_floor_us"))}

    line = {"geometry": f"{B}x{H}x{W}", "buffer_sets": n, "stage_metrics": run(metrics_call, 5 * map_bytes), "sparsification": {}}
    for name, kind in INPUTS:
        r = run(spars_call(name, kind), 9 * map_bytes)
        r["over_stage_metrics"] = round(r["us_per_call"] / line["stage_metrics"]["us_per_call"], 3)
        hs = hist.cpu()
        r["bins_in_use"] = [int((hs[0, 0, k, :, 0] > 0).sum()) for k in range(2)]           # ranking, oracle: image 0 of map 0
        line["sparsification"][name] = r
    line["stage_metrics_again"] = run(metrics_call, 5 * map_bytes)       # the same process, after: the clock has not moved
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
