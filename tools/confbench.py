#!/usr/bin/env python3
"""Device time of the confidence outputs (development aid, not the judged bench).

    python tools/confbench.py [--iters N] [--forward_iters N]

One JSON line with, from one run:
  - "softargmin_conf": lws_softargmin_conf (conf and sigma written, no low-resolution outputs) on the cost of each of the three
    volume stages at 1 x 368 x 1232, 8 x 256 x 512 and 8 x 368 x 1232: D h w 4 bytes read and 2 H W 4 bytes written per image;
    us per call, the fraction of the measured 6.29 TB/s HBM rate and the time that rate would take;
  - "forward": LWSNet.forward_conf and the plain forward (synthetic weights) at the same shapes, ms per call, and the ratio
    forward_conf / forward.
The kernel's calls rotate over enough distinct buffer sets (> 256 MiB together) that every call streams from HBM rather than from
the Infinity Cache; hipEvents bracket a run of back-to-back calls on one stream, the median of five runs is reported."""
import argparse
import json

import benchkit
import torch


def bench_stage(lib, stage, B, H, W, maxdisplist, iters, dev):
    from lwsnet_amd import _lib
    m = maxdisplist[stage]
    D, start = (m, 0.0) if stage == 0 else (2 * m - 1, float(-m + 1))
    h, w = ((H + 1) // 2) // (4 >> stage), ((W + 1) // 2) // (4 >> stage)
    set_bytes = 4 * B * (D * h * w + 2 * H * W)
    n = benchkit.n_sets(set_bytes)
    g = torch.Generator(device=dev).manual_seed(stage)
    sets = [(torch.rand((B, D, h, w), device=dev, generator=g) * 12, torch.empty((B, 1, H, W), device=dev),
             torch.empty((B, 1, H, W), device=dev)) for _ in range(n)]
    st = benchkit.stream()
    P = benchkit.ptr

    def call(k):
        cost, conf, sigma = sets[k % n]
        _lib.check(lib.lws_softargmin_conf(P(cost), B, D, h, w, start, H, W, None, None, None, P(conf), P(sigma), st), "lws_softargmin_conf")

    benchkit.warm(call, 2 * n)
    runs = benchkit.windows(call, iters)
    return {"kernel": "lws_softargmin_conf", "stage": stage + 1, "geometry": f"{B}x{H}x{W}", "D": D, "low": f"{h}x{w}", "bytes": set_bytes,
            "buffer_sets": n, **benchkit.per_call(runs, set_bytes)}


def bench_forward(model, B, H, W, iters):
    left, right = benchkit.device_batch(B, H, W)
    cases = {"forward": lambda k: model(left, right), "forward_conf": lambda k: model.forward_conf(left, right)}
    res = {}
    for fn in cases.values():
        benchkit.warm(fn, 3)
    for name, fn in cases.items():
        res.update(benchkit.forward_ms(name, benchkit.windows(fn, iters)))
    res["conf_over_forward"] = round(res["forward_conf_ms"] / res["forward_ms"], 4)
    return {"geometry": f"{B}x{H}x{W}", **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--forward_iters", type=int, default=20)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    lib, dev = benchkit.library(build=True), benchkit.DEV
    model = benchkit.seeded_model()
    line = {"softargmin_conf": [], "forward": []}
    shapes = ((1, 368, 1232), (8, 256, 512), (8, 368, 1232))
    for B, H, W in shapes:
        for stage in range(3):
            line["softargmin_conf"].append(bench_stage(lib, stage, B, H, W, model.maxdisplist, a.iters, dev))
            torch.cuda.empty_cache()
    for B, H, W in shapes:
        line["forward"].append(bench_forward(model, B, H, W, a.forward_iters))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
