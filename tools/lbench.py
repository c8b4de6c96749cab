#!/usr/bin/env python3
"""Device time of the left-right consistency check (development aid, not the judged bench).

    python tools/lbench.py [--iters N]

For each geometry (1 x 368 x 1232, 8 x 368 x 1232, 8 x 256 x 512) one JSON line:
  - lws_lr_check with 4 maps, fill on, `right` and row_kept on: 17 bytes per pixel per map (dL and dRm read, out, right and the
    mask byte written); us per call and the fraction of the measured 6.29 TB/s HBM rate;
  - lws_lr_pairs: 24 bytes per input pixel and channel (left and right read, four planes written), same figures;
  - LWSNet.forward_lr (synthetic weights) against a plain forward at B and at 2B, ms per call.
The kernels' calls rotate over enough distinct buffer sets (> 256 MiB together) that every call streams from HBM rather than from
the Infinity Cache; hipEvents bracket a run of back-to-back calls on one stream, the median of five runs is reported."""
import argparse
import ctypes
import json

import benchkit
import torch


def bench_check(lib, B, H, W, iters, dev):
    from lwsnet_amd import _lib
    set_bytes = 17 * 4 * B * H * W
    n = benchkit.n_sets(set_bytes)
    g = torch.Generator(device=dev).manual_seed(0)
    arr = ctypes.c_void_p * 4
    sets = []
    for _ in range(n):
        dl = [torch.rand((B, 1, H, W), device=dev, generator=g) * 40 for _ in range(4)]
        drm = [d.flip(-1) + torch.rand((B, 1, H, W), device=dev, generator=g) for d in dl]
        out = [torch.empty_like(d) for d in dl]
        right = [torch.empty_like(d) for d in dl]
        mask = [torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev) for _ in range(4)]
        kept = torch.empty((4, B, H), dtype=torch.int32, device=dev)
        ts = dl + drm + out + right + mask + [kept]
        sets.append((ts, [arr(*[t.data_ptr() for t in x]) for x in (dl, drm, out, mask, right)], ctypes.c_void_p(kept.data_ptr())))
    st = benchkit.stream()

    def call(k):
        _, (a_dl, a_drm, a_out, a_mask, a_right), kp = sets[k % n]
        _lib.check(lib.lws_lr_check(a_dl, a_drm, 4, B, H, W, 1.0, 1, a_out, a_mask, a_right, kp, st), "lws_lr_check")

    benchkit.warm(call, 2 * n)
    runs = benchkit.windows(call, iters)
    return {"kernel": "lws_lr_check", "geometry": f"{B}x{H}x{W}", "maps": 4, "fill": 1, "right": True, "bytes": set_bytes,
            "buffer_sets": n, **benchkit.per_call(runs, set_bytes)}


def bench_pairs(lib, B, H, W, iters, dev):
    from lwsnet_amd import _lib
    set_bytes = 4 * 3 * B * H * W * (2 + 4)
    n = benchkit.n_sets(set_bytes)
    g = torch.Generator(device=dev).manual_seed(1)
    P = benchkit.ptr
    sets = []
    for _ in range(n):
        l, r = (torch.randn((B, 3, H, W), device=dev, generator=g) for _ in range(2))
        l2, r2 = (torch.empty((2 * B, 3, H, W), device=dev) for _ in range(2))
        sets.append([l, r, l2, r2])
    st = benchkit.stream()

    def call(k):
        l, r, l2, r2 = sets[k % n]
        _lib.check(lib.lws_lr_pairs(P(l), P(r), P(l2), P(r2), B, H, W, st), "lws_lr_pairs")

    benchkit.warm(call, 2 * n)
    runs = benchkit.windows(call, iters)
    return {"kernel": "lws_lr_pairs", "geometry": f"{B}x{H}x{W}", "bytes": set_bytes, "buffer_sets": n,
            **benchkit.per_call(runs, set_bytes)}


def bench_forward(model, B, H, W, iters):
    left, right = benchkit.device_batch(B, H, W)
    left2, right2 = torch.cat([left, left]), torch.cat([right, right])
    cases = {"forward_B": lambda k: model(left, right), "forward_2B": lambda k: model(left2, right2),
             "forward_lr_B": lambda k: model.forward_lr(left, right, tau=1.0, fill=True)}
    res = {}
    for fn in cases.values():
        benchkit.warm(fn, 3)
    for name, fn in cases.items():
        res.update(benchkit.forward_ms(name, benchkit.windows(fn, iters)))
    res["lr_over_2B"] = round(res["forward_lr_B_ms"] / res["forward_2B_ms"], 4)
    return {"kernel": "forward_lr", "geometry": f"{B}x{H}x{W}", **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--forward_iters", type=int, default=20)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    lib, dev = benchkit.library(build=True), benchkit.DEV
    model = benchkit.seeded_model()
    for B, H, W in ((1, 368, 1232), (8, 368, 1232), (8, 256, 512)):
        line = {"geometry": f"{B}x{H}x{W}", "lr_check": bench_check(lib, B, H, W, a.iters, dev),
                "lr_pairs": bench_pairs(lib, B, H, W, a.iters, dev)}
        torch.cuda.empty_cache()
        line["forward_lr"] = bench_forward(model, B, H, W, a.forward_iters)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
