#!/usr/bin/env python3
"""Device time of the one-forward occlusion check (development aid, not the judged bench).

    python tools/occbench.py [--iters N] [--forward_iters N]

One JSON line with, from one run:
  - "occlusion_check": lws_occlusion_check with 4 maps, fill on, `right` and row_kept on at 1 x 368 x 1232, 8 x 256 x 512 and
    8 x 368 x 1232: 13 bytes per pixel per map (dL read; out, right and the mask byte written); us per call and the fraction of the
    measured 6.29 TB/s HBM rate;
  - "lr_check": lws_lr_check on the same shapes (tools/lbench.py's measurement: 17 bytes per pixel per map);
  - "forward": LWSNet.forward_occ, LWSNet.forward_lr and the plain forward (synthetic weights) at 1 x and 8 x 368 x 1232, ms per
    call, and the ratios forward_occ / forward and forward_lr / forward.
The kernels' calls rotate over enough distinct buffer sets (> 256 MiB together) that every call streams from HBM rather than from
the Infinity Cache; hipEvents bracket a run of back-to-back calls on one stream, the median of five runs is reported."""
import argparse
import ctypes
import json

import benchkit
import torch
from lbench import bench_check


def bench_occlusion(lib, B, H, W, iters, dev):
    from lwsnet_amd import _lib
    set_bytes = 13 * 4 * B * H * W
    n = benchkit.n_sets(set_bytes)
    g = torch.Generator(device=dev).manual_seed(0)
    arr = ctypes.c_void_p * 4
    x = torch.arange(W, device=dev, dtype=torch.float32)
    sets = []
    for _ in range(n):
        # a slanted background with plateaus in front of it, plus noise: every code, holes in `right`
        dl = [torch.rand((B, 1, H, 1), device=dev, generator=g) * 30 + 0.01 * x + torch.rand((B, 1, H, W), device=dev, generator=g)
              + 25 * (torch.rand((B, 1, H, W // 16 + 1), device=dev, generator=g) < 0.2).float().repeat_interleave(16, dim=3)[..., :W]
              for _ in range(4)]
        out = [torch.empty_like(d) for d in dl]
        right = [torch.empty_like(d) for d in dl]
        mask = [torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev) for _ in range(4)]
        kept = torch.empty((4, B, H), dtype=torch.int32, device=dev)
        ts = dl + out + right + mask + [kept]
        sets.append((ts, [arr(*[t.data_ptr() for t in v]) for v in (dl, out, mask, right)], ctypes.c_void_p(kept.data_ptr())))
    st = benchkit.stream()

    def call(k):
        _, (a_dl, a_out, a_mask, a_right), kp = sets[k % n]
        _lib.check(lib.lws_occlusion_check(a_dl, 4, B, H, W, 1.0, 1, a_out, a_mask, a_right, kp, st), "lws_occlusion_check")

    benchkit.warm(call, 2 * n)
    runs = benchkit.windows(call, iters)
    density = float(sum(int(t.sum()) for t in (s[0][-1] for s in sets))) / (len(sets) * 4 * B * H * W)
    return {"kernel": "lws_occlusion_check", "geometry": f"{B}x{H}x{W}", "maps": 4, "fill": 1, "right": True, "bytes": set_bytes,
            "buffer_sets": n, "density": round(density, 4), **benchkit.per_call(runs, set_bytes)}


def bench_forward(model, B, H, W, iters):
    left, right = benchkit.device_batch(B, H, W)
    cases = {"forward": lambda k: model(left, right), "forward_occ": lambda k: model.forward_occ(left, right, tau=1.0, fill=True),
             "forward_lr": lambda k: model.forward_lr(left, right, tau=1.0, fill=True)}
    res = {}
    for fn in cases.values():
        benchkit.warm(fn, 3)
    for name, fn in cases.items():
        res.update(benchkit.forward_ms(name, benchkit.windows(fn, iters)))
    res["occ_over_forward"] = round(res["forward_occ_ms"] / res["forward_ms"], 4)
    res["lr_over_forward"] = round(res["forward_lr_ms"] / res["forward_ms"], 4)
    return {"geometry": f"{B}x{H}x{W}", **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--forward_iters", type=int, default=20)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    lib, dev = benchkit.library(build=True), benchkit.DEV
    line = {"occlusion_check": [], "lr_check": [], "forward": []}
    for B, H, W in ((1, 368, 1232), (8, 256, 512), (8, 368, 1232)):
        line["occlusion_check"].append(bench_occlusion(lib, B, H, W, a.iters, dev))
        torch.cuda.empty_cache()
        line["lr_check"].append(bench_check(lib, B, H, W, a.iters, dev))
        torch.cuda.empty_cache()
    model = benchkit.seeded_model()
    for B in (1, 8):
        line["forward"].append(bench_forward(model, B, 368, 1232, a.forward_iters))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
