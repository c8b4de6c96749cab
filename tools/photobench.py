#!/usr/bin/env python3
"""Device time of the photometric reprojection error (development aid, not the judged bench).

    python tools/photobench.py [--iters N] [--forward_iters N]

One JSON line with, from one run:
  - "photometric": lws_photometric with 4 maps, err and scored on, no mask, at 1 x 368 x 1232 and 8 x 368 x 1232: 15 bytes per
    pixel and map (the map and the two images read, err and the scored byte written); us per call and the fraction of the
    measured 6.29 TB/s HBM rate; "with_warped" adds the warped image (18 bytes);
  - "forward": the plain forward (synthetic weights) of the same batch, ms per call, and photometric / forward.
The calls rotate over enough distinct buffer sets (> 256 MiB together) that every call streams from HBM rather than from the
Infinity Cache; hipEvents bracket a run of back-to-back calls on one stream, the median of five runs is reported."""
import argparse
import ctypes
import json

import benchkit
import torch


def bench_photometric(lib, B, H, W, iters, dev, with_warped):
    from lwsnet_amd import _lib
    set_bytes = (18 if with_warped else 15) * 4 * B * H * W
    n = benchkit.n_sets(set_bytes)
    g = torch.Generator(device=dev).manual_seed(0)
    arr = ctypes.c_void_p * 4
    x = torch.arange(W, device=dev, dtype=torch.float32)
    sets = []
    for _ in range(n):
        # a slanted background with plateaus in front of it, plus sub-pixel noise: a smooth map with jumps
        disp = [torch.rand((B, 1, H, 1), device=dev, generator=g) * 30 + 0.01 * x + torch.rand((B, 1, H, W), device=dev, generator=g)
                + 25 * (torch.rand((B, 1, H, W // 16 + 1), device=dev, generator=g) < 0.2).float().repeat_interleave(16, dim=3)[..., :W]
                for _ in range(4)]
        left, right = (torch.randint(0, 256, (B, H, W, 3), device=dev, dtype=torch.uint8, generator=g) for _ in range(2))
        err = [torch.empty_like(d) for d in disp]
        scored = [torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev) for _ in range(4)]
        warped = [torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(4)] if with_warped else []
        sums = torch.empty((4, B, 4), dtype=torch.int64, device=dev)
        ts = disp + [left, right] + err + scored + warped + [sums]
        sets.append((ts, [arr(*[t.data_ptr() for t in v]) for v in (disp, err, scored, warped)], left.data_ptr(), right.data_ptr(), sums.data_ptr()))
    st = benchkit.stream()

    def call(k):
        _, (a_disp, a_err, a_scored, a_warped), lp, rp, sp = sets[k % n]
        _lib.check(lib.lws_photometric(a_disp, 4, lp, rp, arr(), None, B, H, W, 0.85, a_err, a_scored, a_warped, sp, st), "lws_photometric")

    benchkit.warm(call, 2 * n)
    runs = benchkit.windows(call, iters)
    density = float(sum(int(s[0][-1][:, :, 0].sum()) for s in sets)) / (len(sets) * 4 * B * H * W)
    return {"kernel": "lws_photometric", "geometry": f"{B}x{H}x{W}", "maps": 4, "with_warped": with_warped, "bytes": set_bytes,
            "buffer_sets": n, "density": round(density, 4), **benchkit.per_call(runs, set_bytes)}


def bench_forward(model, B, H, W, iters):
    left, right = benchkit.device_batch(B, H, W)
    benchkit.warm(lambda k: model(left, right), 3)
    return {"geometry": f"{B}x{H}x{W}", **benchkit.forward_ms("forward", benchkit.windows(lambda k: model(left, right), iters))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--forward_iters", type=int, default=20)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    lib, dev = benchkit.library(build=True), benchkit.DEV
    line = {"photometric": [], "forward": []}
    for B, H, W in ((1, 368, 1232), (8, 368, 1232)):
        for with_warped in (False, True):
            line["photometric"].append(bench_photometric(lib, B, H, W, a.iters, dev, with_warped))
            torch.cuda.empty_cache()
    model = benchkit.seeded_model()
    for i, B in enumerate((1, 8)):
        f = bench_forward(model, B, 368, 1232, a.forward_iters)
        f["photometric_over_forward"] = round(line["photometric"][2 * i]["us_per_call"] / 1e3 / f["forward_ms"], 4)
        line["forward"].append(f)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
