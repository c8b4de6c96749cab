#!/usr/bin/env python3
"""Device time of the geometry kernels (development aid, not the judged bench).

    python tools/gbench.py [--iters N]

For each geometry (1 x 368 x 1232, 8 x 368 x 1232) one JSON line:
  - lws_depth_maps with a code map and all three outputs: 13 bytes per pixel (disp and the mask byte read; depth, depth16 and
    disp16 written); us per call, the fraction of the measured 6.29 TB/s HBM rate and the HBM floor;
  - lws_point_cloud with a code map and colour (three launches): disp and the mask read twice, the colour once, 16 bytes written
    per kept point; the same figures.
The inputs are model-like disparities (10 .. 150 pixels) with a code map that keeps ~80 % of the pixels.  The calls rotate over
enough distinct buffer sets (> 256 MiB together) that every call streams from HBM rather than from the Infinity Cache; hipEvents
bracket a run of back-to-back calls on one stream, the median of five runs is reported."""
import argparse
import json

import benchkit
import torch

FX, BASELINE = 721.5377, 0.5327


def inputs(B, H, W, dev, g):
    disp = torch.rand((B, 1, H, W), device=dev, generator=g) * 140 + 10
    mask = (torch.rand((B, 1, H, W), device=dev, generator=g) < 0.8).to(torch.uint8)
    return disp, mask


def result(name, B, H, W, set_bytes, n, runs, **extra):
    return {"kernel": name, "geometry": f"{B}x{H}x{W}", "bytes": set_bytes, "buffer_sets": n,
            **benchkit.per_call(runs, set_bytes, benchkit.TRAFFIC + ("over_floor",)), **extra}


def bench_depth(lib, B, H, W, iters, dev):
    from lwsnet_amd import _lib
    set_bytes = 13 * B * H * W
    n = benchkit.n_sets(set_bytes)
    g = torch.Generator(device=dev).manual_seed(0)
    cam = torch.tensor([[FX, FX, 600.0, 170.0, FX * BASELINE]] * B, dtype=torch.float32, device=dev)
    sets = []
    for _ in range(n):
        disp, mask = inputs(B, H, W, dev, g)
        outs = [torch.empty((B, 1, H, W), dtype=dt, device=dev) for dt in (torch.float32, torch.uint16, torch.uint16)]
        sets.append([disp, mask] + outs)
    st = benchkit.stream()

    def call(k):
        disp, mask, depth, depth16, disp16 = sets[k % n]
        _lib.check(lib.lws_depth_maps(disp.data_ptr(), mask.data_ptr(), cam.data_ptr(), B, H, W, 1.0, float("inf"), depth.data_ptr(),
                                      depth16.data_ptr(), disp16.data_ptr(), st), "lws_depth_maps")

    benchkit.warm(call, 2 * n)
    runs = benchkit.windows(call, iters)
    return result("lws_depth_maps", B, H, W, set_bytes, n, runs, outputs=["depth", "depth16", "disp16"], mask=True)


def bench_cloud(lib, B, H, W, iters, dev):
    from lwsnet_amd import _lib
    g = torch.Generator(device=dev).manual_seed(1)
    cam = torch.tensor([[FX, FX, 600.0, 170.0, FX * BASELINE]] * B, dtype=torch.float32, device=dev)
    work = torch.empty((int(lib.lws_point_cloud_workspace(B, H)),), dtype=torch.uint8, device=dev)
    counts = torch.empty((B,), dtype=torch.int64, device=dev)
    n = benchkit.n_sets(26 * B * H * W)
    sets = []
    for _ in range(n):
        disp, mask = inputs(B, H, W, dev, g)
        rgb = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
        sets.append((disp, mask, rgb, torch.empty((B, H * W, 16), dtype=torch.uint8, device=dev)))
    st = benchkit.stream()

    def call(k):
        disp, mask, rgb, points = sets[k % n]
        _lib.check(lib.lws_point_cloud(disp.data_ptr(), mask.data_ptr(), rgb.data_ptr(), cam.data_ptr(), B, H, W, 1.0, float("inf"),
                                       work.data_ptr(), points.data_ptr(), counts.data_ptr(), st), "lws_point_cloud")

    benchkit.warm(call, 1)
    kept = int(counts.sum())
    set_bytes = 2 * 5 * B * H * W + 3 * B * H * W + 16 * kept          # disp + mask twice, rgb once, the kept records
    benchkit.warm(call, 2 * n)
    runs = benchkit.windows(call, iters)
    return result("lws_point_cloud", B, H, W, set_bytes, n, runs, kept_fraction=round(kept / (B * H * W), 4), mask=True, rgb=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    lib, dev = benchkit.library(), benchkit.DEV
    for B, H, W in ((1, 368, 1232), (8, 368, 1232)):
        line = {"geometry": f"{B}x{H}x{W}", "depth_maps": bench_depth(lib, B, H, W, a.iters, dev),
                "point_cloud": bench_cloud(lib, B, H, W, a.iters, dev)}
        torch.cuda.empty_cache()
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
