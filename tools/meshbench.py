#!/usr/bin/env python3
"""Device time of the surface kernels (development aid, not the judged bench).

    python tools/meshbench.py [--iters N]

For each geometry (1 x 368 x 1232, 8 x 368 x 1232) one JSON line:
  - lws_surface_normals with a code map and both outputs: 20 bytes per pixel (disp and the mask byte read; three float planes and
    the 3-byte normal map written); us per call, the fraction of the measured 6.29 TB/s HBM rate and the HBM floor;
  - lws_surface_mesh with a code map, colour, normals and the index map (three launches): disp and the mask read twice, colour and
    normals once, 4 bytes of index per pixel, 32 bytes per vertex, 12 per face; the same figures;
  - lws_point_cloud from the same run (tools/gbench.py's measurement), to set the mesh beside the cloud it extends.
The inputs are a smooth surface (a tilted plane under a slow wave, so that neighbours are connected at max_jump = 1) with a
code map that keeps ~80 % of the pixels.  Buffer rotation and timing are tools/benchkit.py's: more than 256 MiB of distinct
buffer sets, hipEvents around back-to-back calls on one stream, the median of five runs."""
import argparse
import json

import benchkit
import torch
from gbench import BASELINE, FX, bench_cloud, result

ARGS = (1.0, float("inf"), 1.0)         # min_disp, max_depth, max_jump


def inputs(B, H, W, dev, g):
    ys = torch.arange(H, device=dev, dtype=torch.float32).view(1, 1, H, 1)
    xs = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, 1, W)
    phase = torch.rand((B, 1, 1, 1), device=dev, generator=g) * 6.28
    disp = 40 + 0.05 * xs - 0.08 * ys + 6 * torch.sin(xs / 37 + ys / 53 + phase)
    mask = (torch.rand((B, 1, H, W), device=dev, generator=g) < 0.8).to(torch.uint8)
    return disp.contiguous(), mask


def camera(B, dev):
    return torch.tensor([[FX, FX, 600.0, 170.0, FX * BASELINE]] * B, dtype=torch.float32, device=dev)


def bench_normals(lib, B, H, W, iters, dev):
    from lwsnet_amd import _lib
    set_bytes = 20 * B * H * W
    n = benchkit.n_sets(set_bytes)
    g = torch.Generator(device=dev).manual_seed(2)
    cam = camera(B, dev)
    sets = [inputs(B, H, W, dev, g) + (torch.empty((B, 3, H, W), dtype=torch.float32, device=dev),
                                       torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)) for _ in range(n)]
    st = benchkit.stream()

    def call(k):
        disp, mask, normals, normals8 = sets[k % n]
        _lib.check(lib.lws_surface_normals(disp.data_ptr(), mask.data_ptr(), cam.data_ptr(), B, H, W, *ARGS, normals.data_ptr(),
                                           normals8.data_ptr(), st), "lws_surface_normals")

    benchkit.warm(call, 2 * n)
    runs = benchkit.windows(call, iters)
    return result("lws_surface_normals", B, H, W, set_bytes, n, runs, outputs=["normals", "normals8"], mask=True)


def bench_mesh(lib, B, H, W, iters, dev):
    from lwsnet_amd import _lib
    g = torch.Generator(device=dev).manual_seed(3)
    cam = camera(B, dev)
    work = torch.empty((int(lib.lws_surface_mesh_workspace(B, H)),), dtype=torch.uint8, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int64, device=dev)
    px = B * H * W
    n = benchkit.n_sets(85 * px)
    st = benchkit.stream()
    sets = []
    for _ in range(n):
        disp, mask = inputs(B, H, W, dev, g)
        rgb = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
        normals = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        _lib.check(lib.lws_surface_normals(disp.data_ptr(), mask.data_ptr(), cam.data_ptr(), B, H, W, *ARGS, normals.data_ptr(), None, st),
                   "lws_surface_normals")
        sets.append((disp, mask, rgb, normals, torch.empty((B, H * W, 16), dtype=torch.uint8, device=dev),
                     torch.empty((B, H * W, 4), dtype=torch.float32, device=dev),
                     torch.empty((B, 2 * (H - 1) * (W - 1), 3), dtype=torch.int32, device=dev),
                     torch.empty((B, 1, H, W), dtype=torch.int32, device=dev)))

    def call(k):
        disp, mask, rgb, normals, points, vn, faces, index = sets[k % n]
        _lib.check(lib.lws_surface_mesh(disp.data_ptr(), mask.data_ptr(), rgb.data_ptr(), cam.data_ptr(), normals.data_ptr(), B, H, W, *ARGS,
                                        work.data_ptr(), points.data_ptr(), vn.data_ptr(), faces.data_ptr(), index.data_ptr(),
                                        counts.data_ptr(), st), "lws_surface_mesh")

    benchkit.warm(call, 1)
    nv, nf = (int(v) for v in counts.sum(dim=0).cpu())
    set_bytes = (2 * 5 + 3 + 12 + 4) * px + 32 * nv + 12 * nf    # disp + mask twice, rgb, normals, index; vertex and face records
    benchkit.warm(call, 2 * n)
    runs = benchkit.windows(call, iters)
    return result("lws_surface_mesh", B, H, W, set_bytes, n, runs, kept_fraction=round(nv / px, 4),
                  faces_per_cell=round(nf / (B * (H - 1) * (W - 1)), 4), mask=True, rgb=True, normals=True, index=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    lib, dev = benchkit.library(), benchkit.DEV
    for B, H, W in ((1, 368, 1232), (8, 368, 1232)):
        line = {"geometry": f"{B}x{H}x{W}", "surface_normals": bench_normals(lib, B, H, W, a.iters, dev),
                "surface_mesh": bench_mesh(lib, B, H, W, a.iters, dev), "point_cloud": bench_cloud(lib, B, H, W, a.iters, dev)}
        torch.cuda.empty_cache()
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
