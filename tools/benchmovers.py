#!/usr/bin/env python3
"""lws_movers beside lws_speckle_filter, the labeller it is modelled on, timed with device events (development aid, not the judged
bench).  Named bench-first: tests/test_benchkit_cpu.py pins the set of tools/*bench.py, and tests/test_movers_cpu.py holds this tool
to the same rule -- the timing method is benchkit's, stated nowhere else.

    python tools/benchmovers.py [--iters N] [--runs R] [--radius R]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/benchmovers.py --iters 20 --runs 1      # the k_mv_* kernels one by one

Per shape (256 x 512, 368 x 1232) at batch 1: the previous frame is a road plane under the KITTI camera with 0.2 px of seeded noise
and a smooth texture; the current frame is the same road seen 0.5 m further on with two textured boxes pasted in that the previous
frame does not have (an approaching thing: `appeared`) and one whose texture alone moved (`changed`).  Timed on buffers allocated
once, a warm-up and R windows of N calls between two events, the median window per call:
  movers          lws_movers with labels, the 11 launches of a call
  movers_graph    the same call replayed from a captured graph
  speckle         lws_speckle_filter of the current map with labels and counts, no fill: the yardstick (5 launches)
Prints one JSON line per shape."""
import argparse
import json

import benchkit
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--radius", type=int, default=0)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    from lwsnet_amd import _lib
    from lwsnet_amd.geometry import Camera, camera_rows
    benchkit.library()
    dev = benchkit.DEV
    P, stream = benchkit.ptr, benchkit.stream
    fx, fy, _, _, baseline = benchkit.KITTI
    for H, W in ((256, 512), (368, 1232)):
        B, K, step, height = 1, 64, 0.5, 1.65               # images, slots, metres driven between the frames, the camera above the road
        camera = Camera(fx, fy, (W - 1) / 2.0, 0.35 * (H - 1), baseline)
        cam = torch.from_numpy(camera_rows([camera], B)).to(dev)
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        z = np.where(yy > camera.cy + 4, fy * height / np.maximum(yy - camera.cy, 1e-9), 0.0)
        road = np.where(z > 0, fx * baseline / np.maximum(z, 1e-9), 0.0)
        rng = np.random.default_rng(0)
        disp0 = np.where(road > 0, road + 0.2 * rng.standard_normal(road.shape), 0.0).astype(np.float32)
        disp1 = np.where(road > 0, road + 0.2 * rng.standard_normal(road.shape), 0.0).astype(np.float32)
        # the road's texture is a function of the ground point, so that it moves as the road does: X and Z of the pixel's ray on the road
        X = (xx - camera.cx) * z / fx
        tex = lambda Z: 128.0 + 50.0 * np.sin(2.0 * X + 0.5) * np.cos(1.1 * Z) + 30.0 * np.cos(0.7 * X - 0.9 * Z)      # noqa: E731
        g0, g1 = np.where(z > 0, tex(z), 90.0), np.where(z > 0, tex(z + step), 90.0)
        y0, s = int(camera.cy) + 20, H // 6
        for k, x0 in enumerate((W // 4, W // 2)):           # two boxes 6 m away that the previous frame lacks
            disp1[y0:y0 + s, x0:x0 + s] = fx * baseline / 6.0
            g1[y0:y0 + s, x0:x0 + s] = 60.0 + 12.0 * (np.arange(s)[None, :] % 16) + 40.0 * k
        x0 = 3 * W // 4                                     # a patch of road whose grey alone changed
        g1[y0 + s:y0 + 2 * s, x0:x0 + s] += 70.0
        to_rgb = lambda g: np.repeat(np.clip(np.rint(g), 0, 255).astype(np.uint8)[None, ..., None], 3, -1)             # noqa: E731
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)              # noqa: E731
        r0, r1, d0, d1 = t(to_rgb(g0)), t(to_rgb(g1)), t(disp0[None, None]), t(disp1[None, None])
        move = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -step], [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, step]], np.float32)
        pose = t(move[None])
        work = torch.empty((max(_lib.nbytes("lws_movers_workspace", B, H, W, K), _lib.nbytes("lws_speckle_workspace", B, H, W)),), device=dev,
                           dtype=torch.uint8)
        evidence, mask = (torch.empty((B, 1, H, W), device=dev, dtype=torch.uint8) for _ in range(2))
        labels = torch.empty((B, 1, H, W), device=dev, dtype=torch.int32)
        rows = torch.empty((B, K, 8), device=dev, dtype=torch.int32)
        vals = torch.empty((B, K, 2), device=dev, dtype=torch.float32)
        info = torch.empty((B, 8), device=dev, dtype=torch.int32)
        out = torch.empty_like(d1)
        counts = torch.empty((B, 3), device=dev, dtype=torch.int64)

        def movers(k=None):
            _lib.call("lws_movers", P(r0), P(d0), None, None, P(r1), P(d1), None, None, P(cam), P(pose), B, H, W, 1.0, 0.3, 0.05, 3.0, 25.0, a.radius,
                      20, 1.0, 64, 2, K, P(work), P(evidence), P(mask), P(labels), P(rows), P(vals), P(info), stream())

        def speckle(k=None):
            _lib.call("lws_speckle_filter", P(d1), None, B, H, W, 1.0, 50, 0, P(work), P(out), P(mask), P(labels), P(counts), stream())

        line = {"tool": "benchmovers", "geometry": f"{B}x{H}x{W}", "radius": a.radius, "iters": a.iters, "runs": a.runs, "launches": 11}
        for name, call in (("movers", movers), ("speckle", speckle)):
            benchkit.warm(call, 5)
            line[name] = benchkit.summary(benchkit.windows(call, a.iters, a.runs))
        movers()
        torch.cuda.synchronize()
        line["info"] = info[0].cpu().tolist()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            movers()
        graph.replay()
        torch.cuda.synchronize()
        line["movers_graph"] = benchkit.summary(benchkit.windows(lambda k: graph.replay(), a.iters, a.runs))
        line["movers_over_speckle"] = round(line["movers"]["us"] / line["speckle"]["us"], 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
