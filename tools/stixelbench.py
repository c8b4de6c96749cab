#!/usr/bin/env python3
"""The stixel kernel beside the ground kernels, for a kernel trace (development aid, not the judged bench).

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/stixelbench.py [--iters N]

Runs lwsnet_amd.ops.ground and lwsnet_amd.ops.stixels (width 8, 2 layers, bins of a quarter pixel, 768 bins: the defaults) N times
on the 1 x 368 x 1232 road with boxes of tools/groundbench.py, after a warm-up, so that the trace's statistics hold k_stixels next
to k_classify and k_bev_scatter of the same run (the strip passes read from L2, as they do behind ops.ground in the CLI).  Prints
one JSON line with what was found, so that the trace is known to be of a scene with stixels in it."""
import argparse
import json

import benchkit
import torch
from gbench import BASELINE, FX
from groundbench import inputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import Camera
    dev = benchkit.DEV
    B, H, W = 1, 368, 1232
    disp, mask = inputs(B, H, W, dev, torch.Generator(device=dev).manual_seed(4))
    cam = Camera(FX, FX, 600.0, 170.0, BASELINE)
    for _ in range(3):
        g = ops.ground(disp, cam, mask)
        st = ops.stixels(disp, cam, g.codes, g.height)
    torch.cuda.synchronize()
    for _ in range(a.iters):
        g = ops.ground(disp, cam, mask)
        st = ops.stixels(disp, cam, g.codes, g.height)
    torch.cuda.synchronize()
    rows = st.rows[0].cpu().numpy()
    print(json.dumps({"geometry": f"{B}x{H}x{W}", "width": 8, "layers": 2, "sub": 4, "nbins": 768, "iters": a.iters,
                      "status": g.info[:, 0].cpu().tolist(), "stixels_per_layer": (rows[..., 0] > 0).sum(axis=0).tolist(),
                      "holes": int(((rows[..., 0] == 0) & (rows[..., 3] >= 0)).sum())}), flush=True)


if __name__ == "__main__":
    main()
