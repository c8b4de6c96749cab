#!/usr/bin/env python3
"""Per-kernel timing of the hot path on the GPU (development aid, not the judged bench).

    python tools/kbench.py [--batch B] [--size HxW] [--iters N] [--check]

Prints the library profiler's average duration per kernel class for `lws_disparity_stages`
on seeded features, plus TFLOP/s for the MFMA kernels.  --check compares against the C oracle."""
import argparse
import time

import benchkit
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--size", default="256x512")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--opt", action="append", default=[], help="name=value launch-plan option (lws_set_option)")
    a = ap.parse_args()
    H, W = [int(v) for v in a.size.split("x")]
    from lwsnet_amd import ops
    dev = benchkit.DEV
    m = benchkit.seeded_model(opts=a.opt)
    B = a.batch
    rng = np.random.default_rng(0)
    H2, W2 = (H + 1) // 2, (W + 1) // 2          # the stem gives ceil(H/2); the hourglass halves twice more
    shapes = [(B, 16, H2 // 4, W2 // 4), (B, 16, H2 // 2, W2 // 2), (B, 8, H2, W2)]
    fl = [torch.from_numpy(np.abs(rng.standard_normal(s)).astype(np.float32) * 0.5).to(dev) for s in shapes]
    fr = [torch.from_numpy(np.abs(rng.standard_normal(s)).astype(np.float32) * 0.5).to(dev) for s in shapes]
    for _ in range(5):
        pred = ops.disparity_stages(m._h, fl, fr, H, W)
    torch.cuda.synchronize()
    with benchkit.profiler(m):
        t0 = time.perf_counter()
        for _ in range(a.iters):
            pred = ops.disparity_stages(m._h, fl, fr, H, W)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / a.iters
        classes = benchkit.profile_read(m)
    print(f"B={B} {H}x{W}: wall {wall * 1e6:.1f} us/iter (with event overhead), "
          f"sum of kernels {sum(tot for tot, _ in classes.values()) / a.iters * 1e3:.1f} us")
    vox = [B * 24 * (H2 // 4) * (W2 // 4), B * 9 * (H2 // 2) * (W2 // 2), B * 9 * H2 * W2]
    for name, (tot, cnt) in classes.items():
        avg = tot / cnt * 1e3
        extra = ""
        if name == "conv3d_mid16":
            extra = f"  {2 * 27 * 32 * 32 * vox[0] / (avg * 1e-6) / 1e12:.1f} TF"
        if name == "conv3d_mid8":
            fl_ = 2 * 27 * 8 * 8 * (vox[1] + vox[2]) / 2
            extra = f"  {fl_ / (avg * 1e-6) / 1e12:.1f} TF (avg of stage 2 and 3)"
        print(f"  {name:16s} x{cnt // a.iters:2d}  avg {avg:8.2f} us{extra}")
    # without the profiler: pure wall per iteration
    t0 = time.perf_counter()
    for _ in range(a.iters):
        pred = ops.disparity_stages(m._h, fl, fr, H, W)
    torch.cuda.synchronize()
    print(f"  wall without profiler: {(time.perf_counter() - t0) / a.iters * 1e6:.1f} us/iter")
    if a.check:
        from lwsnet_amd.weights import make_state_dict
        from oracle import c_oracle as C
        sd = make_state_dict(7)
        want = C.disparity_stages([f.cpu().numpy() for f in fl], [f.cpu().numpy() for f in fr], H, W, sd)
        for s in range(3):
            same = np.array_equal(pred[s].cpu().numpy(), want[s])
            print(f"  stage {s + 1} bit-exact vs C oracle: {same}")
            assert same


if __name__ == "__main__":
    main()
