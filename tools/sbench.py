#!/usr/bin/env python3
"""Conv3D stack of one stage alone (lws_conv3d_stack): per-kernel-class averages, k_conv3d_mid8q (4x4x1_16B, exact) vs k_conv3d_mid8x (option split_bf16 = 2, not bit-exact) (dev aid)."""
import argparse
import benchkit
import torch
from lwsnet_amd import ops
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--size", default="256x512")
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--opt", action="append", default=[])
a = ap.parse_args()
H, W = [int(v) for v in a.size.split("x")]
dev = benchkit.DEV
m = benchkit.seeded_model(opts=a.opt)
opts = ' '.join(a.opt)
for stage, (D, div) in ((1, (9, 4)), (2, (9, 2))):
    c = torch.rand((a.batch, D, H // div, W // div), device=dev) * 12
    for form in (0, 2):                      # option "split_bf16": 0 = k_conv3d_mid8q (exact), 2 = k_conv3d_mid8x (not bit-exact)
        m.set_option("split_bf16", form)
        for _ in range(5):
            ops.conv3d_stack(m._h, stage, c)
        torch.cuda.synchronize()
        tot, cnt = benchkit.profiled(m, lambda: ops.conv3d_stack(m._h, stage, c), a.iters)["conv3d_mid8"]
        avg = tot / cnt * 1e3
        gf = 2 * 27 * 8 * 8 * a.batch * D * (H // div) * (W // div)
        print(f"stage {stage + 1} B={a.batch} {opts} split_bf16={form}: k_conv3d_mid8{'x' if form else 'q'} avg {avg:7.2f} us = {gf / avg / 1e6:6.1f} TF useful")
