#!/usr/bin/env python3
"""Per-kernel timing of the refinement (lws_refine) on the GPU, with per-launch k_ref_dws durations by dilation, refinement chunked (ref_chunk_mb = 72) and in one chunk (development aid).

    python tools/rbench.py [--batch B] [--size HxW] [--iters N]"""
import argparse
import time

import benchkit
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--size", default="256x512")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--opt", action="append", default=[], help="name=value launch-plan option (lws_set_option)")
    a = ap.parse_args()
    H, W = [int(v) for v in a.size.split("x")]
    from lwsnet_amd import ops
    dev = benchkit.DEV
    m = benchkit.seeded_model(opts=a.opt)
    left = torch.randn((a.batch, 3, H, W), device=dev)
    p3 = torch.rand((a.batch, 1, H, W), device=dev) * 100
    outs = {}
    for fuse in (72, 0):
        m.set_option("ref_chunk_mb", fuse)
        for _ in range(5):
            outs[fuse] = ops.refine(m._h, left, p3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            ops.refine(m._h, left, p3)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / a.iters
        with benchkit.profiler(m):
            for _ in range(a.iters):
                ops.refine(m._h, left, p3)
            torch.cuda.synchronize()
            classes, each = benchkit.profile_read(m), benchkit.profile_each(m, "ref_dws")
        per_launch = None
        per = len(each) // a.iters
        if per:
            # launch order inside lws_refine: refinement1_left d = 2,4,8,16; refinement1_disp 2 (+ first conv),4,8,16; refinement2 8,4,2,1
            nch = max(1, per // 12)          # chunks: refinement1_left of every chunk first, then the rest of every chunk
            dil = [2, 4, 8, 16] * nch + [2, 4, 8, 16, 8, 4, 2, 1] * nch
            avg = [sum(each[k * per + j] for k in range(a.iters)) / a.iters * 1e3 for j in range(per)]
            per_launch = "   ref_dws per launch (dilation: us): " + "  ".join(f"d{d}:{u:.1f}" for d, u in zip(dil, avg))
        print(f"ref_chunk_mb={fuse} B={a.batch} {H}x{W}: wall {wall * 1e6:.1f} us per lws_refine; kernels (with event overhead):")
        for name, (tot, cnt) in classes.items():
            print(f"   {name:12s} x{cnt // a.iters:2d} avg {tot / cnt * 1e3:7.2f} us")
        if per_launch:
            print(per_launch)
    print("bitwise equal:", bool(torch.equal(outs[72], outs[0])))


if __name__ == "__main__":
    main()
