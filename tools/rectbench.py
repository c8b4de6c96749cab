#!/usr/bin/env python3
"""Device time of the rectifying front end (development aid, not the judged bench).

    python tools/rectbench.py [--iters N] [--runs N] [--forward_iters N]

For 1 and 8 raw pairs of 375 x 1242 rectified into the bottom-right 368 x 1232 window (a KITTI-like calibration: f ~ 960 px, strong
barrel distortion, both cameras, rect + input + valid requested): the median over `--runs` runs of the microseconds per
ops.rectify_pair call, each run `--iters` back-to-back calls on one stream between two hipEvents (the launch and the three output
allocations inside), with the fastest and the slowest run beside it; from the same process the two ops.preprocess_rgb8 calls at
the same output shape that the call replaces, and a plain forward of the same batch (synthetic weights).  `gb_per_s` is the
traffic the call cannot avoid -- every output byte written once (16 B per pixel and camera) plus every raw byte read once --
over the median time.  Everything is warmed up first.  Prints one JSON line."""
import argparse
import json

import benchkit
import numpy as np
import torch

benchkit.use_tests()

RAW_HW, OUT_HW = (375, 1242), (368, 1232)
BATCHES = (1, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--forward_iters", type=int, default=10)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    import rectify_reference as R
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import rectify_params
    dev = benchkit.DEV
    model = benchkit.seeded_model(build=True)
    calib = R.kitti_like_calib(RAW_HW)[0]
    origin = (RAW_HW[0] - OUT_HW[0], RAW_HW[1] - OUT_HW[1])
    result = {"tool": "rectbench", "iters": a.iters, "runs": a.runs, "raw": "%dx%d" % RAW_HW, "window": "%dx%d" % OUT_HW, "batches": []}
    for B in BATCHES:
        rng = np.random.default_rng(B)
        raw = [torch.from_numpy(rng.integers(0, 256, (B,) + RAW_HW + (3,), dtype=np.uint8)).to(dev) for _ in range(2)]
        params = torch.from_numpy(rectify_params(calib, B)).to(dev)

        def rectify(k=None):
            return ops.rectify_pair(raw[0], raw[1], params, OUT_HW, origin=origin)

        for _ in range(5):
            out = rectify()
        rect = out["rect"]

        def preprocess(k=None):
            return ops.preprocess_rgb8(rect[0]), ops.preprocess_rgb8(rect[1])

        for _ in range(5):
            preprocess()
        left, right = benchkit.device_batch(B, *OUT_HW)
        benchkit.warm(lambda k: model(left, right), 3)
        t_rect, t_pre = (benchkit.summary(benchkit.windows(call, a.iters, a.runs), "_us") for call in (rectify, preprocess))
        fwd = benchkit.summary(benchkit.windows(lambda k: model(left, right), a.forward_iters, a.runs), "_us")
        nbytes = 2 * B * (16 * OUT_HW[0] * OUT_HW[1] + 3 * RAW_HW[0] * RAW_HW[1])
        t_rect.update(bytes=nbytes, gb_per_s=round(nbytes / t_rect["us"] / 1e3, 1), over_forward=round(t_rect["us"] / fwd["us"], 4),
                      valid_fraction=[round(float(v.float().mean()), 4) for v in out["valid"]])
        result["batches"].append({"batch": B, "rectify_pair": t_rect, "two_preprocess_rgb8": t_pre, "forward": fwd})
        del raw, left, right, out, rect
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
