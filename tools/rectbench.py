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
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

RAW_HW, OUT_HW = (375, 1242), (368, 1232)
BATCHES = (1, 8)


def timed(call, iters, runs):
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        e1.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / iters)
    out.sort()
    return {"us": round(out[len(out) // 2], 2), "min_us": round(out[0], 2), "max_us": round(out[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--forward_iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rectbench.py needs a HIP device")
    import rectify_reference as R
    from lwsnet_amd import build, ops
    from lwsnet_amd.geometry import rectify_params
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.synth import make_batch
    from lwsnet_amd.weights import default_args, make_state_dict
    build.build_library()
    dev = torch.device("cuda:0")
    model = LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()
    calib = R.kitti_like_calib(RAW_HW)[0]
    origin = (RAW_HW[0] - OUT_HW[0], RAW_HW[1] - OUT_HW[1])
    result = {"tool": "rectbench", "iters": a.iters, "runs": a.runs, "raw": "%dx%d" % RAW_HW, "window": "%dx%d" % OUT_HW, "batches": []}
    for B in BATCHES:
        rng = np.random.default_rng(B)
        raw = [torch.from_numpy(rng.integers(0, 256, (B,) + RAW_HW + (3,), dtype=np.uint8)).to(dev) for _ in range(2)]
        params = torch.from_numpy(rectify_params(calib, B)).to(dev)

        def rectify():
            return ops.rectify_pair(raw[0], raw[1], params, OUT_HW, origin=origin)

        for _ in range(5):
            out = rectify()
        rect = out["rect"]

        def preprocess():
            return ops.preprocess_rgb8(rect[0]), ops.preprocess_rgb8(rect[1])

        for _ in range(5):
            preprocess()
        left, right = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in make_batch(B, *OUT_HW)[:2])
        for _ in range(3):
            model(left, right)
        torch.cuda.synchronize()
        t_rect, t_pre = timed(rectify, a.iters, a.runs), timed(preprocess, a.iters, a.runs)
        fwd = timed(lambda: model(left, right), a.forward_iters, a.runs)
        nbytes = 2 * B * (16 * OUT_HW[0] * OUT_HW[1] + 3 * RAW_HW[0] * RAW_HW[1])
        t_rect.update(bytes=nbytes, gb_per_s=round(nbytes / t_rect["us"] / 1e3, 1), over_forward=round(t_rect["us"] / fwd["us"], 4),
                      valid_fraction=[round(float(v.float().mean()), 4) for v in out["valid"]])
        result["batches"].append({"batch": B, "rectify_pair": t_rect, "two_preprocess_rgb8": t_pre, "forward": fwd})
        del raw, left, right, out, rect
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
