#!/usr/bin/env python3
"""lws_temporal_step beside one forward of the same shape, timed with device events (development aid, not the judged bench).

    python tools/temporalbench.py [--iters N] [--runs R]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/temporalbench.py --iters 50 --runs 1      # the k_tp_* kernels one by one

The maps are stage 4 of the seeded model (seed 7) behind forward_occ for two synthetic pairs at 368 x 1232, taken as two frames of a
camera that drove 0.3 m ahead; at batch 8 the pair is repeated.  The first frame makes the state (a first-frame call), then the second
frame's call is timed on buffers allocated once, with the occlusion check's codes as its mask and counts asked for: hold off (the
clearing launch and the fuse launch), hold off without counts (the one launch) and hold on (three launches).  A warm-up, and R
windows of N calls between two events; the median window, per call.  The forward (LWSNet.forward, same batch, same session) is timed
the same way with fewer calls.  Prints one JSON line per batch with the times, the pixels per code and the shader clock the device
held during the forward (lws_clock_read)."""
import argparse
import json

import benchkit
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    from lwsnet_amd import _lib, ops
    from lwsnet_amd.geometry import Camera, camera_rows, relative_pose
    from lwsnet_amd.synth import make_pair
    dev = benchkit.DEV
    H, W = 368, 1232
    model = benchkit.seeded_model()
    cam1 = Camera(*benchkit.KITTI)
    T0 = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float64)
    T1 = T0.copy()
    T1[2, 3] = 0.3
    P, stream = benchkit.ptr, benchkit.stream()
    for B in (1, 8):
        frames = []
        for k in range(2):
            left, right = (np.repeat(x[None], B, axis=0) for x in make_pair(H, W, k)[:2])
            res = model.forward_occ(left, right, tau=1.0, fill=False)
            frames.append((res.disp[3].as_subclass(torch.Tensor).contiguous(), res.mask[3].contiguous(), left, right))
        ghz = benchkit.clock_ghz(model, lambda: model(frames[1][2], frames[1][3]))
        cams = [cam1] * B
        pose = relative_pose(T0, T1)
        s0 = ops.temporal_step(frames[0][0], cams, mask=frames[0][1])
        s1 = ops.temporal_step(frames[1][0], cams, pose=pose, prev=s0[:3], mask=frames[1][1], hold=True)
        cam = torch.from_numpy(camera_rows(cams, B)).to(dev)
        pose_dev = torch.from_numpy(ops.temporal_pose_rows(pose, B)).to(dev)
        work = torch.empty((_lib.nbytes("lws_temporal_workspace", B, H, W, 1),), device=dev, dtype=torch.uint8)
        disp, mask = frames[1][:2]

        def step(hold, counts=s1.counts):
            _lib.call("lws_temporal_step", P(disp), None, P(mask), P(cam), P(pose_dev), P(s0.disp), P(s0.var), P(s0.age), B, H, W, 0.5, 1.0, 0.05, 3.0,
                      0.0, 1.0, hold, 0.05, 4.0, P(work), P(s1.disp), P(s1.var), P(s1.age), P(s1.code), P(counts), stream)

        line = {"tool": "temporalbench", "geometry": f"{B}x{H}x{W}", "iters": a.iters, "runs": a.runs, "clock_ghz": ghz,
                "codes_with_hold": s1.counts[0].cpu().tolist()}
        for name, call in (("hold_off", lambda k: step(0)), ("hold_off_without_counts", lambda k: step(0, None)), ("hold_on", lambda k: step(1)),
                           ("hold_off_again", lambda k: step(0))):
            benchkit.warm(call, 10)
            line[name] = benchkit.summary(benchkit.windows(call, a.iters, a.runs))
        l_dev, r_dev = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in frames[1][2:])     # resident inputs: no upload in the window
        fwd = lambda k: model(l_dev, r_dev)                   # noqa: E731
        benchkit.warm(fwd, 1)
        line["forward"] = benchkit.summary(benchkit.windows(fwd, max(1, a.iters // 20), min(a.runs, 5)))
        line["hold_on_over_forward"] = round(line["hold_on"]["us"] / line["forward"]["us"], 5)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
