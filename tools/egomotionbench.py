#!/usr/bin/env python3
"""lws_egomotion beside one forward of the same shape, timed with device events (development aid, not the judged bench).

    python tools/egomotionbench.py [--iters N] [--runs R] [--levels L] [--gn_iters I]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/egomotionbench.py --iters 20 --runs 1      # the k_ego_* kernels one by one

Per shape (368 x 1232, 256 x 512) and batch (1, 8): the reference frame is a synthetic left image with stage 4 of the seeded model
(seed 7) behind forward_occ and the occlusion check's codes as its mask; the current frame is the same image moved one pixel to the
right, so that the Gauss-Newton steps are taken and not refused.  The call (4 levels x 8 steps unless told otherwise, trace and resid
off) is timed on buffers allocated once: eagerly, and replayed from a captured graph.  A warm-up, and R windows of N calls between two
events; the median window, per call.  The forward (LWSNet.forward, same batch, same session) is timed the same way with fewer calls.
Prints one JSON line per shape and batch with the times, the launches of one call, the call's share of the forward, the status and
info of image 0 and the shader clock the device held during the forward (lws_clock_read)."""
import argparse
import json

import benchkit
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--gn_iters", type=int, default=8)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    from lwsnet_amd import _lib
    from lwsnet_amd.geometry import Camera, camera_rows
    from lwsnet_amd.synth import make_pair, to_rgb8
    dev = benchkit.DEV
    model = benchkit.seeded_model()
    P, stream = benchkit.ptr, benchkit.stream
    fx, fy, _, _, baseline = benchkit.KITTI
    for (H, W), B in ((s, b) for s in ((368, 1232), (256, 512)) for b in (1, 8)):
        left, right = (np.repeat(x[None], B, axis=0) for x in make_pair(H, W, 0)[:2])
        res = model.forward_occ(left, right, tau=1.0, fill=False)
        disp, mask = res.disp[3].as_subclass(torch.Tensor).contiguous(), res.mask[3].contiguous()
        ghz = benchkit.clock_ghz(model, lambda: model(left, right))
        rgb8 = np.ascontiguousarray(np.stack([to_rgb8(x) for x in left]))
        rgb_ref = torch.from_numpy(rgb8).to(dev)
        rgb_cur = torch.from_numpy(np.ascontiguousarray(np.roll(rgb8, 1, axis=2))).to(dev)
        cam = torch.from_numpy(camera_rows([Camera(fx, fy, (W - 1) / 2.0, (H - 1) / 2.0, baseline)] * B, B)).to(dev)
        work = torch.empty((_lib.nbytes("lws_egomotion_workspace", B, H, W, a.levels),), device=dev, dtype=torch.uint8)
        pose = torch.empty((B, 2, 12), device=dev, dtype=torch.float32)
        status = torch.empty((B,), device=dev, dtype=torch.int32)
        info = torch.empty((B, 4), device=dev, dtype=torch.float64)

        def call(k=None):
            _lib.call("lws_egomotion", P(rgb_ref), P(disp), P(mask), P(rgb_cur), P(cam), None, B, H, W, a.levels, a.gn_iters, 1.0, 1.0, 10.0, 0.0,
                      256, P(work), P(pose), P(status), P(info), None, None, stream())

        line = {"tool": "egomotionbench", "geometry": f"{B}x{H}x{W}", "levels": a.levels, "gn_iters": a.gn_iters, "iters": a.iters, "runs": a.runs,
                "launches": a.levels + 2 * a.levels * a.gn_iters + 2, "clock_ghz": ghz}
        benchkit.warm(call, 5)
        line["eager"] = benchkit.summary(benchkit.windows(call, a.iters, a.runs))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        graph.replay()
        torch.cuda.synchronize()
        line["graph"] = benchkit.summary(benchkit.windows(lambda k: graph.replay(), a.iters, a.runs))
        line["status"], line["info"] = int(status[0]), [round(v, 4) for v in info[0].cpu().tolist()]
        l_dev, r_dev = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (left, right))     # resident inputs: no upload in the window
        fwd = lambda k: model(l_dev, r_dev)                   # noqa: E731
        benchkit.warm(fwd, 1)
        line["forward"] = benchkit.summary(benchkit.windows(fwd, max(1, a.iters // 5), min(a.runs, 5)))
        line["eager_over_forward"] = round(line["eager"]["us"] / line["forward"]["us"], 4)
        line["graph_over_forward"] = round(line["graph"]["us"] / line["forward"]["us"], 4)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
