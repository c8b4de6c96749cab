#!/usr/bin/env python3
"""lws_objects beside lws_stixels, timed with device events (development aid, not the judged bench).

    python tools/objectbench.py [--iters N] [--runs R]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/objectbench.py --iters 50 --runs 1      # the k_ob_* kernels one by one

The map is stage 4 of the seeded model (seed 7) behind forward_occ at 1 x 368 x 1232; ops.ground gives its codes and heights and
ops.stixels(udisp=True) its histogram, all with their defaults (width 8, sub 4, 768 bins).  Then each of the two C calls alone, on
buffers allocated once: a warm-up, and R windows of N calls between two events; the median window, per call.  lws_stixels is the
yardstick: its kernel is what it was before lws_objects existed.  Prints one JSON line with the times, what the objects call found
and the shader clock the device held during the forward (lws_clock_read)."""
import argparse
import json

import benchkit
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    from lwsnet_amd import _lib, ops
    from lwsnet_amd.geometry import Camera, camera_rows
    from lwsnet_amd.synth import make_pair
    dev = benchkit.DEV
    B, H, W = 1, 368, 1232
    model = benchkit.seeded_model()
    left, right = (x[None] for x in make_pair(H, W, 0)[:2])
    cams = [Camera(*benchkit.KITTI)]
    res = model.forward_occ(left, right, tau=1.0, fill=False)
    ghz = benchkit.clock_ghz(model, lambda: model.forward_occ(left, right, tau=1.0, fill=False))
    disp = res.disp[3].as_subclass(torch.Tensor).contiguous()
    g = ops.ground(disp, cams, res.mask[3])
    st = ops.stixels(disp, cams, g.codes, g.height, udisp=True)
    ob = ops.objects(disp, cams, g.codes, st.udisp)
    width, sub, nbins = 8, 4, st.udisp.shape[2]
    S = st.udisp.shape[1]
    cam = torch.from_numpy(camera_rows(cams, B)).to(dev)
    work = torch.empty((_lib.nbytes("lws_objects_workspace", B, W, width, nbins),), device=dev, dtype=torch.uint8)
    P, stream = benchkit.ptr, benchkit.stream()
    inf = float("inf")

    def stixels(k=None):
        _lib.call("lws_stixels", P(disp), P(cam), P(g.codes), P(g.height), B, H, W, 1.0, inf, 1 << 2, width, sub, nbins, 1, 2 * width, width // 2, 2,
                  2, P(st.rows), P(st.vals), P(st.udisp), stream)

    def objects(k=None, labels=ob.labels):
        _lib.call("lws_objects", P(disp), P(cam), P(g.codes), P(st.udisp), B, H, W, 1.0, inf, 1 << 2, width, sub, nbins, width, 64, 256, P(work),
                  P(ob.rows), P(ob.vals), P(labels), P(ob.info), stream)

    line = {"tool": "objectbench", "geometry": f"{B}x{H}x{W}", "width": width, "sub": sub, "nbins": nbins, "strips": S, "iters": a.iters,
            "runs": a.runs, "clock_ghz": ghz, "info": ob.info[0].cpu().tolist(), "taking_pixels": int(st.udisp.sum())}
    for name, call in (("stixels", stixels), ("objects", objects), ("objects_without_labels", lambda k: objects(labels=None)), ("stixels_again", stixels)):
        benchkit.warm(call, 10)
        line[name] = benchkit.summary(benchkit.windows(call, a.iters, a.runs))
    line["objects_over_stixels"] = round(line["objects"]["us"] / line["stixels"]["us"], 2)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
