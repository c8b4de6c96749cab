#!/usr/bin/env python3
"""Device time of the speckle filter (development aid, not the judged bench).

    python tools/spbench.py [--iters N] [--forward_iters N] [--inputs KIND ...] [--no_mask]

For each geometry (1 x 368 x 1232, 8 x 256 x 512, 8 x 368 x 1232), mask on, labels and counts on, one JSON line per input
(plateaus with islands, constant, checkerboard, serpentine) and fill (0, 1):
  - us per lws_speckle_filter call and its launches (5 with counts: tile labelling, tile edges, flatten, apply, counts);
  - the byte floor: the compulsory bytes (4 read + 4 written per pixel for the maps, 1 + 1 for the codes, + 4 for the labels) at
    the measured 6.29 TB/s copy rate, the call's time over it, and the bytes the implementation moves (disp and mask are read
    by the tile and the apply kernels: + 5; the parent and size words are written by the tile kernel, read by the flatten and
    apply kernels: + 24 per pixel, more where find walks are long);
  - the forward of the same batch (synthetic weights) and the call's time over it.
The calls rotate over enough distinct buffer sets (> 256 MiB together) that every call streams from HBM rather than from the
Infinity Cache; hipEvents bracket a run of back-to-back calls on one stream, all launches of a call inside; the median of five runs
is reported."""
import argparse
import json

import benchkit
import torch

benchkit.use_tests()
FLOOR_BYTES = 4 + 4 + 1 + 1 + 4
MOVED_BYTES = FLOOR_BYTES + 4 + 1 + 24


def bench_filter(lib, kind, B, H, W, fill, iters, dev, masked=True):
    import speckle_inputs as I
    from lwsnet_amd import _lib
    px = B * H * W
    ws = int(lib.lws_speckle_workspace(B, H, W))
    set_bytes = px * (4 + 1 + 4 + 1 + 4) + ws
    n = benchkit.n_sets(set_bytes)
    base = torch.from_numpy(I.make(kind, B, H, W, 1)).to(dev)
    mask = torch.from_numpy(I.random_mask(B, H, W, 2)).to(dev)
    sets = []
    for _ in range(n):
        ts = (base.clone(), mask.clone(), torch.empty((ws,), dtype=torch.uint8, device=dev), torch.empty_like(base), torch.empty_like(mask),
              torch.empty((B, 1, H, W), dtype=torch.int32, device=dev), torch.empty((B, 3), dtype=torch.int64, device=dev))
        sets.append((ts, [benchkit.ptr(t) for t in ts]))
    st = benchkit.stream()

    def call(k):
        d, m, w, o, mo, lab, cnt = sets[k % n][1]
        m = m if masked else None
        _lib.check(lib.lws_speckle_filter(d, m, B, H, W, 0.5, 50, fill, w, o, mo, lab, cnt, st), "lws_speckle_filter")

    benchkit.warm(call, n + 2)
    runs = benchkit.windows(call, iters)
    us, floor_us = benchkit.median(runs), FLOOR_BYTES * px / benchkit.HBM_TBS / 1e6
    return {"kernel": "lws_speckle_filter", "input": kind, "geometry": f"{B}x{H}x{W}", "mask": masked, "fill": fill, "launches": 5,
            "buffer_sets": n, "us_per_call": round(us, 2), "us_runs": [round(r, 2) for r in runs], "byte_floor_us": round(floor_us, 2),
            "over_byte_floor": round(us / floor_us, 2), "floor_bytes_per_pixel": FLOOR_BYTES, "moved_bytes_per_pixel": MOVED_BYTES,
            "kept_removed": sets[0][0][6].cpu().numpy()[:, 1:].sum(axis=0).tolist()}


def bench_forward(model, B, H, W, iters):
    left, right = benchkit.device_batch(B, H, W)
    benchkit.warm(lambda k: model(left, right), 3)
    return benchkit.median(benchkit.windows(lambda k: model(left, right), iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--forward_iters", type=int, default=10)
    ap.add_argument("--inputs", nargs="+", default=["plateaus", "constant", "checkerboard", "serpentine"])
    ap.add_argument("--no_mask", action="store_true", help="mask = NULL (the serpentine then is ONE component: the longest find walks)")
    a = ap.parse_args()
    benchkit.need_device(__file__)
    lib, dev = benchkit.library(build=True), benchkit.DEV
    model = benchkit.seeded_model()
    for B, H, W in ((1, 368, 1232), (8, 256, 512), (8, 368, 1232)):
        fwd_us = bench_forward(model, B, H, W, a.forward_iters)
        torch.cuda.empty_cache()
        for kind in a.inputs:
            for fill in (0, 1):
                line = bench_filter(lib, kind, B, H, W, fill, a.iters, dev, not a.no_mask)
                line["forward_ms"] = round(fwd_us / 1e3, 3)
                line["over_forward"] = round(line["us_per_call"] / fwd_us, 4)
                print(json.dumps(line), flush=True)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
