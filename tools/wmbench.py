#!/usr/bin/env python3
"""Device time of the edge-aware weighted median filter (development aid, not the judged bench).

    python tools/wmbench.py [--iters N] [--runs N] [--forward_iters N]

For each geometry (1 x 368 x 1232, 8 x 368 x 1232), radius (1, 2, 3), guide (off, on with ops.wmedian_lut(10)) and fill_min (0, 4),
mask and counts on: the median over `--runs` runs of the microseconds per ops.wmedian_filter call, each run `--iters` back-to-back
calls on one stream between two hipEvents (both launches of a call and the output allocation inside), with the fastest and the
slowest run beside it; the same for a plain forward of the same batch (synthetic weights), and each filter time as a share of that
forward.  The input is deterministic: a speckle_inputs plateau map with holes (one pixel in eight, plus its planted specials), the
speckle_inputs code map, and a piecewise-constant guide with a few grey levels of noise.  Everything is warmed up first, and the
shader clock the device held during the stage-1 Conv3D layers of the forward (lws_clock_read) is reported with the numbers.
Prints one JSON line."""
import argparse
import json

import benchkit
import numpy as np
import torch

benchkit.use_tests()

GEOMETRIES = ((1, 368, 1232), (8, 368, 1232))


def piecewise_guide(B, H, W, seed):
    """Constant colour regions (a Voronoi partition of 40 seeds) with noise of up to 3 grey levels per channel."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    K = 40
    cy, cx = rng.uniform(0, H, K), rng.uniform(0, W, K)
    region = np.argmin((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2, axis=0)
    g = rng.integers(0, 256, (K, 3))[region][None] + rng.integers(-3, 4, (B, H, W, 3))
    return np.clip(g, 0, 255).astype(np.uint8)


def filter_inputs(B, H, W, dev):
    import speckle_inputs as I
    d = I.plateaus(B, H, W, 1)
    holes = np.random.default_rng(3).uniform(size=d.shape) < 0.125
    d[holes] = 0.0
    return (torch.from_numpy(d).to(dev), torch.from_numpy(I.random_mask(B, H, W, 2)).to(dev),
            torch.from_numpy(piecewise_guide(B, H, W, 4)).to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--forward_iters", type=int, default=10)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    from lwsnet_amd import ops
    dev = benchkit.DEV
    model = benchkit.seeded_model(build=True)
    wlut = torch.from_numpy(ops.wmedian_lut(10.0)).to(dev)
    result = {"tool": "wmbench", "iters": a.iters, "runs": a.runs, "sigma": 10.0, "geometries": []}
    for B, H, W in GEOMETRIES:
        left, right = benchkit.device_batch(B, H, W)
        benchkit.warm(lambda k: model(left, right), 3)
        fwd = benchkit.summary(benchkit.windows(lambda k: model(left, right), a.forward_iters, a.runs), "_us")
        ghz = benchkit.clock_ghz(model, lambda: model(left, right))
        d, m, g = filter_inputs(B, H, W, dev)
        geo = {"geometry": f"{B}x{H}x{W}", "forward": fwd, "clock_ghz": ghz, "filter": []}
        for radius in (1, 2, 3):
            for guided in (False, True):
                for fill_min in (0, 4):
                    def call(k=None):
                        return ops.wmedian_filter(d, radius, rgb=g if guided else None, wlut=wlut if guided else None, mask=m,
                                                  fill_min=fill_min)
                    for _ in range(5):
                        res = call()
                    torch.cuda.synchronize()
                    t = benchkit.summary(benchkit.windows(call, a.iters, a.runs), "_us")
                    t.update(radius=radius, guide=guided, fill_min=fill_min, over_forward=round(t["us"] / fwd["us"], 4),
                             changed_filled=res.counts.sum(dim=0).tolist())
                    geo["filter"].append(t)
        result["geometries"].append(geo)
        del left, right, d, m, g
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
