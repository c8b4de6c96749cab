#!/usr/bin/env python3
"""Device time of the ground kernels (development aid, not the judged bench).

    python tools/groundbench.py [--iters N]

For each geometry (1 x 368 x 1232, 8 x 368 x 1232) one JSON line with the device time of each of the four calls of
lwsnet_amd.ops.ground at its defaults -- lws_vdisparity (768 bins of a quarter pixel), lws_ground_fit (185 horizon rows x 512
bottom bins, three passes after the voted line; and once with iters = 0, which leaves the vote and one pass), lws_ground_classify
(height, codes and counts) and lws_bev_grid (200 x 300 cells, count and hmax) -- and their sum.  The inputs are a road (a plane
in disparity with a horizon near row 165, a little roll and a quarter pixel of noise) with boxes of constant disparity standing
on it and a code map that keeps ~80 % of the pixels; each call reads what the call before it wrote for the same buffer set.
Buffer rotation and timing are tools/benchkit.py's: more than 256 MiB of distinct buffer sets, hipEvents around back-to-back calls
on one stream, the median of five runs."""
import argparse
import json

import benchkit
import torch
from gbench import BASELINE, FX

SUB, NBINS, TOL_BINS, MIN_SCORE, TOL0, TOL, ITERS = 4, 768, 1, 0, 1.0, 1.0, 3
MIN_DISP, MAX_DEPTH, GROUND_TOL, MAX_HEIGHT = 1.0, float("inf"), 0.2, 3.0
CODE_BITS, X_MIN, CELL, GX, GZ = 1 << 2, -20.0, 0.2, 200, 300


def inputs(B, H, W, dev, g):
    ys = torch.arange(H, device=dev, dtype=torch.float32).view(1, 1, H, 1)
    xs = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, 1, W)
    roll = (torch.rand((B, 1, 1, 1), device=dev, generator=g) - 0.5) * 0.004
    disp = 0.323 * (ys - 165.0) + roll * (xs - W / 2) + 0.25 * torch.randn((B, 1, H, W), device=dev, generator=g)
    for x0, x1, y0, y1, d in ((150, 330, 150, 233, 22.0), (620, 760, 160, 211, 15.0), (900, 1180, 120, 282, 38.0)):
        disp[:, :, y0:y1, x0:x1] = d
    disp = torch.where(disp > 0.5, disp, torch.zeros_like(disp))
    mask = (torch.rand((B, 1, H, W), device=dev, generator=g) < 0.8).to(torch.uint8)
    return disp.contiguous(), mask


def bench(lib, B, H, W, iters, dev):
    from lwsnet_amd import _lib
    px = B * H * W
    set_bytes = (4 + 1 + 4 + 1) * px + 4 * B * H * NBINS + 8 * B * GX * GZ
    n = benchkit.n_sets(set_bytes)
    g = torch.Generator(device=dev).manual_seed(4)
    cam = torch.tensor([[FX, FX, 600.0, 170.0, FX * BASELINE]] * B, dtype=torch.float32, device=dev)
    work = torch.empty((int(lib.lws_ground_workspace(B, H, NBINS)),), dtype=torch.uint8, device=dev)
    yh, qb = (H // 4, min(3 * H // 4, H - 2)), (NBINS // 3, NBINS - 1)
    st = benchkit.stream()
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)                # noqa: E731
    sets = [inputs(B, H, W, dev, g) + (e((B, H, NBINS), torch.uint32), e((B, 4), torch.float32), e((B, 8), torch.int32),
                                       e((B, 1, H, W), torch.float32), e((B, 1, H, W), torch.uint8), e((B, 6), torch.int64),
                                       e((B, GZ, GX), torch.uint32), e((B, GZ, GX), torch.float32)) for _ in range(n)]

    def hist(k):
        s = sets[k % n]
        _lib.check(lib.lws_vdisparity(s[0].data_ptr(), s[1].data_ptr(), B, H, W, MIN_DISP, SUB, NBINS, s[2].data_ptr(), st), "lws_vdisparity")

    def fit(k, it=ITERS):
        s = sets[k % n]
        _lib.check(lib.lws_ground_fit(s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), B, H, W, MIN_DISP, SUB, NBINS, *yh, *qb, TOL_BINS,
                                      MIN_SCORE, TOL0, TOL, it, work.data_ptr(), s[3].data_ptr(), s[4].data_ptr(), st), "lws_ground_fit")

    def classify(k):
        s = sets[k % n]
        _lib.check(lib.lws_ground_classify(s[0].data_ptr(), s[1].data_ptr(), cam.data_ptr(), s[3].data_ptr(), B, H, W, MIN_DISP, MAX_DEPTH,
                                           GROUND_TOL, MAX_HEIGHT, s[5].data_ptr(), s[6].data_ptr(), s[7].data_ptr(), st), "lws_ground_classify")

    def bev(k):
        s = sets[k % n]
        _lib.check(lib.lws_bev_grid(s[0].data_ptr(), cam.data_ptr(), s[6].data_ptr(), s[5].data_ptr(), B, H, W, MIN_DISP, MAX_DEPTH, CODE_BITS,
                                    X_MIN, CELL, GX, GZ, s[8].data_ptr(), s[9].data_ptr(), st), "lws_bev_grid")

    out = {"geometry": f"{B}x{H}x{W}", "buffer_sets": n, "candidates": (yh[1] - yh[0] + 1) * (qb[1] - qb[0] + 1)}
    calls = (("vdisparity", hist), ("ground_fit_iters0", lambda k: fit(k, 0)), ("ground_fit", fit), ("ground_classify", classify),
             ("bev_grid", bev))
    for name, call in calls:                                # in this order: each reads what the one before wrote
        benchkit.warm(call, 2 * n)
        out[name] = benchkit.per_call(benchkit.windows(call, iters))
    info, counts = sets[0][4].cpu(), sets[0][7].cpu()
    out["status"], out["inlier_share"] = info[:, 0].tolist(), round(float(info[:, 4].sum()) / max(int(counts[:, 1:].sum()), 1), 4)
    out["codes"] = counts.sum(dim=0).tolist()
    out["total_us"] = round(sum(out[name]["us_per_call"] for name in ("vdisparity", "ground_fit", "ground_classify", "bev_grid")), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    lib, dev = benchkit.library(), benchkit.DEV
    for B, H, W in ((1, 368, 1232), (8, 368, 1232)):
        print(json.dumps(bench(lib, B, H, W, a.iters, dev)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
