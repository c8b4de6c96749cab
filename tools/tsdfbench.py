#!/usr/bin/env python3
"""The TSDF calls timed with device events (development aid, not the judged bench).

    python tools/tsdfbench.py [--iters N] [--runs R]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/tsdfbench.py --iters 20 --runs 1      # the k_ts_* kernels one by one

The scene is synthetic and exact: a road 1.65 m below the camera and a wall 30 m ahead, rendered at 368 x 1232 with a KITTI camera
from four poses 0.5 m apart, with the normals of ops.surface_normals and a random colour image.  The volume is the inference CLI's
default: 129 x 33 x 257 voxels of 0.2 m from (-12.8, -3.2, 0), a band of 0.6 m, unit weights.  Timed on buffers allocated once,
after a warm-up, R windows of N calls between two events, the median window per call: lws_tsdf_integrate of one frame into the
volume the four frames left (normals, colour and `updated`: two launches), the same without normals, colour and `updated` (one
launch), of the four frames in one call, lws_tsdf_raycast of the third pose (step 0.1 m) with weight and normals and without,
lws_tsdf_points, and lws_tsdf_mesh on the same volume (the three launches of the points and three more).  A window integrates the same frame again and again, so the weights grow; the arithmetic per voxel does not depend
on them.  Then lws_tsdf_window (include/lwsnet_tsdf_window.h), the move of a volume that follows the camera, into a second set of
tensors: a volume of 128 x 32 x 256 voxels with colour cut out of the one above (rows of 512 bytes: every quad is a 16-byte word
on both sides when sx is a multiple of 4) for sx = 16 and sx = 5, the same with every voxel observed, and the 129 x 33 x 257 volume itself for sx = 16 (rows of 516 bytes: three rows in four begin off
a 16-byte boundary and go voxel by voxel); beside each, in the same run, plain Tensor.copy_ of the same three tensors, which moves
the same bytes, and the window's time over the copy's.  Prints one JSON line with the times, the voxels taken per frame, the pixels
that hit, the points and the faces found."""
import argparse
import ctypes
import json

import benchkit
import numpy as np
import torch

H, W = 368, 1232
CAM = benchkit.KITTI
ORIGIN, VOXEL, DIMS, MU0 = (-12.8, -3.2, 0.0), 0.2, (129, 33, 257), 0.6


def render(dz):
    """The true disparity float32 [H,W] of the road and the wall from a camera dz metres ahead of the first."""
    fx, fy, cx, cy, b = CAM
    ys = (np.arange(H, dtype=np.float64)[:, None] - cy) / fy
    with np.errstate(divide="ignore"):
        road = np.where(ys > 0, 1.65 / ys, np.inf)
    depth = np.minimum(np.broadcast_to(road, (H, W)), 30.0 - dz)
    return (fx * b / depth).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=7)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    from lwsnet_amd import _lib, ops
    from lwsnet_amd.geometry import Camera, camera_rows
    from lwsnet_amd.tsdf import TsdfVolume
    benchkit.library()
    dev = benchkit.DEV
    cam1 = Camera(*CAM)
    n = 4
    rng = np.random.default_rng(0)
    poses = np.stack([np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0.5 * k]], np.float64) for k in range(n)])
    disp = torch.from_numpy(np.stack([render(0.5 * k) for k in range(n)])[:, None]).to(dev)
    rgb = torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).to(dev)
    normals = ops.surface_normals(disp, [cam1] * n, max_jump=1.0)[0]
    vol = TsdfVolume(ORIGIN, VOXEL, DIMS, mu0=MU0, colour=True, device=dev)
    updated = vol.integrate(disp, [cam1] * n, poses, normals=normals, rgb=rgb)
    view = vol.raycast(cam1, poses[2], H, W, z_near=0.5, step=0.1, nsteps=560)
    pts = vol.points(1 << 22)
    msh = vol.mesh(1 << 22, 1 << 23)
    line = {"tool": "tsdfbench", "map": f"{H}x{W}", "volume": "x".join(str(d) for d in DIMS), "voxel": VOXEL, "iters": a.iters, "runs": a.runs,
            "updated_per_frame": updated.cpu().tolist(), "pixels_hit": int((view.disp > 0).sum()), "points_found": int(pts.counts[0]),
            "faces_found": int(msh.counts[1])}

    P, stream = benchkit.ptr, benchkit.stream()
    cam = torch.from_numpy(camera_rows([cam1] * n, n)).to(dev)
    pose = torch.from_numpy(ops.tsdf_pose_rows(poses, n)).to(dev)
    grid = (*DIMS, *ORIGIN, VOXEL)
    upd = torch.empty((n,), dtype=torch.int64, device=dev)
    work = torch.empty((_lib.nbytes("lws_tsdf_points_workspace", DIMS[1], DIMS[2]),), dtype=torch.uint8, device=dev)
    mwork = torch.empty((_lib.nbytes("lws_tsdf_mesh_workspace", DIMS[1], DIMS[2]),), dtype=torch.uint8, device=dev)

    def integrate(B, full):
        _lib.call("lws_tsdf_integrate", P(disp), None, None, P(normals) if full else None, P(rgb) if full else None, P(cam), P(pose), B, H, W, P(vol.T),
                  P(vol.Wt), P(vol.C) if full else None, *grid, 0.5, 1.0, float("inf"), MU0, 0.0, 0.05, 0, float("inf"), P(upd) if full else None, stream)

    def raycast(full):
        _lib.call("lws_tsdf_raycast", P(vol.T), P(vol.Wt), *grid, P(cam[2:]), P(pose[2:]), 1, H, W, 0.5, 0.1, 560, 0.0, P(view.disp),
                  P(view.weight) if full else None, P(view.normals) if full else None, stream)

    def points(k=None):
        _lib.call("lws_tsdf_points", P(vol.T), P(vol.Wt), P(vol.C), *grid, 0.0, ctypes.c_int64(1 << 22), P(work), P(pts.points), P(pts.vnormals),
                  P(pts.counts), stream)

    def mesh(k=None):
        _lib.call("lws_tsdf_mesh", P(vol.T), P(vol.Wt), P(vol.C), *grid, 0.0, ctypes.c_int64(1 << 22), ctypes.c_int64(1 << 23), P(mwork), P(msh.points),
                  P(msh.vnormals), P(msh.faces), P(msh.counts), stream)

    for name, call, iters in (("integrate_1_frame", lambda k: integrate(1, True), a.iters), ("integrate_1_frame_plain", lambda k: integrate(1, False), a.iters),
                              ("integrate_4_frames", lambda k: integrate(4, True), a.iters), ("raycast", lambda k: raycast(True), max(1, a.iters // 5)),
                              ("raycast_disp_only", lambda k: raycast(False), max(1, a.iters // 5)), ("points", points, a.iters), ("mesh", mesh, a.iters), ("points_again", points, a.iters),
                              ("integrate_1_frame_again", lambda k: integrate(1, True), a.iters)):
        benchkit.warm(call, 5)
        line[name] = benchkit.summary(benchkit.windows(call, iters, a.runs))

    # the window against a plain copy of the same tensors
    def window_rows(tag, T, Wt, C, shifts):
        g = T.shape[::-1]
        out = tuple(torch.empty_like(t) for t in (T, Wt, C))
        counts = torch.empty((2,), dtype=torch.int64, device=dev)

        def copy(k=None):
            for dst, src in zip(out, (T, Wt, C)):
                dst.copy_(src)
        benchkit.warm(copy, 5)
        line["copy" + tag] = benchkit.summary(benchkit.windows(copy, a.iters, a.runs))
        for sx in shifts:
            def window(k=None):
                _lib.call("lws_tsdf_window", P(T), P(Wt), P(C), *g, sx, 0, 0, P(out[0]), P(out[1]), P(out[2]), *g, P(counts), stream)
            benchkit.warm(window, 5)
            name = f"window{tag}_sx{sx}"
            line[name] = benchkit.summary(benchkit.windows(window, a.iters, a.runs))
            line[name]["live"] = int(counts[0])
            line[name]["over_copy"] = round(line[name]["us"] / line["copy" + tag]["us"], 2)

    cut = ops.tsdf_window(vol.T, vol.Wt, (0, 0, 0), (128, 32, 256), C=vol.C, counts=False)
    window_rows("_128x32x256", cut.T, cut.Wt, cut.C, (16, 5))
    window_rows("_128x32x256_all_observed", cut.T, torch.ones_like(cut.Wt), cut.C, (16, 5))
    window_rows("_129x33x257", vol.T, vol.Wt, vol.C, (16,))
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
