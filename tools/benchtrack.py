#!/usr/bin/env python3
"""lws_track_normal beside lws_ego_normal, and lws_track beside the ray-cast it needs, timed with device events (development aid,
not the judged bench).  Named bench-first: tests/test_benchkit_cpu.py pins the set of tools/*bench.py, and tests/test_track_cpu.py holds this
tool to the same rule -- the timing method is benchkit's, stated nowhere else.

    python tools/benchtrack.py [--iters N] [--runs R] [--gn_iters I]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/benchtrack.py --iters 20 --runs 1      # the k_track_* kernels one by one

Per shape (256 x 512, 368 x 1232) at batch 1: the model view is a road plane under the KITTI camera with the plane's normal, the
grey images a smooth texture and the same texture moved one pixel to the right (so that the Gauss-Newton steps are taken and not
refused), the current disparity the plane with 0.2 px of seeded noise.  Timed on buffers allocated once, a warm-up and R windows of N
calls between two events, the median window per call:
  ego_normal        lws_ego_normal at level 0: the photometric pass alone, the parent's kernel and the yardstick
  track_photo       lws_track_normal with lambda_g = 0: the same pass through the fused kernel
  track_joint       lws_track_normal with both terms; joint - photo is what the geometric term adds inside the fused pass, to be held
                    against a pass of its own, which would pay the launches, the reference reads and the projection again
  track             lws_track, --gn_iters steps, eagerly and replayed from a captured graph
  raycast           ops.tsdf_raycast of the same view (disparity, weight, normals) from a volume the plane was integrated into
Prints one JSON line per shape."""
import argparse
import json

import benchkit
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--gn_iters", type=int, default=6)
    a = ap.parse_args()
    benchkit.need_device(__file__)
    from lwsnet_amd import _lib, ops
    from lwsnet_amd.geometry import Camera, camera_rows
    from lwsnet_amd.tsdf import TsdfVolume
    benchkit.library()
    dev = benchkit.DEV
    P, stream = benchkit.ptr, benchkit.stream
    fx, fy, _, _, baseline = benchkit.KITTI
    for H, W in ((256, 512), (368, 1232)):
        B = 1
        camera = Camera(fx, fy, (W - 1) / 2.0, 0.35 * (H - 1), baseline)
        cam = torch.from_numpy(camera_rows([camera], B)).to(dev)
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        height = 1.65                                       # the camera above the road, metres
        z = np.where(yy > camera.cy + 4, fy * height / np.maximum(yy - camera.cy, 1e-9), 0.0)
        disp0 = np.where(z > 0, fx * baseline / np.maximum(z, 1e-9), 0.0).astype(np.float32)
        rng = np.random.default_rng(0)
        disp1 = np.where(disp0 > 0, disp0 + 0.2 * rng.standard_normal(disp0.shape), 0.0).astype(np.float32)
        grey = 128.0 + 60.0 * np.sin(0.11 * xx + 0.5) * np.cos(0.07 * yy) + 40.0 * np.cos(0.05 * xx - 0.13 * yy)
        rgb0 = np.repeat(np.clip(np.rint(grey), 0, 255).astype(np.uint8)[None, ..., None], 3, -1)
        rgb1 = np.ascontiguousarray(np.roll(rgb0, 1, axis=2))
        normals = np.zeros((B, 3, H, W), np.float32)
        normals[:, 1] = np.where(disp0 > 0, -1.0, 0.0)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)              # noqa: E731
        d_ref, d_cur, n_ref, r0, r1 = t(disp0[None, None]), t(disp1[None, None]), t(normals), t(rgb0), t(rgb1)
        g0, g1 = (t(((77 * x[..., 0].astype(np.int64) + 150 * x[..., 1] + 29 * x[..., 2]) / 256.0).astype(np.float32)[:, None]) for x in (rgb0, rgb1))
        M = t(np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], np.float64))
        work = torch.empty((max(_lib.nbytes("lws_track_workspace", B, H, W), _lib.nbytes("lws_egomotion_workspace", B, H, W, 1)),), device=dev, dtype=torch.uint8)
        sums = torch.empty((B, 32), device=dev, dtype=torch.float64)
        pose = torch.empty((B, 2, 12), device=dev, dtype=torch.float32)
        status = torch.empty((B,), device=dev, dtype=torch.int32)
        info = torch.empty((B, 6), device=dev, dtype=torch.float64)

        def ego_normal(k=None):
            _lib.call("lws_ego_normal", P(g0), P(d_ref), None, P(g1), P(cam), P(M), B, H, W, 0, 1.0, 10.0, P(work), P(sums), None, stream())

        def normal(lambda_g):
            return lambda k=None: _lib.call("lws_track_normal", P(g0), P(d_ref), P(n_ref), None, P(g1), P(d_cur), None, None, P(cam), P(M), B, H, W,
                                            1.0, 10.0, 4.0, 1.5, 4.0, 0.2, 0.05, lambda_g, P(work), P(sums), None, stream())

        def track(k=None):
            _lib.call("lws_track", P(r0), P(d_ref), P(n_ref), None, P(r1), P(d_cur), None, None, P(cam), None, B, H, W, a.gn_iters, 1.0, 10.0, 4.0, 1.5,
                      4.0, 0.2, 0.05, 1.0, 0.0, 256, P(work), P(pose), P(status), P(info), None, None, stream())

        line = {"tool": "benchtrack", "geometry": f"{B}x{H}x{W}", "gn_iters": a.gn_iters, "iters": a.iters, "runs": a.runs, "launches": 2 * a.gn_iters + 3}
        for name, call in (("ego_normal", ego_normal), ("track_photo", normal(0.0)), ("track_joint", normal(1.0)),
                           ("track", track)):
            benchkit.warm(call, 5)
            line[name] = benchkit.summary(benchkit.windows(call, a.iters, a.runs))
            if name == "track_joint":
                line["n_p"], line["n_g"] = int(sums[0, 28]), int(sums[0, 30])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            track()
        graph.replay()
        torch.cuda.synchronize()
        line["track_graph"] = benchkit.summary(benchkit.windows(lambda k: graph.replay(), a.iters, a.runs))
        line["status"], line["info"] = int(status[0]), [round(v, 4) for v in info[0].cpu().tolist()]
        vol = TsdfVolume((-12.8, -1.6, 0.0), 0.2, (129, 25, 257), mu0=0.6, device=dev)
        identity = np.hstack([np.eye(3), np.zeros((3, 1))])
        vol.integrate(d_ref, camera, identity, normals=n_ref)
        pose_rows = torch.from_numpy(ops.tsdf_pose_rows(identity, B)).to(dev)
        cast = lambda k=None: ops.tsdf_raycast(vol.T, vol.Wt, vol.origin, vol.voxel, camera, pose_rows, H, W, z_near=0.5)      # noqa: E731
        benchkit.warm(cast, 3)
        line["raycast"] = benchkit.summary(benchkit.windows(cast, max(1, a.iters // 5), a.runs))
        line["joint_over_ego_normal"] = round(line["track_joint"]["us"] / line["ego_normal"]["us"], 3)
        line["geometric_increment_us"] = round(line["track_joint"]["us"] - line["track_photo"]["us"], 2)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
