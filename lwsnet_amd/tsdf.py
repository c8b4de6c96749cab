"""A truncated signed distance volume over a sequence of disparity maps with poses: the tensors that lwsnet_amd.ops.tsdf_integrate
writes, kept from frame to frame, with the ray-cast and the point extraction on them (include/lwsnet_tsdf.h states the rules)."""
from __future__ import annotations

import numpy as np
import torch

from . import geometry, ops


def volume_bytes(dims, colour=False):
    """The device bytes of a volume of dims = (Gx, Gy, Gz): T and Wt float32, C four bytes a voxel."""
    return int(dims[0]) * int(dims[1]) * int(dims[2]) * (12 if colour else 8)


class TsdfVolume:
    """A dense TSDF volume of fixed extent on one HIP device.  origin: the centre of voxel (0, 0, 0), metres in the frame the poses
    refer to (y down, z forward for KITTI odometry poses); voxel: the voxel's side; dims = (Gx, Gy, Gz).  mu0 (metres) and mu_d (px
    of disparity) set the truncation band max(mu0, mu_d * z^2 / fb); weight "unit" counts frames, "sigma" adds 1 / sigma_z^2 so
    that 1 / Wt is a variance in m^2; w_max caps the weight (a running average that forgets); colour keeps an rgb volume.  Every
    argument is checked here, before any GPU work.  The volume owns T, Wt float32 [Gz,Gy,Gx] and C uint8 [Gz,Gy,Gx,4] (or None); a
    voxel is unobserved iff Wt == 0.  What leaves the volume is not mapped; movers smear; the poses are taken as given."""

    def __init__(self, origin, voxel, dims, mu0, mu_d=0.0, weight="unit", colour=False, w_max=float("inf"), sigma0=0.5, sigma_min=0.05,
                 min_disp=1.0, max_depth=float("inf"), device="cuda"):
        self.grid = ops.tsdf_volume_args(origin, voxel, dims)
        ops._tsdf_integrate_args(sigma0, min_disp, max_depth, mu0, mu_d, sigma_min, weight, w_max)
        self.origin, self.voxel, self.dims = tuple(self.grid[3:6]), self.grid[6], tuple(self.grid[:3])
        self.params = dict(mu0=mu0, mu_d=mu_d, weight=weight, w_max=w_max, sigma0=sigma0, sigma_min=sigma_min, min_disp=min_disp,
                           max_depth=max_depth)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"TsdfVolume lives on a HIP device (the volume has no CPU fallback), got {device}")
        shape = self.dims[::-1]
        self.T = torch.empty(shape, device=device, dtype=torch.float32)        # never read where Wt == 0
        self.Wt = torch.zeros(shape, device=device, dtype=torch.float32)
        self.C = torch.empty((*shape, 4), device=device, dtype=torch.uint8) if colour else None
        self.frames = 0                                     # frames integrated since the last reset

    def reset(self):
        """Clears the volume: Wt = 0 is all it takes."""
        self.Wt.zero_()
        self.frames = 0

    def integrate(self, disp, cameras, poses_c2w, sigma=None, mask=None, normals=None, rgb=None, updated=True):
        """disp [B,1,H,W] with camera-to-world poses, float64 [3,4] or [B,3,4]: B frames in order.  Returns the voxels taken per
        frame (ops.tsdf_integrate)."""
        B = disp.shape[0] if isinstance(disp, torch.Tensor) and disp.dim() == 4 else 1
        pose = ops.tsdf_pose_rows(poses_c2w, B)
        upd = ops.tsdf_integrate(self.T, self.Wt, self.origin, self.voxel, disp, cameras, pose, C=self.C, sigma=sigma, mask=mask, normals=normals,
                                 rgb=rgb, updated=updated, **self.params)
        self.frames += B
        return upd

    def raycast(self, cameras, pose_c2w, H, W, **kw):
        """The model view of one camera-to-world pose [3,4] (or [B,3,4] with a list of B cameras): ops.tsdf_raycast's TsdfView."""
        p = np.asarray(pose_c2w, np.float64)
        pose = ops.tsdf_pose_rows(p, 1 if p.ndim == 2 else p.shape[0])
        return ops.tsdf_raycast(self.T, self.Wt, self.origin, self.voxel, cameras, pose, H, W, **kw)

    def points(self, max_points, w_min=0.0, with_normals=True):
        """ops.tsdf_points on the volume: the zero crossings as oriented, coloured points in world coordinates."""
        return ops.tsdf_points(self.T, self.Wt, self.origin, self.voxel, max_points, C=self.C, w_min=w_min, with_normals=with_normals)

    def write_ply(self, path, max_points=1 << 22, w_min=0.0):
        """Writes the points with their normals as a binary PLY without faces (geometry.write_mesh_ply; geometry.read_mesh_ply reads
        it).  Returns the number of vertices written; more crossings than max_points is an error, nothing is written then."""
        res = self.points(max_points, w_min=w_min)
        n = int(res.counts.item())
        if n > max_points:
            raise ValueError(f"the volume has {n} crossings, more than max_points = {max_points}")
        geometry.write_mesh_ply(path, res.points[:n].cpu().numpy().tobytes(), n, np.zeros((0, 3), np.int32), res.vnormals[:n].cpu().numpy())
        return n

    def mesh(self, max_points, max_faces, w_min=0.0, with_normals=True):
        """ops.tsdf_mesh on the volume: the points above as the vertices of a triangle mesh, and the faces that index them."""
        return ops.tsdf_mesh(self.T, self.Wt, self.origin, self.voxel, max_points, max_faces, C=self.C, w_min=w_min, with_normals=with_normals)

    def write_mesh_ply(self, path, max_points=1 << 22, max_faces=1 << 23, w_min=0.0):
        """Writes the mesh as a binary PLY of vertices with normals and colours and of triangles (geometry.write_mesh_ply): vertex i is
        vertex i of write_ply's file.  Returns (vertices, faces) written; more of either than its capacity is an error, nothing is
        written then."""
        res = self.mesh(max_points, max_faces, w_min=w_min)
        n, m = (int(c) for c in res.counts.cpu())
        if n > max_points:
            raise ValueError(f"the volume has {n} crossings, more than max_points = {max_points}")
        if m > max_faces:
            raise ValueError(f"the mesh has {m} faces, more than max_faces = {max_faces}")
        geometry.write_mesh_ply(path, res.points[:n].cpu().numpy().tobytes(), n, res.faces[:m].cpu().numpy(), res.vnormals[:n].cpu().numpy())
        return n, m
