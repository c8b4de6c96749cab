"""A truncated signed distance volume over a sequence of disparity maps with poses: the tensors that lwsnet_amd.ops.tsdf_integrate
writes, kept from frame to frame, with the ray-cast and the point extraction on them (include/lwsnet_tsdf.h states the rules), and
the volume that follows the camera by whole voxels and hands what leaves it to the extractors first (include/lwsnet_tsdf_window.h)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from . import geometry, ops


def volume_bytes(dims, colour=False):
    """The device bytes of a volume of dims = (Gx, Gy, Gz): T and Wt float32, C four bytes a voxel."""
    return int(dims[0]) * int(dims[1]) * int(dims[2]) * (12 if colour else 8)


def spill_boxes(dims, shift):
    """The boxes of a volume of dims = (Gx, Gy, Gz) that hold every cell a shift by `shift` voxels loses, as [(start, box_dims), ...]
    in source voxels.  Per axis the source voxels that stay are K = [max(0, s), min(G, G + s)); a cell -- 2 x 2 x 2 voxels, low corner
    i -- is kept iff [i, i + 1] lies in K on all three axes and lost otherwise.  If some K holds fewer than 2 layers no cell is kept:
    the one box is the whole volume.  Otherwise each axis with s != 0, in the order x, y, z, gives one box: on that axis the layers
    0 .. s (s > 0) or G + s - 1 .. G - 1 (s < 0), the layers the lost cells touch; the earlier axes restricted to their K, whose lost
    cells an earlier box holds; the later axes whole.  Every lost cell lies in exactly one box and no kept cell in any.  A pure
    function: no GPU."""
    G, s = [int(v) for v in dims], [int(v) for v in shift]
    if len(G) != 3 or len(s) != 3 or min(G) < 2:
        raise ValueError(f"spill_boxes takes dims (Gx, Gy, Gz), each at least 2, and a shift (sx, sy, sz); got {tuple(dims)} and {tuple(shift)}")
    K = [(max(0, s[e]), min(G[e], G[e] + s[e])) for e in range(3)]
    if any(hi - lo < 2 for lo, hi in K):
        return [((0, 0, 0), tuple(G))]
    boxes = []
    for e in range(3):
        if s[e] == 0:
            continue
        start, box = [0, 0, 0], list(G)
        for earlier in range(e):
            start[earlier], box[earlier] = K[earlier][0], K[earlier][1] - K[earlier][0]
        start[e], box[e] = (0, s[e] + 1) if s[e] > 0 else (G[e] + s[e] - 1, 1 - s[e])
        boxes.append((tuple(start), tuple(box)))
    return boxes


def follow_shift(centre, target, voxel, step):
    """The whole-voxel shift that brings a volume's centre to `target`: d = (target - centre) / voxel per axis in float64; (0, 0, 0)
    unless max |d| >= step, and then rint(d) on all three axes.  A pure function: no GPU."""
    c, t = np.asarray(centre, np.float64), np.asarray(target, np.float64)
    d = (t - c) / np.float64(voxel) if c.shape == t.shape == (3,) and voxel > 0 else np.full(3, np.nan)
    if not np.isfinite(d).all():
        raise ValueError(f"follow_shift takes two finite points and a voxel > 0; got {centre}, {target}, {voxel}")
    if not np.abs(d).max() >= step:
        return (0, 0, 0)
    return tuple(int(v) for v in np.rint(d))


def window_origin(origin0, offset, voxel):
    """The float32 origin of a window `offset` voxels from origin0, per axis float32(origin0 + offset * voxel) computed in float64: a
    shift and its reverse restore the bits, whatever lay between."""
    o = np.asarray(origin0, np.float64) + np.asarray(offset, np.int64).astype(np.float64) * np.float64(voxel)
    return tuple(float(v) for v in o.astype(np.float32))


Chunk = namedtuple("Chunk", ["points", "vnormals", "faces"])
Chunk.__doc__ = """A piece of the map on the host: points uint8 [n,16] (geometry.POINT_DTYPE records in world coordinates), vnormals float32
[n,4], faces int32 [m,3] that index this chunk's points (m = 0 for a chunk of points alone)."""


class MeshChunks:
    """Chunks appended into one vertex list and one face list on the host: a chunk's face indices are offset by the vertices before
    it.  A total of 2^31 vertices or more is refused (a face index is an int32).  write(path, faces=True) goes through
    geometry.write_mesh_ply; without faces the same vertices in the same order."""

    def __init__(self):
        self.points, self.vnormals, self.faces, self.vertices, self.triangles = [], [], [], 0, 0

    def append(self, chunk):
        n = len(chunk.points)
        if self.vertices + n >= 1 << 31:
            raise ValueError(f"the chunks hold {self.vertices + n} vertices, a face indexes fewer than 2^31")
        self.points.append(np.ascontiguousarray(chunk.points, np.uint8).reshape(n, 16))
        self.vnormals.append(np.ascontiguousarray(chunk.vnormals, np.float32).reshape(n, 4))
        self.faces.append((np.asarray(chunk.faces, np.int64).reshape(-1, 3) + self.vertices).astype(np.int32))
        self.vertices, self.triangles = self.vertices + n, self.triangles + len(self.faces[-1])

    def write(self, path, faces=True):
        """Writes the PLY; returns (vertices, faces) written."""
        pts = np.concatenate(self.points) if self.points else np.zeros((0, 16), np.uint8)
        vn = np.concatenate(self.vnormals) if self.vnormals else np.zeros((0, 4), np.float32)
        f = np.concatenate(self.faces) if faces and self.faces else np.zeros((0, 3), np.int32)
        geometry.write_mesh_ply(path, pts.tobytes(), self.vertices, f, vn)
        return self.vertices, len(f)


class TsdfVolume:
    """A dense TSDF volume of fixed extent on one HIP device.  origin: the centre of voxel (0, 0, 0), metres in the frame the poses
    refer to (y down, z forward for KITTI odometry poses); voxel: the voxel's side; dims = (Gx, Gy, Gz).  mu0 (metres) and mu_d (px
    of disparity) set the truncation band max(mu0, mu_d * z^2 / fb); weight "unit" counts frames, "sigma" adds 1 / sigma_z^2 so
    that 1 / Wt is a variance in m^2; w_max caps the weight (a running average that forgets); colour keeps an rgb volume.  Every
    argument is checked here, before any GPU work.  The volume owns T, Wt float32 [Gz,Gy,Gx] and C uint8 [Gz,Gy,Gx,4] (or None); a
    voxel is unobserved iff Wt == 0.  What leaves the volume is not mapped, unless the volume is moved: shift() and follow() move it by
    whole voxels and hand what leaves to the extractors first; origin0 (float64) is the origin it was made with and offset the
    voxels it has moved since, origin = float32(origin0 + offset * voxel).  Movers smear; the poses are taken as given."""

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
        self.origin0, self.offset = np.array(self.origin, np.float64), np.zeros(3, np.int64)
        self._spare = None                                  # the second set of tensors, made by the first shift and swapped by each
        self.kept = None                                    # the int64 [2] {live, cleared} voxels of the last shift, on the device

    def reset(self):
        """Clears the volume: Wt = 0 is all it takes.  It stays where it is."""
        self.Wt.zero_()
        self.frames = 0

    def centre(self):
        """The centre of the voxel lattice, float64 [3]: origin0 + (offset + (dims - 1) / 2) * voxel."""
        return self.origin0 + (self.offset + (np.array(self.dims, np.float64) - 1.0) / 2.0) * np.float64(self.voxel)

    def chunk(self, kind, start=(0, 0, 0), dims=None, max_points=1 << 22, max_faces=1 << 23, w_min=0.0):
        """The box of `dims` voxels from voxel `start` on (default: the whole volume) as a Chunk on the host: kind "points" runs
        ops.tsdf_points on it, "mesh" ops.tsdf_mesh.  A box that is not the whole volume is cut out with ops.tsdf_window first; its
        origin is float32(origin0 + (offset + start) * voxel).  More crossings or faces than the capacities is an error."""
        if kind not in ("points", "mesh"):
            raise ValueError(f"kind must be 'points' or 'mesh', got {kind!r}")
        dims = self.dims if dims is None else tuple(dims)
        whole = tuple(start) == (0, 0, 0) and dims == self.dims
        T, Wt, C = (self.T, self.Wt, self.C) if whole else ops.tsdf_window(self.T, self.Wt, start, dims, C=self.C, counts=False)[:3]
        origin = window_origin(self.origin0, self.offset + np.asarray(start, np.int64), self.voxel)
        if kind == "mesh":
            res = ops.tsdf_mesh(T, Wt, origin, self.voxel, max_points, max_faces, C=C, w_min=w_min)
            n, m = (int(c) for c in res.counts.cpu())
        else:
            res = ops.tsdf_points(T, Wt, origin, self.voxel, max_points, C=C, w_min=w_min)
            n, m = int(res.counts.item()), 0
        if n > max_points:
            raise ValueError(f"the volume has {n} crossings, more than max_points = {max_points}")
        if m > max_faces:
            raise ValueError(f"the mesh has {m} faces, more than max_faces = {max_faces}")
        faces = res.faces[:m].cpu().numpy() if kind == "mesh" else np.zeros((0, 3), np.int32)
        return Chunk(res.points[:n].cpu().numpy(), res.vnormals[:n].cpu().numpy(), faces)

    def shift(self, sx, sy, sz, spill=None, max_points=1 << 22, max_faces=1 << 23, w_min=0.0):
        """Moves the volume by (sx, sy, sz) voxels: voxel i of the moved volume is voxel i + s of this one, what comes in is
        unobserved, origin and grid follow.  spill "points" or "mesh": the boxes of spill_boxes -- every cell the move loses -- are
        cut out and extracted first, each a Chunk on the host, in that order (the capacities are per box); None: what leaves is
        dropped.  The move writes a second set of tensors (allocated by the first move, swapped by each): T, Wt and C are other
        tensors afterwards.  Returns the chunks; `kept` holds the device counts {live, cleared} of the moved volume."""
        s = ops.tsdf_window_args(self.dims, (sx, sy, sz))[3:6]
        if spill not in (None, "points", "mesh"):
            raise ValueError(f"spill must be None, 'points' or 'mesh', got {spill!r}")
        if spill is not None:
            ops._int_in("max_points", max_points, 1, (1 << 31) - 1), ops._int_in("max_faces", max_faces, 1, (1 << 31) - 1), ops._tsdf_w_min(w_min)
        if not any(s):
            return []
        chunks = [] if spill is None else [self.chunk(spill, start, box, max_points=max_points, max_faces=max_faces, w_min=w_min)
                                          for start, box in spill_boxes(self.dims, s)]
        if self._spare is None:
            self._spare = (torch.empty_like(self.T), torch.empty_like(self.Wt), None if self.C is None else torch.empty_like(self.C))
        res = ops.tsdf_window(self.T, self.Wt, s, C=self.C, out=self._spare)
        self._spare, (self.T, self.Wt, self.C) = (self.T, self.Wt, self.C), res[:3]
        self.kept = res.counts
        self.offset = self.offset + np.array(s, np.int64)
        self.grid = ops.tsdf_volume_args(window_origin(self.origin0, self.offset, self.voxel), self.voxel, self.dims)
        self.origin = tuple(self.grid[3:6])
        return chunks

    def follow(self, pose_c2w, anchor, step, spill=None, **kw):
        """Keeps `anchor`, a point in the camera's frame, near the volume's centre: target = R . anchor + t of the camera-to-world
        pose [3,4] in float64; follow_shift(centre(), target, voxel, step) says whether and how far to move, and shift(.., spill, **kw)
        moves.  Returns (the shift, the chunks)."""
        p = np.asarray(pose_c2w, np.float64)
        a = np.asarray(anchor, np.float64)
        if p.shape != (3, 4) or a.shape != (3,) or not (np.isfinite(p).all() and np.isfinite(a).all()):
            raise ValueError("follow takes a finite camera-to-world pose [3,4] and an anchor of three finite numbers")
        s = follow_shift(self.centre(), p[:, :3] @ a + p[:, 3], self.voxel, step)
        return s, self.shift(*s, spill=spill, **kw)

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
