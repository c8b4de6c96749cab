"""Tracking the camera against the TSDF model: each frame is aligned with the volume's own view of the previous frame's pose by
lwsnet_amd.ops.track -- one joint photometric + point-to-plane cost (include/lwsnet_track.h states the rule) -- and the motions are
accumulated into camera-to-world poses as lwsnet_amd.egomotion.Odometry accumulates its own.  The frame-to-frame estimate is where
the refinement starts; the model is what keeps a chain of two-frame estimates from adding up each frame's depth noise."""
from __future__ import annotations

import numpy as np
import torch

from . import geometry, ops
from .egomotion import _IDENTITY, compose, invert


class ModelTracker:
    """Tracks the left camera against a lwsnet_amd.tsdf.TsdfVolume.  volume: the volume, which the caller integrates each frame
    into at the pose this tracker gave it (poses()[-1], the frame of the first camera); cameras: one lwsnet_amd.geometry.Camera or a
    list of B, the same for every frame.  The defaults -- 6 Gauss-Newton steps, Huber thresholds of 10 grey levels and 1.5 standard
    deviations, a gate of 4 standard deviations, sigma_p 4 grey levels against a disparity sigma of 0.5 px, lambda_g 1, model pixels
    of any weight above w_min 0, at least 256 terms -- were chosen on a synthetic scene only; they have not met real data.  Every
    argument is checked here, before any GPU work.

    step() takes the frame's uint8 left image [B,H,W,3], its own disparity map [B,1,H,W], code map and sigma map (or None), and the
    motion to start from: `init`, the frame-to-frame estimate (a float32 [B,12] device tensor such as EgoResult.pose[:, 0], or host
    numbers), or None for this tracker's last motion (constant velocity).  It ray-casts the volume at the previous frame's tracked
    pose (disparity, weight, normals); with fill, a pixel whose ray met no surface takes the previous frame's own disparity and code
    with a zero normal, so it still carries the photometric term.  It returns the ops.TrackResult, or None on the first frame.
    Where the status says the result is not to be trusted (ops.TRACK_UNTRUSTED) the motion kept is the one it started from.  The
    camera-to-world poses are accumulated in float64 on the host, the first one the identity: that reads the pose block and the
    status back once per step."""

    def __init__(self, volume, cameras, iters=6, huber_p=10.0, sigma_p=4.0, huber_g=1.5, gate_g=4.0, sigma0=0.5, sigma_min=0.05, lambda_g=1.0,
                 min_disp=1.0, damping=0.0, min_pixels=256, w_min=0.0, fill=True, z_near=0.5):
        from .tsdf import TsdfVolume
        if not isinstance(volume, TsdfVolume):
            raise ValueError("ModelTracker needs a TsdfVolume")
        if cameras is None:
            raise ValueError("ModelTracker needs cameras")
        ops.track_args(min_disp, huber_p, sigma_p, huber_g, gate_g, sigma0, sigma_min, lambda_g)
        ops._int_in("iters", iters, 1, 64)
        ops._finite_nonneg("damping", damping)
        ops._int_in("min_pixels", min_pixels, 1, (1 << 31) - 1)
        self.volume, self.cameras = volume, cameras
        self.params = dict(iters=iters, huber_p=huber_p, sigma_p=sigma_p, huber_g=huber_g, gate_g=gate_g, sigma0=sigma0, sigma_min=sigma_min,
                           lambda_g=lambda_g, min_disp=min_disp, damping=damping, min_pixels=min_pixels)
        self.w_min, self.fill, self.z_near = ops._tsdf_w_min(w_min), bool(fill), ops._finite_pos("z_near", z_near)
        self.reset()

    def reset(self):
        """Drops the previous frame and the poses: the next step is a first frame.  The volume is the caller's to reset."""
        self.prev = None           # (rgb, disp, mask) of the previous frame, copies
        self.last = None           # the TrackResult of the latest step
        self.motion = None         # float32 [B,12] device tensor: the motion the latest step kept, or None
        self.view = None           # the ops.TsdfView the latest step aligned with
        self.status = []           # per step: the status of every image
        self._poses = []           # per frame: float64 [B,3,4] camera-to-world

    def model_view(self, H, W):
        """The reference maps of the next step: (disp_ref, normals_ref, mask_ref) from the volume at the last pose, filled from the
        previous frame where asked."""
        view = self.volume.raycast(self.cameras, self._poses[-1], H, W, z_near=self.z_near, w_min=self.w_min, weight=True, normals=True)
        self.view = view
        hit = view.disp > 0
        normals = torch.where(hit, view.normals, torch.zeros_like(view.normals))
        if not self.fill:
            return view.disp, normals, None
        _, disp, mask = self.prev                           # (no code map: every pixel of the previous frame is usable, filled or not)
        keep = None if mask is None else torch.where(hit, torch.ones_like(mask), mask)
        return torch.where(hit, view.disp, disp), normals, keep

    def step(self, rgb, disp, mask=None, sigma=None, init=None, trace=False, resid=False):
        if self.prev is not None and (tuple(self.prev[1].shape) != tuple(disp.shape) or (self.prev[2] is None) != (mask is None)):
            raise ValueError(f"ModelTracker.step: disp is {tuple(disp.shape)}{'' if mask is None else ' with a mask'}, the previous frame "
                             f"{tuple(self.prev[1].shape)}{'' if self.prev[2] is None else ' with a mask'} (reset() first)")
        res = None
        if self.prev is None:
            ops._disp_map(disp, "disp")
            self._poses.append(np.broadcast_to(_IDENTITY, (disp.shape[0], 3, 4)).copy())
        else:
            B, _, H, W = disp.shape
            start = self.motion if init is None else init
            if start is not None:
                start = ops._device_rows(start, "init", (B, 12), disp.device, lambda: ops._motion_rows(start, B, "init", "float32")).contiguous()
            d_ref, n_ref, m_ref = self.model_view(H, W)
            res = ops.track(self.prev[0], d_ref, rgb, disp, self.cameras, normals_ref=n_ref, mask_ref=m_ref, sigma_cur=sigma, mask_cur=mask,
                            init=start, trace=trace, resid=resid, **self.params)
            self.last = res
            status = res.status.cpu().numpy().copy()
            self.status.append(status)
            kept = res.pose[:, 0]
            if (status & ops.TRACK_UNTRUSTED).any():
                first = start if start is not None else torch.from_numpy(np.broadcast_to(_IDENTITY.reshape(12).astype(np.float32), (B, 12)).copy()).to(disp.device)
                bad = torch.from_numpy((status & ops.TRACK_UNTRUSTED) != 0).to(disp.device)
                kept = torch.where(bad[:, None], first, kept)
            self.motion = kept.contiguous()
            back = self.motion.cpu().numpy().astype(np.float64).reshape(-1, 3, 4)      # previous camera into the current one
            self._poses.append(np.stack([compose(T, invert(m)) for T, m in zip(self._poses[-1], back)]))
        self.prev = (rgb.clone(), disp.clone(), None if mask is None else mask.clone())
        return res

    def poses(self, image=0):
        """float64 (N,3,4): the camera-to-world pose of every frame seen so far, for one image of the batch; the first is the identity."""
        if not self._poses:
            return np.zeros((0, 3, 4))
        return np.stack([p[image] for p in self._poses])

    def write_kitti_poses(self, path, image=0):
        geometry.write_kitti_poses(path, self.poses(image))
