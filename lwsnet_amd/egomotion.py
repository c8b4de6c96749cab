"""Visual odometry over a stereo sequence: the frame-to-frame motion that lwsnet_amd.ops.egomotion estimates, chained from frame to
frame and accumulated into camera-to-world poses (include/lwsnet_egomotion.h states the rule).  The counterpart of
lwsnet_amd.geometry.read_kitti_poses: what write_kitti_poses writes, that reader reads back."""
from __future__ import annotations

import numpy as np

from . import geometry, ops

_IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])


class Odometry:
    """Estimates the motion of the left camera from frame to frame.  cameras: one lwsnet_amd.geometry.Camera or a list of B, the
    same for every frame.  The defaults -- 4 pyramid levels of 8 Gauss-Newton steps each, a Huber threshold of 10 grey levels,
    max_jump 1 px inside a 2 x 2 block of the disparity pyramid, no damping, at least 256 pixels per level -- were chosen on a
    synthetic scene only; they have not met real data.  Every argument is checked here, before any GPU work.

    step() takes the frame's uint8 left image [B,H,W,3], its disparity map [B,1,H,W] and code map (the chain's own stage-4 map and
    `keep`, not a fused state) and returns the ops.EgoResult of the motion from the previous frame to this one, or None on the
    first frame.  It keeps copies of the frame for the next step, starts each estimate from the previous one (constant velocity;
    from the identity after an estimate whose status says it is not to be trusted) and accumulates camera-to-world poses in
    float64 on the host, the first one the identity: that reads the 24 numbers of the pose block back once per step."""

    def __init__(self, cameras, levels=4, iters=8, huber=10.0, min_disp=1.0, max_jump=1.0, damping=0.0, min_pixels=256):
        if cameras is None:
            raise ValueError("Odometry needs cameras")
        ops.ego_args(levels, iters, min_disp, max_jump, huber, damping, min_pixels)
        self.cameras = cameras
        self.params = dict(levels=levels, iters=iters, huber=huber, min_disp=min_disp, max_jump=max_jump, damping=damping,
                           min_pixels=min_pixels)
        self.reset()

    def reset(self):
        """Drops the previous frame and the poses: the next step is a first frame."""
        self.prev = None           # (rgb, disp, mask) of the previous frame, copies
        self.last = None           # the EgoResult of the latest estimate
        self.status = []           # per estimate: the status of every image
        self._poses = []           # per frame: float64 [B,3,4] camera-to-world

    def step(self, rgb, disp, mask=None, trace=False, resid=False):
        if self.prev is not None and (tuple(self.prev[1].shape) != tuple(disp.shape) or (self.prev[2] is None) != (mask is None)):
            raise ValueError(f"Odometry.step: disp is {tuple(disp.shape)}{'' if mask is None else ' with a mask'}, the previous frame "
                             f"{tuple(self.prev[1].shape)}{'' if self.prev[2] is None else ' with a mask'} (reset() first)")
        res = None
        if self.prev is None:
            self._poses.append(np.broadcast_to(_IDENTITY, (disp.shape[0], 3, 4)).copy())
        else:
            init = None
            if self.last is not None and not (self.status[-1] & ops.EGO_UNTRUSTED).any():
                init = self.last.pose[:, 0].contiguous()
            res = ops.egomotion(self.prev[0], self.prev[1], rgb, self.cameras, mask=self.prev[2], init=init, trace=trace, resid=resid,
                                **self.params)
            self.last = res
            self.status.append(res.status.cpu().numpy().copy())
            back = res.pose[:, 0].cpu().numpy().astype(np.float64).reshape(-1, 3, 4)      # previous camera into the current one
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


def invert(m):
    """The inverse of a rigid [R|t] float64 [3,4]: R^T, -(R^T t)."""
    R, t = m[:, :3], m[:, 3]
    return np.hstack([R.T, -(R.T @ t)[:, None]])


def compose(a, b):
    """a . b for two [3,4] rigid motions (b applied first)."""
    return np.hstack([a[:, :3] @ b[:, :3], (a[:, :3] @ b[:, 3] + a[:, 3])[:, None]])


def motion_summary(pose_row):
    """(translation in metres, rotation in degrees) of one float [12] motion: what the CLI logs per frame."""
    m = np.asarray(pose_row, np.float64).reshape(3, 4)
    ang = np.degrees(np.arccos(np.clip((np.trace(m[:, :3]) - 1.0) / 2.0, -1.0, 1.0)))
    return float(np.linalg.norm(m[:, 3])), float(ang)
