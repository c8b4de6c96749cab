"""Moving objects over a stereo sequence: the previous frame's maps kept on the device from frame to frame, and
lwsnet_amd.ops.movers on each pair of consecutive frames (include/lwsnet_movers.h states the rule)."""
from __future__ import annotations

from . import ops


class MoverSegmenter:
    """Segments what moves between consecutive frames.  cameras: one lwsnet_amd.geometry.Camera or a list of B, the same for every
    frame; params: the keyword arguments of ops.movers (gates, radius, cand_bits, min_pixels, grow, ...).  The defaults -- a gate of
    3 standard deviations on the disparity, 25 grey levels on the image, one tap, movers of at least 64 pixels grown by 2 -- were
    chosen on synthetic scenes only; they have not met real data.  Every argument is checked here, before any GPU work.

    step() takes the frame's uint8 left image [B,H,W,3], its disparity map [B,1,H,W], the motion from the previous frame to this one
    (the pose block of ops.egomotion / ops.track, or geometry.relative_pose) and, optionally, its code map and sigma; it returns the
    ops.MoversResult of this frame against the previous one, or None on a first frame and when pose is None (no trusted motion: the
    frame is not segmented).  Either way it keeps copies of the frame's maps for the next step; nothing is read back."""

    def __init__(self, cameras, **params):
        if cameras is None:
            raise ValueError("MoverSegmenter needs cameras")
        unknown = set(params) - set(ops.MOVERS_DEFAULTS)
        if unknown:
            raise ValueError(f"MoverSegmenter: unknown parameters {sorted(unknown)}")
        self.params = {**ops.MOVERS_DEFAULTS, **params}
        ops.movers_args(**self.params)
        self.cameras = cameras
        self.reset()

    def reset(self):
        """Drops the previous frame: the next step is a first frame."""
        self.prev = None           # (rgb, disp, mask, sigma) of the previous frame, copies

    def step(self, rgb, disp, pose, mask=None, sigma=None, labels=True):
        res = None
        if self.prev is not None and pose is not None:
            if tuple(self.prev[1].shape) != tuple(disp.shape):
                raise ValueError(f"MoverSegmenter.step: disp is {tuple(disp.shape)}, the previous frame {tuple(self.prev[1].shape)} (reset() first)")
            p_rgb, p_disp, p_mask, p_sigma = self.prev
            res = ops.movers(p_rgb, p_disp, rgb, disp, self.cameras, pose, sigma_prev=p_sigma, mask_prev=p_mask, sigma_cur=sigma, mask_cur=mask,
                             labels=labels, **self.params)
        self.prev = (rgb.clone(), disp.clone(), None if mask is None else mask.clone(), None if sigma is None else sigma.clone())
        return res
