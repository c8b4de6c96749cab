"""The temporal filter over a sequence of disparity maps with known poses: the state that lwsnet_amd.ops.temporal_step advances,
kept from frame to frame (include/lwsnet_temporal.h states the rule)."""
from __future__ import annotations

from . import ops


class TemporalFilter:
    """Fuses the disparity maps of a sequence.  cameras: one lwsnet_amd.geometry.Camera or a list of B, the same for every frame.
    The defaults -- gate 3 standard deviations, no process noise, sigma0 0.5 px where no per-pixel sigma is given, sigma_min
    0.05 px, max_jump 1 px between the four taps of the previous state, q_hold 0.05 px^2 per held frame, max_var 4 px^2 -- were
    chosen on a synthetic scene only; they have not met real data.  Every argument is checked here, before any GPU work.

    step() returns the ops.TemporalResult of the frame; its disp / var / age are the filter's state.  The filter keeps two sets of
    tensors and writes them in turn (ops.temporal_step never writes the state it reads), so a result is overwritten by the step
    after the next one: clone what must live longer."""

    def __init__(self, cameras, gate=3.0, q=0.0, sigma0=0.5, sigma_min=0.05, max_jump=1.0, hold=False, q_hold=0.05, max_var=4.0, min_disp=1.0):
        if cameras is None:
            raise ValueError("TemporalFilter needs cameras")
        ops._temporal_args(sigma0, min_disp, sigma_min, gate, q, max_jump, hold, q_hold, max_var)
        self.cameras = cameras
        self.params = dict(gate=gate, q=q, sigma0=sigma0, sigma_min=sigma_min, max_jump=max_jump, hold=bool(hold), q_hold=q_hold,
                           max_var=max_var, min_disp=min_disp)
        self.state = None          # the (disp, var, age) of the latest step
        self.frames = 0            # steps since the last reset
        self._sets = [None, None]  # the two sets of (disp, var, age, code) tensors, written in turn

    def reset(self):
        """Drops the state: the next step is a first frame."""
        self.state, self.frames = None, 0

    def step(self, disp, pose=None, sigma=None, mask=None, counts=True):
        """One frame.  pose: geometry.relative_pose(T_prev, T_cur), [2,12] or [B,2,12]; None means the first frame, or a reset: the
        state is dropped and the frame starts a new one."""
        if pose is None:
            self.reset()
        elif self.state is None:
            raise ValueError("TemporalFilter.step: a pose was given but there is no previous frame (pass pose=None on the first frame)")
        elif tuple(self.state[0].shape) != tuple(disp.shape):
            raise ValueError(f"TemporalFilter.step: disp is {tuple(disp.shape)}, the state {tuple(self.state[0].shape)} (reset() first)")
        cur = self.frames & 1
        held = self._sets[cur]
        if held is not None and (tuple(held[0].shape) != tuple(disp.shape) or held[0].device != disp.device):
            held = None                                     # another shape or device: ops.temporal_step makes new tensors
        res = ops.temporal_step(disp, self.cameras, pose=pose, prev=self.state, sigma=sigma, mask=mask, counts=counts, out=held,
                                **self.params)
        self._sets[cur] = (res.disp, res.var, res.age, res.code)
        self.state = (res.disp, res.var, res.age)
        self.frames += 1
        return res
