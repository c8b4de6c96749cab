"""Cameras and point-cloud files for the geometry outputs (metric depth, KITTI 16-bit PNGs, point clouds; include/lwsnet_hip.h,
lws_depth_maps / lws_point_cloud).  numpy only: the device side is lwsnet_amd.ops.depth_maps / point_cloud."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .imageio import CROP_H, CROP_W

POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                        ("alpha", "u1")])   # the 16-byte device record of lws_point_cloud


@dataclass(frozen=True)
class Camera:
    """A rectified stereo camera: focal lengths and principal point in pixels, baseline in metres."""
    fx: float
    fy: float
    cx: float
    cy: float
    baseline: float

    @property
    def fb(self):
        """fx * baseline as the kernels take it: float32(float64(fx) * float64(baseline))."""
        return float(np.float32(float(self.fx) * float(self.baseline)))

    def row(self):
        """The float32 row {fx, fy, cx, cy, fb} of the device camera array."""
        return np.array([self.fx, self.fy, self.cx, self.cy, self.fb], np.float32)

    def check(self):
        vals = (self.fx, self.fy, self.cx, self.cy, self.baseline)
        if not all(np.isfinite(v) for v in vals) or self.fx <= 0 or self.fy <= 0 or self.baseline <= 0:
            raise ValueError(f"camera needs finite values with fx, fy, baseline > 0; got {self}")
        return self

    @classmethod
    def from_kitti(cls, path):
        """Reads a KITTI calibration file: the 2015 `calib_cam_to_cam/*.txt` (P_rect_02, P_rect_03) or the object / odometry
        `calib/*.txt` (P2, P3).  fx, fy, cx, cy come from the left colour camera's projection matrix; baseline =
        (P2[0,3] - P3[0,3]) / fx."""
        mats = {}
        with open(path, encoding="utf-8", errors="replace") as f:
            for line in f:
                key, sep, rest = line.partition(":")
                if not sep:
                    continue
                try:
                    vals = [float(v) for v in rest.split()]
                except ValueError:                              # calib_time: 09-Jan-2012 13:57:47
                    continue
                mats[key.strip()] = vals
        for k2, k3 in (("P_rect_02", "P_rect_03"), ("P2", "P3")):
            if k2 in mats and k3 in mats:
                break
        else:
            raise ValueError(f"{path}: no P_rect_02 / P_rect_03 or P2 / P3 projection matrices")
        if len(mats[k2]) != 12 or len(mats[k3]) != 12:
            raise ValueError(f"{path}: {k2} / {k3} must hold 12 values")
        p2, p3 = np.array(mats[k2]).reshape(3, 4), np.array(mats[k3]).reshape(3, 4)
        fx = p2[0, 0]
        if not fx > 0:
            raise ValueError(f"{path}: focal length {fx} is not positive")
        baseline = (p2[0, 3] - p3[0, 3]) / fx
        if not baseline > 0:
            raise ValueError(f"{path}: baseline {baseline} is not positive")
        try:
            return cls(float(fx), float(p2[1, 1]), float(p2[0, 2]), float(p2[1, 2]), float(baseline)).check()
        except ValueError as e:
            raise ValueError(f"{path}: {e}") from None

    def crop_bottom_right(self, h, w, th=CROP_H, tw=CROP_W):
        """The camera of lwsnet_amd.imageio.crop_bottom_right's crop of an h x w image: the principal point moves by the rows and
        columns cut away."""
        return Camera(self.fx, self.fy, self.cx - (w - tw), self.cy - (h - th), self.baseline)


def camera_rows(cameras, B):
    """One Camera or a list of B -> float32 [B,5]."""
    cams = [cameras] * B if isinstance(cameras, Camera) else list(cameras)
    if len(cams) != B or not all(isinstance(c, Camera) for c in cams):
        raise ValueError(f"cameras must be one Camera or a list of {B}")
    return np.stack([c.check().row() for c in cams])


def ply_bytes(points_bytes, n):
    """Binary little-endian PLY of n records laid out as the device writes them (POINT_DTYPE)."""
    data = memoryview(points_bytes).cast("B")
    if len(data) < 16 * n:
        raise ValueError(f"{len(data)} bytes hold fewer than {n} points")
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex {}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n").format(n)
    return header.encode("ascii") + bytes(data[:16 * n])


def write_ply(path, points_bytes, n):
    with open(path, "wb") as f:
        f.write(ply_bytes(points_bytes, n))


def read_ply(path):
    """The vertices of a file write_ply wrote, as a POINT_DTYPE array."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    n = int(next(l for l in data[:end].decode("ascii").splitlines() if l.startswith("element vertex")).split()[2])
    return np.frombuffer(data, POINT_DTYPE, count=n, offset=end)
