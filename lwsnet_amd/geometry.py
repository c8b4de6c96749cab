"""Cameras, point-cloud and mesh files for the geometry outputs (metric depth, KITTI 16-bit PNGs, point clouds, triangle meshes;
include/lwsnet_hip.h, lws_depth_maps / lws_point_cloud / lws_surface_mesh) and the calibration of a raw stereo rig for the rectifying
front end (lws_rectify_pair).  numpy only: the device side is lwsnet_amd.ops.depth_maps / point_cloud / surface_normals /
surface_mesh / rectify_pair."""
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
        mats = _read_kitti_values(path)
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


@dataclass(frozen=True)
class GroundPlane:
    """The road of lwsnet_amd.ops.ground_fit as the camera sees it: its `height` over the road in metres, `pitch_deg` (> 0: the
    camera looks down, the horizon lies above the principal point), `roll_deg` (> 0: the road's normal leans towards +x) and the
    unit `normal` (nx, ny, nz) of the plane nx*X + ny*Y + nz*Z = height in camera coordinates (x right, y down, z forward)."""
    height: float
    pitch_deg: float
    roll_deg: float
    normal: tuple

    @classmethod
    def from_plane(cls, plane, camera):
        """plane: a row {a, b, c, ...} of ground_fit's output, the road's disparity d = a*x + b*y + c in the pixel coordinates of
        `camera` (a Camera, cropped as the map is).  Host float64: (nx, ny, nz) = (a*fx, b*fy, a*cx + b*cy + c), the plane is
        nx*X + ny*Y + nz*Z = fb.  None for a plane that is not finite (no ground, degenerate) or has no normal."""
        a, b, c = (float(v) for v in np.asarray(plane, np.float64).reshape(-1)[:3])
        cam = camera.check()
        n = np.array([a * float(cam.fx), b * float(cam.fy), a * float(cam.cx) + b * float(cam.cy) + c])
        length = float(np.sqrt(n @ n))
        if not (np.isfinite(length) and length > 0.0):
            return None
        n = n / length
        return cls(float(cam.fb) / length, float(np.degrees(np.arctan2(n[2], np.hypot(n[0], n[1])))),
                   float(np.degrees(np.arctan2(n[0], n[1]))), tuple(float(v) for v in n))


def read_kitti_poses(path):
    """The poses of a KITTI odometry `poses.txt`: float64 (N,3,4), line i the row-major [R|t] that maps a point of the left camera's
    frame at time i into the world (camera-to-world).  Every line holds 12 numbers; empty lines are skipped."""
    rows = []
    with open(path, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            if not line.strip():
                continue
            try:
                v = [float(t) for t in line.split()]
            except ValueError:
                raise ValueError(f"{path}:{n}: not a line of numbers") from None
            if len(v) != 12 or not np.isfinite(v).all():
                raise ValueError(f"{path}:{n}: a pose is 12 finite numbers (a row-major 3x4 [R|t]), got {len(v)}")
            rows.append(v)
    return np.asarray(rows, np.float64).reshape(-1, 3, 4)


def write_kitti_poses(path, poses):
    """Writes camera-to-world poses, float64 (N,3,4), as a KITTI odometry `poses.txt`: line i the 12 numbers of the row-major [R|t]
    of frame i, each with the digits that read back to the same float64 (read_kitti_poses returns exactly `poses`)."""
    p = np.asarray(poses, np.float64)
    if p.ndim != 3 or p.shape[1:] != (3, 4) or not np.isfinite(p).all():
        raise ValueError(f"poses must be finite (N,3,4) camera-to-world [R|t], got shape {p.shape}")
    with open(path, "w", encoding="utf-8") as f:
        for row in p.reshape(-1, 12):
            f.write(" ".join(repr(float(v)) for v in row) + "\n")


def _pose44(T, name):
    T = np.asarray(T, np.float64)
    if T.shape != (3, 4) or not np.isfinite(T).all():
        raise ValueError(f"{name} must be a finite 3x4 [R|t], got shape {T.shape}")
    return np.vstack([T, [0.0, 0.0, 0.0, 1.0]])


def relative_pose(T_prev, T_cur):
    """The `pose` rows of lwsnet_amd.ops.temporal_step for one image, float32 [2][12]: inv(T_cur) . T_prev, which maps a point of
    the previous camera's frame into the current one, and its inverse inv(T_prev) . T_cur, both from camera-to-world 3x4 poses
    (read_kitti_poses) and computed in float64."""
    a, b = _pose44(T_prev, "T_prev"), _pose44(T_cur, "T_cur")
    fwd, back = np.linalg.solve(b, a), np.linalg.solve(a, b)
    return np.stack([fwd[:3].reshape(12), back[:3].reshape(12)]).astype(np.float32)


def _read_kitti_values(path):
    """key -> list of floats for every `key: v v v` line of a KITTI calibration file (lines without numbers are skipped)."""
    mats = {}
    with open(path, encoding="utf-8", errors="replace") as f:
        for line in f:
            key, sep, rest = line.partition(":")
            if not sep:
                continue
            try:
                mats[key.strip()] = [float(v) for v in rest.split()]
            except ValueError:                                  # calib_time: 09-Jan-2012 13:57:47
                continue
    return mats


def _rodrigues(om):
    """Rotation vector -> rotation matrix, float64."""
    om = np.asarray(om, np.float64)
    th = float(np.linalg.norm(om))
    if th == 0.0:
        return np.eye(3)
    k = om / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def _rotation_vector(R):
    """Rotation matrix -> rotation vector (angle < pi), float64."""
    R = np.asarray(R, np.float64)
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = float(np.linalg.norm(axis)) / 2.0                       # sin(angle)
    th = float(np.arctan2(s, (np.trace(R) - 1.0) / 2.0))
    return np.zeros(3) if s == 0.0 else axis / (2.0 * s) * th


@dataclass(frozen=True, eq=False)
class RectifyCalib:
    """A raw stereo rig and its rectification, as a KITTI raw `calib_cam_to_cam.txt` states it: the raw and the rectified image
    size (height, width) and, per camera (0 = left, 1 = right), the raw intrinsics K [3,3], the distortion coefficients
    D = (k1, k2, p1, p2, k3) in OpenCV's order, the rectifying rotation R_rect [3,3] and the rectified projection P_rect [3,4].
    All float64 numpy."""
    raw_hw: tuple
    rect_hw: tuple
    K: tuple
    D: tuple
    R_rect: tuple
    P_rect: tuple

    def __post_init__(self):
        for name, shape in (("K", (3, 3)), ("D", (5,)), ("R_rect", (3, 3)), ("P_rect", (3, 4))):
            pair = tuple(np.array(a, np.float64) for a in getattr(self, name))
            if len(pair) != 2 or any(a.shape != shape for a in pair):
                raise ValueError(f"{name} must hold two arrays of shape {shape}")
            object.__setattr__(self, name, pair)
        object.__setattr__(self, "raw_hw", tuple(int(v) for v in self.raw_hw))
        object.__setattr__(self, "rect_hw", tuple(int(v) for v in self.rect_hw))

    def check(self):
        if len(self.raw_hw) != 2 or len(self.rect_hw) != 2 or min(self.raw_hw + self.rect_hw) < 1:
            raise ValueError(f"image sizes must be positive (height, width) pairs; got {self.raw_hw} and {self.rect_hw}")
        for c, side in enumerate(("left", "right")):
            arrays = (self.K[c], self.D[c], self.R_rect[c], self.P_rect[c])
            if not all(np.isfinite(a).all() for a in arrays):
                raise ValueError(f"{side} camera: the calibration holds values that are not finite")
            if not (self.K[c][0, 0] > 0 and self.K[c][1, 1] > 0 and self.P_rect[c][0, 0] > 0 and self.P_rect[c][1, 1] > 0):
                raise ValueError(f"{side} camera: focal lengths must be > 0")
            m = self.P_rect[c][:, :3] @ self.R_rect[c]
            if not (np.linalg.matrix_rank(m) == 3 and np.isfinite(np.linalg.cond(m)) and np.linalg.cond(m) < 1e12):
                raise ValueError(f"{side} camera: P_rect[:, :3] @ R_rect is not invertible")
        return self

    def params(self):
        """The two float32 records of lws_rectify_pair, [2,18]: {inv(P_rect[:, :3] @ R_rect) row-major, fx, fy, cx, cy, k1, k2, p1,
        p2, k3}; the inverse is taken in float64 and rounded once."""
        self.check()
        rows = []
        for c in range(2):
            inv = np.linalg.inv(self.P_rect[c][:, :3] @ self.R_rect[c])
            k = self.K[c]
            rows.append(np.concatenate([inv.reshape(-1), [k[0, 0], k[1, 1], k[0, 2], k[1, 2]], self.D[c]]))
        return np.stack(rows).astype(np.float32)

    def camera(self):
        """The Camera of the rectified left view, by the formulas of Camera.from_kitti."""
        p2, p3 = self.P_rect
        fx = p2[0, 0]
        return Camera(float(fx), float(p2[1, 1]), float(p2[0, 2]), float(p2[1, 2]), float((p2[0, 3] - p3[0, 3]) / fx)).check()

    @classmethod
    def from_kitti(cls, path, left="02", right="03"):
        """Reads S_xx, K_xx, D_xx, R_rect_xx, P_rect_xx and S_rect_xx of the two cameras from a KITTI raw `calib_cam_to_cam.txt`.
        KITTI-2015's per-frame files hold no K_ / D_ lines: they describe rectified images only."""
        mats = _read_kitti_values(path)
        fields = {name: [] for name in ("S", "K", "D", "R_rect", "P_rect", "S_rect")}
        sizes = {"S": 2, "K": 9, "D": 5, "R_rect": 9, "P_rect": 12, "S_rect": 2}
        for cam in (left, right):
            for name, n in sizes.items():
                key = f"{name}_{cam}"
                if key not in mats:
                    raise ValueError(f"{path}: missing key {key} (a raw calib_cam_to_cam.txt with S_, K_, D_, R_rect_, P_rect_ and "
                                     f"S_rect_ lines is needed)")
                if len(mats[key]) != n:
                    raise ValueError(f"{path}: {key} must hold {n} values, found {len(mats[key])}")
                fields[name].append(np.array(mats[key], np.float64))
        if fields["S"][0].tolist() != fields["S"][1].tolist() or fields["S_rect"][0].tolist() != fields["S_rect"][1].tolist():
            raise ValueError(f"{path}: the two cameras must share one raw and one rectified image size")
        (ws, hs), (wr, hr) = fields["S"][0], fields["S_rect"][0]                # KITTI writes width height
        try:
            return cls((hs, ws), (hr, wr), [k.reshape(3, 3) for k in fields["K"]], fields["D"],
                       [r.reshape(3, 3) for r in fields["R_rect"]], [p.reshape(3, 4) for p in fields["P_rect"]]).check()
        except ValueError as e:
            raise ValueError(f"{path}: {e}") from None

    @classmethod
    def from_rig(cls, K1, D1, K2, D2, R, T, size):
        """Bouguet's rectification of a horizontal rig (the algorithm of cv2.stereoRectify without its alpha / ROI logic; the
        caller crops), in float64.  A point x1 in camera 1 (left) is R @ x1 + T in camera 2 (right); size = (height, width) of both
        raw images and of the rectified frame.  R is split in half between the cameras, the baseline is turned onto +x, both
        cameras get the focal length min(K1[1,1], K2[1,1]) on both axes and the mean of the two raw principal points, and
        P_right[0,3] = -f |T|."""
        K1, K2, R = (np.array(a, np.float64).reshape(3, 3) for a in (K1, K2, R))
        T = np.array(T, np.float64).reshape(3)
        half = _rodrigues(-0.5 * _rotation_vector(R))           # turns camera 2 half way back; its transpose turns camera 1
        t = half @ T
        if not t[0] < 0:
            raise ValueError("from_rig: camera 2 must lie to the right of camera 1 (T[0] < 0 after the rotation is split)")
        uu = np.array([-1.0, 0.0, 0.0])
        ww = np.cross(t, uu)
        nw = float(np.linalg.norm(ww))
        if nw > 0.0:
            ww *= np.arccos(abs(t[0]) / np.linalg.norm(t)) / nw
        wr = _rodrigues(ww)
        r1, r2 = wr @ half.T, wr @ half
        f = min(K1[1, 1], K2[1, 1])
        cx, cy = 0.5 * (K1[0, 2] + K2[0, 2]), 0.5 * (K1[1, 2] + K2[1, 2])
        p1 = np.array([[f, 0.0, cx, 0.0], [0.0, f, cy, 0.0], [0.0, 0.0, 1.0, 0.0]])
        p2 = p1.copy()
        p2[0, 3] = -f * np.linalg.norm(T)
        return cls(size, size, (K1, K2), (D1, D2), (r1, r2), (p1, p2)).check()


def rectify_params(calibs, B):
    """One RectifyCalib or a list of B -> float32 [B,2,18], the params of lws_rectify_pair."""
    cals = [calibs] * B if isinstance(calibs, RectifyCalib) else list(calibs)
    if len(cals) != B or not all(isinstance(c, RectifyCalib) for c in cals):
        raise ValueError(f"calibs must be one RectifyCalib or a list of {B}")
    return np.stack([c.params() for c in cals])


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


VERTEX_NORMAL_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"), ("red", "u1"),
                                ("green", "u1"), ("blue", "u1"), ("alpha", "u1")])   # a vertex of a mesh file with normals
FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])   # `property list uchar int vertex_indices` of a triangle: 13 bytes


def mesh_ply_bytes(points_bytes, n, faces, vnormals=None):
    """Binary little-endian PLY of a triangle mesh (lws_surface_mesh): n vertices laid out as the device writes them
    (POINT_DTYPE), faces int32 [m,3], vnormals None or float32 [n,4] records {nx, ny, nz, 0} (the device's vnormals).  Vertex:
    x y z [nx ny nz] red green blue alpha; face: a uchar count of 3 and three int indices."""
    data = memoryview(points_bytes).cast("B")
    if len(data) < 16 * n:
        raise ValueError(f"{len(data)} bytes hold fewer than {n} points")
    pts = np.frombuffer(data, POINT_DTYPE, count=n)
    faces = np.asarray(faces)
    if faces.dtype != np.int32 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be int32 [m,3]; got {faces.dtype} {faces.shape}")
    if len(faces) and (faces.min() < 0 or faces.max() >= n):
        raise ValueError(f"a face index lies outside 0 .. {n - 1}")
    props = "property float x\nproperty float y\nproperty float z\n"
    if vnormals is None:
        verts = pts
    else:
        vn = np.asarray(vnormals)
        if vn.dtype != np.float32 or vn.shape != (n, 4):
            raise ValueError(f"vnormals must be float32 [{n},4]; got {vn.dtype} {vn.shape}")
        verts = np.empty(n, VERTEX_NORMAL_DTYPE)
        for name in POINT_DTYPE.names:
            verts[name] = pts[name]
        verts["nx"], verts["ny"], verts["nz"] = vn[:, 0], vn[:, 1], vn[:, 2]
        props += "property float nx\nproperty float ny\nproperty float nz\n"
    rec = np.empty(len(faces), FACE_DTYPE)
    rec["n"], rec["v"] = 3, faces
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex {}\n{}property uchar red\nproperty uchar green\nproperty uchar blue\n"
              "property uchar alpha\nelement face {}\nproperty list uchar int vertex_indices\nend_header\n").format(n, props, len(faces))
    return header.encode("ascii") + verts.tobytes() + rec.tobytes()


def write_mesh_ply(path, points_bytes, n, faces, vnormals=None):
    with open(path, "wb") as f:
        f.write(mesh_ply_bytes(points_bytes, n, faces, vnormals))


def read_mesh_ply(path):
    """A file write_mesh_ply wrote -> (vertices: a VERTEX_NORMAL_DTYPE array, or POINT_DTYPE without normals; faces int32 [m,3])."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    n = int(next(l for l in lines if l.startswith("element vertex")).split()[2])
    m = int(next(l for l in lines if l.startswith("element face")).split()[2])
    dtype = VERTEX_NORMAL_DTYPE if "property float nx" in lines else POINT_DTYPE
    verts = np.frombuffer(data, dtype, count=n, offset=end)
    rec = np.frombuffer(data, FACE_DTYPE, count=m, offset=end + n * dtype.itemsize)
    if not np.all(rec["n"] == 3):
        raise ValueError(f"{path}: a face is not a triangle")
    return verts, np.ascontiguousarray(rec["v"])
