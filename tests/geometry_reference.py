"""numpy restatement of the geometry kernels (include/lwsnet_hip.h: lws_depth_maps, lws_point_cloud), one float32 operation per
step in the order of the contract, so the GPU tests compare bit for bit."""
import numpy as np

from lwsnet_amd.geometry import POINT_DTYPE

F = np.float32


def _ok_mask(disp, mask):
    return np.ones(disp.shape, bool) if mask is None else np.asarray(mask) == 1


def u16x256(v):
    """(uint16)fminf(fmaxf(rintf(v * 256), 0), 65535); rint: half to even."""
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(np.asarray(v, F) * F(256.0))
    return np.minimum(np.maximum(np.nan_to_num(r, nan=0.0), F(0)), F(65535)).astype(np.uint16)


def valid_z(disp, mask, cam, min_disp, max_depth):
    """disp [B,1,H,W], cam [B,5] -> (valid, z), each [B,1,H,W]."""
    d = np.asarray(disp, F)
    fb = np.asarray(cam, F)[:, 4].reshape(-1, 1, 1, 1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = fb / d
        valid = _ok_mask(d, mask) & np.isfinite(d) & (d >= F(min_disp)) & (z <= F(max_depth))
    return valid, z


def depth_maps(disp, mask, cam, min_disp, max_depth):
    """-> (depth float32, depth16 uint16, disp16 uint16), each [B,1,H,W]; cam may be None (depth, depth16 are then None)."""
    d = np.asarray(disp, F)
    with np.errstate(invalid="ignore"):
        ok16 = _ok_mask(d, mask) & np.isfinite(d) & (d > F(0))
    disp16 = np.where(ok16, u16x256(np.where(ok16, d, F(0))), np.uint16(0)).astype(np.uint16)
    if cam is None:
        return None, None, disp16
    valid, z = valid_z(d, mask, cam, min_disp, max_depth)
    depth = np.where(valid, z, F(0)).astype(F)
    depth16 = np.where(valid, u16x256(np.where(valid, z, F(0))), np.uint16(0)).astype(np.uint16)
    return depth, depth16, disp16


def point_cloud(disp, mask, rgb, cam, min_disp, max_depth):
    """-> (a list of B POINT_DTYPE arrays, the valid pixels of each image in raster order; counts int64 [B])."""
    d = np.asarray(disp, F)
    cam = np.asarray(cam, F)
    B, _, H, W = d.shape
    valid, z = valid_z(d, mask, cam, min_disp, max_depth)
    clouds = []
    for b in range(B):
        fx, fy, cx, cy, _ = cam[b]
        ys, xs = np.nonzero(valid[b, 0])
        zz = z[b, 0, ys, xs]
        rec = np.empty(len(ys), POINT_DTYPE)
        rec["x"] = ((xs.astype(F) - cx) * zz) / fx
        rec["y"] = ((ys.astype(F) - cy) * zz) / fy
        rec["z"] = zz
        if rgb is None:
            rec["red"] = rec["green"] = rec["blue"] = 255
        else:
            px = np.asarray(rgb, np.uint8)[b, ys, xs]
            rec["red"], rec["green"], rec["blue"] = px[:, 0], px[:, 1], px[:, 2]
        rec["alpha"] = 255
        clouds.append(rec)
    return clouds, np.array([len(c) for c in clouds], np.int64)
