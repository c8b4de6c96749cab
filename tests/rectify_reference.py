"""numpy restatement of lws_rectify_pair (include/lwsnet_hip.h): float32 arrays, one numpy operation per step of the contract in
the order written, np.rint (half to even) and integer arithmetic for the blend, so the device's outputs can be compared bit for
bit -- and the same map in float64 at fractional positions (rectify_map64), which is what the float32 map is measured against.

IEEE 754 fixes neither the sign nor the payload of a NaN an operation produces (0 * inf is -nan on x86 and +nan on the device):
canonical_nans makes the maps comparable on raw bits."""
import numpy as np

F = np.float32
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _map32(rec, H, W, x0, y0):
    """(sx, sy) float32 [H,W] of one record [18] over the window."""
    iR, (fx, fy, cx, cy, k1, k2, p1, p2, k3) = rec[:9], rec[9:]
    two, one = F(2.0), F(1.0)
    xr = np.broadcast_to((np.arange(W, dtype=np.int32) + np.int32(x0)).astype(F)[None, :], (H, W))
    yr = np.broadcast_to((np.arange(H, dtype=np.int32) + np.int32(y0)).astype(F)[:, None], (H, W))
    with np.errstate(all="ignore"):
        X = iR[0] * xr + iR[1] * yr + iR[2]
        Y = iR[3] * xr + iR[4] * yr + iR[5]
        Wc = iR[6] * xr + iR[7] * yr + iR[8]
        x = X / Wc
        y = Y / Wc
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        t = (two * x) * y
        kr = one + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = (x * kr + p1 * t) + p2 * (r2 + two * x2)
        yd = (y * kr + p1 * (r2 + two * y2)) + p2 * t
        sx = fx * xd + cx
        sy = fy * yd + cy
    assert sx.dtype == F and sy.dtype == F
    return sx, sy


def rectify_reference(raw, params, out_hw, origin=(0, 0), border=0, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """raw: (left, right) uint8 [B,Hs,Ws,3]; params float32 [B,2,18]; out_hw = (H, W); origin = (y0, x0).  Returns a dict of
    (left, right) pairs: rect uint8 [B,H,W,3], input float32 [B,3,H,W], valid uint8 [B,1,H,W], map float32 [B,H,W,2]."""
    (H, W), (y0, x0) = out_hw, origin
    params = np.ascontiguousarray(params, dtype=F)
    mean, std = np.asarray(mean, F), np.asarray(std, F)
    out = {"rect": [], "input": [], "valid": [], "map": []}
    for c in range(2):
        src = np.ascontiguousarray(raw[c])
        B, Hs, Ws, _ = src.shape
        rect = np.empty((B, H, W, 3), np.uint8)
        valid = np.empty((B, 1, H, W), np.uint8)
        maps = np.empty((B, H, W, 2), F)
        for b in range(B):
            sx, sy = _map32(params[b, c], H, W, x0, y0)
            maps[b, :, :, 0], maps[b, :, :, 1] = sx, sy
            with np.errstate(invalid="ignore"):
                ok = (np.abs(sx) <= F(32768.0)) & (np.abs(sy) <= F(32768.0))
                qx = np.rint(np.where(ok, sx, F(0.0)) * F(32.0)).astype(np.int32)
                qy = np.rint(np.where(ok, sy, F(0.0)) * F(32.0)).astype(np.int32)
            X0, ax, Y0, ay = qx >> 5, qx & 31, qy >> 5, qy & 31

            def tap(X, Y):
                inside = ok & (X >= 0) & (X < Ws) & (Y >= 0) & (Y < Hs)
                v = src[b][np.clip(Y, 0, Hs - 1), np.clip(X, 0, Ws - 1)].astype(np.int32)
                return np.where(inside[..., None], v, np.int32(border))

            w = [((32 - ax) * (32 - ay))[..., None], (ax * (32 - ay))[..., None], ((32 - ax) * ay)[..., None], (ax * ay)[..., None]]
            acc = w[0] * tap(X0, Y0) + w[1] * tap(X0 + 1, Y0) + w[2] * tap(X0, Y0 + 1) + w[3] * tap(X0 + 1, Y0 + 1)
            px = (acc + 512) >> 10
            rect[b] = np.where(ok[..., None], px, np.int32(border)).astype(np.uint8)
            valid[b, 0] = ok & (X0 >= 0) & (X0 <= Ws - 2) & (Y0 >= 0) & (Y0 <= Hs - 2)
        inp = ((rect.astype(F) / F(255.0)) - mean) / std
        assert inp.dtype == F
        out["rect"].append(rect)
        out["input"].append(np.ascontiguousarray(inp.transpose(0, 3, 1, 2)))
        out["valid"].append(valid)
        out["map"].append(maps)
    return {k: tuple(v) for k, v in out.items()}


def canonical_nans(a):
    """A copy of a float32 array with every NaN replaced by the one quiet NaN 0x7FC00000."""
    a = np.array(a, F)
    a.view(np.uint32)[np.isnan(a)] = 0x7FC00000
    return a


def distort64(x, y, D):
    """The forward radial-tangential model in float64: normalised (x, y) -> distorted normalised (xd, yd)."""
    k1, k2, p1, p2, k3 = (float(v) for v in D)
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    t = 2.0 * x * y
    kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    return x * kr + p1 * t + p2 * (r2 + 2.0 * x2), y * kr + p1 * (r2 + 2.0 * y2) + p2 * t


def rectify_map64(calib, cam, xr, yr, params=None):
    """The raw position (sx, sy) the rectified position (xr, yr) of camera `cam` samples, in float64; xr, yr may be fractional
    arrays.  params: None = the calibration's own float64 matrices; a float32 [2,18] array = those rounded parameters, the
    arithmetic still in float64 (what the float32 map of the kernel is measured against)."""
    xr, yr = np.asarray(xr, np.float64), np.asarray(yr, np.float64)
    if params is None:
        iR = np.linalg.inv(calib.P_rect[cam][:, :3] @ calib.R_rect[cam]).reshape(-1)
        k = calib.K[cam]
        fx, fy, cx, cy, D = k[0, 0], k[1, 1], k[0, 2], k[1, 2], calib.D[cam]
    else:
        rec = np.asarray(params, np.float64)[cam]
        iR, (fx, fy, cx, cy), D = rec[:9], rec[9:13], rec[13:]
    X = iR[0] * xr + iR[1] * yr + iR[2]
    Y = iR[3] * xr + iR[4] * yr + iR[5]
    Wc = iR[6] * xr + iR[7] * yr + iR[8]
    xd, yd = distort64(X / Wc, Y / Wc, D)
    return fx * xd + cx, fy * yd + cy


def kitti_like_calib(hw=(375, 1242)):
    """A made-up rig with KITTI-like numbers (f ~ 960 px, strong barrel distortion, a rotation of a few mrad between the cameras,
    a 0.54 m baseline), rectified by RectifyCalib.from_rig.  Returns (calib, (K1, D1, K2, D2, R, T))."""
    from lwsnet_amd.geometry import RectifyCalib, _rodrigues
    K1 = np.array([[961.3, 0.0, 612.4], [0.0, 958.7, 181.9], [0.0, 0.0, 1.0]])
    K2 = np.array([[958.2, 0.0, 606.8], [0.0, 955.1, 176.3], [0.0, 0.0, 1.0]])
    D1 = np.array([-0.3692, 0.1968, 1.354e-3, 5.677e-4, -0.0677])
    D2 = np.array([-0.3640, 0.1790, 1.148e-3, -6.3e-4, -0.0513])
    R = _rodrigues([4.1e-3, -6.3e-3, 2.2e-3])
    T = np.array([-0.5370, 0.0032, -0.0051])
    return RectifyCalib.from_rig(K1, D1, K2, D2, R, T, hw), (K1, D1, K2, D2, R, T)


def write_kitti(path, calib, skip=()):
    """Writes a KITTI raw calib_cam_to_cam.txt for cameras 02 / 03 (a pathlib path; the keys in `skip` are left out)."""
    lines = ["calib_time: 09-Jan-2012 13:57:47", "corner_dist: 9.950000e-02"]
    for cam, tag in enumerate(("02", "03")):
        vals = {"S": [calib.raw_hw[1], calib.raw_hw[0]], "K": calib.K[cam].reshape(-1), "D": calib.D[cam],
                "R_rect": calib.R_rect[cam].reshape(-1), "P_rect": calib.P_rect[cam].reshape(-1),
                "S_rect": [calib.rect_hw[1], calib.rect_hw[0]]}
        for name, v in vals.items():
            if f"{name}_{tag}" not in skip:
                lines.append(f"{name}_{tag}: " + " ".join(repr(float(x)) for x in v))
    path.write_text("\n".join(lines) + "\n")
    return str(path)
