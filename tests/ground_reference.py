"""numpy restatement of the ground kernels (include/lwsnet_hip.h: lws_vdisparity, lws_ground_fit, lws_ground_classify, lws_bev_grid):
float32 steps as float32 arrays, one numpy operation per step of the contract in its order; the plane fit's float64 steps as Python
floats; its sums as Python integers.  Written for clarity, not speed: keep the Hough candidate ranges small.  Also the synthetic
road scenes the CPU and GPU tests share."""
import math

import numpy as np

F = np.float32
OK, NO_GROUND, DEGENERATE = 0, 1, 2
INVALID, GROUND, OBSTACLE, OVERHEAD, BELOW, NO_PLANE = 0, 1, 2, 3, 4, 5


def counted(d, mask, min_disp, sub, nbins):
    """The pixels lws_vdisparity counts and their bins: (bool [B,1,H,W], int64 [B,1,H,W], 0 where not counted)."""
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        t = np.floor(d * F(sub))
        ok = np.ones(d.shape, bool) if mask is None else (np.asarray(mask) == 1)
        c = ok & np.isfinite(d) & (d >= F(min_disp)) & (t < F(nbins))
    return c, np.where(c, t, F(0)).astype(np.int64)


def vdisparity(d, mask, min_disp, sub, nbins):
    """hist uint32 [B,H,nbins]."""
    c, q = counted(d, mask, min_disp, sub, nbins)
    B, _, H, _ = c.shape
    hist = np.zeros((B, H, nbins), np.uint32)
    for b in range(B):
        for y in range(H):
            hist[b, y] = np.bincount(q[b, 0, y][c[b, 0, y]], minlength=nbins)
    return hist


def hough_scores(hist, yh_lo, yh_hi, qb_lo, qb_hi, tol_bins):
    """The scores of one image's candidates: int64 [yh_hi - yh_lo + 1, qb_hi - qb_lo + 1]."""
    H, nbins = hist.shape
    pre = np.zeros((H, nbins + 1), np.int64)
    pre[:, 1:] = np.cumsum(hist.astype(np.int64), axis=1)
    qb = np.arange(qb_lo, qb_hi + 1, dtype=np.int64)
    scores = np.zeros((yh_hi - yh_lo + 1, len(qb)), np.int64)
    for i, yh in enumerate(range(yh_lo, yh_hi + 1)):
        den = H - 1 - yh
        y = np.arange(max(yh + 1, 0), H, dtype=np.int64)
        k = (2 * qb[None, :] * (y[:, None] - yh) + den) // (2 * den)
        lo, hi = np.maximum(k - tol_bins, 0), np.minimum(k + tol_bins, nbins - 1)
        rows = np.broadcast_to(y[:, None], k.shape)
        scores[i] = (pre[rows, hi + 1] - pre[rows, lo]).sum(axis=0)
    return scores


def hough(hist, yh_lo, yh_hi, qb_lo, qb_hi, tol_bins):
    """(yh, qB, score) of the winner: the highest score, then the smaller qB, then the smaller yh."""
    s = hough_scores(hist, yh_lo, yh_hi, qb_lo, qb_hi, tol_bins)
    best = int(s.max())
    j = int(np.flatnonzero((s == best).any(axis=0))[0])
    i = int(np.flatnonzero(s[:, j] == best)[0])
    return yh_lo + i, qb_lo + j, best


def u16(v):
    """The float32 value of KITTI's 16-bit PNG word of v (lws_depth_maps)."""
    with np.errstate(all="ignore"):
        return np.fmin(np.fmax(np.rint(np.asarray(v, F) * F(256.0)), F(0.0)), F(65535.0))


def fit_sums(Q, c, plane, tol):
    """One pass over one image: the nine integer sums over the inliers of `plane` = (a, b, c) in float64 within tol pixels."""
    a, b, c0 = plane
    H, W = Q.shape
    y, x = np.mgrid[0:H, 0:W]
    xf, yf = x.astype(np.float64), y.astype(np.float64)
    with np.errstate(all="ignore"):
        inl = c & (np.abs(Q.astype(np.float64) - ((a * xf + b * yf) + c0)) <= float(F(tol)) * 256.0)
    xi, yi, qi = (v[inl].astype(np.int64) for v in (x, y, Q))
    return tuple(int(v) for v in (inl.sum(), xi.sum(), yi.sum(), qi.sum(), (xi * xi).sum(), (xi * yi).sum(), (yi * yi).sum(),
                                  (xi * qi).sum(), (yi * qi).sum()))


def solve(sums):
    """The float64 least-squares plane of the sums, each operation on its own; None: degenerate."""
    n, sx, sy, sq, sxx, sxy, syy, sxq, syq = sums
    if n < 3:
        return None
    fn = float(n)
    mx, my, mq = float(sx) / fn, float(sy) / fn, float(sq) / fn
    cxx = float(sxx) / fn - mx * mx
    cxy = float(sxy) / fn - mx * my
    cyy = float(syy) / fn - my * my
    cxq = float(sxq) / fn - mx * mq
    cyq = float(syq) / fn - my * mq
    det = cxx * cyy - cxy * cxy
    if not det > 0.0:
        return None
    a = (cxq * cyy - cyq * cxy) / det
    b = (cyq * cxx - cxq * cxy) / det
    c = (mq - a * mx) - b * my
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return None
    return a, b, c


def hough_plane(H, sub, yh, qb):
    """The winner's line as the plane of pass 0, float64, in 1/256 px."""
    den = H - 1 - yh
    b = (256.0 * float(qb)) / (float(sub) * float(den))
    return 0.0, b, (-b) * float(yh) + 128.0 / float(sub)


def ground_fit(d, mask, hist, min_disp, sub, yh_lo, yh_hi, qb_lo, qb_hi, tol_bins, min_score, tol0, tol, iters, planes64=None):
    """-> (plane float32 [B,4], info int32 [B,8]).  planes64: a list that receives each image's float64 plane (or None)."""
    d = np.asarray(d, F)
    B, _, H, W = d.shape
    nbins = hist.shape[2]
    cnt, _ = counted(d, mask, min_disp, sub, nbins)
    plane = np.full((B, 4), np.nan, F)
    info = np.zeros((B, 8), np.int32)
    for b in range(B):
        yh, qb, score = hough(hist[b], yh_lo, yh_hi, qb_lo, qb_hi, tol_bins)
        info[b, 1:4] = yh, qb, score
        cur = None
        if score < min_score:
            info[b, 0] = NO_GROUND
        else:
            cur = hough_plane(H, sub, yh, qb)
            Q = u16(d[b, 0])
            for p in range(iters + 1):
                sums = fit_sums(Q, cnt[b, 0], cur, tol0 if p == 0 else tol)
                info[b, 4] = sums[0]
                cur = solve(sums)
                if cur is None:
                    info[b, 0] = DEGENERATE
                    break
        if cur is not None:
            plane[b] = [F(cur[0] / 256.0), F(cur[1] / 256.0), F(cur[2] / 256.0), F(0.0)]
        if planes64 is not None:
            planes64.append(None if cur is None else tuple(v / 256.0 for v in cur))
    return plane, info


def valid_z(d, mask, cam, min_disp, max_depth):
    """(valid bool [B,1,H,W], z float32) of lws_depth_maps; cam float32 [B,5]."""
    d = np.asarray(d, F)
    fb = np.asarray(cam, F)[:, 4].reshape(-1, 1, 1, 1)
    with np.errstate(all="ignore"):
        z = fb / d
        ok = np.ones(d.shape, bool) if mask is None else (np.asarray(mask) == 1)
        return ok & np.isfinite(d) & (d >= F(min_disp)) & (z <= F(max_depth)), z


def ground_classify(d, mask, cam, plane, min_disp, max_depth, ground_tol, max_height):
    """-> (height float32 [B,1,H,W], codes uint8 [B,1,H,W], counts int64 [B,6])."""
    d, cam, plane = np.asarray(d, F), np.asarray(cam, F), np.asarray(plane, F)
    B, _, H, W = d.shape
    valid, z = valid_z(d, mask, cam, min_disp, max_depth)
    height, codes = np.zeros(d.shape, F), np.zeros(d.shape, np.uint8)
    xf, yf = np.arange(W, dtype=F)[None, :], np.arange(H, dtype=F)[:, None]
    with np.errstate(all="ignore"):
        for i in range(B):
            a, b, c = plane[i, 0], plane[i, 1], plane[i, 2]
            fx, fy, cx, cy = cam[i, 0], cam[i, 1], cam[i, 2], cam[i, 3]
            dp = (a * xf + b * yf) + c
            nx, ny, nz = a * fx, b * fy, (a * cx + b * cy) + c
            ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
            h = ((d[i, 0] - dp) * z[i, 0]) / ln
            fin = np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(h)
            code = np.where(np.abs(h) <= F(ground_tol), GROUND, np.where(h < 0, BELOW, np.where(h <= F(max_height), OBSTACLE, OVERHEAD)))
            code = np.where(valid[i, 0], np.where(fin, code, NO_PLANE), INVALID).astype(np.uint8)
            codes[i, 0] = code
            height[i, 0] = np.where((code == INVALID) | (code == NO_PLANE), F(0.0), h)
    counts = np.stack([np.bincount(codes[i].reshape(-1), minlength=6) for i in range(B)]).astype(np.int64)
    return height, codes, counts


def bev_grid(d, cam, codes, height, min_disp, max_depth, code_bits, x_min, cell, Gx, Gz):
    """-> (count uint32 [B,Gz,Gx], hmax float32 [B,Gz,Gx]); the maximum is the unsigned maximum of the heights' bit patterns."""
    d, cam = np.asarray(d, F), np.asarray(cam, F)
    B, _, H, W = d.shape
    valid, z = valid_z(d, None, cam, min_disp, max_depth)
    count, hbits = np.zeros((B, Gz, Gx), np.uint32), np.zeros((B, Gz, Gx), np.uint32)
    xf = np.arange(W, dtype=F)[None, :]
    with np.errstate(all="ignore"):
        for i in range(B):
            code = np.asarray(codes)[i, 0].astype(np.int64)
            take = valid[i, 0] & (code < 6) & (((code_bits >> np.minimum(code, 6)) & 1) == 1)
            X = ((xf - cam[i, 2]) * z[i, 0]) / cam[i, 0]
            u = (X - F(x_min)) / F(cell)
            v = z[i, 0] / F(cell)
            take &= (u >= F(0.0)) & (u < F(Gx)) & (v >= F(0.0)) & (v < F(Gz))
            ix, iz = np.floor(u[take]).astype(np.int64), np.floor(v[take]).astype(np.int64)
            np.add.at(count[i], (iz, ix), 1)
            np.maximum.at(hbits[i], (iz, ix), np.ascontiguousarray(np.asarray(height, F)[i, 0]).view(np.uint32)[take])
    return count, hbits.view(F)


# ---- synthetic road scenes ----
def plane_normal(pitch_deg, roll_deg):
    """The unit normal of the road in camera coordinates (x right, y down, z forward): pitch > 0 looks down, roll > 0 leans to +x."""
    t, r = math.radians(pitch_deg), math.radians(roll_deg)
    return np.array([math.sin(r) * math.cos(t), math.cos(r) * math.cos(t), math.sin(t)])


def planted_plane(cam, height, pitch_deg, roll_deg):
    """The road's disparity plane d = a x + b y + c (float64) seen by cam = (fx, fy, cx, cy, fb)."""
    fx, fy, cx, cy, fb = (float(v) for v in cam)
    n = plane_normal(pitch_deg, roll_deg)
    a, b = fb * n[0] / (fx * height), fb * n[1] / (fy * height)
    return a, b, fb * n[2] / height - a * cx - b * cy


BOXES = ((-2.6, -1.4, 7.0, 1.6), (0.3, 1.3, 5.0, 1.2), (1.8, 3.4, 11.0, 2.4))     # X0, X1 (m), depth Z (m), height (m)


def road_scene(H=96, W=160, height=1.65, pitch_deg=1.0, roll_deg=0.0, cam=(120.0, 120.0, 79.5, 47.5, 64.8), boxes=BOXES):
    """A road seen from `height` metres with fronto-parallel boxes standing on it; the sky has disparity 0.  Returns
    (disp float32 [1,1,H,W], cam float32 [1,5], planted (a, b, c), road bool [H,W], box bool [H,W], box height above the road [H,W])."""
    fx, fy, cx, cy, fb = (float(v) for v in cam)
    n = plane_normal(pitch_deg, roll_deg)
    a, b, c = planted_plane(cam, height, pitch_deg, roll_deg)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    d = a * x + b * y + c                                   # the road where positive
    road = d > 0
    d = np.where(road, d, 0.0)
    rx, ry = (x - cx) / fx, (y - cy) / fy
    box, above = np.zeros((H, W), bool), np.zeros((H, W))
    for x0, x1, zb, hb in sorted(boxes, key=lambda v: -v[2]):       # far to near
        hgt = height - zb * (n[0] * rx + n[1] * ry + n[2])  # of the ray's point at depth zb above the road
        hit = (rx * zb >= x0) & (rx * zb <= x1) & (hgt >= 0) & (hgt <= hb) & (fb / zb > d)
        d, box, road = np.where(hit, fb / zb, d), box | hit, road & ~hit
        above = np.where(hit, hgt, above)
    return d.astype(F)[None, None], np.array([cam], F), (a, b, c), road, box, above
