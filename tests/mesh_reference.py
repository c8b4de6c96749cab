"""numpy restatement of the surface kernels (include/lwsnet_hip.h: lws_surface_normals, lws_surface_mesh), vectorised, one float32
operation per step in the order of the contract, so the GPU tests compare bit for bit.  The validity rule and the vertex records
are geometry_reference's."""
import numpy as np

import geometry_reference as G

F = np.float32
QUADRANTS = ((1, 0), (0, 3), (3, 2), (2, 1))       # (D,R), (R,U), (U,L), (L,D) over the neighbours R, D, L, U
SHIFTS = ((0, 1), (1, 0), (0, -1), (-1, 0))        # (dy, dx) of R, D, L, U


def _quiet():
    return np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def effective(disp, mask, cam, min_disp, max_depth):
    """-> (de [B,H,W]: d of a valid pixel, NaN of an invalid one; z [B,H,W])."""
    valid, z = G.valid_z(disp, mask, cam, min_disp, max_depth)
    return np.where(valid[:, 0], np.asarray(disp, F)[:, 0], F(np.nan)).astype(F), z[:, 0].astype(F)


def points(z, cam):
    """P = (X, Y, Z) of every pixel, [B,H,W] each."""
    cam = np.asarray(cam, F)
    B, H, W = z.shape
    fx, fy, cx, cy = (cam[:, k].reshape(B, 1, 1) for k in range(4))
    xs, ys = np.arange(W, dtype=F).reshape(1, 1, W), np.arange(H, dtype=F).reshape(1, H, 1)
    with _quiet():
        return ((xs - cx) * z) / fx, ((ys - cy) * z) / fy, z


def connected(dp, dq, max_jump):
    with _quiet():
        return np.abs(dp - dq) <= F(max_jump)          # False where either is NaN


def _shifted(a, dy, dx):
    """a[b, y + dy, x + dx], NaN outside the image."""
    B, H, W = a.shape
    p = np.full((B, H + 2, W + 2), np.nan, F)
    p[:, 1:-1, 1:-1] = a
    return p[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def surface_normals(disp, mask, cam, min_disp, max_depth, max_jump):
    """-> (normals float32 [B,3,H,W], present quadrants per pixel int [B,H,W])."""
    de, z = effective(disp, mask, cam, min_disp, max_depth)
    P = points(z, cam)
    with _quiet():
        con = [connected(de, _shifted(de, dy, dx), max_jump) for dy, dx in SHIFTS]
        e = [[_shifted(P[k], dy, dx) - P[k] for k in range(3)] for dy, dx in SHIFTS]
        s = [np.zeros(de.shape, F) for _ in range(3)]
        nq = np.zeros(de.shape, np.int64)
        for A, Bq in QUADRANTS:
            a, b = e[A], e[Bq]
            c = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
            present = con[A] & con[Bq]
            s = [np.where(present, s[k] + c[k], s[k]).astype(F) for k in range(3)]
            nq += present
        length = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        good = (nq > 0) & np.isfinite(length) & (length > F(0))
        n = [np.where(good, s[k] / length, F(0)).astype(F) for k in range(3)]
    return np.stack(n, axis=1), nq


def u8(v):
    """(uint8)(int)rintf((v * 0.5f + 0.5f) * 255.0f)"""
    return np.rint((np.asarray(v, F) * F(0.5) + F(0.5)) * F(255.0)).astype(np.int32).astype(np.uint8)


def normals8(normals):
    """float32 [B,3,H,W] -> the normal-map bytes uint8 [B,H,W,3] = {u8(n.x), u8(-n.y), u8(-n.z)}."""
    n = np.asarray(normals, F)
    return np.ascontiguousarray(np.stack([u8(n[:, 0]), u8(-n[:, 1]), u8(-n[:, 2])], axis=-1))


def cell_faces(de, max_jump):
    """de [B,H,W] -> (t0, t1, diag_ae), each bool [B,H-1,W-1]: the two triangles of every cell, and where its diagonal is a-e."""
    a, b, c, e = de[:, :-1, :-1], de[:, :-1, 1:], de[:, 1:, :-1], de[:, 1:, 1:]
    ab, ac, be, ce = (connected(p, q, max_jump) for p, q in ((a, b), (a, c), (b, e), (c, e)))
    bc, ae = connected(b, c, max_jump), connected(a, e, max_jump)
    diag_bc = ~np.isnan(b) & ~np.isnan(c)
    t0 = np.where(diag_bc, bc & ab & ac, ae & ac & ce)
    t1 = np.where(diag_bc, bc & be & ce, ae & ab & be)
    return t0, t1, ~diag_bc


def surface_mesh(disp, mask, rgb, cam, normals, min_disp, max_depth, max_jump):
    """-> (clouds: B POINT_DTYPE arrays, vnormals: B float32 [n,4] arrays or None, faces: B int32 [m,3] arrays, index int32
    [B,1,H,W], counts int64 [B,2])."""
    clouds, nv = G.point_cloud(disp, mask, rgb, cam, min_disp, max_depth)
    de, _ = effective(disp, mask, cam, min_disp, max_depth)
    B, H, W = de.shape
    valid = ~np.isnan(de)
    index = np.where(valid, np.cumsum(valid.reshape(B, -1), axis=1).reshape(B, H, W) - 1, -1).astype(np.int32)
    t0, t1, diag_ae = cell_faces(de, max_jump)
    ia, ib, ic, ie = index[:, :-1, :-1], index[:, :-1, 1:], index[:, 1:, :-1], index[:, 1:, 1:]
    f0 = np.stack([ia, ic, np.where(diag_ae, ie, ib)], axis=-1)                                        # (a, c, b) or (a, c, e)
    f1 = np.stack([np.where(diag_ae, ia, ib), np.where(diag_ae, ie, ic), np.where(diag_ae, ib, ie)], axis=-1)   # (b, c, e) or (a, e, b)
    both = np.stack([f0, f1], axis=3)                               # [B,H-1,W-1,2,3]: raster order of the cells, T0 before T1
    keep = np.stack([t0, t1], axis=3)
    faces = [np.ascontiguousarray(both[b][keep[b]].reshape(-1, 3).astype(np.int32)) for b in range(B)]
    vn = None
    if normals is not None:
        n = np.asarray(normals, F)
        vn = []
        for b in range(B):
            ys, xs = np.nonzero(valid[b])
            rec = np.zeros((len(ys), 4), F)
            rec[:, :3] = n[b, :, ys, xs]
            vn.append(rec)
    counts = np.stack([nv, np.array([len(f) for f in faces], np.int64)], axis=1)
    return clouds, vn, faces, index[:, None], counts
