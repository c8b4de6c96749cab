"""lws_temporal_step (include/lwsnet_temporal.h) restated in numpy float32, operation for operation, and a small renderer of a
static scene -- a road and a wall -- seen from a moving camera.  Every float step below is one float32 numpy operation in the order
the header gives, so the HIP kernels match these arrays bit for bit; the z-buffer of the hold is np.maximum.at on uint64."""
import numpy as np

F = np.float32
DEFAULTS = dict(sigma0=0.5, min_disp=1.0, sigma_min=0.05, gate=3.0, q=0.0, max_jump=1.0, hold=0, q_hold=0.05, max_var=4.0)
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float64)


def params(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return {**DEFAULTS, **kw}


def key_of(d):
    """The order-preserving uint32 of float32 values (lws_occlusion_check's key)."""
    u = np.ascontiguousarray(d, F).view(np.uint32)
    return u ^ np.where(u >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    k = np.ascontiguousarray(k, np.uint32)
    return (k ^ np.where(k >> 31 != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(F)


def _row(M, r, X, Y, Z):
    return ((M[4 * r] * X + M[4 * r + 1] * Y) + M[4 * r + 2] * Z) + M[4 * r + 3]


def _project(cam, Px, Py, Pz, H, W):
    fx, fy, cx, cy, _ = cam
    u = (fx * Px) / Pz + cx
    v = (fy * Py) / Pz + cy
    return u, v, (u >= 0) & (u <= F(W - 1)) & (v >= 0) & (v <= F(H - 1))


def _fold(op, a, b, c, d):
    m = a
    for t in (b, c, d):
        m = np.where(op(t, m), t, m)
    return m


def fuse_image(m, s, ok, cam, pose, prev, p):
    """One image: m, s float32 [H,W], ok bool [H,W], cam float32 [5], pose float32 [2,12] or None, prev (Dp, Vp, Ap) or None.
    Returns D, V, A, code."""
    H, W = m.shape
    cam = np.asarray(cam, F)
    fx, fy, cx, cy, fb = cam
    q, gate = F(p["q"]), F(p["gate"])
    with np.errstate(all="ignore"):
        valid = ok & np.isfinite(m) & (m >= F(p["min_disp"])) & (s >= 0) & np.isfinite(s)
        sg = np.fmax(s, F(p["sigma_min"]))
        r = sg * sg
        assoc = np.zeros((H, W), bool)
        pas = np.zeros((H, W), bool)
        Df = Vf = np.zeros((H, W), F)
        Af = np.zeros((H, W), np.int64)
        if prev is not None:
            Dp, Vp, Ap = prev
            P0, P1 = np.asarray(pose[0], F), np.asarray(pose[1], F)
            z = fb / m
            X = ((np.arange(W, dtype=F)[None, :] - cx) * z) / fx
            Y = ((np.arange(H, dtype=F)[:, None] - cy) * z) / fy
            Qx, Qy, Qz = (_row(P1, k, X, Y, z) for k in range(3))
            u, v, inside = _project(cam, Qx, Qy, Qz, H, W)
            assoc = (Qz > 0) & inside
            dexp = fb / Qz
            us, vs_ = np.where(assoc, u, F(0)), np.where(assoc, v, F(0))
            fu, fv = np.floor(us), np.floor(vs_)
            i0, j0 = fu.astype(np.int64), fv.astype(np.int64)
            i1, j1 = np.minimum(i0 + 1, W - 1), np.minimum(j0 + 1, H - 1)
            a, b = us - fu, vs_ - fv
            taps = ((j0, i0), (j0, i1), (j1, i0), (j1, i1))
            a00, a01, a10, a11 = (Ap[t].astype(np.int64) for t in taps)
            d00, d01, d10, d11 = (Dp[t] for t in taps)
            v00, v01, v10, v11 = (Vp[t] for t in taps)
            assoc &= (a00 > 0) & (a01 > 0) & (a10 > 0) & (a11 > 0)
            mx, mn = _fold(np.greater, d00, d01, d10, d11), _fold(np.less, d00, d01, d10, d11)
            assoc &= (mx - mn) <= F(p["max_jump"])
            dtop, dbot = d00 + a * (d01 - d00), d10 + a * (d11 - d10)
            ds = dtop + b * (dbot - dtop)
            vtop, vbot = v00 + a * (v01 - v00), v10 + a * (v11 - v10)
            vs = vtop + b * (vbot - vtop)
            ag = np.minimum(np.minimum(a00, a01), np.minimum(a10, a11))
            k = dexp / ds
            Zn = _row(P0, 2, Qx * k, Qy * k, Qz * k)
            assoc &= Zn > 0
            dpred = fb / Zn
            g = dpred / ds
            g2 = g * g
            vpred = vs * (g2 * g2) + q
            innov = m - dpred
            S = vpred + r
            pas = valid & assoc & (innov * innov <= (gate * gate) * S)
            K = vpred / S
            Df, Vf, Af = dpred + K * innov, vpred - K * vpred, np.minimum(ag + 1, 65535)
        D = np.where(valid, np.where(pas, Df, m), F(0)).astype(F)
        V = np.where(valid, np.where(pas, Vf, r), F(0)).astype(F)
        A = np.where(valid, np.where(pas, Af, 1), 0).astype(np.uint16)
        code = np.where(valid, np.where(pas, 2, np.where(assoc, 3, 1)), 0).astype(np.uint8)
    return D, V, A, code


def hold_image(D, V, A, code, cam, pose, prev, p):
    """The hold pass on the outputs of fuse_image, in place; returns the z-buffer words (0 where nothing landed on a code-0 pixel)."""
    H, W = D.shape
    cam = np.asarray(cam, F)
    fx, fy, cx, cy, fb = cam
    Dp, Vp, Ap = (t.reshape(-1) for t in prev)
    P0 = np.asarray(pose[0], F)
    src = np.flatnonzero(Ap > 0)
    Z = np.zeros(H * W, np.uint64)
    with np.errstate(all="ignore"):
        d = Dp[src]
        z = fb / d
        X = (((src % W).astype(F) - cx) * z) / fx
        Y = (((src // W).astype(F) - cy) * z) / fy
        Px, Py, Pz = (_row(P0, k, X, Y, z) for k in range(3))
        u, v, inside = _project(cam, Px, Py, Pz, H, W)
        keep = (Pz > 0) & inside
        dn = fb / Pz
        tgt = np.where(keep, np.rint(v), F(0)).astype(np.int64) * W + np.where(keep, np.rint(u), F(0)).astype(np.int64)
        keep &= code.reshape(-1)[tgt] == 0
        word = (key_of(dn).astype(np.uint64) << np.uint64(32)) | src.astype(np.uint64)
        np.maximum.at(Z, tgt[keep], word[keep])
        t = np.flatnonzero((code.reshape(-1) == 0) & (Z != 0))
        s = (Z[t] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        dn = unkey((Z[t] >> np.uint64(32)).astype(np.uint32))
        g = dn / Dp[s]
        g2 = g * g
        vh = (Vp[s] * (g2 * g2) + F(p["q"])) + F(p["q_hold"])
        take = (dn >= F(p["min_disp"])) & (vh <= F(p["max_var"]))
    t, s = t[take], s[take]
    D.reshape(-1)[t], V.reshape(-1)[t], A.reshape(-1)[t], code.reshape(-1)[t] = dn[take], vh[take], Ap[s], 4
    return Z.reshape(H, W)


def step(meas, cam, pose=None, prev=None, sigma=None, mask=None, **kw):
    """The call on [B,1,H,W] arrays: cam float32 [B,5], pose float32 [B,2,12], prev (D, V, A) or None.  Returns D, V, A, code and
    counts int64 [B,5]."""
    p = params(**kw)
    meas = np.asarray(meas, F)
    B, _, H, W = meas.shape
    D, V = np.empty(meas.shape, F), np.empty(meas.shape, F)
    A, code = np.empty(meas.shape, np.uint16), np.empty(meas.shape, np.uint8)
    counts = np.zeros((B, 5), np.int64)
    for b in range(B):
        s = np.asarray(sigma[b, 0], F) if sigma is not None else np.full((H, W), p["sigma0"], F)
        ok = mask[b, 0] == 1 if mask is not None else np.ones((H, W), bool)
        pv = None if prev is None else tuple(np.ascontiguousarray(t[b, 0]) for t in prev)
        po = None if prev is None else np.asarray(pose, F).reshape(-1, 2, 12)[b]
        out = [np.ascontiguousarray(o) for o in fuse_image(meas[b, 0], s, ok, cam[b], po, pv, p)]
        if p["hold"] and prev is not None:
            hold_image(*out, cam[b], po, pv, p)
        D[b, 0], V[b, 0], A[b, 0], code[b, 0] = out
        counts[b] = np.bincount(out[3].reshape(-1), minlength=5)
    return D, V, A, code, counts


# ---- the scene: a road 1.5 m below the camera and a wall across it, seen from a camera with a known pose ----
SCENE_CAM = (120.0, 120.0, 47.5, 20.0, 60.0)               # fx, fy, cx, cy, fx * baseline: 48 x 96
GROUND_Y, WALL_Z, WALL_X, WALL_TOP = 1.5, 12.0, (-1.5, 2.5), -1.0


def forward_pose(k, dz, yaw=0.0, dx=0.0):
    """Camera-to-world [R|t] float64 of frame k: k * dz ahead, k * dx to the right, turned k * yaw radians about the y axis."""
    c, s = np.cos(k * yaw), np.sin(k * yaw)
    return np.array([[c, 0, s, k * dx], [0, 1, 0, 0], [-s, 0, c, k * dz]], np.float64)


def render(T, H=48, W=96, cam=SCENE_CAM):
    """The true disparity float64 [H,W] of the scene seen from the camera-to-world pose T (0 where the ray meets nothing)."""
    fx, fy, cx, cy, fb = cam
    R, t = np.asarray(T, np.float64)[:, :3], np.asarray(T, np.float64)[:, 3]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], -1) @ R.T      # world direction per unit of camera depth
    with np.errstate(all="ignore"):
        sg = (GROUND_Y - t[1]) / ray[..., 1]
        sg = np.where((ray[..., 1] > 0) & (sg > 0), sg, np.inf)
        sw = (WALL_Z - t[2]) / ray[..., 2]
        px, py = t[0] + sw * ray[..., 0], t[1] + sw * ray[..., 1]
        hit = (ray[..., 2] > 0) & (sw > 0) & (px > WALL_X[0]) & (px < WALL_X[1]) & (py >= WALL_TOP) & (py <= GROUND_Y)
        sw = np.where(hit, sw, np.inf)
        depth = np.minimum(sg, sw)
        return np.where(np.isfinite(depth), fb / depth, 0.0)


def relative(T_prev, T_cur):
    """float32 [2,12]: inv(T_cur) . T_prev and its inverse, in float64 (what lwsnet_amd.geometry.relative_pose returns)."""
    a, b = (np.vstack([np.asarray(T, np.float64), [0, 0, 0, 1]]) for T in (T_prev, T_cur))
    return np.stack([np.linalg.solve(b, a)[:3].reshape(12), np.linalg.solve(a, b)[:3].reshape(12)]).astype(F)


def run_sequence(frames, cam, poses, sigmas=None, masks=None, **kw):
    """step() looped over [1,1,H,W] frames with camera-to-world poses: the list of (D, V, A, code, counts) per frame."""
    cam = np.asarray(cam, F).reshape(1, 5)
    out, prev = [], None
    for k, m in enumerate(frames):
        pose = None if k == 0 else relative(poses[k - 1], poses[k])[None]
        res = step(m, cam, pose, prev, None if sigmas is None else sigmas[k], None if masks is None else masks[k], **kw)
        prev = res[:3]
        out.append(res)
    return out
