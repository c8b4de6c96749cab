"""lws_ego_normal and lws_egomotion (include/lwsnet_egomotion.h) restated in numpy, and a textured, anti-aliased rendering of the
road-and-wall scene of tests/temporal_reference.py.  Every per-pixel step is one float32 numpy operation in the order the header
gives, so the kernels match `terms`, `resid` and the pyramids bit for bit; the 29 sums and the update are float64, the sums with
numpy's own order of additions, so they agree with the kernels to summation rounding (sum_bound), not to the bit.  With
dtype=np.float64 the same per-pixel steps run in double: the function whose finite differences the Jacobian is held to."""
import numpy as np

import temporal_reference as T

F = np.float32
SERIES_BELOW = 0.05                                         # radians: below it exp_se3 uses the series
DEFAULTS = dict(levels=3, iters=8, min_disp=0.5, max_jump=1.0, huber=10.0, damping=0.0, min_pixels=64)
TRI = [(i, j) for i in range(6) for j in range(i, 6)]       # the order of the 21 upper-triangle entries
IDENTITY12 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)
BIT_FEW, BIT_SINGULAR, BIT_NONFINITE, BIT_FINAL_FEW, BIT_SMALL = 1, 2, 4, 8, 16
MIN_STEP2 = 2.0 ** -46                                      # |delta|^2 below it: the step is not taken (float32 resolution of a pose)


def params(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return {**DEFAULTS, **kw}


# ---- pyramids ----
def grey_of(rgb):
    """uint8 [..., 3] -> float32 grey: (77 R + 150 G + 29 B) / 256, exact."""
    r = rgb.astype(np.int64)
    return ((77 * r[..., 0] + 150 * r[..., 1] + 29 * r[..., 2]).astype(F) / F(256.0)).astype(F)


def _taps(a):
    H2, W2 = a.shape[0] // 2, a.shape[1] // 2
    a = a[:2 * H2, :2 * W2]
    return a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2]


def down_grey(g):
    a, b, c, d = _taps(g)
    with np.errstate(all="ignore"):
        return (((a + b) + (c + d)) * F(0.25)).astype(F)


def down_disp(d, ok, min_disp, max_jump):
    """d float32 [H,W] in full-resolution pixels, ok bool [H,W] -> [H/2,W/2]: the mean of a 2 x 2 block whose four taps are usable
    and lie within max_jump of each other, else 0."""
    t = _taps(d)
    with np.errstate(all="ignore"):
        usable = np.ones(t[0].shape, bool)
        for x, o in zip(t, _taps(ok)):
            usable &= o & np.isfinite(x) & (x >= F(min_disp))
        mx, mn = T._fold(np.greater, *t), T._fold(np.less, *t)
        usable &= (mx - mn) <= F(max_jump)
        mean = ((t[0] + t[1]) + (t[2] + t[3])) * F(0.25)
        return np.where(usable, mean, F(0)).astype(F)


def level_cam(cam, level, dt=F):
    fx, fy, cx, cy, fb = (dt(v) for v in np.asarray(cam, F))
    s = dt(2.0 ** -level)
    return fx * s, fy * s, (cx + dt(0.5)) * s - dt(0.5), (cy + dt(0.5)) * s - dt(0.5), fb


# ---- one linearisation ----
def normal_image(gref, disp, ok, gcur, cam, M, level, min_disp, huber, dt=F):
    """One image at one level: gref, disp, gcur [H,W], ok bool [H,W], cam the full-resolution row, M float64 [12].
    Returns (terms [H,W,8] of dt, use bool [H,W], reasons: a dict of the exclusion masks)."""
    H, W = gref.shape
    gref, disp, gcur = (np.asarray(a, dt) for a in (gref, disp, gcur))
    fx, fy, cx, cy, fb = level_cam(cam, level, dt)
    Mf = np.asarray(M, np.float64).astype(dt)
    hub = dt(huber)
    with np.errstate(all="ignore"):
        use0 = ok & np.isfinite(disp) & (disp >= dt(min_disp))
        z = fb / disp
        X = ((np.arange(W, dtype=dt)[None, :] - cx) * z) / fx
        Y = ((np.arange(H, dtype=dt)[:, None] - cy) * z) / fy
        Qx, Qy, Qz = (T._row(Mf, k, X, Y, z) for k in range(3))
        front = Qz > 0
        u = (fx * Qx) / Qz + cx
        v = (fy * Qy) / Qz + cy
        big = W >= 4 and H >= 4
        inside = (u >= 1) & (u <= dt(W - 2)) & (v >= 1) & (v <= dt(H - 2)) & big
        use = use0 & front & inside
        us, vs = np.where(use, u, dt(1)), np.where(use, v, dt(1))
        if not big:
            terms = np.zeros((H, W, 8), dt)
            return terms, use, dict(invalid=~use0, behind=use0 & ~front, outside=use0 & front & ~inside, nonfinite=np.zeros((H, W), bool))
        i0 = np.minimum(np.floor(us).astype(np.int64), W - 3)
        j0 = np.minimum(np.floor(vs).astype(np.int64), H - 3)
        a, b = us - i0.astype(dt), vs - j0.astype(dt)

        def blend(t):
            t00, t01, t10, t11 = t(j0, i0), t(j0, i0 + 1), t(j0 + 1, i0), t(j0 + 1, i0 + 1)
            top, bot = t00 + a * (t01 - t00), t10 + a * (t11 - t10)
            return top + b * (bot - top)

        Ic = blend(lambda j, i: gcur[j, i])
        gx = blend(lambda j, i: dt(0.5) * (gcur[j, i + 1] - gcur[j, i - 1]))
        gy = blend(lambda j, i: dt(0.5) * (gcur[j + 1, i] - gcur[j - 1, i]))
        r = Ic - gref
        ar = np.abs(r)
        w = np.where(ar <= hub, dt(1), hub / ar)
        ju, jv = (gx * fx) / Qz, (gy * fy) / Qz
        jz = -((ju * Qx + jv * Qy) / Qz)
        J = [ju, jv, jz, jz * Qy - jv * Qz, ju * Qz - jz * Qx, jv * Qx - ju * Qy]
        finite = np.isfinite(r) & np.isfinite(gx) & np.isfinite(gy)
        for j in J:
            finite &= np.isfinite(j)
        nonfinite = use & ~finite
        use = use & finite
        terms = np.stack([r, w] + J, -1)
        terms = np.where(use[..., None], terms, dt(0)).astype(dt)
    return terms, use, dict(invalid=~use0, behind=use0 & ~front, outside=use0 & front & ~inside, nonfinite=nonfinite)


def sums_of(terms, use):
    """(sums float64 [29], mag float64 [29]: the sum of the absolute values of the same products) of one image's terms."""
    t = terms[use].astype(np.float64)
    r, w, J = t[:, 0], t[:, 1], t[:, 2:]
    wJ = w[:, None] * J
    cols = [wJ[:, i] * J[:, j] for i, j in TRI] + [wJ[:, i] * r for i in range(6)] + [(w * r) * r, np.ones(len(t))]
    cols = np.stack(cols, -1) if len(t) else np.zeros((0, 29))
    return cols.sum(0), np.abs(cols).sum(0)


def sum_bound(n, mag):
    """What two orders of adding n float64 products may differ by: each order is within (n - 1) 2^-53 of the exact sum, to first
    order; (n + 64) 2^-53 sum|term| covers both orders and the second-order terms with room to spare."""
    return (n + 64) * 2.0 ** -53 * mag


def normal(grey_ref, disp_ref, mask, grey_cur, cam, M, level, min_disp, huber):
    """The call on [B,1,H,W] (or [B,H,W]) arrays: returns sums [B,29], terms [B,H,W,8], mag [B,29]."""
    B = len(grey_ref)
    g0, d0, g1 = (np.asarray(a, F).reshape(B, *np.shape(a)[-2:]) for a in (grey_ref, disp_ref, grey_cur))
    H, W = g0.shape[1:]
    sums, mags, terms = np.zeros((B, 29)), np.zeros((B, 29)), np.zeros((B, H, W, 8), F)
    for b in range(B):
        ok = np.asarray(mask).reshape(B, H, W)[b] == 1 if mask is not None else np.ones((H, W), bool)
        terms[b], use, _ = normal_image(g0[b], d0[b], ok, g1[b], cam[b], np.asarray(M, np.float64).reshape(B, 12)[b], level, min_disp, huber)
        sums[b], mags[b] = sums_of(terms[b], use)
    return sums, terms, mags


# ---- the update ----
def unpack(sums):
    Hm, b = np.zeros((6, 6)), np.asarray(sums[21:27], np.float64).copy()
    for k, (i, j) in enumerate(TRI):
        Hm[i, j] = Hm[j, i] = sums[k]
    return Hm, b


def exp_coefficients(theta, series=None):
    """A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3; below SERIES_BELOW (or where `series` says) their series to t^6."""
    t2 = theta * theta
    if theta < SERIES_BELOW if series is None else series:
        A = 1.0 - t2 * (1.0 / 6.0 - t2 * (1.0 / 120.0 - t2 * (1.0 / 5040.0)))
        Bc = 0.5 - t2 * (1.0 / 24.0 - t2 * (1.0 / 720.0 - t2 * (1.0 / 40320.0)))
        C = 1.0 / 6.0 - t2 * (1.0 / 120.0 - t2 * (1.0 / 5040.0 - t2 * (1.0 / 362880.0)))
    else:
        A, Bc, C = np.sin(theta) / theta, (1.0 - np.cos(theta)) / t2, (theta - np.sin(theta)) / (t2 * theta)
    return A, Bc, C


def exp_se3(delta, series=None):
    """float64 [3,4] = exp of the twist delta = (translation part, rotation vector): R = I + A K + B K^2, t = (I + B K + C K^2) v."""
    v, om = np.asarray(delta[:3], np.float64), np.asarray(delta[3:], np.float64)
    theta = np.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])
    A, Bc, C = exp_coefficients(theta, series)
    K = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    K2 = K @ K
    R, V = np.eye(3) + A * K + Bc * K2, np.eye(3) + Bc * K + C * K2
    return np.hstack([R, (V @ v)[:, None]])


def compose(E, M):
    """E . M for two [3,4] rigid motions (E applied after M), as float64 [12]."""
    E, M = np.asarray(E, np.float64).reshape(3, 4), np.asarray(M, np.float64).reshape(3, 4)
    return np.hstack([E[:, :3] @ M[:, :3], (E[:, :3] @ M[:, 3] + E[:, 3])[:, None]]).reshape(12)


def cholesky_solve(A, rhs):
    """(x, ok): A x = rhs by Cholesky A = L L^T; ok is False at the first pivot that is not > 0."""
    L = np.zeros((6, 6))
    for j in range(6):
        p = A[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not p > 0:
            return np.zeros(6), False
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (rhs[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (y[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x, True


def update(sums, M, damping, min_pixels):
    """One Gauss-Newton step from the 29 sums: (the new M float64 [12], delta [6], the step's status)."""
    M = np.asarray(M, np.float64).reshape(12)
    if sums[28] < min_pixels:
        return M.copy(), np.zeros(6), BIT_FEW
    if not np.isfinite(sums).all():
        return M.copy(), np.zeros(6), BIT_NONFINITE
    Hm, b = unpack(sums)
    A = Hm + damping * np.diag(np.diag(Hm))
    delta, ok = cholesky_solve(A, -b)
    if not ok:
        return M.copy(), np.zeros(6), BIT_SINGULAR
    dd = (((((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2]) + delta[3] * delta[3]) + delta[4] * delta[4])
          + delta[5] * delta[5])
    if not np.isfinite(dd):
        return M.copy(), np.zeros(6), BIT_NONFINITE
    if dd < MIN_STEP2:
        return M.copy(), delta, BIT_SMALL
    new = compose(exp_se3(delta), M)
    if not np.isfinite(new).all():
        return M.copy(), np.zeros(6), BIT_NONFINITE
    return new, delta, 0


def inverse12(M):
    """The inverse of a rigid motion as the header forms it in double: R^T, 0 - ((R0i t0 + R1i t1) + R2i t2)."""
    M = np.asarray(M, np.float64).reshape(3, 4)
    R, t = M[:, :3], M[:, 3]
    back = np.array([0.0 - ((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)])
    return np.hstack([R.T, back[:, None]]).reshape(12)


# ---- the whole estimate ----
def pyramids(rgb_ref, disp_ref, ok, rgb_cur, levels, min_disp, max_jump):
    """Per level: (grey_ref, disp, ok, grey_cur) of one image."""
    g0, g1 = grey_of(rgb_ref), grey_of(rgb_cur)
    out = [(g0, np.asarray(disp_ref, F), ok, g1)]
    d, o = out[0][1], ok
    for _ in range(1, levels):
        g0, g1 = down_grey(g0), down_grey(g1)
        d = down_disp(d, o, min_disp, max_jump)
        o = np.ones(d.shape, bool)
        out.append((g0, d, o, g1))
    return out


def estimate_image(rgb_ref, disp_ref, ok, rgb_cur, cam, init=None, **kw):
    """One image.  Returns dict(M float64 [12], pose float32 [2,12], status, info float64 [4], trace float64 [levels*iters,48],
    resid float32 [H,W])."""
    p = params(**kw)
    pyr = pyramids(rgb_ref, disp_ref, ok, rgb_cur, p["levels"], p["min_disp"], p["max_jump"])
    M = IDENTITY12.copy() if init is None else np.asarray(init, F).astype(np.float64).reshape(12)
    status, last, steps, trace = 0, 0.0, 0, []
    for level in range(p["levels"] - 1, -1, -1):
        g0, d, o, g1 = pyr[level]
        for _ in range(p["iters"]):
            terms, use, _ = normal_image(g0, d, o, g1, cam, M, level, p["min_disp"], p["huber"])
            sums, _ = sums_of(terms, use)
            new, delta, st = update(sums, M, p["damping"], p["min_pixels"])
            trace.append(np.concatenate([M, sums, delta, [st]]))
            status |= st
            if st == 0:
                last, steps = float(np.sqrt((delta * delta).sum())), steps + 1
            M = new
    g0, d, o, g1 = pyr[0]
    terms, use, _ = normal_image(g0, d, o, g1, cam, M, 0, p["min_disp"], p["huber"])
    sums, _ = sums_of(terms, use)
    n = sums[28]
    if n < p["min_pixels"]:
        status |= BIT_FINAL_FEW
    info = np.array([n, np.sqrt(sums[27] / n) if n > 0 else 0.0, last, steps])
    pose = np.stack([M, inverse12(M)]).astype(F)
    return dict(M=M, pose=pose, status=status, info=info, trace=np.array(trace), resid=terms[..., 0].copy())


def estimate(rgb_ref, disp_ref, mask, rgb_cur, cam, init=None, **kw):
    """The call on batches: rgb uint8 [B,H,W,3], disp_ref [B,1,H,W], mask uint8 [B,1,H,W] or None, cam [B,5], init [B,12] or None."""
    B = len(rgb_ref)
    out = []
    for b in range(B):
        H, W = rgb_ref[b].shape[:2]
        ok = np.asarray(mask)[b].reshape(H, W) == 1 if mask is not None else np.ones((H, W), bool)
        out.append(estimate_image(rgb_ref[b], np.asarray(disp_ref, F)[b].reshape(H, W), ok, rgb_cur[b], cam[b],
                                  None if init is None else np.asarray(init)[b], **kw))
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


# ---- the scene, textured and anti-aliased ----
def _texture(hit_wall, px, py, pz):
    """Grey level 0..255 as a smooth function of world coordinates: waves on the road (x, z) that fade out with z, since a row of
    the image covers z^2 / (fy * height) metres of road and no wave survives that far out; shorter ones on the wall (x, y)."""
    fade = 1.0 / (1.0 + (pz / 14.0) ** 4)
    road = 128.0 + fade * (45.0 * np.sin(2.1 * px + 0.5) * np.cos(0.4 * pz) + 35.0 * np.sin(0.5 * pz + 0.7 * px) + 20.0 * np.cos(3.0 * px - 0.2 * pz))
    wall = 120.0 + 50.0 * np.sin(1.9 * px + 0.3) * np.cos(1.6 * py) + 40.0 * np.cos(1.3 * px - 2.0 * py + 1.0)
    return np.where(hit_wall, wall, road)


def render_grey(Tcw, H=48, W=96, cam=T.SCENE_CAM, ss=4):
    """uint8 [H,W]: the mean of ss x ss texture samples per pixel (the sky is 90), rounded to uint8 -- band-limited, which a direct
    method needs: with one sample per pixel the far road aliases and the estimate is biased by a third of the step."""
    fx, fy, cx, cy, _ = cam
    R, t = np.asarray(Tcw, np.float64)[:, :3], np.asarray(Tcw, np.float64)[:, 3]
    off = (np.arange(ss) + 0.5) / ss - 0.5
    ys = (np.arange(H)[:, None] + off[None, :]).reshape(-1)
    xs = (np.arange(W)[:, None] + off[None, :]).reshape(-1)
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    ray = np.stack([(xx - cx) / fx, (yy - cy) / fy, np.ones_like(xx)], -1) @ R.T
    with np.errstate(all="ignore"):
        sg = (T.GROUND_Y - t[1]) / ray[..., 1]
        sg = np.where((ray[..., 1] > 0) & (sg > 0), sg, np.inf)
        sw = (T.WALL_Z - t[2]) / ray[..., 2]
        px, py = t[0] + sw * ray[..., 0], t[1] + sw * ray[..., 1]
        hit = (ray[..., 2] > 0) & (sw > 0) & (px > T.WALL_X[0]) & (px < T.WALL_X[1]) & (py >= T.WALL_TOP) & (py <= T.GROUND_Y)
        sw = np.where(hit, sw, np.inf)
        s = np.minimum(sg, sw)
        wall = sw <= sg
        sf = np.where(np.isfinite(s), s, 0.0)
        P = t[None, None, :] + sf[..., None] * ray
        val = np.where(np.isfinite(s), _texture(wall, P[..., 0], P[..., 1], P[..., 2]), 90.0)
    img = val.reshape(H, ss, W, ss).mean(axis=(1, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def scene_cam(H, W):
    """The scene's camera scaled to H x W (48 x 96 is T.SCENE_CAM itself)."""
    s = W / 96.0
    fx, fy, cx, cy, fb = T.SCENE_CAM
    return (fx * s, fy * s, (cx + 0.5) * s - 0.5, (cy + 0.5) * s - 0.5, fb * s)


def edge_codes(d, jump=1.0):
    """uint8 [H,W] codes as lws_lr_check gives them: 0 at the pixels next to a disparity step of more than `jump`, 1 elsewhere.  At
    such an edge the anti-aliased grey mixes two surfaces while the disparity belongs to one of them; a consistency check drops
    these pixels on real data, and left in they pull the estimate by several centimetres."""
    e = np.zeros(d.shape, bool)
    dx, dy = np.abs(d[:, 1:] - d[:, :-1]) > jump, np.abs(d[1:] - d[:-1]) > jump
    e[:, 1:] |= dx
    e[:, :-1] |= dx
    e[1:] |= dy
    e[:-1] |= dy
    return (~e).astype(np.uint8)


def scene_pair(H, W, T0, T1, cam=None):
    """(rgb_ref uint8 [H,W,3], disp_ref float32 [H,W], mask uint8 [H,W], rgb_cur) of the scene seen from the camera-to-world poses
    T0 then T1."""
    cam = cam or scene_cam(H, W)
    g0, g1 = render_grey(T0, H, W, cam), render_grey(T1, H, W, cam)
    d0 = T.render(T0, H, W, cam).astype(F)
    return np.repeat(g0[..., None], 3, -1), d0, edge_codes(d0), np.repeat(g1[..., None], 3, -1)


def true_motion(T0, T1):
    """float64 [12]: what maps a point of camera T0's frame into camera T1's (pose[0] of lws_temporal_step)."""
    a, b = (np.vstack([np.asarray(t, np.float64), [0, 0, 0, 1]]) for t in (T0, T1))
    return np.linalg.solve(b, a)[:3].reshape(12)


def motion_error(M, Mtrue):
    """(translation error in metres, rotation error in degrees) between two [12] motions."""
    A, Bm = np.asarray(M, np.float64).reshape(3, 4), np.asarray(Mtrue, np.float64).reshape(3, 4)
    dR = A[:, :3] @ Bm[:, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return float(np.linalg.norm(A[:, 3] - Bm[:, 3])), float(ang)
