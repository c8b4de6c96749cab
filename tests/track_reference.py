"""lws_track_normal and lws_track (include/lwsnet_track.h) restated in numpy.  Every per-pixel step is one float32 numpy operation
in the order the header gives, so the kernels match `terms` and `resid` bit for bit; the 32 sums and the update are float64, the
sums with numpy's own order of additions, so they agree with the kernels to summation rounding (egomotion_reference.sum_bound).
With dtype=np.float64 the same per-pixel steps run in double: the function whose finite differences the Jacobian is held to.  The
photometric half, the update and the scene are egomotion_reference's; Odometry and ModelTracker over a short sequence are restated
here too (run_sequence), on tsdf_reference's volume with mesh_reference's normals."""
import math

import numpy as np

import egomotion_reference as E
import temporal_reference as T

F = np.float32
DEFAULTS = dict(iters=6, min_disp=0.5, huber_p=10.0, sigma_p=4.0, huber_g=1.5, gate_g=4.0, sigma0=0.5, sigma_min=0.05, lambda_g=1.0,
                damping=0.0, min_pixels=64)
BIT_NO_MODEL = 32
REASONS = ("ref_invalid", "behind", "p_outside", "p_nonfinite", "p_on", "p_huber_in", "p_huber_out", "g_no_normals", "g_no_normal",
           "g_outside_left", "g_outside_right", "g_outside_top", "g_outside_bottom", "g_tap_invalid", "g_sigma_invalid", "g_sigma_floor",
           "g_gated", "g_nonfinite", "g_on", "g_huber_in", "g_huber_out")


def params(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return {**DEFAULTS, **kw}


def weights(p):
    """(kp, kg): the terms' weights in the sums, formed in double from the float32 scalars"""
    sp = np.float64(F(p["sigma_p"]))
    return 1.0 / (sp * sp), np.float64(F(p["lambda_g"]))


def normal_image(gref, disp, ok, normals, gcur, dcur, scur, okc, cam, M, p, dt=F, taps=None):
    """One image: gref, disp, gcur, dcur [H,W]; normals [3,H,W] or None; scur [H,W] or None; ok, okc bool [H,W]; cam the camera
    row; M float64 [12].  taps = (iv, iu, sz) holds the geometric term's association and its standard deviation fixed.  Returns
    (terms [H,W,16] of dt, use_p, use_g, reasons: a dict of masks named in REASONS, (iv, iu, sz))."""
    H, W = gref.shape
    tp, use_p, rs = E.normal_image(gref, disp, ok, gcur, cam, M, 0, p["min_disp"], p["huber_p"], dt)
    disp, dcur = np.asarray(disp, dt), np.asarray(dcur, dt)
    fx, fy, cx, cy, fb = E.level_cam(cam, 0, dt)
    Mf = np.asarray(M, np.float64).astype(dt)
    z0 = np.zeros((H, W), bool)
    why = {k: z0.copy() for k in REASONS}
    why.update(ref_invalid=rs["invalid"], behind=rs["behind"], p_outside=rs["outside"], p_nonfinite=rs["nonfinite"], p_on=use_p)
    with np.errstate(all="ignore"):
        ar = np.abs(tp[..., 0])
        why["p_huber_in"], why["p_huber_out"] = use_p & (ar <= dt(p["huber_p"])), use_p & (ar > dt(p["huber_p"]))
        use0 = ok & np.isfinite(disp) & (disp >= dt(p["min_disp"]))
        z = fb / disp
        X = ((np.arange(W, dtype=dt)[None, :] - cx) * z) / fx
        Y = ((np.arange(H, dtype=dt)[:, None] - cy) * z) / fy
        Qx, Qy, Qz = (T._row(Mf, k, X, Y, z) for k in range(3))
        use = use0 & (Qz > 0)
        u = (fx * Qx) / Qz + cx
        v = (fy * Qy) / Qz + cy
        tg = np.zeros((H, W, 8), dt)
        on = normals is not None and F(p["lambda_g"]) > 0
        if not on:
            why["g_no_normals"] = use.copy()
            return np.concatenate([tp, tg], -1), use_p, z0.copy(), why, None
        n = np.asarray(normals, dt)
        has = np.isfinite(n).all(0) & ~((n[0] == 0) & (n[1] == 0) & (n[2] == 0))
        why["g_no_normal"] = use & ~has
        g = use & has
        why["g_outside_left"], why["g_outside_right"] = g & ~(u >= 0), g & (u >= 0) & ~(u <= dt(W - 1))
        inx = (u >= 0) & (u <= dt(W - 1))
        why["g_outside_top"], why["g_outside_bottom"] = g & inx & ~(v >= 0), g & inx & (v >= 0) & ~(v <= dt(H - 1))
        g = g & inx & (v >= 0) & (v <= dt(H - 1))
        if taps is None:
            iu = np.rint(np.where(g, u, 0)).astype(np.int64)
            iv = np.rint(np.where(g, v, 0)).astype(np.int64)
        else:
            iv, iu = taps[:2]
        dc = dcur[iv, iu]
        tap_ok = okc[iv, iu] & np.isfinite(dc) & (dc >= dt(p["min_disp"]))
        why["g_tap_invalid"] = g & ~tap_ok
        g = g & tap_ok
        s = np.asarray(scur, dt)[iv, iu] if scur is not None else np.full((H, W), dt(F(p["sigma0"])))
        s_ok = (s >= 0) & np.isfinite(s)
        why["g_sigma_invalid"] = g & ~s_ok
        g = g & s_ok
        why["g_sigma_floor"] = g & (s < dt(F(p["sigma_min"])))
        zc = fb / dc
        Px = ((iu.astype(dt) - cx) * zc) / fx
        Py = ((iv.astype(dt) - cy) * zc) / fy
        mx, my, mz = ((Mf[4 * r] * n[0] + Mf[4 * r + 1] * n[1]) + Mf[4 * r + 2] * n[2] for r in range(3))
        sg = np.maximum(s, dt(F(p["sigma_min"])))
        sz = sg * ((Qz * Qz) / fb) if taps is None else taps[2]
        ex, ey, ez = Qx - Px, Qy - Py, Qz - zc
        rg = ((ex * mx + ey * my) + ez * mz) / sz
        ag = np.abs(rg)
        gate_ok = ag <= dt(F(p["gate_g"]))
        why["g_gated"] = g & ~gate_ok
        g = g & gate_ok
        hub = dt(F(p["huber_g"]))
        wg = np.where(ag <= hub, dt(1), hub / ag)
        c0, c1, c2 = Py * mz - zc * my, zc * mx - Px * mz, Px * my - Py * mx
        J = [mx / sz, my / sz, mz / sz, c0 / sz, c1 / sz, c2 / sz]
        finite = np.isfinite(rg)
        for j in J:
            finite &= np.isfinite(j)
        why["g_nonfinite"] = g & ~finite
        g = g & finite
        why["g_on"], why["g_huber_in"], why["g_huber_out"] = g, g & (ag <= hub), g & (ag > hub)
        tg = np.where(g[..., None], np.stack([rg, wg] + J, -1), dt(0)).astype(dt)
    return np.concatenate([tp, tg], -1), use_p, g, why, (iv, iu, sz)


def _cols(t, k):
    r, w, J = t[:, 0], t[:, 1], t[:, 2:]
    kw = k * w
    wJ = kw[:, None] * J
    cols = [wJ[:, i] * J[:, j] for i, j in E.TRI] + [wJ[:, i] * r for i in range(6)] + [(kw * r) * r, np.ones(len(t))]
    return np.stack(cols, -1) if len(t) else np.zeros((0, 29))


def sums_of(terms, use_p, use_g, p):
    """(sums float64 [32], mag float64 [32], n float64 [32]: per entry the sum of the products' absolute values and their number)"""
    kp, kg = weights(p)
    cp, cg = _cols(terms[use_p][:, :8].astype(np.float64), kp), _cols(terms[use_g][:, 8:].astype(np.float64), kg)
    sums, mag, n = np.zeros(32), np.zeros(32), np.zeros(32)
    sums[:27], mag[:27] = cp[:, :27].sum(0) + cg[:, :27].sum(0), np.abs(cp[:, :27]).sum(0) + np.abs(cg[:, :27]).sum(0)
    n[:27] = len(cp) + len(cg)
    sums[27:29], mag[27:29], n[27:29] = cp[:, 27:].sum(0), np.abs(cp[:, 27:]).sum(0), len(cp)
    sums[29:31], mag[29:31], n[29:31] = cg[:, 27:].sum(0), np.abs(cg[:, 27:]).sum(0), len(cg)
    return sums, mag, n


def _ok(mask, b, H, W):
    return np.asarray(mask).reshape(-1, H, W)[b] == 1 if mask is not None else np.ones((H, W), bool)


def normal(grey_ref, disp_ref, normals_ref, mask_ref, grey_cur, disp_cur, sigma_cur, mask_cur, cam, M, **kw):
    """The call on [B,1,H,W] arrays (normals [B,3,H,W]): dict(sums [B,32], terms [B,H,W,16], mag, n [B,32], why: a list of dicts)."""
    p = params(**kw)
    B = len(grey_ref)
    H, W = np.shape(grey_ref)[-2:]
    m = lambda a: None if a is None else np.asarray(a, F).reshape(B, H, W)
    g0, d0, g1, d1, s1 = m(grey_ref), m(disp_ref), m(grey_cur), m(disp_cur), m(sigma_cur)
    out = dict(sums=np.zeros((B, 32)), mag=np.zeros((B, 32)), n=np.zeros((B, 32)), terms=np.zeros((B, H, W, 16), F), why=[])
    for b in range(B):
        t, up, ug, why, _ = normal_image(g0[b], d0[b], _ok(mask_ref, b, H, W), None if normals_ref is None else np.asarray(normals_ref, F)[b],
                                         g1[b], d1[b], None if s1 is None else s1[b], _ok(mask_cur, b, H, W), cam[b],
                                         np.asarray(M, np.float64).reshape(B, 12)[b], p)
        out["terms"][b] = t
        out["sums"][b], out["mag"][b], out["n"][b] = sums_of(t, up, ug, p)
        out["why"].append(why)
    return out


def update(sums, M, damping, min_pixels):
    """One Gauss-Newton step from the 32 sums: egomotion_reference.update with n = n_p + n_g and every sum required finite."""
    s29 = np.concatenate([sums[:27], [0.0 if np.isfinite(sums).all() else np.nan, sums[28] + sums[30]]])
    return E.update(s29, M, damping, min_pixels)


def track_image(rgb_ref, disp_ref, normals_ref, ok, rgb_cur, disp_cur, sigma_cur, okc, cam, init=None, dt=F, **kw):
    """One image.  Returns dict(M float64 [12], pose float32 [2,12], status, info float64 [6], trace float64 [iters,51], resid
    float32 [2,H,W], mags: per step the (mag, n) of its sums)."""
    p = params(**kw)
    g0, g1 = E.grey_of(rgb_ref), E.grey_of(rgb_cur)
    M = E.IDENTITY12.copy() if init is None else np.asarray(init, F).astype(np.float64).reshape(12)
    kp, kg = weights(p)
    status, last, steps, trace, mags = 0, 0.0, 0, [], []
    lin = lambda M: normal_image(g0, disp_ref, ok, normals_ref, g1, disp_cur, sigma_cur, okc, cam, M, p, dt)
    for _ in range(p["iters"]):
        t, up, ug, _, _ = lin(M)
        sums, mag, n = sums_of(t, up, ug, p)
        new, delta, st = update(sums, M, p["damping"], p["min_pixels"])
        trace.append(np.concatenate([M, sums, delta, [st]]))
        mags.append((mag, n))
        status |= st
        if st == 0:
            last, steps = float(np.sqrt((delta * delta).sum())), steps + 1
        M = new
    t, up, ug, _, _ = lin(M)
    sums, _, _ = sums_of(t, up, ug, p)
    n_p, n_g = sums[28], sums[30]
    if n_p + n_g < p["min_pixels"]:
        status |= E.BIT_FINAL_FEW
    if n_g < p["min_pixels"]:
        status |= BIT_NO_MODEL
    info = np.array([n_p, np.sqrt(sums[27] / (kp * n_p)) if n_p > 0 else 0.0, n_g, np.sqrt(sums[29] / (kg * n_g)) if n_g > 0 else 0.0, last, steps])
    pose = np.stack([M, E.inverse12(M)]).astype(F)
    return dict(M=M, pose=pose, status=status, info=info, trace=np.array(trace), resid=np.stack([t[..., 0], t[..., 8]]).astype(F), mags=mags)


def track(rgb_ref, disp_ref, normals_ref, mask_ref, rgb_cur, disp_cur, sigma_cur, mask_cur, cam, init=None, **kw):
    """The call on batches, as normal(); init [B,12] or None."""
    B = len(rgb_ref)
    H, W = rgb_ref[0].shape[:2]
    m = lambda a: None if a is None else np.asarray(a, F).reshape(B, H, W)
    d0, d1, s1 = m(disp_ref), m(disp_cur), m(sigma_cur)
    out = [track_image(rgb_ref[b], d0[b], None if normals_ref is None else np.asarray(normals_ref, F)[b], _ok(mask_ref, b, H, W), rgb_cur[b], d1[b],
                       None if s1 is None else s1[b], _ok(mask_cur, b, H, W), cam[b], None if init is None else np.asarray(init)[b], **kw)
           for b in range(B)]
    return {k: (np.stack([o[k] for o in out]) if k != "mags" else [o[k] for o in out]) for k in out[0]}


# ---- analytic scenes of planes: model maps and current maps without a volume ----
CORNER = ((np.array([0.0, 1.0, 0.0]), 0.7), (np.array([0.0, 0.0, 1.0]), 6.0), (np.array([1.0, 0.0, 0.3]) / np.hypot(1.0, 0.3), 3.0))
ROAD_WALL = ((np.array([0.0, 1.0, 0.0]), T.GROUND_Y), (np.array([0.0, 0.0, 1.0]), T.WALL_Z))


def planes_view(planes, Tcw, H, W, cam):
    """(disp float32 [H,W], normals float32 [3,H,W] in the camera's frame, facing it) of the world planes {m . P = h} seen from the
    camera-to-world pose Tcw: per pixel the nearest plane in front of the camera; 0 and a zero normal where no plane is met."""
    fx, fy, cx, cy, fb = cam
    Tcw = np.asarray(Tcw, np.float64)
    R, t = Tcw[:, :3], Tcw[:, 3]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray_c = np.stack([(xx - cx) / fx, (yy - cy) / fy, np.ones_like(xx)], -1)          # z = 1 along the ray: s is the depth
    ray = ray_c @ R.T
    best, nrm = np.full((H, W), np.inf), np.zeros((H, W, 3))
    with np.errstate(all="ignore"):
        for m, h in planes:
            s = (h - m @ t) / (ray @ m)
            hit = np.isfinite(s) & (s > 0.05) & (s < best)
            nc = R.T @ m
            nc = np.where((ray_c @ nc)[..., None] > 0, -nc, nc)
            best, nrm = np.where(hit, s, best), np.where(hit[..., None], nc, nrm)
        disp = np.where(np.isfinite(best), fb / best, 0.0)
    return disp.astype(F), np.moveaxis(nrm, -1, 0).astype(F)


def motion_pose(delta):
    """The camera-to-world pose of a camera that the twist delta moves away from the identity pose: the inverse of exp(delta)."""
    M = E.exp_se3(delta)
    return E.inverse12(M.reshape(12)).reshape(3, 4)


# ---- a short sequence: the frame-to-frame chain alone, and the chain refined against the volume ----
SEQUENCE = dict(H=48, W=96, frames=7, dz=0.3, yaw=0.01, origin=(-5.0, -1.5, 0.5), vs=0.125, dims=(81, 27, 105), mu0=0.5, mu_d=0.6, noise=0.2,
                z_near=0.5, w_min=0.0, max_jump=1.0)


def sequence_inputs(noise, seed, frames=None, codes=True, **kw):
    """The synthetic road-and-wall scene over `frames` poses forward_pose(k, dz, yaw): per frame (rgb uint8 [H,W,3], disp float32
    [H,W] with seeded Gaussian noise of `noise` px on its valid pixels, codes uint8 [H,W] from the clean map's edges -- all 1, which is
    what a frame without a code map means, where `codes` is off), the camera
    row and the true camera-to-world poses."""
    s = {**SEQUENCE, **kw}
    H, W, n = s["H"], s["W"], frames or s["frames"]
    cam = E.scene_cam(H, W)
    rng = np.random.default_rng(seed)
    poses = [T.forward_pose(k, s["dz"], yaw=s["yaw"]) for k in range(n)]
    out = []
    for P in poses:
        g, d = E.render_grey(P, H, W, cam), T.render(P, H, W, cam).astype(F)
        noisy = np.where(d > 0, d + F(noise) * rng.standard_normal(d.shape).astype(F), d).astype(F)
        out.append((np.repeat(g[..., None], 3, -1), noisy, E.edge_codes(d) if codes else np.ones(d.shape, np.uint8)))
    return out, np.asarray(cam, F), np.stack(poses)


def _c2w_step(Tprev, M):
    """The camera-to-world pose after the motion M (previous camera into the current one), in float64, from the float32 pose block."""
    m = np.asarray(M, F).astype(np.float64).reshape(3, 4)
    inv = np.hstack([m[:, :3].T, -(m[:, :3].T @ m[:, 3])[:, None]])
    return np.hstack([Tprev[:, :3] @ inv[:, :3], (Tprev[:, :3] @ inv[:, 3] + Tprev[:, 3])[:, None]])


def run_sequence(inputs, cam, ego_kw, track_kw, fill=True, **kw):
    """Odometry alone and Odometry + ModelTracker + TsdfVolume on the same inputs, restated: dict(chain, tracked: float64 [n,3,4]
    camera-to-world poses, ego, track: the per-frame results, bounds: per tracked frame the bound on what two orders of adding the
    sums may move its motion by)."""
    import mesh_reference as SN
    import tsdf_reference as V
    s = {**SEQUENCE, **kw}
    min_disp = track_kw.get("min_disp", DEFAULTS["min_disp"])
    H, W = inputs[0][1].shape
    Gx, Gy, Gz = s["dims"]
    Tv, Wv = np.zeros((Gz, Gy, Gx), F), np.zeros((Gz, Gy, Gx), F)
    far = s["z_near"] + s["vs"] * math.sqrt(sum((g - 1) ** 2 for g in s["dims"]))        # ops.tsdf_raycast's own default reach
    nsteps = min(max(int(math.ceil((far - s["z_near"]) / (0.5 * s["vs"]))) + 1, 2), 65535)
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    chain, tracked, egos, tracks, bounds = [ident], [ident], [], [], []
    last_ego, last_motion = None, None
    for k in range(1, len(inputs)):
        (rgb0, d0, c0), (rgb1, d1, c1) = inputs[k - 1], inputs[k]
        init = None if last_ego is None or last_ego["status"] & E.BIT_FINAL_FEW else last_ego["pose"][0]
        ego = E.estimate_image(rgb0, d0, c0 == 1, rgb1, cam, init, **ego_kw)
        last_ego = ego
        egos.append(ego)
        chain.append(_c2w_step(chain[-1], ego["pose"][0]))
        # the volume takes frame k - 1 at its tracked pose, then shows it from there
        pb = V.pose_block(tracked[-1])[None]
        sn, _ = SN.surface_normals(d0[None, None], c0[None, None], cam[None], min_disp, np.inf, s["max_jump"])      # the plane distance, as the CLI's volume
        Tv, Wv, _, _ = V.integrate(Tv, Wv, None, s["origin"], s["vs"], d0[None, None], cam[None], pb, mask=c0[None, None], normals=sn, mu0=s["mu0"], mu_d=s["mu_d"],
                                   min_disp=min_disp, sigma0=track_kw.get("sigma0", DEFAULTS["sigma0"]))
        vd, _, vn = V.raycast(Tv, Wv, s["origin"], s["vs"], cam[None], pb, H, W, s["z_near"], 0.5 * s["vs"], nsteps, s["w_min"])
        hit = vd[0, 0] > 0
        n_ref = np.where(hit[None], vn[0], F(0))
        d_ref, ok_ref = (np.where(hit, vd[0, 0], d0), hit | (c0 == 1)) if fill else (vd[0, 0], np.ones((H, W), bool))
        start = ego["pose"][0] if not ego["status"] & E.BIT_FINAL_FEW else last_motion
        tr = track_image(rgb0, d_ref, n_ref, ok_ref, rgb1, d1, None, c1 == 1, cam, start, **track_kw)
        kept = tr["pose"][0] if not tr["status"] & E.BIT_FINAL_FEW else (np.asarray(start, F) if start is not None else E.IDENTITY12.astype(F))
        last_motion = kept
        tr["hit"] = hit                                     # where the model gave the reference disparity; elsewhere the fill did, or nothing
        tracks.append(tr)
        tracked.append(_c2w_step(tracked[-1], kept))
        bounds.append(step_bound(tr))
    return dict(chain=np.stack(chain), tracked=np.stack(tracked), ego=egos, track=tracks, bounds=bounds)


def step_bound(tr):
    """What the order of the additions may move a lws_track result's motion by, to first order: per step taken the sums differ by
    at most sum_bound, which moves delta = -(A^-1 b) by at most |A^-1| (|db| + |dA| |delta|) (2-norms); the steps add up.  The
    float32 rounding of the pose block (2^-23 of entries below 2 in magnitude: 2^-22) comes on top."""
    total = 2.0 ** -22
    for row, (mag, n) in zip(tr["trace"], tr["mags"]):
        if row[50] != 0:
            continue
        b = E.sum_bound(n, mag)
        Hm, _ = E.unpack(row[12:39])
        dH, db = E.unpack(b[:27])
        total += np.linalg.norm(np.linalg.inv(Hm), 2) * (np.linalg.norm(db) + np.linalg.norm(dH, 2) * np.linalg.norm(row[44:50]))
    return total
