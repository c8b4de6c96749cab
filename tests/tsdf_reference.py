"""lws_tsdf_integrate, lws_tsdf_raycast and lws_tsdf_points (include/lwsnet_tsdf.h) restated in numpy float32, operation for
operation.  Every float step below is one float32 numpy operation in the order the header gives, so the HIP kernels match these
arrays bit for bit.  Nothing here modifies its arguments: a volume goes in and a new one comes out."""
import numpy as np

F = np.float32
INTEGRATE_DEFAULTS = dict(sigma0=0.5, min_disp=1.0, max_depth=np.inf, mu0=0.25, mu_d=0.0, sigma_min=0.05, wmode=0, w_max=np.inf)
BRANCHES = ("behind", "outside", "invalid", "below_band", "truncated", "in_band", "first_touch", "clamped", "zero_normal", "colour_written",
            "colour_not_written", "colour_blended", "colour_cleared")


def _quiet():
    return np.errstate(all="ignore")


def _row(M, r, X, Y, Z):
    return ((M[4 * r] * X + M[4 * r + 1] * Y) + M[4 * r + 2] * Z) + M[4 * r + 3]


def _rot(M, r, X, Y, Z):
    return (M[4 * r] * X + M[4 * r + 1] * Y) + M[4 * r + 2] * Z


def _lerp(p, q, s):
    return p + s * (q - p)


def _normalise(gx, gy, gz):
    """-> [..., 3]: g / len where len is finite and > 0, zero elsewhere."""
    with _quiet():
        ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
        good = np.isfinite(ln) & (ln > 0)
        return np.stack([np.where(good, g / ln, F(0)) for g in (gx, gy, gz)], -1).astype(F)


def centres(origin, vs, dims):
    """The voxel centres (xw [Gx], yw [Gy], zw [Gz]) of a volume of dims = (Gx, Gy, Gz): o + (float)i * vs."""
    return tuple(F(o) + np.arange(g, dtype=F) * F(vs) for o, g in zip(origin, dims))


def pose_block(c2w):
    """float32 [2,12] of a camera-to-world [3,4] float64 pose: world -> camera (the inverse, in float64) and camera -> world."""
    m = np.vstack([np.asarray(c2w, np.float64).reshape(3, 4), [0, 0, 0, 1]])
    return np.stack([np.linalg.inv(m)[:3].reshape(12), m[:3].reshape(12)]).astype(F)


def integrate_frame(T, Wt, C, origin, vs, disp, sigma, ok, normals, rgb, cam, P0, p, stats=None):
    """One frame into the volume.  T, Wt [Gz,Gy,Gx], C uint8 [Gz,Gy,Gx,4] or None; disp [H,W], sigma [H,W] or None, ok bool [H,W],
    normals [3,H,W] or None, rgb uint8 [H,W,3] or None, cam [5], P0 float32 [12].  -> (T, Wt, C, voxels taken); stats: a dict that
    gathers the voxels per branch of the rule."""
    Gz, Gy, Gx = T.shape
    H, W = disp.shape
    fx, fy, cx, cy, fb = np.asarray(cam, F)
    P0 = np.asarray(P0, F)
    xs, ys, zs = centres(origin, vs, (Gx, Gy, Gz))
    xw, yw, zw = xs[None, None, :], ys[None, :, None], zs[:, None, None]
    with _quiet():
        Px, Py, Pz = (np.broadcast_to(_row(P0, r, xw, yw, zw), T.shape) for r in range(3))
        front = Pz > 0
        u = (fx * Px) / Pz + cx
        v = (fy * Py) / Pz + cy
        inn = front & (u >= 0) & (u <= F(W - 1)) & (v >= 0) & (v <= F(H - 1))
        iu = np.where(inn, np.rint(u), F(0)).astype(np.int64)
        iv = np.where(inn, np.rint(v), F(0)).astype(np.int64)
        d = np.asarray(disp, F)[iv, iu]
        z = fb / d
        valid = ok[iv, iu] & np.isfinite(d) & (d >= F(p["min_disp"])) & (z <= F(p["max_depth"]))
        s = np.asarray(sigma, F)[iv, iu] if sigma is not None else np.full(T.shape, p["sigma0"], F)
        valid &= (s >= 0) & np.isfinite(s)
        sg = np.fmax(s, F(p["sigma_min"]))
        X = ((iu.astype(F) - cx) * z) / fx
        Y = ((iv.astype(F) - cy) * z) / fy
        sdf = z - Pz
        has_n = np.zeros(T.shape, bool)
        if normals is not None:
            nx, ny, nz = (np.asarray(normals, F)[k][iv, iu] for k in range(3))
            has_n = (nx != 0) | (ny != 0) | (nz != 0)
            sdf = np.where(has_n, -(((X - Px) * nx + (Y - Py) * ny) + (z - Pz) * nz), sdf)
        zz = (z * z) / fb
        mu = np.fmax(F(p["mu0"]), F(p["mu_d"]) * zz)
        w = np.ones(T.shape, F) if p["wmode"] == 0 else F(1) / ((sg * zz) * (sg * zz))
        wok = np.isfinite(w) & (w > 0)
        take = inn & valid & (sdf >= -mu) & wok
        t = np.fmin(sdf, mu)
        Wn = Wt + w
        seen = Wt > 0
        Tn = np.where(seen, (T * Wt + t * w) / Wn, t)
        T2 = np.where(take, Tn, T).astype(F)
        W2 = np.where(take, np.fmin(Wn, F(p["w_max"])), Wt).astype(F)
        C2 = None
        coloured = take & (sdf <= mu)
        if C is not None:
            C2 = C.copy()
            blend = seen & (C[..., 3] == 255)
            for k in range(3):
                c = np.asarray(rgb)[iv, iu, k]
                m = np.fmin(np.fmax(np.rint((C[..., k].astype(F) * Wt + c.astype(F) * w) / Wn), F(0)), F(255)).astype(np.uint8)
                C2[..., k] = np.where(coloured, np.where(blend, m, c), C[..., k])
            C2[..., 3] = np.where(coloured, np.uint8(255), C[..., 3])
            C2[take & ~coloured & ~seen] = 0
    if stats is not None:
        meas = inn & valid & wok
        for key, m in (("behind", ~front), ("outside", front & ~inn), ("invalid", inn & ~(valid & wok)), ("below_band", meas & ~(sdf >= -mu)),
                       ("truncated", take & (sdf > mu)), ("in_band", take & ~(sdf > mu)), ("first_touch", take & ~seen),
                       ("clamped", take & (Wn > F(p["w_max"]))), ("zero_normal", take & ~has_n if normals is not None else take & False),
                       ("colour_written", coloured if C is not None else take & False),
                       ("colour_not_written", take & ~coloured if C is not None else take & False),
                       ("colour_blended", coloured & blend if C is not None else take & False),
                       ("colour_cleared", take & ~coloured & ~seen if C is not None else take & False)):
            stats[key] = stats.get(key, 0) + int(m.sum())
    return T2, W2, C2, int(take.sum())


def integrate(T, Wt, C, origin, vs, disp, cam, pose, sigma=None, mask=None, normals=None, rgb=None, stats=None, **kw):
    """The call: disp [B,1,H,W], cam float32 [B,5], pose float32 [B,2,12], sigma [B,1,H,W], mask uint8 [B,1,H,W], normals
    [B,3,H,W], rgb uint8 [B,H,W,3].  -> (T, Wt, C, updated int64 [B]); the frames are integrated in order."""
    unknown = set(kw) - set(INTEGRATE_DEFAULTS)
    assert not unknown, unknown
    assert (C is None) == (rgb is None)
    p = {**INTEGRATE_DEFAULTS, **kw}
    disp = np.asarray(disp, F)
    B, _, H, W = disp.shape
    pose = np.asarray(pose, F).reshape(B, 2, 12)
    updated = np.zeros(B, np.int64)
    for b in range(B):
        ok = mask[b, 0] == 1 if mask is not None else np.ones((H, W), bool)
        T, Wt, C, updated[b] = integrate_frame(T, Wt, C, origin, vs, disp[b, 0], None if sigma is None else sigma[b, 0], ok,
                                               None if normals is None else normals[b], None if rgb is None else rgb[b], cam[b], pose[b, 0], p, stats)
    return T, Wt, C, updated


def sample(T, Wt, origin, vs, w_min, px, py, pz):
    """sample(P) of the header on arrays of points -> (f, wf, inside, known); f means something only where known, wf where inside."""
    Gz, Gy, Gx = T.shape
    with _quiet():
        g = [(q - F(o)) / F(vs) for q, o in zip((px, py, pz), origin)]
        inside = np.ones(np.shape(px), bool)
        for gi, G in zip(g, (Gx, Gy, Gz)):
            inside &= (gi >= 0) & (gi < F(G - 1))
        fl = [np.where(inside, np.floor(gi), F(0)) for gi in g]
        ix, iy, iz = (f.astype(np.int64) for f in fl)
        ax, ay, az = (gi - f for gi, f in zip(g, fl))
        known = inside.copy()
        tw, tt = {}, {}
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    w = Wt[iz + dz, iy + dy, ix + dx]
                    tw[dz, dy, dx], tt[dz, dy, dx] = w, T[iz + dz, iy + dy, ix + dx]
                    known &= (w > 0) & (w >= F(w_min))

        def blend(t):
            lo = _lerp(_lerp(t[0, 0, 0], t[0, 0, 1], ax), _lerp(t[0, 1, 0], t[0, 1, 1], ax), ay)
            hi = _lerp(_lerp(t[1, 0, 0], t[1, 0, 1], ax), _lerp(t[1, 1, 0], t[1, 1, 1], ax), ay)
            return _lerp(lo, hi, az).astype(F)
        return blend(tt), blend(tw), inside, known


def raycast(T, Wt, origin, vs, cam, pose, H, W, z_near, step, nsteps, w_min=0.0, stats=None):
    """The call: cam float32 [B,5], pose float32 [B,2,12] -> (disp [B,1,H,W], weight [B,1,H,W], normals [B,3,H,W]); stats: a dict
    that gathers the pixels per way a ray ends."""
    cam = np.asarray(cam, F).reshape(-1, 5)
    B = cam.shape[0]
    pose = np.asarray(pose, F).reshape(B, 2, 12)
    disp, weight, normals = np.zeros((B, 1, H, W), F), np.zeros((B, 1, H, W), F), np.zeros((B, 3, H, W), F)
    vs = F(vs)
    for b in range(B):
        fx, fy, cx, cy, fb = cam[b]
        P0, P1 = pose[b]
        xn = np.broadcast_to((np.arange(W, dtype=F)[None, :] - cx) / fx, (H, W))
        yn = np.broadcast_to((np.arange(H, dtype=F)[:, None] - cy) / fy, (H, W))

        def ray(zc):
            X, Y = xn * zc, yn * zc
            return tuple(_row(P1, r, X, Y, zc) for r in range(3))

        done, hit = np.zeros((H, W), bool), np.zeros((H, W), bool)
        pk, fp, zp, zs = np.zeros((H, W), bool), np.zeros((H, W), F), np.zeros((H, W), F), np.ones((H, W), F)
        ever_inside, ever_unknown, first_interval = np.zeros((H, W), bool), np.zeros((H, W), bool), np.zeros((H, W), bool)
        with _quiet():
            for k in range(nsteps):
                zc = np.full((H, W), F(z_near) + F(k) * F(step), F)
                f, _, inside, known = sample(T, Wt, origin, vs, w_min, *ray(zc))
                both = known & pk & ~done
                h = both & (fp > 0) & (f <= 0)
                m = both & (fp <= 0) & (f > 0)
                zs = np.where(h, zp + (fp / (fp - f)) * (zc - zp), zs).astype(F)
                first_interval |= h & (k == 1)
                ever_inside |= inside & ~done
                ever_unknown |= inside & ~known & ~done
                hit |= h
                done |= h | m
                pk, fp, zp = known, f, zc
                if done.all():
                    break
            hx, hy, hz = ray(zs)
            _, wf, inside, _ = sample(T, Wt, origin, vs, w_min, hx, hy, hz)
            disp[b, 0] = np.where(hit, fb / zs, F(0))
            weight[b, 0] = np.where(hit & inside, wf, F(0))
            six = [sample(T, Wt, origin, vs, w_min, hx + dx, hy + dy, hz + dz)
                   for dx, dy, dz in ((vs, 0, 0), (-vs, 0, 0), (0, vs, 0), (0, -vs, 0), (0, 0, vs), (0, 0, -vs))]
            all_known = np.logical_and.reduce([s[3] for s in six])
            gx, gy, gz = six[0][0] - six[1][0], six[2][0] - six[3][0], six[4][0] - six[5][0]
            n = _normalise(*(_rot(P0, r, gx, gy, gz) for r in range(3)))
            normals[b] = np.where((hit & all_known)[None], np.moveaxis(n, -1, 0), F(0))
        if stats is not None:
            for key, msk in (("never_inside", ~ever_inside), ("hit", hit), ("back_face", done & ~hit), ("exhausted", ever_inside & ~done),
                             ("unknown_on_the_way", ever_unknown), ("first_interval", first_interval), ("normal_unknown", hit & ~all_known),
                             ("normal", hit & all_known)):
                stats[key] = stats.get(key, 0) + int(msk.sum())
    return disp, weight, normals


def points(T, Wt, C, origin, vs, w_min=0.0):
    """-> (xyz float32 [n,3], rgba uint8 [n,4], normals float32 [n,4], axis int [n], up bool [n]: Ta <= 0) of every crossing, in the
    order of the header: voxels in raster order, the axes x, y, z per voxel."""
    Gz, Gy, Gx = T.shape
    xs, ys, zs = centres(origin, vs, (Gx, Gy, Gz))
    with _quiet():
        obs = (Wt > 0) & (Wt >= F(w_min))
        cross = np.zeros((Gz, Gy, Gx, 3), bool)
        Tb = np.zeros((Gz, Gy, Gx, 3), F)
        for e, ax in enumerate((2, 1, 0)):                  # e = x, y, z is the array axis 2, 1, 0
            a = [slice(None)] * 3
            b = [slice(None)] * 3
            a[ax], b[ax] = slice(0, -1), slice(1, None)
            a, b = tuple(a), tuple(b)
            Ta_, Tb_ = T[a], T[b]
            cross[a + (e,)] = obs[a] & obs[b] & (((Ta_ > 0) & (Tb_ <= 0)) | ((Ta_ <= 0) & (Tb_ > 0)))
            Tb[a + (e,)] = Tb_
        iz, iy, ix, e = np.nonzero(cross)
        Ta, Tb = T[iz, iy, ix], Tb[iz, iy, ix, e]
        s = Ta / (Ta - Tb)
        along = s * F(vs)
        xyz = np.stack([np.where(e == 0, xs[ix] + along, xs[ix]), np.where(e == 1, ys[iy] + along, ys[iy]),
                        np.where(e == 2, zs[iz] + along, zs[iz])], -1).astype(F)
        far = ~(s <= F(0.5))
        jx, jy, jz = ix + (far & (e == 0)), iy + (far & (e == 1)), iz + (far & (e == 2))
        rgba = C[jz, jy, jx] if C is not None else np.full((len(ix), 4), 255, np.uint8)
        inner = (jx >= 1) & (jy >= 1) & (jz >= 1) & (jx + 1 < Gx) & (jy + 1 < Gy) & (jz + 1 < Gz)
        kx, ky, kz = np.clip(jx, 1, Gx - 2), np.clip(jy, 1, Gy - 2), np.clip(jz, 1, Gz - 2)
        nb = ((kz, ky, kx + 1), (kz, ky, kx - 1), (kz, ky + 1, kx), (kz, ky - 1, kx), (kz + 1, ky, kx), (kz - 1, ky, kx))
        good = inner & np.logical_and.reduce([obs[i] for i in nb]) if len(ix) else inner
        n = _normalise(T[nb[0]] - T[nb[1]], T[nb[2]] - T[nb[3]], T[nb[4]] - T[nb[5]])
        normals = np.zeros((len(ix), 4), F)
        normals[:, :3] = np.where(good[:, None], n, F(0))
    return xyz, np.ascontiguousarray(rgba), normals, e, Ta <= 0


def records(xyz, rgba):
    """The 16-byte records of lws_tsdf_points as uint8 [n,16]."""
    out = np.empty((len(xyz), 16), np.uint8)
    out[:, :12] = np.ascontiguousarray(xyz, F).view(np.uint8).reshape(-1, 12)
    out[:, 12:] = rgba
    return out


# ---- the cases of the tests: tests/test_tsdf_cpu.py asserts what they reach, tests/test_gpu_tsdf.py runs them on the device ----
VOLUMES, MAPS, BATCHES = ((5, 3, 2), (33, 4, 5), (65, 7, 9)), ((5, 7), (48, 96)), (1, 3)
# lws_tsdf_points scans its Gy * Gz row counts in chunks of 256 with a carry: volumes (for points_volume(dims, 1)) of exactly 256
# rows, of 258 rows and of 520 rows (two carries), with 972, 728 and 2919 crossings
POINTS_CHUNKED = {(6, 16, 16): 972, (5, 3, 86): 728, (9, 20, 26): 2919}
# camera-to-world motions (temporal_reference.forward_pose: dz, yaw, dx); the last one puts part of every volume behind the camera
MOTIONS = {"identity": (0.0, 0.0, 0.0), "yaw_and_step": (0.3, 0.05, 0.2), "backward": (11.8, 0.0, 0.0)}
_CASES = {}


def case_camera(H, W):
    """The float32 camera row of an H x W view of temporal_reference's scene, with a baseline that keeps the wall above 1 px."""
    f = max(1.25 * W, 8.0)
    return np.array([f, f, (W - 1) / 2.0, 0.4 * (H - 1), 4.0 * f], F)


def case_volume(dims):
    """(origin, vs) of a volume of dims that is 8 m wide and centred where the scene's wall meets its road."""
    vs = 8.0 / (dims[0] - 1)
    return (-4.0, 1.5 - 0.5 * (dims[1] - 1) * vs, 12.0 - 0.5 * (dims[2] - 1) * vs), vs


def poisoned_state(dims, mu, rng, colour):
    """A volume that already holds state: weights 0, 1 and 2.5, T in the band; where Wt == 0, T is NaN and C 0xFF -- never read."""
    shape = dims[::-1]
    Wt = rng.choice(np.array([0.0, 0.0, 1.0, 2.5], F), size=shape)
    T = np.where(Wt > 0, rng.uniform(-mu, mu, shape), np.nan).astype(F)
    C = None
    if colour:
        C = rng.integers(0, 256, (*shape, 4), dtype=np.uint8)
        C[..., 3] = rng.choice(np.array([0, 255, 255], np.uint8), size=shape)
        C[Wt == 0] = 0xFF
    return T, Wt, C


def integrate_case(dims, hw, B, i=0):
    """Case i of (volume, map, batch): the inputs, and `want` = (T, Wt, C, updated) with `stats`, the voxels per branch."""
    import mesh_reference as M
    import temporal_reference as TR
    key = (tuple(dims), tuple(hw), B, i)
    if key in _CASES:
        return _CASES[key]
    n = VOLUMES.index(tuple(dims)) * 4 + MAPS.index(tuple(hw)) * 2 + BATCHES.index(B) + i
    rng = np.random.default_rng(100 + n)
    H, W = hw
    cam = np.tile(case_camera(H, W), (B, 1))
    origin, vs = case_volume(dims)
    names = list(MOTIONS)
    c2w = [TR.forward_pose(1, *MOTIONS[names[(n + b) % 3]]) for b in range(B)]
    pose = np.stack([pose_block(p) for p in c2w])
    truth = np.stack([TR.render(p, H, W, tuple(float(v) for v in cam[0])) for p in c2w])[:, None]
    disp = np.where(truth > 0, truth + rng.normal(0, 0.05, truth.shape), 0).astype(F)
    normals = M.surface_normals(disp, None, cam, 1.0, np.inf, 1.0)[0]
    flat = disp.reshape(-1)
    idx = rng.choice(flat.size, size=max(1, flat.size // 8), replace=False)
    flat[idx] = np.array([np.nan, np.inf, -np.inf, 0.0, -3.0, 0.5], F)[np.arange(len(idx)) % 6]
    nf = np.moveaxis(normals, 1, -1).reshape(-1, 3)          # (a copy: moveaxis of a [B,3,H,W] array is not contiguous)
    nf[::7] = 0.0                                           # the zero normal: the distance along the ray
    nf[3::11] *= F(2.0)                                     # a normal that is not a unit vector is followed as it is
    nf[5::97, 1] = np.nan
    normals = np.ascontiguousarray(np.moveaxis(nf.reshape(B, H, W, 3), -1, 1))
    sigma = rng.uniform(0.0, 1.0, disp.shape).astype(F)
    sigma.reshape(-1)[::9] = 0.0
    sigma.reshape(-1)[4::13] = np.nan
    sigma.reshape(-1)[6::17] = -0.25
    mask = rng.choice(np.array([0, 1, 1, 1, 2], np.uint8), size=disp.shape)
    rgb = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    use = dict(sigma=n % 2 == 0, mask=n % 4 >= 2, normals=n % 3 != 0, rgb=n % 5 != 1)
    kw = dict(sigma0=0.25, min_disp=1.0, max_depth=(np.inf, 12.6)[n % 2], mu0=(1.5 * vs, 0.75 * vs)[n // 2 % 2], mu_d=(0.0, 0.5)[n // 3 % 2],
              sigma_min=0.05, wmode=(0, 1)[n // 2 % 2], w_max=(np.inf, 3.0)[n % 3 == 1])
    T0, W0, C0 = poisoned_state(dims, kw["mu0"], rng, use["rgb"])
    c = dict(dims=tuple(dims), origin=origin, vs=vs, B=B, H=H, W=W, cam=cam, pose=pose, c2w=c2w, disp=disp, T0=T0, W0=W0, C0=C0, kw=kw,
             sigma=sigma if use["sigma"] else None, mask=mask if use["mask"] else None, normals=normals if use["normals"] else None,
             rgb=rgb if use["rgb"] else None, stats={})
    c["want"] = integrate(T0, W0, C0, origin, vs, disp, cam, pose, c["sigma"], c["mask"], c["normals"], c["rgb"], stats=c["stats"], **kw)
    _CASES[key] = c
    return c


def integrate_cases():
    return [integrate_case(d, hw, B) for d in VOLUMES for hw in MAPS for B in BATCHES]


def crafted_volume(dims=(20, 12, 16), vs=0.25, seed=0):
    """A tilted wall about 2 m in front of the origin, written as a volume by hand: T the distance to the plane clipped to +-mu,
    unobserved (and poisoned) behind the band and in random holes, weights 1 .. 3.  -> (T, Wt, origin, vs)."""
    rng = np.random.default_rng(seed)
    origin = (-0.5 * (dims[0] - 1) * vs, -0.5 * (dims[1] - 1) * vs, 0.0)
    xs, ys, zs = centres(origin, vs, dims)
    mu = 3 * vs
    dist = (2.0 + 0.2 * xs[None, None, :] - 0.1 * ys[None, :, None]) - zs[:, None, None]
    Wt = rng.choice(np.array([1.0, 2.0, 3.0], F), size=dims[::-1])
    Wt[dist < -mu] = 0
    Wt[rng.random(dims[::-1]) < 0.03] = 0
    T = np.where(Wt > 0, np.clip(dist, -mu, mu), np.nan).astype(F)
    return T, Wt.astype(F), origin, vs


def raycast_views():
    """(cam [3,5], pose [3,2,12]) of three 24 x 40 views of crafted_volume: from the front -- the view is wider than the volume, so
    rays at its rim never enter it --, from inside the band behind the wall looking back (the back-face stop), and from the side."""
    import temporal_reference as TR
    cam = np.tile(np.array([30.0, 30.0, 19.5, 11.5, 15.0], F), (3, 1))
    back = np.array([[-1, 0, 0, 0.0], [0, 1, 0, 0], [0, 0, -1, 2.5]], np.float64)        # at z = 2.5, turned half a circle about y
    c2w = [TR.forward_pose(1, 0.25), back, TR.forward_pose(1, 0.5, yaw=0.6, dx=-1.0)]
    return cam, np.stack([pose_block(p) for p in c2w])


# the settings of the ray-caster over raycast_views(): a long walk; three steps that start just in front of the wall; a w_min that
# blinds the taps of weight 1; a start behind the wall, from where the view that looks back never enters the volume
RAYCASTS = (dict(z_near=0.5, step=0.125, nsteps=40), dict(z_near=1.9, step=0.25, nsteps=3), dict(z_near=0.5, step=0.125, nsteps=40, w_min=2.0),
            dict(z_near=2.6, step=0.125, nsteps=20))


def points_volume(dims, seed):
    """A volume with crossings on every axis in both directions: T uniform noise with exact zeros, a third of the voxels unobserved
    (and poisoned), weights 1 and 2, a colour per voxel.  -> (T, Wt, C, origin, vs)."""
    rng = np.random.default_rng(seed)
    shape = dims[::-1]
    Wt = rng.choice(np.array([0.0, 1.0, 2.0], F), size=shape)
    T = rng.uniform(-1, 1, shape).astype(F)
    T[rng.random(shape) < 0.1] = 0.0
    T[Wt == 0] = np.nan
    C = rng.integers(0, 256, (*shape, 4), dtype=np.uint8)
    C[Wt == 0] = 0xFF
    return T, Wt, C, (-1.0, 0.5, 2.0), 0.25
