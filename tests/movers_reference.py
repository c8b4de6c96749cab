"""lws_movers (include/lwsnet_movers.h) restated in numpy float32, operation for operation: the evidence codes, the components by a
plain flood fill in raster order (so the numbering falls out of the scan), the dilation, rows / vals / info -- and a compositor
that pastes a fronto-parallel textured box into the road-and-wall scene of tests/temporal_reference.py.  Every float step below is
one float32 numpy operation in the order the header gives, so the HIP kernels match these arrays bit for bit."""
import numpy as np

import egomotion_reference as E
import temporal_reference as T

F = np.float32
DEFAULTS = dict(min_disp=1.0, sigma0=0.5, sigma_min=0.05, gate_g=3.0, gate_p=25.0, radius=0, cand_bits=1 << 2 | 1 << 4, max_diff=1.0,
                min_pixels=64, grow=2, max_movers=64)
UNTESTED, STATIC, APPEARED, UNCOVERED, CHANGED = range(5)
MOVER_CODE = 4
EMPTY_ROW = (0, -1, -1, -1, -1, -1, -1, 0)


def params(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return {**DEFAULTS, **kw}


def residuals(rgb_prev, d_prev, s_prev, ok_prev, rgb_cur, d_cur, s_cur, ok_cur, cam, pose, p):
    """One image: rgb uint8 [H,W,3], d float32 [H,W], s float32 [H,W] or None, ok bool [H,W], cam [5], pose float32 [2,12].
    Returns (tested bool, rg float32, photo bool: the photometric test is on, rp float32, (iv, iu, u, v))."""
    H, W = d_cur.shape
    fx, fy, cx, cy, fb = (F(c) for c in np.asarray(cam, F))
    M = np.asarray(pose, F).reshape(2, 12)[1]
    md, R = F(p["min_disp"]), int(p["radius"])
    d = np.asarray(d_cur, F)
    dpv = np.asarray(d_prev, F)
    sc = np.full((H, W), p["sigma0"], F) if s_cur is None else np.asarray(s_cur, F)
    spv = np.full((H, W), p["sigma0"], F) if s_prev is None else np.asarray(s_prev, F)
    with np.errstate(all="ignore"):
        use = ok_cur & np.isfinite(d) & (d >= md)
        z = fb / d
        X = ((np.arange(W, dtype=F)[None, :] - cx) * z) / fx
        Y = ((np.arange(H, dtype=F)[:, None] - cy) * z) / fy
        Qx, Qy, Qz = (T._row(M, k, X, Y, z) for k in range(3))
        use &= Qz > 0
        u = (fx * Qx) / Qz + cx
        v = (fy * Qy) / Qz + cy
        use &= (u >= 0) & (u <= F(W - 1)) & (v >= 0) & (v <= F(H - 1))
        use &= np.isfinite(sc) & (sc >= 0)
        iu = np.rint(np.where(use, u, F(0))).astype(np.int64)
        iv = np.rint(np.where(use, v, F(0))).astype(np.int64)
        dq = fb / Qz
        sc2 = sc * sc
        have, rg = np.zeros((H, W), bool), np.zeros((H, W), F)
        for j in range(-R, R + 1):
            for i in range(-R, R + 1):
                ty, tx = iv + j, iu + i
                inside = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
                ty, tx = np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)
                dp, sp = dpv[ty, tx], spv[ty, tx]
                usable = use & inside & ok_prev[ty, tx] & np.isfinite(dp) & (dp >= md) & np.isfinite(sp) & (sp >= 0)
                s = np.sqrt(sc2 + sp * sp)
                sg = np.fmax(s, F(p["sigma_min"]))
                r = (dp - dq) / sg
                usable &= ~np.isnan(r)
                better = usable & (~have | (np.abs(r) < np.abs(rg)))
                rg = np.where(better, r, rg)
                have |= usable
        big = W >= 4 and H >= 4
        photo = have & big & (u >= 1) & (u <= F(W - 2)) & (v >= 1) & (v <= F(H - 2))
        rp = np.zeros((H, W), F)
        if big:
            up, vp = np.where(photo, u, F(1)), np.where(photo, v, F(1))
            i0 = np.minimum(np.floor(up).astype(np.int64), W - 3)
            j0 = np.minimum(np.floor(vp).astype(np.int64), H - 3)
            a, b = up - i0.astype(F), vp - j0.astype(F)
            g0, g1 = E.grey_of(rgb_prev), E.grey_of(rgb_cur)
            t00, t01, t10, t11 = g0[j0, i0], g0[j0, i0 + 1], g0[j0 + 1, i0], g0[j0 + 1, i0 + 1]
            top, bot = t00 + a * (t01 - t00), t10 + a * (t11 - t10)
            rp = np.where(photo, g1 - (top + b * (bot - top)), F(0)).astype(F)
    return have, rg.astype(F), photo, rp, (iv, iu, u, v)


def evidence_image(rgb_prev, d_prev, s_prev, ok_prev, rgb_cur, d_cur, s_cur, ok_cur, cam, pose, p):
    """uint8 [H,W]: the evidence codes of one image."""
    have, rg, photo, rp, _ = residuals(rgb_prev, d_prev, s_prev, ok_prev, rgb_cur, d_cur, s_cur, ok_cur, cam, pose, p)
    gg, gp = F(p["gate_g"]), F(p["gate_p"])
    with np.errstate(all="ignore"):
        near = have & (np.abs(rg) <= gg)
        code = np.zeros(rg.shape, np.uint8)
        code[near] = STATIC
        code[have & (rg < -gg)] = APPEARED
        code[have & (rg > gg)] = UNCOVERED
        code[near & photo & (np.abs(rp) > gp)] = CHANGED
    return code


def joined(a, b, max_diff):
    with np.errstate(all="ignore"):
        return bool(np.abs(F(a) - F(b)) <= F(max_diff))


def components(cand, d, max_diff):
    """int32 [H,W]: the component of every candidate pixel, numbered by the raster index of its first pixel (-1: no candidate),
    by a flood fill over the 4-neighbours joined iff |d_p - d_q| <= max_diff in float32; and the components' sizes."""
    H, W = cand.shape
    lab = np.full((H, W), -1, np.int32)
    sizes = []
    for y0, x0 in zip(*np.nonzero(cand)):
        if lab[y0, x0] >= 0:
            continue
        k, n, stack = len(sizes), 0, [(y0, x0)]
        lab[y0, x0] = k
        while stack:
            y, x = stack.pop()
            n += 1
            for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                if 0 <= yy < H and 0 <= xx < W and cand[yy, xx] and lab[yy, xx] < 0 and joined(d[y, x], d[yy, xx], max_diff):
                    lab[yy, xx] = k
                    stack.append((yy, xx))
        sizes.append(n)
    return lab, np.array(sizes, np.int64)


def u16(d):
    with np.errstate(all="ignore"):
        return np.fmin(np.fmax(np.rint(np.asarray(d, F) * F(256.0)), F(0)), F(65535.0)).astype(np.int64)


def grow_flags(m, grow):
    """bool [H,W]: the pixels within Chebyshev distance `grow` of a True of m."""
    H, W = m.shape
    out = np.zeros((H, W), bool)
    pad = np.zeros((H + 2 * grow, W + 2 * grow), bool)
    pad[grow:grow + H, grow:grow + W] = m
    for j in range(2 * grow + 1):
        for i in range(2 * grow + 1):
            out |= pad[j:j + H, i:i + W]
    return out


def segment_image(code, d_cur, mask_cur, cam, p):
    """The part of the call behind the evidence, one image: code uint8 [H,W], d_cur float32 [H,W], mask_cur uint8 [H,W] or None.
    Returns dict(mask, labels, rows, vals, info, comp: the component map before the size test)."""
    H, W = code.shape
    d = np.asarray(d_cur, F)
    fb = F(np.asarray(cam, F)[4])
    K = int(p["max_movers"])
    cand = ((int(p["cand_bits"]) >> code.astype(np.int64)) & 1).astype(bool)
    comp, sizes = components(cand, d, p["max_diff"])
    movers = np.flatnonzero(sizes >= p["min_pixels"])       # component numbers, in the order of their first pixels
    number = np.full(len(sizes) + 1, -1, np.int64)          # (the last entry serves comp == -1)
    is_mover = np.zeros(len(sizes) + 1, bool)
    is_mover[movers] = True
    number[movers] = np.arange(len(movers))
    number[number >= K] = -1
    member = is_mover[comp]
    labels = np.where(member, number[comp], -1).astype(np.int32)
    rows = np.tile(np.array(EMPTY_ROW, np.int32), (K, 1))
    vals = np.zeros((K, 2), F)
    ys, xs = np.mgrid[0:H, 0:W]
    for j, k in enumerate(movers[:K]):
        m = comp == k
        n = int(m.sum())
        rows[j] = (n, xs[m].min(), xs[m].max(), ys[m].min(), ys[m].max(), (code[m] == APPEARED).sum(), (code[m] == UNCOVERED).sum(),
                   (code[m] == CHANGED).sum())
        dm = F((float(u16(d[m]).sum()) / float(n)) / 256.0)
        with np.errstate(all="ignore"):
            vals[j] = (dm, fb / dm)
    grown = grow_flags(member, int(p["grow"]))
    with np.errstate(all="ignore"):
        keep = np.asarray(mask_cur, np.uint8) if mask_cur is not None else (np.isfinite(d) & (d > 0)).astype(np.uint8)
    mask = np.where(grown, np.uint8(MOVER_CODE), keep).astype(np.uint8)
    counts = np.bincount(code.reshape(-1), minlength=5)
    info = np.array([counts[1:].sum(), counts[1], counts[2], counts[3], counts[4], len(sizes), len(movers), grown.sum()], np.int32)
    return dict(mask=mask, labels=labels, rows=rows, vals=vals, info=info, comp=comp)


def segment(rgb_prev, disp_prev, rgb_cur, disp_cur, cam, pose, sigma_prev=None, mask_prev=None, sigma_cur=None, mask_cur=None, **kw):
    """The call on batches: rgb uint8 [B,H,W,3], disp [B,1,H,W], sigmas [B,1,H,W] or None, masks uint8 [B,1,H,W] or None, cam [B,5],
    pose float32 [B,2,12].  Returns dict(evidence, mask [B,1,H,W] uint8, labels [B,1,H,W] int32, rows [B,K,8], vals [B,K,2], info [B,8])."""
    p = params(**kw)
    B, _, H, W = np.shape(disp_cur)
    out = []
    for b in range(B):
        pick = lambda a: None if a is None else np.asarray(a)[b, 0]
        okp = pick(mask_prev) == 1 if mask_prev is not None else np.ones((H, W), bool)
        okc = pick(mask_cur) == 1 if mask_cur is not None else np.ones((H, W), bool)
        code = evidence_image(rgb_prev[b], pick(disp_prev), pick(sigma_prev), okp, rgb_cur[b], pick(disp_cur), pick(sigma_cur), okc, cam[b],
                              np.asarray(pose, F).reshape(-1, 2, 12)[b], p)
        res = segment_image(code, pick(disp_cur), pick(mask_cur), cam[b], p)
        res.pop("comp")
        out.append(dict(evidence=code[None], mask=res["mask"][None], labels=res["labels"][None], rows=res["rows"], vals=res["vals"], info=res["info"]))
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


# ---- the scene with a box in it ----
def box_rect(cam, centre, size, depth, H, W):
    """(x0, x1, y0, y1), half-open: the pixels whose centres a fronto-parallel square of `size` metres covers, centred at the camera
    coordinates `centre` = (X, Y) metres and `depth` metres away."""
    fx, fy, cx, cy, _ = cam
    uc, vc = cx + fx * centre[0] / depth, cy + fy * centre[1] / depth
    hx, hy = 0.5 * size * fx / depth, 0.5 * size * fy / depth
    return (max(int(np.ceil(uc - hx)), 0), min(int(np.ceil(uc + hx)), W), max(int(np.ceil(vc - hy)), 0), min(int(np.ceil(vc + hy)), H))


def box_texture(h, w):
    """Grey levels [h,w] of the box, a function of the offset from its top-left corner, so that it moves with the box: a ramp of 12
    levels a column (a sawtooth of period 16 columns, which no box here reaches) with a ripple of period 3 down the rows."""
    i, j = np.arange(w)[None, :], np.arange(h)[:, None]
    return (40 + 12 * (i % 16) + 3 * (j % 3)).astype(np.uint8)


def mover_box(disp, grey, cam, centre, size, depth):
    """Pastes the box into disp float [H,W] and grey uint8 [H,W] (copies are returned) where it is the nearer surface; returns
    (disp, grey, inside bool [H,W]: the pixels the box took)."""
    H, W = disp.shape
    x0, x1, y0, y1 = box_rect(cam, centre, size, depth, H, W)
    d_box = cam[4] / depth
    inside = np.zeros((H, W), bool)
    inside[y0:y1, x0:x1] = True
    tex = np.zeros((H, W), np.uint8)
    tex[y0:y1, x0:x1] = box_texture(y1 - y0, x1 - x0)
    inside &= ~(disp > d_box)
    disp, grey = disp.copy(), grey.copy()
    disp[inside] = d_box
    grey[inside] = tex[inside]
    return disp, grey, inside


def scene_frame(k, H=48, W=96, box=None, noise=0.0, seed=0, dz=0.3, yaw=0.01):
    """Frame k of the drive forward_pose(k, dz, yaw) through the road-and-wall scene: (rgb uint8 [H,W,3], disp float32 [H,W], codes
    uint8 [H,W] as edge_codes gives them, the camera-to-world pose, inside bool [H,W]).  box = (centre, size, depth) or None; noise: the
    standard deviation in px of seeded Gaussian noise on the disparities of the pixels that see something."""
    cam = E.scene_cam(H, W)
    Tk = T.forward_pose(k, dz, yaw=yaw)
    d, g = T.render(Tk, H, W, cam), E.render_grey(Tk, H, W, cam)
    codes = E.edge_codes(d.astype(F))                       # the scene's own edges, where the anti-aliased grey mixes two surfaces; the
    inside = np.zeros((H, W), bool)                         # box is pasted with hard edges and mixes nothing
    if box is not None:
        d, g, inside = mover_box(d, g, cam, *box)
    if noise:
        rng = np.random.default_rng(seed + 1000 * k)
        d = np.where(d > 0, d + noise * rng.standard_normal(d.shape), d)
    return np.repeat(g[..., None], 3, -1), d.astype(F), codes, Tk, inside


def scene_pair(box_prev=None, box_cur=None, noise=0.0, seed=0, H=48, W=96, frames=(2, 3)):
    """The two frames as the arguments of segment(), batch 1: dict(rgb_prev, disp_prev, mask_prev, rgb_cur, disp_cur, mask_cur, cam,
    pose) with the true relative pose, and the box's pixels in the current frame."""
    r0, d0, c0, T0, _ = scene_frame(frames[0], H, W, box_prev, noise, seed)
    r1, d1, c1, T1, inside = scene_frame(frames[1], H, W, box_cur, noise, seed)
    cam = np.asarray(E.scene_cam(H, W), F)[None]
    args = dict(rgb_prev=r0[None], disp_prev=d0[None, None], mask_prev=c0[None, None], rgb_cur=r1[None], disp_cur=d1[None, None],
                mask_cur=c1[None, None], cam=cam, pose=T.relative(T0, T1)[None])
    return args, inside


# the four scenes of the segmentation tests: (the box in the previous frame, in the current one); a box of 12 x 12 px in the current frame
BOX = dict(approaching=(((0.0, 0.0), 0.32, 4.0), ((0.0, 0.0), 0.32, 3.2)),
           receding=(((0.0, 0.0), 0.4, 3.2), ((0.0, 0.0), 0.4, 4.0)),
           lateral=(((-0.15, 0.0), 0.4, 4.0), ((0.0, 0.0), 0.4, 4.0)))


# ---- hand-made inputs for the bit-for-bit tests ----
IDENTITY_POSE = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]] * 2, F)


def exact_cam(H, W):
    """A camera whose numbers keep the projection of the cases below exact: fx = fy = 128, half-integer cx, cy, fb = 64, so that a
    disparity of 8 is a depth of 8 and one of 16 a depth of 4."""
    return np.array([128.0, 128.0, (W - 1) / 2.0, (H - 1) / 2.0, 64.0], F)


def spiral(H, W, margin=2):
    """bool [H,W]: a one-pixel path that winds inwards from (margin, margin), clockwise, one free pixel between its laps."""
    m = np.zeros((H, W), bool)
    inside = lambda yy, xx: margin <= yy <= H - 1 - margin and margin <= xx <= W - 1 - margin
    y, x, k, turned = margin, margin, 0, 0
    m[y, x] = True
    while turned < 2:
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[k % 4]
        if inside(y + dy, x + dx) and not m[y + dy, x + dx] and not (inside(y + 2 * dy, x + 2 * dx) and m[y + 2 * dy, x + 2 * dx]):
            y, x, turned = y + dy, x + dx, 0
            m[y, x] = True
        else:
            k, turned = k + 1, turned + 1
    return m


def pattern_case(want, near=None, seed=0):
    """The arguments of segment() (batch 1) for which the evidence of pixel p is want[p] (uint8 [H,W], codes 0..4) under the identity
    motion and exact_cam: the current disparity is 8 (16 where `near`, bool [H,W], says so), the previous one 6 less where a pixel
    is to have appeared and 6 more where it is to be uncovered, the current grey 80 levels above the previous one where it is to
    have changed, and mask_cur 0 where it is to stay untested.  A pixel on the image's border cannot come out as changed: the
    photometric test is off there."""
    H, W = want.shape
    rng = np.random.default_rng(seed)
    d_cur = np.where(near if near is not None else np.zeros((H, W), bool), F(16), F(8)).astype(F)
    d_prev = (d_cur + np.where(want == APPEARED, F(-6), np.where(want == UNCOVERED, F(6), F(0)))).astype(F)
    g0 = rng.integers(40, 120, (H, W)).astype(np.uint8)
    g1 = (g0 + np.where(want == CHANGED, 80, 0)).astype(np.uint8)
    rgb = lambda g: np.repeat(g[..., None], 3, -1)[None]
    return dict(rgb_prev=rgb(g0), disp_prev=d_prev[None, None], mask_prev=None, rgb_cur=rgb(g1), disp_cur=d_cur[None, None],
                mask_cur=(want != UNTESTED).astype(np.uint8)[None, None], cam=exact_cam(H, W)[None], pose=IDENTITY_POSE[None].copy())


def shift_case(H, W, sx, sy, seed=0):
    """As pattern_case with every pixel at disparity 8 and a motion that moves the projection by exactly (sx, sy) pixels (multiples
    of 1/8): u = x + sx, v = y + sy in float32 without a rounding.  The previous frame and the greys are random, so every code occurs."""
    rng = np.random.default_rng(seed)
    cam = exact_cam(H, W)
    pose = IDENTITY_POSE.copy()
    pose[1, 3], pose[1, 7] = sx * 8.0 / 128.0, sy * 8.0 / 128.0      # X + tx projects to x + fx * tx / z
    pose[0, 3], pose[0, 7] = -pose[1, 3], -pose[1, 7]
    d_cur = np.full((H, W), 8, F)
    d_prev = (8 + rng.choice([0.0, 0.0, -6.0, 6.0, 1.5], (H, W))).astype(F)
    g0, g1 = (rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2))
    return dict(rgb_prev=g0[None], disp_prev=d_prev[None, None], mask_prev=None, rgb_cur=g1[None], disp_cur=d_cur[None, None], mask_cur=None,
                cam=cam[None], pose=pose[None])


def messy_case(H, W, seed=0, specials=True, tz=0.0, yaw=0.02):
    """Arguments with nothing exact about them: smooth disparities with steps and noise, sigma maps, random masks, a small motion
    (tz metres along the axis, yaw radians), and -- with specials -- NaN, +-inf, 0, values below min_disp and huge ones sprinkled over
    both disparity maps and both sigma maps (NaN, inf, negative)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    base = 6.0 + 0.04 * xs + 0.08 * ys + 5.0 * ((xs // 11 + ys // 7) % 3 == 0)
    d_prev = (base + 0.3 * rng.standard_normal((H, W))).astype(F)
    d_cur = (base + 0.3 * rng.standard_normal((H, W)) + 4.0 * (rng.random((H, W)) < 0.15) * rng.choice([-1.0, 1.0], (H, W))).astype(F)
    s_prev, s_cur = ((0.2 + 0.6 * rng.random((H, W))).astype(F) for _ in range(2))
    if specials:
        for a, vals in ((d_prev, (np.nan, np.inf, -np.inf, 0.0, 0.4, 1e30)), (d_cur, (np.nan, np.inf, -np.inf, 0.0, 0.4, 1e30)),
                        (s_prev, (np.nan, np.inf, -0.1, 0.0, 1e30)), (s_cur, (np.nan, np.inf, -0.1, 0.0, 1e30))):
            hit = rng.random((H, W)) < 0.06
            a[hit] = rng.choice(np.array(vals, F), int(hit.sum()))
    m_prev, m_cur = ((rng.random((H, W)) < 0.9).astype(np.uint8) * rng.choice([1, 1, 1, 3], (H, W)).astype(np.uint8) for _ in range(2))
    g0 = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    g1 = np.clip(g0.astype(np.int64) + rng.integers(-12, 13, (H, W, 3)) + 90 * (rng.random((H, W, 1)) < 0.1), 0, 255).astype(np.uint8)
    f = max(1.25 * W, 8.0)
    cam = np.array([f, f, (W - 1) / 2.0 + 0.3, 0.4 * (H - 1), 0.5 * f], F)
    pose = T.relative(T.forward_pose(0, 0.0), T.forward_pose(1, tz, yaw=yaw, dx=0.02))
    return dict(rgb_prev=g0[None], disp_prev=d_prev[None, None], sigma_prev=s_prev[None, None], mask_prev=m_prev[None, None], rgb_cur=g1[None],
                disp_cur=d_cur[None, None], sigma_cur=s_cur[None, None], mask_cur=m_cur[None, None], cam=cam[None], pose=pose[None])


def stack_cases(cases):
    """Cases of one shape as one batch; a map that some cases lack (None) must be lacking in all."""
    out = {}
    for k in cases[0]:
        vals = [c.get(k) for c in cases]
        assert all(v is None for v in vals) or all(v is not None for v in vals), k
        out[k] = None if vals[0] is None else np.concatenate(vals)
    return out


def run_case(case, **kw):
    """segment() on a case's dictionary."""
    c = dict(case)
    return segment(c.pop("rgb_prev"), c.pop("disp_prev"), c.pop("rgb_cur"), c.pop("disp_cur"), c.pop("cam"), c.pop("pose"), **c, **kw)
