"""lws_ego_normal and lws_egomotion on the device against the numpy restatement (tests/egomotion_reference.py): the per-pixel terms
and the final residual bit for bit, the pixel count exactly, the 29 sums to the rounding of two orders of summation, every traced
Gauss-Newton step to the conditioning of its own matrix.  The shapes of lws_ego_normal start below the 4 x 4 a level needs, pass
the quad, the wave and the 1024-pixel tile of a workgroup; five motions (identity, forward, a yaw with a lateral step, a drive through
the wall that puts points behind the camera, a turn that takes the scene out of view) meet three kinds of input (the scene, uniform
noise, images and maps sprinkled with NaN, +-inf, -0.0 and 1e30), mask given or not.  Then: views one element past a 16-byte
boundary, poisoned guard bands, batch independence, a captured graph, a singular case, identical frames, the pose block against the
last M that a run one step longer traces, Odometry feeding TemporalFilter, the CLI against the ops composed by hand."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import egomotion_reference as E
import guarded
import temporal_reference as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_egomotion_cpu import MAX_COND, MOTIONS as SCENE_MOTIONS, SIZES, bound, scene_case  # noqa: E402
from test_gpu_geometry import KITTI15_CALIB, cam_rows, cu, misaligned  # noqa: E402

F = np.float32
HS, WS, BS, LEVELS = (1, 3, 4, 5, 17), (1, 3, 4, 5, 63, 64, 65, 257), (1, 2), (0, 2)
KINDS = ("scene", "uniform", "special")
# camera-to-world pose of the current frame (the reference frame is the identity): dz, yaw, dx
MOTIONS = {"identity": (0.0, 0.0, 0.0), "forward": (0.5, 0.0, 0.0), "yaw_and_step": (0.3, 0.05, 0.2), "through": (15.0, 0.0, 0.0),
           "out_of_view": (0.2, 0.6, 3.0)}
MIN_DISP, HUBER = 0.5, 4.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, hip_lib):
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    return LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()


def level_camera(H, W, level):
    """(the full-resolution Camera whose level-`level` camera views the scene at H x W, that level camera as a tuple)."""
    from lwsnet_amd.geometry import Camera
    f, cx, cy = max(1.25 * W, 8.0), (W - 1) / 2.0, 0.4 * (H - 1)
    s = 2.0 ** level
    full = Camera(f * s, f * s, (cx + 0.5) * s - 0.5, (cy + 0.5) * s - 0.5, 0.5 / s)      # fb = f * 0.5 at every level
    return full, (f, f, cx, cy, f * 0.5)


def images(kind, H, W, cam_l, pose, rng):
    """(grey float32 [H,W], disparity float32 [H,W]) of `kind` seen from the camera-to-world `pose`."""
    if kind == "uniform":
        return rng.uniform(0.0, 255.0, (H, W)).astype(F), rng.uniform(0.3, 40.0, (H, W)).astype(F)
    g = E.render_grey(pose, H, W, cam_l, ss=2).astype(F) + rng.uniform(-3.0, 3.0, (H, W)).astype(F)
    d = T.render(pose, H, W, cam_l).astype(F)
    if kind == "special":
        special = np.array([np.nan, np.inf, -np.inf, -0.0, 1e30, -3.0], F)
        for a in (g, d):
            flat = a.reshape(-1)
            idx = rng.choice(flat.size, size=max(1, flat.size // 8), replace=False)
            flat[idx] = special[np.arange(len(idx)) % len(special)]
    return g, d


_WANT = {}


def normal_cases(H, W, B):
    """Per (level, motion): the inputs of the case and its restatement, computed once."""
    if (H, W, B) not in _WANT:
        out = []
        for level, (i, motion) in itertools.product(LEVELS, enumerate(MOTIONS)):
            rng = np.random.default_rng(1000 * H + 10 * W + B + 7 * i + level)
            kind = KINDS[(i + H + W + B + level) % len(KINDS)]
            with_mask = (i + W + level) % 2 == 0
            full, cam_l = level_camera(H, W, level)
            names = list(MOTIONS)
            g0, d0, g1, M = np.empty((B, 1, H, W), F), np.empty((B, 1, H, W), F), np.empty((B, 1, H, W), F), np.empty((B, 12))
            for b in range(B):
                dz, yaw, dx = MOTIONS[names[(i + b) % len(names)]]
                T0, T1 = T.forward_pose(0, 0.0), T.forward_pose(1, dz, yaw, dx)
                g0[b, 0], d0[b, 0] = images(kind, H, W, cam_l, T0, rng)
                g1[b, 0], _ = images(kind, H, W, cam_l, T1, rng)
                M[b] = E.true_motion(T0, T1) + rng.normal(0, 1e-3, 12)          # near the truth, not at it
            mask = rng.choice(np.array([0, 1, 1, 1, 2], np.uint8), size=(B, 1, H, W)) if with_mask else None
            rows = cam_rows([full] * B)
            sums, terms, mags = E.normal(g0, d0, mask, g1, rows, M, level, MIN_DISP, HUBER)
            reasons = [E.normal_image(g0[b, 0], d0[b, 0], mask[b, 0] == 1 if with_mask else np.ones((H, W), bool), g1[b, 0], rows[b], M[b], level,
                                      MIN_DISP, HUBER)[2] for b in range(B)]
            out.append(dict(level=level, motion=motion, kind=kind, cams=[full] * B, rows=rows, g0=g0, d0=d0, g1=g1, mask=mask, M=M, sums=sums,
                            terms=terms, mags=mags, reasons=reasons))
        _WANT[(H, W, B)] = out
    return _WANT[(H, W, B)]


def check_sums(got, want, mags, what):
    """The count exactly, every other sum within (n + 64) 2^-53 sum|term| of the restatement's float64 sum."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, got.dtype)
    assert (got[..., 28] == want[..., 28]).all(), (what, got[..., 28], want[..., 28])
    allowed = E.sum_bound(want[..., 28:29], mags)
    worst = np.abs(got - want) - allowed
    assert (worst[..., :28] <= 0).all(), (what, int(np.argmax(worst[..., :28])), float(worst[..., :28].max()))


@pytest.mark.parametrize("H,W,B", list(itertools.product(HS, WS, BS)))
def test_ego_normal_terms_bitexact_and_sums_to_rounding(dev, hip_lib, H, W, B):
    from lwsnet_amd import ops
    for c in normal_cases(H, W, B):
        what = f"B={B} {H}x{W} level {c['level']} {c['motion']} {c['kind']} mask={c['mask'] is not None}"
        sums, terms = ops.ego_normal(cu(c["g0"], dev), cu(c["d0"], dev), cu(c["g1"], dev), c["cams"], c["M"], level=c["level"],
                                     mask=None if c["mask"] is None else cu(c["mask"], dev), min_disp=MIN_DISP, huber=HUBER, terms=True)
        guarded.assert_bits(terms, c["terms"], what + " terms")
        check_sums(sums, c["sums"], c["mags"], what)
        none, no_terms = ops.ego_normal(cu(c["g0"], dev), cu(c["d0"], dev), cu(c["g1"], dev), c["cams"], c["M"], level=c["level"],
                                        mask=None if c["mask"] is None else cu(c["mask"], dev), min_disp=MIN_DISP, huber=HUBER)
        assert no_terms is None
        guarded.assert_bits(none, sums.cpu().numpy(), what + " sums without terms")     # the same bytes on every run


def test_the_cases_reach_every_branch():
    """Over all the cases above (their restatements; computed here where that test did not run): both Huber branches and the
    out-of-range, behind-camera and non-finite exclusions each occur, and so do used pixels under every kind of input."""
    seen = dict(inlier=0, outlier=0, invalid=0, behind=0, outside=0, nonfinite=0)
    used = {k: 0 for k in KINDS}
    for H, W, B in itertools.product(HS, WS, BS):
        for c in normal_cases(H, W, B):
            t = c["terms"]
            seen["inlier"] += int((t[..., 1] == 1).sum())
            seen["outlier"] += int(((t[..., 1] > 0) & (t[..., 1] < 1)).sum())
            used[c["kind"]] += int(c["sums"][:, 28].sum())
            for r in c["reasons"]:
                for k in ("invalid", "behind", "outside", "nonfinite"):
                    seen[k] += int(r[k].sum())
    print("pixels per branch over all cases:", seen, "used per kind:", used)
    assert all(v > 0 for v in seen.values()) and all(v > 0 for v in used.values())


# ---- the whole estimate ----
def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


EGO_KW = dict(min_disp=0.5, max_jump=1.0, huber=10.0, damping=0.0, min_pixels=64)


def raw_egomotion(lib, dev, b, shape, levels, iters, kw=EGO_KW):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_egomotion(P(b["rgb_ref"]), P(b["disp_ref"]), P(b.get("mask")), P(b["rgb_cur"]), P(b["cam"]), P(b.get("init")), *shape,
                                     levels, iters, kw["min_disp"], kw["max_jump"], kw["huber"], kw["damping"], kw["min_pixels"], P(b["work"]),
                                     P(b["pose"]), P(b["status"]), P(b["info"]), P(b.get("trace")), P(b.get("resid")),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "lws_egomotion")


def batch_case(H, W, B, first="forward"):
    """B images of the scene at H x W, image b moving by the motion b places behind `first` in the CPU test's list, with the
    restatement's estimate of each (shared with tests/test_egomotion_cpu.py)."""
    names = [m for m in SCENE_MOTIONS if m != "identity"]
    cs = [scene_case(H, W, names[(names.index(first) + b) % len(names)]) for b in range(B)]
    stack = lambda k: np.stack([c[k] for c in cs])          # noqa: E731
    return dict(cs=cs, motions=[names[(names.index(first) + b) % len(names)] for b in range(B)], rgb_ref=stack("rgb0"),
                disp_ref=stack("d0")[:, None], mask=stack("mask")[:, None], rgb_cur=stack("rgb1"), cam=stack("cam"))


def output_buffers(dev, B, H, W, levels, iters, lib):
    return dict(work=torch.empty((lib.lws_egomotion_workspace(B, H, W, levels),), dtype=torch.uint8, device=dev),
                pose=torch.empty((B, 2, 12), dtype=torch.float32, device=dev), status=torch.empty((B,), dtype=torch.int32, device=dev),
                info=torch.empty((B, 4), dtype=torch.float64, device=dev), trace=torch.empty((B, levels * iters, 48), dtype=torch.float64, device=dev),
                resid=torch.empty((B, 1, H, W), dtype=torch.float32, device=dev))


def check_estimate(c, got, levels, iters, what, init=None):
    """Holds one call's outputs (numpy) to the restatement, image by image."""
    pose, status, info, trace, resid = got
    B, _, H, W = c["disp_ref"].shape
    for b in range(B):
        ok = c["mask"][b, 0] == 1 if c.get("mask") is not None else np.ones((H, W), bool)
        pyr = E.pyramids(c["rgb_ref"][b], c["disp_ref"][b, 0], ok, c["rgb_cur"][b], levels, EGO_KW["min_disp"], EGO_KW["max_jump"])
        tr = trace[b]
        M0 = E.IDENTITY12 if init is None else np.asarray(init[b], F).astype(np.float64)
        assert (tr[0, :12] == M0).all(), what
        st, steps, last, nxt = 0, 0, 0.0, None
        for s in range(levels * iters):
            level = levels - 1 - s // iters
            g0, d, o, g1 = pyr[level]
            M, sums, delta, code = tr[s, :12], tr[s, 12:41], tr[s, 41:47], int(tr[s, 47])
            terms, use, _ = E.normal_image(g0, d, o, g1, c["cam"][b], M, level, EGO_KW["min_disp"], EGO_KW["huber"])
            want, mag = E.sums_of(terms, use)
            check_sums(sums[None], want[None], mag[None], f"{what} image {b} step {s}")
            new, wd, wcode = E.update(sums, M, EGO_KW["damping"], EGO_KW["min_pixels"])
            assert code == wcode, (what, b, s, code, wcode)
            st |= code
            nxt = tr[s + 1, :12] if s + 1 < levels * iters else None
            if code != 0:
                assert nxt is None or (nxt == M).all(), (what, b, s)
                continue
            cond = np.linalg.cond(E.unpack(sums)[0])
            assert cond < MAX_COND, (what, b, s, cond)
            tol = 64 * cond * 2.0 ** -52
            assert np.abs(delta - wd).max() <= tol * np.abs(wd).max(), (what, b, s, delta, wd)
            if nxt is not None:
                assert np.abs(nxt - new).max() <= tol * np.abs(new).max(), (what, b, s, np.abs(nxt - new).max(), tol)
            steps, last, final_ref, final_tol = steps + 1, float(np.sqrt((delta * delta).sum())), new, tol * np.abs(new).max()
        # the pose block: the float32 rounding of the last M, which lies within the last step's tolerance of the restatement's
        if int(tr[-1, 47]) == 0:
            half_ulp = np.spacing(np.abs(final_ref).astype(F)).astype(np.float64) / 2
            assert (np.abs(pose[b, 0].astype(np.float64) - final_ref) <= final_tol + half_ulp).all(), (what, b)
        else:                                               # the last step was refused: the last M is the traced one
            guarded.assert_bits(pose[b, 0], tr[-1, :12].astype(F), f"{what} image {b} pose[0]")
            guarded.assert_bits(pose[b, 1], E.inverse12(tr[-1, :12]).astype(F), f"{what} image {b} pose[1]")
        Mf = pose[b, 0].astype(np.float64)
        assert np.abs(pose[b, 1].astype(np.float64) - E.inverse12(Mf)).max() <= 2.0 ** -22 * max(1.0, np.abs(Mf).max()), (what, b)
        # float32(M) is all the final linearisation sees of M: resid bit for bit, n exactly, the rms to rounding
        terms, use, _ = E.normal_image(*pyr[0], c["cam"][b], Mf, 0, EGO_KW["min_disp"], EGO_KW["huber"])
        guarded.assert_bits(resid[b, 0], terms[..., 0], f"{what} image {b} resid")
        fs, fm = E.sums_of(terms, use)
        assert info[b, 0] == fs[28] and info[b, 3] == steps and abs(info[b, 2] - last) <= 1e-12 * max(last, 1e-30), (what, b, info[b], steps, last)
        rms = np.sqrt(fs[27] / fs[28]) if fs[28] > 0 else 0.0
        assert abs(info[b, 1] - rms) <= 1e-12 * max(rms, 1e-30), (what, b)
        assert status[b] == (st | (E.BIT_FINAL_FEW if fs[28] < EGO_KW["min_pixels"] else 0)), (what, b, status[b], st)


def run_estimate(lib, dev, c, levels, iters, init=None):
    B, _, H, W = c["disp_ref"].shape
    b = {k: cu(c[k], dev) for k in ("rgb_ref", "disp_ref", "mask", "rgb_cur", "cam")}
    if init is not None:
        b["init"] = cu(np.asarray(init, F), dev)
    b.update(output_buffers(dev, B, H, W, levels, iters, lib))
    raw_egomotion(lib, dev, b, (B, H, W), levels, iters)
    torch.cuda.synchronize(dev)
    return tuple(b[k].cpu().numpy() for k in ("pose", "status", "info", "trace", "resid"))


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("H,W", list(SIZES))
def test_egomotion_traced_steps_and_final_outputs(dev, hip_lib, H, W, B):
    levels, iters = SIZES[(H, W)], 8
    c = batch_case(H, W, B)
    got = run_estimate(hip_lib, dev, c, levels, iters)
    check_estimate(c, got, levels, iters, f"B={B} {H}x{W}")
    for b, motion in enumerate(c["motions"]):               # the CPU test's bound to the true motion
        et, er = E.motion_error(got[0][b, 0].astype(np.float64), c["cs"][b]["true"])
        print(f"{H}x{W} image {b} {motion}: error {et:.5f} m, {er:.4f} deg, status {got[1][b]}, info {got[2][b].tolist()}")
        bt, br = bound(H, W, motion)
        assert et <= bt and er <= br and got[1][b] & ~E.BIT_SMALL == 0


@pytest.mark.parametrize("H,W,k", [(48, 96, 5), (96, 192, 3)])
def test_the_pose_block_is_the_float32_rounding_of_the_last_M_and_of_its_double_inverse(dev, hip_lib, H, W, k):
    """The last M of a call is not among its outputs, but the call is deterministic: with one level, the run with k + 1 steps repeats
    the run with k steps and then traces, as M before step k, the M the shorter run ended with.  The shorter run's pose block is
    held to the float32 rounding of that double M and of its inverse formed in double, on bytes; every step is a step taken, so M
    is a double no float32 holds."""
    B = 2
    c = batch_case(H, W, B, "far")
    short, longer = run_estimate(hip_lib, dev, c, 1, k), run_estimate(hip_lib, dev, c, 1, k + 1)
    assert np.array_equal(guarded.as_bits(short[3]), guarded.as_bits(longer[3][:, :k])), "the first k steps of the two runs"
    assert (short[3][:, :, 47] == 0).all() and (longer[3][:, :, 47] == 0).all()
    last = longer[3][:, k, :12]
    assert (last.astype(F).astype(np.float64) != last).any(axis=1).all()
    guarded.assert_bits(short[0][:, 0], last.astype(F), "pose[0]")
    guarded.assert_bits(short[0][:, 1], np.stack([E.inverse12(m) for m in last]).astype(F), "pose[1]")
    # and it is not what an inverse formed from the rounded M, or in float32, would give
    rounded = np.stack([E.inverse12(m.astype(F).astype(np.float64)) for m in last]).astype(F)
    print(f"{H}x{W}: entries of pose[1] that an inverse of the float32 M would get wrong: {int((rounded != short[0][:, 1]).sum())} of {rounded.size}")


@pytest.mark.parametrize("H,W", list(SIZES))
def test_identical_frames_give_the_identity_in_bits(dev, hip_lib, H, W):
    """The same frame twice: every step is below the pose's float32 resolution (code 16) and is not taken, its delta is traced as
    it was solved, and the pose block is the identity and its inverse, in bits."""
    levels, iters = SIZES[(H, W)], 4
    s = scene_case(H, W, "identity")
    assert np.array_equal(s["rgb0"], s["rgb1"])
    c = dict(rgb_ref=s["rgb0"][None], disp_ref=s["d0"][None, None], mask=s["mask"][None, None], rgb_cur=s["rgb1"][None], cam=s["cam"][None])
    pose, status, info, trace, resid = got = run_estimate(hip_lib, dev, c, levels, iters)
    check_estimate(c, got, levels, iters, f"identity {H}x{W}")
    assert (trace[0, :, 47] == E.BIT_SMALL).all() and status[0] == E.BIT_SMALL and info[0, 2] == 0 and info[0, 3] == 0
    d2 = (trace[0, :, 41:47] ** 2).sum(axis=1)
    print(f"{H}x{W}: |delta| of the steps not taken: {np.sqrt(d2.min()):.3g} .. {np.sqrt(d2.max()):.3g} (the floor is {2.0 ** -23:.3g})")
    assert (d2 > 0).all() and (d2 < E.MIN_STEP2).all()
    guarded.assert_bits(pose[0], np.stack([E.IDENTITY12, E.IDENTITY12]).astype(F), "pose")
    assert np.abs(resid).max() < 1e-3 and info[0, 0] > 0.4 * H * W


def test_init_is_kept_where_no_step_is_taken_and_the_inverse_is_formed_in_double(dev, hip_lib):
    """min_pixels above the pixel count: every step has code 1, so M is init throughout, and the pose block is init and the float32
    rounding of its inverse formed in double, bit for bit."""
    H, W, B = 48, 96, 2
    c = batch_case(H, W, B)
    rng = np.random.default_rng(2)
    init = np.stack([E.compose(E.exp_se3(rng.normal(size=6) * 0.2), E.IDENTITY12) for _ in range(B)]).astype(F)
    b = {k: cu(c[k], dev) for k in ("rgb_ref", "disp_ref", "mask", "rgb_cur", "cam")}
    b.update(output_buffers(dev, B, H, W, 2, 3, hip_lib), init=cu(init, dev))
    raw_egomotion(hip_lib, dev, b, (B, H, W), 2, 3, {**EGO_KW, "min_pixels": H * W + 1})
    guarded.assert_bits(b["pose"][:, 0], init, "pose[0]")
    guarded.assert_bits(b["pose"][:, 1], np.stack([E.inverse12(m.astype(np.float64)) for m in init]).astype(F), "pose[1]")
    assert (b["status"].cpu().numpy() == E.BIT_FEW | E.BIT_FINAL_FEW).all() and (b["trace"].cpu().numpy()[:, :, 47] == E.BIT_FEW).all()
    assert (b["info"].cpu().numpy()[:, 2:] == 0).all()


def test_constant_images_are_singular_and_keep_init(dev, hip_lib):
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import Camera
    H, W, B = 24, 48, 2
    rgb = torch.full((B, H, W, 3), 100, dtype=torch.uint8, device=dev)
    disp = torch.full((B, 1, H, W), 6.0, dtype=torch.float32, device=dev)
    init = np.stack([E.IDENTITY12, E.compose(E.exp_se3(np.array([0.1, 0, -0.2, 0, 0.01, 0])), E.IDENTITY12)]).astype(F)
    res = ops.egomotion(rgb, disp, rgb.clone(), Camera(*T.SCENE_CAM[:4], 0.5), init=cu(init, dev), levels=2, iters=3, min_disp=0.5, min_pixels=16,
                        trace=True, resid=True)
    assert (res.status.cpu().numpy() == E.BIT_SINGULAR).all() and (res.trace.cpu().numpy()[:, :, 47] == E.BIT_SINGULAR).all()
    guarded.assert_bits(res.pose[:, 0], init, "pose[0]")
    assert (res.resid == 0).all() and (res.info[:, 0] > 16).all() and (res.info[:, 1:] == 0).all()


# ---- call hygiene ----
def test_one_element_past_a_16_byte_boundary(dev, hip_lib):
    H, W, B, levels, iters = 48, 96, 2, 2, 2
    c = batch_case(H, W, B, "far")
    want = run_estimate(hip_lib, dev, c, levels, iters)
    check_estimate(c, want, levels, iters, "aligned")
    b = {k: misaligned(c[k], dev) for k in ("rgb_ref", "disp_ref", "mask", "rgb_cur", "cam")}
    out = output_buffers(dev, B, H, W, levels, iters, hip_lib)
    b.update(work=out["work"], pose=misaligned(np.zeros((B, 2, 12), F), dev), status=misaligned(np.zeros((B,), np.int32), dev), info=out["info"],
             trace=out["trace"], resid=misaligned(np.zeros((B, 1, H, W), F), dev))
    raw_egomotion(hip_lib, dev, b, (B, H, W), levels, iters)
    for k, w in zip(("pose", "status", "info", "trace", "resid"), want):
        guarded.assert_bits(b[k], w, f"misaligned {k}")      # the same bytes as from aligned memory
    # lws_ego_normal
    n = normal_cases(17, 65, 2)[2]
    from lwsnet_amd import _lib
    sums, terms = torch.empty((2, 29), dtype=torch.float64, device=dev), misaligned(np.zeros((2, 17, 65, 8), F), dev)
    work = torch.empty((hip_lib.lws_egomotion_workspace(2, 17, 65, 1),), dtype=torch.uint8, device=dev)
    nb = {k: misaligned(n[k], dev) for k in ("g0", "d0", "g1", "rows")}         # (held here until the call has run)
    nb.update(mask=None if n["mask"] is None else misaligned(n["mask"], dev), M=cu(n["M"], dev))
    with torch.cuda.device(dev):
        _lib.check(hip_lib.lws_ego_normal(P(nb["g0"]), P(nb["d0"]), P(nb["mask"]), P(nb["g1"]), P(nb["rows"]), P(nb["M"]), 2, 17, 65, n["level"], MIN_DISP,
                                          HUBER, P(work), P(sums), P(terms), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "lws_ego_normal")
    guarded.assert_bits(terms, n["terms"], "misaligned terms")
    check_sums(sums, n["sums"], n["mags"], "misaligned sums")


@pytest.mark.parametrize("word", guarded.FLOAT_WORDS, ids=guarded.word_id)
def test_memory_contract(dev, hip_lib, word):
    """Inputs, outputs and the workspace between poisoned flanks, the outputs and the workspace poisoned inside: no flank changes,
    every output element is written, and the bytes are those of a call on plain memory.  17 x 65 at three levels: a level of 4 x 16
    with a last tile of a few pixels; 2 images."""
    from lwsnet_amd import _lib
    B, H, W, levels, iters = 2, 17, 65, 3, 2
    rng = np.random.default_rng(11)
    full, cam_l = level_camera(H, W, 0)
    T0, T1 = T.forward_pose(0, 0.0), T.forward_pose(1, 0.3, 0.01)
    g = [np.stack([np.repeat(np.clip(images("scene", H, W, cam_l, t, rng)[0], 0, 255).astype(np.uint8)[..., None], 3, -1) for _ in range(B)]) for t in (T0, T1)]
    d = np.stack([images("special", H, W, cam_l, T0, rng)[1] for _ in range(B)])[:, None]
    mask = rng.choice(np.array([0, 1, 1, 1, 2], np.uint8), size=(B, 1, H, W))
    c = dict(rgb_ref=g[0], disp_ref=d, mask=mask, rgb_cur=g[1], cam=cam_rows([full] * B))
    kw = {**EGO_KW, "min_pixels": 16}
    plain = {k: cu(v, dev) for k, v in c.items()}
    plain.update(output_buffers(dev, B, H, W, levels, iters, hip_lib))
    raw_egomotion(hip_lib, dev, plain, (B, H, W), levels, iters, kw)
    assert (plain["trace"].cpu().numpy()[:, :, 47] == 0).any() and np.isfinite(plain["info"].cpu().numpy()).all()
    gd = guarded.Guard(dev, word, skew=1)
    b = dict(rgb_ref=gd.place(c["rgb_ref"], plane=3 * H * W, name="rgb_ref"), disp_ref=gd.place(c["disp_ref"], name="disp_ref"),
             mask=gd.place(c["mask"], word=guarded.MASK_WORD, name="mask"), rgb_cur=gd.place(c["rgb_cur"], plane=3 * H * W, name="rgb_cur"),
             cam=gd.place(c["cam"], name="cam"),
             work=gd.empty((hip_lib.lws_egomotion_workspace(B, H, W, levels),), np.uint8, align16=True, word=gd.word, name="workspace"),
             pose=gd.empty((B, 2, 12), F, name="pose"), status=gd.empty((B,), np.int32, name="status"),
             info=gd.empty((B, 4), np.float64, align16=True, name="info"), trace=gd.empty((B, levels * iters, 48), np.float64, align16=True, name="trace"),
             resid=gd.empty((B, 1, H, W), F, name="resid"))
    raw_egomotion(hip_lib, dev, b, (B, H, W), levels, iters, kw)
    for k in ("pose", "status", "info", "trace", "resid"):
        guarded.assert_bits(b[k], plain[k].cpu().numpy(), f"guarded {k}")
    gd.check()
    # lws_ego_normal the same way
    n = normal_cases(17, 65, 2)[1]
    gn = guarded.Guard(dev, word, skew=1)
    nb = dict(g0=gn.place(n["g0"], name="grey_ref"), d0=gn.place(n["d0"], name="disp_ref"), g1=gn.place(n["g1"], name="grey_cur"),
              mask=None if n["mask"] is None else gn.place(n["mask"], word=guarded.MASK_WORD, name="mask"), cam=gn.place(n["rows"], name="cam"),
              M=gn.place(n["M"], align16=True, name="M"), work=gn.empty((hip_lib.lws_egomotion_workspace(2, 17, 65, 1),), np.uint8, align16=True, word=gn.word, name="workspace"),
              sums=gn.empty((2, 29), np.float64, align16=True, name="sums"), terms=gn.empty((2, 17, 65, 8), F, plane=8 * 17 * 65, name="terms"))
    with torch.cuda.device(dev):
        _lib.check(hip_lib.lws_ego_normal(P(nb["g0"]), P(nb["d0"]), P(nb["mask"]), P(nb["g1"]), P(nb["cam"]), P(nb["M"]), 2, 17, 65, n["level"], MIN_DISP, HUBER,
                                          P(nb["work"]), P(nb["sums"]), P(nb["terms"]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "lws_ego_normal")
    guarded.assert_bits(nb["terms"], n["terms"], "guarded terms")
    check_sums(nb["sums"], n["sums"], n["mags"], "guarded sums")
    gn.check()


def test_batch_independence(dev, hip_lib):
    """The same image alone, first of two and second of two gives the same bytes, in every output."""
    H, W, levels, iters = 48, 96, 2, 4
    c = batch_case(H, W, 2)

    def run(order):
        idx = list(order)
        return run_estimate(hip_lib, dev, {k: np.ascontiguousarray(c[k][idx]) for k in ("rgb_ref", "disp_ref", "mask", "rgb_cur", "cam")}, levels, iters)

    both, swapped, alone = run((0, 1)), run((1, 0)), run((1,))
    for g, s, a, key in zip(both, swapped, alone, ("pose", "status", "info", "trace", "resid")):
        bits = guarded.as_bits(g[1])
        assert np.array_equal(bits, guarded.as_bits(s[0])) and np.array_equal(bits, guarded.as_bits(a[0])), key
    again = run((0, 1))
    for g, a, key in zip(both, again, ("pose", "status", "info", "trace", "resid")):
        assert np.array_equal(guarded.as_bits(g), guarded.as_bits(a)), key      # and on every run


def test_graph_capture_replays_on_two_input_sets(dev, hip_lib):
    H, W, B, levels, iters = 48, 96, 2, 2, 3
    first, second = batch_case(H, W, B, "forward"), batch_case(H, W, B, "yaw")
    keys = ("rgb_ref", "disp_ref", "mask", "rgb_cur")
    want = {id(c): run_estimate(hip_lib, dev, c, levels, iters) for c in (first, second)}
    b = {k: cu(first[k], dev) for k in keys + ("cam",)}
    b.update(output_buffers(dev, B, H, W, levels, iters, hip_lib))
    raw_egomotion(hip_lib, dev, b, (B, H, W), levels, iters)     # the code object is loaded before the capture
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_egomotion(hip_lib, dev, b, (B, H, W), levels, iters)
    for c in (first, second, first):
        for k in keys:
            b[k].copy_(cu(c[k], dev))
        for k in ("pose", "status", "info", "trace", "resid", "work"):
            b[k].fill_(77)
        graph.replay()
        torch.cuda.synchronize(dev)
        for k, w in zip(("pose", "status", "info", "trace", "resid"), want[id(c)]):
            guarded.assert_bits(b[k], w, f"replay {k}")


# ---- the state-holding class ----
def _sequence(n, H=48, W=96):
    poses = [T.forward_pose(k, 0.3, yaw=0.01) for k in range(n)]
    cam = E.scene_cam(H, W)
    rgb = [np.repeat(E.render_grey(p, H, W, cam)[..., None], 3, -1)[None] for p in poses]
    disp = [T.render(p, H, W, cam).astype(F)[None, None] for p in poses]
    mask = [E.edge_codes(d[0, 0])[None, None] for d in disp]
    return poses, rgb, disp, mask


def test_odometry_over_four_frames_feeding_the_filter(dev, hip_lib):
    from lwsnet_amd import egomotion, ops
    from lwsnet_amd.geometry import Camera
    from lwsnet_amd.temporal import TemporalFilter
    poses, rgb, disp, mask = _sequence(4)
    cam = Camera(120.0, 120.0, 47.5, 20.0, 0.5)
    kw = dict(levels=2, iters=6, min_disp=0.5, min_pixels=64)
    odo, filt = egomotion.Odometry(cam, **kw), TemporalFilter(cam, min_disp=0.5)
    prev_state, prev_pose, world = None, None, [np.hstack([np.eye(3), np.zeros((3, 1))])]
    for k in range(4):
        r, d, m = cu(rgb[k], dev), cu(disp[k], dev), cu(mask[k], dev)
        ego = odo.step(r, d, m)
        fused = filt.step(d, None if ego is None else ego.pose, mask=m)
        if k == 0:
            assert ego is None
            by_hand = ops.temporal_step(d, cam, mask=m, min_disp=0.5)
        else:
            want = ops.egomotion(cu(rgb[k - 1], dev), cu(disp[k - 1], dev), r, cam, mask=cu(mask[k - 1], dev), init=prev_pose, **kw)
            for g, w, key in zip(ego, want, ops.EgoResult._fields):
                assert (g is None and w is None) or np.array_equal(guarded.as_bits(g.cpu().numpy()), guarded.as_bits(w.cpu().numpy())), (k, key)
            by_hand = ops.temporal_step(d, cam, pose=want.pose, prev=prev_state, mask=m, min_disp=0.5)
            prev_pose = want.pose[:, 0].contiguous()
            world.append(egomotion.compose(world[-1], egomotion.invert(want.pose[0, 0].cpu().numpy().astype(np.float64).reshape(3, 4))))
            assert int(want.status[0]) & ~E.BIT_SMALL == 0
        for g, w, key in zip(fused, by_hand, ops.TemporalResult._fields):
            assert np.array_equal(guarded.as_bits(g.cpu().numpy()), guarded.as_bits(w.cpu().numpy())), (k, key)
        prev_state = tuple(t.clone() for t in by_hand[:3])
    got = odo.poses()
    assert got.shape == (4, 3, 4) and (got[0] == world[0]).all() and (got == np.stack(world)).all()
    assert (fused.code == 2).any()
    et, er = E.motion_error(got[3].reshape(12), np.vstack([poses[3]]).reshape(12))
    print(f"after three steps of 0.3 m: position error {et:.4f} m, rotation error {er:.4f} deg")
    assert et <= 3 * 0.2 * 0.3 and er <= 1.5                # three steps, each under a fifth of its length and half a degree


# ---- the CLI ----
def test_inference_cli_egomotion_files(dev, model, tmp_path):
    from PIL import Image
    from lwsnet_amd import imageio as io
    from lwsnet_amd import inference, ops, outputs, synth
    from lwsnet_amd import postprocess as post
    from lwsnet_amd.egomotion import compose, invert
    from lwsnet_amd.geometry import Camera, read_kitti_poses
    n = 3
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, n)
    calib = tmp_path / "calib.txt"
    calib.write_text(KITTI15_CALIB.format(fx=721.5377, cx=609.5593, cy=172.854, t3=44.85728 - 0.54 * 721.5377))
    out, pose_file = tmp_path / "out", tmp_path / "est_poses.txt"
    written = inference.main(["--img_path", root + "/", "--synthetic_weights", "--calib", str(calib), "--occ_check", "1", "--save_path", str(out),
                              "--egomotion", "--ego_levels", "3", "--ego_iters", "4", "--save_poses", str(pose_file), "--save_ego",
                              "--temporal", "--save_temporal"])
    stems = [f"{k:06d}_10" for k in range(n)]
    assert sorted(os.listdir(out)) == sorted(s + e for s in stems for e in (".png", "_occ.png", "_ego.png", "_tcode.png", "_tsigma.png"))
    assert len(written) == 5 * n + 1 and str(pose_file) in written
    opts = post.Options.make(occ_check=1.0)
    ego_kw = dict(levels=3, iters=4, huber=10.0, min_disp=1.0, max_jump=1.0, damping=0.0, min_pixels=256)     # the flags and Odometry's defaults
    prev_frame = prev_state = init = None
    world, trusted_frames = [np.hstack([np.eye(3), np.zeros((3, 1))])], 0
    for k, stem in enumerate(stems):
        full = io.load_rgb(os.path.join(root, "image_2", stem + ".png"))
        left = io.crop_bottom_right(full)
        l_in = io.to_input(left)[None]
        r_in = io.to_input(io.crop_bottom_right(io.load_rgb(os.path.join(root, "image_3", stem + ".png"))))[None]
        cam = Camera.from_kitti(str(calib)).crop_bottom_right(*full.shape[:2])
        res = post.run_chain(model, l_in, r_in, opts)
        rgb, d, keep = outputs.rgb_on_device(left, dev), res.disp[3].as_subclass(torch.Tensor), res.keep[3]
        ego, pose = None, None
        if prev_frame is not None:                          # ops.egomotion and ops.temporal_step composed by hand
            ego = ops.egomotion(prev_frame[0], prev_frame[1], rgb, cam, mask=prev_frame[2], init=init, resid=True, **ego_kw)
            trusted = not int(ego.status[0]) & ops.EGO_UNTRUSTED
            init = ego.pose[:, 0].contiguous() if trusted else None
            pose = ego.pose if trusted else None
            trusted_frames += int(trusted)
            m = ego.pose[0, 0].cpu().numpy().astype(np.float64).reshape(3, 4)
            world.append(compose(world[-1], invert(m)))
            print(f"frame {k}: status {int(ego.status[0])}, info {ego.info[0].cpu().tolist()}")
        fused = ops.temporal_step(d, cam, pose=pose, prev=prev_state if pose is not None else None, mask=keep)
        prev_frame, prev_state = (rgb.clone(), d.clone(), keep.clone()), tuple(t.clone() for t in fused[:3])
        want_ego = np.zeros(left.shape[:2], np.uint8) if ego is None else outputs.ego_to_u8(ego.resid[0, 0].cpu().numpy())
        assert np.array_equal(np.asarray(Image.open(out / (stem + "_ego.png"))), want_ego)
        assert np.array_equal(np.asarray(Image.open(out / (stem + ".png"))), io.disparity_to_color(fused.disp[0, 0].cpu().numpy()))
        assert np.array_equal(np.asarray(Image.open(out / (stem + "_tcode.png"))), outputs.temporal_to_rgb(fused.code[0, 0].cpu().numpy()))
    assert trusted_frames >= 1                              # the filter was fed an estimate at least once
    got = read_kitti_poses(str(pose_file))
    assert got.shape == (n, 3, 4) and (got[0] == world[0]).all() and (got == np.stack(world)).all()


# ---- the CLI's three sequence stages together, over four pairs of which pair 1 is skipped ----
@pytest.fixture(scope="module")
def gap_sequence(dev, model, tmp_path_factory):
    """(the CLI flags of a KITTI tree whose pair 1 is smaller than the crop, with its calibration and --occ_check 1; per processed pair
    its index, stem, left crop, camera and the chain's stage-4 map and `keep` codes), computed once."""
    from PIL import Image
    from lwsnet_amd import imageio as io, postprocess as post, synth
    from lwsnet_amd.geometry import Camera
    base = tmp_path_factory.mktemp("gap")
    root = str(base / "kitti")
    synth.write_kitti_tree(root, 4)
    for side in ("image_2", "image_3"):
        Image.fromarray(np.zeros((io.CROP_H - 1, io.CROP_W, 3), np.uint8)).save(os.path.join(root, side, "000001_10.png"))
    (base / "calib.txt").write_text(KITTI15_CALIB.format(fx=721.5377, cx=609.5593, cy=172.854, t3=44.85728 - 0.54 * 721.5377))
    frames = []
    for k, stem in ((k, f"{k:06d}_10") for k in (0, 2, 3)):
        full = io.load_rgb(os.path.join(root, "image_2", stem + ".png"))
        left = io.crop_bottom_right(full)
        r_in = io.to_input(io.crop_bottom_right(io.load_rgb(os.path.join(root, "image_3", stem + ".png"))))[None]
        res = post.run_chain(model, io.to_input(left)[None], r_in, post.Options.make(occ_check=1.0))
        cam = Camera.from_kitti(str(base / "calib.txt")).crop_bottom_right(*full.shape[:2])
        frames.append((k, stem, left, cam, res.disp[3].as_subclass(torch.Tensor).clone(), res.keep[3].clone()))
    return ["--img_path", root + "/", "--synthetic_weights", "--calib", str(base / "calib.txt"), "--occ_check", "1"], frames


def _by_hand(dev, frames, out, tmp, vol, hold, motion):
    """The filter and the volume composed by hand over `frames`, their files compared byte for byte with the CLI's in `out`.
    motion(k, rgb, d, keep) -> (the EgoResult or None, the filter's pose block or None, the camera-to-world pose [3,4]); the volume's
    frame is the first camera integrated.  Returns the voxels updated per frame."""
    from lwsnet_amd import imageio as io, ops, outputs
    from lwsnet_amd.temporal import TemporalFilter
    filt, first, updated, inf = None, None, [], float("inf")
    for k, stem, left, cam, d, keep in frames:
        filt = filt or TemporalFilter(cam, gate=3.0, q=0.0, sigma0=0.5, hold=hold, min_disp=1.0)
        rgb = outputs.rgb_on_device(left, dev)
        ego, pose, world = motion(k, rgb, d, keep)
        fused = filt.step(d, pose, mask=keep)
        kept = (fused.code != 0).to(torch.uint8)
        world = np.vstack([world, [0.0, 0.0, 0.0, 1.0]])
        first = world if first is None else first
        into_first = np.linalg.solve(first, world)[:3]
        normals = ops.surface_normals(fused.disp, cam, mask=kept, min_disp=1.0, max_depth=inf, max_jump=1.0)[0]
        updated.append(int(vol.integrate(fused.disp, cam, into_first, sigma=torch.sqrt(fused.var), mask=kept, normals=normals, rgb=rgb)[0]))
        view = vol.raycast(cam, into_first, *d.shape[2:], z_near=0.5, weight=False, normals=False)
        want = {".png": (io.save_png, io.disparity_to_color(fused.disp[0, 0].cpu().numpy())),
                "_tcode.png": (io.save_png, outputs.temporal_to_rgb(fused.code[0, 0].cpu().numpy())),
                "_tsigma.png": (outputs.save_png_gray8, outputs.sigma_to_u8(np.sqrt(fused.var[0, 0].cpu().numpy().astype(np.float64)), 8.0)),
                "_ego.png": (outputs.save_png_gray8, np.zeros(left.shape[:2], np.uint8) if ego is None else outputs.ego_to_u8(ego.resid[0, 0].cpu().numpy())),
                "_tsdf.png": (io.save_png, io.disparity_to_color(view.disp[0, 0].cpu().numpy()))}
        for suffix in (s for s in want if os.path.exists(out / (stem + s))):
            want[suffix][0](str(tmp / "want.png"), want[suffix][1])
            assert (out / (stem + suffix)).read_bytes() == (tmp / "want.png").read_bytes(), stem + suffix
    return updated


def test_inference_cli_three_stages_over_a_gap_with_estimated_poses(dev, model, gap_sequence, tmp_path, caplog):
    """--egomotion, --temporal and --tsdf in one run: the filter takes the estimate's motion (nothing on the first frame and after an
    estimate that is not to be trusted), the volume the accumulated pose and the filter's map and sigma.  Every file is what Odometry,
    TemporalFilter, ops.surface_normals and TsdfVolume give composed by hand; the skipped pair keeps its line of the poses file."""
    import logging
    import re
    from lwsnet_amd import inference, ops
    from lwsnet_amd.egomotion import Odometry
    from lwsnet_amd.geometry import read_kitti_poses, read_mesh_ply
    from lwsnet_amd.tsdf import TsdfVolume
    flags, frames = gap_sequence
    out, pose_file, ply = tmp_path / "out", tmp_path / "est_poses.txt", tmp_path / "map.ply"
    with caplog.at_level(logging.INFO, logger="lwsnet_amd.inference"):
        written = inference.main(flags + ["--save_path", str(out), "--egomotion", "--ego_levels", "3", "--ego_iters", "4", "--save_poses", str(pose_file),
                                          "--save_ego", "--temporal", "--save_temporal", "--tsdf", "--tsdf_voxel", "0.4", "--tsdf_extent", "-8", "8", "-3.2", "3.2",
                                          "0", "32", "--tsdf_weight", "sigma", "--save_tsdf", "--save_tsdf_ply", str(ply)])
    names = [stem + e for _, stem, *_ in frames for e in (".png", "_occ.png", "_tcode.png", "_tsigma.png", "_ego.png", "_tsdf.png")]
    assert sorted(os.listdir(out)) == sorted(names) and written == [str(out / n) for n in names] + [str(pose_file), str(ply)]
    lines = [r.getMessage() for r in caplog.records]
    assert "TSDF: volume 41 x 17 x 81 voxels of 0.4 m from (-8, -3.2, 0), {} bytes".format(12 * 41 * 17 * 81) in lines
    odo, world, resets = Odometry(frames[0][3], levels=3, iters=4, huber=10.0, min_disp=1.0), {}, []

    def motion(k, rgb, d, keep):                            # pair 2 is aligned with pair 0: the estimate spans the gap
        ego = odo.step(rgb, d, keep, resid=True)
        world[k] = odo.poses()[-1]
        trusted = ego is not None and not int(ego.status[0]) & ops.EGO_UNTRUSTED
        resets.extend([k] * (ego is not None and not trusted))
        return ego, ego.pose if trusted else None, world[k]

    vol = TsdfVolume((-8.0, -3.2, 0.0), 0.4, (41, 17, 81), mu0=3.0 * 0.4, weight="sigma", colour=True, min_disp=1.0, max_depth=float("inf"), device=dev)
    updated = _by_hand(dev, frames, out, tmp_path, vol, False, motion)
    assert sum(line.startswith("Temporal: the ego-motion estimate") for line in lines) == len(resets)
    assert [int(m[1]) for m in (re.fullmatch(r"TSDF: voxels updated = (\d+)", line) for line in lines) if m] == updated and min(updated) > 0
    got = read_kitti_poses(str(pose_file))
    assert got.shape == (4, 3, 4) and (got[1] == got[0]).all() and (got == np.stack([world[0], world[0], world[2], world[3]])).all()
    n = vol.write_ply(str(tmp_path / "by_hand.ply"))
    logged = [int(m[1]) for m in (re.fullmatch(r"Save TSDF points = .*, vertices = (\d+)", line) for line in lines) if m]
    assert logged == [n] and len(read_mesh_ply(str(ply))[0]) == n > 0 and ply.read_bytes() == (tmp_path / "by_hand.ply").read_bytes()


def test_inference_cli_filter_and_volume_over_a_gap_with_given_poses(dev, model, gap_sequence, tmp_path):
    """--poses of four lines over the same tree: the third and fourth pairs take lines 2 and 3 of the file -- a pose source that
    counted the frames processed would take lines 1 and 2 -- and the filter bridges the gap with relative_pose(line 0, line 2)."""
    from lwsnet_amd import inference
    from lwsnet_amd.geometry import relative_pose
    from lwsnet_amd.tsdf import TsdfVolume
    flags, frames = gap_sequence
    poses = np.stack([T.forward_pose(k, 0.3, yaw=0.002) for k in range(4)])
    pose_file, out, seen = tmp_path / "poses.txt", tmp_path / "out", []
    pose_file.write_text("".join(" ".join(repr(float(v)) for v in p.reshape(12)) + "\n" for p in poses))
    inference.main(flags + ["--save_path", str(out), "--poses", str(pose_file), "--temporal", "--temporal_hold", "--tsdf", "--save_tsdf"])
    assert sorted(os.listdir(out)) == sorted(stem + e for _, stem, *_ in frames for e in (".png", "_occ.png", "_tsdf.png"))

    def motion(k, rgb, d, keep):
        seen.append(k)
        return None, relative_pose(poses[seen[-2]], poses[k]) if len(seen) > 1 else None, poses[k]

    vol = TsdfVolume((-12.8, -3.2, 0.0), 0.2, (129, 33, 257), mu0=3.0 * 0.2, colour=True, min_disp=1.0, max_depth=float("inf"), device=dev)
    assert min(_by_hand(dev, frames, out, tmp_path, vol, True, motion)) > 0 and seen == [0, 2, 3]
