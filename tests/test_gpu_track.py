"""lws_track_normal and lws_track on the device against the numpy restatement (tests/track_reference.py): the per-pixel terms of
both kinds and the final residuals bit for bit, the two counts exactly, the 32 sums to the rounding of two orders of summation,
every traced Gauss-Newton step to the conditioning of its own matrix.  The shapes of lws_track_normal sit on the edges of the
1024-pixel tile (1023, 1024, 1025 pixels) and below a wave (4 x 4, 5 x 7); six motions (a small one, turns that take the view out of
each side of the image, a drive through the scene that puts points behind the camera) meet inputs sprinkled with NaN, +-inf, 0 and
1e30 in every map, four parameter sets (a finite and an infinite gate, lambda_g = 0, no normals), masks given or not.  Then: views
one element past a 16-byte boundary, poisoned guard bands, batch independence, a stalled stream, a captured graph, identical frames,
the pose block against the last M that a run one step longer traces, ModelTracker over a short noisy sequence against the frame-to-
frame chain and against the restatement's poses, the CLI against the classes composed by hand."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import egomotion_reference as E
import guarded
import stream_stall
import temporal_reference as T
import track_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_geometry import KITTI15_CALIB, cam_rows, cu, misaligned  # noqa: E402

F = np.float32
SHAPES, BS = ((31, 33), (32, 32), (25, 41), (4, 4), (5, 7)), (1, 3)
I34 = np.hstack([np.eye(3), np.zeros((3, 1))])
# the twist that moves the current camera away from the reference one: translation (m), rotation vector (rad)
TWISTS = {"small": (0.05, -0.03, 0.1, 0.01, -0.02, 0.015), "left": (0, 0, 0, 0, 0.5, 0), "right": (0, 0, 0, 0, -0.5, 0), "up": (0, 0, 0, 0.45, 0, 0),
          "down": (0, 0, 0, -0.45, 0, 0), "through": (0, 0, -9.0, 0, 0, 0)}
# per case, in turn: the scalars and which optional maps are given
VARIANTS = (dict(gate_g=4.0, huber_g=1.5, lambda_g=1.0, sigma=True, normals=True),
            dict(gate_g=np.inf, huber_g=1.0, lambda_g=0.5, sigma=False, normals=True, sigma_min=1e-38, sigma0=0.0),
            dict(gate_g=4.0, huber_g=1.5, lambda_g=0.0, sigma=True, normals=True),
            dict(gate_g=6.0, huber_g=2.0, lambda_g=2.0, sigma=False, normals=False))
NORMAL_KW = dict(min_disp=0.5, huber_p=4.0, sigma_p=3.0, sigma0=0.3, sigma_min=0.05)
SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, 1e30, -3.0], F)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, hip_lib):
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    return LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()


def case_camera(H, W):
    from lwsnet_amd.geometry import Camera
    f = max(1.25 * W, 8.0)
    return Camera(f, f, (W - 1) / 2.0, 0.4 * (H - 1), 0.5)


def sprinkle(a, rng, share, values=SPECIAL):
    flat = a.reshape(-1)
    idx = rng.choice(flat.size, size=max(1, int(flat.size * share)), replace=False)
    flat[idx] = values[np.arange(len(idx)) % len(values)]


_WANT = {}


def normal_cases(H, W, B):
    """Per variant: the inputs of the case and its restatement, computed once.  The model maps are the corner of three planes seen
    from the identity, the current maps the same corner from the moved camera with noise of about a standard deviation, a few
    pixels far off (gated) and the specials; the grey images are noise, so both sides of the photometric Huber threshold occur."""
    if (H, W, B) not in _WANT:
        out, names = [], list(TWISTS)
        cam = case_camera(H, W)
        rows = cam_rows([cam] * B)
        for i, var in enumerate(VARIANTS):
            rng = np.random.default_rng(1000 * H + 10 * W + B + 7 * i)
            kw = {**NORMAL_KW, **{k: v for k, v in var.items() if k not in ("sigma", "normals")}}
            g0, g1 = (rng.uniform(0.0, 255.0, (B, 1, H, W)).astype(F) for _ in range(2))
            g1 = (0.9 * g0 + 0.1 * g1).astype(F)
            d0, d1, n0, M = np.empty((B, 1, H, W), F), np.empty((B, 1, H, W), F), np.empty((B, 3, H, W), F), np.empty((B, 12))
            sigma = rng.choice(np.array([0.0, 0.01, 0.2, 0.3, 0.5], F), size=(B, 1, H, W)) if var["sigma"] else None
            for b in range(B):
                tw = np.array(TWISTS[names[(i + H + b) % len(names)]], np.float64)
                T1 = R.motion_pose(tw)
                d0[b, 0], n0[b] = R.planes_view(R.CORNER, I34, H, W, rows[b])
                d1[b, 0], _ = R.planes_view(R.CORNER, T1, H, W, rows[b])
                M[b] = E.true_motion(I34, T1) + rng.normal(0, 1e-3, 12)           # near the truth, not at it
            d1 += (0.3 * rng.standard_normal(d1.shape)).astype(F)
            far = rng.random(d1.shape) < 0.05
            d1[far] *= F(1.6)
            for a, share in ((g0, 0.03), (g1, 0.03), (d0, 0.06), (d1, 0.06), (n0, 0.04)):
                sprinkle(a, rng, share)
            n0[:, :, rng.random((H, W)) < 0.05] = 0                               # no normal: a ray that found no gradient
            if sigma is not None:
                sprinkle(sigma, rng, 0.06, np.array([np.nan, np.inf, -1.0, -np.inf], F))
            mask_ref = rng.choice(np.array([0, 1, 1, 1, 1, 2], np.uint8), size=(B, 1, H, W)) if i % 2 == 0 else None
            mask_cur = rng.choice(np.array([0, 1, 1, 1, 1, 2], np.uint8), size=(B, 1, H, W)) if (i + W) % 2 == 0 else None
            normals = n0 if var["normals"] else None
            want = R.normal(g0, d0, normals, mask_ref, g1, d1, sigma, mask_cur, rows, M, **{**R.DEFAULTS, **kw, "iters": 1})
            out.append(dict(variant=i, kw=kw, cams=[cam] * B, rows=rows, g0=g0, d0=d0, n0=normals, mask_ref=mask_ref, g1=g1, d1=d1, sigma=sigma,
                            mask_cur=mask_cur, M=M, **want))
        _WANT[(H, W, B)] = out
    return _WANT[(H, W, B)]


def check_sums(got, want, mag, n, what):
    """The two counts exactly, the spare 0, every other sum within (n + 64) 2^-53 sum|term| of the restatement's float64 sum."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, got.dtype)
    for k in (28, 30, 31):
        assert (got[..., k] == want[..., k]).all(), (what, k, got[..., k], want[..., k])
    worst = np.abs(got - want) - E.sum_bound(n, mag)
    assert (worst <= 0).all(), (what, int(np.argmax(worst)), float(worst.max()))


def dv(a, dev):
    return None if a is None else cu(a, dev)


def run_normal(dev, c, terms=True):
    from lwsnet_amd import ops
    return ops.track_normal(cu(c["g0"], dev), cu(c["d0"], dev), cu(c["g1"], dev), cu(c["d1"], dev), c["cams"], c["M"], normals_ref=dv(c["n0"], dev),
                            mask_ref=dv(c["mask_ref"], dev), sigma_cur=dv(c["sigma"], dev), mask_cur=dv(c["mask_cur"], dev), terms=terms, **c["kw"])


@pytest.mark.parametrize("H,W,B", [(h, w, b) for (h, w), b in itertools.product(SHAPES, BS)])
def test_track_normal_terms_bitexact_and_sums_to_rounding(dev, hip_lib, H, W, B):
    for c in normal_cases(H, W, B):
        what = f"B={B} {H}x{W} variant {c['variant']}"
        res = run_normal(dev, c)
        assert res.pose is None and res.resid is None
        guarded.assert_bits(res.terms, c["terms"], what + " terms")
        check_sums(res.sums, c["sums"], c["mag"], c["n"], what)
        again = run_normal(dev, c, terms=False)
        assert again.terms is None
        guarded.assert_bits(again.sums, res.sums.cpu().numpy(), what + " sums without terms")     # the same bytes on every run


def test_with_lambda_zero_the_photometric_half_is_ego_normal_in_bits(dev, hip_lib):
    from lwsnet_amd import ops
    c = normal_cases(25, 41, 3)[2]
    assert c["kw"]["lambda_g"] == 0.0 and c["mask_ref"] is not None
    res = run_normal(dev, c)
    sums, terms = ops.ego_normal(cu(c["g0"], dev), cu(c["d0"], dev), cu(c["g1"], dev), c["cams"], c["M"], level=0, mask=cu(c["mask_ref"], dev),
                                 min_disp=c["kw"]["min_disp"], huber=c["kw"]["huber_p"], terms=True)
    guarded.assert_bits(res.terms[..., :8].contiguous(), terms.cpu().numpy(), "terms[:8]")
    assert (res.terms[..., 8:] == 0).all() and (res.sums[:, 28] == sums[:, 28]).all() and (res.sums[:, 29:] == 0).all()


def test_the_cases_reach_every_branch():
    """Over all the cases above (their restatements; computed here where that test did not run): every exclusion of either term
    occurs, each side of the image is left, both sides of both Huber thresholds are met, the sigma floor is used, and the special
    values reach every input."""
    seen = {k: 0 for k in R.REASONS}
    lam0 = no_normals = 0
    special = {name: np.zeros(3, bool) for name in ("g0", "g1", "d0", "d1", "n0", "sigma")}
    for (H, W), B in itertools.product(SHAPES, BS):
        for c in normal_cases(H, W, B):
            for why in c["why"]:
                for k in R.REASONS:
                    seen[k] += int(why[k].sum())
            lam0 += c["kw"]["lambda_g"] == 0.0
            no_normals += c["n0"] is None
            for name, flags in special.items():
                if c[name] is not None:
                    flags |= [np.isnan(c[name]).any(), np.isinf(c[name]).any(), (c[name] == 0).any()]
    print("pixels per branch over all cases:", seen)
    assert all(v > 0 for v in seen.values()), seen
    assert all(flags.all() for flags in special.values()), special           # NaN, inf and 0 in every input
    assert lam0 > 0 and no_normals > 0


# ---- the whole refinement ----
def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


TRACK_KW = dict(min_disp=0.5, huber_p=10.0, sigma_p=4.0, huber_g=1.5, gate_g=4.0, sigma0=0.2, sigma_min=0.05, lambda_g=1.0, damping=0.0, min_pixels=64)
SCALARS = ("min_disp", "huber_p", "sigma_p", "huber_g", "gate_g", "sigma0", "sigma_min", "lambda_g")
INPUTS = ("rgb_ref", "disp_ref", "normals_ref", "mask_ref", "rgb_cur", "disp_cur", "sigma_cur", "mask_cur", "cam")
OUTPUTS = ("pose", "status", "info", "trace", "resid")
# camera-to-world pose of the current frame (the reference frame is the identity): dz, yaw, dx
MOTIONS = {"forward": (0.3, 0.0, 0.0), "yaw": (0.1, 0.02, 0.0), "far": (0.6, 0.03, 0.05)}


def raw_track(lib, dev, b, shape, iters, kw=TRACK_KW):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_track(*(P(b.get(k)) for k in INPUTS), P(b.get("init")), *shape, iters, *(kw[k] for k in SCALARS), kw["damping"], kw["min_pixels"],
                                 P(b["work"]), P(b["pose"]), P(b["status"]), P(b["info"]), P(b.get("trace")), P(b.get("resid")),
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "lws_track")


_PAIRS = {}


def scene_pair(H, W, motion, seed=0):
    """The road-and-wall scene before and after `motion`: the model maps are the clean first view with the normals of its own
    surface, the current maps the second view with 0.2 px of seeded noise and a sigma map that says so."""
    import mesh_reference as SN
    if (H, W, motion, seed) not in _PAIRS:
        dz, yaw, dx = MOTIONS[motion]
        T0, T1 = T.forward_pose(0, 0.0), T.forward_pose(1, dz, yaw, dx)
        cam = np.array(E.scene_cam(H, W), F)
        rgb0, d0, mask, rgb1 = E.scene_pair(H, W, T0, T1)
        n0, _ = SN.surface_normals(d0[None, None], mask[None, None], cam[None], TRACK_KW["min_disp"], np.inf, 1.0)
        clean = T.render(T1, H, W, tuple(cam)).astype(F)
        rng = np.random.default_rng(seed + 17)
        d1 = np.where(clean > 0, clean + F(0.2) * rng.standard_normal(clean.shape).astype(F), clean).astype(F)
        sigma = np.full((H, W), 0.2, F)
        _PAIRS[(H, W, motion, seed)] = dict(rgb_ref=rgb0, disp_ref=d0[None], normals_ref=n0[0], mask_ref=mask[None], rgb_cur=rgb1, disp_cur=d1[None],
                                            sigma_cur=sigma[None], mask_cur=E.edge_codes(clean)[None], cam=cam, true=E.true_motion(T0, T1))
    return _PAIRS[(H, W, motion, seed)]


def batch_case(H, W, B, first="forward"):
    names = list(MOTIONS)
    cs = [scene_pair(H, W, names[(names.index(first) + b) % len(names)], b) for b in range(B)]
    out = {k: np.stack([c[k] for c in cs]) for k in INPUTS}
    out["true"] = [c["true"] for c in cs]
    return out


def output_buffers(dev, B, H, W, iters, lib):
    return dict(work=torch.empty((lib.lws_track_workspace(B, H, W),), dtype=torch.uint8, device=dev),
                pose=torch.empty((B, 2, 12), dtype=torch.float32, device=dev), status=torch.empty((B,), dtype=torch.int32, device=dev),
                info=torch.empty((B, 6), dtype=torch.float64, device=dev), trace=torch.empty((B, iters, 51), dtype=torch.float64, device=dev),
                resid=torch.empty((B, 2, H, W), dtype=torch.float32, device=dev))


def run_track(lib, dev, c, iters, init=None, kw=TRACK_KW, drop=()):
    B, _, H, W = c["disp_ref"].shape
    b = {k: cu(c[k], dev) for k in INPUTS if k not in drop}
    if init is not None:
        b["init"] = cu(np.asarray(init, F), dev)
    b.update(output_buffers(dev, B, H, W, iters, lib))
    raw_track(lib, dev, b, (B, H, W), iters, kw)
    torch.cuda.synchronize(dev)
    return tuple(b[k].cpu().numpy() for k in OUTPUTS)


MAX_COND = 1e8


def linearise(c, b, M, kw):
    p = R.params(**{k: kw[k] for k in R.DEFAULTS if k in kw})
    H, W = c["disp_ref"].shape[2:]
    ok = lambda m: m[b, 0] == 1 if m is not None else np.ones((H, W), bool)         # noqa: E731
    terms, up, ug, _, _ = R.normal_image(E.grey_of(c["rgb_ref"][b]), c["disp_ref"][b, 0], ok(c.get("mask_ref")),
                                         None if c.get("normals_ref") is None else c["normals_ref"][b], E.grey_of(c["rgb_cur"][b]), c["disp_cur"][b, 0],
                                         None if c.get("sigma_cur") is None else c["sigma_cur"][b, 0], ok(c.get("mask_cur")), c["cam"][b], M, p)
    return terms, R.sums_of(terms, up, ug, p), p


def check_track(c, got, iters, what, init=None, kw=TRACK_KW):
    """Holds one call's outputs (numpy) to the restatement, image by image: the sums of every traced step at the traced M, its code,
    its delta and the next M to the conditioning of the step's matrix; then the pose block, resid, info and status."""
    pose, status, info, trace, resid = got
    B = len(pose)
    for b in range(B):
        tr = trace[b]
        M0 = E.IDENTITY12 if init is None else np.asarray(init[b], F).astype(np.float64)
        assert (tr[0, :12] == M0).all(), what
        st, steps, last, final_ref, final_tol = 0, 0, 0.0, None, 0.0
        for s in range(iters):
            M, sums, delta, code = tr[s, :12], tr[s, 12:44], tr[s, 44:50], int(tr[s, 50])
            _, (want, mag, n), _ = linearise(c, b, M, kw)
            check_sums(sums[None], want[None], mag[None], n[None], f"{what} image {b} step {s}")
            new, wd, wcode = R.update(sums, M, kw["damping"], kw["min_pixels"])
            assert code == wcode, (what, b, s, code, wcode)
            st |= code
            nxt = tr[s + 1, :12] if s + 1 < iters else None
            if code != 0:
                assert nxt is None or (nxt == M).all(), (what, b, s)
                continue
            cond = np.linalg.cond(E.unpack(sums[:27])[0])
            assert cond < MAX_COND, (what, b, s, cond)
            tol = 64 * cond * 2.0 ** -52
            assert np.abs(delta - wd).max() <= tol * np.abs(wd).max(), (what, b, s, delta, wd)
            if nxt is not None:
                assert np.abs(nxt - new).max() <= tol * np.abs(new).max(), (what, b, s)
            steps, last, final_ref, final_tol = steps + 1, float(np.sqrt((delta * delta).sum())), new, tol * np.abs(new).max()
        if int(tr[-1, 50]) == 0:
            half_ulp = np.spacing(np.abs(final_ref).astype(F)).astype(np.float64) / 2
            assert (np.abs(pose[b, 0].astype(np.float64) - final_ref) <= final_tol + half_ulp).all(), (what, b)
        else:                                               # the last step was refused: the last M is the traced one
            guarded.assert_bits(pose[b, 0], tr[-1, :12].astype(F), f"{what} image {b} pose[0]")
            guarded.assert_bits(pose[b, 1], E.inverse12(tr[-1, :12]).astype(F), f"{what} image {b} pose[1]")
        Mf = pose[b, 0].astype(np.float64)
        assert np.abs(pose[b, 1].astype(np.float64) - E.inverse12(Mf)).max() <= 2.0 ** -22 * max(1.0, np.abs(Mf).max()), (what, b)
        # float32(M) is all the final linearisation sees of M: resid bit for bit, the counts exactly, the rms to rounding
        terms, (fs, _, _), p = linearise(c, b, Mf, kw)
        guarded.assert_bits(resid[b], np.stack([terms[..., 0], terms[..., 8]]), f"{what} image {b} resid")
        kp, kg = R.weights(p)
        assert info[b, 0] == fs[28] and info[b, 2] == fs[30] and info[b, 5] == steps and abs(info[b, 4] - last) <= 1e-12 * max(last, 1e-30), (what, b, info[b])
        for k, (e, n, wgt) in ((1, (fs[27], fs[28], kp)), (3, (fs[29], fs[30], kg))):
            rms = np.sqrt(e / (wgt * n)) if n > 0 else 0.0
            assert abs(info[b, k] - rms) <= 1e-12 * max(rms, 1e-30), (what, b, k)
        flags = (E.BIT_FINAL_FEW if fs[28] + fs[30] < kw["min_pixels"] else 0) | (R.BIT_NO_MODEL if fs[30] < kw["min_pixels"] else 0)
        assert status[b] == st | flags, (what, b, status[b], st, flags)


@pytest.mark.parametrize("B", (1, 2))
def test_track_traced_steps_and_final_outputs(dev, hip_lib, B):
    H, W, iters = 48, 96, 6
    c = batch_case(H, W, B)
    got = run_track(hip_lib, dev, c, iters)
    check_track(c, got, iters, f"B={B}")
    for b in range(B):
        et, er = E.motion_error(got[0][b, 0].astype(np.float64), c["true"][b])
        print(f"image {b}: error {et:.5f} m, {er:.4f} deg, status {got[1][b]}, info {got[2][b].tolist()}")
        assert got[1][b] & ~E.BIT_SMALL == 0 and got[2][b, 2] > 1000 and et <= 0.06 and er <= 0.5      # a fifth of the shortest step, half a degree
    # without normals, and with lambda_g = 0, the model does not constrain the pose: bit 5
    for drop, kw in ((("normals_ref",), TRACK_KW), ((), {**TRACK_KW, "lambda_g": 0.0})):
        c2 = {k: v for k, v in c.items() if k not in drop}
        alone = run_track(hip_lib, dev, c2, iters, kw=kw, drop=drop)
        check_track(c2, alone, iters, f"B={B} photometric only", kw=kw)
        assert (alone[1] & R.BIT_NO_MODEL).all() and (alone[2][:, 2:4] == 0).all() and (alone[3][:, :, 12 + 29:12 + 32] == 0).all()


def test_the_pose_block_is_the_float32_rounding_of_the_last_M_and_of_its_double_inverse(dev, hip_lib):
    """The run with k + 1 steps repeats the run with k steps and then traces, as M before step k, the M the shorter run ended with."""
    H, W, B, k = 48, 96, 2, 3
    c = batch_case(H, W, B, "far")
    short, longer = run_track(hip_lib, dev, c, k), run_track(hip_lib, dev, c, k + 1)
    assert np.array_equal(guarded.as_bits(short[3]), guarded.as_bits(longer[3][:, :k])), "the first k steps of the two runs"
    assert (short[3][:, :, 50] == 0).all() and (longer[3][:, :, 50] == 0).all()
    last = longer[3][:, k, :12]
    assert (last.astype(F).astype(np.float64) != last).any(axis=1).all()
    guarded.assert_bits(short[0][:, 0], last.astype(F), "pose[0]")
    guarded.assert_bits(short[0][:, 1], np.stack([E.inverse12(m) for m in last]).astype(F), "pose[1]")


def test_identical_frames_and_a_model_of_the_same_frame_give_the_identity_in_bits(dev, hip_lib):
    H, W, iters = 48, 96, 4
    s = scene_pair(H, W, "forward")
    c = {k: s[k][None] for k in INPUTS}
    c.update(rgb_cur=c["rgb_ref"], disp_cur=c["disp_ref"], mask_cur=c["mask_ref"])
    pose, status, info, trace, resid = got = run_track(hip_lib, dev, c, iters)
    check_track(c, got, iters, "identity")
    assert (trace[0, :, 50] == E.BIT_SMALL).all() and status[0] == E.BIT_SMALL and info[0, 4] == 0 and info[0, 5] == 0
    guarded.assert_bits(pose[0], np.stack([E.IDENTITY12, E.IDENTITY12]).astype(F), "pose")
    assert (resid[0, 1] == 0).all() and np.abs(resid[0, 0]).max() < 1e-3 and info[0, 0] > 0.4 * H * W and info[0, 2] > 0.2 * H * W and info[0, 3] == 0


def test_init_is_kept_where_no_step_is_taken_and_the_inverse_is_formed_in_double(dev, hip_lib):
    H, W, B = 48, 96, 2
    c = batch_case(H, W, B)
    rng = np.random.default_rng(2)
    init = np.stack([E.compose(E.exp_se3(rng.normal(size=6) * 0.2), E.IDENTITY12) for _ in range(B)]).astype(F)
    kw = {**TRACK_KW, "min_pixels": 2 * H * W + 1}
    pose, status, info, trace, resid = got = run_track(hip_lib, dev, c, 3, init=init, kw=kw)
    check_track(c, got, 3, "no step", init=init, kw=kw)
    guarded.assert_bits(pose[:, 0], init, "pose[0]")
    guarded.assert_bits(pose[:, 1], np.stack([E.inverse12(m.astype(np.float64)) for m in init]).astype(F), "pose[1]")
    assert (status == E.BIT_FEW | E.BIT_FINAL_FEW | R.BIT_NO_MODEL).all() and (trace[:, :, 50] == E.BIT_FEW).all() and (info[:, 4:] == 0).all()


# ---- call hygiene ----
def test_batch_independence(dev, hip_lib):
    """The same image alone, first of two and second of two gives the same bytes, in every output."""
    H, W, iters = 48, 96, 3
    c = batch_case(H, W, 2)

    def run(order):
        idx = list(order)
        return run_track(hip_lib, dev, {k: np.ascontiguousarray(c[k][idx]) for k in INPUTS}, iters)

    both, swapped, alone = run((0, 1)), run((1, 0)), run((1,))
    for g, s, a, key in zip(both, swapped, alone, OUTPUTS):
        bits = guarded.as_bits(g[1])
        assert np.array_equal(bits, guarded.as_bits(s[0])) and np.array_equal(bits, guarded.as_bits(a[0])), key
    again = run((0, 1))
    for g, a, key in zip(both, again, OUTPUTS):
        assert np.array_equal(guarded.as_bits(g), guarded.as_bits(a)), key      # and on every run


def normal_buffers(put, c):
    return dict(g0=put(c["g0"], "grey_ref"), d0=put(c["d0"], "disp_ref"), n0=None if c["n0"] is None else put(c["n0"], "normals_ref"),
                mask_ref=None if c["mask_ref"] is None else put(c["mask_ref"], "mask_ref"), g1=put(c["g1"], "grey_cur"), d1=put(c["d1"], "disp_cur"),
                sigma=None if c["sigma"] is None else put(c["sigma"], "sigma_cur"), mask_cur=None if c["mask_cur"] is None else put(c["mask_cur"], "mask_cur"),
                cam=put(c["rows"], "cam"))


def raw_normal(lib, dev, nb, shape, kw):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_track_normal(*(P(nb[k]) for k in ("g0", "d0", "n0", "mask_ref", "g1", "d1", "sigma", "mask_cur", "cam", "M")), *shape,
                                        *(float(kw[k]) for k in SCALARS), P(nb["work"]), P(nb["sums"]), P(nb["terms"]),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "lws_track_normal")


def test_one_element_past_a_16_byte_boundary(dev, hip_lib):
    H, W, B, iters = 48, 96, 2, 2
    c = batch_case(H, W, B, "far")
    want = run_track(hip_lib, dev, c, iters)
    b = {k: misaligned(c[k], dev) for k in INPUTS}
    out = output_buffers(dev, B, H, W, iters, hip_lib)
    b.update(work=out["work"], pose=misaligned(np.zeros((B, 2, 12), F), dev), status=misaligned(np.zeros((B,), np.int32), dev), info=out["info"],
             trace=out["trace"], resid=misaligned(np.zeros((B, 2, H, W), F), dev))
    raw_track(hip_lib, dev, b, (B, H, W), iters)
    for k, w in zip(OUTPUTS, want):
        guarded.assert_bits(b[k], w, f"misaligned {k}")      # the same bytes as from aligned memory
    # lws_track_normal: terms on the scalar path
    n = normal_cases(25, 41, 3)[0]
    nb = normal_buffers(lambda a, name: misaligned(a, dev), n)
    nb.update(M=cu(n["M"], dev), sums=torch.empty((3, 32), dtype=torch.float64, device=dev), terms=misaligned(np.zeros((3, 25, 41, 16), F), dev),
              work=torch.empty((hip_lib.lws_track_workspace(3, 25, 41),), dtype=torch.uint8, device=dev))
    raw_normal(hip_lib, dev, nb, (3, 25, 41), {**R.DEFAULTS, **n["kw"]})
    guarded.assert_bits(nb["terms"], n["terms"], "misaligned terms")
    check_sums(nb["sums"], n["sums"], n["mag"], n["n"], "misaligned sums")


@pytest.mark.parametrize("word", guarded.FLOAT_WORDS, ids=guarded.word_id)
def test_memory_contract(dev, hip_lib, word):
    """Inputs, outputs and the workspace between poisoned flanks, the outputs and the workspace poisoned inside: no flank changes,
    every output element is written, and the bytes are those of a call on plain memory.  25 x 41: a last tile of one pixel."""
    B, H, W, iters = 3, 25, 41, 2
    n = normal_cases(H, W, B)[0]
    rng = np.random.default_rng(11)
    rgb = [np.repeat(np.clip(np.nan_to_num(g[:, 0], nan=7.0, posinf=255.0, neginf=0.0), 0, 255).astype(np.uint8)[..., None], 3, -1) for g in (n["g0"], n["g1"])]
    c = dict(rgb_ref=rgb[0], disp_ref=n["d0"], normals_ref=n["n0"], mask_ref=n["mask_ref"], rgb_cur=rgb[1], disp_cur=n["d1"], sigma_cur=n["sigma"],
             mask_cur=rng.choice(np.array([0, 1, 1, 1, 2], np.uint8), size=(B, 1, H, W)), cam=n["rows"])
    kw = {**TRACK_KW, "min_pixels": 16}
    init = np.stack([E.true_motion(I34, R.motion_pose(np.array(TWISTS["small"]))) for _ in range(B)]).astype(F)
    plain = {k: cu(v, dev) for k, v in c.items()}
    plain.update(output_buffers(dev, B, H, W, iters, hip_lib), init=cu(init, dev))
    raw_track(hip_lib, dev, plain, (B, H, W), iters, kw)
    assert np.isfinite(plain["info"].cpu().numpy()).all() and (plain["info"].cpu().numpy()[:, [0, 2]] > 0).any()
    gd = guarded.Guard(dev, word, skew=1)
    b = dict(rgb_ref=gd.place(c["rgb_ref"], plane=3 * H * W, name="rgb_ref"), disp_ref=gd.place(c["disp_ref"], name="disp_ref"),
             normals_ref=gd.place(c["normals_ref"], name="normals_ref"), mask_ref=gd.place(c["mask_ref"], word=guarded.MASK_WORD, name="mask_ref"),
             rgb_cur=gd.place(c["rgb_cur"], plane=3 * H * W, name="rgb_cur"), disp_cur=gd.place(c["disp_cur"], name="disp_cur"),
             sigma_cur=gd.place(c["sigma_cur"], name="sigma_cur"), mask_cur=gd.place(c["mask_cur"], word=guarded.MASK_WORD, name="mask_cur"),
             cam=gd.place(c["cam"], name="cam"), init=gd.place(init, name="init"),
             work=gd.empty((hip_lib.lws_track_workspace(B, H, W),), np.uint8, align16=True, word=gd.word, name="workspace"),
             pose=gd.empty((B, 2, 12), F, name="pose"), status=gd.empty((B,), np.int32, name="status"),
             info=gd.empty((B, 6), np.float64, align16=True, name="info"), trace=gd.empty((B, iters, 51), np.float64, align16=True, name="trace"),
             resid=gd.empty((B, 2, H, W), F, name="resid"))
    raw_track(hip_lib, dev, b, (B, H, W), iters, kw)
    for k in OUTPUTS:
        guarded.assert_bits(b[k], plain[k].cpu().numpy(), f"guarded {k}")
    gd.check()
    # lws_track_normal the same way
    gn = guarded.Guard(dev, word, skew=1)
    nb = normal_buffers(lambda a, name: gn.place(a, word=guarded.MASK_WORD if a.dtype == np.uint8 else None, name=name), n)
    nb.update(M=gn.place(n["M"], align16=True, name="M"), work=gn.empty((hip_lib.lws_track_workspace(B, H, W),), np.uint8, align16=True, word=gn.word, name="workspace"),
              sums=gn.empty((B, 32), np.float64, align16=True, name="sums"), terms=gn.empty((B, H, W, 16), F, plane=16 * H * W, name="terms"))
    raw_normal(hip_lib, dev, nb, (B, H, W), {**R.DEFAULTS, **n["kw"]})
    guarded.assert_bits(nb["terms"], n["terms"], "guarded terms")
    check_sums(nb["sums"], n["sums"], n["mag"], n["n"], "guarded sums")
    gn.check()


def test_a_stalled_stream_holds_the_call_and_its_inputs(dev, hip_lib):
    """The call on a stream held by a device-side delay: it returns while the stream is still held (nothing is read back), and it
    reads inputs that were written on that stream behind the delay -- a launch on any other stream would read the poison."""
    H, W, B, iters = 48, 96, 2, 2
    c = batch_case(H, W, B)
    want = run_track(hip_lib, dev, c, iters)
    real = {k: cu(c[k], dev) for k in INPUTS}
    for stream in stream_stall.caller_streams(dev):
        b = {k: (torch.full_like(v, 1) if v.dtype == torch.uint8 else torch.full_like(v, float("nan"))) for k, v in real.items()}
        b["cam"] = real["cam"]
        b.update(output_buffers(dev, B, H, W, iters, hip_lib))
        for k in OUTPUTS + ("work",):
            b[k].fill_(77)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            held = stream_stall.stall(stream)
            for k in INPUTS[:-1]:
                b[k].copy_(real[k], non_blocking=True)
            raw_track(hip_lib, dev, b, (B, H, W), iters)
            stream_stall.assert_still_stalled(held, "lws_track")
        stream.synchronize()
        for k, w in zip(OUTPUTS, want):
            guarded.assert_bits(b[k], w, f"stalled {k}")


def test_graph_capture_replays_on_two_input_sets(dev, hip_lib):
    H, W, B, iters = 48, 96, 2, 3
    first, second = batch_case(H, W, B, "forward"), batch_case(H, W, B, "yaw")
    keys = INPUTS[:-1]
    want = {id(c): run_track(hip_lib, dev, c, iters) for c in (first, second)}
    b = {k: cu(first[k], dev) for k in INPUTS}
    b.update(output_buffers(dev, B, H, W, iters, hip_lib))
    raw_track(hip_lib, dev, b, (B, H, W), iters)              # the code object is loaded before the capture
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_track(hip_lib, dev, b, (B, H, W), iters)
    for c in (first, second, first):
        for k in keys:
            b[k].copy_(cu(c[k], dev))
        for k in OUTPUTS + ("work",):
            b[k].fill_(77)
        graph.replay()
        torch.cuda.synchronize(dev)
        for k, w in zip(OUTPUTS, want[id(c)]):
            guarded.assert_bits(b[k], w, f"replay {k}")


# ---- the state-holding class ----
# The float32-per-step restatement of both estimators on the sequence below (R.run_sequence), measured once on the CPU: the final
# position error in metres of the frame-to-frame chain and of the chain refined against the volume, per noise level in px and
# seed.  At every level the chain's error is mostly the bias of the photometric minimum on this scene (it hardly moves with the
# noise); the model takes a quarter off it.  With the weight of the point-to-plane term taken at the tap's own noisy depth, as the
# rule was first written, the tracked error at 0.3 px was 0.092 / 0.102 m, twice the chain's: see include/lwsnet_track.h.
MEASURED = {(0.0, 1): (0.0529, 0.0373), (0.2, 1): (0.0481, 0.0349), (0.2, 2): (0.0538, 0.0454), (0.3, 1): (0.0475, 0.0353), (0.3, 2): (0.0541, 0.0444)}
SEQ_SEED = 1
EGO_KW = dict(levels=3, iters=8, min_disp=0.5, min_pixels=64)
SEQ_TRACK_KW = dict(iters=6, min_disp=0.5, sigma0=R.SEQUENCE["noise"], min_pixels=64)


def test_model_tracker_over_a_short_sequence_against_the_chain_and_the_restatement(dev, hip_lib):
    """Seven frames of the road-and-wall scene, 0.3 m and 0.01 rad apart, 0.2 px of disparity noise.  Odometry alone and Odometry +
    ModelTracker + TsdfVolume on the same inputs: the tracked final position is no further from the truth than the chain's, and
    every tracked pose is the restatement's to the bound its sums' rounding gives (R.step_bound per frame, accumulated: a pose is
    the product of the motions before it)."""
    from lwsnet_amd import egomotion, ops
    from lwsnet_amd.geometry import Camera
    from lwsnet_amd.tracking import ModelTracker
    from lwsnet_amd.tsdf import TsdfVolume
    s = R.SEQUENCE
    inputs, cam_row, truth = R.sequence_inputs(s["noise"], SEQ_SEED)
    want = R.run_sequence(inputs, cam_row, EGO_KW, SEQ_TRACK_KW)
    H, W = s["H"], s["W"]
    cam = Camera(*(float(v) for v in cam_row[:4]), float(cam_row[4] / cam_row[0]))
    odo = egomotion.Odometry(cam, **EGO_KW)
    vol = TsdfVolume(s["origin"], s["vs"], s["dims"], mu0=s["mu0"], mu_d=s["mu_d"], min_disp=0.5, sigma0=s["noise"], device=dev)
    trk = ModelTracker(vol, cam, w_min=s["w_min"], z_near=s["z_near"], **SEQ_TRACK_KW)
    for k, (rgb, d, codes) in enumerate(inputs):
        r, dd, m = cu(rgb[None], dev), cu(d[None, None], dev), cu(codes[None, None], dev)
        ego = odo.step(r, dd, m)
        init = None if ego is None or int(ego.status[0]) & ops.EGO_UNTRUSTED else ego.pose[:, 0].contiguous()
        res = trk.step(r, dd, m, init=init)
        assert (res is None) == (k == 0)
        normals = ops.surface_normals(dd, cam, mask=m, min_disp=0.5, max_depth=float("inf"), max_jump=s["max_jump"])[0]
        vol.integrate(dd, cam, trk.poses()[-1], mask=m, normals=normals)
        if res is not None:
            print(f"frame {k}: status {int(res.status[0])}, info {res.info[0].cpu().tolist()}")
            assert int(res.status[0]) & ~E.BIT_SMALL == want["track"][k - 1]["status"] & ~E.BIT_SMALL       # (a last step at the resolution's edge may fall either way)
    chain, tracked = odo.poses(), trk.poses()
    e_chain, e_track = (float(np.linalg.norm(p[-1, :, 3] - truth[-1, :, 3])) for p in (chain, tracked))
    r_chain, r_track = (float(np.linalg.norm(want[k][-1, :, 3] - truth[-1, :, 3])) for k in ("chain", "tracked"))
    print(f"final position error: chain {e_chain:.4f} m (restated {r_chain:.4f}), tracked {e_track:.4f} m (restated {r_track:.4f}); MEASURED {MEASURED[(s['noise'], SEQ_SEED)]}")
    assert abs(r_chain - MEASURED[(s["noise"], SEQ_SEED)][0]) <= 1e-4 and abs(r_track - MEASURED[(s["noise"], SEQ_SEED)][1]) <= 1e-4
    assert e_track <= e_chain
    allowed = 0.0
    for k in range(1, len(inputs)):
        allowed += want["bounds"][k - 1] * max(1.0, np.abs(want["tracked"][k]).max())
        assert np.abs(tracked[k] - want["tracked"][k]).max() <= allowed, (k, np.abs(tracked[k] - want["tracked"][k]).max(), allowed)


def test_model_tracker_without_code_maps_keeps_the_filled_pixels(dev, hip_lib):
    """step(rgb, disp) with no code map, fill on: where the ray met nothing the reference takes the previous frame's disparity, and
    those pixels carry the photometric term -- without a code map every pixel is usable.  Three frames against the restatement with
    codes of 1 everywhere: the same terms at the filled pixels, to the few a last bit of the pose may move across an edge."""
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import Camera
    from lwsnet_amd.tracking import ModelTracker
    from lwsnet_amd.tsdf import TsdfVolume
    s = R.SEQUENCE
    inputs, cam_row, _ = R.sequence_inputs(s["noise"], SEQ_SEED, frames=3, codes=False)
    want = R.run_sequence(inputs, cam_row, EGO_KW, SEQ_TRACK_KW)
    cam = Camera(*(float(v) for v in cam_row[:4]), float(cam_row[4] / cam_row[0]))
    vol = TsdfVolume(s["origin"], s["vs"], s["dims"], mu0=s["mu0"], mu_d=s["mu_d"], min_disp=0.5, sigma0=s["noise"], device=dev)
    trk = ModelTracker(vol, cam, w_min=s["w_min"], z_near=s["z_near"], **SEQ_TRACK_KW)
    for k, (rgb, d, _) in enumerate(inputs):
        r, dd = cu(rgb[None], dev), cu(d[None, None], dev)
        init = None if k == 0 else cu(want["ego"][k - 1]["pose"][0][None], dev)       # the restatement's own frame-to-frame estimate
        res = trk.step(r, dd, init=init, resid=True)
        normals = ops.surface_normals(dd, cam, min_disp=0.5, max_depth=float("inf"), max_jump=s["max_jump"])[0]
        vol.integrate(dd, cam, trk.poses()[-1], normals=normals)
        if res is None:
            continue
        w = want["track"][k - 1]
        hit = (trk.view.disp[0, 0] > 0).cpu().numpy()
        assert int((hit != w["hit"]).sum()) <= 4, k          # the same view, to the few rays a last bit of the pose before may move
        rp = res.resid[0, 0].cpu().numpy()
        filled, filled_want = int(((rp != 0) & ~hit).sum()), int(((w["resid"][0] != 0) & ~w["hit"]).sum())
        n_p, n_p_want = int(res.info[0, 0]), int(w["info"][0])
        print(f"frame {k}: n_p {n_p} (restated {n_p_want}), of them filled {filled} (restated {filled_want}), hit {int(hit.sum())}")
        assert filled_want > 200 and abs(filled - filled_want) <= 4 and abs(n_p - n_p_want) <= 4
        assert n_p > int(((rp != 0) & hit).sum()) + 200


# ---- the CLI ----
def test_inference_cli_tracking_files(dev, model, tmp_path, caplog):
    """Four frames with --egomotion --tsdf --tsdf_track: the files exist, the poses file is what Odometry, ModelTracker and TsdfVolume
    give composed by hand, bit for bit, and so is every <stem>_track.png; the same line without --tsdf_track writes the chain's poses."""
    import logging
    from PIL import Image
    from lwsnet_amd import imageio as io
    from lwsnet_amd import inference, ops, outputs, synth
    from lwsnet_amd import postprocess as post
    from lwsnet_amd.egomotion import Odometry
    from lwsnet_amd.geometry import Camera, read_kitti_poses
    from lwsnet_amd.tracking import ModelTracker
    from lwsnet_amd.tsdf import TsdfVolume
    n = 4
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, n)
    calib = tmp_path / "calib.txt"
    calib.write_text(KITTI15_CALIB.format(fx=721.5377, cx=609.5593, cy=172.854, t3=44.85728 - 0.54 * 721.5377))
    out, pose_file, plain_out, plain_poses = tmp_path / "out", tmp_path / "tracked.txt", tmp_path / "plain", tmp_path / "chain.txt"
    common = ["--img_path", root + "/", "--synthetic_weights", "--calib", str(calib), "--occ_check", "1", "--egomotion", "--ego_levels", "3", "--ego_iters", "4",
              "--tsdf", "--tsdf_voxel", "0.4", "--tsdf_extent", "-8", "8", "-3.2", "3.2", "0", "32"]
    with caplog.at_level(logging.INFO, logger="lwsnet_amd.inference"):
        written = inference.main(common + ["--save_path", str(out), "--tsdf_track", "--track_iters", "3", "--save_poses", str(pose_file), "--save_track"])
    lines = [r.getMessage() for r in caplog.records]
    stems = [f"{k:06d}_10" for k in range(n)]
    assert sorted(os.listdir(out)) == sorted(s + e for s in stems for e in (".png", "_occ.png", "_track.png"))
    assert len(written) == 3 * n + 1 and str(pose_file) in written
    assert sum(line.startswith("Tracking: photometric pixels = ") for line in lines) == n - 1
    opts = post.Options.make(occ_check=1.0)
    odo = trk = None
    vol = TsdfVolume((-8.0, -3.2, 0.0), 0.4, (41, 17, 81), mu0=3.0 * 0.4, colour=True, min_disp=1.0, max_depth=float("inf"), device=dev)
    for k, stem in enumerate(stems):
        full = io.load_rgb(os.path.join(root, "image_2", stem + ".png"))
        left = io.crop_bottom_right(full)
        r_in = io.to_input(io.crop_bottom_right(io.load_rgb(os.path.join(root, "image_3", stem + ".png"))))[None]
        cam = Camera.from_kitti(str(calib)).crop_bottom_right(*full.shape[:2])
        res = post.run_chain(model, io.to_input(left)[None], r_in, opts)
        rgb, d, keep = outputs.rgb_on_device(left, dev), res.disp[3].as_subclass(torch.Tensor), res.keep[3]
        odo = odo or Odometry(cam, levels=3, iters=4, huber=10.0, min_disp=1.0)
        trk = trk or ModelTracker(vol, cam, iters=3, lambda_g=1.0, gate_g=4.0, huber_g=1.5, min_disp=1.0, z_near=0.5)
        ego = odo.step(rgb, d, keep)
        init = None if ego is None or int(ego.status[0]) & ops.EGO_UNTRUSTED else ego.pose[:, 0].contiguous()
        track = trk.step(rgb, d, keep, init=init, resid=True)
        normals = ops.surface_normals(d, cam, mask=keep, min_disp=1.0, max_depth=float("inf"), max_jump=1.0)[0]
        vol.integrate(d, cam, trk.poses()[-1], mask=keep, normals=normals, rgb=rgb)
        want = np.zeros((*left.shape[:2], 3), np.uint8) if track is None else outputs.track_to_rgb(track.resid[0, 1].cpu().numpy())
        assert np.array_equal(np.asarray(Image.open(out / (stem + "_track.png"))), want), stem
        if track is not None:
            print(f"frame {k}: status {int(track.status[0])}, info {track.info[0].cpu().tolist()}")
    got = read_kitti_poses(str(pose_file))
    assert got.shape == (n, 3, 4) and (got == trk.poses()).all() and (got[0] == I34).all()
    # the same line without the flag: no tracking file, the chain's own poses
    inference.main(common + ["--save_path", str(plain_out), "--save_poses", str(plain_poses)])
    assert sorted(os.listdir(plain_out)) == sorted(s + e for s in stems for e in (".png", "_occ.png"))
    chain = read_kitti_poses(str(plain_poses))
    assert (chain == odo.poses()).all()
    print("tracked and chained poses differ:", not (chain == got).all())
    for stem in stems:
        assert (plain_out / (stem + ".png")).read_bytes() == (out / (stem + ".png")).read_bytes()
