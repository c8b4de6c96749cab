"""Ego-motion without a GPU: the numpy restatement (tests/egomotion_reference.py) recovering known motions of the textured
road-and-wall scene, its guard against levels that are too coarse, its Jacobian against finite differences of its own residual, the
se(3) exponential across the threshold of its series; the host pieces (the poses writer, argument errors of the C ABI, of
ops.ego_normal / ops.egomotion and of Odometry, the inference CLI's flags); and the CLI's pose source over a stub Odometry."""
import ctypes
import os

import numpy as np
import pytest

import egomotion_reference as E
import temporal_reference as T
from cli_helpers import CAMERA, cli_refused as _cli_refused, poses_file, sequence_dir as _sequence_dir
from lwsnet_amd import _lib

F = np.float32
# camera-to-world pose of the second frame (the first is the identity): dz, yaw, dx
MOTIONS = {"identity": (0.0, 0.0, 0.0), "forward": (0.3, 0.0, 0.0), "yaw": (0.1, 0.02, 0.0), "far": (0.8, 0.03, 0.0)}
SIZES = {(48, 96): 2, (96, 192): 3}                         # H, W -> levels
# The error of this restatement, measured once (printed by the test below), metres and degrees; the bounds are twice these.  The
# largest is 7 % of the step and 0.28 degrees: under the 20 % / 0.5 degrees that would mean a bug or an aliased scene.  What is
# left is the bias of the photometric minimum itself (the cost at the estimate is below the cost at the true motion), along the
# weakest direction of the normal matrix, the translation along the optical axis.
MEASURED = {(48, 96, "forward"): (0.01447, 0.0273), (48, 96, "yaw"): (0.00170, 0.0142), (48, 96, "far"): (0.03029, 0.1544),
            (96, 192, "forward"): (0.02101, 0.1131), (96, 192, "yaw"): (0.00519, 0.0053), (96, 192, "far"): (0.05506, 0.2721)}
MAX_COND = 1e8


def bound(H, W, motion):
    return tuple(2.0 * v for v in MEASURED[(H, W, motion)])


_CASES = {}


def scene_case(H, W, motion):
    """The scene seen before and after `motion`, and the restatement's estimate, computed once."""
    if (H, W, motion) not in _CASES:
        dz, yaw, dx = MOTIONS[motion]
        T0, T1 = T.forward_pose(0, 0.0), T.forward_pose(1, dz, yaw, dx)
        rgb0, d0, mask, rgb1 = E.scene_pair(H, W, T0, T1)
        cam = np.array(E.scene_cam(H, W), F)
        est = E.estimate_image(rgb0, d0, mask == 1, rgb1, cam, levels=SIZES[(H, W)])
        _CASES[(H, W, motion)] = dict(rgb0=rgb0, d0=d0, mask=mask, rgb1=rgb1, cam=cam, est=est, true=E.true_motion(T0, T1))
    return _CASES[(H, W, motion)]


@pytest.mark.parametrize("H,W", list(SIZES))
def test_identical_frames_give_the_identity_exactly(H, W):
    c = scene_case(H, W, "identity")
    est = c["est"]
    assert (est["M"] == E.IDENTITY12).all() and (est["pose"] == E.IDENTITY12.astype(F)).all()
    assert est["status"] == E.BIT_SMALL and est["info"][3] == 0 and est["info"][0] > 0.4 * H * W
    assert (est["trace"][:, 47] == E.BIT_SMALL).all()       # every step was below the pose's resolution, none was taken


@pytest.mark.parametrize("motion", ["forward", "yaw", "far"])
@pytest.mark.parametrize("H,W", list(SIZES))
def test_known_motions_are_recovered(H, W, motion):
    c = scene_case(H, W, motion)
    est = c["est"]
    et, er = E.motion_error(est["M"], c["true"])
    step = float(np.linalg.norm(c["true"].reshape(3, 4)[:, 3]))
    conds = [np.linalg.cond(E.unpack(tr[12:41])[0]) for tr in est["trace"]]
    print(f"{H}x{W} {motion}: error {et:.5f} m ({100 * et / step:.1f} % of the step), {er:.4f} deg; pixels {est['info'][0]:.0f}, rms "
          f"{est['info'][1]:.3f}, status {est['status']}, steps {est['info'][3]:.0f}, cond <= {max(conds):.3g}")
    bt, br = bound(H, W, motion)
    assert et <= bt and er <= br
    assert et <= 0.2 * step and er <= 0.5                   # what the feature was asked to stay under
    assert est["status"] & ~E.BIT_SMALL == 0 and max(conds) < MAX_COND
    inv = est["pose"][1].astype(np.float64).reshape(3, 4)   # pose[1] is the inverse of pose[0]
    both = E.compose(est["pose"][0].astype(np.float64).reshape(3, 4), inv)
    assert np.abs(both - E.IDENTITY12).max() <= 1e-6


def test_a_level_that_is_too_coarse_is_skipped_and_does_not_move_the_pose():
    """24 x 48 with 3 levels: the 6 x 12 level has fewer than min_pixels usable pixels; 12 x 24 with 3 levels: the 3 x 6 level is
    under 4 x 4.  Either way the level's steps carry code 1, M passes through them unchanged, and the finer levels still converge."""
    for (H, W), n_top in (((24, 48), None), ((12, 24), 0)):
        dz, yaw, dx = MOTIONS["forward"]
        T0, T1 = T.forward_pose(0, 0.0), T.forward_pose(1, dz, yaw, dx)
        rgb0, d0, mask, rgb1 = E.scene_pair(H, W, T0, T1)
        init = np.array([1, 0, 0, 0.01, 0, 1, 0, 0, 0, 0, 1, -0.2], F)
        est = E.estimate_image(rgb0, d0, mask == 1, rgb1, np.array(E.scene_cam(H, W), F), init=init, levels=3, iters=4,
                               min_pixels=64 if n_top is None else 16)
        top = est["trace"][:4]
        assert (top[:, 47] == E.BIT_FEW).all() and (top[:, :12] == init.astype(np.float64)).all() and (top[:, 41:47] == 0).all()
        assert (top[:, 40] < 64).all() and (n_top is None or (top[:, 40] == n_top).all())
        assert est["status"] & E.BIT_FEW and not est["status"] & E.BIT_FINAL_FEW
        assert (est["trace"][4:, 47] == 0).any()
        et, _ = E.motion_error(est["M"], E.true_motion(T0, T1))
        print(f"{H}x{W}: error {et:.4f} m after the skipped level")
        assert et <= 0.2 * 0.3


def test_pyramid_rules():
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    g = E.grey_of(rgb)
    wide = rgb.astype(np.int64)
    want = (77 * wide[..., 0] + 150 * wide[..., 1] + 29 * wide[..., 2]) / 256.0
    assert g.dtype == F and (g.astype(np.float64) == want).all()          # exact: an integer below 2^16 over 2^8
    assert E.down_grey(g).shape == (2, 3)
    d = np.full((4, 4), 8.0, F)
    d[0, 0], d[2, 3] = 9.5, np.nan                          # a jump of more than max_jump; a tap that is not finite
    ok = np.ones((4, 4), bool)
    ok[3, 0] = False                                        # a tap the mask drops
    assert E.down_disp(d, ok, 0.5, 1.0).tolist() == [[0.0, 8.0], [0.0, 0.0]]
    assert E.down_disp(d, np.ones((4, 4), bool), 0.5, 2.0).tolist() == [[8.375, 8.0], [8.0, 0.0]]
    fx, fy, cx, cy, fb = E.level_cam(np.array(T.SCENE_CAM, F), 2)
    assert (fx, fy, cx, cy, fb) == (30.0, 30.0, 11.5, 4.625, 60.0)       # pixel centres: (47.5 + 0.5) / 4 - 0.5


def _residual64(img, disp, cam, M, level=0):
    """(r, use, J) of the restatement run in float64 on the image `img` as the current one against a zero reference."""
    terms, use, _ = E.normal_image(np.zeros_like(img), disp, np.ones(img.shape, bool), img, cam, M, level, 0.5, 1e30, dt=np.float64)
    return terms[..., 0], use, terms[..., 2:]


def test_jacobian_against_finite_differences_of_the_residual():
    """d r / d delta for M <- exp(delta) . M, in float64.  On a ramp I = 2 x + 3 y + 5 the four-tap blend and the blended central
    differences are both exact, so J must meet the central finite difference of r to the difference's own error (h = 1e-6: h^2 and
    2^-53 |I| / h, far below 1e-6 of the largest entry).  On a wave A sin(kx x + ky y) the blended central difference is the
    gradient at (u, v) while the blend's own derivative is the one at the middle of the cell: with K = kx + ky they differ by at
    most e = A K^2 (1/2 + K/3) per component (half a pixel times the second derivative, plus the interpolation errors of either),
    so |FD - J| <= e (|du/d delta| + |dv/d delta|) + 1e-6 max|J|, the geometric factors taken from the ramps I = x and I = y."""
    H, W = 24, 48
    cam = np.array(E.scene_cam(H, W), F)
    disp = T.render(T.forward_pose(0, 0.0), H, W, E.scene_cam(H, W))
    M0 = E.compose(E.exp_se3(np.array([0.02, -0.01, -0.15, 0.004, 0.01, -0.003])), E.IDENTITY12)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    A, kx, ky = 40.0, 0.09, 0.06
    images = {"ramp": 2.0 * xs + 3.0 * ys + 5.0, "x": xs, "y": ys, "wave": A * np.sin(kx * xs + ky * ys + 0.3)}
    h = 1e-6
    out = {}
    for name, img in images.items():
        r0, use, J = _residual64(img, disp, cam, M0)
        fd = np.zeros_like(J)
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            rp, up, _ = _residual64(img, disp, cam, E.compose(E.exp_se3(d), M0))
            rm, um, _ = _residual64(img, disp, cam, E.compose(E.exp_se3(-d), M0))
            use = use & up & um
            fd[..., k] = (rp - rm) / (2 * h)
        out[name] = (J, fd, use)
    J, fd, use = out["ramp"]
    assert use.sum() > 300
    err = np.abs(fd - J)[use].max()
    print(f"ramp: max |FD - J| = {err:.3g} of max |J| = {np.abs(J[use]).max():.3g} over {use.sum()} pixels")
    assert err <= 1e-6 * np.abs(J[use]).max()
    Jw, fdw, usew = out["wave"]
    usew = usew & out["x"][2] & out["y"][2]
    K = kx + ky
    e = A * K * K * (0.5 + K / 3.0)
    allowed = e * (np.abs(out["x"][0]) + np.abs(out["y"][0])) + 1e-6 * np.abs(Jw[usew]).max()
    worst = (np.abs(fdw - Jw) / allowed)[usew].max()
    rel = np.abs(fdw - Jw)[usew].max() / np.abs(Jw[usew]).max()
    print(f"wave: max |FD - J| / allowed = {worst:.3f}; max |FD - J| = {rel:.3f} of max |J|")
    assert worst <= 1.0 and rel < 0.5


def test_exp_series_meets_the_closed_form_across_its_threshold():
    """Below 0.05 rad the series is truncated after t^6: the next term is t^8 / 9! < 2^-52 of the coefficient there; the closed
    form cancels: (1 - cos t) / t^2 and (t - sin t) / t^3 lose 2^-53 / (t^2 / 2) and 2^-53 / (t^2 / 6) relative, below 3e-13 at the
    threshold.  So both agree to 1e-12 on either side of it, and the exponential is a rotation and inverts with -delta."""
    for theta in (0.5 * E.SERIES_BELOW, np.nextafter(E.SERIES_BELOW, 0), E.SERIES_BELOW, 2 * E.SERIES_BELOW):
        a = np.array(E.exp_coefficients(theta, series=True))
        b = np.array(E.exp_coefficients(theta, series=False))
        assert np.abs(a / b - 1).max() <= (1e-12 if theta <= E.SERIES_BELOW else 1e-9), theta
    assert E.exp_coefficients(np.nextafter(E.SERIES_BELOW, 0)) == E.exp_coefficients(np.nextafter(E.SERIES_BELOW, 0), series=True)
    assert E.exp_coefficients(E.SERIES_BELOW) == E.exp_coefficients(E.SERIES_BELOW, series=False)
    assert (E.exp_se3(np.zeros(6)).reshape(12) == E.IDENTITY12).all()
    for delta in (np.array([0.3, -0.1, 0.8, 0.01, 0.03, -0.02]), np.array([0.1, 0.2, -0.3, 0.4, -0.5, 0.3])):
        Ex = E.exp_se3(delta)
        R = Ex[:, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-15 * 8 and abs(np.linalg.det(R) - 1) <= 1e-14
        assert np.abs(E.compose(E.exp_se3(-delta), Ex) - E.IDENTITY12).max() <= 1e-15 * 16
    # a pure translation and a pure rotation about y by the angle of forward_pose
    assert (E.exp_se3(np.array([1.0, 2.0, 3.0, 0, 0, 0]))[:, 3] == [1.0, 2.0, 3.0]).all()
    assert np.abs(E.exp_se3(np.array([0, 0, 0, 0, 0.3, 0]))[:, :3] - T.forward_pose(1, 0.0, yaw=0.3)[:, :3]).max() <= 1e-15


def test_update_codes():
    rng = np.random.default_rng(1)
    J = rng.normal(size=(200, 6))
    r = rng.normal(size=200)
    sums = np.concatenate([[(J[:, i] * J[:, j]).sum() for i, j in E.TRI], J.T @ r, [(r * r).sum(), 200.0]])
    M = E.IDENTITY12
    new, delta, code = E.update(sums, M, 0.0, 64)
    assert code == 0 and np.abs(delta - np.linalg.solve(J.T @ J, -(J.T @ r))).max() <= 1e-12
    assert np.abs(new - E.compose(E.exp_se3(delta), M)).max() == 0
    _, damped, _ = E.update(sums, M, 0.5, 64)
    assert np.abs(damped - np.linalg.solve(J.T @ J + 0.5 * np.diag(np.diag(J.T @ J)), -(J.T @ r))).max() <= 1e-12
    assert E.update(sums, M, 0.0, 201)[2] == E.BIT_FEW
    bad = sums.copy()
    bad[3] = np.inf
    assert E.update(bad, M, 0.0, 64)[2] == E.BIT_NONFINITE
    flat = np.zeros(29)
    flat[28] = 200.0
    out = E.update(flat, M, 0.0, 64)
    assert out[2] == E.BIT_SINGULAR and (out[0] == M).all() and (out[1] == 0).all()
    tiny = sums.copy()
    tiny[21:27] *= 1e-9
    out = E.update(tiny, M, 0.0, 64)
    assert out[2] == E.BIT_SMALL and (out[0] == M).all() and (out[1] != 0).any()


# ---- host pieces ----
def test_poses_writer_round_trip(tmp_path):
    from lwsnet_amd import egomotion, geometry
    rng = np.random.default_rng(5)
    poses = np.stack([E.compose(E.exp_se3(rng.normal(size=6) * 0.3), E.IDENTITY12).reshape(3, 4) for _ in range(6)])
    poses[0] = E.IDENTITY12.reshape(3, 4)
    path = str(tmp_path / "poses.txt")
    geometry.write_kitti_poses(path, poses)
    got = geometry.read_kitti_poses(path)
    assert got.dtype == np.float64 and (got == poses).all()                 # to the bit: repr() of a float64 reads back to it
    assert open(path).readline().split() == ["1.0", "0.0", "0.0", "0.0", "0.0", "1.0", "0.0", "0.0", "0.0", "0.0", "1.0", "0.0"]
    for bad in (poses[0], np.full((2, 3, 4), np.nan)):
        with pytest.raises(ValueError, match=r"poses must be finite \(N,3,4\)"):
            geometry.write_kitti_poses(path, bad)
    m = poses[3]
    assert np.abs(egomotion.compose(m, egomotion.invert(m)) - E.IDENTITY12.reshape(3, 4)).max() <= 1e-15 * 8
    assert (egomotion.invert(m).reshape(12) == E.inverse12(m)).all()
    t, deg = egomotion.motion_summary(T.forward_pose(1, 0.5, yaw=0.02).reshape(12))
    assert abs(t - 0.5) <= 1e-12 and abs(deg - np.degrees(0.02)) <= 1e-9


def _p(k, off=0):
    """Fake device pointers 1 GiB apart: never dereferenced, every call below is refused first."""
    return ctypes.c_void_p((1 << 40) + (k << 30) + off)


def test_ego_normal_rejects_bad_arguments(hip_lib):
    names = ("grey_ref", "disp_ref", "mask", "grey_cur", "cam", "M", "workspace", "sums", "terms")
    base = {name: _p(k) for k, name in enumerate(names)}
    INV = _lib.LWS_ERR_INVALID

    def call(B=1, H=8, W=16, level=0, min_disp=1.0, huber=10.0, **ptrs):
        a = {**base, **ptrs}
        return hip_lib.lws_ego_normal(a["grey_ref"], a["disp_ref"], a["mask"], a["grey_cur"], a["cam"], a["M"], B, H, W, level, min_disp, huber,
                                      a["workspace"], a["sums"], a["terms"], None)

    def at(name, off):
        return _p(names.index(name), off)

    w = b"ego_normal: "
    null_in = w + b"grey_ref, disp_ref, grey_cur, cam and M must not be null"
    al = w + b"grey_ref / disp_ref / grey_cur / cam / terms must be 4-byte, M / sums / workspace 8-byte aligned"
    nan = float("nan")
    for kw, msg in [
        (dict(grey_ref=None), null_in), (dict(disp_ref=None), null_in), (dict(grey_cur=None), null_in), (dict(cam=None), null_in), (dict(M=None), null_in),
        (dict(workspace=None), w + b"workspace and sums must not be null"), (dict(sums=None), w + b"workspace and sums must not be null"),
        (dict(B=0), w + b"bad shape B=0 H=8 W=16"), (dict(B=65536), w + b"bad shape B=65536 H=8 W=16"), (dict(H=0), w + b"bad shape B=1 H=0 W=16"),
        (dict(H=1 << 16, W=1 << 15), w + b"H*W = 65536x32768 must be < 2^31"),
        (dict(H=1, W=(1 << 24) + 1), w + b"H=1 W=16777217 exceed 16777216 (pixel coordinates are exact floats)"),
        (dict(level=-1), w + b"level -1 outside 0..7"), (dict(level=8), w + b"level 8 outside 0..7"),
        (dict(grey_ref=at("grey_ref", 2)), al), (dict(disp_ref=at("disp_ref", 1)), al), (dict(grey_cur=at("grey_cur", 3)), al), (dict(cam=at("cam", 2)), al),
        (dict(terms=at("terms", 2)), al), (dict(M=at("M", 4)), al), (dict(sums=at("sums", 4)), al), (dict(workspace=at("workspace", 4)), al),
        (dict(min_disp=0.0), w + b"min_disp must be finite and > 0, got 0"), (dict(min_disp=nan), w + b"min_disp must be finite and > 0, got nan"),
        (dict(huber=0.0), w + b"huber must be finite and > 0, got 0"), (dict(huber=float("inf")), w + b"huber must be finite and > 0, got inf"),
        (dict(terms=at("sums", 8 * 29 - 4)), w + b"terms and sums overlap"), (dict(workspace=at("terms", 32 * 128 - 8)), w + b"workspace and terms overlap"),
        (dict(grey_ref=at("sums", 0)), w + b"grey_ref and sums overlap"), (dict(disp_ref=at("terms", 0)), w + b"disp_ref and terms overlap"),
        (dict(mask=at("workspace", 0)), w + b"mask and workspace overlap"), (dict(grey_cur=at("sums", 4)), w + b"grey_cur and sums overlap"),
        (dict(cam=at("terms", 4)), w + b"cam and terms overlap"), (dict(M=at("workspace", 8)), w + b"M and workspace overlap"),
    ]:
        assert call(**kw) == INV, kw
        assert hip_lib.lws_last_error() == msg, (kw, hip_lib.lws_last_error())
    # inputs may share memory with each other: the next refusal is about something else
    assert call(grey_cur=at("grey_ref", 0), huber=0.0) == INV and hip_lib.lws_last_error() == w + b"huber must be finite and > 0, got 0"


def test_egomotion_rejects_bad_arguments(hip_lib):
    names = ("rgb_ref", "disp_ref", "mask", "rgb_cur", "cam", "init", "workspace", "pose", "status", "info", "trace", "resid")
    base = {name: _p(k) for k, name in enumerate(names)}
    INV = _lib.LWS_ERR_INVALID

    def call(B=1, H=8, W=16, levels=2, iters=3, min_disp=1.0, max_jump=1.0, huber=10.0, damping=0.0, min_pixels=16, **ptrs):
        a = {**base, **ptrs}
        return hip_lib.lws_egomotion(a["rgb_ref"], a["disp_ref"], a["mask"], a["rgb_cur"], a["cam"], a["init"], B, H, W, levels, iters, min_disp,
                                     max_jump, huber, damping, min_pixels, a["workspace"], a["pose"], a["status"], a["info"], a["trace"],
                                     a["resid"], None)

    def at(name, off):
        return _p(names.index(name), off)

    w = b"egomotion: "
    null_in = w + b"rgb_ref, disp_ref, rgb_cur and cam must not be null"
    null_out = w + b"workspace, pose, status and info must not be null"
    al = w + b"disp_ref / cam / init / pose / status / resid must be 4-byte, info / trace / workspace 8-byte aligned"
    nan = float("nan")
    for kw, msg in [
        (dict(rgb_ref=None), null_in), (dict(disp_ref=None), null_in), (dict(rgb_cur=None), null_in), (dict(cam=None), null_in),
        (dict(workspace=None), null_out), (dict(pose=None), null_out), (dict(status=None), null_out), (dict(info=None), null_out),
        (dict(B=0), w + b"bad shape B=0 H=8 W=16"), (dict(W=0), w + b"bad shape B=1 H=8 W=0"),
        (dict(H=1 << 16, W=1 << 15), w + b"H*W = 65536x32768 must be < 2^31"),
        (dict(H=(1 << 24) + 1, W=1), w + b"H=16777217 W=1 exceed 16777216 (pixel coordinates are exact floats)"),
        (dict(levels=0), w + b"levels 0 outside 1..8"), (dict(levels=9), w + b"levels 9 outside 1..8"),
        (dict(iters=0), w + b"iters 0 outside 1..64"), (dict(iters=65), w + b"iters 65 outside 1..64"),
        (dict(disp_ref=at("disp_ref", 2)), al), (dict(cam=at("cam", 1)), al), (dict(init=at("init", 2)), al), (dict(pose=at("pose", 2)), al),
        (dict(status=at("status", 2)), al), (dict(resid=at("resid", 1)), al), (dict(info=at("info", 4)), al), (dict(trace=at("trace", 4)), al),
        (dict(workspace=at("workspace", 4)), al),
        (dict(min_disp=0.0), w + b"min_disp must be finite and > 0, got 0"), (dict(max_jump=-1.0), w + b"max_jump must be >= 0 (+inf allowed), got -1"),
        (dict(max_jump=nan), w + b"max_jump must be >= 0 (+inf allowed), got nan"), (dict(huber=-2.0), w + b"huber must be finite and > 0, got -2"),
        (dict(damping=-0.5), w + b"damping must be finite and >= 0, got -0.5"), (dict(damping=float("inf")), w + b"damping must be finite and >= 0, got inf"),
        (dict(min_pixels=0), w + b"min_pixels 0 < 1"),
        (dict(status=at("pose", 92)), w + b"status and pose overlap"), (dict(info=at("status", 0)), w + b"info and status overlap"),
        (dict(trace=at("info", 24)), w + b"trace and info overlap"), (dict(resid=at("trace", 8 * 48 * 6 - 4)), w + b"resid and trace overlap"),
        (dict(workspace=at("resid", 4 * 128 - 8)), w + b"workspace and resid overlap"),
        (dict(rgb_ref=at("pose", 0)), w + b"rgb_ref and pose overlap"), (dict(disp_ref=at("resid", 0)), w + b"disp_ref and resid overlap"),
        (dict(mask=at("info", 0)), w + b"mask and info overlap"), (dict(rgb_cur=at("workspace", 64)), w + b"rgb_cur and workspace overlap"),
        (dict(cam=at("trace", 0)), w + b"cam and trace overlap"), (dict(init=at("status", 0)), w + b"init and status overlap"),
    ]:
        assert call(**kw) == INV, kw
        assert hip_lib.lws_last_error() == msg, (kw, hip_lib.lws_last_error())
    # the optional pointers may be null: the next refusal is about something else
    assert call(mask=None, init=None, trace=None, resid=None, huber=0.0) == INV
    assert hip_lib.lws_last_error() == w + b"huber must be finite and > 0, got 0"
    # the workspace: 16 state doubles and 29 per tile of 1024 pixels and image, three float pyramids, rounded up to 16 bytes
    ws = hip_lib.lws_egomotion_workspace
    assert ws(2, 40, 60, 1) == 8 * 2 * (16 + 29 * 3) + 4 * 3 * 2 * 2400
    assert ws(2, 40, 60, 3) == 8 * 2 * (16 + 29 * 3) + 4 * 3 * 2 * (2400 + 600 + 150)
    assert ws(1, 5, 7, 2) == (8 * (16 + 29) + 4 * 3 * (35 + 6) + 15) // 16 * 16
    assert ws(0, 5, 7, 1) == INV and hip_lib.lws_last_error() == b"egomotion_workspace: bad shape B=0 H=5 W=7"
    assert ws(1, 5, 7, 0) == INV and hip_lib.lws_last_error() == b"egomotion_workspace: levels 0 outside 1..8"
    assert ws(1, 5, 7, 9) == INV


def test_ops_and_odometry_validate_before_any_gpu_call():
    from lwsnet_amd import egomotion, ops
    from lwsnet_amd.geometry import Camera
    cam = Camera(120.0, 120.0, 47.5, 20.0, 0.5)
    z = np.zeros((1, 1, 4, 4), F)
    with pytest.raises(ValueError, match="egomotion needs cameras"):
        ops.egomotion(z, z, z, None)
    with pytest.raises(ValueError, match="ego_normal needs cameras"):
        ops.ego_normal(z, z, z, None, E.IDENTITY12)
    with pytest.raises(ValueError, match="Odometry needs cameras"):
        egomotion.Odometry(None)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.egomotion(z, z, z, cam)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.ego_normal(z, z, z, cam, E.IDENTITY12)
    bad = ((dict(levels=0), "levels must be an integer in 1 .. 8"), (dict(levels=9), "levels"), (dict(levels=2.5), "levels"),
           (dict(iters=0), "iters must be an integer in 1 .. 64"), (dict(iters=65), "iters"), (dict(min_disp=0.0), "min_disp must be finite and > 0"),
           (dict(max_jump=-1.0), "max_jump must be >= 0"), (dict(max_jump=float("nan")), "max_jump"), (dict(huber=0.0), "huber must be finite and > 0"),
           (dict(huber=float("inf")), "huber"), (dict(damping=-1.0), "damping must be finite and >= 0"), (dict(min_pixels=0), "min_pixels must be an integer in 1"))
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            ops.egomotion(None, None, None, cam, **kw)
        with pytest.raises(ValueError, match=msg):
            egomotion.Odometry(cam, **kw)
    for kw, msg in ((dict(level=8), "level must be an integer in 0 .. 7"), (dict(level=-1), "level"), (dict(huber=0.0), "huber must be finite and > 0")):
        with pytest.raises(ValueError, match=msg):
            ops.ego_normal(None, None, None, cam, E.IDENTITY12, **kw)
    for M, shape in ((np.zeros((4, 4)), r"\(4, 4\)"), (np.zeros((2, 12)), r"\(2, 12\)"), (np.full(12, np.nan), r"\(1, 12\)")):
        with pytest.raises(ValueError, match="M must be a finite .* got shape " + shape):
            ops._motion_rows(M, 1, "M", "float64")
    assert ops._motion_rows(E.IDENTITY12.reshape(3, 4), 3, "M", "float32").shape == (3, 12)
    assert ops._motion_rows(np.zeros((2, 3, 4)), 2, "M", "float64").dtype == np.float64
    assert ops.EgoResult._fields == ("pose", "status", "info", "trace", "resid") and ops.EGO_UNTRUSTED == E.BIT_FINAL_FEW
    assert ops.ego_args(4, 8, 1.0, float("inf"), 10.0, 0.0, 256) == (4, 8, 1.0, float("inf"), 10.0, 0.0, 256)
    odo = egomotion.Odometry(cam, levels=3, iters=5)
    assert odo.prev is None and odo.poses().shape == (0, 3, 4) and odo.params["levels"] == 3 and odo.params["min_pixels"] == 256


# ---- the inference CLI ----
NEW_FLAGS = ("egomotion", "ego_levels", "ego_iters", "ego_huber", "save_poses", "save_ego")


def test_egomotion_flags_default_off(tmp_path):
    from lwsnet_amd import inference
    p = inference.build_parser()
    a = p.parse_args([])
    assert not any(hasattr(a, name) for name in NEW_FLAGS)                      # the namespace of a line without them
    with_flags = vars(p.parse_args(["--egomotion", "--ego_levels", "3", "--ego_iters", "5", "--ego_huber", "8", "--save_poses", "x", "--save_ego"]))
    assert {k: v for k, v in with_flags.items() if k not in NEW_FLAGS} == vars(a)
    inference.check_geometry_arguments(p, a)
    inference.check_egomotion_arguments(p, a)
    inference.check_temporal_arguments(p, a)
    assert tuple(getattr(a, f) for f in NEW_FLAGS) == (False, 4, 8, 10.0, None, False)
    seq = _sequence_dir(tmp_path, 3)
    a = p.parse_args(seq + ["--egomotion", "--temporal", "--ego_levels", "3", "--save_ego", "--save_poses", str(tmp_path / "p.txt")] + CAMERA)
    inference.check_occ_arguments(p, a)
    inference.check_geometry_arguments(p, a)
    inference.check_egomotion_arguments(p, a)
    inference.check_temporal_arguments(p, a)                                    # --temporal without --poses: the estimate gives them
    assert a.egomotion and a.temporal and a.poses is None and (a.ego_levels, a.ego_iters, a.ego_huber) == (3, 8, 10.0) and a.save_ego


def test_cli_refuses_egomotion_without_what_it_needs(tmp_path, capsys):
    seq = _sequence_dir(tmp_path, 3)
    ok = seq + ["--egomotion"] + CAMERA
    assert _cli_refused(seq + ["--egomotion"], capsys).endswith(": error: --egomotion and --save_ego need a camera: --calib PATH or --camera FX FY CX CY BASELINE\n")
    assert _cli_refused(ok + ["--workers", "2"], capsys).endswith(": error: --egomotion / --save_ego run in the sequential mode only: use --workers 0\n")
    assert _cli_refused(["--left_img", str(tmp_path / "left_test.png"), "--egomotion"] + CAMERA, capsys).endswith(
        ": error: --egomotion follows a sequence: use directory mode (--img_path), not --left_img\n")
    needs = ": error: --ego_levels, --ego_iters, --ego_huber, --save_poses and --save_ego need --egomotion\n"
    for flags in (["--ego_levels", "3"], ["--ego_iters", "4"], ["--ego_huber", "5"], ["--save_poses", "p.txt"], ["--save_ego"]):
        assert _cli_refused(seq + flags + CAMERA, capsys).endswith(needs)
    for flags in (["--ego_levels", "0"], ["--ego_iters", "0"], ["--ego_huber", "0"]):            # a zero is a value given, not a flag left out
        assert _cli_refused(seq + flags + CAMERA, capsys).endswith(needs)
    assert _cli_refused(ok + ["--ego_levels", "0"], capsys).endswith(": error: --ego_levels must be in 1 .. 8, got 0\n")
    assert _cli_refused(ok + ["--ego_levels", "9"], capsys).endswith(": error: --ego_levels must be in 1 .. 8, got 9\n")
    assert _cli_refused(ok + ["--ego_iters", "65"], capsys).endswith(": error: --ego_iters must be in 1 .. 64, got 65\n")
    assert _cli_refused(ok + ["--ego_huber", "0"], capsys).endswith(": error: --ego_huber must be finite and > 0, got 0.0\n")
    assert _cli_refused(ok + ["--ego_huber", "nan"], capsys).endswith(": error: --ego_huber must be finite and > 0, got nan\n")
    poses = poses_file(tmp_path / "poses.txt", 3)
    assert _cli_refused(ok + ["--temporal", "--poses", poses], capsys).endswith(
        ": error: --temporal --egomotion takes the filter's poses from the estimate: do not give --poses as well\n")
    # --temporal alone keeps its text
    assert _cli_refused(seq + ["--temporal"] + CAMERA, capsys).endswith(": error: --temporal needs --poses PATH, the camera-to-world pose of every pair\n")
    assert not os.path.exists(tmp_path / "out")             # refused before the output folder is touched


def test_odometry_step_refuses_a_frame_that_does_not_match_the_previous_one():
    """The first step keeps the frame and estimates nothing (no GPU call), so the check of the second can be met on host tensors."""
    import torch
    from lwsnet_amd import egomotion
    from lwsnet_amd.geometry import Camera
    odo = egomotion.Odometry(Camera(120.0, 120.0, 47.5, 20.0, 0.5))
    rgb, disp, mask = torch.zeros((1, 4, 6, 3), dtype=torch.uint8), torch.ones((1, 1, 4, 6)), torch.ones((1, 1, 4, 6), dtype=torch.uint8)
    assert odo.step(rgb, disp, mask) is None and odo.poses().shape == (1, 3, 4) and (odo.poses()[0].reshape(12) == E.IDENTITY12).all()
    with pytest.raises(ValueError, match=r"Odometry.step: disp is \(1, 1, 4, 8\) with a mask, the previous frame \(1, 1, 4, 6\) with a mask \(reset\(\) first\)"):
        odo.step(torch.zeros((1, 4, 8, 3), dtype=torch.uint8), torch.ones((1, 1, 4, 8)), torch.ones((1, 1, 4, 8), dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"Odometry.step: disp is \(1, 1, 4, 6\), the previous frame \(1, 1, 4, 6\) with a mask"):
        odo.step(rgb, disp, None)
    assert odo.poses().shape == (1, 3, 4)                   # a refused step leaves the state as it was
    odo.reset()
    assert odo.step(torch.zeros((1, 4, 8, 3), dtype=torch.uint8), torch.ones((1, 1, 4, 8))) is None and odo.prev[2] is None


def test_a_skipped_pair_keeps_its_line_of_the_poses_file(tmp_path, caplog):
    """The pose source over a stub Odometry whose poses() grows by one per processed pair.  Pairs 0 and 3 of five are skipped: line i
    still belongs to pair i, a skipped pair repeating the pose before it (the identity where there is none), and each skip is
    warned about.  The world pose is the latest accumulated one; the filter is handed None on the first frame and, with a warning,
    for an estimate that is not to be trusted, else the estimate's own block."""
    import logging
    from types import SimpleNamespace
    from lwsnet_amd import geometry, ops, sequence
    poses = np.stack([T.forward_pose(k, 0.4, yaw=0.01) for k in range(3)])
    done, handed, block = [], [], np.zeros((1, 2, 12), F)
    src = sequence.PoseSource(5)
    src.odometry = SimpleNamespace(poses=lambda: poses[:len(done)])
    stage = sequence._Odometry(SimpleNamespace(save_poses=str(tmp_path / "p.txt")), src)
    log = logging.getLogger("test_egomotion_cpu")
    with caplog.at_level(logging.WARNING, logger=log.name):
        for index, name in enumerate(("a.png", "b.png", "c.png", "d.png", "e.png")):
            if index in (0, 3):
                stage.skip(name, log)
                continue
            done.append(index)                              # the stub's step
            src.frame(index)
            assert (src.world() == poses[len(done) - 1]).all()
            ego = None if len(done) == 1 else SimpleNamespace(status=[1 | (ops.EGO_UNTRUSTED if index == 2 else 0)], pose=block)
            handed.append(src.relative(SimpleNamespace(frame=SimpleNamespace(path=name), ego=ego), log))
    assert handed[0] is None and handed[1] is None and handed[2] is block
    skipped = "Egomotion: {} was skipped; its line of the poses file repeats the pose of the pair before it"
    assert [r.getMessage() for r in caplog.records] == [
        skipped.format("a.png"), "Temporal: the ego-motion estimate of c.png is not to be trusted (status 9): the filter starts anew", skipped.format("d.png")]
    assert stage.finish(log) == [str(tmp_path / "p.txt")]
    got = geometry.read_kitti_poses(str(tmp_path / "p.txt"))
    ident = E.IDENTITY12.reshape(3, 4)
    assert got.shape == (5, 3, 4) and (got == np.stack([ident, poses[0], poses[1], poses[1], poses[2]])).all()


def test_ego_file_helper():
    from lwsnet_amd import outputs
    u8 = outputs.ego_to_u8(np.array([[0.0, -0.4, 0.6], [-12.5, 254.6, -1e9]], F))
    assert u8.dtype == np.uint8 and u8.tolist() == [[0, 0, 1], [12, 255, 255]]
