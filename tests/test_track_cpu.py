"""Model tracking without a GPU: the numpy restatement (tests/track_reference.py) -- the point-to-plane Jacobian against finite
differences of its own float64 residual, geometric-only Gauss-Newton on a corner of three planes, the road-and-wall scene that
geometry alone leaves free along x and the joint cost pins down, the update's codes -- and the host pieces: argument errors of the C
ABI, of ops.track_normal / ops.track and of ModelTracker, the inference CLI's flags, the header's table."""
import ctypes
import os

import numpy as np
import pytest

import egomotion_reference as E
import temporal_reference as T
import track_reference as R
from cli_helpers import CAMERA, cli_refused as _cli_refused, poses_file, sequence_dir as _sequence_dir
from lwsnet_amd import _lib

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "lwsnet_track.h"
I34 = np.hstack([np.eye(3), np.zeros((3, 1))])
DELTA = np.array([0.05, -0.03, 0.1, 0.01, -0.02, 0.015])   # the twist the corner scene is moved by: translation (m), rotation (rad)
# Measured once with this restatement (printed by the tests): the corner scene's error after 10 geometric-only steps, metres and
# degrees -- float32 terms on 1152 pixels; the road-and-wall scene's geometric-only code (2: a pivot of exactly 0, there is no condition number to state;
# were it not singular, MIN_COND_GEOMETRIC is what is asked of it) and the joint cost's error.  The
# bounds below are ten times the corner's error (a wrong sign or a swapped cross product leaves centimetres and tenths of a degree)
# and twice the joint error, as test_egomotion_cpu.py bounds its own.
MEASURED = {"corner": (8.93e-5, 1.81e-3), "road_wall_code": 2, "road_wall_joint": (0.00438, 0.01643)}
MIN_COND_GEOMETRIC = 1e10                                   # what "free along x" means in numbers: a well-posed 6 x 6 here is below 1e5


def corner_pair(H=24, W=48, delta=DELTA):
    cam = E.scene_cam(H, W)
    T1 = R.motion_pose(delta)
    d0, n0 = R.planes_view(R.CORNER, I34, H, W, cam)
    d1, _ = R.planes_view(R.CORNER, T1, H, W, cam)
    return cam, d0, n0, d1, E.true_motion(I34, T1)


def test_the_three_planes_of_the_corner_are_all_seen():
    cam, d0, n0, d1, _ = corner_pair()
    assert (d0 > 0).all() and (d1 > 0).all()
    assert len(np.unique(np.round(n0.reshape(3, -1).T, 5), axis=0)) == 3 and (n0[2] <= 0).all()       # n.z < 0 faces the camera


def test_point_to_plane_jacobian_matches_finite_differences():
    """Jg against central differences of the float64 rg under M <- exp(eps e_k) . M, the association (iv, iu) and the
    standard deviation sz held as the header says.  rg is linear in the translation and smooth in the rotation: with eps = 1e-6 the
    truncation error is ~1e-12 of |J| and the rounding of the difference ~1e-16 / 1e-6 = 1e-10 of |rg|, so 1e-7 relative to the largest |J| is a wide berth."""
    cam, d0, n0, d1, Mtrue = corner_pair()
    H, W = d0.shape
    g = np.full((H, W), 100.0)
    ok = np.ones((H, W), bool)
    p = R.params(gate_g=np.inf, huber_g=1e6)
    M = E.compose(E.exp_se3(0.5 * DELTA), E.IDENTITY12)      # away from the minimum: the residuals are not small
    t0, _, use, _, taps = R.normal_image(g, d0, ok, n0, g, d1, None, ok, cam, M, p, dt=np.float64)
    assert use.sum() > 0.9 * H * W
    eps, worst = 1e-6, 0.0
    for k in range(6):
        e = np.zeros(6)
        e[k] = eps
        rp = R.normal_image(g, d0, ok, n0, g, d1, None, ok, cam, E.compose(E.exp_se3(e), M), p, dt=np.float64, taps=taps)[0][..., 8]
        rm = R.normal_image(g, d0, ok, n0, g, d1, None, ok, cam, E.compose(E.exp_se3(-e), M), p, dt=np.float64, taps=taps)[0][..., 8]
        fd = (rp - rm) / (2 * eps)
        worst = max(worst, np.abs(fd - t0[..., 10 + k])[use].max() / np.abs(t0[..., 10:])[use].max())
    print("Jg vs finite differences, relative:", worst)
    assert worst <= 1e-7


def test_what_the_jacobian_leaves_out_is_the_derivative_of_the_weight():
    """sz = sg Qz^2 / fb moves with M, and Jg holds it as a weight.  Finite differences of the float64 rg with sz free (the
    association still held) differ from Jg by -(2 rg / Qz) dQz / d delta, dQz / d delta = (0, 0, 1, Qy, -Qx, 0): proportional to the
    residual, so it vanishes where the residual does.  Same eps and berth as above, relative to the largest |Jg|."""
    cam, d0, n0, d1, _ = corner_pair()
    H, W = d0.shape
    g = np.full((H, W), 100.0)
    ok = np.ones((H, W), bool)
    p = R.params(gate_g=np.inf, huber_g=1e6)
    M = E.compose(E.exp_se3(0.5 * DELTA), E.IDENTITY12)
    t0, _, use, _, (iv, iu, _) = R.normal_image(g, d0, ok, n0, g, d1, None, ok, cam, M, p, dt=np.float64)
    fx, fy, cx, cy, fb = E.level_cam(cam, 0, np.float64)
    z = fb / d0.astype(np.float64)
    X, Y = (np.arange(W)[None, :] - cx) * z / fx, (np.arange(H)[:, None] - cy) * z / fy
    Qx, Qy, Qz = (T._row(M, k, X, Y, z) for k in range(3))
    dQz = [0.0 * Qz, 0.0 * Qz, 1.0 + 0.0 * Qz, Qy, -Qx, 0.0 * Qz]
    eps, worst, share = 1e-6, 0.0, 0.0
    scale = np.abs(t0[..., 10:])[use].max()

    def free(e):                                            # the association held, sz taken anew: taps[2] = None is not a held sz
        Me = E.compose(E.exp_se3(e), M)
        sz = R.normal_image(g, d0, ok, n0, g, d1, None, ok, cam, Me, p, dt=np.float64)[4][2]
        return R.normal_image(g, d0, ok, n0, g, d1, None, ok, cam, Me, p, dt=np.float64, taps=(iv, iu, sz))[0][..., 8]

    for k in range(6):
        e = np.zeros(6)
        e[k] = eps
        fd = (free(e) - free(-e)) / (2 * eps)
        left_out = -(2.0 * t0[..., 8] / Qz) * dQz[k]
        worst = max(worst, np.abs(fd - t0[..., 10 + k] - left_out)[use].max() / scale)
        share = max(share, np.abs(left_out)[use].max() / scale)
    print("what Jg leaves out, relative to the largest |Jg|:", share, "; unexplained:", worst)
    assert worst <= 1e-7 and share > 1e-4


def test_geometry_alone_recovers_a_motion_in_a_corner():
    """Three mutually non-parallel planes: the residual at the true motion is zero for any association that stays on one plane, so
    geometric-only Gauss-Newton (constant images: rp = 0 and Jp = 0 everywhere) finds it."""
    cam, d0, n0, d1, Mtrue = corner_pair()
    H, W = d0.shape
    g = np.full((H, W, 3), 100, np.uint8)
    ok = np.ones((H, W), bool)
    out = R.track_image(g, d0, n0, ok, g, d1, None, ok, cam, iters=10, gate_g=50.0, huber_g=50.0, min_pixels=16)
    err = E.motion_error(out["M"], Mtrue)
    print("corner:", err, out["status"], out["info"])
    assert out["status"] & ~E.BIT_SMALL == 0 and out["info"][2] > 0.9 * H * W and out["info"][1] == 0.0
    assert err[0] <= 10 * MEASURED["corner"][0] and err[1] <= 10 * MEASURED["corner"][1]
    assert np.array_equal(out["pose"][0], out["M"].astype(F)) and np.array_equal(out["pose"][1], E.inverse12(out["M"]).astype(F))


def road_wall_pair(H=48, W=96):
    """The road and a wall across it, both unbounded along x: nothing geometric changes when the camera slides along x."""
    cam = E.scene_cam(H, W)
    T0, T1 = T.forward_pose(0, 0.0), T.forward_pose(1, 0.2, yaw=0.01, dx=0.05)
    d0, n0 = R.planes_view(R.ROAD_WALL, T0, H, W, cam)
    d1, _ = R.planes_view(R.ROAD_WALL, T1, H, W, cam)
    rgb0, _, codes, rgb1 = E.scene_pair(H, W, T0, T1, cam)
    return cam, d0, n0, d1, rgb0, rgb1, E.true_motion(T0, T1)


def test_road_and_wall_leave_x_free_and_the_joint_cost_pins_it():
    cam, d0, n0, d1, rgb0, rgb1, Mtrue = road_wall_pair()
    H, W = d0.shape
    ok = (d0 > 0)
    flat = np.full((H, W, 3), 100, np.uint8)
    geo = R.track_image(flat, d0, n0, ok, flat, d1, None, d1 > 0, cam, iters=1, gate_g=50.0, huber_g=50.0, min_pixels=16)
    Hm, _ = E.unpack(geo["trace"][0][12:39])
    w = np.linalg.eigvalsh(Hm)
    cond = w[-1] / max(abs(w[0]), 1e-300)
    print("road and wall, geometric only: cond =", cond, "code", geo["trace"][0][50])
    assert geo["trace"][0][50] == E.BIT_SINGULAR or cond >= MIN_COND_GEOMETRIC
    assert abs(Hm[0, 0]) <= 1e-9 * Hm[2, 2]                 # no normal has an x component: translation along x is unseen
    # the same maps with the images: the joint cost recovers the motion.  The planes_view road has no far edge, the rendered scene's
    # wall is bounded: the geometric term meets the rendered disparity only where the two agree
    rgb0, dr, codes, rgb1 = E.scene_pair(H, W, T.forward_pose(0, 0.0), T.forward_pose(1, 0.2, yaw=0.01, dx=0.05), cam)
    d1r = T.render(T.forward_pose(1, 0.2, yaw=0.01, dx=0.05), H, W, cam).astype(F)
    n_model = np.where((np.abs(d0 - dr) < 1e-3)[None], n0, F(0))
    joint = R.track_image(rgb0, dr, n_model, codes == 1, rgb1, d1r, None, E.edge_codes(d1r) == 1, cam, iters=12, sigma0=0.1, min_pixels=64)
    err = E.motion_error(joint["M"], Mtrue)
    print("road and wall, joint:", err, joint["status"], joint["info"])
    assert joint["status"] & ~E.BIT_SMALL == 0 and joint["info"][0] > 1000 and joint["info"][2] > 500
    assert err[0] <= 2 * MEASURED["road_wall_joint"][0] and err[1] <= 2 * MEASURED["road_wall_joint"][1]


def test_update_codes():
    sums = np.zeros(32)
    Hm = np.diag([4.0, 5.0, 6.0, 7.0, 8.0, 9.0])
    for k, (i, j) in enumerate(E.TRI):
        sums[k] = Hm[i, j]
    sums[21:27] = [-0.4, 0.5, -0.6, 0.07, -0.08, 0.09]
    sums[28], sums[30] = 40, 30
    new, delta, code = R.update(sums, E.IDENTITY12, 0.0, 64)
    assert code == 0 and np.allclose(delta, [0.1, -0.1, 0.1, -0.01, 0.01, -0.01]) and np.allclose(new, E.exp_se3(delta).reshape(12))
    assert R.update(sums, E.IDENTITY12, 0.0, 71)[2] == E.BIT_FEW            # n_p + n_g = 70 is what is counted
    assert R.update(sums, E.IDENTITY12, 0.0, 70)[2] == 0
    for k in (0, 27, 29, 31):                               # every one of the 32 sums must be finite
        bad = sums.copy()
        bad[k] = np.inf
        assert R.update(bad, E.IDENTITY12, 0.0, 64)[2] == E.BIT_NONFINITE, k
    sing = sums.copy()
    sing[0] = 0.0
    assert R.update(sing, E.IDENTITY12, 0.0, 64)[2] == E.BIT_SINGULAR
    small = sums.copy()
    small[21:27] *= 1e-7
    M, d, code = R.update(small, E.IDENTITY12, 0.0, 64)
    assert code == E.BIT_SMALL and (M == E.IDENTITY12).all() and (d != 0).all()
    assert R.BIT_NO_MODEL == 32 and R.weights(R.params(sigma_p=4.0, lambda_g=0.5)) == (1.0 / 16.0, 0.5)


# ---- argument errors ----
def _p(k, off=0):
    """Fake device pointers 1 GiB apart: never dereferenced, every call below is refused first."""
    return ctypes.c_void_p((1 << 40) + (k << 30) + off)


SCALARS = dict(min_disp=1.0, huber_p=10.0, sigma_p=4.0, huber_g=1.5, gate_g=4.0, sigma0=0.5, sigma_min=0.05, lambda_g=1.0)
INF, NAN = float("inf"), float("nan")


def scalar_refusals(w):
    return [(dict(min_disp=0.0), w + b"min_disp must be finite and > 0, got 0"), (dict(min_disp=NAN), w + b"min_disp must be finite and > 0, got nan"),
            (dict(huber_p=0.0), w + b"huber_p must be finite and > 0, got 0"), (dict(huber_p=INF), w + b"huber_p must be finite and > 0, got inf"),
            (dict(sigma_p=0.0), w + b"sigma_p must be finite and > 0, got 0"), (dict(sigma_p=-1.0), w + b"sigma_p must be finite and > 0, got -1"),
            (dict(huber_g=0.0), w + b"huber_g must be finite and > 0, got 0"), (dict(huber_g=INF, gate_g=INF), w + b"huber_g must be finite and > 0, got inf"),
            (dict(gate_g=1.0), w + b"gate_g must be >= huber_g (+inf allowed), got 1 < 1.5"), (dict(gate_g=NAN), w + b"gate_g must be >= huber_g (+inf allowed), got nan < 1.5"),
            (dict(sigma0=-0.1), w + b"sigma0 must be finite and >= 0, got -0.1"), (dict(sigma0=INF), w + b"sigma0 must be finite and >= 0, got inf"),
            (dict(sigma_min=0.0), w + b"sigma_min must be finite and > 0, got 0"), (dict(lambda_g=-1.0), w + b"lambda_g must be finite and >= 0, got -1"),
            (dict(lambda_g=NAN), w + b"lambda_g must be finite and >= 0, got nan")]


def test_track_normal_rejects_bad_arguments(hip_lib):
    names = ("grey_ref", "disp_ref", "normals_ref", "mask_ref", "grey_cur", "disp_cur", "sigma_cur", "mask_cur", "cam", "M", "workspace", "sums", "terms")
    base = {name: _p(k) for k, name in enumerate(names)}
    INV = _lib.LWS_ERR_INVALID

    def call(B=1, H=8, W=16, **kw):
        a = {**base, **SCALARS, **kw}
        return hip_lib.lws_track_normal(*(a[n] for n in names[:10]), B, H, W, *(a[n] for n in SCALARS), a["workspace"], a["sums"], a["terms"], None)

    def at(name, off):
        return _p(names.index(name), off)

    w = b"track_normal: "
    null_in = w + b"grey_ref, disp_ref, grey_cur, disp_cur, cam and M must not be null"
    al = w + b"grey_ref / disp_ref / normals_ref / grey_cur / disp_cur / sigma_cur / cam / terms must be 4-byte, M / sums / workspace 8-byte aligned"
    for kw, msg in [
        *((dict([(n, None)]), null_in) for n in ("grey_ref", "disp_ref", "grey_cur", "disp_cur", "cam", "M")),
        (dict(workspace=None), w + b"workspace and sums must not be null"), (dict(sums=None), w + b"workspace and sums must not be null"),
        (dict(B=0), w + b"bad shape B=0 H=8 W=16"), (dict(B=65536), w + b"bad shape B=65536 H=8 W=16"), (dict(W=0), w + b"bad shape B=1 H=8 W=0"),
        (dict(H=1 << 16, W=1 << 15), w + b"H*W = 65536x32768 must be < 2^31"),
        (dict(H=1, W=(1 << 24) + 1), w + b"H=1 W=16777217 exceed 16777216 (pixel coordinates are exact floats)"),
        *((dict([(n, at(n, 2))]), al) for n in ("grey_ref", "disp_ref", "normals_ref", "grey_cur", "disp_cur", "sigma_cur", "cam", "terms")),
        (dict(M=at("M", 4)), al), (dict(sums=at("sums", 4)), al), (dict(workspace=at("workspace", 4)), al),
        *scalar_refusals(w),
        (dict(terms=at("sums", 8 * 32 - 4)), w + b"terms and sums overlap"), (dict(workspace=at("terms", 64 * 128 - 8)), w + b"workspace and terms overlap"),
        (dict(grey_ref=at("sums", 0)), w + b"grey_ref and sums overlap"), (dict(normals_ref=at("terms", 0)), w + b"normals_ref and terms overlap"),
        (dict(mask_ref=at("workspace", 0)), w + b"mask_ref and workspace overlap"), (dict(disp_cur=at("sums", 4)), w + b"disp_cur and sums overlap"),
        (dict(sigma_cur=at("terms", 4)), w + b"sigma_cur and terms overlap"), (dict(mask_cur=at("sums", 1)), w + b"mask_cur and sums overlap"),
        (dict(cam=at("terms", 4)), w + b"cam and terms overlap"), (dict(M=at("workspace", 8)), w + b"M and workspace overlap"),
    ]:
        assert call(**kw) == INV, kw
        assert hip_lib.lws_last_error() == msg, (kw, hip_lib.lws_last_error())
    # the optional pointers may be null, gate_g may be +inf, inputs may share memory: the next refusal is about something else
    assert call(normals_ref=None, mask_ref=None, sigma_cur=None, mask_cur=None, terms=None, gate_g=INF, grey_cur=at("grey_ref", 0), lambda_g=0.0,
                sigma_min=0.0) == INV
    assert hip_lib.lws_last_error() == w + b"sigma_min must be finite and > 0, got 0"
    # the workspace: 16 state doubles and 32 per tile of 1024 pixels and image, two grey images, rounded up to 16 bytes
    ws = hip_lib.lws_track_workspace
    assert ws(2, 40, 60) == 8 * 2 * (16 + 32 * 3) + 4 * 2 * 2 * 2400
    assert ws(1, 5, 7) == (8 * (16 + 32) + 4 * 2 * 35 + 15) // 16 * 16
    assert ws(0, 5, 7) == INV and hip_lib.lws_last_error() == b"track_workspace: bad shape B=0 H=5 W=7"
    assert ws(1, 1 << 16, 1 << 15) == INV


def test_track_rejects_bad_arguments(hip_lib):
    names = ("rgb_ref", "disp_ref", "normals_ref", "mask_ref", "rgb_cur", "disp_cur", "sigma_cur", "mask_cur", "cam", "init", "workspace", "pose",
             "status", "info", "trace", "resid")
    base = {name: _p(k) for k, name in enumerate(names)}
    INV = _lib.LWS_ERR_INVALID

    def call(B=1, H=8, W=16, iters=3, damping=0.0, min_pixels=16, **kw):
        a = {**base, **SCALARS, **kw}
        return hip_lib.lws_track(*(a[n] for n in names[:10]), B, H, W, iters, *(a[n] for n in SCALARS), damping, min_pixels,
                                 *(a[n] for n in names[10:]), None)

    def at(name, off):
        return _p(names.index(name), off)

    w = b"track: "
    null_in = w + b"rgb_ref, disp_ref, rgb_cur, disp_cur and cam must not be null"
    null_out = w + b"workspace, pose, status and info must not be null"
    al = (w + b"disp_ref / normals_ref / disp_cur / sigma_cur / cam / init / pose / status / resid must be 4-byte, info / trace / workspace "
          b"8-byte aligned")
    for kw, msg in [
        *((dict([(n, None)]), null_in) for n in ("rgb_ref", "disp_ref", "rgb_cur", "disp_cur", "cam")),
        *((dict([(n, None)]), null_out) for n in ("workspace", "pose", "status", "info")),
        (dict(B=0), w + b"bad shape B=0 H=8 W=16"), (dict(H=(1 << 24) + 1, W=1), w + b"H=16777217 W=1 exceed 16777216 (pixel coordinates are exact floats)"),
        (dict(iters=0), w + b"iters 0 outside 1..64"), (dict(iters=65), w + b"iters 65 outside 1..64"),
        *((dict([(n, at(n, 2))]), al) for n in ("disp_ref", "normals_ref", "disp_cur", "sigma_cur", "cam", "init", "pose", "status", "resid")),
        (dict(info=at("info", 4)), al), (dict(trace=at("trace", 4)), al), (dict(workspace=at("workspace", 4)), al),
        *scalar_refusals(w),
        (dict(damping=-0.5), w + b"damping must be finite and >= 0, got -0.5"), (dict(damping=INF), w + b"damping must be finite and >= 0, got inf"),
        (dict(min_pixels=0), w + b"min_pixels 0 < 1"),
        (dict(status=at("pose", 92)), w + b"status and pose overlap"), (dict(info=at("status", 0)), w + b"info and status overlap"),
        (dict(trace=at("info", 40)), w + b"trace and info overlap"), (dict(resid=at("trace", 8 * 51 * 3 - 4)), w + b"resid and trace overlap"),
        (dict(workspace=at("resid", 8 * 128 - 8)), w + b"workspace and resid overlap"),
        (dict(rgb_ref=at("pose", 0)), w + b"rgb_ref and pose overlap"), (dict(normals_ref=at("resid", 0)), w + b"normals_ref and resid overlap"),
        (dict(mask_ref=at("info", 0)), w + b"mask_ref and info overlap"), (dict(rgb_cur=at("workspace", 64)), w + b"rgb_cur and workspace overlap"),
        (dict(disp_cur=at("trace", 0)), w + b"disp_cur and trace overlap"), (dict(sigma_cur=at("pose", 4)), w + b"sigma_cur and pose overlap"),
        (dict(mask_cur=at("status", 0)), w + b"mask_cur and status overlap"), (dict(cam=at("trace", 0)), w + b"cam and trace overlap"),
        (dict(init=at("status", 0)), w + b"init and status overlap"),
    ]:
        assert call(**kw) == INV, kw
        assert hip_lib.lws_last_error() == msg, (kw, hip_lib.lws_last_error())
    assert call(normals_ref=None, mask_ref=None, sigma_cur=None, mask_cur=None, init=None, trace=None, resid=None, gate_g=INF, huber_p=0.0) == INV
    assert hip_lib.lws_last_error() == w + b"huber_p must be finite and > 0, got 0"


def test_ops_and_tracker_validate_before_any_gpu_call():
    import torch
    from lwsnet_amd import ops, tracking, tsdf
    from lwsnet_amd.geometry import Camera
    cam = Camera(120.0, 120.0, 47.5, 20.0, 0.5)
    z = np.zeros((1, 1, 4, 4), F)
    with pytest.raises(ValueError, match="track needs cameras"):
        ops.track(z, z, z, z, None)
    with pytest.raises(ValueError, match="track_normal needs cameras"):
        ops.track_normal(z, z, z, z, None, E.IDENTITY12)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.track(z, z, z, z, cam)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.track_normal(z, z, z, z, cam, E.IDENTITY12)
    bad = ((dict(min_disp=0.0), "min_disp must be finite and > 0"), (dict(huber_p=0.0), "huber_p must be finite and > 0"),
           (dict(sigma_p=float("inf")), "sigma_p must be finite and > 0"), (dict(huber_g=-1.0), "huber_g must be finite and > 0"),
           (dict(gate_g=1.0), "gate_g must be >= huber_g"), (dict(gate_g=NAN), "gate_g must be >= huber_g"), (dict(sigma0=-1.0), "sigma0 must be finite and >= 0"),
           (dict(sigma_min=0.0), "sigma_min must be finite and > 0"), (dict(lambda_g=-0.5), "lambda_g must be finite and >= 0"))
    more = ((dict(iters=0), "iters must be an integer in 1 .. 64"), (dict(iters=2.5), "iters"), (dict(damping=-1.0), "damping must be finite and >= 0"),
            (dict(min_pixels=0), "min_pixels must be an integer in 1"))

    class NoVolume(tsdf.TsdfVolume):
        def __init__(self):                                 # a volume without a device: the tracker's checks come before any use of it
            pass

    for kw, msg in bad + more:
        with pytest.raises(ValueError, match=msg):
            ops.track(None, None, None, None, cam, **kw)
        with pytest.raises(ValueError, match=msg):
            tracking.ModelTracker(NoVolume(), cam, **kw)
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            ops.track_normal(None, None, None, None, cam, E.IDENTITY12, **kw)
    for kw, msg in ((dict(w_min=-1.0), "w_min must be finite and >= 0"), (dict(z_near=0.0), "z_near must be finite and > 0")):
        with pytest.raises(ValueError, match=msg):
            tracking.ModelTracker(NoVolume(), cam, **kw)
    with pytest.raises(ValueError, match="ModelTracker needs a TsdfVolume"):
        tracking.ModelTracker(None, cam)
    with pytest.raises(ValueError, match="ModelTracker needs cameras"):
        tracking.ModelTracker(NoVolume(), None)
    assert ops.track_args(1.0, 10.0, 4.0, 1.5, INF, 0.0, 0.05, 0.0) == (1.0, 10.0, 4.0, 1.5, INF, 0.0, 0.05, 0.0)
    assert ops.TrackResult._fields == ("pose", "status", "info", "trace", "resid", "sums", "terms")
    assert ops.TRACK_UNTRUSTED == E.BIT_FINAL_FEW == ops.EGO_UNTRUSTED and ops.TRACK_NO_MODEL == R.BIT_NO_MODEL
    # the first step keeps the frame and estimates nothing (no GPU call), so the check of the second is met on host tensors
    trk = tracking.ModelTracker(NoVolume(), cam, iters=4)
    assert trk.params["iters"] == 4 and trk.params["min_pixels"] == 256 and trk.fill and trk.poses().shape == (0, 3, 4)
    rgb, disp = torch.zeros((1, 4, 6, 3), dtype=torch.uint8), torch.ones((1, 1, 4, 6))
    with pytest.raises(RuntimeError, match="HIP device"):
        trk.step(rgb, disp)
    assert trk.poses().shape == (0, 3, 4)


# ---- the inference CLI ----
NEW_FLAGS = ("tsdf_track", "track_iters", "track_lambda", "track_gate", "save_track")


def test_track_flags_default_off(tmp_path):
    from lwsnet_amd import inference, sequence
    assert sequence.TRACK_DEFAULTS == dict(tsdf_track=False, track_iters=6, track_lambda=1.0, track_gate=4.0, save_track=False)
    assert not set(NEW_FLAGS) & (set(sequence.TSDF_DEFAULTS) | set(sequence.EGO_DEFAULTS) | set(sequence.TEMPORAL_DEFAULTS))
    p = inference.build_parser()
    a = p.parse_args([])
    assert not any(hasattr(a, name) for name in NEW_FLAGS)                      # the namespace of a line without them
    with_flags = vars(p.parse_args(["--tsdf_track", "--track_iters", "3", "--track_lambda", "0.5", "--track_gate", "5", "--save_track"]))
    assert {k: v for k, v in with_flags.items() if k not in NEW_FLAGS} == vars(a)
    inference.check_tsdf_arguments(p, a)
    sequence.check_track_arguments(p, a)
    assert tuple(getattr(a, f) for f in NEW_FLAGS) == (False, 6, 1.0, 4.0, False)
    seq = _sequence_dir(tmp_path, 3)
    a = p.parse_args(seq + ["--egomotion", "--tsdf", "--tsdf_track", "--track_iters", "3", "--save_track"] + CAMERA)
    inference.check_occ_arguments(p, a)
    inference.check_geometry_arguments(p, a)
    inference.check_egomotion_arguments(p, a)
    inference.check_temporal_arguments(p, a)
    inference.check_tsdf_arguments(p, a)
    sequence.check_track_arguments(p, a)
    assert a.tsdf_track and a.save_track and (a.track_iters, a.track_lambda, a.track_gate) == (3, 1.0, 4.0)


def test_cli_refuses_tracking_without_what_it_needs(tmp_path, capsys):
    seq = _sequence_dir(tmp_path, 3)
    ok = seq + ["--egomotion", "--tsdf", "--tsdf_track"] + CAMERA
    assert _cli_refused(seq + ["--egomotion", "--tsdf_track"] + CAMERA, capsys).endswith(": error: --tsdf_track needs --tsdf, the volume it tracks against\n")
    poses = poses_file(tmp_path / "poses.txt", 3)
    assert _cli_refused(seq + ["--tsdf", "--poses", poses, "--tsdf_track"] + CAMERA, capsys).endswith(
        ": error: --tsdf_track estimates the poses: do not give --poses as well\n")
    assert _cli_refused(seq + ["--tsdf", "--tsdf_track"] + CAMERA, capsys).endswith(": error: --tsdf needs the pose of every pair: --poses PATH or --egomotion\n")
    assert _cli_refused(["--left_img", str(tmp_path / "left_test.png"), "--tsdf_track"] + CAMERA, capsys).endswith(
        ": error: --tsdf_track follows a sequence: use directory mode (--img_path), not --left_img\n")
    needs = ": error: --track_iters, --track_lambda, --track_gate and --save_track need --tsdf_track\n"
    for flags in (["--track_iters", "3"], ["--track_lambda", "0"], ["--track_gate", "5"], ["--save_track"]):
        assert _cli_refused(seq + ["--egomotion", "--tsdf"] + flags + CAMERA, capsys).endswith(needs)
    assert _cli_refused(ok + ["--track_iters", "0"], capsys).endswith(": error: --track_iters must be in 1 .. 64, got 0\n")
    assert _cli_refused(ok + ["--track_iters", "65"], capsys).endswith(": error: --track_iters must be in 1 .. 64, got 65\n")
    assert _cli_refused(ok + ["--track_lambda", "-1"], capsys).endswith(": error: --track_lambda must be finite and >= 0, got -1.0\n")
    assert _cli_refused(ok + ["--track_gate", "1"], capsys).endswith(": error: --track_gate must be in 1.5 .. inf, got 1.0\n")
    assert _cli_refused(ok + ["--track_gate", "nan"], capsys).endswith(": error: --track_gate must be in 1.5 .. inf, got nan\n")
    assert not os.path.exists(tmp_path / "out")             # refused before the output folder is touched


def test_the_pose_source_answers_from_the_tracker_while_it_is_on(tmp_path):
    import logging
    from types import SimpleNamespace
    from lwsnet_amd import geometry, ops, sequence
    chain = np.stack([T.forward_pose(k, 0.4, yaw=0.01) for k in range(3)])
    tracked = np.stack([T.forward_pose(k, 0.41, yaw=0.011) for k in range(3)])
    src = sequence.PoseSource(3)
    assert src.tracker is None
    src.odometry = SimpleNamespace(poses=lambda: chain)
    for k in range(3):
        src.frame(k)
    assert (src.world() == chain[2]).all() and (src.lines() == chain).all()
    src.tracker = SimpleNamespace(poses=lambda: tracked)
    assert (src.world() == tracked[2]).all() and (src.lines() == tracked).all()
    log = logging.getLogger("test_track_cpu")
    block = np.zeros((1, 2, 12), F)
    rec = lambda track: SimpleNamespace(frame=SimpleNamespace(path="x.png"), ego=SimpleNamespace(status=[ops.EGO_UNTRUSTED], pose=None), track=track)
    assert src.relative(rec(None), log) is None
    assert src.relative(rec(SimpleNamespace(status=[ops.TRACK_NO_MODEL | 16], pose=block)), log) is block
    assert src.relative(rec(SimpleNamespace(status=[ops.TRACK_UNTRUSTED], pose=block)), log) is None
    # the stage order: ego-motion, tracking, filter, volume
    assert [c.__name__ for c in (sequence._Odometry, sequence._Tracker, sequence._Sequence, sequence._Volume)] == ["_Odometry", "_Tracker", "_Sequence", "_Volume"]
    from lwsnet_amd import outputs
    rgb = outputs.track_to_rgb(np.array([[0.0, 4.0, -8.0, 2.0]]))
    assert rgb.tolist() == [[[0, 0, 0], [255, 0, 0], [0, 0, 255], [255, 128, 128]]]


# ---- the ABI ----
EXPECTED_NAMES = ["lws_track", "lws_track_normal", "lws_track_workspace"]


def test_the_header_is_read_into_a_table_of_its_own(hip_lib):
    from lwsnet_amd import build
    assert _lib.TRACK_HEADERS == (HEADER,) == tuple(_lib.TRACK_ABI)
    protos, spellings, path = _lib.TRACK_ABI[HEADER]
    assert os.path.samefile(path, os.path.join(ROOT, "include", HEADER))
    assert sorted(protos) == EXPECTED_NAMES == sorted(spellings) and protos == _lib.TRACK_PROTOTYPES
    c, v, i, f = ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert protos["lws_track_workspace"] == (ctypes.c_int64, [i, i, i])
    assert protos["lws_track_normal"] == (i, [v] * 10 + [i] * 3 + [f] * 8 + [v] * 4)
    assert protos["lws_track"] == (i, [v] * 10 + [i] * 4 + [f] * 9 + [i] + [v] * 7)
    for name, (res, args) in protos.items():
        fn = getattr(hip_lib, name)
        assert fn.argtypes == args and fn.restype is res, name
    assert spellings["lws_track_normal"][1][9] == "const double *" and spellings["lws_track"][1][-4:] == ["double *", "double *", "float *", "void *"]
    assert "lws_track.hip" in build.SOURCES and hip_lib.lws_abi_version() == 8 == _lib.LWS_ABI_VERSION
    # the tables the other tests count are what they were
    assert len(_lib.HEADERS) == 5 == len(_lib.ABI) and HEADER not in _lib.HEADERS and len(_lib.PROTOTYPES) == 67 and len(_lib.ALL_PROTOTYPES) == 78
    assert _lib.MESH_HEADERS == ("lwsnet_tsdf_mesh.h",) and not set(protos) & (set(_lib.ALL_PROTOTYPES) | set(_lib.MESH_PROTOTYPES))
    assert sorted(_lib.ABI["lwsnet_egomotion.h"][0]) == ["lws_ego_normal", "lws_egomotion", "lws_egomotion_workspace"]


def test_a_compiler_agrees_with_the_reading_of_the_header(tmp_path):
    from test_abi_cpu import _assert_line, compiles
    spellings = _lib.TRACK_ABI[HEADER][1]
    lines = {name: _assert_line(name, sp) for name, sp in spellings.items()}
    ok = compiles(HEADER, tmp_path / "track.cpp", lines.values())
    assert ok.returncode == 0, ok.stderr
    ret, params = spellings["lws_track"]
    assert params[13] == "int" and params[14] == "float"           # iters, min_disp
    flipped = dict(lines, lws_track=_assert_line("lws_track", (ret, params[:13] + ["float"] + params[14:])))
    bad = compiles(HEADER, tmp_path / "track_flipped.cpp", flipped.values())
    assert bad.returncode != 0 and '"lws_track"' in bad.stderr and bad.stderr.count("error:") == 1, bad.stderr


# ---- the benchmark tool ----
def test_the_benchmark_tool_takes_its_method_from_benchkit():
    """tools/benchtrack.py under the rule tests/test_benchkit_cpu.py holds tools/*bench.py to: it compiles, imports benchkit, and
    neither defines nor borrows a timing method of its own."""
    import ast
    from test_benchkit_cpu import _names
    path = os.path.join(ROOT, "tools", "benchtrack.py")
    with open(path) as f:
        src = f.read()
    compile(src, path, "exec")
    tree = ast.parse(src)
    defs = {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}
    assert not defs & {"timed", "n_sets"}, defs
    stored = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store)}
    assert "HBM_TBS" not in stored
    used = set(_names(tree))
    assert not used & {"Event", "lws_clock_read", "lws_profile_read", "lws_clock_stamp", "lws_profile_enable"}, used
    imports = {a.name for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom)) for a in n.names}
    assert "benchkit" in imports
    assert {"lws_track", "lws_track_normal", "lws_ego_normal"} <= used
