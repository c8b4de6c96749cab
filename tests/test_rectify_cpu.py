"""The rectifying front end without a GPU: the geometry of the map against a forward projection of 3-D points (the direction of
R_rect and of the inverse, which a test against one's own restatement cannot see), the float32 map against float64, the identity
and integer-shift calibrations on the numpy restatement (tests/rectify_reference.py), RectifyCalib.from_kitti, the argument errors
of lws_rectify_pair through the C ABI and the CLI flags."""
import ctypes

import numpy as np
import pytest

import rectify_reference as R
from lwsnet_amd import _lib
from lwsnet_amd.geometry import Camera, RectifyCalib, rectify_params

KITTI_K = (721.5377, 721.5377, 609.5593, 172.854)          # fx, fy, cx, cy of KITTI-2015's P_rect_02
HW = (375, 1242)


def plain_calib(p_cx=KITTI_K[2], p_cy=KITTI_K[3], hw=HW):
    """No distortion, no rotation, P[:, :3] = K up to the principal point (p_cx, p_cy)."""
    fx, fy, cx, cy = KITTI_K
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    P = np.array([[fx, 0, p_cx, 0], [0, fy, p_cy, 0], [0, 0, 1.0, 0]])
    P2 = P.copy()
    P2[0, 3] = -fx * 0.54
    return RectifyCalib(hw, hw, (K, K), (np.zeros(5), np.zeros(5)), (np.eye(3), np.eye(3)), (P, P2))


def random_raw(B, H, W, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8) for _ in range(2))


def test_map_geometry_against_forward_projection():
    calib, (K1, D1, K2, D2, Rm, T) = R.kitti_like_calib()
    rng = np.random.default_rng(0)
    Z = rng.uniform(5.0, 80.0, 200)
    pts = np.stack([rng.uniform(-0.45, 0.45, 200) * Z, rng.uniform(-0.15, 0.15, 200) * Z, Z], axis=1)   # in the left raw camera
    ref = np.concatenate([pts @ calib.R_rect[0].T, np.ones((200, 1))], axis=1)          # in the rectified left camera, homogeneous
    rows, cols = [], []
    for cam, (K, D, x) in enumerate(((K1, D1, pts), (K2, D2, pts @ Rm.T + T))):
        xd, yd = R.distort64(x[:, 0] / x[:, 2], x[:, 1] / x[:, 2], D)                   # the raw pixel the camera really sees
        raw_u, raw_v = K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]
        h = ref @ calib.P_rect[cam].T                                                   # KITTI's rule: P_rect_xx of the reference frame
        u, v = h[:, 0] / h[:, 2], h[:, 1] / h[:, 2]
        sx, sy = R.rectify_map64(calib, cam, u, v)
        err = max(np.abs(sx - raw_u).max(), np.abs(sy - raw_v).max())
        print(f"camera {cam}: |map(rectified) - raw| = {err:.3e} px")
        assert err < 1e-6
        rows.append(v)
        cols.append(u)
    assert np.abs(rows[0] - rows[1]).max() < 1e-6, "the two rectified rows of a point must agree"
    assert np.abs((cols[0] - cols[1]) * ref[:, 2] / calib.camera().fb - 1.0).max() < 1e-6, "x_left - x_right = fb / Z"


def test_right_view_is_the_left_view_shifted_along_the_baseline():
    """x2_rect = R_rect[1] (R x1 + T) = R_rect[0] x1 + (P_right[0,3] / f, 0, 0): the identity the test above relies on."""
    calib, (_, _, _, _, Rm, T) = R.kitti_like_calib()
    x1 = np.random.default_rng(1).uniform(-10, 10, (50, 3)) + [0, 0, 30]
    a = (x1 @ Rm.T + T) @ calib.R_rect[1].T
    b = x1 @ calib.R_rect[0].T + [calib.P_rect[1][0, 3] / calib.P_rect[1][0, 0], 0, 0]
    assert np.abs(a - b).max() < 1e-9
    assert calib.P_rect[1][0, 3] == pytest.approx(-calib.P_rect[0][0, 0] * np.linalg.norm(T), rel=1e-12)
    f = min(958.7, 955.1)
    assert calib.P_rect[0][0, 0] == f and calib.P_rect[0][1, 1] == f and calib.rect_hw == calib.raw_hw == HW
    assert calib.P_rect[0][0, 2] == pytest.approx(0.5 * (612.4 + 606.8)) and calib.P_rect[0][1, 2] == pytest.approx(0.5 * (181.9 + 176.3))


def test_float32_map_against_float64():
    calib, _ = R.kitti_like_calib()
    H, W = HW
    params = calib.params()
    assert params.shape == (2, 18) and params.dtype == np.float32
    want = R.rectify_reference(random_raw(1, 8, 8, 0), params[None], HW)["map"]
    xr, yr = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    for cam in range(2):
        sx, sy = R.rectify_map64(calib, cam, xr, yr, params=params)
        ex, ey = np.abs(want[cam][0, :, :, 0] - sx).max(), np.abs(want[cam][0, :, :, 1] - sy).max()
        print(f"camera {cam}: float32 map against float64: {ex:.2e} px in x, {ey:.2e} px in y")
        assert ex < 1e-3 and ey < 1e-3


def test_identity_calibration_copies_the_image():
    H, W = HW
    raw = random_raw(1, H, W, 2)
    out = R.rectify_reference(raw, rectify_params(plain_calib(), 1), HW, border=77)
    for cam in range(2):
        assert np.array_equal(out["rect"][cam], raw[cam])
        want = np.ones((1, 1, H, W), np.uint8)
        want[:, :, -1, :] = 0
        want[:, :, :, -1] = 0
        assert np.array_equal(out["valid"][cam], want)
        u = np.arange(W, dtype=np.float32)[None, :]
        assert np.abs(out["map"][cam][0, :, :, 0] - u).max() < 1.0 / 64


@pytest.mark.parametrize("dx,dy", [(5, 3), (-7, 2), (4, -6), (0, 0)])
def test_integer_shift_of_the_principal_point(dx, dy):
    """P's principal point moved by (dx, dy): rect[v, u] = raw[v - dy, u - dx], `border` where that falls outside."""
    H, W = 41, 67
    raw = random_raw(2, H, W, 3)
    cx, cy = KITTI_K[2:]
    out = R.rectify_reference(raw, rectify_params(plain_calib(cx + dx, cy + dy, (H, W)), 2), (H, W), border=200)
    for cam in range(2):
        want = np.full((2, H, W, 3), 200, np.uint8)
        ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0))
        yd, xd = slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), W + min(-dx, 0))
        want[:, ys, xs] = raw[cam][:, yd, xd]
        assert np.array_equal(out["rect"][cam], want), (cam, dx, dy)
        inside = np.zeros((2, 1, H, W), np.uint8)
        inside[:, :, max(dy, 0):min(H, H - 1 + dy), max(dx, 0):min(W, W - 1 + dx)] = 1     # 0 <= u - dx <= W - 2, the same in y
        assert np.array_equal(out["valid"][cam], inside), (cam, dx, dy)


def test_input_is_the_preprocess_transform_of_rect():
    from lwsnet_amd import imageio as io
    raw = random_raw(1, 20, 30, 4)
    out = R.rectify_reference(raw, rectify_params(R.kitti_like_calib((20, 30))[0], 1), (20, 30))
    for cam in range(2):
        assert np.array_equal(out["input"][cam][0].view(np.uint32), io.to_input(out["rect"][cam][0]).view(np.uint32))


def test_from_kitti_round_trip(tmp_path):
    calib, _ = R.kitti_like_calib()
    path = R.write_kitti(tmp_path / "calib_cam_to_cam.txt", calib)
    back = RectifyCalib.from_kitti(path)
    assert back.raw_hw == calib.raw_hw and back.rect_hw == calib.rect_hw
    for name in ("K", "D", "R_rect", "P_rect"):
        for cam in range(2):
            assert np.array_equal(getattr(back, name)[cam], getattr(calib, name)[cam]), name
    assert np.array_equal(back.params().view(np.uint32), calib.params().view(np.uint32))
    assert back.camera() == Camera.from_kitti(path) == calib.camera()
    assert rectify_params(back, 3).shape == (3, 2, 18) and rectify_params([back, calib], 2).shape == (2, 2, 18)
    with pytest.raises(ValueError, match="list of 2"):
        rectify_params([back], 2)


def test_from_kitti_names_the_missing_key(tmp_path):
    calib, _ = R.kitti_like_calib()
    with pytest.raises(ValueError, match="missing key D_02"):
        RectifyCalib.from_kitti(R.write_kitti(tmp_path / "a.txt", calib, skip=("D_02",)))
    with pytest.raises(ValueError, match="missing key K_03"):
        RectifyCalib.from_kitti(R.write_kitti(tmp_path / "b.txt", calib, skip=("K_03",)))


def test_check_rejects_a_broken_calibration():
    good = plain_calib()
    for field, cam, value in (("K", 0, np.diag([0.0, 700.0, 1.0])), ("D", 1, np.array([np.nan, 0, 0, 0, 0])),
                              ("P_rect", 0, np.zeros((3, 4))), ("R_rect", 1, np.zeros((3, 3)))):
        pair = list(getattr(good, field))
        pair[cam] = value
        kw = {n: getattr(good, n) for n in ("raw_hw", "rect_hw", "K", "D", "R_rect", "P_rect")}
        kw[field] = tuple(pair)
        with pytest.raises(ValueError):
            RectifyCalib(**kw).check()
    with pytest.raises(ValueError, match="to the right"):
        RectifyCalib.from_rig(np.eye(3), np.zeros(5), np.eye(3), np.zeros(5), np.eye(3), [0.5, 0, 0], (8, 8))


def test_library_exports_the_entry_point(hip_lib):
    assert hip_lib.lws_rectify_pair.argtypes == _lib.PROTOTYPES["lws_rectify_pair"][1]
    assert hip_lib.lws_abi_version() == 8


def _call(lib, raw=(1 << 20, 1 << 24), params=1 << 28, B=1, Hs=8, Ws=8, H=4, W=4, x0=0, y0=0, border=0, std=(0.229, 0.224, 0.225),
          rect=(1 << 30, None), inp=(None, None), valid=(None, None), mp=(None, None)):
    """lws_rectify_pair with made-up (never dereferenced) device addresses: every argument error returns before any GPU call."""
    arr = lambda pair: (ctypes.c_void_p * 2)(*pair)       # noqa: E731
    mean = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
    return lib.lws_rectify_pair(arr(raw), params, B, Hs, Ws, H, W, x0, y0, border, mean, (ctypes.c_float * 3)(*std), arr(rect), arr(inp),
                                arr(valid), arr(mp), None)


def test_argument_errors_through_the_c_abi(hip_lib):
    lib = hip_lib
    bad = [(dict(raw=(None, 1 << 24)), b"raw"), (dict(raw=(1 << 20, None)), b"raw"), (dict(rect=(None, None)), b"no output"),
           (dict(border=256), b"border"), (dict(border=-1), b"border"), (dict(inp=(1 << 32, None), std=(0.229, 0.0, 0.225)), b"std[1]"),
           (dict(B=0), b"B = 0"), (dict(B=32768), b"B = 32768"), (dict(Ws=16385), b"raw size"), (dict(Hs=16385), b"raw size"),
           (dict(Hs=0), b"raw size"), (dict(H=0), b"window"), (dict(x0=-1), b"window"), (dict(y0=-1), b"window"),
           (dict(x0=32765), b"window"), (dict(y0=32765), b"window"), (dict(params=None), b"params"),
           (dict(rect=(1 << 20, None)), b"raw[0] and rect[0] overlap"), (dict(rect=((1 << 20) + 100, None)), b"overlap"),
           (dict(rect=(None, 1 << 24)), b"raw[1] and rect[1] overlap"), (dict(valid=(1 << 28, None)), b"params and valid[0] overlap"),
           (dict(mp=((1 << 30) + 40, None)), b"map[0] and rect[0] overlap"), (dict(inp=(1 << 32, (1 << 32) + 64)), b"input[1] and input[0]"),
           (dict(inp=((1 << 32) + 2, None)), b"aligned"), (dict(params=(1 << 28) + 1), b"aligned")]
    for kw, word in bad:
        assert _call(lib, **kw) == _lib.LWS_ERR_INVALID, kw
        msg = lib.lws_last_error()
        assert msg.startswith(b"rectify_pair:") and word in msg, (kw, msg)
        with pytest.raises(ValueError, match="rectify_pair"):
            _lib.check(_lib.LWS_ERR_INVALID)
    # std is not looked at when no input is requested
    assert _call(lib, std=(0.0, 0.0, 0.0), border=300) == _lib.LWS_ERR_INVALID and b"border" in lib.lws_last_error()


# (moved buffer, the written buffer it is moved 4 bytes into, the whole error): every written / any pair of the table, each alone
_OVERLAPS = [
    ("rect[1]", "rect[0]", b"rectify_pair: rect[1] and rect[0] overlap"),
    ("input[0]", "rect[0]", b"rectify_pair: input[0] and rect[0] overlap"),
    ("input[1]", "rect[0]", b"rectify_pair: input[1] and rect[0] overlap"),
    ("valid[0]", "rect[0]", b"rectify_pair: valid[0] and rect[0] overlap"),
    ("valid[1]", "rect[0]", b"rectify_pair: valid[1] and rect[0] overlap"),
    ("map[0]", "rect[0]", b"rectify_pair: map[0] and rect[0] overlap"), ("map[1]", "rect[0]", b"rectify_pair: map[1] and rect[0] overlap"),
    ("raw[0]", "rect[0]", b"rectify_pair: raw[0] and rect[0] overlap"), ("raw[1]", "rect[0]", b"rectify_pair: raw[1] and rect[0] overlap"),
    ("params", "rect[0]", b"rectify_pair: params and rect[0] overlap"),
    ("input[0]", "rect[1]", b"rectify_pair: input[0] and rect[1] overlap"),
    ("input[1]", "rect[1]", b"rectify_pair: input[1] and rect[1] overlap"),
    ("valid[0]", "rect[1]", b"rectify_pair: valid[0] and rect[1] overlap"),
    ("valid[1]", "rect[1]", b"rectify_pair: valid[1] and rect[1] overlap"),
    ("map[0]", "rect[1]", b"rectify_pair: map[0] and rect[1] overlap"), ("map[1]", "rect[1]", b"rectify_pair: map[1] and rect[1] overlap"),
    ("raw[0]", "rect[1]", b"rectify_pair: raw[0] and rect[1] overlap"), ("raw[1]", "rect[1]", b"rectify_pair: raw[1] and rect[1] overlap"),
    ("params", "rect[1]", b"rectify_pair: params and rect[1] overlap"),
    ("input[1]", "input[0]", b"rectify_pair: input[1] and input[0] overlap"),
    ("valid[0]", "input[0]", b"rectify_pair: valid[0] and input[0] overlap"),
    ("valid[1]", "input[0]", b"rectify_pair: valid[1] and input[0] overlap"),
    ("map[0]", "input[0]", b"rectify_pair: map[0] and input[0] overlap"),
    ("map[1]", "input[0]", b"rectify_pair: map[1] and input[0] overlap"),
    ("raw[0]", "input[0]", b"rectify_pair: raw[0] and input[0] overlap"),
    ("raw[1]", "input[0]", b"rectify_pair: raw[1] and input[0] overlap"),
    ("params", "input[0]", b"rectify_pair: params and input[0] overlap"),
    ("valid[0]", "input[1]", b"rectify_pair: valid[0] and input[1] overlap"),
    ("valid[1]", "input[1]", b"rectify_pair: valid[1] and input[1] overlap"),
    ("map[0]", "input[1]", b"rectify_pair: map[0] and input[1] overlap"),
    ("map[1]", "input[1]", b"rectify_pair: map[1] and input[1] overlap"),
    ("raw[0]", "input[1]", b"rectify_pair: raw[0] and input[1] overlap"),
    ("raw[1]", "input[1]", b"rectify_pair: raw[1] and input[1] overlap"),
    ("params", "input[1]", b"rectify_pair: params and input[1] overlap"),
    ("valid[1]", "valid[0]", b"rectify_pair: valid[1] and valid[0] overlap"),
    ("map[0]", "valid[0]", b"rectify_pair: map[0] and valid[0] overlap"),
    ("map[1]", "valid[0]", b"rectify_pair: map[1] and valid[0] overlap"),
    ("raw[0]", "valid[0]", b"rectify_pair: raw[0] and valid[0] overlap"),
    ("raw[1]", "valid[0]", b"rectify_pair: raw[1] and valid[0] overlap"),
    ("params", "valid[0]", b"rectify_pair: params and valid[0] overlap"),
    ("map[0]", "valid[1]", b"rectify_pair: map[0] and valid[1] overlap"),
    ("map[1]", "valid[1]", b"rectify_pair: map[1] and valid[1] overlap"),
    ("raw[0]", "valid[1]", b"rectify_pair: raw[0] and valid[1] overlap"),
    ("raw[1]", "valid[1]", b"rectify_pair: raw[1] and valid[1] overlap"),
    ("params", "valid[1]", b"rectify_pair: params and valid[1] overlap"), ("map[1]", "map[0]", b"rectify_pair: map[1] and map[0] overlap"),
    ("raw[0]", "map[0]", b"rectify_pair: raw[0] and map[0] overlap"), ("raw[1]", "map[0]", b"rectify_pair: raw[1] and map[0] overlap"),
    ("params", "map[0]", b"rectify_pair: params and map[0] overlap"), ("raw[0]", "map[1]", b"rectify_pair: raw[0] and map[1] overlap"),
    ("raw[1]", "map[1]", b"rectify_pair: raw[1] and map[1] overlap"), ("params", "map[1]", b"rectify_pair: params and map[1] overlap"),
]


def test_every_overlapping_pair_is_named(hip_lib):
    names = ["rect[0]", "rect[1]", "input[0]", "input[1]", "valid[0]", "valid[1]", "map[0]", "map[1]", "raw[0]", "raw[1]", "params"]
    base = {n: (k + 1) << 24 for k, n in enumerate(names)}
    assert len({frozenset(c[:2]) for c in _OVERLAPS}) == len(_OVERLAPS) == sum(10 - i for i in range(8))
    for moved, onto, msg in _OVERLAPS:
        a = {**base, moved: base[onto] + 4}
        pair = lambda n: (a[n + "[0]"], a[n + "[1]"])         # noqa: E731
        rc = _call(hip_lib, raw=pair("raw"), params=a["params"], rect=pair("rect"), inp=pair("input"), valid=pair("valid"), mp=pair("map"))
        assert rc == _lib.LWS_ERR_INVALID, (moved, onto)
        assert hip_lib.lws_last_error() == msg


def test_shared_checks_keep_their_whole_text(hip_lib):
    cases = [(dict(inp=((1 << 32) + 2, None)), b"rectify_pair: params, input and map must be 4-byte aligned"),
             (dict(mp=(None, (1 << 33) + 1)), b"rectify_pair: params, input and map must be 4-byte aligned"),
             (dict(params=(1 << 28) + 1), b"rectify_pair: params, input and map must be 4-byte aligned")]
    for kw, msg in cases:
        assert _call(hip_lib, **kw) == _lib.LWS_ERR_INVALID, kw
        assert hip_lib.lws_last_error() == msg, kw


def test_ops_validates_before_the_library():
    from lwsnet_amd import ops
    z = np.zeros((1, 8, 8, 3), np.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.rectify_pair(z, z, np.zeros((1, 2, 18), np.float32), (4, 4))


ARGV_ERRORS = [["--save_rect"], ["--rectify", "calib.txt", "--workers", "4"], ["--rectify", "no/such/file.txt"]]


@pytest.mark.parametrize("argv", ARGV_ERRORS)
def test_cli_argument_errors(argv, capsys, monkeypatch, tmp_path):
    from lwsnet_amd import inference
    if "calib.txt" in argv:
        argv = [R.write_kitti(tmp_path / "calib.txt", R.kitti_like_calib()[0]) if a == "calib.txt" else a for a in argv]
    loaded = []
    monkeypatch.setattr(inference, "load_model", lambda *a, **k: loaded.append("inference"))
    with pytest.raises(SystemExit) as e:
        inference.main(["--synthetic_weights", "--left_img", "nowhere/left.png"] + argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--rectify" in err and ("sequential mode only: use --workers 0" in err or "--workers" not in argv)
    assert loaded == [], "a parser error must come before any model work"


def test_cli_rejects_a_kitti2015_calibration(tmp_path, capsys):
    """KITTI-2015's per-frame files hold P_rect only: fine for --calib, an error naming the key for --rectify."""
    from lwsnet_amd import inference
    path = R.write_kitti(tmp_path / "c.txt", R.kitti_like_calib()[0], skip=("K_02", "D_02", "K_03", "D_03"))
    assert Camera.from_kitti(path).fx > 0
    with pytest.raises(SystemExit):
        inference.main(["--synthetic_weights", "--left_img", "nowhere/left.png", "--rectify", path])
    assert "missing key K_02" in capsys.readouterr().err


def test_cli_defaults_are_unchanged(tmp_path):
    from lwsnet_amd import evaluate, inference
    args = vars(inference.build_parser().parse_args([]))
    assert args.pop("rectify") is None and args.pop("save_rect") is False
    assert args == {"max_disparity": 192, "img_path": "dataset/kitti2015/testing/", "left_img": "",
                    "model": "results/finetune/checkpoint.pdparams", "save_path": "results/inference", "maxdisplist": [24, 5, 5],
                    "channels_3d": 8, "layers_3d": 4, "growth_rate": [4, 1, 1], "gpu_id": 0, "synthetic_weights": False, "vis": False,
                    "split_bf16": False, "workers": 0, "gpu_workers": 3, "lr_check": None, "lr_fill": False, "speckle": None,
                    "speckle_diff": None, "speckle_fill": False, "wmedian": None, "wmedian_sigma": None, "wmedian_fill": None,
                    "calib": None, "camera": None, "min_disp": 1.0, "max_depth": float("inf"), "save_disp16": False,
                    "save_depth": False, "save_ply": False}
    assert "rectify" not in vars(evaluate.build_parser().parse_args([])), "the evaluate CLI is unchanged"
    p = inference.build_parser()
    a = p.parse_args(["--rectify", R.write_kitti(tmp_path / "c.txt", R.kitti_like_calib()[0]), "--save_rect", "--save_ply"])
    inference.check_geometry_arguments(p, a)            # the calibration brings its own camera
    inference.check_rectify_arguments(p, a)


def test_cli_rectify_error_texts(tmp_path, capsys):
    from lwsnet_amd import inference

    def error(argv):
        with pytest.raises(SystemExit) as e:
            inference.main(["--synthetic_weights"] + argv)
        assert e.value.code == 2
        return capsys.readouterr().err.rstrip("\n").split(": error: ", 1)[1]

    calib = R.write_kitti(tmp_path / "calib.txt", R.kitti_like_calib()[0])
    missing = str(tmp_path / "missing.txt")
    assert error(["--save_rect"]) == "--save_rect needs --rectify PATH"
    assert error(["--rectify", calib, "--workers", "4"]) == "--rectify runs in the sequential mode only: use --workers 0"
    assert error(["--rectify", missing, "--workers", "4"]) == "--rectify runs in the sequential mode only: use --workers 0", "the mode before the file"
    assert error(["--rectify", str(tmp_path), "--left_img", "nowhere/left_test.png"]) == (
        "--rectify: a folder of calibration files needs directory mode (--img_path); give a file with --left_img")
    assert error(["--rectify", missing]).startswith(f"--rectify: cannot read {missing}: [Errno 2] ")
    # the geometry check runs first and takes the calibration's camera on trust; the confidence check runs after the rectify check
    assert error(["--rectify", missing, "--save_ply", "--max_depth", "0"]) == "--max_depth must be > 0, got 0.0"
    assert error(["--rectify", missing, "--sigma_max", "4"]).startswith("--rectify: cannot read ")
