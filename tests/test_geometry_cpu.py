"""The geometry outputs without a GPU: the numpy restatement (tests/geometry_reference.py) on constructed values, KITTI calibration
files, the crop shift, PLY and 16-bit PNG files, the host-side argument checks of lws_depth_maps / lws_point_cloud and the
inference CLI's refusals."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

import geometry_reference as G
from cli_helpers import CAMERA, cli_refused as _refused
from lwsnet_amd import _lib
from lwsnet_amd.geometry import POINT_DTYPE, Camera, read_ply, write_ply

F = np.float32

# KITTI 2015 training/calib_cam_to_cam/000000.txt (the rectified colour cameras of the 2011_09_26 drives)
KITTI15 = """calib_time: 09-Jan-2012 13:57:47
corner_dist: 9.950000e-02
S_00: 1.392000e+03 5.120000e+02
K_00: 9.842439e+02 0.000000e+00 6.900000e+02 0.000000e+00 9.808141e+02 2.331966e+02 0.000000e+00 0.000000e+00 1.000000e+00
R_rect_00: 1.000000e+00 0.000000e+00 0.000000e+00 0.000000e+00 1.000000e+00 0.000000e+00 0.000000e+00 0.000000e+00 1.000000e+00
P_rect_00: 7.215377e+02 0.000000e+00 6.095593e+02 0.000000e+00 0.000000e+00 7.215377e+02 1.728540e+02 0.000000e+00 0.000000e+00 0.000000e+00 1.000000e+00 0.000000e+00
S_rect_02: 1.242000e+03 3.750000e+02
P_rect_02: 7.215377e+02 0.000000e+00 6.095593e+02 4.485728e+01 0.000000e+00 7.215377e+02 1.728540e+02 2.163791e-01 0.000000e+00 0.000000e+00 1.000000e+00 2.745884e-03
P_rect_03: 7.215377e+02 0.000000e+00 6.095593e+02 -3.395242e+02 0.000000e+00 7.215377e+02 1.728540e+02 2.199936e+00 0.000000e+00 0.000000e+00 1.000000e+00 2.729905e-03
"""
# KITTI object training/calib/000000.txt
OBJECT = """P0: 7.070493000000e+02 0.000000000000e+00 6.040814000000e+02 0.000000000000e+00 0.000000000000e+00 7.070493000000e+02 1.805066000000e+02 0.000000000000e+00 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 0.000000000000e+00
P1: 7.070493000000e+02 0.000000000000e+00 6.040814000000e+02 -3.797842000000e+02 0.000000000000e+00 7.070493000000e+02 1.805066000000e+02 0.000000000000e+00 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 0.000000000000e+00
P2: 7.070493000000e+02 0.000000000000e+00 6.040814000000e+02 4.575831000000e+01 0.000000000000e+00 7.070493000000e+02 1.805066000000e+02 -3.454157000000e-01 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 4.981016000000e-03
P3: 7.070493000000e+02 0.000000000000e+00 6.040814000000e+02 -3.341081000000e+02 0.000000000000e+00 7.070493000000e+02 1.805066000000e+02 2.330660000000e+00 0.000000000000e+00 0.000000000000e+00 1.000000000000e+00 3.201153000000e-03
R0_rect: 9.999128000000e-01 1.009263000000e-02 -8.511932000000e-03 -1.012729000000e-02 9.999406000000e-01 -4.037671000000e-03 8.470675000000e-03 4.123522000000e-03 9.999556000000e-01
Tr_velo_to_cam: 6.927964000000e-03 -9.999722000000e-01 -2.757829000000e-03 -2.457729000000e-02 -1.162982000000e-03 2.749836000000e-03 -9.999955000000e-01 -6.127237000000e-02 9.999753000000e-01 6.931141000000e-03 -1.143899000000e-03 -3.321029000000e-01
"""


def _img(vals):
    return np.asarray(vals, F).reshape(1, 1, 1, -1)


def _cam(fb, fx=700.0, fy=700.0, cx=600.0, cy=180.0):
    return np.array([[fx, fy, cx, cy, fb]], F)


# ---- the restatement ----
def test_depth_maps_special_values():
    d = _img([np.nan, np.inf, -np.inf, -2.0, 0.0, 1e-30, 0.5, 1.0, 2.0, 1e30])
    depth, depth16, disp16 = G.depth_maps(d, None, _cam(400.0), 1.0, np.inf)
    assert depth[0, 0, 0].tolist() == [0, 0, 0, 0, 0, 0, 0, 400.0, 200.0, F(400.0) / F(1e30)]
    assert depth16[0, 0, 0].tolist() == [0, 0, 0, 0, 0, 0, 0, 65535, 51200, 0]           # 1e30: z * 256 rounds to 0
    # disp16 ignores min_disp and the camera: every finite d > 0
    assert disp16[0, 0, 0].tolist() == [0, 0, 0, 0, 0, 0, 128, 256, 512, 65535]
    assert G.depth_maps(d, None, None, 1.0, np.inf)[2].tolist() == disp16.tolist()


def test_max_depth_cut_and_min_disp():
    d = _img([4.0, 5.0, 8.0, 10.0])
    depth, depth16, _ = G.depth_maps(d, None, _cam(400.0), 5.0, 80.0)
    assert depth[0, 0, 0].tolist() == [0.0, 80.0, 50.0, 40.0]                              # 4 < min_disp; z = 80 <= max_depth
    depth, _, _ = G.depth_maps(d, None, _cam(400.0), 1.0, np.nextafter(F(80), F(0)))
    assert depth[0, 0, 0].tolist() == [0.0, 0.0, 50.0, 40.0]                            # z = 100, 80 > max_depth


def test_mask_keeps_code_one_only():
    d = _img([2.0, 2.0, 2.0, 2.0])
    mask = np.array([1, 0, 2, 1], np.uint8).reshape(d.shape)
    depth, depth16, disp16 = G.depth_maps(d, mask, _cam(100.0), 1.0, np.inf)
    assert depth[0, 0, 0].tolist() == [50.0, 0, 0, 50.0]
    assert disp16[0, 0, 0].tolist() == [512, 0, 0, 512]
    clouds, counts = G.point_cloud(d, mask, None, _cam(100.0), 1.0, np.inf)
    assert counts.tolist() == [2] and clouds[0]["z"].tolist() == [50.0, 50.0]


def test_clamp_and_half_to_even_ties():
    # d * 256 = k + 0.5 exactly: rint goes to the even neighbour
    d = _img([0.5 / 256, 1.5 / 256, 2.5 / 256, 3.5 / 256, 100.5 / 256, 255.0, 255.99609375, 256.0, 300.0])
    disp16 = G.depth_maps(d, None, None, 1.0, np.inf)[2][0, 0, 0]
    assert disp16.tolist() == [0, 2, 2, 4, 100, 65280, 65535, 65535, 65535]
    # depth16: z = fb / d with z * 256 = k + 0.5
    z = G.depth_maps(_img([1.0, 0.5]), None, np.array([[1, 1, 0, 0, 10.5 / 256]], F), 1e-3, np.inf)[1]
    assert z[0, 0, 0].tolist() == [10, 21]


def test_point_cloud_records():
    H, W = 3, 5
    d = np.full((2, 1, H, W), 4.0, F)
    d[0, 0, 1, 2] = 0.5                                                                   # below min_disp
    d[1, 0, 0, :] = np.nan
    rgb = np.arange(2 * H * W * 3, dtype=np.uint8).reshape(2, H, W, 3)
    cam = np.array([[100, 110, 2, 1, 40], [50, 60, 1.5, 0.5, 20]], F)
    clouds, counts = G.point_cloud(d, None, rgb, cam, 1.0, np.inf)
    assert counts.tolist() == [H * W - 1, (H - 1) * W]
    c0 = clouds[0]
    assert np.all(c0["z"] == 10.0) and np.all(c0["alpha"] == 255)
    assert c0["x"][0] == F((F(0) - F(2)) * F(10)) / F(100) and c0["y"][0] == F(-10) / F(110)
    assert c0[W + 2 - 0]["x"] == F(10) / F(100)                                          # (1, 2) is skipped: (1, 3) follows (1, 1)
    assert (c0["red"][0], c0["green"][0], c0["blue"][0]) == (0, 1, 2)
    white, _ = G.point_cloud(d, None, None, cam, 1.0, np.inf)
    assert np.all(white[1]["red"] == 255) and np.all(white[1]["blue"] == 255)


# ---- cameras ----
def test_camera_from_kitti_2015(tmp_path):
    p = tmp_path / "000000.txt"
    p.write_text(KITTI15)
    cam = Camera.from_kitti(str(p))
    assert (cam.fx, cam.fy, cam.cx, cam.cy) == (721.5377, 721.5377, 609.5593, 172.854)
    assert cam.baseline == pytest.approx((44.85728 + 339.5242) / 721.5377) and 0.53 < cam.baseline < 0.54
    assert cam.fb == float(F(721.5377 * cam.baseline))
    assert cam.row().dtype == np.float32 and cam.row().tolist() == [F(721.5377), F(721.5377), F(609.5593), F(172.854), F(cam.fb)]


def test_camera_from_kitti_object(tmp_path):
    p = tmp_path / "calib.txt"
    p.write_text(OBJECT)
    cam = Camera.from_kitti(str(p))
    assert (cam.fx, cam.cx, cam.cy) == (707.0493, 604.0814, 180.5066)
    assert cam.baseline == pytest.approx((45.75831 + 334.1081) / 707.0493)


@pytest.mark.parametrize("text,msg", [
    ("calib_time: 09-Jan-2012 13:57:47\n", "P_rect_02"),
    (KITTI15.replace("P_rect_03", "P_rect_13"), "P_rect_02"),
    (OBJECT.replace("P3:", "Px:"), "P2 / P3"),
    (KITTI15.replace("4.485728e+01", "-3.395242e+02"), "baseline"),                       # P2[0,3] == P3[0,3]: baseline 0
    (KITTI15.replace("1.000000e+00 2.745884e-03", "1.0"), "12 values"),
])
def test_camera_from_kitti_errors_name_the_file(tmp_path, text, msg):
    p = tmp_path / "bad_calib.txt"
    p.write_text(text)
    with pytest.raises(ValueError, match=msg) as e:
        Camera.from_kitti(str(p))
    assert "bad_calib.txt" in str(e.value)


def test_crop_shift():
    cam = Camera(721.5, 721.5, 609.5, 172.8, 0.54)
    c = cam.crop_bottom_right(375, 1242)
    assert (c.fx, c.fy, c.baseline) == (cam.fx, cam.fy, cam.baseline)
    assert c.cx == 609.5 - 10 and c.cy == 172.8 - 7
    assert cam.crop_bottom_right(368, 1232) == cam
    c = cam.crop_bottom_right(100, 200, th=60, tw=150)
    assert (c.cx, c.cy) == (609.5 - 50, 172.8 - 40)


# ---- files ----
def test_ply_header_and_round_trip(tmp_path):
    rec = np.zeros(5, POINT_DTYPE)
    rec["x"], rec["y"], rec["z"] = np.arange(5), -np.arange(5), 2.5
    rec["red"], rec["green"], rec["blue"], rec["alpha"] = 1, 2, 3, 255
    assert POINT_DTYPE.itemsize == 16
    buf = np.concatenate([rec.view(np.uint8), np.full(32, 7, np.uint8)])                 # two unwritten records after them
    path = tmp_path / "c.ply"
    write_ply(str(path), buf, 5)
    data = path.read_bytes()
    head, body = data.split(b"end_header\n", 1)
    assert head.decode().splitlines() == ["ply", "format binary_little_endian 1.0", "element vertex 5", "property float x",
                                          "property float y", "property float z", "property uchar red", "property uchar green",
                                          "property uchar blue", "property uchar alpha"]
    assert len(body) == 5 * 16
    assert np.array_equal(np.frombuffer(body, POINT_DTYPE), rec)
    assert np.array_equal(read_ply(str(path)), rec)
    write_ply(str(path), buf, 0)
    assert read_ply(str(path)).size == 0


def test_png_gray16_read_back_by_pil_and_the_kitti_reader(tmp_path):
    from lwsnet_amd import datasets as D
    from lwsnet_amd import imageio as lio
    rng = np.random.default_rng(0)
    img = rng.integers(0, 65536, (37, 53)).astype(np.uint16)
    img[0, :4] = [0, 1, 256, 65535]
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(lio.encode_png_gray16(img)))), img)
    path = tmp_path / "000000_10.png"
    lio.save_png_gray16(str(path), img)
    im = Image.open(path)
    assert im.mode == "I;16" and im.size == (53, 37)
    ds = D.StereoPairs([str(path)], [str(path)], [str(path)], training=False, kitti_set=True)
    assert np.array_equal(ds._disparity(str(path)), img.astype(np.float32) / 256)
    with pytest.raises(ValueError):
        lio.encode_png_gray16(img.astype(np.int32))


# ---- C ABI argument checks (no GPU call is reached) ----
_P = ctypes.c_void_p(256)                                    # never dereferenced: every call below is refused first


def test_depth_maps_rejects_bad_arguments(hip_lib):
    def call(disp=_P, cam=_P, B=1, H=8, W=16, min_disp=1.0, max_depth=float("inf"), depth=_P, depth16=_P, disp16=_P):
        return hip_lib.lws_depth_maps(disp, None, cam, B, H, W, min_disp, max_depth, depth, depth16, disp16, None)

    cases = [
        (dict(disp=None), b"null"), (dict(depth=None, depth16=None, disp16=None), b"no output"),
        (dict(cam=None), b"cam"), (dict(cam=None, depth16=None), b"cam"),
        (dict(B=0), b"shape"), (dict(H=0), b"shape"), (dict(W=-1), b"shape"), (dict(B=65536), b"shape"),
        (dict(H=1 << 16, W=1 << 15), b"2^31"),
        (dict(min_disp=0.0), b"min_disp"), (dict(min_disp=-1.0), b"min_disp"), (dict(min_disp=float("inf")), b"min_disp"),
        (dict(min_disp=float("nan")), b"min_disp"),
        (dict(max_depth=0.0), b"max_depth"), (dict(max_depth=float("nan")), b"max_depth"),
        (dict(depth16=ctypes.c_void_p(257)), b"aligned"),
    ]
    for kw, msg in cases:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert msg in hip_lib.lws_last_error(), (kw, hip_lib.lws_last_error())
    texts = [
        (dict(B=0), b"depth_maps: bad shape B=0 H=8 W=16"), (dict(B=65536), b"depth_maps: bad shape B=65536 H=8 W=16"),
        (dict(H=0), b"depth_maps: bad shape B=1 H=0 W=16"), (dict(W=-1), b"depth_maps: bad shape B=1 H=8 W=-1"),
        (dict(H=1 << 16, W=1 << 15), b"depth_maps: H*W = 65536x32768 must be < 2^31"),
        (dict(min_disp=0.0), b"depth_maps: min_disp must be finite and > 0, got 0"),
        (dict(min_disp=-1.0), b"depth_maps: min_disp must be finite and > 0, got -1"),
        (dict(min_disp=float("inf")), b"depth_maps: min_disp must be finite and > 0, got inf"),
        (dict(min_disp=float("nan")), b"depth_maps: min_disp must be finite and > 0, got nan"),
        (dict(disp=ctypes.c_void_p(258)), b"depth_maps: disp is not 4-byte aligned"),
        (dict(cam=ctypes.c_void_p(258)), b"depth_maps: cam / depth must be 4-byte, depth16 / disp16 2-byte aligned"),
        (dict(disp16=ctypes.c_void_p(257)), b"depth_maps: cam / depth must be 4-byte, depth16 / disp16 2-byte aligned"),
    ]
    for kw, msg in texts:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert hip_lib.lws_last_error() == msg, kw


def test_point_cloud_rejects_bad_arguments(hip_lib):
    def call(disp=_P, cam=_P, B=1, H=8, W=16, min_disp=1.0, max_depth=100.0, work=_P, points=_P, counts=_P):
        return hip_lib.lws_point_cloud(disp, None, None, cam, B, H, W, min_disp, max_depth, work, points, counts, None)

    cases = [
        (dict(disp=None), b"null"), (dict(cam=None), b"null"), (dict(work=None), b"null"), (dict(points=None), b"null"),
        (dict(counts=None), b"null"), (dict(B=0), b"shape"), (dict(W=0), b"shape"), (dict(H=1 << 20, W=1 << 11), b"2^31"),
        (dict(min_disp=0.0), b"min_disp"), (dict(max_depth=-1.0), b"max_depth"),
        (dict(points=ctypes.c_void_p(264)), b"aligned"),
    ]
    for kw, msg in cases:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert msg in hip_lib.lws_last_error(), (kw, hip_lib.lws_last_error())
    texts = [
        (dict(B=0), b"point_cloud: bad shape B=0 H=8 W=16"), (dict(W=0), b"point_cloud: bad shape B=1 H=8 W=0"),
        (dict(H=1 << 20, W=1 << 11), b"point_cloud: H*W = 1048576x2048 must be < 2^31"),
        (dict(min_disp=float("inf")), b"point_cloud: min_disp must be finite and > 0, got inf"),
        (dict(disp=ctypes.c_void_p(258)), b"point_cloud: disp is not 4-byte aligned"),
        (dict(counts=ctypes.c_void_p(260)), b"point_cloud: cam / workspace must be 4-byte, points 16-byte, counts 8-byte aligned"),
    ]
    for kw, msg in texts:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert hip_lib.lws_last_error() == msg, kw
    assert hip_lib.lws_point_cloud_workspace(2, 368) == 3072                            # 2 x 368 int32, in 256-byte units
    assert hip_lib.lws_point_cloud_workspace(0, 368) == _lib.LWS_ERR_INVALID


# ---- the inference CLI refuses before any model or GPU work ----
@pytest.mark.parametrize("flag", ["--save_depth", "--save_ply"])
def test_cli_refuses_depth_without_camera(flag, capsys):
    assert "need a camera" in _refused([flag], capsys)


def test_cli_refuses_calib_and_camera_together(tmp_path, capsys):
    p = tmp_path / "c.txt"
    p.write_text(KITTI15)
    assert "not allowed with" in _refused(["--save_depth", "--calib", str(p), "--camera", "700", "700", "600", "180", "0.5"], capsys)


def test_cli_refuses_unreadable_calibration(tmp_path, capsys):
    assert "cannot read" in _refused(["--save_ply", "--calib", str(tmp_path / "missing.txt")], capsys)
    p = tmp_path / "bad.txt"
    p.write_text("calib_time: 09-Jan-2012 13:57:47\n")
    assert "cannot read" in _refused(["--save_ply", "--calib", str(p)], capsys)
    # a folder: every frame needs its <frame>.txt
    kdir = tmp_path / "kitti"
    (kdir / "image_2").mkdir(parents=True)
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(kdir / "image_2" / "000007_10.png")
    (tmp_path / "calib").mkdir()
    err = _refused(["--img_path", str(kdir), "--save_depth", "--calib", str(tmp_path / "calib")], capsys)
    assert "cannot read" in err and "000007.txt" in err


@pytest.mark.parametrize("flag", ["--save_disp16", "--save_depth", "--save_ply"])
def test_cli_refuses_geometry_with_workers(flag, capsys):
    assert "sequential mode only" in _refused([flag, "--camera", "700", "700", "600", "180", "0.5", "--workers", "2"], capsys)


@pytest.mark.parametrize("argv,msg", [(["--min_disp", "0"], "--min_disp"), (["--min_disp", "inf"], "--min_disp"),
                                      (["--max_depth", "-1"], "--max_depth"), (["--camera", "0", "700", "600", "180", "0.5"], "--camera"),
                                      (["--camera", "700", "700", "600", "180", "-0.5"], "--camera")])
def test_cli_refuses_bad_geometry_values(argv, msg, capsys):
    assert msg in _refused(["--save_ply"] + argv, capsys)


def test_geometry_flags_default_off():
    from lwsnet_amd import inference
    a = inference.build_parser().parse_args([])
    assert (a.calib, a.camera, a.save_disp16, a.save_depth, a.save_ply) == (None, None, False, False, False)
    assert a.min_disp == 1.0 and a.max_depth == float("inf")


NEEDS_CAMERA = " need a camera: --calib PATH or --camera FX FY CX CY BASELINE"
SEQUENTIAL = " in the sequential mode only: use --workers 0"
OUTPUTS_SEQUENTIAL = "--save_disp16 / --save_depth / --save_ply / --save_normals / --save_mesh run" + SEQUENTIAL
OUTPUTS_CAMERA = "--save_depth, --save_ply, --save_normals and --save_mesh" + NEEDS_CAMERA
GROUND_HEIGHTS = "--ground_tol and --max_height must be finite with 0 <= ground_tol <= max_height, got -1.0 and 3.0"


def _error(argv, capsys):
    """The message of the parser error `argv` ends in: argparse's last line without its "prog: error: "."""
    err = _refused(argv, capsys)
    assert err.endswith("\n") and ": error: " in err
    return err[:-1].split(": error: ", 1)[1]


@pytest.mark.parametrize("argv,text", [
    (["--save_ply", "--min_disp", "0"], "--min_disp must be finite and > 0, got 0.0"),
    (["--save_ply", "--min_disp", "inf"], "--min_disp must be finite and > 0, got inf"),
    (["--save_ply", "--max_depth", "-1"], "--max_depth must be > 0, got -1.0"),
    (["--max_depth", "nan"], "--max_depth must be > 0, got nan"),
    (["--save_depth"], OUTPUTS_CAMERA),
    (["--save_ply"], OUTPUTS_CAMERA),
    (["--save_normals"], OUTPUTS_CAMERA),
    (["--save_disp16", "--workers", "2"], OUTPUTS_SEQUENTIAL),
    (["--save_mesh", "--workers", "1"] + CAMERA, OUTPUTS_SEQUENTIAL),
    (["--camera", "0", "700", "600", "180", "0.5"], "--camera: camera needs finite values with fx, fy, baseline > 0; got Camera(fx=0.0, fy=700.0, cx=600.0, cy=180.0, baseline=0.5)"),
    (["--left_img", "nowhere/left_test.png", "--calib", "."], "--calib: a folder of calibration files needs directory mode (--img_path); give a file with --left_img"),
])
def test_cli_geometry_error_texts(argv, text, capsys):
    assert _error(argv, capsys) == text


def test_cli_calib_error_text_names_the_file(tmp_path, capsys):
    missing = str(tmp_path / "missing.txt")
    assert _error(["--calib", missing], capsys).startswith(f"--calib: cannot read {missing}: [Errno 2] ")


@pytest.mark.parametrize("argv,text", [
    (["--ground_tol", "-1", "--max_jump", "-1"], GROUND_HEIGHTS),
    (["--max_jump", "-1", "--min_disp", "0"], "--max_jump must be finite and >= 0, got -1.0"),
    (["--min_disp", "0", "--max_depth", "-1"], "--min_disp must be finite and > 0, got 0.0"),
    (["--max_depth", "-1", "--save_ply"], "--max_depth must be > 0, got -1.0"),
    (["--save_ply", "--stixel_width", "0"], OUTPUTS_CAMERA),
    (["--stixel_width", "0", "--stixel_layers", "0"], "--stixel_width must be in 1 .. 64, got 0"),
    (["--stixel_layers", "0", "--stixels"], "--stixel_layers must be in 1 .. 4, got 0"),
    (["--stixels", "--workers", "2"], "--stixels and --save_stixels" + NEEDS_CAMERA),
    (["--stixels", "--workers", "2"] + CAMERA, "--stixels / --save_stixels run" + SEQUENTIAL),
    (["--ground", "--workers", "2"], "--ground and --save_ground" + NEEDS_CAMERA),
    (["--ground", "--save_disp16", "--workers", "2"] + CAMERA, "--ground / --save_ground run" + SEQUENTIAL),
    (["--save_disp16", "--workers", "2", "--camera", "0", "700", "600", "180", "0.5"], OUTPUTS_SEQUENTIAL),
    (["--save_disp16", "--lr_check", "1", "--workers", "2"], "--lr_check runs" + SEQUENTIAL),
    (["--save_disp16", "--workers", "2", "--rectify", "nowhere.txt"], OUTPUTS_SEQUENTIAL),
    (["--save_rect", "--save_conf", "--lr_check", "1"], "--save_rect needs --rectify PATH"),
    (["--save_conf", "--lr_check", "1", "--photo_alpha", "0.5"],
     "--save_conf / --conf_min / --sigma_max_keep use the network's own confidence and do not combine with --lr_check or --occ_check"),
])
def test_cli_earlier_check_wins(argv, text, capsys):
    """Two errors apply to each line: the one whose check comes first is reported (the checks of check_geometry_arguments in their
    order, then the order of main()'s check_* calls)."""
    assert _error(argv, capsys) == text


DEFAULT_NAMESPACE = {"max_disparity": 192, "img_path": "dataset/kitti2015/testing/", "left_img": "",
                     "model": "results/finetune/checkpoint.pdparams", "save_path": "results/inference", "maxdisplist": [24, 5, 5],
                     "channels_3d": 8, "layers_3d": 4, "growth_rate": [4, 1, 1], "gpu_id": 0, "synthetic_weights": False, "vis": False,
                     "split_bf16": False, "workers": 0, "gpu_workers": 3, "lr_check": None, "lr_fill": False, "speckle": None,
                     "speckle_diff": None, "speckle_fill": False, "wmedian": None, "wmedian_sigma": None, "wmedian_fill": None,
                     "calib": None, "camera": None, "min_disp": 1.0, "max_depth": float("inf"), "save_disp16": False,
                     "save_depth": False, "save_ply": False, "rectify": None, "save_rect": False}


@pytest.mark.parametrize("argv,changed", [
    ([], {}),
    (["--lr_check", "1", "--lr_fill"], dict(lr_check=1.0, lr_fill=True)),
    (["--occ_check", "0.5", "--occ_fill"], dict(occ_check=0.5, occ_fill=True)),
    (["--speckle", "60", "--speckle_diff", "0.5", "--speckle_fill"], dict(speckle=60, speckle_diff=0.5, speckle_fill=True)),
    (["--wmedian", "2", "--wmedian_sigma", "4", "--wmedian_fill", "3"], dict(wmedian=2, wmedian_sigma=4.0, wmedian_fill=3)),
    (["--save_disp16", "--save_depth", "--save_ply", "--min_disp", "0.5", "--max_depth", "80"] + CAMERA,
     dict(save_disp16=True, save_depth=True, save_ply=True, min_disp=0.5, max_depth=80.0, camera=[700.0, 700.0, 600.0, 180.0, 0.5])),
    (["--save_normals", "--save_mesh", "--max_jump", "2", "--calib", "c.txt"], dict(save_normals=True, save_mesh=True, max_jump=2.0, calib="c.txt")),
    (["--ground", "--save_ground", "--ground_tol", "0.3", "--max_height", "2"], dict(ground=True, save_ground=True, ground_tol=0.3, max_height=2.0)),
    (["--stixels", "--save_stixels", "--stixel_width", "4", "--stixel_layers", "3"], dict(stixels=True, save_stixels=True, stixel_width=4, stixel_layers=3)),
    (["--rectify", "r.txt", "--save_rect", "--workers", "2", "--gpu_workers", "1"], dict(rectify="r.txt", save_rect=True, workers=2, gpu_workers=1)),
    (["--save_conf", "--sigma_max", "4", "--conf_min", "0.3", "--sigma_max_keep", "2"], dict(save_conf=True, sigma_max=4.0, conf_min=0.3, sigma_max_keep=2.0)),
    (["--photometric", "--photo_alpha", "0.5", "--save_photo"], dict(photometric=True, photo_alpha=0.5, save_photo=True)),
])
def test_command_lines_parse_to_the_same_namespaces(argv, changed):
    """What build_parser() alone makes of a command line, before any check_* writes a default: the flags given and no others."""
    from lwsnet_amd import inference
    assert vars(inference.build_parser().parse_args(argv)) == {**DEFAULT_NAMESPACE, **changed}
