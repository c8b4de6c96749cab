"""Surface normals and the triangle mesh without a GPU: the numpy restatement (tests/mesh_reference.py) against things it was not
written from -- a float64 plane normal, the topology of a full grid, a depth step, the four one-corner-missing cells -- the
host-side argument checks of lws_surface_normals / lws_surface_mesh, mesh PLY files and the inference CLI's refusals."""
import ctypes
from collections import Counter

import numpy as np
import pytest

import geometry_reference as G
import mesh_reference as M
from cli_helpers import CAMERA, cli_refused as _refused
from lwsnet_amd import _lib
from lwsnet_amd.geometry import POINT_DTYPE, VERTEX_NORMAL_DTYPE, Camera, camera_rows, mesh_ply_bytes, read_mesh_ply, write_mesh_ply

F = np.float32
INF = float("inf")
KITTI = Camera(721.5377, 721.5377, 609.5593, 172.854, 0.5327)


def _cam():
    return camera_rows(KITTI, 1)


def _plane(H, W, d0, ax, ay):
    ys, xs = np.mgrid[0:H, 0:W]
    return (d0 + ax * xs + ay * ys).astype(F)[None, None]


def _positions(rec):
    return np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float64)


# ---- the restatement against things it was not written from ----
def test_slanted_plane_matches_the_float64_normal():
    """A plane in disparity space is a plane in space.  Gate 1e-4 per component: the restatement's own float32 distance measured
    with this camera is 4.6e-5 (the X of a pixel 600 columns from the principal point carries a rounding error of 1e-6 m against
    edge vectors of 2e-2 m), a wrong quadrant order or sign moves a component by at least 1e-2."""
    H, W = 9, 13
    d = _plane(H, W, 30.0, 0.8, -0.5)
    cam = _cam()
    n, nq = M.surface_normals(d, None, cam, 1.0, INF, 1.0)
    fx, fy, cx, cy, fb = (float(v) for v in cam[0])

    def P(x, y):
        z = fb / float(d[0, 0, y, x])
        return np.array([(x - cx) * z / fx, (y - cy) * z / fy, z])

    want = np.cross(P(0, H - 1) - P(0, 0), P(W - 1, 0) - P(0, 0))
    want /= np.linalg.norm(want)
    assert want[2] < 0
    err = np.abs(n[0].astype(np.float64) - want[:, None, None]).max()
    print(f"slanted plane: max distance to the float64 normal {err:.3g}")
    assert err <= 1e-4
    # corners see one quadrant, the other border pixels two, the interior four
    assert nq[0, 0, 0] == nq[0, 0, -1] == nq[0, -1, 0] == nq[0, -1, -1] == 1
    assert np.all(nq[0, 1:-1, 1:-1] == 4) and np.all(nq[0, 0, 1:-1] == 2) and np.all(nq[0, 1:-1, 0] == 2)
    assert sorted(np.unique(nq)) == [1, 2, 4]


def test_fronto_parallel_plane_is_exactly_minus_z():
    d = np.full((1, 1, 5, 6), 40.0, F)
    n, _ = M.surface_normals(d, None, _cam(), 1.0, INF, 1.0)
    assert np.all(n[0, :2] == 0.0) and np.all(n[0, 2] == -1.0)
    n8 = M.normals8(n)
    assert n8.shape == (1, 5, 6, 3) and np.all(n8 == np.array([128, 128, 255], np.uint8))     # -0 * 0.5 + 0.5 -> 127.5 -> 128


def test_invalid_and_isolated_pixels_have_the_zero_normal():
    d = np.full((1, 1, 3, 3), 40.0, F)
    d[0, 0, 1, 1] = np.nan
    d[0, 0, 0, 2] = 90.0                                                # valid, but connected to no neighbour
    n, nq = M.surface_normals(d, None, _cam(), 1.0, INF, 1.0)
    for y, x in ((1, 1), (0, 2)):
        assert nq[0, y, x] == 0 and n[0, :, y, x].view(np.uint32).tolist() == [0, 0, 0]
        assert M.normals8(n)[0, y, x].tolist() == [128, 128, 128]


def test_all_valid_grid_is_a_closed_sheet():
    H, W = 6, 7
    d = _plane(H, W, 30.0, 0.3, -0.2)
    cam = _cam()
    n, _ = M.surface_normals(d, None, cam, 1.0, INF, 1.0)
    clouds, vn, faces, index, counts = M.surface_mesh(d, None, None, cam, n, 1.0, INF, 1.0)
    f = faces[0]
    assert counts.tolist() == [[H * W, 2 * (H - 1) * (W - 1)]] and f.shape == (2 * (H - 1) * (W - 1), 3)
    assert np.array_equal(index[0, 0], np.arange(H * W, dtype=np.int32).reshape(H, W))
    edges = Counter()
    for tri in f.tolist():
        for i in range(3):
            edges[tuple(sorted((tri[i], tri[(i + 1) % 3])))] += 1
    want = {}
    for y in range(H):
        for x in range(W):
            v = y * W + x
            if x + 1 < W:
                want[(v, v + 1)] = 1 if y in (0, H - 1) else 2          # a horizontal grid edge
            if y + 1 < H:
                want[(v, v + W)] = 1 if x in (0, W - 1) else 2          # a vertical one
            if x + 1 < W and y + 1 < H:
                want[(v + 1, v + W)] = 2                                # the b-c diagonal of the cell
    assert dict(edges) == want
    p = _positions(clouds[0])
    g = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    assert np.all(g[:, 2] < 0)
    for k in range(3):
        assert np.all((g * vn[0][f[:, k], :3]).sum(axis=1) > 0)
    assert np.all(vn[0][:, 3] == 0)


def test_no_face_spans_a_step_wider_than_max_jump():
    H, W, k = 7, 12, 6
    left, right = _plane(H, W, 40.0, 0.3, -0.2), _plane(H, W, 20.0, -0.25, 0.15)
    d = left.copy()
    d[..., k:] = right[..., k:]
    cam = _cam()
    n, _ = M.surface_normals(d, None, cam, 1.0, INF, 1.0)
    _, _, faces, index, counts = M.surface_mesh(d, None, None, cam, n, 1.0, INF, 1.0)
    side = (index[0, 0] % W >= k).reshape(-1)                          # all valid: vertex = raster index
    f = faces[0]
    assert len(f) == 2 * (H - 1) * (W - 2) == counts[0, 1]
    assert np.all(side[f].min(axis=1) == side[f].max(axis=1))
    # the normals on each side are those of the side alone (the other half masked out), bit for bit
    for lo, hi in ((0, k), (k, W)):
        mask = np.zeros(d.shape, np.uint8)
        mask[..., lo:hi] = 1
        alone, _ = M.surface_normals(d, mask, cam, 1.0, INF, 1.0)
        assert np.array_equal(n[..., lo:hi].view(np.uint32), alone[..., lo:hi].view(np.uint32))
    with_jump, _ = M.surface_normals(d, None, cam, 1.0, INF, 30.0)
    assert not np.array_equal(with_jump[..., k - 1:k + 1], n[..., k - 1:k + 1])


@pytest.mark.parametrize("corner,want", [((0, 0), (0, 1, 2)),           # a missing: the b-c diagonal, T1 = (b, c, e)
                                         ((0, 1), (0, 1, 2)),           # b missing: the a-e diagonal, T0 = (a, c, e)
                                         ((1, 0), (0, 2, 1)),           # c missing: the a-e diagonal, T1 = (a, e, b)
                                         ((1, 1), (0, 2, 1))])          # e missing: the b-c diagonal, T0 = (a, c, b)
def test_cell_with_one_invalid_corner(corner, want):
    d = np.full((1, 1, 2, 2), 40.0, F)
    mask = np.ones(d.shape, np.uint8)
    mask[0, 0][corner] = 2
    clouds, _, faces, index, counts = M.surface_mesh(d, mask, None, _cam(), None, 1.0, INF, 1.0)
    assert counts.tolist() == [[3, 1]] and faces[0].tolist() == [list(want)]
    ix = index[0, 0].reshape(-1).tolist()
    assert ix[2 * corner[0] + corner[1]] == -1 and [v for v in ix if v >= 0] == [0, 1, 2]
    p = _positions(clouds[0])
    a, b, c = (p[i] for i in want)
    assert np.cross(b - a, c - a)[2] < 0


def test_both_diagonals_blocked_emit_nothing():
    d = np.array([[40.0, 60.0], [60.0, 40.0]], F)[None, None]           # b-c is the diagonal (both valid) and a is connected to neither
    _, _, faces, _, counts = M.surface_mesh(d, None, None, _cam(), None, 1.0, INF, 1.0)
    assert counts.tolist() == [[4, 0]] and faces[0].shape == (0, 3)


# ---- C ABI argument checks (no GPU call is reached) ----
def _p(k, off=0):
    """Fake device pointers 1 GiB apart: never dereferenced, every call below is refused first."""
    return ctypes.c_void_p((1 << 40) + (k << 30) + off)


def test_surface_normals_rejects_bad_arguments(hip_lib):
    def call(disp=_p(0), mask=_p(1), cam=_p(2), B=1, H=8, W=16, min_disp=1.0, max_depth=INF, max_jump=1.0, normals=_p(3), normals8=_p(4)):
        return hip_lib.lws_surface_normals(disp, mask, cam, B, H, W, min_disp, max_depth, max_jump, normals, normals8, None)

    texts = [
        (dict(disp=None), b"surface_normals: disp is null"), (dict(cam=None), b"surface_normals: cam is null"),
        (dict(normals=None, normals8=None), b"surface_normals: no output requested (normals and normals8 are both null)"),
        (dict(disp=_p(0, 2)), b"surface_normals: disp is not 4-byte aligned"), (dict(cam=_p(2, 1)), b"surface_normals: cam is not 4-byte aligned"),
        (dict(normals=_p(3, 2)), b"surface_normals: normals is not 4-byte aligned"),
        (dict(max_jump=-1.0), b"surface_normals: max_jump must be finite and >= 0, got -1"),
        (dict(max_jump=float("nan")), b"surface_normals: max_jump must be finite and >= 0, got nan"),
        (dict(max_jump=INF), b"surface_normals: max_jump must be finite and >= 0, got inf"),
        (dict(min_disp=0.0), b"surface_normals: min_disp must be finite and > 0, got 0"),
        (dict(max_depth=float("nan")), b"surface_normals: max_depth must be > 0 (+inf allowed), got nan"),
        (dict(B=0), b"surface_normals: bad shape B=0 H=8 W=16"), (dict(B=65536), b"surface_normals: bad shape B=65536 H=8 W=16"),
        (dict(H=1 << 15, W=1 << 15), b"surface_normals: H*W = 32768x32768 must be < 2^30"),
        (dict(normals8=_p(3, 12 * 128 - 1)), b"surface_normals: normals8 and normals overlap"),
        (dict(disp=_p(3, 12 * 128 - 4)), b"surface_normals: disp and normals overlap"),
        (dict(mask=_p(4, 3 * 128 - 1)), b"surface_normals: mask and normals8 overlap"),
        (dict(cam=_p(4)), b"surface_normals: cam and normals8 overlap"),
    ]
    for kw, msg in texts:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert hip_lib.lws_last_error() == msg, (kw, hip_lib.lws_last_error())


def test_surface_mesh_rejects_bad_arguments(hip_lib):
    names = ("disp", "mask", "rgb", "cam", "normals", "work", "points", "vnormals", "faces", "index", "counts")
    base = {name: _p(k) for k, name in enumerate(names)}

    def call(B=1, H=8, W=16, min_disp=1.0, max_depth=100.0, max_jump=1.0, **ptrs):
        a = {**base, **ptrs}
        return hip_lib.lws_surface_mesh(a["disp"], a["mask"], a["rgb"], a["cam"], a["normals"], B, H, W, min_disp, max_depth, max_jump,
                                        a["work"], a["points"], a["vnormals"], a["faces"], a["index"], a["counts"], None)

    def at(name, off):
        return _p(names.index(name), off)

    null = b"surface_mesh: workspace, points, faces and counts must not be null"
    a4 = b"surface_mesh: workspace / normals / faces / index must be 4-byte aligned"
    a16 = b"surface_mesh: points / vnormals must be 16-byte, counts 8-byte aligned"
    texts = [
        (dict(disp=None), b"surface_mesh: disp is null"), (dict(cam=None), b"surface_mesh: cam is null"),
        (dict(work=None), null), (dict(points=None), null), (dict(faces=None), null), (dict(counts=None), null),
        (dict(normals=None), b"surface_mesh: normals and vnormals go together (normals is null)"),
        (dict(vnormals=None), b"surface_mesh: normals and vnormals go together (vnormals is null)"),
        (dict(disp=at("disp", 2)), b"surface_mesh: disp is not 4-byte aligned"), (dict(cam=at("cam", 2)), b"surface_mesh: cam is not 4-byte aligned"),
        (dict(work=at("work", 2)), a4), (dict(normals=at("normals", 2)), a4), (dict(faces=at("faces", 1)), a4), (dict(index=at("index", 2)), a4),
        (dict(points=at("points", 8)), a16), (dict(vnormals=at("vnormals", 4)), a16), (dict(counts=at("counts", 4)), a16),
        (dict(max_jump=-0.5), b"surface_mesh: max_jump must be finite and >= 0, got -0.5"),
        (dict(max_jump=float("nan")), b"surface_mesh: max_jump must be finite and >= 0, got nan"),
        (dict(max_jump=INF), b"surface_mesh: max_jump must be finite and >= 0, got inf"),
        (dict(min_disp=INF), b"surface_mesh: min_disp must be finite and > 0, got inf"),
        (dict(B=0), b"surface_mesh: bad shape B=0 H=8 W=16"), (dict(W=0), b"surface_mesh: bad shape B=1 H=8 W=0"),
        (dict(H=1 << 10, W=1 << 20), b"surface_mesh: H*W = 1024x1048576 must be < 2^30"),
        (dict(points=at("work", 256)), b"surface_mesh: points and workspace overlap"),              # the face counts' half of it
        (dict(vnormals=at("points", 16 * 127)), b"surface_mesh: vnormals and points overlap"),
        (dict(faces=at("vnormals", 16)), b"surface_mesh: faces and vnormals overlap"),
        (dict(index=at("faces", 12 * 2 * 7 * 15 - 4)), b"surface_mesh: index and faces overlap"),
        (dict(counts=at("index", 8)), b"surface_mesh: counts and index overlap"),
        (dict(disp=at("counts", 8)), b"surface_mesh: disp and counts overlap"),
        (dict(mask=at("points", 0)), b"surface_mesh: mask and points overlap"),
        (dict(rgb=at("faces", 0)), b"surface_mesh: rgb and faces overlap"),
        (dict(cam=at("work", 0)), b"surface_mesh: cam and workspace overlap"),
        (dict(normals=at("vnormals", 16 * 64)), b"surface_mesh: normals and vnormals overlap"),
    ]
    for kw, msg in texts:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert hip_lib.lws_last_error() == msg, (kw, hip_lib.lws_last_error())
    # the optional pointers may be null together
    assert call(H=1 << 10, W=1 << 20, mask=None, rgb=None, normals=None, vnormals=None, index=None) == _lib.LWS_ERR_INVALID
    assert b"2^30" in hip_lib.lws_last_error()


def test_surface_mesh_workspace_size(hip_lib):
    assert hip_lib.lws_surface_mesh_workspace(2, 368) == 2 * 3072                       # 2 x 368 int32 in 256-byte units, twice
    assert hip_lib.lws_surface_mesh_workspace(1, 1) == 512
    assert hip_lib.lws_surface_mesh_workspace(1, 65) == 2 * 512
    assert hip_lib.lws_surface_mesh_workspace(0, 368) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_last_error() == b"surface_mesh_workspace: bad shape B=0 H=368"
    assert hip_lib.lws_surface_mesh_workspace(65536, 1) == _lib.LWS_ERR_INVALID


def test_ops_validate_before_any_gpu_call():
    from lwsnet_amd import ops
    for fn in (ops.surface_normals, ops.surface_mesh):
        with pytest.raises(ValueError, match="needs cameras"):
            fn(None, None)
        with pytest.raises(RuntimeError, match="HIP device"):
            fn(np.zeros((1, 1, 2, 2), F), KITTI)
    with pytest.raises(ValueError, match="at least one"):
        ops.surface_normals(None, KITTI, normals=False, normals8=False)
    assert ops.SurfaceMesh._fields == ("points", "vnormals", "faces", "index", "counts")


# ---- files ----
def _mesh_records():
    rec = np.zeros(4, POINT_DTYPE)
    rec["x"], rec["y"], rec["z"] = np.arange(4), -np.arange(4), 2.5
    rec["red"], rec["green"], rec["blue"], rec["alpha"] = 1, 2, 3, 255
    faces = np.array([[0, 2, 1], [1, 2, 3]], np.int32)
    vn = np.zeros((4, 4), F)
    vn[:, :3] = [[0, 0, -1], [0.6, 0, -0.8], [0, 0.6, -0.8], [0, 0, 0]]
    return rec, faces, vn


def test_mesh_ply_header_and_round_trip_with_normals(tmp_path):
    rec, faces, vn = _mesh_records()
    buf = np.concatenate([rec.view(np.uint8), np.full(32, 7, np.uint8)])                 # two unwritten records after them
    path = tmp_path / "m.ply"
    write_mesh_ply(str(path), buf, 4, faces, vn)
    head, body = path.read_bytes().split(b"end_header\n", 1)
    assert head.decode().splitlines() == [
        "ply", "format binary_little_endian 1.0", "element vertex 4", "property float x", "property float y", "property float z",
        "property float nx", "property float ny", "property float nz", "property uchar red", "property uchar green",
        "property uchar blue", "property uchar alpha", "element face 2", "property list uchar int vertex_indices"]
    assert VERTEX_NORMAL_DTYPE.itemsize == 28 and len(body) == 4 * 28 + 2 * 13
    assert body[4 * 28:] == b"\x03" + faces[0].tobytes() + b"\x03" + faces[1].tobytes()
    verts, got = read_mesh_ply(str(path))
    assert verts.dtype == VERTEX_NORMAL_DTYPE and got.dtype == np.int32 and np.array_equal(got, faces)
    for name in POINT_DTYPE.names:
        assert np.array_equal(verts[name], rec[name]), name
    assert np.array_equal(np.stack([verts["nx"], verts["ny"], verts["nz"]], axis=1), vn[:, :3])


def test_mesh_ply_header_and_round_trip_without_normals(tmp_path):
    rec, faces, _ = _mesh_records()
    path = tmp_path / "m.ply"
    write_mesh_ply(str(path), rec.view(np.uint8), 4, faces)
    head, body = path.read_bytes().split(b"end_header\n", 1)
    assert head.decode().splitlines() == [
        "ply", "format binary_little_endian 1.0", "element vertex 4", "property float x", "property float y", "property float z",
        "property uchar red", "property uchar green", "property uchar blue", "property uchar alpha", "element face 2",
        "property list uchar int vertex_indices"]
    assert len(body) == 4 * 16 + 2 * 13
    verts, got = read_mesh_ply(str(path))
    assert verts.dtype == POINT_DTYPE and np.array_equal(verts, rec) and np.array_equal(got, faces)
    # no vertices, no faces
    write_mesh_ply(str(path), b"", 0, np.zeros((0, 3), np.int32))
    verts, got = read_mesh_ply(str(path))
    assert verts.size == 0 and got.shape == (0, 3)


def test_mesh_ply_rejects_what_it_cannot_write():
    rec, faces, vn = _mesh_records()
    with pytest.raises(ValueError, match="fewer than"):
        mesh_ply_bytes(rec.view(np.uint8), 5, faces)
    with pytest.raises(ValueError, match="outside"):
        mesh_ply_bytes(rec.view(np.uint8), 3, faces)
    with pytest.raises(ValueError, match="int32"):
        mesh_ply_bytes(rec.view(np.uint8), 4, faces.astype(np.int64))
    with pytest.raises(ValueError, match="vnormals"):
        mesh_ply_bytes(rec.view(np.uint8), 4, faces, vn[:3])


# ---- the inference CLI refuses before any model or GPU work ----
@pytest.mark.parametrize("flag", ["--save_normals", "--save_mesh"])
def test_cli_refuses_surface_outputs_without_camera(flag, capsys):
    assert "--save_normals and --save_mesh need a camera" in _refused([flag], capsys)


@pytest.mark.parametrize("flag", ["--save_normals", "--save_mesh"])
def test_cli_refuses_surface_outputs_with_workers(flag, capsys):
    assert "sequential mode only" in _refused([flag, "--workers", "2"] + CAMERA, capsys)


@pytest.mark.parametrize("value", ["-1", "nan", "inf"])
def test_cli_refuses_bad_max_jump(value, capsys):
    assert "--max_jump must be finite and >= 0" in _refused(["--save_mesh", "--max_jump", value] + CAMERA, capsys)


def test_cli_conf_masks_count_the_surface_outputs(capsys):
    assert "give one of them" in _refused(["--conf_min", "0.5"], capsys)
    assert "--save_mesh" in _refused(["--sigma_max_keep", "2"], capsys)
    # with a surface output the confidence masks are accepted: the refusal that follows is the missing camera's
    assert "need a camera" in _refused(["--conf_min", "0.5", "--save_normals"], capsys)


def test_surface_flags_default_off():
    from lwsnet_amd import inference
    p = inference.build_parser()
    a = p.parse_args([])
    assert not any(hasattr(a, name) for name in ("save_normals", "save_mesh", "max_jump"))      # the namespace of a line without them
    inference.check_geometry_arguments(p, a)
    assert (a.save_normals, a.save_mesh, a.max_jump) == (False, False, 1.0)
    a = p.parse_args(["--save_normals", "--save_mesh", "--max_jump", "2.5"] + CAMERA)
    inference.check_geometry_arguments(p, a)
    assert (a.save_normals, a.save_mesh, a.max_jump) == (True, True, 2.5)


@pytest.mark.parametrize("value,shown", [("-1", "-1.0"), ("nan", "nan"), ("inf", "inf")])
def test_cli_max_jump_error_text(value, shown, capsys):
    assert _refused(["--max_jump", value], capsys).endswith(f": error: --max_jump must be finite and >= 0, got {shown}\n")


def test_cli_surface_error_texts(capsys):
    camera = ": error: --save_depth, --save_ply, --save_normals and --save_mesh need a camera: --calib PATH or --camera FX FY CX CY BASELINE\n"
    assert _refused(["--save_mesh"], capsys).endswith(camera)
    assert _refused(["--save_normals", "--workers", "2"], capsys).endswith(camera), "the camera comes before the mode"
    assert _refused(["--save_normals", "--workers", "2"] + CAMERA, capsys).endswith(
        ": error: --save_disp16 / --save_depth / --save_ply / --save_normals / --save_mesh run in the sequential mode only: use --workers 0\n")
