"""lws_tsdf_mesh without a GPU: the case table the library exports against the one tests/tsdf_mesh_reference.py builds from the rule,
the properties that make the table crack-free, the numpy mesh on analytic volumes, the argument checks of the C entry points and of
lwsnet_amd.ops.tsdf_mesh, the reading of include/lwsnet_tsdf_mesh.h, and the inference CLI's flag."""
import ctypes
import os

import numpy as np
import pytest

import tsdf_mesh_reference as MR
import tsdf_reference as R
from cli_helpers import CAMERA, cli_refused as _cli_refused, poses_file as _poses_file, sequence_dir as _sequence_dir
from conftest import ROOT
from lwsnet_amd import _lib

F = np.float32
VP, I, FL, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int64
HEADER = "lwsnet_tsdf_mesh.h"


# ---- the table ----
def test_the_exported_table_is_the_one_the_rule_gives(hip_lib):
    got = np.zeros((256, 32), np.uint8)
    assert hip_lib.lws_tsdf_mesh_table(got.ctypes.data_as(ctypes.c_void_p)) == _lib.LWS_OK
    want = MR.table()
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))
    assert int(got[:, 0].max()) == _lib.LWS_TSDF_MESH_MAX_TRIS <= 10
    assert hip_lib.lws_tsdf_mesh_table(None) == _lib.LWS_ERR_INVALID and hip_lib.lws_last_error() == b"tsdf_mesh_table: table is null"


@pytest.mark.parametrize("which", ["library", "reference"])
def test_table_properties_of_all_256_cases(hip_lib, which):
    """Per case, from the table's bytes and the rule's face segments alone (no loop is traced here): the edges used are the case's
    crossing edges; every face segment is a directed triangle edge exactly once and its reverse never; every other directed
    triangle edge -- a fan edge inside the cube -- has its reverse exactly once.  Two valid cubes that share a face hold the same
    segments there (the segments depend on the face's signs only) in opposite directions (the outside of one is the inside of the
    other), so their triangles close."""
    table = np.zeros((256, 32), np.uint8)
    if which == "library":
        hip_lib.lws_tsdf_mesh_table(table.ctypes.data_as(ctypes.c_void_p))
    else:
        table = MR.table()
    for case in range(256):
        n = int(table[case, 0])
        assert n <= _lib.LWS_TSDF_MESH_MAX_TRIS and (table[case, 1 + 3 * n:] == 255).all() and (table[case, 1:1 + 3 * n] < 12).all(), case
        tris = table[case, 1:1 + 3 * n].reshape(n, 3).tolist()
        crossing = {e for e in range(12) if ((case >> MR.edge_corners(e)[0]) & 1) != ((case >> MR.edge_corners(e)[1]) & 1)}
        assert {e for t in tris for e in t} == crossing, case
        assert all(len(set(t)) == 3 for t in tris), case
        directed = MR.directed_edges(tris)
        segments = MR.face_segments(case)
        assert len(segments) == len(set(segments)) == len(crossing), case       # every crossing edge starts one segment
        for a, b in segments:
            assert directed.get((a, b), 0) == 1 and (b, a) not in directed, (case, a, b)
        for (a, b), count in directed.items():
            if (a, b) not in segments:
                assert count == 1 and directed.get((b, a), 0) == 1 and (b, a) not in segments, (case, a, b)
    assert table[0, 0] == 0 and table[255, 0] == 0
    assert table[254, :4].tolist() == [1, 0, 4, 8]                  # the anchor: only corner 0 non-positive


def test_the_segments_of_a_shared_face_agree():
    """The face x = 1 of a cube is the face x = 0 of its +x neighbour: for every pair of cases that agree on those four corners, the
    segments of the one on that face are the segments of the other, reversed, once the edge ids are carried across."""
    def on_face(case, side):
        edges = {e for e in range(12) if e >> 2 != 0 and all(MR.corner_of(c)[0] == side for c in MR.edge_corners(e))}
        return {(a, b) for a, b in MR.face_segments(case) if a in edges and b in edges}
    across = {e: e - 1 for e in (5, 7, 9, 11)}                      # the y and z edges at dx = 1 are those at dx = 0 of the neighbour

    def spread(four, dx):                                           # four signs -> the corners dx, dx + 2, dx + 4, dx + 6
        return sum(((four >> i) & 1) << (2 * i + dx) for i in range(4))
    for shared in range(16):
        for far_a in (0, 5, 9, 15):
            for far_b in (0, 6, 10, 15):
                a = on_face(spread(shared, 1) | spread(far_a, 0), 1)
                b = on_face(spread(shared, 0) | spread(far_b, 1), 0)
                assert {(across[q], across[p]) for p, q in a} == b, (shared, far_a, far_b)
                assert len(a) == {0: 0, 15: 0, 6: 2, 9: 2}.get(shared, 1)


# ---- the numpy mesh on analytic volumes ----
def closed_and_oriented(faces):
    d = MR.directed_edges(faces)
    return all(count == 1 and d.get((b, a), 0) == 1 for (a, b), count in d.items())


def test_a_sphere_is_closed_oriented_and_has_its_volume():
    """The sanity check against the analytic volume: marching cubes cuts the corners of a convex body, so the mesh of a sphere of
    R = 5 voxels (1.25 m) holds 7.985636 m^3 of the 8.181231 m^3 of the ball: 2.39 % short, measured with this reference on the
    CPU.  The margin is twice that; the device is held to this reference's bits (tests/test_gpu_tsdf_mesh.py), not to the margin."""
    T, Wt = MR.sphere_volume()
    assert not (T == 0).any()
    rec, nrm, faces = MR.mesh(T, Wt, None, (0.0, 0.0, 0.0), MR.VS)
    assert len(faces) > 0 and closed_and_oriented(faces) and MR.euler(faces) == 2
    assert len(np.unique(faces)) == len(rec)                        # fully observed: every crossing is some cube's vertex
    volume, ball = MR.signed_volume(MR.positions(rec), faces), 4.0 / 3.0 * np.pi * (5.0 * MR.VS) ** 3
    print(f"sphere: {len(rec)} vertices, {len(faces)} faces, volume {volume:.6f} of {ball:.6f} m^3 ({100 * (1 - volume / ball):.2f} % short)")
    assert volume > 0 and abs(volume / ball - 1.0) <= 2 * 0.0239
    # the triangle normals point to the free side, as the vertex normals (the gradient of T) do
    p = MR.positions(rec).astype(np.float64)[faces]
    tri_n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    vert_n = nrm[faces[:, 0], :3].astype(np.float64)
    assert (np.einsum("ij,ij->i", tri_n, vert_n) >= 0).all() and (vert_n != 0).any()


def test_two_spheres_and_a_torus_have_their_euler_characteristics():
    T, Wt = MR.two_spheres_volume()
    faces = MR.mesh(T, Wt, None, (0.0, 0.0, 0.0), MR.VS)[2]
    assert closed_and_oriented(faces) and MR.euler(faces) == 4
    T, Wt = MR.torus_volume()
    faces = MR.mesh(T, Wt, None, (0.0, 0.0, 0.0), MR.VS)[2]
    assert closed_and_oriented(faces) and MR.euler(faces) == 0


def test_a_sphere_with_unobserved_space_is_open_and_still_a_surface():
    T, Wt = MR.sphere_volume()
    Wt = Wt.copy()
    Wt[6:10, 2:7, 3:9] = 0
    Wt[7, 7, 12] = Wt[7, 9, 12] = 0                                 # every cube around the crossing x-edge 12 -> 13 of the row y = 8, z = 7 is invalid
    T = np.where(Wt > 0, T, np.nan).astype(F)
    full = MR.mesh(*MR.sphere_volume(), None, (0.0, 0.0, 0.0), MR.VS)[2]
    rec, nrm, faces = MR.mesh(T, Wt, None, (0.0, 0.0, 0.0), MR.VS)
    d = MR.directed_edges(faces)
    assert 0 < len(faces) < len(full) and all(count == 1 for count in d.values())          # no edge in more than two faces, none twice one way
    assert any((b, a) not in d for a, b in d)                       # a boundary: not capped
    assert len(np.unique(faces)) < len(rec)                         # a vertex no face uses stays


def test_degenerate_triangles_are_kept():
    """A corner with T == 0 exactly: the crossings of its edges towards positive neighbours all lie on it."""
    T = np.ones((3, 3, 3), F)
    T[1, 1, 1] = 0.0
    rec, nrm, faces = MR.mesh(T, np.ones_like(T), None, (0.0, 0.0, 0.0), 1.0)
    assert len(rec) == 6 and len(faces) == 8 and (MR.positions(rec) == 1.0).all() and closed_and_oriented(faces)


# ---- the argument checks of the C entry points ----
def _p(k, off=0):
    """Fake device pointers 64 GiB apart: never dereferenced, every call below is refused first."""
    return ctypes.c_void_p((1 << 44) + (k << 36) + off)


def _refused(hip_lib, rc, msg, kw):
    assert rc == _lib.LWS_ERR_INVALID, kw
    assert hip_lib.lws_last_error() == msg, (kw, hip_lib.lws_last_error())


def test_mesh_rejects_bad_arguments(hip_lib):
    names = ("T", "Wt", "C", "workspace", "points", "vnormals", "faces", "counts")
    base = {name: _p(k) for k, name in enumerate(names)}

    def call(G=(8, 4, 3), o=(0.0, 0.0, 0.0), vs=0.25, w_min=0.0, max_points=100, max_faces=50, **ptrs):
        a = {**base, **ptrs}
        return hip_lib.lws_tsdf_mesh(a["T"], a["Wt"], a["C"], *G, *o, vs, w_min, max_points, max_faces, a["workspace"], a["points"], a["vnormals"],
                                     a["faces"], a["counts"], None)

    def at(name, off):
        return _p(names.index(name), off)

    w = b"tsdf_mesh: "
    null = w + b"workspace, points, faces and counts must not be null"
    al = w + b"C / faces must be 4-byte, workspace / counts 8-byte, points / vnormals 16-byte aligned"
    nan, inf = float("nan"), float("inf")
    for kw, msg in [
        (dict(T=None), w + b"T and Wt must not be null"), (dict(Wt=None), w + b"T and Wt must not be null"), (dict(workspace=None), null),
        (dict(points=None), null), (dict(faces=None), null), (dict(counts=None), null),
        (dict(G=(1, 4, 3)), w + b"bad volume Gx=1 Gy=4 Gz=3 (each in 2..4096)"), (dict(G=(8, 4097, 3)), w + b"bad volume Gx=8 Gy=4097 Gz=3 (each in 2..4096)"),
        (dict(G=(2048, 1024, 1024)), w + b"Gx*Gy*Gz = 2048x1024x1024 must be < 2^31"), (dict(o=(0.0, nan, 0.0)), w + b"the origin (0, nan, 0) must be finite"),
        (dict(vs=-1.0), w + b"vs must be finite and > 0, got -1"), (dict(vs=inf), w + b"vs must be finite and > 0, got inf"),
        (dict(T=at("T", 2)), w + b"T / Wt must be 4-byte aligned"),
        (dict(w_min=nan), w + b"w_min must be finite and >= 0, got nan"), (dict(w_min=-1.0), w + b"w_min must be finite and >= 0, got -1"),
        (dict(max_points=0), w + b"max_points 0 outside 1 .. 2^31 - 1"), (dict(max_points=1 << 31), w + b"max_points 2147483648 outside 1 .. 2^31 - 1"),
        (dict(max_faces=0), w + b"max_faces 0 outside 1 .. 2^31 - 1"), (dict(max_faces=1 << 31), w + b"max_faces 2147483648 outside 1 .. 2^31 - 1"),
        (dict(C=at("C", 2)), al), (dict(faces=at("faces", 2)), al), (dict(workspace=at("workspace", 4)), al), (dict(points=at("points", 8)), al),
        (dict(vnormals=at("vnormals", 4)), al), (dict(counts=at("counts", 4)), al),
        (dict(points=at("workspace", 496)), w + b"points and workspace overlap"), (dict(vnormals=at("points", 1600 - 16)), w + b"vnormals and points overlap"),
        (dict(faces=at("vnormals", 1596)), w + b"faces and vnormals overlap"), (dict(counts=at("faces", 600 - 8)), w + b"counts and faces overlap"),
        (dict(faces=at("counts", 12)), w + b"counts and faces overlap"), (dict(T=at("points", 0)), w + b"T and points overlap"),
        (dict(Wt=at("counts", 12)), w + b"Wt and counts overlap"), (dict(C=at("workspace", 0)), w + b"C and workspace overlap"),
        (dict(T=at("faces", 4)), w + b"T and faces overlap"),
    ]:
        _refused(hip_lib, call(**kw), msg, kw)
    # C and vnormals may be null, and the inputs may share memory: the next refusal is about something else
    _refused(hip_lib, call(C=None, vnormals=None, max_faces=-5), w + b"max_faces -5 outside 1 .. 2^31 - 1", {})
    _refused(hip_lib, call(Wt=at("T", 0), max_points=-1), w + b"max_points -1 outside 1 .. 2^31 - 1", {})
    ws = hip_lib.lws_tsdf_mesh_workspace
    assert ws(4, 3) == 256 + 256 and ws(40, 128) == 8 * 40 * 128 + (8 * 39 * 127 + 255) // 256 * 256 and ws(33, 3) == 1024 + 512
    assert ws(1, 3) == _lib.LWS_ERR_INVALID and hip_lib.lws_last_error() == b"tsdf_mesh_workspace: bad volume Gy=1 Gz=3 (each in 2..4096)"
    assert ws(4, 4097) == _lib.LWS_ERR_INVALID


def test_ops_and_the_volume_validate_before_any_gpu_call():
    import torch
    from lwsnet_amd import ops, tsdf
    T = torch.zeros((3, 4, 8))
    for kw, msg in ((dict(max_points=0, max_faces=4), "max_points must be an integer in 1"), (dict(max_points=4, max_faces=0), "max_faces must be an integer in 1"),
                    (dict(max_points=4, max_faces=1 << 31), "max_faces"), (dict(max_points=4, max_faces=2.5), "max_faces"),
                    (dict(max_points=4, max_faces=4, w_min=-1.0), "w_min must be finite and >= 0")):
        with pytest.raises(ValueError, match=msg):
            ops.tsdf_mesh(T, T, (0, 0, 0), 0.25, **kw)
    with pytest.raises(ValueError, match="voxel must be finite and > 0"):
        ops.tsdf_mesh(T, T, (0, 0, 0), 0.0, 4, 4)
    with pytest.raises(ValueError, match="dims must be"):
        ops.tsdf_mesh(None, None, (0, 0, 0), 0.25, 4, 4)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.tsdf_mesh(T, T, (0, 0, 0), 0.25, 16, 16)
    assert ops.TsdfMesh._fields == ("points", "vnormals", "faces", "counts") and ops.TsdfPoints._fields == ("points", "vnormals", "counts")
    assert callable(tsdf.TsdfVolume.mesh) and callable(tsdf.TsdfVolume.write_mesh_ply)


# ---- the header ----
EXPECTED = {"lws_tsdf_mesh": (I, [VP] * 3 + [I] * 3 + [FL] * 5 + [I64, I64] + [VP] * 6), "lws_tsdf_mesh_workspace": (I64, [I, I]), "lws_tsdf_mesh_table": (I, [VP])}


def test_the_header_is_read_into_a_table_of_its_own(hip_lib):
    from lwsnet_amd import build
    assert _lib.MESH_HEADERS == (HEADER,) == tuple(_lib.MESH_ABI)
    protos, spellings, path = _lib.MESH_ABI[HEADER]
    assert os.path.samefile(path, os.path.join(ROOT, "include", HEADER))
    assert protos == EXPECTED == _lib.MESH_PROTOTYPES and sorted(spellings) == sorted(EXPECTED)
    for name, (res, args) in EXPECTED.items():
        fn = getattr(hip_lib, name)
        assert fn.argtypes == args and fn.restype is res, name
    assert spellings["lws_tsdf_mesh"][1][11:13] == ["int64_t", "int64_t"] and spellings["lws_tsdf_mesh"][1][16] == "int32_t *"
    assert spellings["lws_tsdf_mesh"][1][-1] == "void *" and spellings["lws_tsdf_mesh_table"] == ("int", ["uint8_t *"])
    assert "lws_tsdf_mesh.hip" in build.SOURCES and hip_lib.lws_abi_version() == 8 == _lib.LWS_ABI_VERSION
    # the tables the other tests count are what they were
    assert len(_lib.HEADERS) == 5 == len(_lib.ABI) and HEADER not in _lib.HEADERS and len(_lib.PROTOTYPES) == 67 and len(_lib.ALL_PROTOTYPES) == 78
    assert not set(EXPECTED) & set(_lib.ALL_PROTOTYPES)
    assert sorted(_lib.ABI["lwsnet_tsdf.h"][0]) == ["lws_tsdf_integrate", "lws_tsdf_points", "lws_tsdf_points_workspace", "lws_tsdf_raycast"]


def test_a_compiler_agrees_with_the_reading_of_the_header(tmp_path):
    from test_abi_cpu import _assert_line, compiles
    spellings = _lib.MESH_ABI[HEADER][1]
    lines = {name: _assert_line(name, sp) for name, sp in spellings.items()}
    ok = compiles(HEADER, tmp_path / "mesh.cpp", lines.values())
    assert ok.returncode == 0, ok.stderr
    ret, params = spellings["lws_tsdf_mesh"]
    assert params[5] == "int" and params[6] == "float"             # Gz, ox
    flipped = dict(lines, lws_tsdf_mesh=_assert_line("lws_tsdf_mesh", (ret, params[:5] + ["float"] + params[6:])))
    bad = compiles(HEADER, tmp_path / "mesh_flipped.cpp", flipped.values())
    assert bad.returncode != 0 and '"lws_tsdf_mesh"' in bad.stderr and bad.stderr.count("error:") == 1, bad.stderr
    text = "static_assert(LWS_TSDF_MESH_MAX_TRIS == %d, \"max\");\n" % _lib.LWS_TSDF_MESH_MAX_TRIS
    assert compiles(HEADER, tmp_path / "mesh_max.cpp", [text]).returncode == 0


# ---- the inference CLI ----
def test_the_flag_is_off_by_default_and_leaves_the_namespace_alone(tmp_path):
    from lwsnet_amd import inference, sequence
    assert sequence.TSDF_MESH_DEFAULTS == dict(save_tsdf_mesh=None) and "save_tsdf_mesh" not in inference.TSDF_DEFAULTS
    p = inference.build_parser()
    a = p.parse_args([])
    assert not hasattr(a, "save_tsdf_mesh")
    with_flag = vars(p.parse_args(["--save_tsdf_mesh", "m.ply"]))
    assert with_flag.pop("save_tsdf_mesh") == "m.ply" and with_flag == vars(a)
    inference.check_tsdf_arguments(p, a)
    inference.check_tsdf_mesh_arguments(p, a)
    assert a.save_tsdf_mesh is None and a.save_tsdf_ply is None and not a.tsdf
    seq = _sequence_dir(tmp_path, 3)
    poses = _poses_file(tmp_path / "poses.txt", 3)
    a = p.parse_args(seq + ["--tsdf", "--poses", poses, "--save_tsdf_mesh", "m.ply"] + CAMERA)
    for check in (inference.check_occ_arguments, inference.check_geometry_arguments, inference.check_egomotion_arguments,
                  inference.check_temporal_arguments, inference.check_tsdf_arguments, inference.check_tsdf_mesh_arguments):
        check(p, a)
    assert a.tsdf and a.save_tsdf_mesh == "m.ply" and a.save_tsdf_ply is None


def test_cli_refuses_the_flag_without_tsdf(tmp_path, capsys):
    seq = _sequence_dir(tmp_path, 3)
    assert _cli_refused(seq + ["--save_tsdf_mesh", "m.ply"] + CAMERA, capsys).endswith(": error: --save_tsdf_mesh needs --tsdf\n")
    # the flags --tsdf came with keep their text
    needs = ": error: --tsdf_voxel, --tsdf_extent, --tsdf_trunc, --tsdf_trunc_px, --tsdf_weight, --tsdf_sdf, --save_tsdf_ply and --save_tsdf need --tsdf\n"
    assert _cli_refused(seq + ["--save_tsdf_ply", "x.ply"] + CAMERA, capsys).endswith(needs)
    assert _cli_refused(seq + ["--save_tsdf_ply", "x.ply", "--save_tsdf_mesh", "m.ply"] + CAMERA, capsys).endswith(needs)
    assert _cli_refused(seq + ["--tsdf", "--save_tsdf_mesh", "m.ply"] + CAMERA, capsys).endswith(": error: --tsdf needs the pose of every pair: --poses PATH or --egomotion\n")
    assert not os.path.exists(tmp_path / "out")             # refused before the output folder is touched
