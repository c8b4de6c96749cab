"""The volume that follows the camera, without a GPU: the numpy restatement of lws_tsdf_window (tests/tsdf_window_reference.py)
held to the rule voxel by voxel; spill_boxes held by brute force to "each lost cell once, kept cells never"; the conservation of the
mesh -- the triangles of a volume are those of the spill boxes plus those of the shifted volume, bit for bit -- with the numpy
marching cubes of tests/tsdf_mesh_reference.py; follow_shift and the origin's bookkeeping; MeshChunks; the argument checks of the C
entry point and of lwsnet_amd.ops.tsdf_window; the reading of include/lwsnet_tsdf_window.h; the inference CLI's flag."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import tsdf_mesh_reference as MR
import tsdf_window_reference as WR
from cli_helpers import CAMERA, cli_refused as _cli_refused, poses_file as _poses_file, sequence_dir as _sequence_dir
from conftest import ROOT
from lwsnet_amd import _lib

F = np.float32
VP, I = ctypes.c_void_p, ctypes.c_int
HEADER = "lwsnet_tsdf_window.h"
G = (11, 9, 10)
SHIFTS = [(3, 0, 0), (-2, 0, 0), (0, 0, 4), (2, -3, 1), (-5, 2, -1), (9, 0, 0), (10, 1, 0), (1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, -1)]


# ---- the restatement ----
@pytest.mark.parametrize("shift,dims", [((0, 0, 0), None), ((2, -1, 3), None), ((-3, 2, -1), None), ((7, 0, 0), None), ((0, -6, 0), None),
                                        ((1, 2, 0), (4, 3, 5)), ((-2, -1, -2), (10, 8, 9)), ((3, 3, 3), (2, 2, 2))])
def test_the_restatement_is_the_rule_voxel_by_voxel(shift, dims):
    T, Wt, C, _, _ = WR.noise_volume((7, 6, 5), 1, holes=0.2, special=True)
    assert np.isnan(Wt).any() and np.isinf(Wt).any() and (Wt < 0).any() and (np.signbit(Wt) & (Wt == 0)).any()
    fast, slow = WR.window(T, Wt, C, shift, dims), WR.window_by_voxel(T, Wt, C, shift, dims)
    for a, b in zip(fast[:3], slow[:3]):
        assert WR.same_bits(a, b)
    assert fast[3] == slow[3] and sum(fast[3]) == fast[0].size
    T2, Wt2, C2, (live, dead) = fast
    with np.errstate(invalid="ignore"):
        cleared = Wt2 == 0
    assert not np.signbit(Wt2[cleared]).any() and not T2[cleared].view(np.uint32).any() and not C2[cleared].any()      # +0.0, +0.0, {0, 0, 0, 0}
    assert int(cleared.sum()) == dead
    if shift == (7, 0, 0):
        assert live == 0 and not T2.view(np.uint32).any()
    if shift == (0, 0, 0) and dims is None:
        keep = ~cleared
        assert WR.same_bits(T2[keep], T[keep]) and WR.same_bits(Wt2[keep], Wt[keep]) and (C2[keep] == C[keep]).all()
        assert not np.isnan(T2[cleared]).any() and np.isnan(T[cleared]).all()       # the poison is scrubbed


def test_no_colour():
    T, Wt, C, _, _ = WR.noise_volume((7, 6, 5), 2)
    T2, Wt2, C2, counts = WR.window(T, Wt, None, (1, 0, -1))
    assert C2 is None and WR.same_bits(T2, WR.window(T, Wt, C, (1, 0, -1))[0])


# ---- spill_boxes ----
def cells(dims):
    return itertools.product(*(range(n - 1) for n in dims))


def kept(dims, shift, cell):
    return all(max(0, s) <= i and i + 1 <= min(n, n + s) - 1 for n, s, i in zip(dims, shift, cell))


@pytest.mark.parametrize("shift", SHIFTS + [(0, 0, 0), (0, 8, 0), (0, 0, -9), (-11, 0, 0), (4096, 0, 0)])
def test_spill_boxes_hold_each_lost_cell_once_and_no_kept_cell(shift):
    from lwsnet_amd.tsdf import spill_boxes
    boxes = spill_boxes(G, shift)
    for start, box in boxes:
        assert all(b >= 2 and 0 <= a and a + b <= n for a, b, n in zip(start, box, G)), (start, box)
    lost = 0
    for cell in cells(G):
        n = sum(all(a <= i and i + 1 <= a + b - 1 for a, b, i in zip(start, box, cell)) for start, box in boxes)
        assert n == (0 if kept(G, shift, cell) else 1), (shift, cell, n)
        lost += n
    if shift == (0, 0, 0):
        assert boxes == []
    if any(abs(s) >= n - 1 for s, n in zip(shift, G)):      # fewer than two layers stay on some axis: nothing is kept
        assert boxes == [((0, 0, 0), G)] and lost == 10 * 8 * 9
    if shift == (2, -3, 1):
        assert boxes == [((0, 0, 0), (3, 9, 10)), ((2, 5, 0), (9, 4, 10)), ((2, 0, 0), (9, 6, 2))]


def test_spill_boxes_refuses_what_is_not_a_volume():
    from lwsnet_amd.tsdf import spill_boxes
    for dims, shift in (((1, 4, 4), (0, 0, 0)), ((4, 4), (0, 0, 0)), ((4, 4, 4), (1, 2))):
        with pytest.raises(ValueError, match="spill_boxes takes"):
            spill_boxes(dims, shift)


# ---- conservation ----
_WHOLE = {}


def whole_mesh():
    """The noise volume of the conservation tests and its mesh, computed once (tests/test_gpu_tsdf_window.py shares it)."""
    if not _WHOLE:
        T, Wt, C, origin, vs = WR.noise_volume(G, 3)
        rec, nrm, faces = MR.mesh(T, Wt, C, origin, vs)
        _WHOLE.update(volume=(T, Wt, C, origin, vs), rec=rec, faces=faces, triangles=WR.triangles(rec, faces))
    return _WHOLE


@pytest.mark.parametrize("shift", SHIFTS)
def test_the_spill_boxes_and_the_shifted_volume_hold_the_triangles_of_the_whole(shift):
    """The multiset of triangles, as triples of 16-byte vertex records: what the boxes spill plus what the shifted volume still
    holds is what the whole volume held, bit for bit.  Normals are not compared: at a box's border they are zero."""
    from lwsnet_amd.tsdf import spill_boxes
    w = whole_mesh()
    T, Wt, C, origin, vs = w["volume"]
    assert (Wt == 0).any() and (T[Wt > 0] == 0).any() and len(w["rec"]) > 500 and len(w["faces"]) > 500
    parts, seen = [], 0
    for start, box in spill_boxes(G, shift) + [(shift, G)]:             # the boxes, then the shifted volume
        T2, Wt2, C2, _ = WR.window(T, Wt, C, start, box)
        rec, nrm, faces = MR.mesh(T2, Wt2, C2, WR.moved_origin(origin, start, vs), vs)
        parts += WR.triangles(rec, faces)
        seen += len(rec)
    print(f"shift {shift}: {len(w['rec'])} vertices and {len(w['faces'])} faces in the whole volume, {seen} vertices in the parts")
    assert sorted(parts) == w["triangles"]
    assert seen >= len(np.unique(w["faces"]))                            # a seam vertex is in both parts that meet there


# ---- follow_shift and the origin ----
def test_follow_shift_is_the_float64_rule():
    from lwsnet_amd.tsdf import follow_shift
    assert follow_shift((0, 0, 0), (0.74, 0.0, -0.74), 0.25, 3) == (0, 0, 0)                # |d| = 2.96 < 3
    assert follow_shift((0, 0, 0), (0.75, 0.0, -0.3), 0.25, 3) == (3, 0, -1)                # 3.0 >= 3: every axis is rounded
    assert follow_shift((1.0, 2.0, 3.0), (1.0, 2.0, 7.1), 0.2, 16) == (0, 0, 20)            # 20.4999..: float64, to nearest
    assert follow_shift((0, 0, 0), (0.625, -0.625, 0.375), 0.25, 1) == (2, -2, 2)           # 2.5, -2.5, 1.5: rint is to even
    assert follow_shift((0, 0, 0), (0.2, 0.0, 0.0), 0.2, 1) == (1, 0, 0)
    d = (np.float64(3.3) - np.float64(0.1)) / np.float64(0.2)
    assert follow_shift((0.1, 0, 0), (3.3, 0, 0), 0.2, 16) == ((int(np.rint(d)), 0, 0) if abs(d) >= 16 else (0, 0, 0))
    for bad in ((0, 0), (np.nan, 0, 0)):
        with pytest.raises(ValueError, match="follow_shift takes"):
            follow_shift((0, 0, 0), bad, 0.2, 1)


def test_the_origin_is_float32_of_a_float64_sum_and_a_shift_and_its_reverse_restore_its_bits():
    from lwsnet_amd.tsdf import window_origin
    origin0, vs = (-12.8, -3.2, 0.1), 0.2
    offset = np.zeros(3, np.int64)
    first = window_origin(origin0, offset, vs)
    assert first == tuple(float(F(v)) for v in origin0)
    for s in ((16, 0, 3), (7, -2, 33), (-16, 0, -3), (-7, 2, -33)):        # out and back: the offset is an integer again zero
        offset = offset + np.array(s)
        got = window_origin(origin0, offset, vs)
        want = tuple(float(np.float32(np.float64(o) + np.float64(k) * np.float64(vs))) for o, k in zip(origin0, offset))
        assert np.array(got, F).tobytes() == np.array(want, F).tobytes()
    assert np.array(got, F).tobytes() == np.array(first, F).tobytes()
    # a running float32 sum would not come back: the rule is not that
    run = F(origin0[0])
    for k in (16, 7, -16, -7):
        run = F(run + F(k) * F(vs))
    print("a running float32 origin after out and back:", repr(run), "against", repr(F(origin0[0])))


# ---- MeshChunks ----
def test_mesh_chunks_offset_the_faces_and_write_both_files(tmp_path):
    from lwsnet_amd.geometry import read_mesh_ply
    from lwsnet_amd.tsdf import Chunk, MeshChunks
    rng = np.random.default_rng(5)
    a = Chunk(rng.integers(0, 256, (4, 16), dtype=np.uint8), rng.uniform(-1, 1, (4, 4)).astype(F), np.array([[0, 1, 2], [1, 3, 2]], np.int32))
    b = Chunk(rng.integers(0, 256, (3, 16), dtype=np.uint8), rng.uniform(-1, 1, (3, 4)).astype(F), np.array([[2, 1, 0]], np.int32))
    empty = Chunk(np.zeros((0, 16), np.uint8), np.zeros((0, 4), F), np.zeros((0, 3), np.int32))
    for c in (a, b):
        c.points[:, :12] = rng.uniform(-4, 4, (len(c.points), 3)).astype(F).view(np.uint8)
    chunks = MeshChunks()
    for c in (a, empty, b):
        chunks.append(c)
    assert (chunks.vertices, chunks.triangles) == (7, 3)
    mesh, cloud = str(tmp_path / "m.ply"), str(tmp_path / "p.ply")
    assert chunks.write(mesh) == (7, 3) and chunks.write(cloud, faces=False) == (7, 0)
    verts, faces = read_mesh_ply(mesh)
    assert faces.tolist() == [[0, 1, 2], [1, 3, 2], [6, 5, 4]] and len(read_mesh_ply(cloud)[1]) == 0
    assert verts.tobytes() == read_mesh_ply(cloud)[0].tobytes()
    assert np.stack([verts["x"], verts["y"], verts["z"]], -1).tobytes() == np.concatenate([a.points, b.points])[:, :12].tobytes()
    assert MeshChunks().write(str(tmp_path / "none.ply")) == (0, 0)

    class Many:                                             # a chunk that only claims its size: the refusal comes before anything is copied
        points, vnormals, faces = np.broadcast_to(np.zeros((1, 16), np.uint8), ((1 << 31) - 7, 16)), None, None
    with pytest.raises(ValueError, match="a face indexes fewer than 2\\^31"):
        chunks.append(Many)
    assert chunks.vertices == 7


# ---- the argument checks of the C entry point ----
def _p(k, off=0):
    """Fake device pointers 64 GiB apart: never dereferenced, every call below is refused first."""
    return ctypes.c_void_p((1 << 44) + (k << 36) + off)


def test_window_rejects_bad_arguments(hip_lib):
    names = ("T", "Wt", "C", "T2", "Wt2", "C2", "counts")
    base = {name: _p(k) for k, name in enumerate(names)}

    def call(G=(8, 4, 3), s=(1, 0, -1), D=(8, 4, 3), **ptrs):
        a = {**base, **ptrs}
        return hip_lib.lws_tsdf_window(a["T"], a["Wt"], a["C"], *G, *s, a["T2"], a["Wt2"], a["C2"], *D, a["counts"], None)

    def at(name, off):
        return _p(names.index(name), off)

    w = b"tsdf_window: "
    null, both = w + b"T, Wt, T2 and Wt2 must not be null", w + b"C and C2 must be given together (both null: no colour)"
    al = w + b"T / Wt / C / T2 / Wt2 / C2 must be 4-byte, counts 8-byte aligned"
    for kw, msg in [
        (dict(T=None), null), (dict(Wt=None), null), (dict(T2=None), null), (dict(Wt2=None), null), (dict(C=None), both), (dict(C2=None), both),
        (dict(G=(1, 4, 3)), w + b"bad source volume 1x4x3 (each in 2..4096)"), (dict(G=(8, 4097, 3)), w + b"bad source volume 8x4097x3 (each in 2..4096)"),
        (dict(D=(8, 4, 1)), w + b"bad destination volume 8x4x1 (each in 2..4096)"), (dict(D=(4097, 4, 3)), w + b"bad destination volume 4097x4x3 (each in 2..4096)"),
        (dict(G=(2048, 1024, 1024)), w + b"the source volume 2048x1024x1024 must hold fewer than 2^31 voxels"),
        (dict(D=(2048, 1024, 1024)), w + b"the destination volume 2048x1024x1024 must hold fewer than 2^31 voxels"),
        (dict(s=(4097, 0, 0)), w + b"bad shift (4097, 0, 0) (each in -4096..4096)"), (dict(s=(0, -4097, 0)), w + b"bad shift (0, -4097, 0) (each in -4096..4096)"),
        (dict(s=(0, 0, 1 << 30)), w + b"bad shift (0, 0, 1073741824) (each in -4096..4096)"),
        (dict(T=at("T", 2)), al), (dict(Wt=at("Wt", 1)), al), (dict(C=at("C", 2)), al), (dict(T2=at("T2", 3)), al), (dict(Wt2=at("Wt2", 2)), al),
        (dict(C2=at("C2", 1)), al), (dict(counts=at("counts", 4)), al),
        (dict(T2=at("T", 0)), w + b"T and T2 overlap"), (dict(T2=at("T", 380)), w + b"T and T2 overlap"), (dict(Wt2=at("T2", 0)), w + b"Wt2 and T2 overlap"),
        (dict(Wt2=at("Wt", 4)), w + b"Wt and Wt2 overlap"), (dict(C2=at("C", 0)), w + b"C and C2 overlap"), (dict(C2=at("Wt2", 380)), w + b"C2 and Wt2 overlap"),
        (dict(counts=at("T2", 376)), w + b"counts and T2 overlap"), (dict(counts=at("Wt", 0)), w + b"Wt and counts overlap"),
        (dict(T=at("counts", 8)), w + b"T and counts overlap"), (dict(T2=at("Wt", 0), D=(2, 2, 2)), w + b"Wt and T2 overlap"),
    ]:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert hip_lib.lws_last_error() == msg, (kw, hip_lib.lws_last_error())
    # colour and counts may be null on both sides, and the inputs may share memory: the next refusal is about something else
    assert call(C=None, C2=None, counts=None, s=(0, 0, 5000)) == _lib.LWS_ERR_INVALID and hip_lib.lws_last_error() == w + b"bad shift (0, 0, 5000) (each in -4096..4096)"
    assert call(Wt=at("T", 0), s=(-5000, 0, 0)) == _lib.LWS_ERR_INVALID and hip_lib.lws_last_error().startswith(w + b"bad shift")


def test_ops_and_the_volume_validate_before_any_gpu_call():
    import torch
    from lwsnet_amd import ops, tsdf
    T = torch.zeros((3, 4, 8))
    for kw, msg in ((dict(offset=(0, 0)), "offset must be"), (dict(offset=(0, 0, 4097)), r"offset\[2\] must be an integer in -4096 .. 4096"),
                    (dict(offset=(0.5, 0, 0)), r"offset\[0\]"), (dict(offset=(0, 0, 0), dims=(8, 4)), "out_dims must be"),
                    (dict(offset=(0, 0, 0), dims=(8, 1, 3)), r"out_dims\[1\] must be an integer in 2 .. 4096"),
                    (dict(offset=(0, 0, 0), dims=(2048, 1024, 1024)), "fewer than 2\\^31 voxels")):
        with pytest.raises(ValueError, match=msg):
            ops.tsdf_window(T, T, **kw)
    with pytest.raises(ValueError, match="dims must be"):
        ops.tsdf_window(None, None, (0, 0, 0))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.tsdf_window(T, T, (1, 0, 0))
    assert ops.tsdf_window_args((8, 4, 3), (1, -2, 0)) == (8, 4, 3, 1, -2, 0, 8, 4, 3)
    assert ops.tsdf_window_args((8, 4, 3), (0, 0, 0), (2, 3, 4)) == (8, 4, 3, 0, 0, 0, 2, 3, 4)
    assert ops.TsdfWindow._fields == ("T", "Wt", "C", "counts")
    for name in ("shift", "follow", "chunk", "centre"):
        assert callable(getattr(tsdf.TsdfVolume, name))
    with pytest.raises(RuntimeError, match="HIP device"):
        tsdf.TsdfVolume((0, 0, 0), 0.25, (8, 4, 3), mu0=0.5, device="cpu")


# ---- the header ----
EXPECTED = {"lws_tsdf_window": (I, [VP] * 3 + [I] * 6 + [VP] * 3 + [I] * 3 + [VP] * 2)}


def test_the_header_is_read_into_a_table_of_its_own(hip_lib):
    from lwsnet_amd import build
    assert _lib.WINDOW_HEADERS == (HEADER,) == tuple(_lib.WINDOW_ABI)
    protos, spellings, path = _lib.WINDOW_ABI[HEADER]
    assert os.path.samefile(path, os.path.join(ROOT, "include", HEADER))
    assert protos == EXPECTED == _lib.WINDOW_PROTOTYPES and sorted(spellings) == sorted(EXPECTED)
    fn = hip_lib.lws_tsdf_window
    assert fn.argtypes == EXPECTED["lws_tsdf_window"][1] and fn.restype is I
    ret, params = spellings["lws_tsdf_window"]
    assert ret == "int" and params[:3] == ["const float *", "const float *", "const uint8_t *"] and params[9:12] == ["float *", "float *", "uint8_t *"]
    assert params[15:] == ["int64_t *", "void *"] and params[3:9] == ["int"] * 6
    assert "lws_tsdf_window.hip" in build.SOURCES and hip_lib.lws_abi_version() == 8 == _lib.LWS_ABI_VERSION
    # the tables the other tests count are what they were
    assert len(_lib.HEADERS) == 5 == len(_lib.ABI) and HEADER not in _lib.HEADERS and len(_lib.ALL_PROTOTYPES) == 78
    assert not set(EXPECTED) & (set(_lib.ALL_PROTOTYPES) | set(_lib.MESH_PROTOTYPES) | set(_lib.TRACK_PROTOTYPES))


def test_a_compiler_agrees_with_the_reading_of_the_header(tmp_path):
    from test_abi_cpu import _assert_line, compiles
    spellings = _lib.WINDOW_ABI[HEADER][1]
    lines = {name: _assert_line(name, sp) for name, sp in spellings.items()}
    ok = compiles(HEADER, tmp_path / "window.cpp", lines.values())
    assert ok.returncode == 0, ok.stderr
    ret, params = spellings["lws_tsdf_window"]
    flipped = {"lws_tsdf_window": _assert_line("lws_tsdf_window", (ret, params[:8] + ["float"] + params[9:]))}
    bad = compiles(HEADER, tmp_path / "window_flipped.cpp", flipped.values())
    assert bad.returncode != 0 and '"lws_tsdf_window"' in bad.stderr and bad.stderr.count("error:") == 1, bad.stderr


# ---- the inference CLI ----
def test_the_flag_is_off_by_default_and_leaves_the_namespace_alone(tmp_path):
    from lwsnet_amd import inference, sequence
    assert sequence.TSDF_FOLLOW_DEFAULTS == dict(tsdf_follow=None) and "tsdf_follow" not in inference.TSDF_DEFAULTS
    assert "tsdf_follow" not in sequence.TSDF_MESH_DEFAULTS and inference.TSDF_FOLLOW_DEFAULTS is sequence.TSDF_FOLLOW_DEFAULTS
    p = inference.build_parser()
    a = p.parse_args([])
    assert not hasattr(a, "tsdf_follow")
    with_flag = vars(p.parse_args(["--tsdf_follow"]))
    assert with_flag.pop("tsdf_follow") == 16 == sequence.TSDF_FOLLOW_STEP and with_flag == vars(a)
    assert p.parse_args(["--tsdf_follow", "5"]).tsdf_follow == 5
    inference.check_tsdf_arguments(p, a)
    inference.check_tsdf_mesh_arguments(p, a)
    inference.check_tsdf_follow_arguments(p, a)
    assert a.tsdf_follow is None and not a.tsdf
    seq = _sequence_dir(tmp_path, 3)
    poses = _poses_file(tmp_path / "poses.txt", 3)
    for given, want in ((["--tsdf_follow"], 16), (["--tsdf_follow", "1"], 1), (["--tsdf_follow", "30"], 30), ([], None)):
        a = p.parse_args(seq + ["--tsdf", "--poses", poses] + given + CAMERA)
        for check in (inference.check_occ_arguments, inference.check_geometry_arguments, inference.check_egomotion_arguments,
                      inference.check_temporal_arguments, inference.check_tsdf_arguments, inference.check_tsdf_mesh_arguments,
                      inference.check_tsdf_follow_arguments):
            check(p, a)
        assert a.tsdf and a.tsdf_follow == want


def test_cli_refuses_the_flag_without_tsdf_and_a_step_out_of_range(tmp_path, capsys):
    seq = _sequence_dir(tmp_path, 3)
    poses = _poses_file(tmp_path / "poses.txt", 3)
    assert _cli_refused(seq + ["--tsdf_follow"] + CAMERA, capsys).endswith(": error: --tsdf_follow needs --tsdf\n")
    assert _cli_refused(seq + ["--tsdf_follow", "4"] + CAMERA, capsys).endswith(": error: --tsdf_follow needs --tsdf\n")
    run = seq + ["--tsdf", "--poses", poses] + CAMERA
    # the default volume is 129 x 33 x 257 voxels: N < 33 - 2
    out_of_range = ": error: --tsdf_follow must be at least 1 and below the volume's smallest dimension minus 2 = 31 voxels, got {}\n"
    for n in ("0", "-3", "31", "400"):
        assert _cli_refused(run + ["--tsdf_follow", n], capsys).endswith(out_of_range.format(n))
    small = run + ["--tsdf_voxel", "0.5", "--tsdf_extent", "-2", "2", "-1", "1", "0", "8"]        # 9 x 5 x 17 voxels: N < 3
    assert _cli_refused(small + ["--tsdf_follow", "3"], capsys).endswith(": error: --tsdf_follow must be at least 1 and below the volume's smallest dimension minus 2 = 3 voxels, got 3\n")
    assert "invalid int value" in _cli_refused(run + ["--tsdf_follow", "2.5"], capsys)
    assert not os.path.exists(tmp_path / "out")             # refused before the output folder is touched
