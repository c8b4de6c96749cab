"""Objects without a GPU: the numpy restatement (tests/object_reference.py) finds the three boxes of the synthetic road scenes and
follows the rule on hand-made cell patterns; every argument error of lws_objects, of ops.objects and of the inference CLI's flags is
raised before any GPU work; the CSV and PNG helpers on a two-object example."""
import ctypes
import os
import re

import numpy as np
import pytest

import object_reference as O
import stixel_reference as X
from cli_helpers import CAMERA, cli_refused as _cli_refused
from conftest import ROOT
from lwsnet_amd import _lib
from test_stixels_cpu import CAM, CAM1, scene

F = np.float32
INF = float("inf")
# the parameters of the road scenes: the strips, bins and code of test_stixels_cpu.STIX
OBJ = dict(min_disp=1.0, max_depth=INF, code_bits=1 << 2, width=4, sub=4, nbins=128, min_count=4, min_pixels=64, max_objects=8)

_OBJECTS = {}


def tile():
    """(T_s, T_k): the tile of the labelling kernel, read from its source."""
    text = open(os.path.join(ROOT, "lwsnet_amd", "csrc", "lws_objects.hip")).read()
    m = re.search(r"constexpr int kTK = (\d+), kTS = (\d+);", text)
    return int(m.group(2)), int(m.group(1))


def road_objects(roll):
    """The restatement on a road scene of test_stixels_cpu, computed once: (the scene, rows, vals, labels, info of its one image)."""
    if roll not in _OBJECTS:
        s = scene(roll)
        rows, vals, labels, info = O.run(s["d"], s["cam"], s["codes"], s["udisp"][None], OBJ)
        _OBJECTS[roll] = (s, rows[0], vals[0], labels[0, 0], info[0])
    return _OBJECTS[roll]


@pytest.mark.parametrize("roll,pixels", [(0.0, (576, 504, 353)), (1.4, (575, 504, 353))])
def test_reference_finds_the_three_boxes(roll, pixels):
    """Exactly three objects, nearest first (5 m, 7 m, 11 m), each in one bin: floor(4 * 64.8 / Z) = 51, 37, 23; z within 0.05 m; the
    pixel box within a column / a row of the box's own pixels, the base up to 6 rows short (the rows within ground_tol of the road
    are ground); every taking pixel a member.  Measured: 576 / 504 / 353 pixels in 7 / 6 / 5 cells at roll 0, 575 / 504 / 353 at 1.4."""
    s, rows, vals, labels, info = road_objects(roll)
    print(f"roll {roll}: info {info.tolist()}\n{rows[:4]}\n{vals[:4]}")
    take, _ = X.taking(s["d"], s["cam"], s["codes"], 1.0, INF, 1 << 2, 4, 128)
    occupied = s["udisp"] >= OBJ["min_count"]
    assert info.tolist() == [18, 3, 3, int(take.sum())] and info[3] == s["udisp"][occupied].sum() == sum(pixels)
    assert rows[:3, 0].tolist() == list(pixels) and rows[:3, 7].tolist() == [7, 6, 5]
    assert (rows[3:] == np.array(O.EMPTY_ROW)).all() and (vals[3:].view(np.uint32) == 0).all()
    near, mid, far = s["boxes"][1], s["boxes"][0], s["boxes"][2]
    far = far & ~near                                       # the far box stands behind the near one
    for j, (box, zb, k) in enumerate(((near, 5.0, 51), (mid, 7.0, 37), (far, 11.0, 23))):
        n, x_min, x_max, y_min, y_max, k_min, k_max, cells = rows[j].tolist()
        ys, xs = np.nonzero(box)
        assert k_min == k_max == k == int(4 * 64.8 / zb)
        assert abs(float(vals[j, 1]) - zb) <= 0.05 and abs(float(vals[j, 6]) - zb) <= 0.05 and abs(float(vals[j, 7]) - zb) <= 0.05
        assert abs(x_min - xs.min()) <= 1 and abs(x_max - xs.max()) <= 1 and abs(y_min - ys.min()) <= 1
        assert ys.max() - 6 <= y_max <= ys.max()
        assert vals[j, 2] <= vals[j, 3] and vals[j, 4] <= vals[j, 5]
        x0, x1 = O.G.BOXES[(1, 0, 2)[j]][:2]               # the lateral extent in metres, within a pixel's width at that depth
        assert abs(float(vals[j, 2]) - x0) <= zb / 120.0 + 1e-3 and abs(float(vals[j, 3]) - x1) <= zb / 120.0 + 1e-3
        assert ((labels == j) == (take[0, 0] & box & (labels >= 0))).all() and (labels == j).sum() == n
    assert ((labels >= 0) == take[0, 0]).all()             # labels >= 0 lie exactly on the members: here every taking pixel


# ---- hand-made cell patterns: 8 strips of 2 columns, 16 bins of one pixel ----
HAND = dict(min_disp=1.0, max_depth=INF, code_bits=1 << 2, width=2, sub=1, nbins=16, min_count=4, min_pixels=4, max_objects=4)
# name: (the cells, the parameters that differ, the int32 rows of the written objects, info)
PATTERNS = {
    # two cells that touch only diagonally are joined
    "diagonal": ({(1, 5): 4, (2, 6): 6}, {}, [[10, 2, 5, 0, 2, 5, 6, 2]], [2, 1, 1, 10]),
    # two cells two bins apart are not
    "two_apart": ({(1, 5): 4, (1, 7): 6}, {}, [[6, 2, 3, 2, 4, 7, 7, 1], [4, 2, 3, 0, 1, 5, 5, 1]], [2, 2, 2, 10]),
    # min_count pixels make a cell, min_count - 1 do not: their pixels belong to nothing, though the cell touches the other
    "min_count": ({(3, 9): 4, (4, 9): 3}, {}, [[4, 6, 7, 0, 1, 9, 9, 1]], [1, 1, 1, 4]),
    # min_pixels members keep a component, min_pixels - 1 do not
    "min_pixels": ({(0, 3): 8, (4, 12): 7}, dict(min_count=1, min_pixels=8), [[8, 0, 1, 0, 3, 3, 3, 1]], [2, 2, 1, 8]),
    # numbered by the nearest cell, then the leftmost: (6,12)+(7,11), then (2,10), then (5,10), then (0,3)+(1,4)
    "numbering": ({(0, 3): 4, (1, 4): 4, (5, 10): 4, (2, 10): 4, (7, 11): 4, (6, 12): 4}, {},
                  [[8, 12, 15, 0, 1, 11, 12, 2], [4, 4, 5, 0, 1, 10, 10, 1], [4, 10, 11, 0, 1, 10, 10, 1], [8, 0, 3, 0, 1, 3, 4, 2]], [6, 4, 4, 24]),
    # more kept components than max_objects: the first are written, all are counted, the pixels of the rest get -1
    "cap": ({(0, 2): 4, (2, 4): 4, (4, 6): 4, (6, 8): 4, (1, 14): 2}, dict(max_objects=3, min_count=2, min_pixels=2),
            [[2, 2, 3, 0, 0, 14, 14, 1], [4, 12, 13, 0, 1, 8, 8, 1], [4, 8, 9, 0, 1, 6, 6, 1]], [5, 5, 5, 18]),
    "empty": ({}, {}, [], [0, 0, 0, 0]),
}


def pattern(name, H=8, W=16):
    """(d, codes, udisp, p, the rows expected, the info expected) of a hand-made pattern."""
    cells, kw, want_rows, want_info = PATTERNS[name]
    p = {**HAND, **kw}
    d, codes = O.cell_map(H, W, p["width"], p["sub"], cells)
    return d, codes, O.udisp_of(d, CAM1, codes, p), p, want_rows, want_info


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_reference_on_hand_made_cells(name):
    d, codes, udisp, p, want_rows, want_info = pattern(name)
    cells = PATTERNS[name][0]
    assert all(udisp[0, s, k] == n for (s, k), n in cells.items()) and udisp.sum() == sum(cells.values())
    rows, vals, labels, info = O.run(d, CAM1, codes, udisp, p)
    assert info[0].tolist() == want_info
    assert rows[0, :len(want_rows)].tolist() == want_rows
    assert (rows[0, len(want_rows):] == np.array(O.EMPTY_ROW)).all() and (vals[0, len(want_rows):].view(np.uint32) == 0).all()
    for j, r in enumerate(want_rows):
        m = labels[0, 0] == j
        assert m.sum() == r[0] and (codes[0, 0][m] == 2).all()
        dv = d[0, 0][m]
        assert vals[0, j, 0] == F(dv.astype(np.float64).mean()) and vals[0, j, 1] == F(50.0) / vals[0, j, 0]
        assert vals[0, j, 6] == (F(50.0) / dv).min() and vals[0, j, 7] == (F(50.0) / dv).max()
        ys, xs = np.nonzero(m)
        with np.errstate(divide="ignore"):
            z = F(50.0) / d[0, 0]
        assert vals[0, j, 2] == (((xs.astype(F) - F(7.5)) * z[m]) / F(100.0)).min() and vals[0, j, 5] == (((ys.astype(F) - F(15.5)) * z[m]) / F(100.0)).max()
    assert (labels >= len(want_rows)).sum() == 0 and (labels >= 0).sum() == sum(r[0] for r in want_rows)


# ---- the numbering's per-image scan takes 256 blocks of 2048 cells a round: a cell from c = 524 288 on is scanned in round two ----
WIDE = dict(min_disp=0.25, max_depth=INF, code_bits=1 << 2, width=1, sub=1, nbins=64, min_count=1, min_pixels=1, max_objects=8)
WIDE_W = 8193                                               # S = W strips of one column (W <= 16384): S * nbins = 524 352 cells, 257 blocks


def second_round_case():
    """(d, codes, udisp, p, the rows expected, the info expected) of a 2 x 8193 image whose four kept components are single cells
    of one or two pixels: in the first block, in the last block of the scan's first round, in the first block of its second round
    and in the last cell.  c = (nbins - 1 - k) * S + s; written down by hand as PATTERNS is."""
    S, nbins = WIDE_W, WIDE["nbins"]
    cells = {(5, 63): 2, (7000, 0): 1, (8130, 0): 2, (8192, 0): 1}
    c = [(nbins - 1 - k) * S + s for s, k in cells]
    assert [v // 2048 for v in c] == [0, 255, 256, 256] and c[1] < 256 * 2048 <= c[2] and c[3] == S * nbins - 1
    d, codes = O.cell_map(2, WIDE_W, WIDE["width"], WIDE["sub"], cells)
    want_rows = [[2, 5, 5, 0, 1, 63, 63, 1], [1, 7000, 7000, 0, 0, 0, 0, 1], [2, 8130, 8130, 0, 1, 0, 0, 1], [1, 8192, 8192, 0, 0, 0, 0, 1]]
    return d, codes, O.udisp_of(d, CAM1, codes, WIDE), WIDE, want_rows, [4, 4, 4, 6]


def test_reference_on_the_scan_second_round():
    d, codes, udisp, p, want_rows, want_info = second_round_case()
    rows, vals, labels, info = O.run(d, CAM1, codes, udisp, p)
    assert info[0].tolist() == want_info and rows[0, :4].tolist() == want_rows
    assert (rows[0, 4:] == np.array(O.EMPTY_ROW)).all() and (vals[0, 4:].view(np.uint32) == 0).all()
    assert [int((labels == j).sum()) for j in range(-1, 5)] == [2 * WIDE_W - 6, 2, 1, 2, 1, 0]
    assert vals[0, :4, 0].tolist() == [63.5, 0.5, 0.5, 0.5] and vals[0, :4, 1].tolist() == [float(F(50.0) / F(63.5)), 100.0, 100.0, 100.0]


def test_reference_orders_the_zeros_and_follows_a_foreign_udisp():
    """-0.0 < +0.0 in the minima and maxima (a pixel on the optical axis has X = +0.0, one left of it times a tiny z may give -0.0);
    a udisp that is not the map's own is followed as it is: occupied and joined come from it alone."""
    assert O.ordered_min(np.array([0.0, -0.0, 1.0], F)).view(np.uint32) == 0x80000000
    assert O.ordered_max(np.array([-0.0, 0.0, -1.0], F)).view(np.uint32) == 0
    assert O.ordered_max(np.array([-0.0, -1.0], F)).view(np.uint32) == 0x80000000
    d, codes, udisp, p, _, _ = pattern("two_apart")
    udisp[0, 1, 6] = 9                                      # a bridge no pixel stands in
    udisp[0, 1, 7] = 0                                      # ... and the far cell emptied: its six pixels belong to nothing
    rows, _, labels, info = O.run(d, CAM1, codes, udisp, p)
    assert info[0].tolist() == [2, 1, 1, 4] and rows[0, 0].tolist() == [4, 2, 3, 0, 1, 5, 6, 2] and (labels >= 0).sum() == 4


# ---- C ABI argument checks (no GPU call is reached) ----
def _p(k, off=0):
    """Fake device pointers 1 GiB apart: never dereferenced, every call below is refused first."""
    return ctypes.c_void_p((1 << 40) + (k << 30) + off)


def test_objects_rejects_bad_arguments(hip_lib):
    names = ("disp", "cam", "codes", "udisp", "workspace", "rows", "vals", "labels", "info")
    base = {name: _p(k) for k, name in enumerate(names)}

    def call(B=1, H=8, W=16, min_disp=1.0, max_depth=INF, code_bits=4, width=4, sub=4, nbins=64, min_count=4, min_pixels=64, max_objects=8, **ptrs):
        a = {**base, **ptrs}
        return hip_lib.lws_objects(a["disp"], a["cam"], a["codes"], a["udisp"], B, H, W, min_disp, max_depth, code_bits, width, sub, nbins, min_count,
                                   min_pixels, max_objects, a["workspace"], a["rows"], a["vals"], a["labels"], a["info"], None)

    def at(name, off):
        return _p(names.index(name), off)

    null_in, null_out = b"objects: cam, codes and udisp must not be null", b"objects: workspace, rows, vals and info must not be null"
    al = b"objects: cam / udisp / rows / vals / labels / info must be 4-byte, workspace 16-byte aligned"
    ws = hip_lib.lws_objects_workspace(1, 16, 4, 64)
    assert ws == 256 * 4 + 256 * 64 + 256                   # 256 cells: the parent words, the records, one block's four counts
    for kw, msg in [
        (dict(disp=None), b"objects: disp is null"), (dict(cam=None), null_in), (dict(codes=None), null_in), (dict(udisp=None), null_in),
        (dict(workspace=None), null_out), (dict(rows=None), null_out), (dict(vals=None), null_out), (dict(info=None), null_out),
        (dict(disp=at("disp", 2)), b"objects: disp is not 4-byte aligned"), (dict(cam=at("cam", 2)), al), (dict(udisp=at("udisp", 1)), al),
        (dict(rows=at("rows", 2)), al), (dict(vals=at("vals", 3)), al), (dict(labels=at("labels", 2)), al), (dict(info=at("info", 2)), al),
        (dict(workspace=at("workspace", 8)), al),
        (dict(B=0), b"objects: bad shape B=0 H=8 W=16"), (dict(W=0), b"objects: bad shape B=1 H=8 W=0"),
        (dict(H=16385), b"objects: H=16385 W=16 exceed 16384 (the 64-bit sums)"), (dict(W=16385), b"objects: H=8 W=16385 exceed 16384 (the 64-bit sums)"),
        (dict(min_disp=0.0), b"objects: min_disp must be finite and > 0, got 0"),
        (dict(max_depth=float("nan")), b"objects: max_depth must be > 0 (+inf allowed), got nan"),
        (dict(code_bits=-1), b"objects: code_bits -1 outside 0..63"), (dict(code_bits=64), b"objects: code_bits 64 outside 0..63"),
        (dict(width=0), b"objects: width 0 outside 1..64"), (dict(width=65), b"objects: width 65 outside 1..64"),
        (dict(sub=0), b"objects: sub 0 outside 1..16"), (dict(sub=17), b"objects: sub 17 outside 1..16"),
        (dict(nbins=0), b"objects: nbins 0 outside 1..4096"), (dict(nbins=4097, sub=16), b"objects: nbins 4097 outside 1..4096"),
        (dict(nbins=1025), b"objects: nbins 1025 outside 1..min(4096, 256 * sub = 1024)"),
        (dict(W=16384, width=1, sub=16, nbins=257), b"objects: S * nbins = 16384 * 257 exceeds 4194304 cells (the workspace would pass 286 MB per image)"),
        (dict(min_count=0), b"objects: min_count 0 < 1"), (dict(min_pixels=0), b"objects: min_pixels 0 < 1"),
        (dict(max_objects=0), b"objects: max_objects 0 outside 1..65536"), (dict(max_objects=65537), b"objects: max_objects 65537 outside 1..65536"),
        (dict(rows=at("workspace", ws - 4)), b"objects: rows and workspace overlap"), (dict(vals=at("rows", 8 * 32 - 4)), b"objects: vals and rows overlap"),
        (dict(labels=at("vals", 0)), b"objects: labels and vals overlap"), (dict(info=at("labels", 4 * 8 * 16 - 4)), b"objects: info and labels overlap"),
        (dict(disp=at("info", 12)), b"objects: disp and info overlap"), (dict(cam=at("rows", 0)), b"objects: cam and rows overlap"),
        (dict(codes=at("workspace", 64)), b"objects: codes and workspace overlap"), (dict(udisp=at("vals", 64)), b"objects: udisp and vals overlap"),
        (dict(udisp=at("workspace", ws - 4)), b"objects: udisp and workspace overlap"),
    ]:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert hip_lib.lws_last_error() == msg, (kw, hip_lib.lws_last_error())
    # a code_bits with the bits of ground and of the codes without a height is taken: the next refusal is about something else
    assert call(code_bits=0x3f, labels=None, min_pixels=0) == _lib.LWS_ERR_INVALID and hip_lib.lws_last_error() == b"objects: min_pixels 0 < 1"
    for dims, msg in (((0, 16, 4, 64), b"objects_workspace: bad shape B=0 W=16 (W <= 16384)"), ((1, 16, 0, 64), b"objects_workspace: width 0 outside 1..64"),
                      ((1, 16, 4, 4097), b"objects_workspace: nbins 4097 outside 1..4096")):
        assert hip_lib.lws_objects_workspace(*dims) == _lib.LWS_ERR_INVALID and hip_lib.lws_last_error() == msg
    assert hip_lib.lws_objects_workspace(3, 13, 4, 70) == (3 * 4 * 70 * 4 // 256 * 256 + 256) + 3 * 4 * 70 * 64 + 256
    assert hip_lib.lws_objects_workspace(2, 1232, 8, 768) == 2 * 154 * 768 * 68 + 2048          # 58 blocks of 2048 cells an image: 1856 bytes of counts
    assert tile() == (64, 32)


def test_ops_validate_before_any_gpu_call():
    from lwsnet_amd import ops
    z = np.zeros((1, 1, 2, 2), F)
    with pytest.raises(ValueError, match="objects needs cameras"):
        ops.objects(z, None, None, None)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.objects(z, CAM, None, None)
    for kw, msg in ((dict(min_disp=0.0), "min_disp"), (dict(code_bits=64), "code_bits must be an integer in 0 .. 63"), (dict(width=0), "width must be an integer in 1 .. 64"),
                    (dict(width=65), "width"), (dict(width=2.5), "width"), (dict(sub=17), "sub"), (dict(min_count=0), "min_count"),
                    (dict(min_pixels=0), "min_pixels"), (dict(max_objects=0), "max_objects"), (dict(max_objects=65537), "max_objects must be an integer in 1 .. 65536")):
        with pytest.raises(ValueError, match=msg):
            ops.objects(None, CAM, None, None, **kw)
    assert ops._object_args(1.0, 4, 8, 4, None, 64, 256) == (1.0, 4, 8, 4, 8, 64, 256)        # min_count None is width
    assert ops._object_args(1.0, 0x3f, 3, 1, 2, 1, 1)[1:5] == (0x3f, 3, 1, 2)                  # no bit of code_bits is refused
    assert ops.ObjectResult._fields == ("rows", "vals", "labels", "info")


# ---- the inference CLI ----
NEW_FLAGS = ("objects", "save_objects", "object_min_pixels")


def test_object_flags_default_off():
    from lwsnet_amd import inference
    p = inference.build_parser()
    a = p.parse_args([])
    assert not any(hasattr(a, name) for name in NEW_FLAGS)                      # the namespace of a line without them
    with_flags = vars(p.parse_args(["--objects", "--save_objects", "--object_min_pixels", "9"]))
    assert {k: v for k, v in with_flags.items() if k not in NEW_FLAGS} == vars(a)
    inference.check_geometry_arguments(p, a)
    assert (a.objects, a.save_objects, a.object_min_pixels, a.stixels, a.ground) == (False, False, 64, False, False)
    assert not inference._geometry_requested(a)
    a = p.parse_args(["--save_objects", "--object_min_pixels", "9"] + CAMERA)
    inference.check_geometry_arguments(p, a)
    assert (a.objects, a.save_objects, a.object_min_pixels) == (True, True, 9)
    assert a.stixels and a.ground and not a.save_stixels and not a.save_ground and inference._geometry_requested(a)


@pytest.mark.parametrize("flag", ["--objects", "--save_objects"])
def test_cli_refuses_objects_without_camera_or_with_workers(flag, capsys):
    assert _cli_refused([flag], capsys).endswith(
        ": error: --objects and --save_objects need a camera: --calib PATH or --camera FX FY CX CY BASELINE\n")
    assert _cli_refused([flag, "--workers", "2"] + CAMERA, capsys).endswith(
        ": error: --objects / --save_objects run in the sequential mode only: use --workers 0\n")
    assert _cli_refused([flag, "--object_min_pixels", "0"] + CAMERA, capsys).endswith(": error: --object_min_pixels must be >= 1, got 0\n")


def test_object_file_helpers():
    from lwsnet_amd import inference, outputs
    rows = np.array([[6, 1, 3, 0, 2, 9, 10, 2], [2, 0, 0, 2, 3, 4, 4, 1], [0, -1, -1, -1, -1, -1, -1, 0]], np.int32)
    vals = np.zeros((3, 8), F)
    vals[0] = (9.5, 7.5, -1.25, 1.5, -0.5, 0.25, 7.25, 7.75)
    vals[1] = (4.25, 15.0, -3.0, -3.0, 0.5, 0.75, 15.0, 15.0)
    assert outputs.objects_to_csv(rows, vals) == (
        "object,n,x_min,x_max,y_min,y_max,k_min,k_max,cells,disparity,z,X_min,X_max,Y_min,Y_max,Z_min,Z_max\n"
        "0,6,1,3,0,2,9,10,2,9.500000,7.500000,-1.250000,1.500000,-0.500000,0.250000,7.250000,7.750000\n"
        "1,2,0,0,2,3,4,4,1,4.250000,15.000000,-3.000000,-3.000000,0.500000,0.750000,15.000000,15.000000\n")
    left = np.full((4, 5, 3), 100, np.uint8)
    labels = np.full((4, 5), -1, np.int32)
    labels[0, 1:4], labels[1, 2], labels[2:4, 0] = 0, 0, 1
    rgb = inference.objects_to_rgb(rows, labels, left)
    assert rgb.dtype == np.uint8 and rgb.shape == (4, 5, 3)
    c0, c1 = (outputs.OBJECT_COLOURS[j].astype(int) for j in (0, 1))
    assert rgb[3, 4].tolist() == [100, 100, 100]                                # outside every object and box: the grey
    assert rgb[1, 2].tolist() == ((c0 + 100 + 1) >> 1).tolist()                 # a member inside the box: tinted
    assert rgb[0, 1].tolist() == rgb[1, 1].tolist() == rgb[2, 3].tolist() == rgb[2, 2].tolist() == c0.tolist()  # the outline of the box x 1..3, y 0..2
    assert rgb[2, 0].tolist() == rgb[3, 0].tolist() == c1.tolist()              # a box one pixel wide is all outline
    assert len(outputs.OBJECT_COLOURS) >= 8 and len({tuple(c) for c in outputs.OBJECT_COLOURS.tolist()}) == len(outputs.OBJECT_COLOURS)
