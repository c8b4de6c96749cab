"""Stixels without a GPU: the numpy restatement (tests/stixel_reference.py) finds the boxes of the synthetic road scenes and
follows the rule on hand-made columns; every argument error of lws_stixels, of ops.stixels and of the inference CLI's flags is
raised before any GPU work; the CSV and PNG helpers on a two-stixel example."""
import ctypes

import numpy as np
import pytest

import ground_reference as G
import stixel_reference as X
from cli_helpers import CAMERA, cli_refused as _cli_refused
from lwsnet_amd import _lib
from lwsnet_amd.geometry import Camera
from test_gpu_ground import ROAD

F = np.float32
INF = float("inf")
CAM = Camera(120.0, 120.0, 79.5, 47.5, 0.54)
HEIGHT, PITCH = 1.65, 1.3
STIX = dict(min_disp=1.0, max_depth=INF, code_bits=1 << 2, width=4, sub=4, nbins=128, tol_bins=1, min_count=8, min_row=2, max_gap=2, layers=3)

_SCENES = {}


def ref(d, cam, codes, height, p):
    return X.stixels(d, cam, codes, height, p["min_disp"], p["max_depth"], p["code_bits"], p["width"], p["sub"], p["nbins"], p["tol_bins"],
                     p["min_count"], p["min_row"], p["max_gap"], p["layers"])


def box_masks(roll):
    """The pixels each box of G.BOXES covers by itself (nothing in front of it taken away), with road_scene's formulas."""
    fx, fy, cx, cy, _ = (float(v) for v in CAM.row())
    n = G.plane_normal(PITCH, roll)
    y, x = np.mgrid[0:96, 0:160].astype(np.float64)
    rx, ry = (x - cx) / fx, (y - cy) / fy
    out = []
    for x0, x1, zb, hb in G.BOXES:
        hgt = HEIGHT - zb * (n[0] * rx + n[1] * ry + n[2])
        out.append((rx * zb >= x0) & (rx * zb <= x1) & (hgt >= 0) & (hgt <= hb))
    return out


def scene(roll):
    """A 96 x 160 road scene, the restatement of the ground calls with ROAD, and the stixels of the result, computed once."""
    if roll not in _SCENES:
        d, cam, *_ = G.road_scene(height=HEIGHT, pitch_deg=PITCH, roll_deg=roll, cam=CAM.row())
        p = ROAD
        hist = G.vdisparity(d, None, p["min_disp"], p["sub"], p["nbins"])
        plane, info = G.ground_fit(d, None, hist, p["min_disp"], p["sub"], *p["yh"], *p["qb"], p["tol_bins"], p["min_score"], p["tol0"], p["tol"],
                                   p["iters"])
        assert info[0, 0] == G.OK
        height, codes, _ = G.ground_classify(d, None, cam, plane, p["min_disp"], p["max_depth"], p["ground_tol"], p["max_height"])
        rows, vals, udisp = ref(d, cam, codes, height, STIX)
        _SCENES[roll] = dict(d=d, cam=cam, codes=codes, height=height, rows=rows[0], vals=vals[0], udisp=udisp[0], boxes=box_masks(roll))
    return _SCENES[roll]


@pytest.mark.parametrize("roll", [0.0, 1.4])
def test_reference_finds_the_boxes(roll):
    """Every strip wholly inside the columns of the box that is nearest there carries it in layer 0: z within 0.05 m, the top within a
    row of the box's first row, the base at most 6 rows above its last (the rows within ground_tol of the road are ground).  The 11 m
    box shows above the 5 m box in three strips, which carry it in layer 1.  Measured on both scenes: z within 0.001 m, the tops
    equal, the bases 2 to 5 rows short, 12 stixels in layer 0 and 3 in layer 1."""
    s = scene(roll)
    rows, vals, w = s["rows"], s["vals"], STIX["width"]
    near, mid, far = s["boxes"][1], s["boxes"][0], s["boxes"][2]       # 5 m, 7 m, 11 m
    checked = {0: 0, 1: 0}
    for strip in range(rows.shape[0]):
        cols = slice(strip * w, strip * w + w)
        inside = [bool(m[:, cols].any(axis=0).all()) for m in (near, mid, far)]
        touched = [bool(m[:, cols].any()) for m in (near, mid, far)]
        for k, (box, zb) in enumerate(((near, 5.0), (mid, 7.0), (far, 11.0))):
            if not inside[k] or (k == 2 and touched[0]):                # the far box stands behind the near one
                continue
            ys = np.flatnonzero(box[:, cols].any(axis=1))
            n, y_top, y_base, k_peak = rows[strip, 0].tolist()
            print(f"roll {roll} strip {strip} layer 0: {rows[strip, 0].tolist()} z = {vals[strip, 0, 1]:.4f} (box at {zb} m, rows {ys[0]}..{ys[-1]})")
            assert n > 0 and abs(float(vals[strip, 0, 1]) - zb) <= 0.05
            assert abs(y_top - ys[0]) <= 1 and ys[-1] - 6 <= y_base <= ys[-1]
            checked[0] += 1
        if inside[2] and touched[0]:                                    # the far box above the near one: layer 1
            ys, below = np.flatnonzero(far[:, cols].any(axis=1)), np.flatnonzero(near[:, cols].any(axis=1))
            n, y_top, y_base, k_peak = rows[strip, 1].tolist()
            print(f"roll {roll} strip {strip} layer 1: {rows[strip, 1].tolist()} z = {vals[strip, 1, 1]:.4f}")
            assert n > 0 and abs(float(vals[strip, 1, 1]) - 11.0) <= 0.05
            assert abs(y_top - ys[0]) <= 1 and ys[0] <= y_base < below[0]
            assert abs(float(vals[strip, 0, 1]) - 5.0) <= 0.05
            checked[1] += 1
    assert checked == {0: 11, 1: 3}, checked
    found = rows[..., 0] > 0
    print(f"roll {roll}: {found.sum(axis=0).tolist()} stixels per layer")
    assert found[:, 0].sum() >= 11 and found[:, 1].sum() >= 3
    # a slot is empty exactly when it has no rows, and an empty one holds zeros
    empty = ~found
    assert (rows[empty][:, 1:3] == -1).all() and (vals[empty].view(np.uint32) == 0).all() and (rows[found][:, 1] >= 0).all()
    # the heights: a stixel of a box is about as tall as the box
    for strip, hb in ((10, 1.6), (23, 1.2)):
        assert abs(float(vals[strip, 0, 3]) - hb) < 0.1, (strip, vals[strip, 0])
    # u-disparity: the column sums are the obstacle pixels that take part
    take, _ = X.taking(s["d"], s["cam"], s["codes"], 1.0, INF, 1 << 2, 4, 128)
    assert s["udisp"].sum() == take.sum() > 1000


# ---- hand-made columns ----
CAM1 = np.array([[100.0, 100.0, 7.5, 15.5, 50.0]], F)
COL = dict(min_disp=1.0, max_depth=INF, code_bits=1 << 2, width=2, sub=1, nbins=16, tol_bins=1, min_count=4, min_row=2, max_gap=2, layers=2)


def columns(strips, H=32, W=16, **kw):
    """The restatement on a hand-made map of 8 strips of 2 columns: (rows [S,layers,4], vals, udisp, the inputs)."""
    p = {**COL, **kw}
    d, codes, height = X.column_map(H, W, p["width"], strips)
    rows, vals, udisp = ref(d, CAM1, codes, height, p)
    return rows[0], vals[0], udisp[0], (d, codes, height, p)


HAND_MADE = {
    # two pixels each in the bins 11 and 10: only the window around 11 holds min_count, and the peak of the tie is the larger bin
    "tie": (dict(strips={0: [(4, 4, 11.5), (5, 5, 10.5)]}), {0: [[4, 4, 5, 11], [0, -1, -1, -1]]}),
    # windows clipped at bin 0 (a layer at bin 1 reaching below 0) and at nbins - 1
    "clip_low": (dict(strips={1: [(20, 25, 1.5)]}), {1: [[12, 20, 25, 1], [0, -1, -1, -1]]}),
    "clip_high": (dict(strips={2: [(3, 8, 15.5)], 3: [(3, 8, 15.5), (9, 12, 14.5)]}),
                  {2: [[12, 3, 8, 15], [0, -1, -1, -1]], 3: [[20, 3, 12, 15], [0, -1, -1, -1]]}),
    # the windows of layer 1 are clipped at kmax_1 = 12 - 1 - 1 = 10: without bin 11's four pixels bin 10's two are too few
    "clip_kmax": (dict(strips={4: [(0, 5, 12.5), (6, 7, 11.5), (8, 8, 10.5)]}), {4: [[16, 0, 7, 12], [0, -1, -1, -1]]}),
    "below_kmax": (dict(strips={4: [(0, 5, 12.5), (6, 7, 11.5), (8, 13, 10.5)]}), {4: [[16, 0, 7, 12], [12, 8, 13, 10]]}),
    # gaps of exactly max_gap rows are bridged, of max_gap + 1 are not; a gap that runs to row 0
    "gap_equal": (dict(strips={5: [(4, 6, 8.5), (9, 12, 8.5)]}), {5: [[14, 4, 12, 8], [0, -1, -1, -1]]}),
    "gap_more": (dict(strips={5: [(4, 5, 8.5), (9, 12, 8.5)]}), {5: [[8, 9, 12, 8], [0, -1, -1, -1]]}),
    "gap_zero": (dict(strips={5: [(4, 6, 8.5), (8, 12, 8.5)]}, max_gap=0), {5: [[10, 8, 12, 8], [0, -1, -1, -1]]}),
    "gap_zero_solid": (dict(strips={5: [(0, 12, 8.5)]}, max_gap=0), {5: [[26, 0, 12, 8], [0, -1, -1, -1]]}),
    "gap_to_row_0": (dict(strips={6: [(2, 9, 8.5)]}), {6: [[16, 2, 9, 8], [0, -1, -1, -1]]}),
    # min_count not reached: 2 pixels against 3
    "too_few": (dict(strips={7: [(5, 5, 6.5)]}, min_count=3), {7: [[0, -1, -1, -1], [0, -1, -1, -1]]}),
}


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_reference_on_hand_made_columns(name):
    kw, want = HAND_MADE[name]
    rows, vals, udisp, (d, codes, _, p) = columns(**kw)
    for s in range(rows.shape[0]):
        assert rows[s].tolist() == want.get(s, [[0, -1, -1, -1]] * 2), (name, s, rows[s].tolist())
    for s, slots in want.items():
        for layer, (n, y_top, y_base, k) in enumerate(slots):
            if n:
                d_st, z, xs, h = (float(v) for v in vals[s, layer])
                sel = d[0, 0, y_top:y_base + 1, 2 * s:2 * s + 2]
                member = (codes[0, 0, y_top:y_base + 1, 2 * s:2 * s + 2] == 2) & (np.abs(np.floor(sel) - k) <= p["tol_bins"])
                assert member.sum() == n and d_st == float(F(sel[member].astype(np.float64).mean())) and abs(z - 50.0 / d_st) < 1e-4 and abs(xs - (2 * s + 0.5 - 7.5) * z / 100.0) < 1e-4
                assert h == float(F(0.05) * F(32 - y_top))              # the tallest member is the top row's
            else:
                assert (vals[s, layer].view(np.uint32) == 0).all()


def hole_map():
    """Strip 3: bin 12 has 8 pixels but one per row (a diagonal); bin 6 has six full rows."""
    d, codes, height = X.column_map(32, 16, 2, {3: [(14, 19, 6.5)]})
    for y in range(8):
        d[0, 0, y, 6 + (y & 1)], codes[0, 0, y, 6 + (y & 1)] = 12.5, 2
    return d, codes, height


def test_reference_hole_then_a_real_layer():
    """No row of the diagonal is flagged with min_row 2: a hole that keeps its k_peak; the layer below it is real."""
    d, codes, height = hole_map()
    rows, vals, _ = ref(d, CAM1, codes, height, COL)
    assert rows[0, 3].tolist() == [[0, -1, -1, 12], [12, 14, 19, 6]]
    assert (vals[0, 3, 0].view(np.uint32) == 0).all() and vals[0, 3, 1, 0] == 6.5
    rows, _, _ = ref(d, CAM1, codes, height, {**COL, "min_row": 1})    # with min_row 1 the diagonal stands
    assert rows[0, 3].tolist() == [[8, 0, 7, 12], [12, 14, 19, 6]]


def test_reference_ignores_other_codes_and_invalid_pixels():
    d, codes, height = X.column_map(32, 16, 2, {0: [(4, 9, 9.5)], 1: [(4, 9, 9.5)], 2: [(4, 9, 9.5)], 3: [(4, 9, 0.5)], 4: [(4, 9, 16.0)]})
    codes[0, 0, :, 0:2] = 3                                 # overhead: not in code_bits
    codes[0, 0, :, 2:4] = 6                                 # no code
    d[0, 0, 4:10, 4:6] = np.nan
    rows, _, udisp = ref(d, CAM1, codes, height, COL)
    assert (rows[0, :, :, 0] == 0).all() and udisp.sum() == 0           # 0.5 < min_disp; 16.0 is past the last bin
    rows, _, udisp = ref(d, CAM1, codes, height, {**COL, "code_bits": (1 << 2) | (1 << 3)})
    assert rows[0, 0, 0].tolist() == [12, 4, 9, 9] and udisp.sum() == 12


# ---- C ABI argument checks (no GPU call is reached) ----
def _p(k, off=0):
    """Fake device pointers 1 GiB apart: never dereferenced, every call below is refused first."""
    return ctypes.c_void_p((1 << 40) + (k << 30) + off)


def test_stixels_rejects_bad_arguments(hip_lib):
    names = ("disp", "cam", "codes", "height", "rows", "vals", "udisp")
    base = {name: _p(k) for k, name in enumerate(names)}

    def call(B=1, H=8, W=16, min_disp=1.0, max_depth=INF, code_bits=4, width=4, sub=4, nbins=64, tol_bins=1, min_count=8, min_row=2, max_gap=2,
             layers=2, **ptrs):
        a = {**base, **ptrs}
        return hip_lib.lws_stixels(a["disp"], a["cam"], a["codes"], a["height"], B, H, W, min_disp, max_depth, code_bits, width, sub, nbins,
                                   tol_bins, min_count, min_row, max_gap, layers, a["rows"], a["vals"], a["udisp"], None)

    def at(name, off):
        return _p(names.index(name), off)

    null_in, null_out = b"stixels: cam, codes and height must not be null", b"stixels: rows and vals must not be null"
    al = b"stixels: cam / height / rows / vals / udisp must be 4-byte aligned"
    pos = b"stixels: code_bits %d selects a code other than 2 and 3, whose heights are not positive"
    for kw, msg in [
        (dict(disp=None), b"stixels: disp is null"), (dict(cam=None), null_in), (dict(codes=None), null_in), (dict(height=None), null_in),
        (dict(rows=None), null_out), (dict(vals=None), null_out),
        (dict(disp=at("disp", 2)), b"stixels: disp is not 4-byte aligned"), (dict(cam=at("cam", 2)), al), (dict(height=at("height", 1)), al),
        (dict(rows=at("rows", 2)), al), (dict(vals=at("vals", 3)), al), (dict(udisp=at("udisp", 2)), al),
        (dict(B=0), b"stixels: bad shape B=0 H=8 W=16"), (dict(W=0), b"stixels: bad shape B=1 H=8 W=0"),
        (dict(H=16385), b"stixels: H=16385 W=16 exceed 16384 (a row's byte in LDS, the 64-bit sums)"),
        (dict(W=16385), b"stixels: H=8 W=16385 exceed 16384 (a row's byte in LDS, the 64-bit sums)"),
        (dict(min_disp=0.0), b"stixels: min_disp must be finite and > 0, got 0"),
        (dict(max_depth=float("nan")), b"stixels: max_depth must be > 0 (+inf allowed), got nan"),
        (dict(code_bits=-1), b"stixels: code_bits -1 outside 0..63"), (dict(code_bits=64), b"stixels: code_bits 64 outside 0..63"),
        (dict(code_bits=5), pos % 5), (dict(code_bits=6), pos % 6), (dict(code_bits=16), pos % 16), (dict(code_bits=32), pos % 32),
        (dict(width=0), b"stixels: width 0 outside 1..64"), (dict(width=65), b"stixels: width 65 outside 1..64"),
        (dict(sub=0), b"stixels: sub 0 outside 1..16"), (dict(sub=17), b"stixels: sub 17 outside 1..16"),
        (dict(nbins=0), b"stixels: nbins 0 outside 1..min(4096, 256 * sub = 1024)"),
        (dict(nbins=1025), b"stixels: nbins 1025 outside 1..min(4096, 256 * sub = 1024)"),
        (dict(sub=16, nbins=4097), b"stixels: nbins 4097 outside 1..min(4096, 256 * sub = 4096)"),
        (dict(tol_bins=-1), b"stixels: tol_bins -1 outside 0..8"), (dict(tol_bins=9), b"stixels: tol_bins 9 outside 0..8"),
        (dict(min_count=0), b"stixels: min_count 0 < 1"), (dict(min_row=0), b"stixels: min_row 0 < 1"), (dict(max_gap=-1), b"stixels: max_gap -1 < 0"),
        (dict(layers=0), b"stixels: layers 0 outside 1..4"), (dict(layers=5), b"stixels: layers 5 outside 1..4"),
        (dict(vals=at("rows", 16 * 4 * 2 - 4)), b"stixels: vals and rows overlap"), (dict(udisp=at("vals", 0)), b"stixels: udisp and vals overlap"),
        (dict(disp=at("udisp", 4 * 4 * 64 - 4)), b"stixels: disp and udisp overlap"), (dict(cam=at("rows", 0)), b"stixels: cam and rows overlap"),
        (dict(codes=at("vals", 64)), b"stixels: codes and vals overlap"), (dict(height=at("rows", 124)), b"stixels: height and rows overlap"),
    ]:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert hip_lib.lws_last_error() == msg, (kw, hip_lib.lws_last_error())
    # no histogram asked for: the next refusal is not about udisp
    assert call(udisp=None, layers=0) == _lib.LWS_ERR_INVALID and hip_lib.lws_last_error() == b"stixels: layers 0 outside 1..4"


def test_prototype_matches_the_library(hip_lib):
    assert hip_lib.lws_stixels.argtypes == _lib.PROTOTYPES["lws_stixels"][1] and len(_lib.PROTOTYPES["lws_stixels"][1]) == 22
    assert hip_lib.lws_abi_version() == 8


def test_ops_validate_before_any_gpu_call():
    from lwsnet_amd import ops
    z = np.zeros((1, 1, 2, 2), F)
    with pytest.raises(ValueError, match="stixels needs cameras"):
        ops.stixels(z, None, None, None)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.stixels(z, CAM, None, None)
    for kw, msg in ((dict(min_disp=0.0), "min_disp"), (dict(code_bits=64), "code_bits"), (dict(code_bits=6), "not positive"),
                    (dict(width=0), "width must be an integer in 1 .. 64"), (dict(width=65), "width"), (dict(width=2.5), "width"),
                    (dict(sub=17), "sub"), (dict(nbins=0), "nbins"), (dict(nbins=1025), "nbins must be an integer in 1 .. 1024"),
                    (dict(maxdisp=0), "maxdisp"), (dict(tol_bins=9), "tol_bins"), (dict(min_count=0), "min_count"), (dict(min_row=0), "min_row"),
                    (dict(max_gap=-1), "max_gap"), (dict(layers=0), "layers"), (dict(layers=5), "layers must be an integer in 1 .. 4")):
        with pytest.raises(ValueError, match=msg):
            ops.stixels(None, CAM, None, None, **kw)
    assert ops._stixel_args(1.0, 4, 8, 192, 4, None, 1, None, None, 2, 2) == (1.0, 4, 8, 4, 768, 1, 16, 4, 2, 2)
    assert ops._stixel_args(1.0, 12, 1, 192, 4, None, 0, None, None, 0, 1)[6:8] == (2, 1)
    assert ops.StixelResult._fields == ("rows", "vals", "udisp")
    assert ops.GroundResult._fields == ("hist", "plane", "info", "height", "codes", "counts", "bev_count", "bev_hmax")


# ---- the inference CLI ----
NEW_FLAGS = ("stixels", "save_stixels", "stixel_width", "stixel_layers")


def test_stixel_flags_default_off():
    from lwsnet_amd import inference
    p = inference.build_parser()
    a = p.parse_args([])
    assert not any(hasattr(a, name) for name in NEW_FLAGS)                      # the namespace of a line without them
    with_flags = vars(p.parse_args(["--stixels", "--save_stixels", "--stixel_width", "4", "--stixel_layers", "3"]))
    assert {k: v for k, v in with_flags.items() if k not in NEW_FLAGS} == vars(a)
    inference.check_geometry_arguments(p, a)
    assert (a.stixels, a.save_stixels, a.stixel_width, a.stixel_layers, a.ground) == (False, False, 8, 2, False)
    assert not inference._geometry_requested(a)
    a = p.parse_args(["--save_stixels", "--stixel_width", "4", "--stixel_layers", "3"] + CAMERA)
    inference.check_geometry_arguments(p, a)
    assert (a.stixels, a.save_stixels, a.stixel_width, a.stixel_layers) == (True, True, 4, 3)
    assert a.ground and not a.save_ground and inference._geometry_requested(a)  # --stixels implies --ground


@pytest.mark.parametrize("flag", ["--stixels", "--save_stixels"])
def test_cli_refuses_stixels_without_camera_or_with_workers(flag, capsys):
    assert "--stixels and --save_stixels need a camera" in _cli_refused([flag], capsys)
    assert "sequential mode only" in _cli_refused([flag, "--workers", "2"] + CAMERA, capsys)


@pytest.mark.parametrize("extra,text", [(["--stixel_width", "0"], "--stixel_width must be in 1 .. 64"),
                                        (["--stixel_width", "65"], "--stixel_width must be in 1 .. 64"),
                                        (["--stixel_layers", "0"], "--stixel_layers must be in 1 .. 4"),
                                        (["--stixel_layers", "5"], "--stixel_layers must be in 1 .. 4")])
def test_cli_refuses_bad_stixel_sizes(extra, text, capsys):
    assert text in _cli_refused(["--stixels"] + extra + CAMERA, capsys)


def test_stixel_file_helpers():
    from lwsnet_amd import inference
    rows = np.array([[[6, 1, 3, 9], [0, -1, -1, 4]], [[0, -1, -1, -1], [0, -1, -1, -1]], [[2, 0, 1, 7], [3, 2, 3, 2]]], np.int32)
    vals = np.zeros((3, 2, 4), F)
    vals[0, 0] = (9.5, 7.5, -1.25, 1.5)
    vals[2, 0] = (7.25, 15.0, 0.5, 2.0)
    vals[2, 1] = (2.5, 60.0, 0.75, 0.25)
    text = inference.stixels_to_csv(rows, vals, 2, 5)
    assert text == ("strip,layer,x0,x1,y_top,y_base,n,disparity,z,x,height\n"
                    "0,0,0,1,1,3,6,9.500000,7.500000,-1.250000,1.500000\n"
                    "2,0,4,4,0,1,2,7.250000,15.000000,0.500000,2.000000\n"
                    "2,1,4,4,2,3,3,2.500000,60.000000,0.750000,0.250000\n")     # the last strip is clipped at W
    left = np.full((4, 5, 3), 100, np.uint8)
    rgb = inference.stixels_to_rgb(rows, vals, left, 2, 60.0)
    assert rgb.dtype == np.uint8 and rgb.shape == (4, 5, 3)
    assert rgb[0, 0].tolist() == [100, 100, 100] and rgb[0, 2].tolist() == [100, 100, 100]     # outside every stixel: the grey
    assert rgb[1, 0].tolist() == rgb[3, 1].tolist() == [(223 + 100 + 1) >> 1, (64 + 100 + 1) >> 1, (32 + 100 + 1) >> 1]   # z = 7.5 of 60: t = 0.125
    assert rgb[0, 4].tolist() == [(191 + 100 + 1) >> 1, (128 + 100 + 1) >> 1, (64 + 100 + 1) >> 1]                       # t = 0.25
    assert rgb[3, 4].tolist() == [50, 50, 178]                                  # t = 1: blue


@pytest.mark.parametrize("flag", ["--stixels", "--save_stixels"])
def test_cli_stixel_error_texts(flag, capsys):
    camera = ": error: --stixels and --save_stixels need a camera: --calib PATH or --camera FX FY CX CY BASELINE\n"
    assert _cli_refused([flag], capsys).endswith(camera)
    assert _cli_refused([flag, "--workers", "2"], capsys).endswith(camera), "the camera comes before the mode, the stixels' before the ground's"
    assert _cli_refused([flag, "--workers", "2"] + CAMERA, capsys).endswith(
        ": error: --stixels / --save_stixels run in the sequential mode only: use --workers 0\n")
    assert _cli_refused([flag, "--stixel_width", "65"], capsys).endswith(": error: --stixel_width must be in 1 .. 64, got 65\n"), "sizes before the camera"
    assert _cli_refused([flag, "--stixel_layers", "5"] + CAMERA, capsys).endswith(": error: --stixel_layers must be in 1 .. 4, got 5\n")
