"""The ground pipeline without a GPU: the numpy restatement (tests/ground_reference.py) recovers planted roads and labels what
stands on them, GroundPlane gives back the planted pose, and every argument error of the four entry points, of the ops wrappers
and of the inference CLI's flags is raised before any GPU work."""
import ctypes

import numpy as np
import pytest

import ground_reference as G
from cli_helpers import CAMERA, cli_refused as _cli_refused
from lwsnet_amd import _lib
from lwsnet_amd.geometry import Camera, GroundPlane

F = np.float32
INF = float("inf")
CAM = Camera(120.0, 120.0, 79.5, 47.5, 0.54)
HEIGHT, PITCH = 1.65, 1.0
SUB, NBINS, TOL, GROUND_TOL, MAX_HEIGHT = 4, 128, 1.0, 0.2, 3.0

_SCENES = {}


def fitted(roll):
    """A 96 x 160 road scene and the restatement's results on it, computed once."""
    if roll not in _SCENES:
        d, cam, planted, road, box, above = G.road_scene(height=HEIGHT, pitch_deg=PITCH, roll_deg=roll, cam=CAM.row())
        H = d.shape[2]
        hist = G.vdisparity(d, None, 1.0, SUB, NBINS)
        planes64 = []
        plane, info = G.ground_fit(d, None, hist, 1.0, SUB, H // 4, 3 * H // 4, NBINS // 3, NBINS - 1, 1, 1, 1.0, TOL, 3, planes64)
        height, codes, counts = G.ground_classify(d, None, cam, plane, 1.0, INF, GROUND_TOL, MAX_HEIGHT)
        _SCENES[roll] = dict(d=d, cam=cam, planted=planted, road=road, box=box, above=above, hist=hist, plane=plane, info=info,
                             plane64=planes64[0], height=height, codes=codes, counts=counts)
    return _SCENES[roll]


@pytest.mark.parametrize("roll", [0.0, 2.0])
def test_reference_recovers_the_planted_plane(roll):
    """Status ok, and over the rows below the horizon the fitted plane lies within the inlier tolerance of the planted one (the
    condition); measured: 0.019 px without roll, 0.018 px at 2 degrees."""
    s = fitted(roll)
    assert s["info"][0, 0] == G.OK and s["info"][0, 4] > 5000
    a, b, c = s["plane64"]
    pa, pb, pc = s["planted"]
    y, x = np.mgrid[0:96, 0:160]
    below = (pa * x + pb * y + pc) > 0
    err = float(np.abs((a - pa) * x + (b - pb) * y + (c - pc))[below].max())
    print(f"roll {roll}: the fitted plane is within {err:.4f} px of the planted one; info = {s['info'][0, :5].tolist()}")
    assert err <= TOL
    assert np.array_equal(s["plane"][0, :3], np.array([a, b, c]).astype(F)) and s["plane"][0, 3] == 0


@pytest.mark.parametrize("roll", [0.0, 2.0])
def test_reference_labels_boxes_and_road(roll):
    """Box pixels are obstacles and road pixels ground.  A box stands on the road, so its lowest GROUND_TOL metres are ground by the
    definition of the codes: the box pixels held to code 2 are those planted more than 5 cm (a quarter of GROUND_TOL, for the fit's
    error) above that.  The valid road pixels not labelled ground: measured 0 of 6121 on both scenes, which is the cap -- with the
    plane within 0.02 px, a road point is off by 0.2 m only beyond 390 m, far below min_disp."""
    s = fitted(roll)
    codes = s["codes"][0, 0]
    box = s["box"] & (s["above"] > GROUND_TOL + 0.05)
    assert box.sum() > 1300 and (codes[box] == G.OBSTACLE).all()
    road = s["road"] & (s["d"][0, 0] >= 1.0)
    wrong = int((codes[road] != G.GROUND).sum())
    print(f"roll {roll}: {wrong} of {int(road.sum())} valid road pixels are not labelled ground")
    assert road.sum() > 6000 and wrong == 0
    assert (codes[s["d"][0, 0] < 1.0] == G.INVALID).all()
    assert s["counts"][0].tolist() == np.bincount(codes.reshape(-1), minlength=6).tolist()
    # the heights of the box pixels are the planted ones within 5 cm
    assert np.abs(s["height"][0, 0][s["box"]] - s["above"][s["box"]]).max() < 0.05


def test_reference_bev_grid_holds_the_boxes():
    s = fitted(0.0)
    count, hmax = G.bev_grid(s["d"], s["cam"], s["codes"], s["height"], 1.0, INF, 1 << 2, -8.0, 0.2, 80, 100)
    assert count.sum() == s["counts"][0, G.OBSTACLE]
    for x0, x1, z, hb in G.BOXES:                           # each box: cells in its depth row, the top near its height
        iz = int(z / 0.2)
        cells = slice(int((x0 + 8.0) / 0.2) + 1, int((x1 + 8.0) / 0.2))
        assert (count[0, iz - 1:iz + 1, cells].sum(axis=0) > 0).all(), (x0, x1, z)
        top = hmax[0, iz - 1:iz + 1, cells].max()
        assert hb - 0.15 < top <= hb + 0.05, (hb, top)
    assert (hmax[count == 0] == 0).all() and (hmax[count > 0] > GROUND_TOL).all()
    nothing, _ = G.bev_grid(s["d"], s["cam"], s["codes"], s["height"], 1.0, INF, 1 << 3, -8.0, 0.2, 80, 100)
    assert nothing.sum() == 0                               # no overhead pixels in the scene


def test_reference_hough_tie_rule_and_clipping():
    hist = np.zeros((6, 8), np.uint32)
    hist[5, 3] = hist[5, 5] = 7                             # two bottom bins with equal support
    assert G.hough(hist, 0, 3, 1, 7, 0) == (0, 3, 7)        # the smaller qB, then the smaller yh
    assert G.hough(hist, 2, 3, 4, 7, 0) == (2, 5, 7)
    assert G.hough(hist, -4, -4, 1, 7, 1)[2] == 14          # tol_bins 1 around qB = 4 reaches both
    hist[:] = 0
    hist[:, 0] = hist[:, 7] = 1                             # windows clipped at bin 0 and at nbins - 1
    assert G.hough_scores(hist, 0, 0, 7, 7, 8)[0, 0] == 10


@pytest.mark.parametrize("roll", [0.0, 2.0])
def test_ground_plane_gives_back_the_planted_pose(roll):
    gp = GroundPlane.from_plane(G.planted_plane(CAM.row(), HEIGHT, PITCH, roll), CAM)
    assert abs(gp.height - HEIGHT) < 1e-6 and abs(gp.pitch_deg - PITCH) < 1e-6 and abs(gp.roll_deg - roll) < 1e-6
    assert np.allclose(gp.normal, G.plane_normal(PITCH, roll), atol=1e-9)
    got = GroundPlane.from_plane(fitted(roll)["plane"][0], CAM)                 # the fitted plane: within 1 cm and 0.05 degrees
    assert abs(got.height - HEIGHT) < 0.01 and abs(got.pitch_deg - PITCH) < 0.05 and abs(got.roll_deg - roll) < 0.05
    assert GroundPlane.from_plane([np.nan, np.nan, np.nan, np.nan], CAM) is None
    assert GroundPlane.from_plane([0.0, 0.0, 0.0, 0.0], CAM) is None


# ---- C ABI argument checks (no GPU call is reached) ----
def _p(k, off=0):
    """Fake device pointers 1 GiB apart: never dereferenced, every call below is refused first."""
    return ctypes.c_void_p((1 << 40) + (k << 30) + off)


def _refused(call, texts, lib):
    for kw, msg in texts:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert lib.lws_last_error() == msg, (kw, lib.lws_last_error())


def test_vdisparity_rejects_bad_arguments(hip_lib):
    def call(disp=_p(0), mask=_p(1), B=1, H=8, W=16, min_disp=1.0, sub=4, nbins=64, hist=_p(2)):
        return hip_lib.lws_vdisparity(disp, mask, B, H, W, min_disp, sub, nbins, hist, None)

    _refused(call, [
        (dict(disp=None), b"vdisparity: disp is null"), (dict(hist=None), b"vdisparity: hist is null"),
        (dict(disp=_p(0, 2)), b"vdisparity: disp is not 4-byte aligned"), (dict(hist=_p(2, 1)), b"vdisparity: hist is not 4-byte aligned"),
        (dict(B=0), b"vdisparity: bad shape B=0 H=8 W=16"), (dict(W=0), b"vdisparity: bad shape B=1 H=8 W=0"),
        (dict(H=1 << 16, W=1 << 15), b"vdisparity: H*W = 65536x32768 must be < 2^31"),
        (dict(min_disp=0.0), b"vdisparity: min_disp must be finite and > 0, got 0"),
        (dict(min_disp=INF), b"vdisparity: min_disp must be finite and > 0, got inf"),
        (dict(min_disp=float("nan")), b"vdisparity: min_disp must be finite and > 0, got nan"),
        (dict(sub=0), b"vdisparity: sub 0 outside 1..16"), (dict(sub=17), b"vdisparity: sub 17 outside 1..16"),
        (dict(nbins=0), b"vdisparity: nbins 0 outside 1..min(4096, 256 * sub = 1024)"),
        (dict(nbins=1025), b"vdisparity: nbins 1025 outside 1..min(4096, 256 * sub = 1024)"),
        (dict(sub=16, nbins=4097), b"vdisparity: nbins 4097 outside 1..min(4096, 256 * sub = 4096)"),
        (dict(disp=_p(2, 4 * 8 * 64 - 4)), b"vdisparity: disp and hist overlap"), (dict(mask=_p(2)), b"vdisparity: mask and hist overlap"),
    ], hip_lib)


def test_ground_fit_rejects_bad_arguments(hip_lib):
    names = ("disp", "mask", "hist", "work", "plane", "info")
    base = {name: _p(k) for k, name in enumerate(names)}

    def call(B=1, H=8, W=16, min_disp=1.0, sub=4, nbins=64, yh=(2, 6), qb=(1, 63), tol_bins=1, min_score=0, tol0=1.0, tol=1.0, iters=3, **ptrs):
        a = {**base, **ptrs}
        return hip_lib.lws_ground_fit(a["disp"], a["mask"], a["hist"], B, H, W, min_disp, sub, nbins, yh[0], yh[1], qb[0], qb[1], tol_bins,
                                      min_score, tol0, tol, iters, a["work"], a["plane"], a["info"], None)

    def at(name, off):
        return _p(names.index(name), off)

    null = b"ground_fit: hist, workspace, plane and info must not be null"
    al = b"ground_fit: hist / plane / info must be 4-byte, workspace 8-byte aligned"
    _refused(call, [
        (dict(disp=None), b"ground_fit: disp is null"), (dict(hist=None), null), (dict(work=None), null), (dict(plane=None), null),
        (dict(info=None), null), (dict(hist=at("hist", 2)), al), (dict(plane=at("plane", 1)), al), (dict(info=at("info", 2)), al),
        (dict(work=at("work", 4)), al), (dict(sub=0), b"ground_fit: sub 0 outside 1..16"),
        (dict(nbins=2000), b"ground_fit: nbins 2000 outside 1..min(4096, 256 * sub = 1024)"),
        (dict(H=16385, yh=(0, 0)), b"ground_fit: H=16385 W=16 exceed 16384 (the 64-bit sums)"),
        (dict(W=16385), b"ground_fit: H=8 W=16385 exceed 16384 (the 64-bit sums)"),
        (dict(yh=(2, 7)), b"ground_fit: yh range 2..7 outside -65536..H - 2 = 6"),
        (dict(yh=(5, 4)), b"ground_fit: yh range 5..4 outside -65536..H - 2 = 6"),
        (dict(yh=(-65537, 4)), b"ground_fit: yh range -65537..4 outside -65536..H - 2 = 6"),
        (dict(qb=(0, 63)), b"ground_fit: qB range 0..63 outside 1..nbins - 1 = 63"),
        (dict(qb=(1, 64)), b"ground_fit: qB range 1..64 outside 1..nbins - 1 = 63"),
        (dict(qb=(9, 8)), b"ground_fit: qB range 9..8 outside 1..nbins - 1 = 63"),
        (dict(sub=16, nbins=4096, yh=(-2000, 6), qb=(1, 4095)), b"ground_fit: 2007 x 4095 candidates exceed 4194304"),
        (dict(tol_bins=-1), b"ground_fit: tol_bins -1 outside 0..8"), (dict(tol_bins=9), b"ground_fit: tol_bins 9 outside 0..8"),
        (dict(min_score=-1), b"ground_fit: min_score -1 < 0"),
        (dict(tol0=-1.0), b"ground_fit: tol0 and tol must be finite and >= 0, got -1 and 1"),
        (dict(tol=float("nan")), b"ground_fit: tol0 and tol must be finite and >= 0, got 1 and nan"),
        (dict(iters=-1), b"ground_fit: iters -1 outside 0..8"), (dict(iters=9), b"ground_fit: iters 9 outside 0..8"),
        (dict(plane=at("work", 128)), b"ground_fit: plane and workspace overlap"),
        (dict(info=at("plane", 12)), b"ground_fit: info and plane overlap"),
        (dict(disp=at("info", 28)), b"ground_fit: disp and info overlap"),
        (dict(mask=at("plane", 0)), b"ground_fit: mask and plane overlap"),
        (dict(hist=at("work", 252)), b"ground_fit: hist and workspace overlap"),
    ], hip_lib)


def test_ground_workspace_size(hip_lib):
    assert hip_lib.lws_ground_workspace(1, 368, 768) == 256
    assert hip_lib.lws_ground_workspace(2, 368, 768) == 256
    assert hip_lib.lws_ground_workspace(3, 1, 1) == 512
    assert hip_lib.lws_ground_workspace(0, 368, 768) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_last_error() == b"ground_workspace: bad shape B=0 H=368 nbins=768"
    assert hip_lib.lws_ground_workspace(1, 368, 4097) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_ground_workspace(65536, 1, 1) == _lib.LWS_ERR_INVALID


def test_ground_classify_rejects_bad_arguments(hip_lib):
    names = ("disp", "mask", "cam", "plane", "height", "codes", "counts")
    base = {name: _p(k) for k, name in enumerate(names)}

    def call(B=1, H=8, W=16, min_disp=1.0, max_depth=INF, ground_tol=0.2, max_height=3.0, **ptrs):
        a = {**base, **ptrs}
        return hip_lib.lws_ground_classify(a["disp"], a["mask"], a["cam"], a["plane"], B, H, W, min_disp, max_depth, ground_tol, max_height,
                                           a["height"], a["codes"], a["counts"], None)

    def at(name, off):
        return _p(names.index(name), off)

    al = b"ground_classify: cam / plane / height must be 4-byte, counts 8-byte aligned"
    _refused(call, [
        (dict(disp=None), b"ground_classify: disp is null"), (dict(cam=None), b"ground_classify: cam and plane must not be null"),
        (dict(plane=None), b"ground_classify: cam and plane must not be null"),
        (dict(height=None, codes=None), b"ground_classify: no output requested (height and codes are both null)"),
        (dict(cam=at("cam", 2)), al), (dict(plane=at("plane", 1)), al), (dict(height=at("height", 2)), al), (dict(counts=at("counts", 4)), al),
        (dict(B=65536), b"ground_classify: bad shape B=65536 H=8 W=16"),
        (dict(min_disp=-1.0), b"ground_classify: min_disp must be finite and > 0, got -1"),
        (dict(max_depth=0.0), b"ground_classify: max_depth must be > 0 (+inf allowed), got 0"),
        (dict(ground_tol=-0.1), b"ground_classify: need finite 0 <= ground_tol <= max_height, got -0.1 and 3"),
        (dict(ground_tol=4.0), b"ground_classify: need finite 0 <= ground_tol <= max_height, got 4 and 3"),
        (dict(max_height=INF), b"ground_classify: need finite 0 <= ground_tol <= max_height, got 0.2 and inf"),
        (dict(ground_tol=float("nan")), b"ground_classify: need finite 0 <= ground_tol <= max_height, got nan and 3"),
        (dict(codes=at("height", 4 * 128 - 1)), b"ground_classify: codes and height overlap"),
        (dict(counts=at("codes", 120)), b"ground_classify: counts and codes overlap"),
        (dict(disp=at("counts", 40)), b"ground_classify: disp and counts overlap"),
        (dict(mask=at("height", 0)), b"ground_classify: mask and height overlap"),
        (dict(cam=at("codes", 0)), b"ground_classify: cam and codes overlap"),
        (dict(plane=at("height", 0)), b"ground_classify: plane and height overlap"),
    ], hip_lib)


def test_bev_grid_rejects_bad_arguments(hip_lib):
    names = ("disp", "cam", "codes", "height", "count", "hmax")
    base = {name: _p(k) for k, name in enumerate(names)}

    def call(B=1, H=8, W=16, min_disp=1.0, max_depth=INF, code_bits=4, x_min=-2.0, cell=0.5, Gx=8, Gz=4, **ptrs):
        a = {**base, **ptrs}
        return hip_lib.lws_bev_grid(a["disp"], a["cam"], a["codes"], a["height"], B, H, W, min_disp, max_depth, code_bits, x_min, cell, Gx, Gz,
                                    a["count"], a["hmax"], None)

    def at(name, off):
        return _p(names.index(name), off)

    al = b"bev_grid: cam / height / count / hmax must be 4-byte aligned"
    pos = b"bev_grid: code_bits %d selects a code other than 2 and 3, whose heights are not positive; hmax cannot be requested"
    _refused(call, [
        (dict(disp=None), b"bev_grid: disp is null"), (dict(cam=None), b"bev_grid: cam and codes must not be null"),
        (dict(codes=None), b"bev_grid: cam and codes must not be null"),
        (dict(count=None, hmax=None), b"bev_grid: no output requested (count and hmax are both null)"),
        (dict(height=None), b"bev_grid: hmax needs height"),
        (dict(cam=at("cam", 2)), al), (dict(height=at("height", 1)), al), (dict(count=at("count", 2)), al), (dict(hmax=at("hmax", 2)), al),
        (dict(code_bits=-1), b"bev_grid: code_bits -1 outside 0..63"), (dict(code_bits=64), b"bev_grid: code_bits 64 outside 0..63"),
        (dict(code_bits=5), pos % 5), (dict(code_bits=6), pos % 6), (dict(code_bits=16), pos % 16), (dict(code_bits=32), pos % 32),
        (dict(x_min=INF), b"bev_grid: x_min must be finite, got inf"), (dict(x_min=float("nan")), b"bev_grid: x_min must be finite, got nan"),
        (dict(cell=0.0), b"bev_grid: cell must be finite and > 0, got 0"), (dict(cell=INF), b"bev_grid: cell must be finite and > 0, got inf"),
        (dict(Gx=0), b"bev_grid: grid Gx=0 Gz=4 outside 1..4096"), (dict(Gz=4097), b"bev_grid: grid Gx=8 Gz=4097 outside 1..4096"),
        (dict(hmax=at("count", 4 * 31)), b"bev_grid: hmax and count overlap"), (dict(disp=at("hmax", 0)), b"bev_grid: disp and hmax overlap"),
        (dict(codes=at("count", 0)), b"bev_grid: codes and count overlap"), (dict(height=at("hmax", 64)), b"bev_grid: height and hmax overlap"),
        (dict(cam=at("count", 0)), b"bev_grid: cam and count overlap"),
    ], hip_lib)
    # any code may be counted when no maximum is asked for; the refusal that follows is the grid's, which is checked later
    assert call(code_bits=63, hmax=None, height=None, Gx=0) == _lib.LWS_ERR_INVALID and b"grid Gx=0" in hip_lib.lws_last_error()


def test_prototypes_match_the_library(hip_lib):
    for name in ("lws_vdisparity", "lws_ground_workspace", "lws_ground_fit", "lws_ground_classify", "lws_bev_grid"):
        assert getattr(hip_lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert _lib.PROTOTYPES["lws_ground_workspace"][0] is ctypes.c_int64


# ---- the ops wrappers refuse before any GPU work ----
def test_ops_validate_before_any_gpu_call():
    import torch

    from lwsnet_amd import ops
    z = np.zeros((1, 1, 2, 2), F)
    for fn, args in ((ops.ground, (z, None)), (ops.ground_classify, (z, None, None)), (ops.bev_grid, (z, None, None))):
        with pytest.raises(ValueError, match="needs cameras"):
            fn(*args)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.ground(z, CAM)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.vdisparity(z)
    for kw, msg in ((dict(min_disp=0.0), "min_disp"), (dict(sub=0), "sub must be an integer in 1 .. 16"), (dict(sub=2.5), "sub"),
                    (dict(nbins=0), "nbins"), (dict(nbins=1025), "nbins must be an integer in 1 .. 1024"), (dict(sub=16, nbins=4097), "4096"),
                    (dict(maxdisp=0), "maxdisp")):
        with pytest.raises(ValueError, match=msg):
            ops.vdisparity(None, **kw)
    hist = torch.zeros((1, 8, 64), dtype=torch.uint32)
    with pytest.raises(ValueError, match="hist must be the uint32"):
        ops.ground_fit(None, torch.zeros((1, 8, 64)))
    for kw, msg in ((dict(yh_range=(2, 7)), "yh_range"), (dict(yh_range=(5, 4)), "lo <= hi"), (dict(qb_range=(0, 3)), "qb_range"),
                    (dict(qb_range=(1, 64)), "qb_range"), (dict(tol_bins=9), "tol_bins"), (dict(iters=-1), "iters"), (dict(min_score=-1), "min_score"),
                    (dict(tol0=-1.0), "tol0"), (dict(tol=INF), "tol must be finite"), (dict(sub=17), "sub")):
        with pytest.raises(ValueError, match=msg):
            ops.ground_fit(None, hist, **kw)
    with pytest.raises(ValueError, match="2\\^22 candidates"):
        ops.ground_fit(None, torch.zeros((1, 8, 4096), dtype=torch.uint32), sub=16, yh_range=(-2000, 6), qb_range=(1, 4095))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.ground_fit(z, hist)
    for kw, msg in ((dict(ground_tol=-1.0), "ground_tol"), (dict(max_height=INF), "max_height"), (dict(ground_tol=4.0), "<= max_height"),
                    (dict(height=False, codes=False), "at least one")):
        with pytest.raises(ValueError, match=msg):
            ops.ground_classify(None, CAM, None, **kw)
    for kw, msg in ((dict(code_bits=64), "code_bits"), (dict(code_bits=6), "not positive"), (dict(x_min=INF), "x_min"), (dict(cell=0.0), "cell"),
                    (dict(grid=(0, 4)), "grid"), (dict(grid=(4, 4097)), "grid"), (dict(grid=(4,)), "grid"), (dict(count=False, hmax=False), "at least one"),
                    (dict(height=None), "hmax needs height")):
        with pytest.raises(ValueError, match=msg):
            ops.bev_grid(None, CAM, None, **{"height": z, **kw})
    for kw, msg in ((dict(ground_tol=5.0), "<= max_height"), (dict(code_bits=1), "not positive"), (dict(sub=0), "sub"), (dict(cell=-1.0), "cell")):
        with pytest.raises(ValueError, match=msg):
            ops.ground(None, CAM, **kw)
    assert ops.GroundResult._fields == ("hist", "plane", "info", "height", "codes", "counts", "bev_count", "bev_hmax")
    assert len(ops.GROUND_CODES) == 6 and len(ops.GROUND_STATUS) == 3


# ---- the inference CLI ----
NEW_FLAGS = ("ground", "save_ground", "ground_tol", "max_height")


def test_ground_flags_default_off():
    from lwsnet_amd import inference
    p = inference.build_parser()
    a = p.parse_args([])
    assert not any(hasattr(a, name) for name in NEW_FLAGS)                      # the namespace of a line without them
    with_flags = vars(p.parse_args(["--ground", "--save_ground", "--ground_tol", "0.3", "--max_height", "2.5"]))
    assert {k: v for k, v in with_flags.items() if k not in NEW_FLAGS} == vars(a)
    inference.check_geometry_arguments(p, a)
    assert (a.ground, a.save_ground, a.ground_tol, a.max_height) == (False, False, 0.2, 3.0)
    assert not inference._geometry_requested(a)
    a = p.parse_args(["--save_ground", "--ground_tol", "0.3", "--max_height", "2.5"] + CAMERA)
    inference.check_geometry_arguments(p, a)
    assert (a.ground, a.save_ground, a.ground_tol, a.max_height) == (True, True, 0.3, 2.5)
    assert inference._geometry_requested(a)


@pytest.mark.parametrize("flag", ["--ground", "--save_ground"])
def test_cli_refuses_ground_without_camera_or_with_workers(flag, capsys):
    assert "--ground and --save_ground need a camera" in _cli_refused([flag], capsys)
    assert "sequential mode only" in _cli_refused([flag, "--workers", "2"] + CAMERA, capsys)


@pytest.mark.parametrize("extra", [["--ground_tol", "-1"], ["--ground_tol", "nan"], ["--max_height", "inf"], ["--ground_tol", "4"]])
def test_cli_refuses_bad_ground_heights(extra, capsys):
    assert "0 <= ground_tol <= max_height" in _cli_refused(["--ground"] + extra + CAMERA, capsys)


def test_ground_png_helpers():
    from lwsnet_amd import inference
    codes = np.array([[0, 1, 2], [3, 4, 5]], np.uint8)
    left = np.full((2, 3, 3), 100, np.uint8)
    left[0, 0] = (255, 255, 255)
    rgb = inference.ground_to_rgb(codes, left)
    assert rgb.dtype == np.uint8 and rgb.shape == (2, 3, 3)
    assert rgb[0, 0].tolist() == [128, 128, 128] and rgb[0, 1].tolist() == [50, 150, 50] and rgb[0, 2].tolist() == [178, 50, 50]
    bev = inference.bev_to_u8(np.array([[0.0, 1.5], [3.0, 4.0]], F), 3.0)
    assert bev.tolist() == [[255, 255], [0, 128]]                               # row 0 the farthest; rint(127.5) = 128
    assert inference.bev_to_u8(np.array([[0.0, 1.0]], F), 0.0).tolist() == [[0, 255]]


@pytest.mark.parametrize("flag", ["--ground", "--save_ground"])
def test_cli_ground_error_texts(flag, capsys):
    assert _cli_refused([flag], capsys).endswith(": error: --ground and --save_ground need a camera: --calib PATH or --camera FX FY CX CY BASELINE\n")
    assert _cli_refused([flag, "--workers", "2"], capsys).endswith("--camera FX FY CX CY BASELINE\n"), "the camera comes before the mode"
    assert _cli_refused([flag, "--workers", "2"] + CAMERA, capsys).endswith(
        ": error: --ground / --save_ground run in the sequential mode only: use --workers 0\n")
    assert _cli_refused([flag, "--ground_tol", "4"] + CAMERA, capsys).endswith(
        ": error: --ground_tol and --max_height must be finite with 0 <= ground_tol <= max_height, got 4.0 and 3.0\n")
    assert _cli_refused([flag, "--max_height", "inf", "--max_jump", "-1"], capsys).endswith(
        ": error: --ground_tol and --max_height must be finite with 0 <= ground_tol <= max_height, got 0.2 and inf\n"), "the heights come first"
