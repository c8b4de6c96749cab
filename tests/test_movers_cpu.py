"""Mover segmentation without a GPU: the numpy restatement (tests/movers_reference.py) against brute force -- the components by
repeated relaxation, the order of the taps on hand-made ties --, what it finds in the road-and-wall scene with a box pasted in (a
static scene, a box that approaches, recedes, moves sideways; recall and false positives under noise), and the host pieces:
argument errors of the C ABI, of ops.movers and of MoverSegmenter, the inference CLI's flags, the header's table, the benchmark tool."""
import ctypes
import os

import numpy as np
import pytest

import movers_reference as R
import temporal_reference as T
from cli_helpers import CAMERA, cli_refused as _cli_refused, poses_file, sequence_dir as _sequence_dir
from lwsnet_amd import _lib

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "lwsnet_movers.h"
INF, NAN = float("inf"), float("nan")
SCENE_KW = dict(min_disp=0.5, sigma0=0.5)                   # the gates at their defaults: 3 standard deviations, 25 grey levels
# Measured once with this restatement on the scenes below at 0.2 px of disparity noise, seed 0 (printed by the test): the box's
# pixels that are members of a mover over the box's visible pixels, and the mover pixels outside the box.  The approaching box
# stands 3.03 standard deviations from the static prediction at its centre, so 0.2 px of noise takes a third of it below the gate.
MEASURED = {"approaching": (99 / 144, 0), "lateral": (144 / 144, 0)}
BOX_PERIMETER = 44                                          # the pixels on the edge of the 12 x 12 box


def run_scene(name, noise=0.0, seed=0, **kw):
    boxes = R.BOX.get(name, (None, None))
    case, inside = R.scene_pair(*boxes, noise=noise, seed=seed)
    return R.run_case(case, **{**SCENE_KW, **kw}), inside


# ---- the restatement against brute force ----
def relaxed_components(cand, d, max_diff):
    """The component map by repeated relaxation: every candidate starts with its raster index, every joined pair takes the smaller
    of its two labels, until nothing changes; then the labels are ranked."""
    H, W = cand.shape
    lab = np.where(cand, np.arange(H * W).reshape(H, W), -1)
    with np.errstate(all="ignore"):
        jx = cand[:, 1:] & cand[:, :-1] & (np.abs(d[:, 1:] - d[:, :-1]) <= F(max_diff))
        jy = cand[1:] & cand[:-1] & (np.abs(d[1:] - d[:-1]) <= F(max_diff))
    while True:
        before = lab.copy()
        for a, b, j in ((lab[:, 1:], lab[:, :-1], jx), (lab[1:], lab[:-1], jy)):         # views: a label only ever goes down
            m = np.minimum(a, b)
            a[j] = np.minimum(a[j], m[j])
            b[j] = np.minimum(b[j], m[j])
        if (lab == before).all():
            break
    roots = np.unique(lab[lab >= 0])
    return np.where(lab >= 0, np.searchsorted(roots, lab), -1).astype(np.int32)


@pytest.mark.parametrize("seed", range(4))
def test_flood_fill_matches_repeated_relaxation(seed):
    rng = np.random.default_rng(seed)
    H, W = 23, 31
    cand = rng.random((H, W)) < (0.45, 0.6, 0.75, 1.0)[seed]
    d = (8 + rng.integers(0, 4, (H, W)) * F(0.5)).astype(F)
    d[rng.random((H, W)) < 0.05] = np.nan                   # a NaN joins nothing
    for max_diff in (0.0, 0.5, 1.0, INF):
        comp, sizes = R.components(cand, d, max_diff)
        want = relaxed_components(cand, d, max_diff)
        assert np.array_equal(comp, want), (seed, max_diff)
        assert np.array_equal(sizes, np.bincount(want[want >= 0], minlength=len(sizes)))
    assert R.components(R.spiral(H, W), np.zeros((H, W), F), 1.0)[1].tolist() == [int(R.spiral(H, W).sum())]


def test_the_first_tap_wins_a_tie_in_row_major_order():
    """Two taps of the window at the same distance from the prediction, one above it and one below: the earlier in the scan gives the
    sign, and with it the code."""
    H, W = 7, 9
    want = np.full((H, W), R.STATIC, np.uint8)
    y, x = 3, 4
    for first, second, code in (((y - 1, x - 1), (y - 1, x), R.UNCOVERED), ((y - 1, x), (y, x - 1), R.UNCOVERED), ((y, x + 1), (y + 1, x), R.UNCOVERED)):
        for sign in (1, -1):
            case = R.pattern_case(want)
            dp = np.full((H, W), 8 + 5, F)                  # every other tap is further off
            dp[first], dp[second] = 8 + 2 * sign, 8 - 2 * sign
            case["disp_prev"] = dp[None, None]
            okc = np.ones((H, W), bool)
            p = R.params(radius=1, gate_g=1.0)
            have, rg, _, _, _ = R.residuals(case["rgb_prev"][0], dp, None, okc, case["rgb_cur"][0], case["disp_cur"][0, 0], None, okc, case["cam"][0],
                                            case["pose"][0], p)
            s = np.sqrt(F(0.5) * F(0.5) + F(0.5) * F(0.5))
            assert have[y, x] and rg[y, x] == F(2 * sign) / s, (first, sign, rg[y, x])
            ev = R.run_case(case, radius=1, gate_g=1.0)["evidence"][0, 0]
            assert ev[y, x] == (R.UNCOVERED if sign > 0 else R.APPEARED)
    # radius 0 sees the centre tap alone
    assert R.run_case(case, radius=0, gate_g=1.0)["evidence"][0, 0][y, x] == R.UNCOVERED


def test_rows_vals_and_info_of_a_hand_made_image():
    want = np.full((6, 10), R.STATIC, np.uint8)
    want[1, 1:5] = R.APPEARED
    want[2, 1:3] = R.UNCOVERED
    want[4, 6:9] = R.CHANGED
    want[0, 9] = R.UNTESTED
    out = R.run_case(R.pattern_case(want), cand_bits=28, min_pixels=3, grow=1, max_movers=3)
    assert np.array_equal(out["evidence"][0, 0], want)
    assert out["rows"][0].tolist() == [[6, 1, 4, 1, 2, 4, 2, 0], [3, 6, 8, 4, 4, 0, 0, 3], list(R.EMPTY_ROW)]
    assert out["vals"][0].tolist() == [[8.0, 8.0], [8.0, 8.0], [0.0, 0.0]]
    assert out["info"][0].tolist() == [59, 50, 4, 2, 3, 2, 2, (6 * 3 + 4) + 5 * 3]
    assert out["labels"][0, 0][1, 1] == 0 and out["labels"][0, 0][4, 7] == 1 and out["mask"][0, 0][0, 9] == 0 and out["mask"][0, 0][0, 0] == 4


# ---- what it finds in a scene ----
@pytest.mark.parametrize("radius", (0, 1))
@pytest.mark.parametrize("noise", (0.0, 0.2))
def test_a_static_scene_has_no_movers(noise, radius):
    out, _ = run_scene("static", noise=noise, radius=radius)
    info = out["info"][0]
    print("static scene, noise", noise, "radius", radius, "info", info.tolist())
    assert info[0] > 2500 and info[2] == info[3] == info[4] == 0 and info[5] == info[6] == info[7] == 0
    assert (out["labels"] == -1).all() and (out["mask"] != R.MOVER_CODE).all()


@pytest.mark.parametrize("radius", (0, 1))
def test_an_approaching_box_is_one_mover(radius):
    out, inside = run_scene("approaching", radius=radius)
    ev, lab = out["evidence"][0, 0], out["labels"][0, 0]
    print("approaching, radius", radius, "info", out["info"][0].tolist(), "rows", out["rows"][0, 0].tolist(), "vals", out["vals"][0, 0].tolist())
    assert inside.sum() == 144 and (ev[inside] == R.APPEARED).all() and (lab[inside] == 0).all() and out["info"][0, 6] == 1
    assert out["rows"][0, 0, 0] >= 144 and abs(out["vals"][0, 0, 1] - 3.2) < 0.01
    ys, xs = np.nonzero(inside)
    oy, ox = np.nonzero((lab >= 0) & ~inside)
    if len(oy):
        dist = np.min(np.maximum(np.abs(oy[:, None] - ys[None]), np.abs(ox[:, None] - xs[None])), 1)
        assert dist.max() <= 1 + radius
    grown = R.grow_flags(lab >= 0, 2)
    assert np.array_equal(out["mask"][0, 0] == R.MOVER_CODE, grown)


def test_a_receding_box_is_uncovered_and_a_mover_only_when_asked():
    out, inside = run_scene("receding")
    assert inside.sum() == 144 and (out["evidence"][0, 0][inside] == R.UNCOVERED).all()
    assert out["info"][0, 6] == 0 and (out["labels"] == -1).all()
    out, _ = run_scene("receding", cand_bits=R.DEFAULTS["cand_bits"] | 1 << R.UNCOVERED)
    lab = out["labels"][0, 0]
    assert out["info"][0, 6] >= 1 and len(np.unique(lab[inside])) == 1 and lab[inside][0] >= 0
    j = lab[inside][0]
    assert out["rows"][0, j, 0] == 144 and out["rows"][0, j, 6] == 144 and abs(out["vals"][0, j, 1] - 4.0) < 0.01


def test_a_lateral_box_is_changed_over_its_old_footprint_and_appeared_beside_it():
    out, inside = run_scene("lateral")
    prev_rect = R.box_rect(R.E.scene_cam(48, 96), *R.BOX["lateral"][0], 48, 96)
    ev = out["evidence"][0, 0]
    xs = np.broadcast_to(np.arange(96)[None, :], (48, 96))
    # the camera turns 0.01 rad between the frames: the old footprint is seen fx * 0.01 = 1.2 columns further left in the current frame
    old = inside & (xs < prev_rect[1] - 2)
    new = inside & (xs >= prev_rect[1])
    print("lateral: box codes", np.bincount(ev[inside], minlength=5).tolist(), "old footprint", int(old.sum()), "new ground", int(new.sum()))
    assert old.sum() >= 60 and new.sum() >= 60
    assert (ev[old] == R.CHANGED).all() and (ev[new] == R.APPEARED).all() and set(ev[inside].tolist()) == {R.APPEARED, R.CHANGED}
    assert out["info"][0, 6] == 1 and (out["labels"][0, 0][inside] == 0).all() and out["rows"][0, 0, 0] == 144


@pytest.mark.parametrize("name", ("approaching", "lateral"))
def test_recall_and_false_positives_under_noise(name):
    """0.2 px of seeded noise on both disparity maps, seed 0.  Recall no lower than the measured value less 0.05 and false positives
    no more than the measured count plus the box's perimeter.  The restatement is deterministic per seed, so the margin is not there
    for this seed; seeds 1 and 2 are printed beside it (DESIGN.md has them): the approaching box, which stands at the gate's edge,
    moves by more than the margin from seed to seed, the lateral one does not move."""
    recall0, fp0 = MEASURED[name]
    for seed in (0, 1, 2):
        out, inside = run_scene(name, noise=0.2, seed=seed)
        member = out["labels"][0, 0] >= 0
        recall, fp = (member & inside).sum() / inside.sum(), int((member & ~inside).sum())
        print(name, "seed", seed, "recall", round(float(recall), 4), "false positives", fp, "info", out["info"][0].tolist())
        if seed == 0:
            assert abs(recall - recall0) < 1e-9 and fp == fp0          # MEASURED is what this restatement gives
            assert recall >= recall0 - 0.05 and fp <= fp0 + BOX_PERIMETER


# ---- argument errors ----
def _p(k, off=0):
    """Fake device pointers 1 GiB apart: never dereferenced, every call below is refused first."""
    return ctypes.c_void_p((1 << 40) + (k << 30) + off)


NAMES = ("rgb_prev", "disp_prev", "sigma_prev", "mask_prev", "rgb_cur", "disp_cur", "sigma_cur", "mask_cur", "cam", "pose", "workspace", "evidence",
         "mask_out", "labels", "rows", "vals", "info")
SCALARS = dict(min_disp=1.0, sigma0=0.5, sigma_min=0.05, gate_g=3.0, gate_p=25.0, radius=0, cand_bits=20, max_diff=1.0, min_pixels=64, grow=2,
               max_movers=64)


def test_movers_rejects_bad_arguments(hip_lib):
    base = {name: _p(k) for k, name in enumerate(NAMES)}
    INV = _lib.LWS_ERR_INVALID

    def call(B=1, H=8, W=16, **kw):
        a = {**base, **SCALARS, **kw}
        return hip_lib.lws_movers(*(a[n] for n in NAMES[:10]), B, H, W, *(a[n] for n in SCALARS), *(a[n] for n in NAMES[10:]), None)

    def at(name, off):
        return _p(NAMES.index(name), off)

    w = b"movers: "
    null_in = w + b"rgb_prev, disp_prev, rgb_cur, disp_cur, cam and pose must not be null"
    null_out = w + b"workspace, evidence, mask_out, rows, vals and info must not be null"
    al = w + b"disp / sigma / cam / pose / labels / rows / vals / info must be 4-byte, workspace 16-byte aligned"
    for kw, msg in [
        *((dict([(n, None)]), null_in) for n in ("rgb_prev", "disp_prev", "rgb_cur", "disp_cur", "cam", "pose")),
        *((dict([(n, None)]), null_out) for n in ("workspace", "evidence", "mask_out", "rows", "vals", "info")),
        (dict(B=0), w + b"bad shape B=0 H=8 W=16"), (dict(B=65536), w + b"bad shape B=65536 H=8 W=16"), (dict(H=0), w + b"bad shape B=1 H=0 W=16"),
        (dict(H=1 << 16, W=1 << 15), w + b"H*W = 65536x32768 must be < 2^31"),
        (dict(H=1, W=(1 << 24) + 1), w + b"H=1 W=16777217 exceed 16777216 (pixel coordinates are exact floats)"),
        (dict(max_movers=0), w + b"max_movers 0 outside 1..65536"), (dict(max_movers=65537), w + b"max_movers 65537 outside 1..65536"),
        *((dict([(n, at(n, 2))]), al) for n in ("disp_prev", "sigma_prev", "disp_cur", "sigma_cur", "cam", "pose", "labels", "rows", "vals", "info")),
        (dict(workspace=at("workspace", 8)), al),
        (dict(min_disp=0.0), w + b"min_disp must be finite and > 0, got 0"), (dict(min_disp=NAN), w + b"min_disp must be finite and > 0, got nan"),
        (dict(sigma0=-0.1), w + b"sigma0 must be finite and >= 0, got -0.1"), (dict(sigma0=INF), w + b"sigma0 must be finite and >= 0, got inf"),
        (dict(sigma_min=0.0), w + b"sigma_min must be finite and > 0, got 0"),
        (dict(gate_g=0.0), w + b"gate_g must be finite and > 0, got 0"), (dict(gate_g=INF), w + b"gate_g must be finite and > 0, got inf"),
        (dict(gate_p=0.0), w + b"gate_p must be > 0 (+inf: no photometric test), got 0"),
        (dict(gate_p=NAN), w + b"gate_p must be > 0 (+inf: no photometric test), got nan"),
        (dict(radius=-1), w + b"radius -1 outside 0..2"), (dict(radius=3), w + b"radius 3 outside 0..2"),
        *((dict(cand_bits=c), w + b"cand_bits %d outside 0..31 or with bit 0 or 1 set (untested and static pixels are no candidates)" % c)
          for c in (-1, 1, 2, 21, 32)),
        (dict(max_diff=-1.0), w + b"max_diff must be >= 0 (+inf allowed), got -1"), (dict(max_diff=NAN), w + b"max_diff must be >= 0 (+inf allowed), got nan"),
        (dict(min_pixels=0), w + b"min_pixels 0 < 1"), (dict(grow=-1), w + b"grow -1 outside 0..8"), (dict(grow=9), w + b"grow 9 outside 0..8"),
        (dict(evidence=at("workspace", 16)), w + b"evidence and workspace overlap"), (dict(mask_out=at("evidence", 127)), w + b"mask_out and evidence overlap"),
        (dict(labels=at("mask_out", 0)), w + b"labels and mask_out overlap"), (dict(rows=at("labels", 4 * 128 - 4)), w + b"rows and labels overlap"),
        (dict(vals=at("rows", 32 * 64 - 4)), w + b"vals and rows overlap"), (dict(info=at("vals", 8 * 64 - 4)), w + b"info and vals overlap"),
        (dict(mask_cur=at("info", 31)), w + b"mask_cur and info overlap"), (dict(mask_cur=at("mask_out", 1)), w + b"mask_cur and mask_out overlap"),
        (dict(rgb_prev=at("workspace", 0)), w + b"rgb_prev and workspace overlap"), (dict(disp_prev=at("evidence", 0)), w + b"disp_prev and evidence overlap"),
        (dict(sigma_prev=at("labels", 0)), w + b"sigma_prev and labels overlap"), (dict(mask_prev=at("mask_out", 0)), w + b"mask_prev and mask_out overlap"),
        (dict(rgb_cur=at("rows", 0)), w + b"rgb_cur and rows overlap"), (dict(disp_cur=at("vals", 0)), w + b"disp_cur and vals overlap"),
        (dict(sigma_cur=at("info", 0)), w + b"sigma_cur and info overlap"), (dict(cam=at("evidence", 4)), w + b"cam and evidence overlap"),
        (dict(pose=at("workspace", 64)), w + b"pose and workspace overlap"),
    ]:
        assert call(**kw) == INV, kw
        assert hip_lib.lws_last_error() == msg, (kw, hip_lib.lws_last_error())
    # the optional pointers may be null, the photometric gate and max_diff +inf, cand_bits 0, mask_out may be mask_cur itself, and
    # inputs may share memory: the next refusal is about something else
    assert call(sigma_prev=None, mask_prev=None, sigma_cur=None, mask_cur=None, labels=None, gate_p=INF, max_diff=INF, cand_bits=0,
                rgb_cur=at("rgb_prev", 0), min_pixels=0) == INV
    assert hip_lib.lws_last_error() == w + b"min_pixels 0 < 1"
    assert call(mask_out=at("mask_cur", 0), grow=9) == INV and hip_lib.lws_last_error() == w + b"grow 9 outside 0..8"
    # the workspace: per pixel 4 + 48 + 1 + 1 bytes, 16 per evidence tile of 4 x 64 and 8 per block of 2048 pixels, each part to 256
    ws, r = hip_lib.lws_movers_workspace, lambda n: -(-n // 256) * 256
    assert ws(2, 40, 60, 64) == r(4 * 4800) + r(48 * 4800) + 2 * r(4800) + r(16 * 2 * 10) + r(8 * 2 * 2)
    assert ws(1, 5, 7, 1) == r(140) + r(48 * 35) + 2 * r(35) + r(16 * 2) + r(8)
    assert ws(0, 5, 7, 1) == INV and hip_lib.lws_last_error() == b"movers_workspace: bad shape B=0 H=5 W=7"
    assert ws(1, 5, 7, 0) == INV and hip_lib.lws_last_error() == b"movers_workspace: max_movers 0 outside 1..65536"
    assert ws(1, 1 << 16, 1 << 15, 1) == INV


def test_ops_and_segmenter_validate_before_any_gpu_call():
    import inspect
    import torch
    from lwsnet_amd import movers, ops
    from lwsnet_amd.geometry import Camera
    cam = Camera(120.0, 120.0, 47.5, 20.0, 0.5)
    z = np.zeros((1, 1, 4, 4), F)
    pose = np.array(R.IDENTITY_POSE)
    with pytest.raises(ValueError, match="movers needs cameras"):
        ops.movers(z, z, z, z, None, pose)
    with pytest.raises(ValueError, match="movers needs pose"):
        ops.movers(z, z, z, z, cam, None)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.movers(z, z, z, z, cam, pose)
    bad = ((dict(min_disp=0.0), "min_disp must be finite and > 0"), (dict(sigma0=-1.0), "sigma0 must be finite and >= 0"),
           (dict(sigma_min=0.0), "sigma_min must be finite and > 0"), (dict(gate_g=INF), "gate_g must be finite and > 0"),
           (dict(gate_p=0.0), "gate_p must be > 0"), (dict(gate_p=NAN), "gate_p must be > 0"), (dict(radius=3), "radius must be an integer in 0 .. 2"),
           (dict(cand_bits=32), "cand_bits must be an integer in 0 .. 31"), (dict(cand_bits=5), "cand_bits must leave bits 0 and 1 clear"),
           (dict(max_diff=-1.0), "max_diff must be >= 0"), (dict(min_pixels=0), "min_pixels must be an integer in 1"),
           (dict(grow=9), "grow must be an integer in 0 .. 8"), (dict(max_movers=65537), "max_movers must be an integer in 1 .. 65536"))
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            ops.movers(None, None, None, None, cam, pose, **kw)
        with pytest.raises(ValueError, match=msg):
            movers.MoverSegmenter(cam, **kw)
    with pytest.raises(ValueError, match="MoverSegmenter needs cameras"):
        movers.MoverSegmenter(None)
    with pytest.raises(ValueError, match="unknown parameters"):
        movers.MoverSegmenter(cam, gate=3.0)
    sig = inspect.signature(ops.movers).parameters
    assert {k: sig[k].default for k in ops.MOVERS_DEFAULTS} == ops.MOVERS_DEFAULTS == {**R.DEFAULTS}
    assert ops.movers_args(**ops.MOVERS_DEFAULTS) == tuple(ops.MOVERS_DEFAULTS.values()) and list(ops.MOVERS_DEFAULTS) == list(SCALARS)
    assert ops.MoversResult._fields == ("evidence", "mask", "labels", "rows", "vals", "info")
    assert ops.MOVER_CODE == R.MOVER_CODE == 4 and ops.MOVER_CANDIDATES == 20 and len(ops.MOVER_EVIDENCE) == 5
    # the first step keeps the frame and segments nothing (no GPU call), and so does a step without a pose
    seg = movers.MoverSegmenter(cam, min_pixels=8)
    assert seg.params["min_pixels"] == 8 and seg.params["grow"] == 2 and seg.prev is None
    rgb, disp = torch.zeros((1, 4, 6, 3), dtype=torch.uint8), torch.ones((1, 1, 4, 6))
    assert seg.step(rgb, disp, None) is None and seg.prev is not None and seg.prev[2] is None
    assert seg.step(rgb, disp, None, mask=torch.ones((1, 1, 4, 6), dtype=torch.uint8)) is None and seg.prev[2] is not None
    with pytest.raises(RuntimeError, match="HIP device"):
        seg.step(rgb, disp, pose)
    with pytest.raises(ValueError, match="the previous frame"):
        seg.step(rgb, torch.ones((1, 1, 4, 5)), pose)


# ---- the inference CLI ----
NEW_FLAGS = ("movers", "movers_gate", "movers_gate_p", "movers_radius", "movers_min_pixels", "movers_grow", "movers_uncovered", "save_movers")


def test_movers_flags_default_off(tmp_path):
    from lwsnet_amd import inference, sequence
    assert sequence.MOVERS_DEFAULTS == dict(movers=False, movers_gate=3.0, movers_gate_p=25.0, movers_radius=0, movers_min_pixels=64, movers_grow=2,
                                            movers_uncovered=False, save_movers=False)
    assert tuple(sequence.MOVERS_DEFAULTS) == NEW_FLAGS
    assert not set(NEW_FLAGS) & (set(sequence.TSDF_DEFAULTS) | set(sequence.EGO_DEFAULTS) | set(sequence.TEMPORAL_DEFAULTS) | set(sequence.TRACK_DEFAULTS))
    p = inference.build_parser()
    a = p.parse_args([])
    assert not any(hasattr(a, name) for name in NEW_FLAGS)                      # the namespace of a line without them
    with_flags = vars(p.parse_args(["--movers", "--movers_gate", "4", "--movers_gate_p", "inf", "--movers_radius", "1", "--movers_min_pixels", "32",
                                    "--movers_grow", "0", "--movers_uncovered", "--save_movers"]))
    assert {k: v for k, v in with_flags.items() if k not in NEW_FLAGS} == vars(a)
    assert [with_flags[f] for f in NEW_FLAGS] == [True, 4.0, INF, 1, 32, 0, True, True]
    sequence.check_movers_arguments(p, a)
    assert tuple(getattr(a, f) for f in NEW_FLAGS) == tuple(sequence.MOVERS_DEFAULTS.values())
    seq = _sequence_dir(tmp_path, 3)
    a = p.parse_args(seq + ["--egomotion", "--movers", "--movers_gate_p", "inf", "--save_movers"] + CAMERA)
    inference.check_geometry_arguments(p, a)
    inference.check_egomotion_arguments(p, a)
    inference.check_temporal_arguments(p, a)
    inference.check_tsdf_arguments(p, a)
    sequence.check_movers_arguments(p, a)
    assert a.movers and a.save_movers and (a.movers_gate, a.movers_gate_p, a.movers_radius, a.movers_min_pixels, a.movers_grow) == (3.0, INF, 0, 64, 2)


def test_cli_refuses_movers_without_what_it_needs(tmp_path, capsys):
    seq = _sequence_dir(tmp_path, 3)
    ok = seq + ["--egomotion", "--movers"] + CAMERA
    poses = poses_file(tmp_path / "poses.txt", 3)
    assert _cli_refused(seq + ["--movers"] + CAMERA, capsys).endswith(": error: --movers needs the motion between the frames: --poses PATH or --egomotion\n")
    assert _cli_refused(seq + ["--poses", poses, "--movers"], capsys).endswith(
        ": error: --movers and --save_movers need a camera: --calib PATH or --camera FX FY CX CY BASELINE\n")
    assert _cli_refused(seq + ["--poses", poses, "--movers", "--workers", "2"] + CAMERA, capsys).endswith(
        ": error: --movers / --save_movers run in the sequential mode only: use --workers 0\n")
    assert _cli_refused(["--left_img", str(tmp_path / "left_test.png"), "--movers"] + CAMERA, capsys).endswith(
        ": error: --movers follows a sequence: use directory mode (--img_path), not --left_img\n")
    short = poses_file(tmp_path / "short.txt", 2)
    assert "short.txt holds 2 poses for 3 pairs" in _cli_refused(seq + ["--poses", short, "--movers"] + CAMERA, capsys)       # the file is read for --movers alone
    assert _cli_refused(seq + ["--poses", poses] + CAMERA, capsys).endswith(": error: --poses, --temporal_gate, --temporal_q, --temporal_sigma and --temporal_hold need --temporal\n")
    needs = (": error: --movers_gate, --movers_gate_p, --movers_radius, --movers_min_pixels, --movers_grow, --movers_uncovered and --save_movers "
             "need --movers\n")
    for flags in (["--movers_gate", "3"], ["--movers_gate_p", "10"], ["--movers_radius", "1"], ["--movers_min_pixels", "8"], ["--movers_grow", "1"],
                  ["--movers_uncovered"], ["--save_movers"]):
        assert _cli_refused(seq + ["--egomotion"] + flags + CAMERA, capsys).endswith(needs)
    assert _cli_refused(ok + ["--movers_gate", "0"], capsys).endswith(": error: --movers_gate must be finite and > 0, got 0.0\n")
    assert _cli_refused(ok + ["--movers_gate", "inf"], capsys).endswith(": error: --movers_gate must be finite and > 0, got inf\n")
    assert _cli_refused(ok + ["--movers_gate_p", "0"], capsys).endswith(": error: --movers_gate_p must be > 0 (inf switches the term off), got 0.0\n")
    assert _cli_refused(ok + ["--movers_gate_p", "nan"], capsys).endswith(": error: --movers_gate_p must be > 0 (inf switches the term off), got nan\n")
    assert _cli_refused(ok + ["--movers_radius", "3"], capsys).endswith(": error: --movers_radius must be in 0 .. 2, got 3\n")
    assert _cli_refused(ok + ["--movers_min_pixels", "0"], capsys).endswith(": error: --movers_min_pixels must be in 1 .. 2147483647, got 0\n")
    assert _cli_refused(ok + ["--movers_grow", "9"], capsys).endswith(": error: --movers_grow must be in 0 .. 8, got 9\n")
    assert _cli_refused(ok + ["--movers_grow", "-1"], capsys).endswith(": error: --movers_grow must be in 0 .. 8, got -1\n")
    assert _cli_refused(seq + ["--tsdf", "--poses", poses, "--movers", "--movers_radius", "5"] + CAMERA, capsys).endswith(
        ": error: --movers_radius must be in 0 .. 2, got 5\n")                  # a poses file is a pose source too
    assert not os.path.exists(tmp_path / "out")             # refused before the output folder is touched


def test_the_stage_sits_between_tracking_and_the_filter_and_asks_quietly(caplog):
    import logging
    from types import SimpleNamespace
    from lwsnet_amd import ops, outputs, sequence
    args = SimpleNamespace(egomotion=True, tsdf_track=False, movers=True, temporal=True, tsdf=False, poses=None)
    _, stages = sequence.begin(args, 3, None, logging.getLogger("test_movers_cpu"))
    assert [type(s).__name__ for s in stages] == ["_Odometry", "_Movers", "_Sequence"]
    assert args.movers_gate == 3.0 and args.save_movers is False
    src = sequence.PoseSource(3)
    log = logging.getLogger("test_movers_cpu")
    rec = SimpleNamespace(frame=SimpleNamespace(path="x.png"), ego=SimpleNamespace(status=[ops.EGO_UNTRUSTED], pose=None), track=None)
    with caplog.at_level(logging.WARNING, logger="test_movers_cpu"):
        assert src.relative(rec, log, warn=False) is None and not caplog.records      # the movers stage asks first and says its own line
        assert src.relative(rec, log) is None and len(caplog.records) == 1             # the filter's warning comes once
    src.tracker = SimpleNamespace(poses=lambda: None)
    rec.track = SimpleNamespace(status=[ops.TRACK_UNTRUSTED], pose=None)
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="test_movers_cpu"):
        assert src.relative(rec, log, warn=False) is None and not caplog.records
    # the converters behind --save_movers and the log line
    ev = np.array([[0, 1, 2], [3, 4, 4], [1, 1, 1]], np.uint8)
    lab = np.array([[-1, -1, 0], [-1, 0, 0], [-1, -1, -1]], np.int32)
    rgb = outputs.movers_to_rgb(ev, lab)
    assert rgb[0, 0].tolist() == [0, 0, 0] and rgb[0, 1].tolist() == outputs.MOVERS_COLOURS[1].tolist() and rgb[1, 0].tolist() == outputs.MOVERS_COLOURS[3].tolist()
    assert all(rgb[y, x].tolist() == [255, 255, 255] for y, x in ((0, 2), (1, 1), (1, 2)))          # a mover this small is all outline
    big = outputs.movers_to_rgb(np.full((5, 5), 2, np.uint8), np.pad(np.zeros((3, 3), np.int32), 1, constant_values=-1))
    assert big[2, 2].tolist() == outputs.MOVERS_COLOURS[2].tolist() and big[1, 1].tolist() == [255, 255, 255] and big[0, 0].tolist() == outputs.MOVERS_COLOURS[2].tolist()
    assert outputs.MOVERS_CODES == ops.MOVER_EVIDENCE and outputs.MOVERS_COLOURS.shape == (5, 3)
    rows = np.array([[30, 1, 6, 2, 7, 30, 0, 0], [50, 10, 19, 3, 8, 0, 0, 50], list(R.EMPTY_ROW)], np.int32)
    vals = np.array([[6.0, 10.0], [15.0, 4.0], [0.0, 0.0]], F)
    assert outputs.movers_line([100, 20, 30, 0, 50, 7, 2, 140], rows, vals) == (
        "Movers: tested = 100, static = 20, appeared = 30, uncovered = 0, changed = 50, components = 7, movers = 2, masked pixels = 140, "
        "nearest = #1 x 10..19 y 3..8 (50 px) at 4.00 m")
    assert outputs.movers_line([9, 9, 0, 0, 0, 0, 0, 0], rows[2:], vals[2:]).endswith("movers = 0, masked pixels = 0")


def test_a_run_without_codes_gets_a_stage4_keep():
    import torch
    from lwsnet_amd import postprocess as post
    d = [torch.zeros((1, 1, 2, 3)) for _ in range(4)]
    mask = torch.tensor([[[[1, 4, 4], [0, 1, 1]]]], dtype=torch.uint8)
    res = post.ChainResult(d, None, None, None, None, None, None)
    new = res.with_stage4_keep(mask)
    assert new.keep[3] is mask and all((k == 1).all() and k.dtype == torch.uint8 for k in new.keep[:3]) and new.disp[3] is d[3]
    old = [torch.full((1, 1, 2, 3), s, dtype=torch.uint8) for s in range(4)]
    kept = post.ChainResult(d, None, None, old, None, None, None, occ_masks="m", occ_density="d").with_stage4_keep(mask)
    assert kept.keep[3] is mask and all(kept.keep[s] is old[s] for s in range(3)) and (kept.occ_masks, kept.occ_density) == ("m", "d")


# ---- the ABI ----
EXPECTED_NAMES = ["lws_movers", "lws_movers_workspace"]


def test_the_header_is_read_into_a_table_of_its_own(hip_lib):
    from lwsnet_amd import build
    assert _lib.MOVERS_HEADERS == (HEADER,) == tuple(_lib.MOVERS_ABI)
    protos, spellings, path = _lib.MOVERS_ABI[HEADER]
    assert os.path.samefile(path, os.path.join(ROOT, "include", HEADER))
    assert sorted(protos) == EXPECTED_NAMES == sorted(spellings) and protos == _lib.MOVERS_PROTOTYPES
    v, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert protos["lws_movers_workspace"] == (ctypes.c_int64, [i, i, i, i])
    assert protos["lws_movers"] == (i, [v] * 10 + [i] * 3 + [f] * 5 + [i] * 2 + [f] + [i] * 3 + [v] * 8)
    for name, (res, args) in protos.items():
        fn = getattr(hip_lib, name)
        assert fn.argtypes == args and fn.restype is res, name
    sp = spellings["lws_movers"][1]
    assert sp[0] == "const uint8_t *" and sp[9] == "const float *" and sp[-8:] == ["void *", "uint8_t *", "uint8_t *", "int32_t *", "int32_t *", "float *", "int32_t *", "void *"]
    assert "lws_movers.hip" in build.SOURCES and hip_lib.lws_abi_version() == 8 == _lib.LWS_ABI_VERSION
    # the tables the other tests count are what they were, and no name is shared with them
    assert len(_lib.HEADERS) == 5 == len(_lib.ABI) and HEADER not in _lib.HEADERS and len(_lib.PROTOTYPES) == 67 and len(_lib.ALL_PROTOTYPES) == 78
    others = set(_lib.ALL_PROTOTYPES) | set(_lib.MESH_PROTOTYPES) | set(_lib.TRACK_PROTOTYPES) | set(_lib.WINDOW_PROTOTYPES)
    assert not set(protos) & others
    with pytest.raises(ValueError, match="lws_movers is declared by"):
        _lib.merge_headers({"lwsnet_track.h": {**_lib.TRACK_PROTOTYPES, "lws_movers": None}, HEADER: protos})
    # the four headers that named the gap point at this one
    for name in ("lwsnet_tsdf.h", "lwsnet_track.h", "lwsnet_egomotion.h", "lwsnet_temporal.h"):
        with open(os.path.join(ROOT, "include", name)) as fh:
            assert "include/lwsnet_movers.h" in fh.read(), name


def test_a_compiler_agrees_with_the_reading_of_the_header(tmp_path):
    from test_abi_cpu import _assert_line, compiles
    spellings = _lib.MOVERS_ABI[HEADER][1]
    lines = {name: _assert_line(name, sp) for name, sp in spellings.items()}
    ok = compiles(HEADER, tmp_path / "movers.cpp", lines.values())
    assert ok.returncode == 0, ok.stderr
    ret, params = spellings["lws_movers"]
    assert params[17] == "float" and params[18] == "int"            # gate_p, radius
    flipped = dict(lines, lws_movers=_assert_line("lws_movers", (ret, params[:18] + ["float"] + params[19:])))
    bad = compiles(HEADER, tmp_path / "movers_flipped.cpp", flipped.values())
    assert bad.returncode != 0 and '"lws_movers"' in bad.stderr and bad.stderr.count("error:") == 1, bad.stderr


# ---- the benchmark tool ----
def test_the_benchmark_tool_takes_its_method_from_benchkit():
    """tools/benchmovers.py under the rule tests/test_benchkit_cpu.py holds tools/*bench.py to: it compiles, imports benchkit, and
    neither defines nor borrows a timing method of its own."""
    import ast
    from test_benchkit_cpu import _names
    path = os.path.join(ROOT, "tools", "benchmovers.py")
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
    assert {"lws_movers", "lws_speckle_filter"} <= used
