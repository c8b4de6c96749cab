"""The temporal filter without a GPU: the numpy restatement (tests/temporal_reference.py) on an identity pose, on a box that jumps,
on pixels entering the view and on bad input; its noise and its hold on the synthetic road-and-wall scene, held to the conditions
the feature was asked to meet; the host pieces (poses, argument errors of the C ABI, of ops.temporal_step, of TemporalFilter and of
the inference CLI's flags); and the CLI's pose source over a poses file with skipped pairs."""
import ctypes
import os

import numpy as np
import pytest

import temporal_reference as T
from cli_helpers import CAMERA, cli_refused as _cli_refused, poses_file, sequence_dir
from lwsnet_amd import _lib

F = np.float32
# a camera whose projection round-trips exactly at z = 8: fx = fy a power of two, d = 8 = fb / 8
EXACT_CAM = np.array([[128.0, 128.0, 47.5, 20.0, 64.0]], F)
IDENT = T.relative(T.IDENTITY, T.IDENTITY)[None]


def test_identity_pose_is_a_fixed_point_and_the_variance_falls_as_one_over_n():
    m = np.full((1, 1, 48, 96), 8.0, F)
    prev, r = None, F(0.5) * F(0.5)
    for n in range(1, 9):
        D, V, A, code, counts = T.step(m, EXACT_CAM, IDENT, prev, sigma0=0.5)
        assert (D == F(8.0)).all() and (A == n).all()
        assert np.abs(V.astype(np.float64) / (float(r) / n) - 1.0).max() <= 4 * n * 2.0 ** -24      # a few roundings per frame
        assert (code == (1 if n == 1 else 2)).all() and counts[0].tolist() == ([0, 48 * 96, 0, 0, 0] if n == 1 else [0, 0, 48 * 96, 0, 0])
        prev = (D, V, A)


def test_a_box_that_jumps_is_reset_by_the_gate():
    """A box 3 px wide, 10 px nearer than its background, jumps 3 px to the right under an identity pose.  Code 3 (history
    disagreed) on the box and on the pixels it uncovered; the pixels whose four taps of the previous state straddle the old box's
    edge (more than max_jump apart) associate with nothing and are code 1; everything else fuses."""
    a = np.full((1, 1, 32, 40), 8.0, F)
    b = a.copy()
    a[0, 0, 10:20, 10:13] = 18.0
    b[0, 0, 10:20, 13:16] = 18.0
    s0 = T.step(a, EXACT_CAM, None, None)
    D, V, A, code, counts = T.step(b, EXACT_CAM, IDENT, s0[:3])
    want = np.full((32, 40), 2, np.uint8)
    want[9:20, 9:13] = 1                                    # a tap pair (x, x + 1) or (y, y + 1) with one foot in the old box ...
    want[10:19, 10:12] = 3                                  # ... but for the pixels whose four taps all lay inside it: uncovered
    want[10:20, 13:16] = 3                                  # the box, on what was background
    assert (code[0, 0] == want).all(), np.argwhere(code[0, 0] != want)[:8]
    assert counts[0].tolist() == [0, int((want == 1).sum()), int((want == 2).sum()), int((want == 3).sum()), 0]
    reset = want != 2
    assert (D[0, 0][reset] == b[0, 0][reset]).all() and (A[0, 0][reset] == 1).all() and (A[0, 0][~reset] == 2).all()


def test_pixels_entering_the_view_are_new():
    """The camera steps 3 px worth to the right in front of a fronto-parallel plane: the columns that were outside the previous
    image are code 1, the rest fuses."""
    m = np.full((1, 1, 16, 64), 8.0, F)
    cam = np.array([[128.0, 128.0, 31.5, 8.0, 64.0]], F)
    pose = T.relative(T.forward_pose(0, 0.0), T.forward_pose(1, 0.0, dx=3 * 8.0 / 128.0))[None]
    s0 = T.step(m, cam, None, None)
    D, V, A, code, _ = T.step(m, cam, pose, s0[:3])
    assert (code[0, 0, :, :60] == 2).all() and (code[0, 0, :, 61:] == 1).all()      # column 60 lands on the previous image's last column
    assert (D == F(8.0)).all() and (A[0, 0, :, :60] == 2).all() and (A[0, 0, :, 61:] == 1).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, -3.0, "sigma"])
def test_bad_input_is_code_0_and_never_poisons_a_neighbour(bad):
    m0 = np.full((1, 1, 12, 12), 8.0, F)
    sig = np.full((1, 1, 12, 12), 0.5, F)
    if bad == "sigma":
        sig[0, 0, 5, 5] = np.nan
    else:
        m0[0, 0, 5, 5] = bad
    cam = np.array([[128.0, 128.0, 5.5, 5.5, 64.0]], F)
    s0 = T.step(m0, cam, None, None, sigma=sig)
    assert s0[3][0, 0, 5, 5] == 0 and s0[2][0, 0, 5, 5] == 0 and (s0[3] == 1).sum() == 143
    good = np.full((1, 1, 12, 12), 8.0, F)
    s1 = T.step(good, cam, IDENT, s0[:3])
    want = np.full((12, 12), 2, np.uint8)
    want[4:6, 4:6] = 1                                      # the pixels with a tap on (5, 5) refuse it through Ap == 0
    assert (s1[3][0, 0] == want).all()
    s2 = T.step(good, cam, IDENT, s1[:3])
    assert (s2[3] == 2).all()
    for s in (s0, s1, s2):
        assert np.isfinite(s[0]).all() and np.isfinite(s[1]).all()


# ---- the synthetic scene: a road and a wall, the camera driving at the wall for eight frames ----
def _sequence(sigma, dz, seed, holes=False):
    rng = np.random.default_rng(seed)
    poses = [T.forward_pose(k, dz) for k in range(8)]
    truth = [T.render(p) for p in poses]
    frames = []
    for k, t in enumerate(truth):
        m = np.where(t > 0, t + rng.normal(0, sigma, t.shape), 0).astype(F)
        if holes and k >= 3:
            m[rng.random(t.shape) < 0.1] = np.nan
            m[30:40, 20:30] = np.nan
        frames.append(m[None, None])
    return poses, truth, frames


@pytest.mark.parametrize("sigma,dz", [(0.1, 0.3), (0.1, 0.6), (0.3, 0.3), (0.3, 0.6)])
def test_noise_on_the_static_scene(sigma, dz):
    """Over the pixels fused at least six times: RMS(fused - truth) / RMS(meas - truth) <= 0.5 (the ideal for eight frames is 0.354),
    |mean error| <= 0.02 px, at least half of the valid pixels there, at most 1 % of them reset by the gate.  Measured with this
    restatement: ratio 0.277 / 0.353 / 0.252 / 0.334, bias +0.0018 / +0.0008 / -0.0009 / -0.0035 px, share 0.76 / 0.77 / 0.67 / 0.70,
    8 pixels of code 3 in each."""
    poses, truth, frames = _sequence(sigma, dz, 0)
    D, V, A, code, _ = T.run_sequence(frames, T.SCENE_CAM, poses, sigma0=sigma, gate=3.0, q=0.0, max_jump=1.0, min_disp=0.5)[-1]
    valid = truth[-1] > 0.5
    sel = (A[0, 0] >= 6) & valid
    ef = D[0, 0][sel].astype(np.float64) - truth[-1][sel]
    em = frames[-1][0, 0][sel].astype(np.float64) - truth[-1][sel]
    ratio, bias, share, resets = np.sqrt((ef ** 2).mean() / (em ** 2).mean()), ef.mean(), sel.sum() / valid.sum(), int((code == 3).sum())
    print(f"sigma {sigma} dz {dz}: ratio {ratio:.3f}, bias {bias:+.4f} px, share {share:.3f}, code 3: {resets} of {valid.sum()}")
    assert ratio <= 0.5 and abs(bias) <= 0.02 and share >= 0.5 and resets <= 0.01 * valid.sum()


def test_hold_fills_what_was_seen_before():
    """sigma 0.3, dz 0.6; from frame 3 on a seeded 10 % of the pixels and a 10 x 10 block are NaN.  Of the last frame's holes with a
    true surface at least 70 % are held, with a median error <= 0.3 px and at most 5 % above 1 px; without hold they are all code 0.
    Measured with this restatement: 427 holes, 324 held (76 %), median 0.11 px, 8.3 % above 0.5 px, 1.2 % above 1 px."""
    poses, truth, frames = _sequence(0.3, 0.6, 1, holes=True)
    kw = dict(sigma0=0.3, gate=3.0, q=0.0, max_jump=1.0, min_disp=0.5, q_hold=0.05, max_var=4.0)
    D, V, A, code, _ = T.run_sequence(frames, T.SCENE_CAM, poses, hold=1, **kw)[-1]
    holes = np.isnan(frames[-1][0, 0]) & (truth[-1] > 0.5)
    held = holes & (code[0, 0] == 4)
    err = np.abs(D[0, 0][held].astype(np.float64) - truth[-1][held])
    print(f"holes {holes.sum()}, held {held.sum()}, median {np.median(err):.3f} px, > 0.5 px {(err > 0.5).mean():.3f}, > 1 px {(err > 1).mean():.3f}")
    assert held.sum() >= 0.7 * holes.sum() and np.median(err) <= 0.3 and (err > 1).mean() <= 0.05
    assert set(np.unique(code[0, 0][holes]).tolist()) <= {0, 4} and (A[0, 0][held] > 0).all() and (V[0, 0][held] <= 4.0).all()
    code0 = T.run_sequence(frames, T.SCENE_CAM, poses, hold=0, **kw)[-1][3]
    assert (code0[0, 0][holes] == 0).all()


def test_z_buffer_nearest_wins_then_the_larger_index():
    assert (np.diff(T.key_of(np.array([-1.0, -0.0, 0.0, 1e-3, 2.0, np.inf], F)).astype(np.int64)) > 0).all()
    assert (T.unkey(T.key_of(np.array([0.5, 7.25], F))) == np.array([0.5, 7.25], F)).all()
    # two previous pixels of equal disparity land on one hole: the larger source index is read back
    cam = np.array([[128.0, 128.0, 3.5, 0.0, 64.0]], F)
    prev = (np.full((1, 1, 1, 8), 8.0, F), np.full((1, 1, 1, 8), 0.25, F), np.array([1, 2, 3, 4, 5, 6, 7, 8], np.uint16).reshape(1, 1, 1, 8))
    m = np.full((1, 1, 1, 8), np.nan, F)
    back = T.relative(T.forward_pose(0, 0.0), T.forward_pose(1, -8.0))[None]        # the camera backs away: depth 8 -> 16, the row shrinks to half
    D, V, A, code, counts = T.step(m, cam, back, prev, hold=1, min_disp=0.5, max_var=4.0)
    assert code[0, 0, 0].tolist() == [0, 0, 4, 4, 4, 4, 0, 0] and counts[0].tolist() == [4, 0, 0, 0, 4]
    # u = (x - 3.5) / 2 + 3.5: sources 0..7 land on rint(1.75, 2.25, 2.75, 3.25, 3.75, 4.25, 4.75, 5.25) = 2, 2, 3, 3, 4, 4, 5, 5
    assert A[0, 0, 0].tolist() == [0, 0, 2, 4, 6, 8, 0, 0] and (D[0, 0, 0, 2:6] == F(4.0)).all()
    assert (V[0, 0, 0, 2:6] == (F(0.25) * (F(0.25) * F(0.25)) + F(0.0)) + F(0.05)).all()


# ---- host pieces ----
def test_pose_reader_round_trip_and_relative_pose(tmp_path):
    from lwsnet_amd import geometry
    rng = np.random.default_rng(3)
    poses = np.stack([T.forward_pose(k, 0.7, yaw=0.03, dx=0.1) for k in range(5)])
    path = tmp_path / "poses.txt"
    path.write_text("".join(" ".join(repr(float(v)) for v in p.reshape(12)) + "\n" for p in poses) + "\n")
    got = geometry.read_kitti_poses(str(path))
    assert got.dtype == np.float64 and got.shape == (5, 3, 4) and (got == poses).all()
    rel = geometry.relative_pose(poses[1], poses[3])
    assert rel.dtype == np.float32 and rel.shape == (2, 12) and (rel == T.relative(poses[1], poses[3])).all()
    a, b = (np.vstack([r.reshape(3, 4).astype(np.float64), [0, 0, 0, 1]]) for r in rel)
    assert np.abs(a @ b - np.eye(4)).max() <= 1e-6
    p = rng.normal(size=3)                                  # a world point seen from both cameras
    cam1, cam3 = (np.linalg.solve(np.vstack([poses[k], [0, 0, 0, 1]]), np.append(p, 1.0)) for k in (1, 3))
    assert np.abs(a @ cam1 - cam3).max() <= 1e-6
    for text, msg in (("1 2 3\n", "12 finite numbers"), ("a b\n", "not a line of numbers"), (" ".join(["nan"] * 12) + "\n", "12 finite numbers")):
        path.write_text(text)
        with pytest.raises(ValueError, match=msg):
            geometry.read_kitti_poses(str(path))
    with pytest.raises(ValueError, match="T_prev must be a finite 3x4"):
        geometry.relative_pose(np.eye(4), poses[0])


def _p(k, off=0):
    """Fake device pointers 1 GiB apart: never dereferenced, every call below is refused first."""
    return ctypes.c_void_p((1 << 40) + (k << 30) + off)


def test_temporal_step_rejects_bad_arguments(hip_lib):
    names = ("meas", "sigma", "mask", "cam", "pose", "Dp", "Vp", "Ap", "workspace", "D", "V", "A", "code", "counts")
    base = {name: _p(k) for k, name in enumerate(names)}
    INV = _lib.LWS_ERR_INVALID

    def call(B=1, H=8, W=16, sigma0=0.5, min_disp=1.0, sigma_min=0.05, gate=3.0, q=0.0, max_jump=1.0, hold=1, q_hold=0.05, max_var=4.0, **ptrs):
        a = {**base, **ptrs}
        return hip_lib.lws_temporal_step(a["meas"], a["sigma"], a["mask"], a["cam"], a["pose"], a["Dp"], a["Vp"], a["Ap"], B, H, W, sigma0, min_disp,
                                         sigma_min, gate, q, max_jump, hold, q_hold, max_var, a["workspace"], a["D"], a["V"], a["A"], a["code"],
                                         a["counts"], None)

    def at(name, off):
        return _p(names.index(name), off)

    w = b"temporal_step: "
    al = w + b"meas / sigma / cam / pose / Dp / Vp / D / V must be 4-byte, Ap / A 2-byte, counts / workspace 8-byte aligned"
    together = w + b"Dp, Vp and Ap must be given together (all three null: the first frame)"
    nan = float("nan")
    for kw, msg in [
        (dict(meas=None), w + b"meas and cam must not be null"), (dict(cam=None), w + b"meas and cam must not be null"),
        (dict(D=None), w + b"D, V, A and code must not be null"), (dict(V=None), w + b"D, V, A and code must not be null"),
        (dict(A=None), w + b"D, V, A and code must not be null"), (dict(code=None), w + b"D, V, A and code must not be null"),
        (dict(Dp=None), together), (dict(Vp=None), together), (dict(Ap=None), together), (dict(Dp=None, Vp=None), together),
        (dict(pose=None), w + b"a previous state needs pose"),
        (dict(B=0), w + b"bad shape B=0 H=8 W=16"), (dict(B=65536), w + b"bad shape B=65536 H=8 W=16"), (dict(W=0), w + b"bad shape B=1 H=8 W=0"),
        (dict(H=1 << 16, W=1 << 15), w + b"H*W = 65536x32768 must be < 2^31"),
        (dict(H=1, W=(1 << 24) + 1), w + b"H=1 W=16777217 exceed 16777216 (pixel coordinates are exact floats)"),
        (dict(hold=2), w + b"hold 2 (0 = off, 1 = hold what was seen before)"),
        (dict(workspace=None), w + b"hold needs a workspace (lws_temporal_workspace)"),
        (dict(meas=at("meas", 2)), al), (dict(Ap=at("Ap", 1)), al), (dict(A=at("A", 1)), al), (dict(counts=at("counts", 4)), al),
        (dict(workspace=at("workspace", 4)), al), (dict(pose=at("pose", 2)), al), (dict(V=at("V", 2)), al),
        (dict(sigma=None, sigma0=-1.0), w + b"sigma0 must be finite and >= 0 where sigma is null, got -1"),
        (dict(min_disp=0.0), w + b"min_disp must be finite and > 0, got 0"), (dict(sigma_min=0.0), w + b"sigma_min must be finite and > 0, got 0"),
        (dict(gate=0.0), w + b"gate must be finite and > 0, got 0"), (dict(gate=float("inf")), w + b"gate must be finite and > 0, got inf"),
        (dict(q=-1.0), w + b"q must be finite and >= 0, got -1"), (dict(max_jump=nan), w + b"max_jump must be >= 0 (+inf allowed), got nan"),
        (dict(max_jump=-1.0), w + b"max_jump must be >= 0 (+inf allowed), got -1"), (dict(q_hold=nan), w + b"q_hold must be finite and >= 0, got nan"),
        (dict(max_var=0.0), w + b"max_var must be > 0 (+inf allowed), got 0"),
        (dict(V=at("D", 4 * 128 - 4)), w + b"V and D overlap"), (dict(A=at("V", 0)), w + b"A and V overlap"), (dict(code=at("A", 2 * 128 - 1)), w + b"code and A overlap"),
        (dict(counts=at("code", 120)), w + b"counts and code overlap"), (dict(workspace=at("counts", 32)), w + b"workspace and counts overlap"),
        (dict(D=at("Dp", 0)), w + b"Dp and D overlap"), (dict(V=at("Vp", 508)), w + b"Vp and V overlap"), (dict(A=at("Ap", 0)), w + b"Ap and A overlap"),
        (dict(meas=at("D", 0)), w + b"meas and D overlap"), (dict(sigma=at("V", 0)), w + b"sigma and V overlap"), (dict(mask=at("code", 0)), w + b"mask and code overlap"),
        (dict(cam=at("workspace", 8 * 128 - 4)), w + b"cam and workspace overlap"), (dict(pose=at("counts", 36)), w + b"pose and counts overlap"),
    ]:
        assert call(**kw) == INV, kw
        assert hip_lib.lws_last_error() == msg, (kw, hip_lib.lws_last_error())
    # without hold the workspace is not looked at: the next refusal is about something else
    assert call(hold=0, workspace=at("D", 0), gate=0.0) == INV and hip_lib.lws_last_error() == w + b"gate must be finite and > 0, got 0"
    assert hip_lib.lws_temporal_workspace(2, 5, 7, 1) == 2 * 5 * 7 * 8 and hip_lib.lws_temporal_workspace(2, 5, 7, 0) == 0
    assert hip_lib.lws_temporal_workspace(0, 5, 7, 1) == INV and hip_lib.lws_last_error() == b"temporal_workspace: bad shape B=0 H=5 W=7"
    assert hip_lib.lws_temporal_workspace(1, 5, 7, 3) == INV


def test_ops_and_filter_validate_before_any_gpu_call():
    from lwsnet_amd import ops, temporal
    from lwsnet_amd.geometry import Camera
    cam = Camera(128.0, 128.0, 47.5, 20.0, 0.5)
    z = np.zeros((1, 1, 2, 2), F)
    with pytest.raises(ValueError, match="temporal_step needs cameras"):
        ops.temporal_step(z, None)
    with pytest.raises(ValueError, match="TemporalFilter needs cameras"):
        temporal.TemporalFilter(None)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.temporal_step(z, cam)
    bad = ((dict(min_disp=0.0), "min_disp must be finite and > 0"), (dict(sigma0=-1.0), "sigma0 must be finite and >= 0"), (dict(sigma_min=0.0), "sigma_min"),
           (dict(gate=0.0), "gate must be finite and > 0"), (dict(gate=float("nan")), "gate"), (dict(q=-0.5), "q must be finite and >= 0"),
           (dict(max_jump=-1.0), "max_jump must be >= 0"), (dict(max_jump=float("nan")), "max_jump"), (dict(hold=2), "hold must be False or True"),
           (dict(q_hold=float("inf")), "q_hold must be finite and >= 0"), (dict(max_var=0.0), "max_var must be > 0"))
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            ops.temporal_step(None, cam, **kw)
        with pytest.raises(ValueError, match=msg):
            temporal.TemporalFilter(cam, **kw)
    with pytest.raises(ValueError, match="prev must be the"):
        ops.temporal_step(None, cam, pose=IDENT[0], prev=(z, z))
    with pytest.raises(ValueError, match="a previous state needs pose"):
        ops.temporal_step(None, cam, prev=(z, z, z))
    for pose, shape in ((np.zeros((3, 4)), r"\(3, 4\)"), (np.zeros((2, 2, 12)), r"\(2, 2, 12\)"), (np.full((2, 12), np.nan), r"\(1, 2, 12\)")):
        with pytest.raises(ValueError, match="pose must be a finite float32 .* got shape " + shape):
            ops.temporal_pose_rows(pose, 1)
    assert ops.temporal_pose_rows(IDENT[0], 3).shape == (3, 2, 12)
    f = temporal.TemporalFilter(cam, hold=True)
    assert f.state is None and f.frames == 0 and f.params["hold"] is True
    with pytest.raises(ValueError, match="there is no previous frame"):
        f.step(z, pose=IDENT[0])
    f.reset()
    assert ops.TemporalResult._fields == ("disp", "var", "age", "code", "counts")
    assert ops._temporal_args(0.5, 1.0, 0.05, 3.0, 0.0, float("inf"), True, 0.05, float("inf")) == (0.5, 1.0, 0.05, 3.0, 0.0, float("inf"), 1, 0.05,
                                                                                                    float("inf"))


# ---- the inference CLI ----
NEW_FLAGS = ("temporal", "poses", "temporal_gate", "temporal_q", "temporal_sigma", "temporal_hold", "save_temporal")


def test_temporal_flags_default_off(tmp_path):
    from lwsnet_amd import inference
    p = inference.build_parser()
    a = p.parse_args([])
    assert not any(hasattr(a, name) for name in NEW_FLAGS)                      # the namespace of a line without them
    with_flags = vars(p.parse_args(["--temporal", "--poses", "x", "--temporal_gate", "2", "--temporal_q", "0.1", "--temporal_sigma", "net",
                                    "--temporal_hold", "--save_temporal"]))
    assert {k: v for k, v in with_flags.items() if k not in NEW_FLAGS} == vars(a)
    inference.check_geometry_arguments(p, a)
    inference.check_temporal_arguments(p, a)
    assert tuple(getattr(a, f) for f in NEW_FLAGS) == (False, None, 3.0, 0.0, "0.5", False, False)
    seq, poses = sequence_dir(tmp_path, 3), poses_file(tmp_path / "poses.txt", 3)
    a = p.parse_args(seq + ["--save_temporal", "--poses", poses, "--temporal_sigma", "net", "--temporal_hold"] + CAMERA)
    inference.check_occ_arguments(p, a)
    inference.check_geometry_arguments(p, a)
    inference.check_temporal_arguments(p, a)
    assert a.temporal and a.save_temporal and a.temporal_hold and inference.temporal_sigma(a) is None and a.temporal_gate == 3.0
    a.temporal_sigma = "0.25"
    assert inference.temporal_sigma(a) == 0.25


def test_cli_refuses_temporal_without_what_it_needs(tmp_path, capsys):
    seq, poses, enough = sequence_dir(tmp_path, 4), poses_file(tmp_path / "poses.txt", 3), poses_file(tmp_path / "enough.txt", 4)
    ok = seq + ["--temporal", "--poses", enough] + CAMERA
    assert _cli_refused(seq + ["--temporal"] + CAMERA, capsys).endswith(": error: --temporal needs --poses PATH, the camera-to-world pose of every pair\n")
    assert _cli_refused(seq + ["--temporal", "--poses", enough], capsys).endswith(
        ": error: --temporal and --save_temporal need a camera: --calib PATH or --camera FX FY CX CY BASELINE\n")
    assert _cli_refused(ok + ["--workers", "2"], capsys).endswith(": error: --temporal / --save_temporal run in the sequential mode only: use --workers 0\n")
    assert _cli_refused(seq + ["--temporal", "--poses", poses] + CAMERA, capsys).endswith(
        f": error: --poses: {poses} holds 3 poses for 4 pairs (line i belongs to the i-th pair in sorted order)\n")
    assert _cli_refused(seq + ["--temporal", "--poses", str(tmp_path / "none.txt")] + CAMERA, capsys).count("--poses: cannot read") == 1
    assert _cli_refused(seq + ["--temporal_hold", "--poses", enough] + CAMERA, capsys).endswith(
        ": error: --poses, --temporal_gate, --temporal_q, --temporal_sigma and --temporal_hold need --temporal\n")
    assert _cli_refused(["--left_img", str(tmp_path / "left_test.png"), "--temporal", "--poses", enough] + CAMERA, capsys).endswith(
        ": error: --temporal fuses a sequence: use directory mode (--img_path), not --left_img\n")
    assert _cli_refused(ok + ["--temporal_sigma", "wide"], capsys).endswith(
        ": error: --temporal_sigma must be a finite number of pixels >= 0 or `net`, got wide\n")
    assert _cli_refused(ok + ["--temporal_sigma", "net", "--lr_check", "1"], capsys).endswith(
        ": error: --temporal_sigma net uses the network's own sigma and does not combine with --lr_check or --occ_check\n")
    assert _cli_refused(ok + ["--temporal_gate", "0"], capsys).endswith(": error: --temporal_gate must be finite and > 0, got 0.0\n")
    assert _cli_refused(ok + ["--temporal_q", "-1"], capsys).endswith(": error: --temporal_q must be finite and >= 0, got -1.0\n")
    assert not os.path.exists(tmp_path / "out")             # refused before the output folder is touched


def test_temporal_file_helpers():
    from lwsnet_amd import outputs
    code = np.array([[0, 1, 2], [3, 4, 2]], np.uint8)
    rgb = outputs.temporal_to_rgb(code)
    assert rgb.dtype == np.uint8 and rgb.shape == (2, 3, 3) and rgb[0, 0].tolist() == [0, 0, 0] and (rgb[0, 2] == rgb[1, 2]).all()
    assert len({tuple(c) for c in outputs.TEMPORAL_COLOURS.tolist()}) == 5 == len(outputs.TEMPORAL_CODES)
    assert outputs.TEMPORAL_CODES == ("nothing", "new", "fused", "reset", "held")


def test_pose_source_counts_pairs_not_processed_frames():
    """The CLI's pose source over a poses file of five lines, pairs 1 and 3 skipped: the filter is handed nothing on the first frame,
    then geometry.relative_pose of the two pairs it fuses, bit for bit; the world pose of pair 4 is line 4, not the third line."""
    from types import SimpleNamespace
    from lwsnet_amd import geometry, sequence
    poses = np.stack([T.forward_pose(k, 0.7, yaw=0.03, dx=0.1) for k in range(5)])
    src = sequence.PoseSource(5, poses)
    handed = {}
    for index in (0, 2, 4):
        src.frame(index)
        handed[index] = src.relative(SimpleNamespace(frame=SimpleNamespace(path=f"{index}.png"), ego=None), None)
        assert (src.world() == poses[index]).all()
    assert handed[0] is None and (src.world() != poses[2]).any()
    for prev, index in ((0, 2), (2, 4)):
        want = geometry.relative_pose(poses[prev], poses[index])
        assert handed[index].dtype == want.dtype == np.float32 and handed[index].tobytes() == want.tobytes()
        assert handed[index].tobytes() != geometry.relative_pose(poses[index - 1], poses[index]).tobytes()
