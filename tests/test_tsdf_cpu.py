"""The TSDF volume without a GPU: what the numpy restatement (tests/tsdf_reference.py) gives on the exact wall and on the road
scene, that the cases of tests/test_gpu_tsdf.py reach every branch of the rules, the argument checks of the C entry points, of
lwsnet_amd.ops.tsdf_* and of TsdfVolume, and the inference CLI's flags."""
import ctypes
import os

import numpy as np
import pytest

import mesh_reference as M
import temporal_reference as TR
import tsdf_reference as R
from cli_helpers import CAMERA, cli_refused as _cli_refused, poses_file as _poses_file, sequence_dir as _sequence_dir
from lwsnet_amd import _lib

F = np.float32
CAM = np.array([TR.SCENE_CAM], F)

# the exact wall: d = 7.5 px at fb = 60 is z = 8 m; origin, voxel, z_near and step are multiples of 0.25
WALL = dict(origin=(-6.0, -3.0, 0.0), vs=0.25, dims=(48, 20, 48), mu0=0.75, hits=3780)
# the road scene: five poses into a 0.125 m volume, ray-cast from the third.  p95 and max of |ray-cast - truth| in px over the scored
# pixels that hit are what tsdf_reference gives (measured on the CPU, asserted below); the GPU test allows 1.5 x these.
SCENE = dict(origin=(-8.0, -3.0, 0.0), vs=0.125, dims=(128, 40, 128), mu0=0.25, poses=[TR.forward_pose(k, 0.5, yaw=0.01) for k in range(5)],
             scored=2400, hits=2361, hits_without_normals=1613, p95=0.002639, max=0.193126)
_CACHE = {}


def wall_volume(frames):
    """The wall integrated `frames` times: T, Wt, updated of the last frame, the view and the points."""
    if ("wall", frames) not in _CACHE:
        shape = WALL["dims"][::-1]
        T, Wt = np.zeros(shape, F), np.zeros(shape, F)
        d = np.full((1, 1, 48, 96), 7.5, F)
        pose = R.pose_block(TR.IDENTITY)[None]
        for _ in range(frames):
            T, Wt, _, upd = R.integrate(T, Wt, None, WALL["origin"], WALL["vs"], d, CAM, pose, mu0=WALL["mu0"])
        view = R.raycast(T, Wt, WALL["origin"], WALL["vs"], CAM, pose, 48, 96, 1.0, 0.25, 60)
        xyz, rgba, nrm, _, _ = R.points(T, Wt, None, WALL["origin"], WALL["vs"])
        _CACHE["wall", frames] = dict(T=T, Wt=Wt, updated=int(upd[0]), view=view, points=(R.records(xyz, rgba), nrm))
    return _CACHE["wall", frames]


def scene_volume(use_normals):
    """The road scene integrated from its five poses, with the point-to-plane distance or without, and the view from the third."""
    if ("scene", use_normals) not in _CACHE:
        shape = SCENE["dims"][::-1]
        T, Wt = np.zeros(shape, F), np.zeros(shape, F)
        frames, normals = [], []
        for p in SCENE["poses"]:
            d = TR.render(p).astype(F)[None, None]
            n = M.surface_normals(d, None, CAM, 1.0, np.inf, 1.0)[0] if use_normals else None
            T, Wt, _, _ = R.integrate(T, Wt, None, SCENE["origin"], SCENE["vs"], d, CAM, R.pose_block(p)[None], normals=n, mu0=SCENE["mu0"], mu_d=0.0, wmode=0)
            frames.append(d)
            normals.append(n)
        view = R.raycast(T, Wt, SCENE["origin"], SCENE["vs"], CAM, R.pose_block(SCENE["poses"][2])[None], 48, 96, 1.0, 0.0625, 240)
        _CACHE["scene", use_normals] = dict(T=T, Wt=Wt, frames=frames, normals=normals, view=view)
    return _CACHE["scene", use_normals]


# ---- the reference's own checks ----
def test_the_integrate_cases_reach_every_branch():
    total = {}
    for c in R.integrate_cases():
        for k, v in c["stats"].items():
            total[k] = total.get(k, 0) + v
    print("voxels per branch over all cases:", total)
    assert sorted(total) == sorted(R.BRANCHES) and all(total[k] > 0 for k in R.BRANCHES), total
    cases = R.integrate_cases()
    for key in ("sigma", "mask", "normals", "rgb"):                 # every optional input given and not given
        assert {c[key] is None for c in cases} == {True, False}, key
    assert {c["kw"]["wmode"] for c in cases} == {0, 1} and any(np.isfinite(c["kw"]["w_max"]) for c in cases)
    assert all((c["W0"] > 0).any() and np.isnan(c["T0"][c["W0"] == 0]).all() for c in cases)      # state, poisoned where unobserved
    flat = np.concatenate([c["disp"].reshape(-1) for c in cases])
    assert np.isnan(flat).any() and (flat == np.inf).any() and (flat == -np.inf).any() and (flat == 0).any() and (flat < 0).any()


def test_the_raycast_cases_reach_every_ending():
    T, Wt, origin, vs = R.crafted_volume()
    cam, pose = R.raycast_views()
    total, per = {}, []
    for kw in R.RAYCASTS:
        st = {}
        R.raycast(T, Wt, origin, vs, cam, pose, 24, 40, stats=st, **kw)
        per.append(st)
        for k, v in st.items():
            total[k] = total.get(k, 0) + v
    print(per)
    assert all(v > 0 for v in total.values()) and len(total) == 8, total
    assert per[1]["first_interval"] > 0 and per[1]["exhausted"] > 0             # three steps: a hit in the first interval, or none
    assert 0 < per[2]["hit"] < per[0]["hit"]                                    # w_min = 2 blinds the taps of weight 1
    assert per[3]["never_inside"] > 0 and per[0]["back_face"] > 0 and per[0]["normal_unknown"] > 0


@pytest.mark.parametrize("dims", [(5, 3, 2), (33, 4, 5), (65, 7, 9), (300, 3, 2)])
def test_the_points_cases_cross_on_every_axis_both_ways(dims):
    T, Wt, C, origin, vs = R.points_volume(dims, 1)
    xyz, rgba, nrm, e, up = R.points(T, Wt, C, origin, vs)
    assert len(xyz) > 0 and np.isfinite(xyz).all()
    if dims != (5, 3, 2):
        for axis in range(3):
            assert (up[e == axis]).any() and (~up[e == axis]).any(), axis
        assert (nrm[:, :3] != 0).any() or dims[1] < 4
    assert ((T == 0) & (Wt > 0)).any()                              # Tb == 0 exactly: a crossing from above, none from below
    lo = np.array(origin, F)
    assert (xyz >= lo).all() and (xyz <= lo + F(vs) * (np.array(dims, F) - 1)).all()


@pytest.mark.parametrize("dims", list(R.POINTS_CHUNKED))
def test_the_chunked_points_cases_cross_on_both_sides_of_every_carry(dims):
    """The x-row of a crossing on an x-edge can be read off its y and z, which are voxel centres: rows on both sides of every
    chunk boundary of the scan hold records, so a wrong carry moves records that the bit-exact comparison sees."""
    T, Wt, C, origin, vs = R.points_volume(dims, 1)
    xyz, rgba, nrm, e, up = R.points(T, Wt, C, origin, vs)
    assert len(xyz) == R.POINTS_CHUNKED[dims]
    xs, ys, zs = R.centres(origin, vs, dims)
    on_x = xyz[e == 0]
    iy, iz = np.searchsorted(ys, on_x[:, 1]), np.searchsorted(zs, on_x[:, 2])
    assert (ys[iy] == on_x[:, 1]).all() and (zs[iz] == on_x[:, 2]).all()
    row, rows = iz * dims[1] + iy, dims[1] * dims[2]
    for edge in range(256, rows + 256, 256):                 # the chunk [edge - 256, edge) and, if any row follows it, what follows
        assert ((row >= edge - 256) & (row < edge)).any(), edge
        assert (row >= edge).any() == (rows > edge), edge
    assert (rows - 1) // 256 == {(6, 16, 16): 0, (5, 3, 86): 1, (9, 20, 26): 2}[dims]      # the carries of the scan


def test_the_exact_wall():
    for frames in (1, 5):
        w = wall_volume(frames)
        r, wt, n = w["view"]
        hit = r > 0
        assert hit.sum() == WALL["hits"] and (r[hit] == F(7.5)).all() and (wt[hit] == F(frames)).all()
        nh = np.moveaxis(n[0], 0, -1)[hit[0, 0]]
        assert ((nh == np.array([0, 0, -1], F)).all(axis=1) | (nh == 0).all(axis=1)).all() and (nh[:, 2] == -1).any()
        rec, nrm = w["points"]
        assert len(rec) > 0 and (rec[:, :12].copy().view(F).reshape(-1, 3)[:, 2] == F(8.0)).all() and (rec[:, 12:] == 255).all()
        with_n = (nrm != 0).any(axis=1)
        assert with_n.any() and (nrm[with_n] == np.array([0, 0, -1, 0], F)).all()


def test_the_road_scene_and_why_the_distance_is_point_to_plane():
    truth = TR.render(SCENE["poses"][2])
    scored = truth >= 4.5
    assert scored.sum() == SCENE["scored"]
    hits = {}
    for use_normals in (True, False):
        r = scene_volume(use_normals)["view"][0][0, 0]
        hit = r > 0
        assert not (hit & (truth == 0)).any()
        hits[use_normals] = int((scored & hit).sum())
        err = np.abs(r[scored & hit].astype(np.float64) - truth[scored & hit])
        print(f"normals={use_normals}: {hits[use_normals]} of {int(scored.sum())} hit, p95 {np.percentile(err, 95):.6f} max {err.max():.6f} px")
        if use_normals:
            assert hits[True] >= 0.95 * scored.sum()
            assert abs(np.percentile(err, 95) - SCENE["p95"]) < 5e-7 and abs(err.max() - SCENE["max"]) < 5e-7      # the measured figures
    assert hits == {True: SCENE["hits"], False: SCENE["hits_without_normals"]} and hits[False] < hits[True]


def test_a_cleared_volume_forgets_what_it_held():
    """Zeroing Wt alone clears a volume: T and C poisoned where Wt == 0 give the same result as zeros there."""
    c = R.integrate_case((33, 4, 5), (5, 7), 1)
    assert c["C0"] is not None and c["stats"]["colour_cleared"] > 0 and c["stats"]["first_touch"] > 0
    unseen = c["W0"] == 0
    T1, C1 = np.where(unseen, F(0), c["T0"]), c["C0"].copy()
    C1[unseen] = 0
    got = R.integrate(T1, c["W0"], C1, c["origin"], c["vs"], c["disp"], c["cam"], c["pose"], c["sigma"], c["mask"], c["normals"], c["rgb"], **c["kw"])
    taken = got[1] != c["W0"]
    assert taken.any() and np.array_equal(got[0][taken], c["want"][0][taken]) and np.array_equal(got[1], c["want"][1])
    assert np.array_equal(got[2][taken], c["want"][2][taken])


# ---- the argument checks of the C entry points ----
def _p(k, off=0):
    """Fake device pointers 64 GiB apart: never dereferenced, every call below is refused first."""
    return ctypes.c_void_p((1 << 44) + (k << 36) + off)


def _refused(hip_lib, rc, msg, kw):
    assert rc == _lib.LWS_ERR_INVALID, kw
    assert hip_lib.lws_last_error() == msg, (kw, hip_lib.lws_last_error())


def test_integrate_rejects_bad_arguments(hip_lib):
    names = ("disp", "sigma", "mask", "normals", "rgb", "cam", "pose", "T", "Wt", "C", "updated")
    base = {name: _p(k) for k, name in enumerate(names)}

    def call(B=2, H=8, W=16, G=(8, 4, 3), o=(0.0, 0.0, 0.0), vs=0.25, sigma0=0.5, min_disp=1.0, max_depth=float("inf"), mu0=0.5, mu_d=0.0,
             sigma_min=0.05, wmode=0, w_max=float("inf"), **ptrs):
        a = {**base, **ptrs}
        return hip_lib.lws_tsdf_integrate(a["disp"], a["sigma"], a["mask"], a["normals"], a["rgb"], a["cam"], a["pose"], B, H, W, a["T"], a["Wt"], a["C"],
                                          *G, *o, vs, sigma0, min_disp, max_depth, mu0, mu_d, sigma_min, wmode, w_max, a["updated"], None)

    def at(name, off):
        return _p(names.index(name), off)

    w = b"tsdf_integrate: "
    al = w + b"disp / sigma / normals / C must be 4-byte, updated 8-byte aligned"
    pair = w + b"rgb and C must be given together (rgb colours C; both null: no colour)"
    nan, inf = float("nan"), float("inf")
    for kw, msg in [
        (dict(disp=None), w + b"disp is null"), (dict(cam=None), w + b"cam and pose must not be null"), (dict(pose=None), w + b"cam and pose must not be null"),
        (dict(T=None), w + b"T and Wt must not be null"), (dict(Wt=None), w + b"T and Wt must not be null"),
        (dict(B=0), w + b"bad shape B=0 H=8 W=16"), (dict(B=65536), w + b"bad shape B=65536 H=8 W=16"), (dict(W=0), w + b"bad shape B=2 H=8 W=0"),
        (dict(H=1 << 16, W=1 << 15), w + b"H*W = 65536x32768 must be < 2^31"),
        (dict(H=1, W=(1 << 24) + 1), w + b"H=1 W=16777217 exceed 16777216 (pixel coordinates are exact floats)"),
        (dict(G=(1, 4, 3)), w + b"bad volume Gx=1 Gy=4 Gz=3 (each in 2..4096)"), (dict(G=(8, 4097, 3)), w + b"bad volume Gx=8 Gy=4097 Gz=3 (each in 2..4096)"),
        (dict(G=(8, 4, 0)), w + b"bad volume Gx=8 Gy=4 Gz=0 (each in 2..4096)"), (dict(G=(2048, 1024, 1024)), w + b"Gx*Gy*Gz = 2048x1024x1024 must be < 2^31"),
        (dict(o=(nan, 0.0, 0.0)), w + b"the origin (nan, 0, 0) must be finite"), (dict(o=(0.0, 0.0, -inf)), w + b"the origin (0, 0, -inf) must be finite"),
        (dict(vs=0.0), w + b"vs must be finite and > 0, got 0"), (dict(vs=inf), w + b"vs must be finite and > 0, got inf"),
        (dict(rgb=None), pair), (dict(C=None), pair),
        (dict(disp=at("disp", 2)), al), (dict(sigma=at("sigma", 1)), al), (dict(normals=at("normals", 2)), al), (dict(C=at("C", 2)), al),
        (dict(updated=at("updated", 4)), al), (dict(T=at("T", 2)), w + b"T / Wt must be 4-byte aligned"), (dict(cam=at("cam", 2)), w + b"cam / pose must be 4-byte aligned"),
        (dict(min_disp=0.0), w + b"min_disp must be finite and > 0, got 0"), (dict(max_depth=0.0), w + b"max_depth must be > 0 (+inf allowed), got 0"),
        (dict(max_depth=nan), w + b"max_depth must be > 0 (+inf allowed), got nan"), (dict(mu0=0.0), w + b"mu0 must be finite and > 0, got 0"),
        (dict(mu0=inf), w + b"mu0 must be finite and > 0, got inf"), (dict(mu_d=-1.0), w + b"mu_d must be finite and >= 0, got -1"),
        (dict(sigma=None, sigma0=-0.5), w + b"sigma0 must be finite and >= 0 where sigma is null, got -0.5"),
        (dict(sigma_min=0.0), w + b"sigma_min must be finite and > 0, got 0"), (dict(wmode=2), w + b"wmode 2 (0 = unit weights, 1 = 1 / sigma_z^2)"),
        (dict(w_max=0.0), w + b"w_max must be > 0 (+inf allowed), got 0"), (dict(w_max=nan), w + b"w_max must be > 0 (+inf allowed), got nan"),
        (dict(Wt=at("T", 4 * 96 - 4)), w + b"Wt and T overlap"), (dict(C=at("Wt", 0)), w + b"C and Wt overlap"), (dict(updated=at("C", 4 * 96 - 8)), w + b"updated and C overlap"),
        (dict(disp=at("T", 0)), w + b"disp and T overlap"), (dict(sigma=at("Wt", 8)), w + b"sigma and Wt overlap"), (dict(mask=at("C", 1)), w + b"mask and C overlap"),
        (dict(normals=at("updated", 0)), w + b"normals and updated overlap"), (dict(rgb=at("T", 5)), w + b"rgb and T overlap"),
        (dict(cam=at("updated", 12)), w + b"cam and updated overlap"), (dict(pose=at("Wt", 4 * 95)), w + b"pose and Wt overlap"),
    ]:
        _refused(hip_lib, call(**kw), msg, kw)
    # the optional pointers may be null, and a sigma0 that is not read may be anything: the next refusal is about something else
    _refused(hip_lib, call(sigma=None, mask=None, normals=None, rgb=None, C=None, updated=None, wmode=-1), w + b"wmode -1 (0 = unit weights, 1 = 1 / sigma_z^2)", {})
    _refused(hip_lib, call(sigma0=nan, wmode=3), w + b"wmode 3 (0 = unit weights, 1 = 1 / sigma_z^2)", {})
    _refused(hip_lib, call(sigma=at("disp", 0), w_max=-1.0), w + b"w_max must be > 0 (+inf allowed), got -1", {})        # inputs may share memory


def test_raycast_rejects_bad_arguments(hip_lib):
    names = ("T", "Wt", "cam", "pose", "disp", "weight", "normals")
    base = {name: _p(k) for k, name in enumerate(names)}

    def call(G=(8, 4, 3), o=(0.0, 0.0, 0.0), vs=0.25, B=2, H=8, W=16, z_near=0.5, step=0.1, nsteps=10, w_min=0.0, **ptrs):
        a = {**base, **ptrs}
        return hip_lib.lws_tsdf_raycast(a["T"], a["Wt"], *G, *o, vs, a["cam"], a["pose"], B, H, W, z_near, step, nsteps, w_min, a["disp"], a["weight"],
                                        a["normals"], None)

    def at(name, off):
        return _p(names.index(name), off)

    w = b"tsdf_raycast: "
    nan, inf = float("nan"), float("inf")
    for kw, msg in [
        (dict(T=None), w + b"T and Wt must not be null"), (dict(cam=None), w + b"cam and pose must not be null"), (dict(disp=None), w + b"disp is null"),
        (dict(G=(8, 1, 3)), w + b"bad volume Gx=8 Gy=1 Gz=3 (each in 2..4096)"), (dict(vs=nan), w + b"vs must be finite and > 0, got nan"),
        (dict(B=0), w + b"bad shape B=0 H=8 W=16"), (dict(H=0), w + b"bad shape B=2 H=0 W=16"),
        (dict(weight=at("weight", 2)), w + b"disp / weight / normals must be 4-byte aligned"), (dict(Wt=at("Wt", 1)), w + b"T / Wt must be 4-byte aligned"),
        (dict(z_near=0.0), w + b"z_near must be finite and > 0, got 0"), (dict(z_near=inf), w + b"z_near must be finite and > 0, got inf"),
        (dict(step=0.0), w + b"step must be finite and > 0, got 0"), (dict(step=nan), w + b"step must be finite and > 0, got nan"),
        (dict(nsteps=1), w + b"nsteps 1 outside 2..65535"), (dict(nsteps=65536), w + b"nsteps 65536 outside 2..65535"),
        (dict(w_min=-1.0), w + b"w_min must be finite and >= 0, got -1"), (dict(w_min=inf), w + b"w_min must be finite and >= 0, got inf"),
        (dict(weight=at("disp", 4 * 256 - 4)), w + b"weight and disp overlap"), (dict(normals=at("weight", 0)), w + b"normals and weight overlap"),
        (dict(T=at("disp", 0)), w + b"T and disp overlap"), (dict(Wt=at("normals", 12 * 256 - 4)), w + b"Wt and normals overlap"),
        (dict(cam=at("weight", 8)), w + b"cam and weight overlap"), (dict(pose=at("disp", 0)), w + b"pose and disp overlap"),
    ]:
        _refused(hip_lib, call(**kw), msg, kw)
    _refused(hip_lib, call(weight=None, normals=None, nsteps=0), w + b"nsteps 0 outside 2..65535", {})
    _refused(hip_lib, call(Wt=at("T", 0), nsteps=0), w + b"nsteps 0 outside 2..65535", {})          # inputs may share memory


def test_points_rejects_bad_arguments(hip_lib):
    names = ("T", "Wt", "C", "workspace", "points", "vnormals", "counts")
    base = {name: _p(k) for k, name in enumerate(names)}

    def call(G=(8, 4, 3), o=(0.0, 0.0, 0.0), vs=0.25, w_min=0.0, max_points=100, **ptrs):
        a = {**base, **ptrs}
        return hip_lib.lws_tsdf_points(a["T"], a["Wt"], a["C"], *G, *o, vs, w_min, max_points, a["workspace"], a["points"], a["vnormals"], a["counts"], None)

    def at(name, off):
        return _p(names.index(name), off)

    w = b"tsdf_points: "
    null = w + b"workspace, points and counts must not be null"
    al = w + b"C must be 4-byte, workspace / counts 8-byte, points / vnormals 16-byte aligned"
    for kw, msg in [
        (dict(Wt=None), w + b"T and Wt must not be null"), (dict(workspace=None), null), (dict(points=None), null), (dict(counts=None), null),
        (dict(G=(4097, 4, 3)), w + b"bad volume Gx=4097 Gy=4 Gz=3 (each in 2..4096)"), (dict(vs=-1.0), w + b"vs must be finite and > 0, got -1"),
        (dict(w_min=float("nan")), w + b"w_min must be finite and >= 0, got nan"),
        (dict(max_points=0), w + b"max_points 0 outside 1 .. 2^31 - 1"), (dict(max_points=1 << 31), w + b"max_points 2147483648 outside 1 .. 2^31 - 1"),
        (dict(C=at("C", 2)), al), (dict(workspace=at("workspace", 4)), al), (dict(points=at("points", 8)), al), (dict(vnormals=at("vnormals", 4)), al),
        (dict(counts=at("counts", 4)), al),
        (dict(points=at("workspace", 240)), w + b"points and workspace overlap"), (dict(vnormals=at("points", 1600 - 16)), w + b"vnormals and points overlap"),
        (dict(counts=at("vnormals", 8)), w + b"counts and vnormals overlap"), (dict(T=at("points", 0)), w + b"T and points overlap"),
        (dict(Wt=at("counts", 4)), w + b"Wt and counts overlap"), (dict(C=at("workspace", 0)), w + b"C and workspace overlap"),
    ]:
        _refused(hip_lib, call(**kw), msg, kw)
    _refused(hip_lib, call(C=None, vnormals=None, max_points=-5), w + b"max_points -5 outside 1 .. 2^31 - 1", {})
    ws = hip_lib.lws_tsdf_points_workspace
    assert ws(4, 3) == 256 and ws(40, 128) == 8 * 40 * 128 and ws(33, 3) == 1024
    assert ws(1, 3) == _lib.LWS_ERR_INVALID and hip_lib.lws_last_error() == b"tsdf_points_workspace: bad volume Gy=1 Gz=3 (each in 2..4096)"
    assert ws(4, 4097) == _lib.LWS_ERR_INVALID


# ---- the host-side checks ----
def test_ops_and_the_volume_validate_before_any_gpu_call():
    import torch
    from lwsnet_amd import ops, tsdf
    from lwsnet_amd.geometry import Camera
    cam = Camera(120.0, 120.0, 47.5, 20.0, 0.5)
    T = torch.zeros((3, 4, 8))
    d = torch.zeros((1, 1, 4, 6))
    pose = ops.tsdf_pose_rows(TR.IDENTITY, 1)
    assert pose.shape == (1, 2, 12) and pose.dtype == np.float32 and np.array_equal(pose[0], R.pose_block(TR.IDENTITY))
    p3 = ops.tsdf_pose_rows(np.stack(SCENE["poses"][:3]), 3)
    assert np.array_equal(p3, np.stack([R.pose_block(p) for p in SCENE["poses"][:3]]))
    for bad in (np.zeros((4, 4)), np.zeros((2, 3, 4)), np.full((3, 4), np.nan)):
        with pytest.raises(ValueError, match="poses must be finite camera-to-world"):
            ops.tsdf_pose_rows(bad, 1)
    for args, msg in ((((0, 0), 0.25, (8, 4, 3)), "origin must be three finite numbers"),
                      (((0, 0, float("nan")), 0.25, (8, 4, 3)), "origin must be three finite numbers"), (((0, 0, 0), 0.0, (8, 4, 3)), "voxel must be finite and > 0"),
                      (((0, 0, 0), float("inf"), (8, 4, 3)), "voxel must be finite and > 0"), (((0, 0, 0), 0.25, (8, 4)), r"dims must be \(Gx, Gy, Gz\)"),
                      (((0, 0, 0), 0.25, (1, 4, 3)), r"dims\[0\] must be an integer in 2 .. 4096"), (((0, 0, 0), 0.25, (8, 4.5, 3)), r"dims\[1\] must be an integer"),
                      (((0, 0, 0), 0.25, (8, 4, 4097)), r"dims\[2\] must be an integer in 2 .. 4096"), (((0, 0, 0), 0.25, (2048, 1024, 1024)), "fewer than 2\\^31 voxels")):
        with pytest.raises(ValueError, match=msg):
            ops.tsdf_volume_args(*args)
    assert ops.tsdf_volume_args((-1, 2.5, 0), 0.125, (8, 4, 3)) == (8, 4, 3, -1.0, 2.5, 0.0, 0.125)
    scalars = ((dict(min_disp=0.0), "min_disp must be finite and > 0"), (dict(max_depth=0.0), "max_depth must be > 0"), (dict(max_depth=float("nan")), "max_depth"),
               (dict(mu0=0.0), "mu0 must be finite and > 0"), (dict(mu0=float("inf")), "mu0"), (dict(mu_d=-1.0), "mu_d must be finite and >= 0"),
               (dict(sigma0=-1.0), "sigma0 must be finite and >= 0"), (dict(sigma_min=0.0), "sigma_min must be finite and > 0"),
               (dict(weight="both"), "weight must be one of"), (dict(w_max=0.0), "w_max must be > 0"), (dict(w_max=float("nan")), "w_max"))
    for kw, msg in scalars:
        with pytest.raises(ValueError, match=msg):
            ops.tsdf_integrate(T, T, (0, 0, 0), 0.25, d, cam, pose, **kw)
        with pytest.raises(ValueError, match=msg):
            tsdf.TsdfVolume((0, 0, 0), 0.25, (8, 4, 3), **{"mu0": 0.5, **kw})
    with pytest.raises(ValueError, match="tsdf_integrate needs cameras"):
        ops.tsdf_integrate(T, T, (0, 0, 0), 0.25, d, None, pose)
    with pytest.raises(ValueError, match="voxel must be finite and > 0"):
        ops.tsdf_integrate(T, T, (0, 0, 0), -1.0, d, cam, pose)
    with pytest.raises(ValueError, match="dims must be"):
        ops.tsdf_integrate(None, None, (0, 0, 0), 0.25, d, cam, pose)
    for call in (lambda: ops.tsdf_integrate(T, T, (0, 0, 0), 0.25, d, cam, pose), lambda: ops.tsdf_raycast(T, T, (0, 0, 0), 0.25, cam, pose, 4, 6),
                 lambda: ops.tsdf_points(T, T, (0, 0, 0), 0.25, 16), lambda: tsdf.TsdfVolume((0, 0, 0), 0.25, (8, 4, 3), mu0=0.5, device="cpu")):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    for kw, msg in ((dict(max_points=0), "max_points must be an integer in 1"), (dict(max_points=1 << 31), "max_points"), (dict(max_points=2.5), "max_points"),
                    (dict(max_points=4, w_min=-1.0), "w_min must be finite and >= 0")):
        with pytest.raises(ValueError, match=msg):
            ops.tsdf_points(T, T, (0, 0, 0), 0.25, **kw)
    assert ops.TSDF_WEIGHTS == {"unit": 0, "sigma": 1} and tsdf.volume_bytes((128, 40, 128)) == 8 * 128 * 40 * 128
    assert tsdf.volume_bytes((8, 4, 3), colour=True) == 12 * 96
    assert ops.TsdfView._fields == ("disp", "weight", "normals") and ops.TsdfPoints._fields == ("points", "vnormals", "counts")


# ---- the inference CLI ----
NEW_FLAGS = ("tsdf", "tsdf_voxel", "tsdf_extent", "tsdf_trunc", "tsdf_trunc_px", "tsdf_weight", "tsdf_sdf", "save_tsdf_ply", "save_tsdf")


def test_tsdf_flags_default_off(tmp_path):
    from lwsnet_amd import inference
    assert tuple(inference.TSDF_DEFAULTS) == NEW_FLAGS
    p = inference.build_parser()
    a = p.parse_args([])
    assert not any(hasattr(a, name) for name in NEW_FLAGS)                      # the namespace of a line without them
    with_flags = vars(p.parse_args(["--tsdf", "--tsdf_voxel", "0.5", "--tsdf_extent", "-4", "4", "-2", "2", "0", "16", "--tsdf_trunc", "1", "--tsdf_trunc_px", "0.5",
                                    "--tsdf_weight", "sigma", "--tsdf_sdf", "ray", "--save_tsdf_ply", "x.ply", "--save_tsdf"]))
    assert {k: v for k, v in with_flags.items() if k not in NEW_FLAGS} == vars(a)
    inference.check_geometry_arguments(p, a)
    inference.check_egomotion_arguments(p, a)
    inference.check_temporal_arguments(p, a)
    inference.check_tsdf_arguments(p, a)
    assert tuple(getattr(a, f) for f in NEW_FLAGS) == (False, 0.2, (-12.8, 12.8, -3.2, 3.2, 0.0, 51.2), None, 0.0, "unit", "plane", None, False)
    assert inference.tsdf_grid(a) == ((-12.8, -3.2, 0.0), (129, 33, 257))
    seq = _sequence_dir(tmp_path, 3)
    poses = _poses_file(tmp_path / "poses.txt", 3)
    a = p.parse_args(seq + ["--tsdf", "--poses", poses, "--tsdf_voxel", "0.5", "--tsdf_extent", "-4", "4", "-2", "2", "0", "16", "--save_tsdf"] + CAMERA)
    for check in (inference.check_occ_arguments, inference.check_geometry_arguments, inference.check_egomotion_arguments,
                  inference.check_temporal_arguments, inference.check_tsdf_arguments):
        check(p, a)                                                             # --poses without --temporal: the volume reads them
    assert a.tsdf and not a.temporal and a.tsdf_trunc == 1.5 and a.tsdf_sdf == "plane" and inference.tsdf_grid(a) == ((-4.0, -2.0, 0.0), (17, 9, 33))
    a = p.parse_args(seq + ["--tsdf", "--egomotion", "--temporal"] + CAMERA)
    for check in (inference.check_occ_arguments, inference.check_geometry_arguments, inference.check_egomotion_arguments,
                  inference.check_temporal_arguments, inference.check_tsdf_arguments):
        check(p, a)                                                             # the estimate gives the poses of both
    assert a.tsdf and a.egomotion and a.temporal and a.poses is None


def test_cli_refuses_tsdf_without_what_it_needs(tmp_path, capsys):
    seq = _sequence_dir(tmp_path, 3)
    poses = _poses_file(tmp_path / "poses.txt", 3)
    ok = seq + ["--tsdf", "--poses", poses] + CAMERA
    assert _cli_refused(seq + ["--tsdf", "--poses", poses], capsys).endswith(": error: --tsdf and --save_tsdf need a camera: --calib PATH or --camera FX FY CX CY BASELINE\n")
    assert _cli_refused(ok + ["--workers", "2"], capsys).endswith(": error: --tsdf / --save_tsdf run in the sequential mode only: use --workers 0\n")
    assert _cli_refused(["--left_img", str(tmp_path / "left_test.png"), "--tsdf", "--poses", poses] + CAMERA, capsys).endswith(
        ": error: --tsdf maps a sequence: use directory mode (--img_path), not --left_img\n")
    assert _cli_refused(seq + ["--tsdf"] + CAMERA, capsys).endswith(": error: --tsdf needs the pose of every pair: --poses PATH or --egomotion\n")
    needs = ": error: --tsdf_voxel, --tsdf_extent, --tsdf_trunc, --tsdf_trunc_px, --tsdf_weight, --tsdf_sdf, --save_tsdf_ply and --save_tsdf need --tsdf\n"
    for flags in (["--tsdf_voxel", "0.5"], ["--tsdf_extent", "0", "1", "0", "1", "0", "1"], ["--tsdf_trunc", "1"], ["--tsdf_trunc_px", "0"],
                  ["--tsdf_weight", "unit"], ["--tsdf_sdf", "ray"], ["--save_tsdf_ply", "x.ply"], ["--save_tsdf"]):
        assert _cli_refused(seq + flags + CAMERA, capsys).endswith(needs)
    assert _cli_refused(ok + ["--tsdf_voxel", "0"], capsys).endswith(": error: --tsdf_voxel must be finite and > 0, got 0.0\n")
    assert _cli_refused(ok + ["--tsdf_voxel", "nan"], capsys).endswith(": error: --tsdf_voxel must be finite and > 0, got nan\n")
    assert _cli_refused(ok + ["--tsdf_extent", "1", "1", "0", "1", "0", "1"], capsys).endswith(
        ": error: --tsdf_extent must be finite X0 < X1, Y0 < Y1, Z0 < Z1, got 1.0 1.0 0.0 1.0 0.0 1.0\n")
    assert _cli_refused(ok + ["--tsdf_voxel", "0.001"], capsys).endswith(": error: --tsdf_extent / --tsdf_voxel: dims[0] must be an integer in 2 .. 4096, got 25601\n")
    assert _cli_refused(ok + ["--tsdf_voxel", "0.02", "--tsdf_extent", "-12.8", "12.8", "-12.8", "12.8", "0", "51.2"], capsys).endswith(
        ": error: --tsdf_extent / --tsdf_voxel: dims (1281, 1281, 2561): a volume holds fewer than 2^31 voxels\n")
    assert _cli_refused(ok + ["--tsdf_trunc", "0"], capsys).endswith(": error: --tsdf_trunc must be finite and > 0, got 0.0\n")
    assert _cli_refused(ok + ["--tsdf_trunc_px", "-1"], capsys).endswith(": error: --tsdf_trunc_px must be finite and >= 0, got -1.0\n")
    assert "invalid choice" in _cli_refused(ok + ["--tsdf_weight", "both"], capsys) and "invalid choice" in _cli_refused(ok + ["--tsdf_sdf", "x"], capsys)
    short = _poses_file(tmp_path / "short.txt", 2)
    assert _cli_refused(seq + ["--tsdf", "--poses", short] + CAMERA, capsys).endswith(
        f": error: --poses: {short} holds 2 poses for 3 pairs (line i belongs to the i-th pair in sorted order)\n")
    # --poses alone keeps its text
    assert _cli_refused(seq + ["--poses", poses] + CAMERA, capsys).endswith(
        ": error: --poses, --temporal_gate, --temporal_q, --temporal_sigma and --temporal_hold need --temporal\n")
    assert not os.path.exists(tmp_path / "out")             # refused before the output folder is touched
