"""lws_tsdf_integrate, lws_tsdf_raycast and lws_tsdf_points on the device, bit for bit against the numpy restatement
(tests/tsdf_reference.py, which also holds the cases; tests/test_tsdf_cpu.py asserts that they reach every branch of the rules).
Volumes of 5 x 3 x 2 (a quad and a tail of one voxel a row), 33 x 4 x 5 (rows at every alignment, a tail of one voxel) and 65 x 7 x 9 (more
than one workgroup) meet maps of 5 x 7 and 48 x 96, one and three frames, three motions, every optional input given or not, inputs
sprinkled with NaN, +-inf, 0 and negative values, both weight modes, a finite w_max, and a volume that already holds state and is
poisoned wherever it is unobserved.  Then: batching, views one element past a 16-byte boundary, the exact wall, the ray-caster and
the point extraction on crafted volumes, guard bands, a captured graph, the road scene against the truth, and TsdfVolume."""
import ctypes
import itertools

import numpy as np
import pytest

import guarded
import temporal_reference as TR
import tsdf_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_geometry import cu, misaligned  # noqa: E402
from test_tsdf_cpu import SCENE, WALL, scene_volume, wall_volume  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


# ---- the raw calls ----
def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def grid(dims, origin, vs):
    return (*dims, *(float(o) for o in origin), float(vs))


def raw_integrate(lib, dev, b, shape, g, kw):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_tsdf_integrate(P(b["disp"]), P(b.get("sigma")), P(b.get("mask")), P(b.get("normals")), P(b.get("rgb")), P(b["cam"]), P(b["pose"]),
                                          *shape, P(b["T"]), P(b["Wt"]), P(b.get("C")), *g, kw["sigma0"], kw["min_disp"], kw["max_depth"], kw["mu0"],
                                          kw["mu_d"], kw["sigma_min"], kw["wmode"], kw["w_max"], P(b.get("updated")), stream()), "lws_tsdf_integrate")


def raw_raycast(lib, dev, b, shape, g, z_near, step, nsteps, w_min=0.0):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_tsdf_raycast(P(b["T"]), P(b["Wt"]), *g, P(b["cam"]), P(b["pose"]), *shape, z_near, step, nsteps, w_min, P(b["disp"]),
                                        P(b.get("weight")), P(b.get("normals")), stream()), "lws_tsdf_raycast")


def raw_points(lib, dev, b, g, max_points, w_min=0.0):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_tsdf_points(P(b["T"]), P(b["Wt"]), P(b.get("C")), *g, w_min, ctypes.c_int64(max_points), P(b["work"]), P(b["points"]),
                                       P(b.get("vnormals")), P(b["counts"]), stream()), "lws_tsdf_points")


def put_colour(C, put):
    """C placed as int32 words, one per voxel, so that a view one element past a boundary keeps the 4-byte alignment C needs."""
    return put(np.ascontiguousarray(C).view(np.int32), "C").view(torch.uint8)


def integrate_buffers(c, put):
    """The device buffers of an integrate case; put(array, name) places one."""
    b = {k: put(c[k], k) for k in ("disp", "cam", "pose", "sigma", "mask", "normals", "rgb") if c[k] is not None}
    b.update(T=put(c["T0"], "T"), Wt=put(c["W0"], "Wt"))
    if c["C0"] is not None:
        b["C"] = put_colour(c["C0"], put)
    return b


def check_volume(b, want, what):
    guarded.assert_bits(b["T"], want[0], what + " T")
    guarded.assert_bits(b["Wt"], want[1], what + " Wt")
    if want[2] is not None:
        guarded.assert_bits(b["C"], want[2], what + " C")
    if "updated" in b:
        guarded.assert_bits(b["updated"], want[3], what + " updated")


def want_points(T, Wt, C, origin, vs, w_min=0.0):
    xyz, rgba, nrm, _, _ = R.points(T, Wt, C, origin, vs, w_min)
    return R.records(xyz, rgba), nrm


# ---- 1. integrate ----
@pytest.mark.parametrize("dims,hw,B", list(itertools.product(R.VOLUMES, R.MAPS, R.BATCHES)))
def test_integrate_bitexact(dev, hip_lib, dims, hw, B):
    c = R.integrate_case(dims, hw, B)
    b = integrate_buffers(c, lambda a, name: cu(a, dev))
    b["updated"] = torch.full((B,), 77, dtype=torch.int64, device=dev)
    raw_integrate(hip_lib, dev, b, (B, *hw), grid(dims, c["origin"], c["vs"]), c["kw"])
    print(f"{dims} {hw} B={B}: voxels per branch {c['stats']}, taken per frame {c['want'][3].tolist()}")
    check_volume(b, c["want"], f"{dims} {hw} B={B}")
    b2 = integrate_buffers(c, lambda a, name: cu(a, dev))   # updated NULL: the one launch
    raw_integrate(hip_lib, dev, b2, (B, *hw), grid(dims, c["origin"], c["vs"]), c["kw"])
    check_volume(b2, c["want"], f"{dims} {hw} B={B} updated NULL")


# ---- 3. batching and alignment ----
@pytest.mark.parametrize("dims,hw", [((33, 4, 5), (5, 7)), ((65, 7, 9), (48, 96))])
def test_a_batch_equals_its_frames_one_by_one(dev, hip_lib, dims, hw):
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import Camera
    c = R.integrate_case(dims, hw, 3)
    assert (c["want"][3] > 0).sum() >= 2
    f = c["cam"][0]
    cams = [Camera(float(f[0]), float(f[1]), float(f[2]), float(f[3]), 4.0)] * 3
    assert np.array_equal(cams[0].row(), f)
    kw = {**{k: v for k, v in c["kw"].items() if k != "wmode"}, "weight": ("unit", "sigma")[c["kw"]["wmode"]]}
    t = lambda a, idx: None if a is None else cu(a[idx], dev)      # noqa: E731
    T, Wt, C = cu(c["T0"], dev), cu(c["W0"], dev), None if c["C0"] is None else cu(c["C0"], dev)
    upd = []
    for k in range(3):
        i = slice(k, k + 1)
        upd.append(ops.tsdf_integrate(T, Wt, c["origin"], c["vs"], t(c["disp"], i), cams[:1], c["pose"][i], C=C, sigma=t(c["sigma"], i), mask=t(c["mask"], i),
                                      normals=t(c["normals"], i), rgb=t(c["rgb"], i), **kw))
    check_volume(dict(T=T, Wt=Wt, C=C, updated=torch.cat(upd)), c["want"], "one by one")


def test_batch_position_independence(dev, hip_lib):
    """A frame gives the same bytes alone, first of two and second of two, where the other frame takes nothing (its map is empty)."""
    dims, hw = (65, 7, 9), (48, 96)
    c = R.integrate_case(dims, hw, 1)
    assert c["want"][3][0] > 0
    g = grid(dims, c["origin"], c["vs"])
    for pos in (0, 1):
        two = {k: None if c[k] is None else np.concatenate([c[k], c[k]]) for k in ("disp", "cam", "pose", "sigma", "mask", "normals", "rgb")}
        two["disp"][1 - pos] = 0
        b = {k: cu(v, dev) for k, v in two.items() if v is not None}
        b.update(T=cu(c["T0"], dev), Wt=cu(c["W0"], dev), updated=torch.full((2,), 77, dtype=torch.int64, device=dev))
        if c["C0"] is not None:
            b["C"] = cu(c["C0"], dev)
        raw_integrate(hip_lib, dev, b, (2, *hw), g, c["kw"])
        want_upd = np.zeros(2, np.int64)
        want_upd[pos] = c["want"][3][0]
        check_volume(b, (*c["want"][:3], want_upd), f"position {pos}")


@pytest.mark.parametrize("dims,hw,B", [((33, 4, 5), (5, 7), 3), ((65, 7, 9), (48, 96), 1), ((64, 4, 3), (48, 96), 1)])
def test_one_element_past_a_16_byte_boundary(dev, hip_lib, dims, hw, B):
    """Every tensor starts one element past a 16-byte boundary; 64 x 4 x 3 is the volume whose every quad is whole, aligned when the
    base is (run both ways)."""
    if dims in R.VOLUMES:
        c = R.integrate_case(dims, hw, B)
    else:
        base = R.integrate_case((65, 7, 9), hw, B)
        rng = np.random.default_rng(3)
        T0, W0, C0 = R.poisoned_state(dims, base["kw"]["mu0"], rng, base["rgb"] is not None)
        c = {**base, "dims": dims, "T0": T0, "W0": W0, "C0": C0}
        c["want"] = R.integrate(T0, W0, C0, c["origin"], c["vs"], c["disp"], c["cam"], c["pose"], c["sigma"], c["mask"], c["normals"], c["rgb"], **c["kw"])
        assert c["want"][3][0] > 0
    g = grid(dims, c["origin"], c["vs"])
    for put in (lambda a, name: misaligned(a, dev), lambda a, name: cu(a, dev)):
        b = integrate_buffers(c, put)
        b["updated"] = torch.full((B,), 77, dtype=torch.int64, device=dev)
        raw_integrate(hip_lib, dev, b, (B, *hw), g, c["kw"])
        check_volume(b, c["want"], f"{dims}")
    # the read-only calls on the misaligned volume the integrate left
    T, Wt, C = c["want"][:3]
    vb = dict(T=misaligned(T, dev), Wt=misaligned(Wt, dev), cam=misaligned(c["cam"][:1], dev), pose=misaligned(c["pose"][:1], dev), disp=misaligned(np.zeros((1, 1, *hw), F), dev),
              weight=misaligned(np.zeros((1, 1, *hw), F), dev), normals=misaligned(np.zeros((1, 3, *hw), F), dev))
    raw_raycast(hip_lib, dev, vb, (1, *hw), g, 9.0, 0.5 * c["vs"], 64)
    want = R.raycast(T, Wt, c["origin"], c["vs"], c["cam"][:1], c["pose"][:1], *hw, 9.0, 0.5 * c["vs"], 64)
    for key, w in zip(("disp", "weight", "normals"), want):
        guarded.assert_bits(vb[key], w, f"misaligned raycast {key}")


# ---- 4. the exact wall ----
def test_exact_wall(dev, hip_lib):
    """A fronto-parallel wall at d = 7.5 px, z = 8 m, with dyadic origin, voxel and steps: the arithmetic is exact.  After one frame
    and after five, every pixel that hits ray-casts to 7.5 px in bits, every extracted point has Z == 8 and the normal (0, 0, -1)
    wherever the six neighbours are observed."""
    from lwsnet_amd.geometry import Camera
    from lwsnet_amd.tsdf import TsdfVolume
    cam = Camera(120.0, 120.0, 47.5, 20.0, 0.5)
    assert tuple(cam.row()) == tuple(F(v) for v in TR.SCENE_CAM)
    vol = TsdfVolume(WALL["origin"], WALL["vs"], WALL["dims"], mu0=WALL["mu0"], device=dev)
    d = cu(np.full((1, 1, 48, 96), 7.5, F), dev)
    for k in range(5):
        upd = vol.integrate(d, cam, TR.IDENTITY)
        if k not in (0, 4):
            continue
        want = wall_volume(k + 1)
        guarded.assert_bits(vol.Wt, want["Wt"], f"frame {k} Wt")
        seen = want["Wt"] > 0
        assert np.array_equal(guarded.as_bits(vol.T.cpu().numpy()[seen]), guarded.as_bits(want["T"][seen])) and int(upd[0]) == want["updated"]
        view = vol.raycast(cam, TR.IDENTITY, 48, 96, z_near=1.0, step=0.25, nsteps=60)
        r = view.disp.cpu().numpy()
        hit = r > 0
        print(f"frame {k}: {int(hit.sum())} of {hit.size} pixels hit")
        assert hit.sum() == WALL["hits"] and (r[hit] == F(7.5)).all()
        for key, w in zip(("disp", "weight", "normals"), want["view"]):
            guarded.assert_bits(getattr(view, key), w, f"frame {k} view {key}")
        pts = vol.points(4096)
        n = int(pts.counts[0])
        rec = pts.points[:n].cpu().numpy().view(F).reshape(n, 4)
        nrm = pts.vnormals[:n].cpu().numpy()
        with_n = (nrm != 0).any(axis=1)
        assert n == len(want["points"][0]) > 0 and (rec[:, 2] == F(8.0)).all() and with_n.any()
        assert (nrm[with_n] == np.array([0, 0, -1, 0], F)).all()
        guarded.assert_bits(pts.points[:n], want["points"][0], f"frame {k} points")
        guarded.assert_bits(pts.vnormals[:n], want["points"][1], f"frame {k} normals")


# ---- 5. the ray-caster ----
@pytest.mark.parametrize("kw", R.RAYCASTS, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_raycast_bitexact(dev, hip_lib, kw):
    """Three views of the crafted volume in one call (tests/test_tsdf_cpu.py asserts what the four settings reach together: rays
    that never enter the volume, a start inside the surface, the back-face stop, unobserved taps on the way, a hit in the first
    interval, nsteps exhausted, a w_min that blinds taps, normals with an unknown sample)."""
    T, Wt, origin, vs = R.crafted_volume()
    cam, pose = R.raycast_views()
    H, W = 24, 40
    want = R.raycast(T, Wt, origin, vs, cam, pose, H, W, **kw)
    b = dict(T=cu(T, dev), Wt=cu(Wt, dev), cam=cu(cam, dev), pose=cu(pose, dev), disp=torch.full((3, 1, H, W), 7.0, device=dev),
             weight=torch.full((3, 1, H, W), 7.0, device=dev), normals=torch.full((3, 3, H, W), 7.0, device=dev))
    raw_raycast(hip_lib, dev, b, (3, H, W), grid(T.shape[::-1], origin, vs), kw["z_near"], kw["step"], kw["nsteps"], kw.get("w_min", 0.0))
    for key, w in zip(("disp", "weight", "normals"), want):
        guarded.assert_bits(b[key], w, key)
    only = dict(b, disp=torch.full((3, 1, H, W), 7.0, device=dev), weight=None, normals=None)      # weight and normals NULL
    raw_raycast(hip_lib, dev, only, (3, H, W), grid(T.shape[::-1], origin, vs), kw["z_near"], kw["step"], kw["nsteps"], kw.get("w_min", 0.0))
    guarded.assert_bits(only["disp"], want[0], "disp alone")
    swapped = dict(b, cam=cu(cam[::-1], dev), pose=cu(pose[::-1], dev), disp=torch.empty((3, 1, H, W), device=dev))      # batch position
    raw_raycast(hip_lib, dev, swapped, (3, H, W), grid(T.shape[::-1], origin, vs), kw["z_near"], kw["step"], kw["nsteps"], kw.get("w_min", 0.0))
    guarded.assert_bits(swapped["disp"], want[0][::-1], "views in the other order")


# ---- 6. the points ----
def points_buffers(dev, dims, cap, put, T, Wt, C):
    from lwsnet_amd import _lib
    nb = _lib.nbytes("lws_tsdf_points_workspace", dims[1], dims[2])
    assert nb >= 8 * dims[1] * dims[2]
    return dict(T=put(T), Wt=put(Wt), C=None if C is None else put_colour(C, lambda a, name: put(a)), work=torch.full((nb // 8,), -1, dtype=torch.int64, device=dev),
                points=torch.full((cap + 8, 16), 0xA5, dtype=torch.uint8, device=dev), vnormals=torch.full((cap + 8, 4), 7.0, device=dev),
                counts=torch.full((1,), 77, dtype=torch.int64, device=dev))


@pytest.mark.parametrize("dims", [(5, 3, 2), (33, 4, 5), (65, 7, 9), (300, 3, 2), *R.POINTS_CHUNKED])
def test_points_bitexact_order_included(dev, hip_lib, dims):
    """300 x 3 x 2: a row of more than one chunk of 256 voxels; R.POINTS_CHUNKED: 256, 258 and 520 rows, where the scan of the row
    counts carries from chunk to chunk.  Then with a w_min, without C and normals, and with a capacity
    smaller than the count: counts is the full number, the first max_points records are equal, what lies behind is untouched."""
    T, Wt, C, origin, vs = R.points_volume(dims, 1)
    g = grid(dims, origin, vs)
    rec, nrm = want_points(T, Wt, C, origin, vs)
    n = len(rec)
    b = points_buffers(dev, dims, n, lambda a: cu(a, dev), T, Wt, C)
    raw_points(hip_lib, dev, b, g, n)
    assert int(b["counts"][0]) == n > 0
    guarded.assert_bits(b["points"][:n], rec, "points")
    guarded.assert_bits(b["vnormals"][:n], nrm, "normals")
    assert (b["points"][n:] == 0xA5).all() and (b["vnormals"][n:] == 7.0).all()
    rec2, _ = want_points(T, Wt, None, origin, vs, w_min=1.5)
    b2 = points_buffers(dev, dims, n, lambda a: misaligned(a, dev), T, Wt, None)
    b2["vnormals"] = None
    raw_points(hip_lib, dev, b2, g, n, w_min=1.5)
    assert int(b2["counts"][0]) == len(rec2)
    guarded.assert_bits(b2["points"][:len(rec2)], rec2, "points, w_min 1.5, white")
    cap = max(1, n // 3)
    b3 = points_buffers(dev, dims, cap, lambda a: cu(a, dev), T, Wt, C)
    raw_points(hip_lib, dev, b3, g, cap)
    assert int(b3["counts"][0]) == n
    guarded.assert_bits(b3["points"][:cap], rec[:cap], "the first max_points records")
    guarded.assert_bits(b3["vnormals"][:cap], nrm[:cap], "the first max_points normals")
    assert (b3["points"][cap:] == 0xA5).all() and (b3["vnormals"][cap:] == 7.0).all()


def test_points_of_an_empty_volume(dev, hip_lib):
    dims = (33, 4, 5)
    T, Wt, C, origin, vs = R.points_volume(dims, 2)
    b = points_buffers(dev, dims, 4, lambda a: cu(a, dev), T, np.zeros_like(Wt), C)
    raw_points(hip_lib, dev, b, grid(dims, origin, vs), 4)
    assert int(b["counts"][0]) == 0 and (b["points"] == 0xA5).all() and (b["vnormals"] == 7.0).all()


# ---- 7. the memory contract ----
@pytest.mark.parametrize("word", guarded.FLOAT_WORDS, ids=guarded.word_id)
def test_memory_contract(dev, hip_lib, word):
    """Every buffer of the three calls between poisoned flanks, the outputs and the workspace poisoned inside; T and C hold the
    poison word / 0xFF wherever Wt == 0 and must not reach a result."""
    dims, hw, B = (65, 7, 9), (48, 96), 3
    base = R.integrate_case(dims, hw, B)
    rng = np.random.default_rng(8)
    T0, W0, C0 = R.poisoned_state(dims, base["kw"]["mu0"], rng, True)
    rgb = rng.integers(0, 256, (B, *hw, 3), dtype=np.uint8)
    T0 = np.where(W0 > 0, T0, np.array([word], np.uint32).view(F)[0]).astype(F)
    c = {**base, "T0": T0, "W0": W0, "C0": C0, "rgb": rgb}
    want = R.integrate(T0, W0, C0, c["origin"], c["vs"], c["disp"], c["cam"], c["pose"], c["sigma"], c["mask"], c["normals"], rgb, **c["kw"])
    assert (want[3] > 0).any() and (want[1] == 0).any()
    g = grid(dims, c["origin"], c["vs"])
    gd = guarded.Guard(dev, word, skew=1)
    b = integrate_buffers(c, lambda a, name: gd.place(a, name=name, word=guarded.MASK_WORD if name == "mask" else None))
    b["updated"] = gd.empty((B,), np.int64, align16=True, name="updated")
    raw_integrate(hip_lib, dev, b, (B, *hw), g, c["kw"])
    check_volume(b, want, "guarded integrate")
    gd.check()
    # the read-only calls on the volume the integrate left: still poisoned where Wt == 0
    T, Wt, C = want[:3]
    gd = guarded.Guard(dev, word, skew=1)
    v = dict(T=gd.place(T, name="T"), Wt=gd.place(Wt, name="Wt"), cam=gd.place(c["cam"], name="cam"), pose=gd.place(c["pose"], name="pose"),
             disp=gd.empty((B, 1, *hw), F, name="disp"), weight=gd.empty((B, 1, *hw), F, name="weight"), normals=gd.empty((B, 3, *hw), F, name="normals"))
    raw_raycast(hip_lib, dev, v, (B, *hw), g, 9.0, 0.0625, 80)
    view = R.raycast(T, Wt, c["origin"], c["vs"], c["cam"], c["pose"], *hw, 9.0, 0.0625, 80)
    assert (view[0] > 0).any()
    for key, w in zip(("disp", "weight", "normals"), view):
        guarded.assert_bits(v[key], w, f"guarded raycast {key}")
    gd.check()
    rec, nrm = want_points(T, Wt, C, c["origin"], c["vs"])
    n = len(rec)
    assert n > 0
    gd = guarded.Guard(dev, word, skew=1)
    p = dict(T=gd.place(T, name="T"), Wt=gd.place(Wt, name="Wt"), C=put_colour(C, lambda a, name: gd.place(a, name=name)),
             work=gd.empty(((dims[1] * dims[2] + 31) // 32 * 32,), np.int64, align16=True, name="workspace"),
             points=gd.empty((n, 16), np.uint8, align16=True, name="points"), vnormals=gd.empty((n, 4), F, align16=True, name="vnormals"),
             counts=gd.empty((1,), np.int64, align16=True, name="counts"))
    raw_points(hip_lib, dev, p, g, n)
    assert int(p["counts"][0]) == n
    guarded.assert_bits(p["points"], rec, "guarded points")
    guarded.assert_bits(p["vnormals"], nrm, "guarded normals")
    gd.check()


# ---- 8. graph capture ----
def test_graph_capture_replays_on_two_input_sets(dev, hip_lib):
    """Integrate, raycast and points captured once, replayed on two input sets (the volume is reset to its start before each)."""
    dims, hw, B = (65, 7, 9), (48, 96), 3
    first = R.integrate_case(dims, hw, B)
    second = {**first, "disp": np.ascontiguousarray(first["disp"][::-1]), "pose": np.ascontiguousarray(first["pose"][::-1])}
    second["want"] = R.integrate(first["T0"], first["W0"], first["C0"], first["origin"], first["vs"], second["disp"], first["cam"], second["pose"],
                                 first["sigma"], first["mask"], first["normals"], first["rgb"], **first["kw"])
    g = grid(dims, first["origin"], first["vs"])
    b = integrate_buffers(first, lambda a, name: cu(a, dev))
    cap = 4096
    b.update(updated=torch.empty((B,), dtype=torch.int64, device=dev), vdisp=torch.empty((B, 1, *hw), device=dev), weight=torch.empty((B, 1, *hw), device=dev),
             vnormals3=torch.empty((B, 3, *hw), device=dev), work=torch.empty((dims[1] * dims[2] + 32,), dtype=torch.int64, device=dev),
             points=torch.empty((cap, 16), dtype=torch.uint8, device=dev), vnormals=torch.empty((cap, 4), device=dev),
             counts=torch.empty((1,), dtype=torch.int64, device=dev))

    def run():
        raw_integrate(hip_lib, dev, b, (B, *hw), g, first["kw"])
        raw_raycast(hip_lib, dev, dict(T=b["T"], Wt=b["Wt"], cam=b["cam"], pose=b["pose"], disp=b["vdisp"], weight=b["weight"], normals=b["vnormals3"]),
                    (B, *hw), g, 9.0, 0.0625, 80)
        raw_points(hip_lib, dev, b, g, cap)

    run()                                                   # the code objects are loaded before the capture
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for c in (first, second, first):
        for k in ("disp", "pose"):
            b[k].copy_(cu(c[k], dev))
        b["T"].copy_(cu(c["T0"], dev))
        b["Wt"].copy_(cu(c["W0"], dev))
        if c["C0"] is not None:
            b["C"].copy_(cu(c["C0"], dev))
        for k in ("updated", "vdisp", "weight", "vnormals3", "work", "points", "vnormals", "counts"):
            b[k].fill_(77)
        graph.replay()
        torch.cuda.synchronize(dev)
        check_volume(b, c["want"], "replay")
        T, Wt, C = c["want"][:3]
        view = R.raycast(T, Wt, c["origin"], c["vs"], c["cam"], c["pose"], *hw, 9.0, 0.0625, 80)
        for key, w in zip(("vdisp", "weight", "vnormals3"), view):
            guarded.assert_bits(b[key], w, f"replay {key}")
        rec, nrm = want_points(T, Wt, C, c["origin"], c["vs"])
        assert int(b["counts"][0]) == len(rec) <= cap
        guarded.assert_bits(b["points"][:len(rec)], rec, "replay points")
        guarded.assert_bits(b["vnormals"][:len(rec)], nrm, "replay normals")


# ---- 9. accuracy against the truth ----
def test_road_scene_against_the_truth(dev, hip_lib):
    """The road-and-wall scene from five poses into a 0.125 m volume with the point-to-plane distance, ray-cast from the third pose.
    The bounds are 1.5 x what tests/tsdf_reference.py alone gives on the CPU (tests/test_tsdf_cpu.py asserts these figures):
    2361 of 2400 scored pixels hit (98.4 %), p95 0.002639 px, max 0.193126 px; without normals 1613 hit.  The device result is also
    held to the restatement in bytes."""
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import Camera
    from lwsnet_amd.tsdf import TsdfVolume
    cam = Camera(120.0, 120.0, 47.5, 20.0, 0.5)
    hits = {}
    for use_normals in (True, False):
        want = scene_volume(use_normals)
        vol = TsdfVolume(SCENE["origin"], SCENE["vs"], SCENE["dims"], mu0=SCENE["mu0"], mu_d=0.0, weight="unit", device=dev)
        for k, pose in enumerate(SCENE["poses"]):
            d = cu(want["frames"][k], dev)
            n = ops.surface_normals(d, cam, max_jump=1.0)[0] if use_normals else None
            if use_normals:
                guarded.assert_bits(n, want["normals"][k], f"normals of frame {k}")
            vol.integrate(d, cam, pose, normals=n)
        guarded.assert_bits(vol.Wt, want["Wt"], "Wt")
        seen = want["Wt"] > 0
        assert np.array_equal(guarded.as_bits(vol.T.cpu().numpy()[seen]), guarded.as_bits(want["T"][seen]))
        view = vol.raycast(cam, SCENE["poses"][2], 48, 96, z_near=1.0, step=0.0625, nsteps=240)
        for key, w in zip(("disp", "weight", "normals"), want["view"]):
            guarded.assert_bits(getattr(view, key), w, f"normals={use_normals} view {key}")
        r = view.disp[0, 0].cpu().numpy()
        truth = TR.render(SCENE["poses"][2])
        scored, hit = truth >= 4.5, r > 0
        err = np.abs(r[scored & hit].astype(np.float64) - truth[scored & hit])
        hits[use_normals] = int((scored & hit).sum())
        print(f"normals={use_normals}: {hits[use_normals]} of {int(scored.sum())} scored pixels hit, p95 {np.percentile(err, 95):.6f} max {err.max():.6f} px")
        assert not (hit & (truth == 0)).any()
        if use_normals:
            assert hits[True] >= 0.95 * scored.sum()
            assert np.percentile(err, 95) <= 1.5 * SCENE["p95"] and err.max() <= 1.5 * SCENE["max"]
    assert hits[False] < hits[True]


# ---- 10. the class ----
def test_volume_over_four_frames(dev, hip_lib, tmp_path):
    """TsdfVolume with colour and sigma weights over four frames against the reference loop; reset(); the PLY."""
    from lwsnet_amd.geometry import Camera, read_mesh_ply
    from lwsnet_amd.tsdf import TsdfVolume
    cam = Camera(120.0, 120.0, 47.5, 20.0, 0.5)
    rows = cam.row()[None]
    rng = np.random.default_rng(6)
    poses = [TR.forward_pose(k, 0.6, yaw=0.01) for k in range(4)]
    origin, vs, dims = (-4.0, -1.0, 4.0), 0.25, (33, 12, 40)
    kw = dict(mu0=0.5, mu_d=0.5, w_max=1e4)
    vol = TsdfVolume(origin, vs, dims, weight="sigma", colour=True, sigma0=0.3, device=dev, **kw)
    T, Wt, C = np.full(dims[::-1], np.nan, F), np.zeros(dims[::-1], F), np.full((*dims[::-1], 4), 0xFF, np.uint8)
    vol.T.copy_(cu(T, dev))
    vol.C.copy_(cu(C, dev))
    for k, p in enumerate(poses):
        t = TR.render(p)
        d = np.where(t > 0, t + rng.normal(0, 0.1, t.shape), 0).astype(F)[None, None]
        sigma = rng.uniform(0.05, 0.5, d.shape).astype(F) if k % 2 else None
        rgb = rng.integers(0, 256, (1, 48, 96, 3), dtype=np.uint8)
        upd = vol.integrate(cu(d, dev), cam, p, sigma=None if sigma is None else cu(sigma, dev), rgb=cu(rgb, dev))
        T, Wt, C, want_upd = R.integrate(T, Wt, C, origin, vs, d, rows, R.pose_block(p)[None], sigma, None, None, rgb, sigma0=0.3, wmode=1, **kw)
        guarded.assert_bits(upd, want_upd, f"frame {k} updated")
        check_volume(dict(T=vol.T, Wt=vol.Wt, C=vol.C), (T, Wt, C), f"frame {k}")
    assert vol.frames == 4 and want_upd[0] > 0
    path = tmp_path / "map.ply"
    n = vol.write_ply(str(path))
    rec, nrm = want_points(T, Wt, C, origin, vs)
    verts, faces = read_mesh_ply(str(path))
    assert n == len(rec) == len(verts) > 0 and len(faces) == 0
    got = np.stack([verts["x"], verts["y"], verts["z"]], -1)
    assert np.array_equal(guarded.as_bits(got), guarded.as_bits(rec[:, :12].copy().view(F).reshape(-1, 3)))
    assert np.array_equal(guarded.as_bits(np.stack([verts["nx"], verts["ny"], verts["nz"]], -1)), guarded.as_bits(nrm[:, :3]))
    assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"], verts["alpha"]], -1), rec[:, 12:])
    with pytest.raises(ValueError, match="more than max_points"):
        vol.write_ply(str(tmp_path / "small.ply"), max_points=n - 1)
    vol.reset()
    assert vol.frames == 0 and int(vol.points(16).counts[0]) == 0


# ---- 10. the CLI ----
def test_inference_cli_tsdf_files(dev, hip_lib, tmp_path, caplog):
    """--tsdf over a small synthetic sequence with --poses written here: a ray-cast PNG per frame, a PLY that parses and whose vertex
    count is the logged one, one `voxels updated` line per frame."""
    import logging
    import os
    import re
    from PIL import Image
    from lwsnet_amd import inference, synth
    from lwsnet_amd.geometry import read_mesh_ply
    from test_gpu_geometry import KITTI15_CALIB
    n = 3
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, n)
    calib = tmp_path / "calib.txt"
    calib.write_text(KITTI15_CALIB.format(fx=721.5377, cx=609.5593, cy=172.854, t3=44.85728 - 0.54 * 721.5377))
    pose_file = tmp_path / "poses.txt"
    pose_file.write_text("".join(" ".join(repr(float(v)) for v in TR.forward_pose(k + 1, 0.3, yaw=0.002).reshape(12)) + "\n" for k in range(n)))
    out, ply = tmp_path / "out", tmp_path / "map.ply"
    with caplog.at_level(logging.INFO, logger="lwsnet_amd.inference"):
        written = inference.main(["--img_path", root + "/", "--synthetic_weights", "--calib", str(calib), "--occ_check", "1", "--save_path", str(out),
                                  "--tsdf", "--poses", str(pose_file), "--tsdf_voxel", "0.4", "--tsdf_extent", "-8", "8", "-3.2", "3.2", "0", "32",
                                  "--save_tsdf", "--save_tsdf_ply", str(ply)])
    stems = [f"{k:06d}_10" for k in range(n)]
    assert sorted(os.listdir(out)) == sorted(s + e for s in stems for e in (".png", "_occ.png", "_tsdf.png"))
    assert len(written) == 3 * n + 1 and written[-1] == str(ply)
    lines = [r.getMessage() for r in caplog.records]
    updated = [int(m[1]) for m in (re.fullmatch(r"TSDF: voxels updated = (\d+)", line) for line in lines) if m]
    assert len(updated) == n and all(u > 0 for u in updated), updated
    logged = [int(m[1]) for m in (re.fullmatch(r"Save TSDF points = .*, vertices = (\d+)", line) for line in lines) if m]
    verts, faces = read_mesh_ply(str(ply))
    assert logged == [len(verts)] and len(faces) == 0 and np.isfinite(np.stack([verts[k] for k in ("x", "y", "z", "nx", "ny", "nz")])).all()
    for s in stems:
        img = np.asarray(Image.open(out / (s + "_tsdf.png")))
        assert img.shape[:2] == np.asarray(Image.open(out / (s + ".png"))).shape[:2]
