"""lws_tsdf_mesh on the device, bit for bit against the numpy restatement (tests/tsdf_mesh_reference.py; tests/test_tsdf_mesh_cpu.py
holds that restatement's table and meshes to the rule).  All 256 cases on one cube; rows of 255 .. 258 voxels, where a cube's +x
corners lie in the next chunk of 256 voxels and the chunks advance by 255 cubes; the volumes whose row scans carry; holes, a w_min,
NaN, +-inf and 0 in T, C and vnormals given or not, a volume one element past a 16-byte boundary; the capacities; guard bands and a
poisoned workspace; a stalled stream; a captured graph; TsdfVolume and the inference CLI."""
import ctypes

import numpy as np
import pytest

import guarded
import stream_stall as SS
import temporal_reference as TR
import tsdf_mesh_reference as MR
import tsdf_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_geometry import cu, misaligned  # noqa: E402
from test_gpu_tsdf import P, grid, put_colour, raw_points, stream  # noqa: E402

F = np.float32
FACE_FILL = -77                                             # what an unwritten face holds


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def raw_mesh(lib, dev, b, g, max_points, max_faces, w_min=0.0, st=None):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_tsdf_mesh(P(b["T"]), P(b["Wt"]), P(b.get("C")), *g, w_min, ctypes.c_int64(max_points), ctypes.c_int64(max_faces), P(b["work"]),
                                     P(b["points"]), P(b.get("vnormals")), P(b["faces"]), P(b["counts"]), st or stream()), "lws_tsdf_mesh")


def outputs(dev, dims, cap_p, cap_f):
    """The workspace and the outputs, poisoned, with eight spare records and faces behind the capacities."""
    from lwsnet_amd import _lib
    nb = _lib.nbytes("lws_tsdf_mesh_workspace", dims[1], dims[2])
    assert nb >= 8 * (dims[1] * dims[2] + (dims[1] - 1) * (dims[2] - 1)) and nb % 256 == 0
    return dict(work=torch.full((nb // 8,), -1, dtype=torch.int64, device=dev), points=torch.full((cap_p + 8, 16), 0xA5, dtype=torch.uint8, device=dev),
                vnormals=torch.full((cap_p + 8, 4), 7.0, device=dev), faces=torch.full((cap_f + 8, 3), FACE_FILL, dtype=torch.int32, device=dev),
                counts=torch.full((2,), 77, dtype=torch.int64, device=dev))


def buffers(dev, dims, cap_p, cap_f, put, T, Wt, C):
    return dict(outputs(dev, dims, cap_p, cap_f), T=put(T), Wt=put(Wt), C=None if C is None else put_colour(C, lambda a, name: put(a)))


def run_and_check(lib, dev, dims, origin, vs, T, Wt, C, w_min=0.0, put=None, normals=True, what=""):
    """One call with capacities that fit exactly, held to the reference; returns (the buffers, the reference)."""
    want = MR.mesh(T, Wt, C, origin, vs, w_min)
    rec, nrm, faces = want
    n, m = len(rec), len(faces)
    b = buffers(dev, dims, max(n, 1), max(m, 1), put or (lambda a: cu(a, dev)), T, Wt, C)
    if not normals:
        b["vnormals"] = None
    raw_mesh(lib, dev, b, grid(dims, origin, vs), max(n, 1), max(m, 1), w_min)
    assert b["counts"].tolist() == [n, m], (what, b["counts"].tolist(), n, m)
    guarded.assert_bits(b["faces"][:m], faces, what + " faces")
    guarded.assert_bits(b["points"][:n], rec, what + " points")
    assert (b["faces"][m:] == FACE_FILL).all() and (b["points"][n:] == 0xA5).all()
    if normals:
        guarded.assert_bits(b["vnormals"][:n], nrm, what + " normals")
        assert (b["vnormals"][n:] == 7.0).all()
    return b, want


def same_as_points(lib, dev, dims, origin, vs, b, n, w_min=0.0):
    """points / vnormals / counts[0] of the mesh call against lws_tsdf_points on the same device buffers, in bits."""
    from lwsnet_amd import _lib
    p = dict(T=b["T"], Wt=b["Wt"], C=b.get("C"), work=torch.full((_lib.nbytes("lws_tsdf_points_workspace", dims[1], dims[2]) // 8,), -1, dtype=torch.int64, device=dev),
             points=torch.full_like(b["points"], 0xA5), vnormals=None if b.get("vnormals") is None else torch.full_like(b["vnormals"], 7.0),
             counts=torch.full((1,), 77, dtype=torch.int64, device=dev))
    raw_points(lib, dev, p, grid(dims, origin, vs), max(n, 1), w_min)
    assert int(p["counts"][0]) == int(b["counts"][0]) == n
    assert torch.equal(p["points"], b["points"])
    if p["vnormals"] is not None:
        assert torch.equal(p["vnormals"].view(torch.int32), b["vnormals"].view(torch.int32))


def noise_volume(dims, seed, holes=0.05):
    """T uniform noise with exact zeros, weights 1 and 2, a fraction `holes` unobserved and poisoned, a colour per voxel."""
    rng = np.random.default_rng(seed)
    shape = dims[::-1]
    Wt = rng.choice(np.array([1.0, 2.0], F), size=shape)
    Wt[rng.random(shape) < holes] = 0
    T = rng.uniform(-1, 1, shape).astype(F)
    T[rng.random(shape) < 0.05] = 0.0
    T[Wt == 0] = np.nan
    C = rng.integers(0, 256, (*shape, 4), dtype=np.uint8)
    C[Wt == 0] = 0xFF
    return T, Wt, C, (-1.0, 0.5, 2.0), 0.25


# ---- 1. the table on the device ----
def test_all_256_cases_on_one_cube(dev, hip_lib):
    dims, origin, vs = (2, 2, 2), (0.0, 0.0, 0.0), 1.0
    Wt = np.ones((2, 2, 2), F)
    cubes = MR.all_cases_volume()
    b = buffers(dev, dims, 12, 10, lambda a: cu(a, dev), cubes[0], Wt, None)
    table, empty = MR.table(), 0
    for case in range(256):
        rec, nrm, faces = MR.mesh(cubes[case], Wt, None, origin, vs)
        assert len(faces) == table[case, 0]
        b["T"].copy_(cu(cubes[case], dev))
        b["faces"].fill_(FACE_FILL)
        b["counts"].fill_(77)
        raw_mesh(hip_lib, dev, b, grid(dims, origin, vs), 12, 10)
        assert b["counts"].tolist() == [len(rec), len(faces)], case
        guarded.assert_bits(b["faces"][:len(faces)], faces, f"case {case}")
        guarded.assert_bits(b["points"][:len(rec)], rec, f"case {case} points")
        assert (b["faces"][len(faces):] == FACE_FILL).all(), case
        empty += len(faces) == 0
    assert empty == 2


# ---- 2. rows across the chunks of 256 voxels ----
@pytest.mark.parametrize("Gx", [255, 256, 257, 258])
def test_rows_that_meet_the_chunk_of_256_voxels(dev, hip_lib, Gx):
    """255: one chunk whose last thread has no voxel; 256: the last cube reads its +x corners from thread 255; 257 and 258: a second
    chunk of one and two cubes, whose first voxel was the last of the first chunk and is counted once."""
    dims = (Gx, 3, 3)
    T, Wt, C, origin, vs = noise_volume(dims, Gx)
    b, (rec, nrm, faces) = run_and_check(hip_lib, dev, dims, origin, vs, T, Wt, C, what=f"Gx={Gx}")
    assert len(faces) > 0 and faces.max() < len(rec)
    xs = MR.positions(rec)[faces.reshape(-1), 0]
    assert (xs > origin[0] + vs * 253).any()                      # faces of the cubes at the row's far end
    same_as_points(hip_lib, dev, dims, origin, vs, b, len(rec))


# ---- 3. the volumes whose row scans carry ----
@pytest.mark.parametrize("observed", ["a third unobserved", "all observed"])
@pytest.mark.parametrize("dims", list(R.POINTS_CHUNKED))
def test_volumes_whose_row_scans_carry(dev, hip_lib, dims, observed):
    """R.POINTS_CHUNKED: 256, 258 and 520 x-rows and 225, 170 and 475 rows of cubes, with points_volume(dims, 1) as it is and with
    every voxel observed (every cube valid: faces in the rows of cubes on both sides of the carry)."""
    T, Wt, C, origin, vs = R.points_volume(dims, 1)
    if observed == "all observed":
        rng = np.random.default_rng(5)
        T = np.where(Wt > 0, T, rng.uniform(-1, 1, T.shape)).astype(F)
        Wt = np.ones_like(Wt)
    else:
        assert len(MR.mesh(T, Wt, C, origin, vs)[0]) == R.POINTS_CHUNKED[dims]
    b, (rec, nrm, faces) = run_and_check(hip_lib, dev, dims, origin, vs, T, Wt, C, what=f"{dims} {observed}")
    print(f"{dims} {observed}: {len(rec)} vertices, {len(faces)} faces")
    assert len(faces) > 0
    same_as_points(hip_lib, dev, dims, origin, vs, b, len(rec))


# ---- 4. the data ----
def special_volume():
    dims = (33, 7, 9)
    T, Wt, C, origin, vs = noise_volume(dims, 11, holes=0.1)
    rng = np.random.default_rng(12)
    seen = np.flatnonzero(Wt.reshape(-1) > 0)
    pick = rng.choice(seen, size=60, replace=False)
    T.reshape(-1)[pick] = np.array([np.nan, np.inf, -np.inf, 0.0], F)[np.arange(60) % 4]
    return dims, T, Wt, C, origin, vs


@pytest.mark.parametrize("case", ["colour", "w_min", "no colour no normals", "misaligned"])
def test_special_values_holes_and_optional_arguments(dev, hip_lib, case):
    dims, T, Wt, C, origin, vs = special_volume()
    w_min = 1.5 if case == "w_min" else 0.0
    if case == "no colour no normals":
        C = None
    rec, nrm, faces = MR.mesh(T, Wt, C, origin, vs, w_min)
    n, m = len(rec), len(faces)
    assert m > 0 and np.isnan(T[Wt > 0]).any() and np.isinf(T).any() and (T[Wt > 0] == 0).any() and (Wt == 0).any()
    if case == "w_min":
        assert n < len(MR.mesh(T, Wt, C, origin, vs)[0])            # the weights of 1 are blinded
    put = (lambda a: misaligned(a, dev)) if case == "misaligned" else (lambda a: cu(a, dev))
    b = buffers(dev, dims, n, m, put, T, Wt, C)
    if case == "misaligned":
        assert b["T"].data_ptr() % 16 == 4 and b["Wt"].data_ptr() % 16 == 4
    if case == "no colour no normals":
        b["vnormals"] = None
    raw_mesh(hip_lib, dev, b, grid(dims, origin, vs), n, m, w_min)
    assert b["counts"].tolist() == [n, m]
    guarded.assert_bits(b["faces"][:m], faces, case + " faces")
    print(f"{case}: {n} vertices, {m} faces, {int(np.isnan(MR.positions(rec)).sum())} NaN coordinates (an infinite Ta: inf / inf)")
    guarded.assert_bits(b["points"][:n], rec, case + " points")
    if b["vnormals"] is not None:
        guarded.assert_bits(b["vnormals"][:n], nrm, case + " normals")
    assert (b["faces"][m:] == FACE_FILL).all() and (b["points"][n:] == 0xA5).all()
    same_as_points(hip_lib, dev, dims, origin, vs, b, n, w_min)


def test_an_empty_volume(dev, hip_lib):
    dims = (33, 4, 5)
    T, Wt, C, origin, vs = noise_volume(dims, 2)
    b = buffers(dev, dims, 4, 4, lambda a: cu(a, dev), T, np.zeros_like(Wt), C)
    raw_mesh(hip_lib, dev, b, grid(dims, origin, vs), 4, 4)
    assert b["counts"].tolist() == [0, 0] and (b["points"] == 0xA5).all() and (b["faces"] == FACE_FILL).all()


# ---- 5. the capacities ----
def test_capacities(dev, hip_lib):
    dims = (65, 7, 9)
    T, Wt, C, origin, vs = noise_volume(dims, 3)
    rec, nrm, faces = MR.mesh(T, Wt, C, origin, vs)
    n, m = len(rec), len(faces)
    g = grid(dims, origin, vs)
    for cap in (1, m // 3, m - 1):                            # fewer faces than there are: the exact prefix, nothing behind it
        b = buffers(dev, dims, n, cap, lambda a: cu(a, dev), T, Wt, C)
        raw_mesh(hip_lib, dev, b, g, n, cap)
        assert b["counts"].tolist() == [n, m]
        guarded.assert_bits(b["faces"][:cap], faces[:cap], f"the first {cap} faces")
        assert (b["faces"][cap:] == FACE_FILL).all()
        guarded.assert_bits(b["points"][:n], rec, "points")
    for cap in (1, n // 3, n - 1):                            # fewer records than vertices: the prefix of the points, no face at all
        b = buffers(dev, dims, cap, m, lambda a: cu(a, dev), T, Wt, C)
        raw_mesh(hip_lib, dev, b, g, cap, m)
        assert b["counts"].tolist() == [n, m]
        guarded.assert_bits(b["points"][:cap], rec[:cap], f"the first {cap} records")
        guarded.assert_bits(b["vnormals"][:cap], nrm[:cap], f"the first {cap} normals")
        assert (b["points"][cap:] == 0xA5).all() and (b["vnormals"][cap:] == 7.0).all() and (b["faces"] == FACE_FILL).all()
    b = buffers(dev, dims, n, m, lambda a: cu(a, dev), T, Wt, C)            # max_points == the vertices: they fit
    raw_mesh(hip_lib, dev, b, g, n, m)
    guarded.assert_bits(b["faces"][:m], faces, "faces at the exact capacities")


# ---- 6. the memory contract ----
@pytest.mark.parametrize("word", guarded.FLOAT_WORDS, ids=guarded.word_id)
def test_memory_contract(dev, hip_lib, word):
    """Every buffer between poisoned flanks, the outputs and the workspace poisoned inside; T holds the poison word and C 0xFF
    wherever Wt == 0.  Two runs give the same bytes."""
    dims = (65, 7, 9)
    T, Wt, C, origin, vs = noise_volume(dims, 4, holes=0.1)
    T = np.where(Wt > 0, T, np.array([word], np.uint32).view(F)[0]).astype(F)
    rec, nrm, faces = MR.mesh(T, Wt, C, origin, vs)
    n, m = len(rec), len(faces)
    assert n > 0 and m > 0
    from lwsnet_amd import _lib
    nb = _lib.nbytes("lws_tsdf_mesh_workspace", dims[1], dims[2])
    runs = []
    for _ in range(2):
        gd = guarded.Guard(dev, word, skew=1)
        b = dict(T=gd.place(T, name="T"), Wt=gd.place(Wt, name="Wt"), C=put_colour(C, lambda a, name: gd.place(a, name=name)),
                 work=gd.empty((nb // 8,), np.int64, align16=True, name="workspace"), points=gd.empty((n, 16), np.uint8, align16=True, name="points"),
                 vnormals=gd.empty((n, 4), F, align16=True, name="vnormals"), faces=gd.empty((m, 3), np.int32, name="faces"),
                 counts=gd.empty((2,), np.int64, align16=True, name="counts"))
        raw_mesh(hip_lib, dev, b, grid(dims, origin, vs), n, m)
        assert b["counts"].tolist() == [n, m]
        guarded.assert_bits(b["points"], rec, "guarded points")
        guarded.assert_bits(b["vnormals"], nrm, "guarded normals")
        guarded.assert_bits(b["faces"], faces, "guarded faces")
        gd.check()
        runs.append([b[k].cpu().numpy().tobytes() for k in ("points", "vnormals", "faces", "counts")])
    assert runs[0] == runs[1]


# ---- 7. the stream ----
def test_the_call_runs_on_the_stream_it_is_given(dev, hip_lib):
    """The "sequence" scenario of tests/test_gpu_stream_order.py restated for this call: the inputs and outputs hold poison, the
    caller's stream is stalled, the copies that bring the real volume are queued behind the stall and the call behind them.  The call
    returns while the stream is still held; read from another stream meanwhile, no output byte has changed; once the stall ends the
    outputs are the calm run's.  A kernel on another stream would have read the poisoned volume and written at once.  The reading
    stream may share a hardware queue with a caller stream and then waits for the stall itself: such a read shows nothing and is
    not judged, but on one caller stream at least it must fall inside the stall."""
    from test_gpu_stream_order import poison_, poisoned, still_poison
    dims = (33, 4, 5)
    T, Wt, C, origin, vs = noise_volume(dims, 1)
    rec, nrm, faces = MR.mesh(T, Wt, C, origin, vs)
    n, m = len(rec), len(faces)
    assert n > 0 and m > 0
    g = grid(dims, origin, vs)
    src = dict(T=cu(T, dev), Wt=cu(Wt, dev), C=put_colour(C, lambda a, name: cu(a, dev)))
    SS.ticks_per_ms(dev)
    calm = buffers(dev, dims, n, m, lambda a: cu(a, dev), T, Wt, C)
    raw_mesh(hip_lib, dev, calm, g, n, m)                   # calmly first: the kernels are loaded
    poison_(torch.empty_like(src["T"])).copy_(src["T"])
    poison_(torch.empty((8,), dtype=torch.uint8, device=dev)).clone()
    torch.cuda.synchronize()
    guarded.assert_bits(calm["faces"][:m], faces, "calm faces")
    names = ("points", "vnormals", "faces", "counts")
    other, seen_held = torch.cuda.Stream(device=dev), 0
    for i, s in enumerate(SS.caller_streams(dev)):
        b = {k: poisoned(v.shape, v.dtype, dev) for k, v in calm.items() if v is not None}
        torch.cuda.synchronize()
        with torch.cuda.device(dev), torch.cuda.stream(s):
            ev = SS.stall(s)
            for k in ("T", "Wt", "C"):
                b[k].copy_(src[k], non_blocking=True)
            for k in names + ("work",):
                poison_(b[k])
            raw_mesh(hip_lib, dev, b, g, n, m, st=ctypes.c_void_p(s.cuda_stream))
        SS.assert_still_stalled(ev, f"lws_tsdf_mesh on caller stream {i}")
        with torch.cuda.stream(other):
            early = [b[k].clone() for k in names]
            other.synchronize()
        if not ev.query():                                  # the read ran while the caller's stream was held: it saw the outputs of that time
            assert all(still_poison(e.cpu().numpy()) for e in early), f"caller stream {i}: an output changed while the stream was held"
            seen_held += 1
        s.synchronize()
        for k, count in (("points", n), ("vnormals", n), ("faces", m), ("counts", 2)):
            assert torch.equal(b[k][:count].view(torch.uint8), calm[k][:count].view(torch.uint8)), (i, k)
            assert still_poison(b[k][count:].cpu().numpy()), (i, k)
    assert seen_held > 0, "the reading stream shared a hardware queue with every caller stream: no read fell inside a stall"


# ---- 8. graph capture ----
def test_graph_capture_replays_on_two_input_sets(dev, hip_lib):
    dims = (65, 7, 9)
    first, second = noise_volume(dims, 6), noise_volume(dims, 7)
    origin, vs = first[3], first[4]
    cap_p, cap_f = 8192, 8192
    b = buffers(dev, dims, cap_p, cap_f, lambda a: cu(a, dev), *first[:3])
    g = grid(dims, origin, vs)
    raw_mesh(hip_lib, dev, b, g, cap_p, cap_f)              # the code objects are loaded before the capture
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_mesh(hip_lib, dev, b, g, cap_p, cap_f)
    for T, Wt, C, _, _ in (first, second, first):
        b["T"].copy_(cu(T, dev))
        b["Wt"].copy_(cu(Wt, dev))
        b["C"].copy_(put_colour(C, lambda a, name: cu(a, dev)))
        for k in ("work", "points", "vnormals", "faces", "counts"):
            b[k].fill_(77)
        graph.replay()
        torch.cuda.synchronize(dev)
        rec, nrm, faces = MR.mesh(T, Wt, C, origin, vs)
        assert b["counts"].tolist() == [len(rec), len(faces)] and 0 < len(rec) <= cap_p and 0 < len(faces) <= cap_f
        guarded.assert_bits(b["points"][:len(rec)], rec, "replay points")
        guarded.assert_bits(b["vnormals"][:len(rec)], nrm, "replay normals")
        guarded.assert_bits(b["faces"][:len(faces)], faces, "replay faces")


# ---- 9. the class ----
def test_volume_mesh_and_its_ply(dev, hip_lib, tmp_path):
    from lwsnet_amd.geometry import read_mesh_ply
    from lwsnet_amd.tsdf import TsdfVolume
    T, Wt = MR.sphere_volume()
    vol = TsdfVolume((0.0, 0.0, 0.0), MR.VS, (16, 16, 16), mu0=0.5, colour=True, device=dev)
    C = np.random.default_rng(9).integers(0, 256, (16, 16, 16, 4), dtype=np.uint8)
    vol.T.copy_(cu(T, dev))
    vol.Wt.copy_(cu(Wt, dev))
    vol.C.copy_(cu(C, dev))
    rec, nrm, faces = MR.mesh(T, Wt, C, (0.0, 0.0, 0.0), MR.VS)
    res = vol.mesh(4096, 4096)
    assert res.counts.tolist() == [len(rec), len(faces)] and res.faces.dtype == torch.int32 and res.faces.shape == (4096, 3)
    guarded.assert_bits(res.faces[:len(faces)], faces, "TsdfVolume.mesh faces")
    guarded.assert_bits(res.points[:len(rec)], rec, "TsdfVolume.mesh points")
    pts = vol.points(4096)
    assert torch.equal(pts.points[:len(rec)], res.points[:len(rec)]) and vol.mesh(4096, 4096, with_normals=False).vnormals is None
    path, cloud = tmp_path / "mesh.ply", tmp_path / "cloud.ply"
    assert vol.write_mesh_ply(str(path)) == (len(rec), len(faces)) and vol.write_ply(str(cloud)) == len(rec)
    verts, got = read_mesh_ply(str(path))
    assert np.array_equal(got, faces) and verts.tobytes() == read_mesh_ply(str(cloud))[0].tobytes()
    assert np.array_equal(guarded.as_bits(np.stack([verts["x"], verts["y"], verts["z"]], -1)), guarded.as_bits(MR.positions(rec)))
    with pytest.raises(ValueError, match="more than max_points"):
        vol.write_mesh_ply(str(tmp_path / "small.ply"), max_points=len(rec) - 1)
    with pytest.raises(ValueError, match="more than max_faces"):
        vol.write_mesh_ply(str(tmp_path / "small.ply"), max_faces=len(faces) - 1)
    assert not (tmp_path / "small.ply").exists()


# ---- 10. the CLI ----
def test_inference_cli_writes_the_mesh_of_the_points(dev, hip_lib, tmp_path, caplog, monkeypatch):
    """--tsdf over the synthetic sequence of tests/test_gpu_tsdf.py with both files: the mesh's vertices are the point file's, its
    faces those of TsdfVolume.mesh on the run's volume, the log names both counts."""
    import logging
    import re
    from lwsnet_amd import inference, sequence, synth
    from lwsnet_amd.geometry import read_mesh_ply
    from test_gpu_geometry import KITTI15_CALIB
    n = 3
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, n)
    calib = tmp_path / "calib.txt"
    calib.write_text(KITTI15_CALIB.format(fx=721.5377, cx=609.5593, cy=172.854, t3=44.85728 - 0.54 * 721.5377))
    pose_file = tmp_path / "poses.txt"
    pose_file.write_text("".join(" ".join(repr(float(v)) for v in TR.forward_pose(k + 1, 0.3, yaw=0.002).reshape(12)) + "\n" for k in range(n)))
    out, ply, mesh = tmp_path / "out", tmp_path / "a.ply", tmp_path / "m.ply"
    begun, real_begin = [], sequence.begin

    def begin(*args, **kw):
        begun.append(real_begin(*args, **kw))
        return begun[-1]
    monkeypatch.setattr(sequence, "begin", begin)
    with caplog.at_level(logging.INFO, logger="lwsnet_amd.inference"):
        written = inference.main(["--img_path", root + "/", "--synthetic_weights", "--calib", str(calib), "--occ_check", "1", "--save_path", str(out),
                                  "--tsdf", "--poses", str(pose_file), "--tsdf_voxel", "0.4", "--tsdf_extent", "-8", "8", "-3.2", "3.2", "0", "32",
                                  "--save_tsdf_ply", str(ply), "--save_tsdf_mesh", str(mesh)])
    assert written[-2:] == [str(ply), str(mesh)]
    lines = [r.getMessage() for r in caplog.records]
    logged = [(int(m[1]), int(m[2])) for m in (re.fullmatch(r"Save TSDF mesh = .*, vertices = (\d+), faces = (\d+)", line) for line in lines) if m]
    cloud, none = read_mesh_ply(str(ply))
    verts, faces = read_mesh_ply(str(mesh))
    assert logged == [(len(verts), len(faces))] and len(none) == 0 and len(faces) > 0
    assert verts.tobytes() == cloud.tobytes()
    volume = next(st.volume for st in begun[0][1] if hasattr(st, "volume"))
    res = volume.mesh(len(verts), len(faces))
    assert res.counts.tolist() == [len(verts), len(faces)]
    guarded.assert_bits(res.faces, faces, "the file's faces")
    assert faces.min() >= 0 and faces.max() < len(verts)
