"""Surface normals and the triangle mesh on the device: lws_surface_normals and lws_surface_mesh bit for bit against the numpy
restatement (tests/mesh_reference.py) at the smallest shapes that reach each path -- no cells, one cell, partial tiles, ragged
rows, more than one 256-quad chunk per row, more than 256 rows -- and once at full size; views one element past a 16-byte
boundary, batch independence, poisoned guard bands, a captured graph, real maps of the model and the inference CLI's files."""
import ctypes
import os

import numpy as np
import pytest

import guarded
import mesh_reference as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_geometry import KITTI15_CALIB, assert_bits, cam_rows, cameras, cu, misaligned  # noqa: E402

F = np.float32
INF = float("inf")
SPECIAL = np.array([np.nan, np.inf, -np.inf, -3.0, 0.0, 1e-30, 1e30, 0.999], F)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, hip_lib):
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    return LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()


def scene(B, H, W, seed, plain=False):
    """A smooth scene -- a tilted plane with a 7.5-px step down the middle and a second plane patch -- with about 2.5 % special
    values planted, a code map with about 25 % non-1 codes, and RGB.  plain: one tilted plane, neither specials nor codes other than 1."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.empty((B, 1, H, W), F)
    for b in range(B):
        img = 40.0 + 3.0 * b + 0.11 * xs - 0.07 * ys + (0.0 if plain else 7.5) * (xs >= W // 2)
        patch = (ys >= H // 4) & (ys < H // 2 + 1) & (xs >= W // 8) & (xs < W // 3 + 1) & (not plain)
        d[b, 0] = np.where(patch, 25.0 - 0.05 * xs + 0.2 * ys, img).astype(F)
    mask = rng.choice(np.array([0, 1, 1, 1, 1, 1, 1, 2], np.uint8), size=d.shape)
    if plain:
        mask[:] = 1
    else:
        flat = d.reshape(-1)
        idx = rng.choice(flat.size, size=max(1, flat.size // 40), replace=False)
        flat[idx] = SPECIAL[np.arange(len(idx)) % len(SPECIAL)]
    rgb = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    return d, mask, rgb


_REF = {}


def reference(key, d, m, c, rows, min_disp, max_depth, max_jump):
    """The restatement of one case, computed once and shared: (normals, quadrant counts, normals8, mesh)."""
    if key not in _REF:
        n, nq = M.surface_normals(d, m, rows, min_disp, max_depth, max_jump)
        _REF[key] = (n, nq, M.normals8(n), M.surface_mesh(d, m, c, rows, n, min_disp, max_depth, max_jump))
    return _REF[key]


def check_mesh(mesh, want, what, normals=True, index=True):
    clouds, vn, faces, idx, counts = want
    assert_bits(mesh.counts, counts, what + " counts")
    p, f = mesh.points.cpu().numpy(), mesh.faces.cpu().numpy()
    v = mesh.vnormals.cpu().numpy() if normals else None
    assert (mesh.vnormals is None) == (not normals) and (mesh.index is None) == (not index), what
    for b, rec in enumerate(clouds):
        got = p[b, :len(rec)].reshape(-1).view(rec.dtype)
        assert np.array_equal(got.view(np.uint8), rec.view(np.uint8)), f"{what} image {b}: points differ"
        assert_bits(f[b, :len(faces[b])], faces[b], f"{what} image {b} faces")
        if normals:
            assert_bits(v[b, :len(rec)], vn[b], f"{what} image {b} vnormals")
    if index:
        assert_bits(mesh.index, idx, what + " index")


def covers_every_case(d, m, rows, max_jump=1.0):
    """Every quadrant count 0, 1, 2, 4 and all four faces -- T0 and T1 on either diagonal -- occur in the restatement."""
    _, nq = M.surface_normals(d, m, rows, 1.0, INF, max_jump)
    de, _ = M.effective(d, m, rows, 1.0, INF)
    t0, t1, ae = M.cell_faces(de, max_jump)
    seen = (sorted(np.unique(nq).tolist()), bool((t0 & ~ae).any()), bool((t1 & ~ae).any()), bool((t0 & ae).any()), bool((t1 & ae).any()))
    return seen == ([0, 1, 2, 4], True, True, True, True), seen


SHAPES = [(1, 1, 1), (2, 17, 1), (1, 1, 9),         # no cells, zero faces
          (1, 2, 2),                                # the smallest cell (all valid)
          (1, 18, 131),                             # partial tiles both ways
          (3, 63, 255),                             # ragged, rows not 16-byte aligned, batch offsets
          (1, 5, 1029),                             # more than one 256-quad chunk per row: the carry across chunks in the ranks
          (1, 259, 6),                              # more than 256 rows: the carry in the scan
          (1, 368, 1232)]                           # one full-size case
COVERING = [(1, 18, 131), (3, 63, 255), (1, 5, 1029), (1, 259, 6)]


@pytest.mark.parametrize("B,H,W", COVERING)
def test_inputs_reach_every_case(B, H, W):
    d, mask, _ = scene(B, H, W, 7 * B + H + W)
    ok, seen = covers_every_case(d, mask, cam_rows(cameras(B)))
    assert ok, seen


@pytest.mark.parametrize("max_jump", [0.0, 1.0, 1e30])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_normals_and_mesh_bitexact(dev, hip_lib, B, H, W, max_jump):
    from lwsnet_amd import ops
    plain = (B, H, W) == (1, 2, 2)
    d, mask, rgb = scene(B, H, W, 7 * B + H + W, plain=plain)
    cams = cameras(B)
    rows = cam_rows(cams)
    if (B, H, W) in COVERING:
        ok, seen = covers_every_case(d, mask, rows)
        assert ok, seen
    for m in (None, mask):
        for min_disp, max_depth in ((1.0, INF), (0.25, 60.0)):
            c = rgb if m is not None else None
            what = f"B={B} {H}x{W} mask={m is not None} min_disp={min_disp} max_depth={max_depth} max_jump={max_jump}"
            n, _, n8, want = reference((B, H, W, m is not None, min_disp, max_jump), d, m, c, rows, min_disp, max_depth, max_jump)
            dm, mm, cc = cu(d, dev), None if m is None else cu(m, dev), None if c is None else cu(c, dev)
            got_n, got_8 = ops.surface_normals(dm, cams, mm, min_disp, max_depth, max_jump, normals=True, normals8=True)
            assert_bits(got_n, n, what + " normals")
            assert_bits(got_8, n8, what + " normals8")
            mesh = ops.surface_mesh(dm, cams, mm, cc, min_disp, max_depth, max_jump, with_normals=True, want_index=True)
            assert mesh.points.shape == (B, H * W, 16) and mesh.faces.shape == (B, max(1, 2 * (H - 1) * (W - 1)), 3)
            check_mesh(mesh, want, what)
            if plain:
                assert want[4].tolist() == [[4, 2 if max_jump >= 1.0 else 0]]
            # each optional output alone
            only = ops.surface_normals(dm, cams, mm, min_disp, max_depth, max_jump, normals=False, normals8=True)
            assert only[0] is None
            assert_bits(only[1], n8, what + " normals8 alone")
            only = ops.surface_normals(dm, cams, mm, min_disp, max_depth, max_jump)
            assert only[1] is None
            assert_bits(only[0], n, what + " normals alone")
            check_mesh(ops.surface_mesh(dm, cams, mm, cc, min_disp, max_depth, max_jump, with_normals=False), want, what + " bare",
                       normals=False, index=False)
            check_mesh(ops.surface_mesh(dm, cams, mm, cc, min_disp, max_depth, max_jump, with_normals=False, want_index=True), want,
                       what + " index alone", normals=False)
            check_mesh(ops.surface_mesh(dm, cams, mm, cc, min_disp, max_depth, max_jump), want, what + " vnormals alone", index=False)


# ---- the C ABI with the caller's buffers ----
def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_normals(lib, dev, disp, mask, cam, shape, args, normals, normals8):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_surface_normals(P(disp), P(mask), P(cam), *shape, *args, P(normals), P(normals8), stream()), "lws_surface_normals")


def raw_mesh(lib, dev, disp, mask, rgb, cam, normals, shape, args, work, points, vnormals, faces, index, counts):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_surface_mesh(P(disp), P(mask), P(rgb), P(cam), P(normals), *shape, *args, P(work), P(points), P(vnormals),
                                        P(faces), P(index), P(counts), stream()), "lws_surface_mesh")


def skewed(shape, dtype, dev):
    """An uninitialised contiguous device tensor whose data starts one element past a 16-byte boundary."""
    n = int(np.prod(shape))
    v = torch.empty(n + 1, dtype=dtype, device=dev)[1:].view(shape)
    assert v.data_ptr() % 16 != 0
    return v


def test_misaligned_views(dev, hip_lib):
    from lwsnet_amd import ops
    B, H, W = 2, 31, 133
    d, mask, rgb = scene(B, H, W, 5)
    cams = cameras(B)
    rows = cam_rows(cams)
    args = (1.0, 80.0, 1.0)
    n, _, n8, want = reference(("misaligned",), d, mask, rgb, rows, *args)
    # misaligned inputs through ops
    got = ops.surface_normals(misaligned(d, dev), cams, misaligned(mask, dev), *args, normals=True, normals8=True)
    assert_bits(got[0], n, "misaligned inputs normals")
    assert_bits(got[1], n8, "misaligned inputs normals8")
    check_mesh(ops.surface_mesh(misaligned(d, dev), cams, misaligned(mask, dev), misaligned(rgb, dev), *args, want_index=True), want,
               "misaligned inputs")
    # every map one element past a 16-byte boundary through the C ABI (points and vnormals are 16-byte records)
    dd, mm, cc, cam = misaligned(d, dev), misaligned(mask, dev), misaligned(rgb, dev), misaligned(rows, dev)
    on, o8 = skewed((B, 3, H, W), torch.float32, dev), skewed((B, H, W, 3), torch.uint8, dev)
    raw_normals(hip_lib, dev, dd, mm, cam, (B, H, W), args, on, o8)
    assert_bits(on, n, "misaligned output normals")
    assert_bits(o8, n8, "misaligned output normals8")
    work = skewed((int(hip_lib.lws_surface_mesh_workspace(B, H)) // 4,), torch.int32, dev)
    points = torch.empty((B, H * W, 16), dtype=torch.uint8, device=dev)
    vn = torch.empty((B, H * W, 4), dtype=torch.float32, device=dev)
    faces, index = skewed((B, 2 * (H - 1) * (W - 1), 3), torch.int32, dev), skewed((B, 1, H, W), torch.int32, dev)
    counts = torch.empty((B, 2), dtype=torch.int64, device=dev)
    raw_mesh(hip_lib, dev, dd, mm, cc, cam, on, (B, H, W), args, work, points, vn, faces, index, counts)
    check_mesh(ops.SurfaceMesh(points, vn, faces, index, counts), want, "misaligned outputs")


def test_surfaces_are_batch_independent(dev, hip_lib):
    from lwsnet_amd import ops
    B, H, W = 3, 40, 301
    d, mask, rgb = scene(B, H, W, 11)
    cams = cameras(B)
    args = (1.0, 70.0, 1.0)

    def run(d, mask, rgb, cams):
        n, n8 = ops.surface_normals(cu(d, dev), cams, cu(mask, dev), *args, normals=True, normals8=True)
        return n.cpu().numpy(), n8.cpu().numpy(), ops.surface_mesh(cu(d, dev), cams, cu(mask, dev), cu(rgb, dev), *args, want_index=True)

    def same(got, b, ref, rb, what):
        assert_bits(got[0][b], ref[0][rb], what + " normals")
        assert_bits(got[1][b], ref[1][rb], what + " normals8")
        gm, rm = got[2], ref[2]
        nv, nf = (int(v) for v in rm.counts[rb].cpu())
        assert gm.counts[b].cpu().tolist() == [nv, nf] and nv > 0 and nf > 0
        for name, k in (("points", nv), ("vnormals", nv), ("faces", nf)):
            assert torch.equal(getattr(gm, name)[b, :k], getattr(rm, name)[rb, :k]), f"{what} {name}"
        assert torch.equal(gm.index[b], rm.index[rb]), what + " index"

    batch = run(d, mask, rgb, cams)
    for b in range(B):
        same(run(d[b:b + 1], mask[b:b + 1], rgb[b:b + 1], cams[b]), 0, batch, b, f"image {b} alone")
    # the last image first of three, with other content around it
    d2, m2, c2 = scene(B, H, W, 12)
    d2[0], m2[0], c2[0] = d[2], mask[2], rgb[2]
    same(run(d2, m2, c2, [cams[2]] + cams[1:]), 0, batch, 2, "image 2 moved to the front")


WORDS = pytest.mark.parametrize("word", guarded.FLOAT_WORDS, ids=guarded.word_id)


@WORDS
@pytest.mark.parametrize("full", [True, False], ids=["mask+rgb+normals+index", "plain"])
def test_memory_contract(dev, hip_lib, full, word):
    """Inputs and outputs between poisoned flanks, the workspace poisoned: nothing outside the outputs changes, every element the
    header promises is written, and the records past counts[b] still hold the poison."""
    B, H, W = 2, 19, 133
    d_np, mask_np, rgb_np = scene(B, H, W, 8)
    rows = cam_rows(cameras(B))
    args = (1.0, 80.0, 1.0)
    m_np, c_np = (mask_np, rgb_np) if full else (None, None)
    n_np, _, n8_np, want = reference(("contract", full), d_np, m_np, c_np, rows, *args)
    g = guarded.Guard(dev, word, skew=1)
    disp, cam = g.place(d_np, name="disp"), g.place(rows, name="cam")
    mask = g.place(m_np, word=guarded.MASK_WORD, name="mask") if full else None
    rgb = g.place(c_np, plane=H * W * 3, name="rgb") if full else None
    normals = g.empty((B, 3, H, W), np.float32, name="normals")
    normals8 = g.empty((B, H, W, 3), np.uint8, plane=H * W * 3, name="normals8") if full else None
    raw_normals(hip_lib, dev, disp, mask, cam, (B, H, W), args, normals, normals8)
    guarded.assert_bits(normals, n_np, "normals")
    if full:
        guarded.assert_bits(normals8, n8_np, "normals8")
    nbytes = int(hip_lib.lws_surface_mesh_workspace(B, H))
    assert nbytes > 0
    work = g.empty((nbytes,), np.uint8, align16=True, word=word, name="workspace")
    points = g.empty((B, H * W, 16), np.uint8, plane=H * W * 16, align16=True, word=word, name="points")
    vn = g.empty((B, H * W, 4), np.float32, plane=H * W * 4, align16=True, name="vnormals") if full else None
    faces = g.empty((B, 2 * (H - 1) * (W - 1), 3), np.int32, plane=6 * H * W, name="faces")
    index = g.empty((B, 1, H, W), np.int32, name="index") if full else None
    counts = g.empty((B, 2), np.int64, name="counts")
    raw_mesh(hip_lib, dev, disp, mask, rgb, cam, normals if full else None, (B, H, W), args, work, points, vn, faces, index, counts)
    check_mesh(ops_mesh(points, vn, faces, index, counts), want, "guarded", normals=full, index=full)
    p, f = points.cpu().numpy(), faces.cpu().numpy()
    for b in range(B):
        nv, nf = (int(v) for v in want[4][b])
        assert 0 < nv < H * W and 0 < nf < 2 * (H - 1) * (W - 1), "the inputs should leave both records and room behind them"
        assert (p[b, nv:].reshape(-1).view(np.uint32) == word).all(), f"image {b}: points past counts[b] were written"
        assert (f[b, nf:].reshape(-1).view(np.uint32) == guarded.BYTE_WORD).all(), f"image {b}: faces past counts[b] were written"
        if full:
            assert (vn[b, nv:].cpu().numpy().reshape(-1).view(np.uint32) == word).all(), f"image {b}: vnormals past counts[b] were written"
    g.check()


def ops_mesh(points, vn, faces, index, counts):
    from lwsnet_amd import ops
    return ops.SurfaceMesh(points, vn, faces, index, counts)


def test_graph_capture_replays_both_calls(dev, hip_lib):
    from lwsnet_amd import ops
    B, H, W = 2, 37, 301
    cams = cameras(B)
    rows = cam_rows(cams)
    args = (1.0, 80.0, 1.0)
    first, second = scene(B, H, W, 21), scene(B, H, W, 22)
    d, m, c, cam = cu(first[0], dev), cu(first[1], dev), cu(first[2], dev), cu(rows, dev)
    n = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    n8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    work = torch.empty((int(hip_lib.lws_surface_mesh_workspace(B, H)),), dtype=torch.uint8, device=dev)
    points = torch.empty((B, H * W, 16), dtype=torch.uint8, device=dev)
    vn = torch.empty((B, H * W, 4), dtype=torch.float32, device=dev)
    faces = torch.empty((B, 2 * (H - 1) * (W - 1), 3), dtype=torch.int32, device=dev)
    index = torch.empty((B, 1, H, W), dtype=torch.int32, device=dev)
    counts = torch.empty((B, 2), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                           # one stream: the capture stream
        raw_normals(hip_lib, dev, d, m, cam, (B, H, W), args, n, n8)
        raw_mesh(hip_lib, dev, d, m, c, cam, n, (B, H, W), args, work, points, vn, faces, index, counts)
    for d_np, m_np, c_np in (first, second):
        d.copy_(cu(d_np, dev))
        m.copy_(cu(m_np, dev))
        c.copy_(cu(c_np, dev))
        graph.replay()
        torch.cuda.synchronize(dev)
        en, e8 = ops.surface_normals(cu(d_np, dev), cams, cu(m_np, dev), *args, normals=True, normals8=True)
        eager = ops.surface_mesh(cu(d_np, dev), cams, cu(m_np, dev), cu(c_np, dev), *args, want_index=True)
        assert torch.equal(n.view(torch.int32), en.view(torch.int32)) and torch.equal(n8, e8), "replay normals"
        assert torch.equal(counts, eager.counts) and torch.equal(index, eager.index), "replay counts / index"
        for b in range(B):
            nv, nf = (int(v) for v in counts[b].cpu())
            assert nv > 0 and nf > 0
            assert torch.equal(points[b, :nv], eager.points[b, :nv]) and torch.equal(faces[b, :nf], eager.faces[b, :nf])
            assert torch.equal(vn[b, :nv].view(torch.int32), eager.vnormals[b, :nv].view(torch.int32))
        wn, _, w8, want = reference(("graph", d_np is first[0]), d_np, m_np, c_np, rows, *args)
        assert_bits(n, wn, "replay normals against the reference")
        assert_bits(n8, w8, "replay normals8 against the reference")
        check_mesh(ops_mesh(points, vn, faces, index, counts), want, "replay against the reference")


def test_mesh_of_model_maps(dev, model):
    """Real maps: the seeded model at 64 x 256 behind forward_occ, each stage with its code map."""
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import Camera
    from lwsnet_amd.synth import make_pair
    H, W = 64, 256
    left, right = (a[None] for a in make_pair(H, W, 0)[:2])
    rgb = np.ascontiguousarray(np.clip(np.rint((left[0].transpose(1, 2, 0) * 0.2 + 0.5) * 255), 0, 255).astype(np.uint8))[None]
    cams = [Camera(721.5, 721.5, 127.5, 31.5, 0.54)]
    rows = cam_rows(cams)
    res = model.forward_occ(left, right, tau=1.0, fill=False)
    for s in range(4):
        d, m = res.disp[s].numpy(), res.mask[s].cpu().numpy()
        n, _ = M.surface_normals(d, m, rows, 1.0, INF, 1.0)
        want = M.surface_mesh(d, m, rgb, rows, n, 1.0, INF, 1.0)
        mesh = ops.surface_mesh(res.disp[s], cams, res.mask[s], cu(rgb, dev), want_index=True)
        check_mesh(mesh, want, f"forward_occ stage {s + 1}")
        got_n, got_8 = ops.surface_normals(res.disp[s], cams, res.mask[s], normals=True, normals8=True)
        assert_bits(got_n, n, f"forward_occ stage {s + 1} normals")
        assert_bits(got_8, M.normals8(n), f"forward_occ stage {s + 1} normals8")
        print(f"forward_occ stage {s + 1}: vertices, faces = {want[4][0].tolist()}")
        assert want[4][0, 0] > 100


def test_inference_cli_surface_files(dev, model, tmp_path):
    from PIL import Image
    from lwsnet_amd import imageio as io
    from lwsnet_amd import inference, ops, synth
    from lwsnet_amd.geometry import POINT_DTYPE, Camera, read_mesh_ply
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, 1)
    calib = tmp_path / "000000.txt"
    calib.write_text(KITTI15_CALIB.format(fx=721.5377, cx=609.5593, cy=172.854, t3=44.85728 - 0.54 * 721.5377))
    common = ["--img_path", root + "/", "--synthetic_weights", "--calib", str(calib), "--occ_check", "1", "--save_ply"]
    plain, out = tmp_path / "plain", tmp_path / "out"
    inference.main(common + ["--save_path", str(plain)])
    written = inference.main(common + ["--save_path", str(out), "--save_normals", "--save_mesh", "--max_jump", "1.5"])
    stem = "000000_10"
    assert sorted(os.listdir(out)) == sorted(stem + s for s in (".png", "_occ.png", ".ply", "_normals.png", "_mesh.ply"))
    assert len(written) == 5
    assert (out / (stem + ".ply")).read_bytes() == (plain / (stem + ".ply")).read_bytes()
    full = io.load_rgb(os.path.join(root, "image_2", stem + ".png"))
    left = io.crop_bottom_right(full)
    l_in = io.to_input(left)[None]
    r_in = io.to_input(io.crop_bottom_right(io.load_rgb(os.path.join(root, "image_3", stem + ".png"))))[None]
    cam = Camera.from_kitti(str(calib)).crop_bottom_right(*full.shape[:2])
    res = model.forward_occ(l_in, r_in, tau=1.0, fill=False)
    mesh = ops.surface_mesh(res.disp[3], cam, res.mask[3], cu(left[None], dev), max_jump=1.5)
    nv, nf = (int(v) for v in mesh.counts[0].cpu())
    assert nv > 1000 and nf > 100
    verts, faces = read_mesh_ply(str(out / (stem + "_mesh.ply")))
    pts = mesh.points[0, :nv].cpu().numpy().reshape(-1).view(POINT_DTYPE)
    for name in POINT_DTYPE.names:
        assert np.array_equal(guarded.as_bits(verts[name]), guarded.as_bits(pts[name])), name
    vn = mesh.vnormals[0, :nv].cpu().numpy()
    for k, name in enumerate(("nx", "ny", "nz")):
        assert np.array_equal(guarded.as_bits(verts[name]), guarded.as_bits(vn[:, k])), name
    assert np.array_equal(faces, mesh.faces[0, :nf].cpu().numpy())
    _, n8 = ops.surface_normals(res.disp[3], cam, res.mask[3], max_jump=1.5, normals=False, normals8=True)
    assert np.array_equal(np.asarray(Image.open(out / (stem + "_normals.png"))), n8[0].cpu().numpy())
