"""Geometry outputs on the device: lws_depth_maps and lws_point_cloud bit for bit against the numpy restatement
(tests/geometry_reference.py), batch independence, real maps of the model and of forward_lr, and the inference CLI's
--save_disp16 / --save_depth / --save_ply files."""
import os

import numpy as np
import pytest

import geometry_reference as G

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, hip_lib):
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    return LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()


def cameras(B):
    from lwsnet_amd.geometry import Camera
    return [Camera(721.5377 + 10 * b, 721.5377 - 3 * b, 609.5593 - 10 - 7 * b, 172.854 - 7 + b, 0.5327 + 0.01 * b) for b in range(B)]


def cam_rows(cams):
    from lwsnet_amd.geometry import camera_rows
    return camera_rows(cams, len(cams))


def cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def misaligned(a, dev):
    """A contiguous device view of `a` whose data starts one element past a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a[:0].reshape(-1)).dtype, device=dev)
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(bits(got), bits(want)), f"{what}: {int((bits(got) != bits(want)).sum())} elements differ"


def maps(B, H, W, seed):
    """Disparities over 0 .. 200 with NaN, +-inf, negative, zero, tiny and huge values planted; a code map 0 / 1 / 2; RGB."""
    rng = np.random.default_rng(seed)
    d = (rng.random((B, 1, H, W)) * 200).astype(F)
    flat = d.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, -3.0, 0.0, 1e-30, 1e30, 0.999, 1.0, 0.5 / 256 + 1], F)
    idx = rng.choice(flat.size, size=min(flat.size, 10 * max(1, flat.size // 200)), replace=False)
    flat[idx] = special[np.arange(len(idx)) % len(special)]
    mask = rng.choice(np.array([0, 1, 1, 1, 2], np.uint8), size=d.shape)
    rgb = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    return d, mask, rgb


def check_point_cloud(points, counts, want_clouds, want_counts, what):
    assert_bits(counts, want_counts, what + " counts")
    p = points.cpu().numpy()
    for b, rec in enumerate(want_clouds):
        got = p[b, :len(rec)].reshape(-1).view(rec.dtype)
        assert np.array_equal(got.view(np.uint8), rec.view(np.uint8)), f"{what} image {b}: points differ"


@pytest.mark.parametrize("B,H,W", [(1, 368, 1232), (3, 63, 255), (2, 17, 1)])
def test_depth_maps_bitexact(dev, hip_lib, B, H, W):
    from lwsnet_amd import ops
    d, mask, _ = maps(B, H, W, B * W + H)
    cams = cameras(B)
    rows = cam_rows(cams)
    for m in (None, mask):
        for min_disp, max_depth in ((1.0, float("inf")), (0.25, 60.0)):
            what = f"B={B} {H}x{W} mask={m is not None} min_disp={min_disp} max_depth={max_depth}"
            want = G.depth_maps(d, m, rows, min_disp, max_depth)
            got = ops.depth_maps(cu(d, dev), cams, None if m is None else cu(m, dev), min_disp, max_depth)
            for k, name in enumerate(("depth", "depth16", "disp16")):
                assert_bits(got[k], want[k], f"{what} {name}")
            # each output alone, and disp16 without a camera
            only = ops.depth_maps(cu(d, dev), None, None if m is None else cu(m, dev), min_disp, max_depth, depth=False, depth16=False)
            assert only[0] is None and only[1] is None
            assert_bits(only[2], want[2], what + " disp16 alone")
            only = ops.depth_maps(cu(d, dev), cams, None if m is None else cu(m, dev), min_disp, max_depth, depth=False, disp16=False)
            assert_bits(only[1], want[1], what + " depth16 alone")


def test_depth_maps_misaligned_views(dev, hip_lib):
    from lwsnet_amd import ops
    B, H, W = 2, 31, 133
    d, mask, _ = maps(B, H, W, 5)
    cams = cameras(B)
    want = G.depth_maps(d, mask, cam_rows(cams), 1.0, 80.0)
    got = ops.depth_maps(misaligned(d, dev), cams, misaligned(mask, dev), 1.0, 80.0)
    for k, name in enumerate(("depth", "depth16", "disp16")):
        assert_bits(got[k], want[k], "misaligned " + name)
    # misaligned outputs through the C ABI
    import ctypes
    from lwsnet_amd import _lib
    dd, mm = cu(d, dev), cu(mask, dev)
    cam = cu(cam_rows(cams), dev)
    outs = [torch.empty(d.size + 1, dtype=dt, device=dev)[1:].view(d.shape) for dt in (torch.float32, torch.uint16, torch.uint16)]
    with torch.cuda.device(dev):
        _lib.check(hip_lib.lws_depth_maps(dd.data_ptr(), mm.data_ptr(), cam.data_ptr(), B, H, W, 1.0, 80.0, *[o.data_ptr() for o in outs],
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "lws_depth_maps")
    for k, name in enumerate(("depth", "depth16", "disp16")):
        assert_bits(outs[k], want[k], "misaligned output " + name)


@pytest.mark.parametrize("B,H,W", [(1, 368, 1232), (3, 63, 255), (1, 9, 1), (2, 5, 2111)])
def test_point_cloud_bitexact(dev, hip_lib, B, H, W):
    from lwsnet_amd import ops
    d, mask, rgb = maps(B, H, W, 3 * B + W)
    cams = cameras(B)
    rows = cam_rows(cams)
    for m in (None, mask):
        for c in (None, rgb):
            for min_disp, max_depth in ((1.0, float("inf")), (0.25, 60.0)):
                what = f"B={B} {H}x{W} mask={m is not None} rgb={c is not None} min_disp={min_disp} max_depth={max_depth}"
                clouds, counts = G.point_cloud(d, m, c, rows, min_disp, max_depth)
                points, n = ops.point_cloud(cu(d, dev), cams, None if m is None else cu(m, dev), None if c is None else cu(c, dev),
                                            min_disp, max_depth)
                assert points.shape == (B, H * W, 16) and n.dtype == torch.int64
                check_point_cloud(points, n, clouds, counts, what)
    # misaligned inputs
    clouds, counts = G.point_cloud(d, mask, rgb, rows, 1.0, 80.0)
    points, n = ops.point_cloud(misaligned(d, dev), cams, misaligned(mask, dev), misaligned(rgb, dev), 1.0, 80.0)
    check_point_cloud(points, n, clouds, counts, f"B={B} {H}x{W} misaligned")


def test_geometry_is_batch_independent(dev, hip_lib):
    from lwsnet_amd import ops
    B, H, W = 3, 40, 301
    d, mask, rgb = maps(B, H, W, 11)
    cams = cameras(B)
    batch_maps = ops.depth_maps(cu(d, dev), cams, cu(mask, dev), 1.0, 70.0)
    batch_pts, batch_n = ops.point_cloud(cu(d, dev), cams, cu(mask, dev), cu(rgb, dev), 1.0, 70.0)
    for b in range(B):
        alone_maps = ops.depth_maps(cu(d[b:b + 1], dev), cams[b], cu(mask[b:b + 1], dev), 1.0, 70.0)
        for k in range(3):
            assert_bits(batch_maps[k][b:b + 1], alone_maps[k].cpu().numpy(), f"image {b} map {k}")
        pts, n = ops.point_cloud(cu(d[b:b + 1], dev), cams[b], cu(mask[b:b + 1], dev), cu(rgb[b:b + 1], dev), 1.0, 70.0)
        assert int(n[0]) == int(batch_n[b])
        k = int(n[0])
        assert np.array_equal(pts[0, :k].cpu().numpy(), batch_pts[b, :k].cpu().numpy()), f"image {b} points"
    # the same image first of three, with other content around it
    d2, m2, c2 = maps(B, H, W, 12)
    d2[0], m2[0], c2[0] = d[2], mask[2], rgb[2]
    pts, n = ops.point_cloud(cu(d2, dev), [cams[2]] + cams[1:], cu(m2, dev), cu(c2, dev), 1.0, 70.0)
    k = int(batch_n[2])
    assert int(n[0]) == k and np.array_equal(pts[0, :k].cpu().numpy(), batch_pts[2, :k].cpu().numpy())


def test_geometry_of_model_maps(dev, model):
    """Real maps: the stage maps of model(...) at 1x368x1232 and forward_lr's checked maps with their code maps."""
    from lwsnet_amd import ops
    from lwsnet_amd.synth import make_pair
    left, right, _ = make_pair(368, 1232, 0)
    cams = cameras(1)
    rows = cam_rows(cams)
    rgb = np.ascontiguousarray(np.clip(np.rint((left.transpose(1, 2, 0) * 0.2 + 0.5) * 255), 0, 255).astype(np.uint8))[None]
    outs = model(left[None], right[None])
    res = model.forward_lr(left[None], right[None], tau=1.0, fill=False)
    for s in range(4):
        for what, disp, mask in ((f"model stage {s + 1}", outs[s], None), (f"forward_lr stage {s + 1}", res.disp[s], res.mask[s])):
            d = disp.numpy()
            m = None if mask is None else mask.cpu().numpy()
            want = G.depth_maps(d, m, rows, 1.0, 80.0)
            got = ops.depth_maps(disp, cams, mask, 1.0, 80.0)
            for k, name in enumerate(("depth", "depth16", "disp16")):
                assert_bits(got[k], want[k], f"{what} {name}")
            clouds, counts = G.point_cloud(d, m, rgb, rows, 1.0, 80.0)
            points, n = ops.point_cloud(disp, cams, mask, cu(rgb, dev), 1.0, 80.0)
            check_point_cloud(points, n, clouds, counts, what)
            assert counts[0] > 1000, (what, counts)


KITTI15_CALIB = """calib_time: 09-Jan-2012 13:57:47
corner_dist: 9.950000e-02
P_rect_02: {fx:.6e} 0.000000e+00 {cx:.6e} 4.485728e+01 0.000000e+00 {fx:.6e} {cy:.6e} 2.163791e-01 0.000000e+00 0.000000e+00 1.000000e+00 2.745884e-03
P_rect_03: {fx:.6e} 0.000000e+00 {cx:.6e} {t3:.6e} 0.000000e+00 {fx:.6e} {cy:.6e} 2.199936e+00 0.000000e+00 0.000000e+00 1.000000e+00 2.729905e-03
"""


def test_inference_cli_geometry_files(dev, model, tmp_path):
    from PIL import Image
    from lwsnet_amd import datasets as D
    from lwsnet_amd import imageio as io
    from lwsnet_amd import inference, synth
    from lwsnet_amd.geometry import Camera, read_ply
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, 2)
    calib = tmp_path / "kitti" / "calib_cam_to_cam"
    calib.mkdir()
    for i in range(2):
        fx = 721.5377 + 5 * i
        (calib / f"{i:06d}.txt").write_text(KITTI15_CALIB.format(fx=fx, cx=609.5593, cy=172.854, t3=44.85728 - 0.54 * fx))
    common = ["--img_path", root + "/", "--synthetic_weights", "--calib", str(calib), "--save_disp16", "--save_depth", "--save_ply"]
    out = tmp_path / "out"
    written = inference.main(common + ["--save_path", str(out)])
    names = sorted(os.listdir(out))
    assert names == sorted(f"{i:06d}_10{s}" for i in range(2) for s in (".png", "_disp16.png", "_depth16.png", ".ply"))
    assert len(written) == 8
    out_lr = tmp_path / "out_lr"
    inference.main(common + ["--save_path", str(out_lr), "--lr_check", "1"])
    ds = D.StereoPairs([], [], [], training=False, kitti_set=True)
    for i in range(2):
        stem = f"{i:06d}_10"
        full = io.load_rgb(os.path.join(root, "image_2", stem + ".png"))
        l_in = io.to_input(io.crop_bottom_right(full))[None]
        r_in = io.to_input(io.crop_bottom_right(io.load_rgb(os.path.join(root, "image_3", stem + ".png"))))[None]
        d4 = model(l_in, r_in)[3].numpy()
        cam = Camera.from_kitti(str(calib / f"{i:06d}.txt")).crop_bottom_right(*full.shape[:2])
        assert abs(cam.baseline - 0.54) < 1e-6 and cam.cx == 609.5593 - (full.shape[1] - 1232)
        # the disparity PNG, read back by the evaluation reader: rint(d * 256) / 256 of the stage-4 map
        got = ds._disparity(str(out / (stem + "_disp16.png")))
        ok = np.isfinite(d4[0, 0]) & (d4[0, 0] > 0)
        want = np.where(ok, np.minimum(np.rint(np.where(ok, d4[0, 0], 0) * F(256)), F(65535)) / F(256), F(0)).astype(F)
        assert np.array_equal(got, want)
        _, depth16, disp16 = G.depth_maps(d4, None, cam_rows([cam]), 1.0, float("inf"))
        assert np.array_equal(np.asarray(Image.open(out / (stem + "_depth16.png"))), depth16[0, 0])
        pts = read_ply(str(out / (stem + ".ply")))
        assert len(pts) == int((depth16 > 0).sum()) > 1000
        clouds, _ = G.point_cloud(d4, None, io.crop_bottom_right(full)[None], cam_rows([cam]), 1.0, float("inf"))
        assert np.array_equal(pts.view(np.uint8), clouds[0].view(np.uint8))
        # --lr_check 1 (no fill): only code-1 pixels
        res = model.forward_lr(l_in, r_in, tau=1.0, fill=False)
        code = res.mask[3].cpu().numpy()
        clouds, counts = G.point_cloud(res.disp[3].numpy(), code, io.crop_bottom_right(full)[None], cam_rows([cam]), 1.0, float("inf"))
        pts_lr = read_ply(str(out_lr / (stem + ".ply")))
        assert np.array_equal(pts_lr.view(np.uint8), clouds[0].view(np.uint8))
        assert 0 < len(pts_lr) <= int((code == 1).sum()) and len(pts_lr) < len(pts)
        d16_lr = np.asarray(Image.open(out_lr / (stem + "_disp16.png")))
        assert np.all(d16_lr[code[0, 0] != 1] == 0)
