"""The rectifying front end on the device: every output of lws_rectify_pair bit for bit against the numpy restatement
(tests/rectify_reference.py) on strongly distorted records, on window sizes around the kernel's tile edges, on single rows and
columns, with Wc crossing zero and on the golden KITTI pair; each optional output alone, the input planes against
ops.preprocess_rgb8, batch independence, run-to-run identity, hipGraph capture, guard bands and poisoned outputs, the chain
rectify_pair -> forward -> wmedian_filter -> point_cloud, and the --rectify flag of the inference CLI.

The kernel's tile is TILE_H x TILE_W output pixels per workgroup, one wave per row; the constants are read from its source."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest

import geometry_reference as GEO
import guarded as G
import rectify_reference as R
import wmedian_reference as WM
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _kernel_constant(name):
    src = open(os.path.join(ROOT, "lwsnet_amd", "csrc", "lws_rectify.hip")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))


TILE_H, TILE_W = _kernel_constant("kTH"), _kernel_constant("kTW")
KEYS = ("rect", "input", "valid", "map")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, hip_lib):
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    return LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()


def cu(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def raw_images(B, Hs, Ws, seed):
    """Random uint8 images; the right image of the first pair is a smooth ramp (a blend of equal taps hides a wrong weight)."""
    rng = np.random.default_rng(seed)
    left, right = (rng.integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8) for _ in range(2))
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    right[0] = np.stack([(3 * xx + yy) % 256, (2 * yy + xx) % 256, (xx + 5 * yy) % 256], axis=-1).astype(np.uint8)
    return left, right


def records(B, Hs, Ws, H, W, y0, x0, seed, k1=1.2):
    """params [B,2,18], a different strongly distorted record per image and camera: the rectified window looks at the middle of the
    raw image through a small random rotation, and a pincushion k1 > 0 throws the corners of the window outside the raw image."""
    from lwsnet_amd.geometry import _rodrigues
    rng = np.random.default_rng(seed)
    out = np.empty((B, 2, 18), np.float32)
    f = 0.85 * max(W, 32)
    for b in range(B):
        for c in range(2):
            knew = np.array([[f, 0, x0 + 0.5 * W + rng.uniform(-2, 2)], [0, f * rng.uniform(0.95, 1.05), y0 + 0.5 * H + rng.uniform(-2, 2)],
                             [0, 0, 1.0]])
            inv = np.linalg.inv(knew @ _rodrigues(rng.uniform(-0.03, 0.03, 3)))
            fr = f * rng.uniform(0.9, 1.1)
            out[b, c] = np.concatenate([inv.reshape(-1), [fr, fr * rng.uniform(0.97, 1.03), 0.5 * Ws + rng.uniform(-3, 3),
                                                          0.5 * Hs + rng.uniform(-3, 3)],
                                        [k1 * rng.uniform(0.8, 1.2), rng.uniform(-0.3, 0.3), rng.uniform(-0.03, 0.03),
                                         rng.uniform(-0.03, 0.03), rng.uniform(-0.1, 0.1)]])
    return out


def run(dev, raw, params, hw, origin=(0, 0), border=0, **want):
    from lwsnet_amd import ops
    want = want or dict(want_rect=True, want_input=True, want_valid=True, want_map=True)
    return ops.rectify_pair(cu(raw[0], dev), cu(raw[1], dev), params, hw, origin=origin, border=border, **want)


def assert_outputs(got, want, what, keys=KEYS):
    for key in keys:
        for c in range(2):
            g = got[key][c].cpu().numpy()
            w = want[key][c]
            if key == "map":                                # a NaN is some NaN (include/lwsnet_hip.h)
                g, w = R.canonical_nans(g), R.canonical_nans(w)
            G.assert_bits(g, w, f"{what} {key}[{c}]")


@pytest.mark.parametrize("border", [0, 200])
def test_bitexact_on_strongly_distorted_records(dev, hip_lib, border):
    B, Hs, Ws, (H, W), origin = 2, 37, 53, (29, 45), (3, 2)
    raw, params = raw_images(B, Hs, Ws, 1), records(B, Hs, Ws, H, W, *origin, seed=2)
    want = R.rectify_reference(raw, params, (H, W), origin, border)
    for c in range(2):
        v = want["valid"][c]
        print(f"camera {c}: {int(v.sum())} of {v.size} pixels valid")
        assert v.any() and not v.all(), "both valid and invalid pixels must occur, or the border path is not run"
    assert_outputs(run(dev, raw, params, (H, W), origin, border), want, f"border={border}")


@pytest.mark.parametrize("H,W", [(TILE_H, TILE_W), (TILE_H - 1, TILE_W - 1), (TILE_H + 1, TILE_W + 1), (1, TILE_W + 7), (2 * TILE_H + 1, 1),
                                 (1, 1), (2 * TILE_H + 3, 2 * TILE_W + 5)])
def test_bitexact_around_the_tile_edges(dev, hip_lib, H, W):
    B, Hs, Ws, origin = 2, 40, 150, (5, 7)
    raw, params = raw_images(B, Hs, Ws, 10 * H + W), records(B, Hs, Ws, H, W, *origin, seed=H + 3 * W, k1=0.4)
    want = R.rectify_reference(raw, params, (H, W), origin, 9)
    assert_outputs(run(dev, raw, params, (H, W), origin, 9), want, f"{H}x{W}")


def test_wc_crossing_zero_gives_invalid_pixels_and_no_fault(dev, hip_lib):
    """Wc = xr / 64 - 0.5 is exactly 0 at xr = 32 and changes sign there: x = X / 0 = +-inf, and inf - inf or 0 * inf = NaN behind it."""
    B, Hs, Ws, (H, W) = 1, 20, 30, (12, 40)
    params = records(B, Hs, Ws, H, W, 0, 0, seed=5, k1=0.1)
    params[0, :, 6:9] = (1.0 / 64.0, 0.0, -0.5)
    params[0, 0, 13:] = (0.1, 0.2, 0.01, 0.01, 0.3)         # all positive: +inf where x and y are +inf, inf - inf = NaN elsewhere
    params[0, 1, 13:] = 0.0                                 # no distortion on the right: k * inf with k = 0 is NaN
    raw = raw_images(B, Hs, Ws, 6)
    want = R.rectify_reference(raw, params, (H, W), (0, 0), 31)
    for c in range(2):
        m = want["map"][c]
        assert np.isnan(m).any() or np.isinf(m).any()
        assert (want["rect"][c][0, :, 32] == 31).all() and (want["valid"][c][0, 0, :, 32] == 0).all()
    assert np.isinf(want["map"][0]).any() and np.isnan(want["map"][0]).any() and np.isnan(want["map"][1]).any()
    assert_outputs(run(dev, raw, params, (H, W), (0, 0), 31), want, "Wc through zero")


def golden_pair():
    from lwsnet_amd import imageio as io
    src = os.path.join(ROOT, "tests", "golden", "kitti_pair")
    return tuple(io.load_rgb(os.path.join(src, n))[None] for n in ("left_test.png", "right_test.png"))


def test_bitexact_on_the_golden_pair_as_raw_frames(dev, hip_lib):
    from lwsnet_amd.geometry import rectify_params
    raw = golden_pair()
    assert raw[0].shape == (1, 375, 1242, 3)
    calib = R.kitti_like_calib((375, 1242))[0]
    params, hw, origin = rectify_params(calib, 1), (368, 1232), (375 - 368, 1242 - 1232)
    want = R.rectify_reference(raw, params, hw, origin, 0)
    assert want["valid"][0].mean() > 0.9
    assert_outputs(run(dev, raw, params, hw, origin, 0), want, "golden pair")


def test_each_output_alone_gives_the_same_bytes(dev, hip_lib):
    B, Hs, Ws, (H, W), origin = 2, 37, 90, (11, 77), (3, 2)
    raw, params = raw_images(B, Hs, Ws, 21), records(B, Hs, Ws, H, W, *origin, seed=22)
    want = R.rectify_reference(raw, params, (H, W), origin, 17)
    for key in KEYS:
        got = run(dev, raw, params, (H, W), origin, 17, **{f"want_{k}": k == key for k in KEYS})
        assert sorted(got) == [key]
        assert_outputs(got, want, f"{key} alone", keys=(key,))
    # single elements through the C ABI: the left rect and the right valid map only
    rect0 = torch.full((B, H, W, 3), 0xA5, dtype=torch.uint8, device=dev)
    valid1 = torch.full((B, 1, H, W), 0xA5, dtype=torch.uint8, device=dev)
    raw_call(hip_lib, dev, [cu(r, dev) for r in raw], cu(params, dev), (H, W), origin, 17, rect=(rect0, None), valid=(None, valid1))
    G.assert_bits(rect0, want["rect"][0], "rect[0] alone")
    G.assert_bits(valid1, want["valid"][1], "valid[1] alone")


def raw_call(lib, dev, raw, params, hw, origin, border, rect=(None, None), inp=(None, None), valid=(None, None), mp=(None, None)):
    from lwsnet_amd import _lib
    arr = lambda pair: (ctypes.c_void_p * 2)(*[t.data_ptr() if t is not None else None for t in pair])      # noqa: E731
    B, Hs, Ws, _ = raw[0].shape
    mean, std = (ctypes.c_float * 3)(*R.IMAGENET_MEAN), (ctypes.c_float * 3)(*R.IMAGENET_STD)
    with torch.cuda.device(dev):
        _lib.check(lib.lws_rectify_pair(arr(raw), ctypes.c_void_p(params.data_ptr()), B, Hs, Ws, hw[0], hw[1], origin[1], origin[0], border,
                                        mean, std, arr(rect), arr(inp), arr(valid), arr(mp),
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "lws_rectify_pair")


def test_input_equals_preprocess_of_rect(dev, hip_lib):
    from lwsnet_amd import ops
    B, Hs, Ws, (H, W), origin = 2, 37, 90, (11, 77), (3, 2)
    got = run(dev, raw_images(B, Hs, Ws, 31), records(B, Hs, Ws, H, W, *origin, seed=32), (H, W), origin, 128)
    for c in range(2):
        G.assert_bits(got["input"][c], ops.preprocess_rgb8(got["rect"][c]).cpu().numpy(), f"input[{c}]")


def test_batch_independence_and_run_to_run_identity(dev, hip_lib):
    B, Hs, Ws, (H, W), origin = 3, 37, 90, (11, 77), (3, 2)
    raw, params = raw_images(B, Hs, Ws, 41), records(B, Hs, Ws, H, W, *origin, seed=42)
    batch = run(dev, raw, params, (H, W), origin, 5)
    alone = run(dev, [r[1:2] for r in raw], params[1:2], (H, W), origin, 5)
    raw2, params2 = [r.copy() for r in raw_images(B, Hs, Ws, 43)], records(B, Hs, Ws, H, W, *origin, seed=44)
    for c in range(2):
        raw2[c][0] = raw[c][1]
    params2[0] = params[1]
    first = run(dev, raw2, params2, (H, W), origin, 5)
    again = [run(dev, raw, params, (H, W), origin, 5) for _ in range(3)]
    for key in KEYS:
        for c in range(2):
            want = R.canonical_nans(alone[key][c].cpu().numpy()) if key == "map" else alone[key][c].cpu().numpy()
            canon = (lambda t: R.canonical_nans(t.cpu().numpy())) if key == "map" else (lambda t: t.cpu().numpy())
            G.assert_bits(canon(batch[key][c][1:2]), want, f"{key}[{c}] in the middle of three")
            G.assert_bits(canon(first[key][c][0:1]), want, f"{key}[{c}] first of three")
            for r in again:
                G.assert_bits(r[key][c], batch[key][c].cpu().numpy(), f"{key}[{c}] run to run")


def test_graph_capture_replays_the_call(dev, hip_lib):
    B, Hs, Ws, (H, W), origin = 2, 37, 90, (11, 77), (3, 2)
    sets = [(raw_images(B, Hs, Ws, s), records(B, Hs, Ws, H, W, *origin, seed=s + 1)) for s in (51, 53)]
    raw = [cu(r, dev) for r in sets[0][0]]
    params = cu(sets[0][1], dev)
    outs = {"rect": [torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(2)],
            "input": [torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) for _ in range(2)],
            "valid": [torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev) for _ in range(2)],
            "map": [torch.empty((B, H, W, 2), dtype=torch.float32, device=dev) for _ in range(2)]}
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_call(hip_lib, dev, raw, params, (H, W), origin, 64, rect=outs["rect"], inp=outs["input"], valid=outs["valid"], mp=outs["map"])
    for raw_np, params_np in sets:
        for c in range(2):
            raw[c].copy_(cu(raw_np[c], dev))
        params.copy_(cu(params_np, dev))
        graph.replay()
        torch.cuda.synchronize(dev)
        assert_outputs(outs, R.rectify_reference(raw_np, params_np, (H, W), origin, 64), "replay")


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("word", G.FLOAT_WORDS, ids=G.word_id)
def test_guard_bands_and_poisoned_outputs(dev, hip_lib, word, skew):
    """Every buffer between poisoned flanks, the outputs with poisoned interiors: nothing outside an output is written, every output
    element is, and no tap reaches past a raw image (the records throw many taps outside it)."""
    B, Hs, Ws, (H, W), origin = 2, 37, 90, (2 * TILE_H + 3, TILE_W + 13), (3, 2)
    raw_np, params_np = raw_images(B, Hs, Ws, 61), records(B, Hs, Ws, H, W, *origin, seed=62)
    want = R.rectify_reference(raw_np, params_np, (H, W), origin, 99)
    assert not want["valid"][0].all() and not want["valid"][1].all()
    g = G.Guard(dev, word, skew=skew)
    raw = [g.place(r, plane=3 * Hs * Ws, name=f"raw[{c}]") for c, r in enumerate(raw_np)]
    params = g.place(params_np, name="params")
    outs = {"rect": [g.empty((B, H, W, 3), np.uint8, plane=3 * H * W, name=f"rect[{c}]") for c in range(2)],
            "input": [g.empty((B, 3, H, W), name=f"input[{c}]") for c in range(2)],
            "valid": [g.empty((B, 1, H, W), np.uint8, name=f"valid[{c}]") for c in range(2)],
            "map": [g.empty((B, H, W, 2), plane=2 * H * W, name=f"map[{c}]") for c in range(2)]}
    raw_call(hip_lib, dev, raw, params, (H, W), origin, 99, rect=outs["rect"], inp=outs["input"], valid=outs["valid"], mp=outs["map"])
    assert_outputs(outs, want, "guarded")
    for c in range(2):
        G.assert_bits(raw[c], raw_np[c], "raw is only read")
    G.assert_bits(params, params_np, "params is only read")
    g.check()


def test_rectify_forward_wmedian_point_cloud_chain(dev, model):
    """The device chain against the same chain fed from the numpy restatement's outputs."""
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import camera_rows, rectify_params
    H, W, Hs, Ws = 64, 256, 70, 262
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    rng = np.random.default_rng(71)
    base = np.stack([(2 * xx + yy) % 256, (xx + 3 * yy) % 256, (5 * xx) % 256], axis=-1)
    raw = tuple(np.clip(np.roll(base, s, axis=1) + rng.integers(-20, 21, base.shape), 0, 255).astype(np.uint8)[None] for s in (0, -6))
    calib = R.kitti_like_calib((Hs, Ws))[0]
    params, origin = rectify_params(calib, 1), (Hs - H, Ws - W)
    cam = calib.camera().crop_bottom_right(Hs, Ws, H, W)
    wlut = ops.wmedian_lut(10.0)

    def tail(inputs, rect_l, valid_l):
        disp = model(inputs[0], inputs[1])[3]
        wm = ops.wmedian_filter(disp, 1, rgb=rect_l, wlut=wlut)
        return wm, ops.point_cloud(wm.disp, cam, mask=valid_l, rgb=rect_l, min_disp=0.25)

    got = run(dev, raw, params, (H, W), origin, 0, want_rect=True, want_input=True, want_valid=True)
    wm, (points, counts) = tail(got["input"], got["rect"][0], got["valid"][0])
    want = R.rectify_reference(raw, params, (H, W), origin, 0)
    assert not want["valid"][0].all() and want["valid"][0].any()
    wm_ref, (points_ref, counts_ref) = tail([cu(a, dev) for a in want["input"]], cu(want["rect"][0], dev), cu(want["valid"][0], dev))
    G.assert_bits(wm.disp, wm_ref.disp.cpu().numpy(), "filtered map")
    G.assert_bits(counts, counts_ref.cpu().numpy(), "point count")
    n = int(counts[0])
    assert n > 0, "the chain must keep points, or the comparison shows nothing"
    G.assert_bits(points[0, :n], points_ref[0, :n].cpu().numpy(), "points")
    # ... and the tail is what the numpy restatements of its two steps give on the device's disparity map
    d_np = model(got["input"][0], got["input"][1])[3].cpu().numpy()
    wm_np, _ = WM.wmedian_filter(d_np, 1, want["rect"][0], wlut, None, 0)
    G.assert_bits(wm.disp, wm_np, "filtered map against the reference")
    clouds, wn = GEO.point_cloud(wm_np, want["valid"][0], want["rect"][0], camera_rows(cam, 1), 0.25, float("inf"))
    G.assert_bits(counts, wn, "point count against the reference")
    assert np.array_equal(points.cpu().numpy()[0, :n].reshape(-1), clouds[0].view(np.uint8).reshape(-1)), "points differ"


def test_inference_cli_rectify(dev, model, tmp_path):
    """--rectify on the golden pair taken as raw frames, in process: the rectified crops, the stage maps' colour files and the point
    cloud are those of ops.rectify_pair -> forward -> point_cloud with the calibration's own camera and the valid map as mask."""
    from PIL import Image

    from lwsnet_amd import imageio as io
    from lwsnet_amd import inference, ops
    from lwsnet_amd.geometry import read_ply, rectify_params
    src = os.path.join(ROOT, "tests", "golden", "kitti_pair")
    for n in ("left_test.png", "right_test.png"):
        shutil.copy(os.path.join(src, n), tmp_path / n)
    calib = R.kitti_like_calib((375, 1242))[0]
    path = R.write_kitti(tmp_path / "calib_cam_to_cam.txt", calib)
    written = inference.main(["--left_img", str(tmp_path / "left_test.png"), "--synthetic_weights", "--rectify", path, "--save_rect",
                              "--save_ply", "--min_disp", "0.25"])
    names = ["left_test_rect_left.png", "left_test_rect_right.png"] + [f"{s}{t}" for s in (1, 2, 3, 4) for t in (".png", ".ply")]
    assert sorted(os.path.basename(w) for w in written) == sorted(names)
    raw, origin = golden_pair(), (375 - io.CROP_H, 1242 - io.CROP_W)
    got = run(dev, raw, rectify_params(calib, 1), (io.CROP_H, io.CROP_W), origin, 0, want_rect=True, want_input=True, want_valid=True)
    for c, side in enumerate(("left", "right")):
        assert np.array_equal(np.asarray(Image.open(tmp_path / f"left_test_rect_{side}.png")), got["rect"][c][0].cpu().numpy()), side
    disp = model(got["input"][0], got["input"][1])
    cam = calib.camera().crop_bottom_right(375, 1242)
    for s in range(4):
        assert np.array_equal(np.asarray(Image.open(tmp_path / f"{s + 1}.png")), io.disparity_to_color(disp[s].numpy()[0, 0])), f"stage {s + 1}"
    points, counts = ops.point_cloud(disp[3], cam, mask=got["valid"][0], rgb=got["rect"][0], min_disp=0.25)
    n = int(counts[0])
    assert n > 0
    assert np.array_equal(read_ply(str(tmp_path / "4.ply")).view(np.uint8), points[0, :n].cpu().numpy().reshape(-1))
    # a frame of another size than S_xx is an error for that frame: nothing is written for it
    small = tmp_path / "small"
    small.mkdir()
    for n_ in ("left_test.png", "right_test.png"):
        Image.fromarray(raw[0][0, :370]).save(small / n_)
    assert inference.main(["--left_img", str(small / "left_test.png"), "--synthetic_weights", "--rectify", path]) == []


GEOMETRY = [("--save_disp16", "_disp16.png", "Save disp16"), ("--save_depth", "_depth16.png", "Save depth16"), ("--save_ply", ".ply", "Save point"),
            ("--save_normals", "_normals.png", "Save normal"), ("--save_mesh", "_mesh.ply", "Save mesh"), ("--save_ground", "_ground.png", "Ground: status"),
            (None, "_bev.png", "Save ground"), ("--save_stixels", "_stixels.png", "Stixels: "), (None, "_stixels.csv", "Save stixels")]
CHAIN = ["--save_rect", "--speckle", "60", "--wmedian", "2", "--photometric", "--save_photo"]


def _chain_case(check, suffix, words, without=()):
    geo = [g for g in GEOMETRY if g[0] not in without]
    return (CHAIN + check + [g[0] for g in geo if g[0]],
            ["_rect_left.png", "_rect_right.png", ".png", suffix, "_sp.png"] + [g[1] for g in geo] + ["_pe.png", "_warp.png"],
            ["Save rectified", "Save rectified"] + ["Weighted median"] * 4 + ["Photometric (", "Inference 4", words, "Speckle filter:"]
            + [g[2] for g in geo] + ["Save photometric"])


# With --lr_check 1 --speckle 60 no pixel of this pair survives, and an empty point cloud cannot be written (ply_bytes refuses a
# view with a zero in its shape), so that line goes without the two PLY files; they are in the other two lines.
CASES = {"lr": _chain_case(["--lr_check", "1"], "_lr.png", "LR check:", without=("--save_ply", "--save_mesh")),
         "occ": _chain_case(["--occ_check", "1"], "_occ.png", "Occlusion check:"),
         "confidence": (["--save_conf", "--conf_min", "0.3", "--sigma_max_keep", "4"] + [g[0] for g in GEOMETRY if g[0]],
                        [".png", "_conf.png", "_sigma.png"] + [g[1] for g in GEOMETRY], ["Inference 4", "Confidence: "] + [g[2] for g in GEOMETRY])}


@pytest.mark.parametrize("extra,files,lines", list(CASES.values()), ids=list(CASES))
def test_inference_cli_every_output_in_order(extra, files, lines, tmp_path, caplog):
    """One raw frame in directory mode with every output that combines switched on: the names and the order of the returned paths,
    and the order of the log lines between "Begin inference!" and "End inference!" by their leading words.  (What each file
    holds is the business of its feature's own test.)"""
    import logging

    from lwsnet_amd import inference
    src = os.path.join(ROOT, "tests", "golden", "kitti_pair")
    for folder, name in (("image_2", "left_test.png"), ("image_3", "right_test.png")):
        os.makedirs(tmp_path / "kitti" / folder)
        shutil.copy(os.path.join(src, name), tmp_path / "kitti" / folder / "000007_10.png")
    path = R.write_kitti(tmp_path / "calib_cam_to_cam.txt", R.kitti_like_calib((375, 1242))[0])
    with caplog.at_level(logging.INFO, logger="lwsnet_amd.inference"):
        written = inference.main(["--img_path", str(tmp_path / "kitti"), "--save_path", str(tmp_path / "out"), "--synthetic_weights", "--rectify", path,
                                  "--camera", "721.5", "721.5", "609.5", "172.8", "0.54", *extra])
    assert written == [str(tmp_path / "out" / ("000007_10" + f)) for f in files]
    assert all(os.path.getsize(w) > 0 for w in written)
    messages = [r.getMessage() for r in caplog.records if r.name == "lwsnet_amd.inference"]
    messages = messages[messages.index("Begin inference!") + 1:messages.index("End inference!")]
    assert len(messages) == len(lines), messages
    for message, words in zip(messages, lines):
        assert message.startswith(words), (message, words)
