"""Left-right consistency check on the device: lws_lr_pairs and lws_lr_check bit for bit against the numpy restatement
(tests/lr_reference.py), batch independence, LWSNet.forward_lr against two plain forwards, and the --lr_check / --lr_fill flags of
the inference and evaluation CLIs."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import lr_reference as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(bits(got), bits(want)), f"{what}: {int((bits(got) != bits(want)).sum())} elements differ"


def maps(B, H, W, seed):
    """A left-view and a mirrored right-view map: a per-row disparity plus noise, so that tau 0 / 1 / 3 see every code; NaN and
    +-inf planted in both."""
    rng = np.random.default_rng(seed)
    base = rng.random((B, 1, H, 1)) * min(30.0, W / 2.0)
    dl = (base + rng.uniform(-1.5, 1.5, (B, 1, H, W))).astype(np.float32)
    drm = (base + rng.uniform(-1.5, 1.5, (B, 1, H, W))).astype(np.float32)
    dl[rng.random(dl.shape) < 0.01] = 0.0
    for a in (dl, drm):
        flat = a.reshape(-1)
        idx = rng.choice(flat.size, size=min(flat.size, 3 * max(1, flat.size // 500)), replace=False)
        k = len(idx) // 3
        flat[idx[:k]] = np.nan
        flat[idx[k:2 * k]] = np.inf
        flat[idx[2 * k:]] = -np.inf
    return dl, drm


@pytest.mark.parametrize("B,H,W", [(1, 256, 512), (3, 63, 255)])
def test_lr_pairs_bitexact(dev, hip_lib, B, H, W):
    from lwsnet_amd import ops
    rng = np.random.default_rng(B * W)
    left = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    right = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    l2, r2 = ops.lr_pairs(cu(left, dev), cu(right, dev))
    wl, wr = R.lr_pairs(left, right)
    assert_bits(l2, wl, "left2")
    assert_bits(r2, wr, "right2")


@pytest.mark.parametrize("B,H,W", [(1, 256, 512), (3, 368, 1232), (2, 63, 255), (1, 8, 1)])
def test_lr_check_bitexact(dev, hip_lib, B, H, W):
    from lwsnet_amd import ops
    stages = [maps(B, H, W, 10 * s + W) for s in range(4)]
    dls, drms = [cu(m[0], dev) for m in stages], [cu(m[1], dev) for m in stages]
    for nmaps in (1, 4):
        for tau in (0.0, 1.0, 3.0):
            for fill in (0, 1):
                want_right = (nmaps + fill) % 2 == 1 or tau == 1.0          # the optional output both ways
                out, mask, right, kept = ops.lr_check(dls[:nmaps], drms[:nmaps], tau, fill, want_right=want_right)
                assert (right is None) != want_right
                for s in range(nmaps):
                    wo, wm, wr, wk = R.lr_check(stages[s][0], stages[s][1], tau, fill)
                    what = f"B={B} {H}x{W} nmaps={nmaps} tau={tau} fill={fill} map {s}"
                    assert_bits(out[s], wo, what + " out")
                    assert_bits(mask[s], wm, what + " mask")
                    if want_right:
                        assert_bits(right[s], wr, what + " right")
                    assert_bits(kept[s], wk, what + " row_kept")
                if tau == 1.0 and nmaps == 4:
                    codes = np.concatenate([m.cpu().numpy().ravel() for m in mask])
                    assert set(np.unique(codes)) <= {0, 1, 2}
                    if H * W > 64:
                        assert {0, 1, 2} <= set(np.unique(codes)), "the inputs should reach every code"


def test_lr_check_without_row_kept(dev, hip_lib):
    """row_kept is optional in the C ABI as well (NULL: skipped)."""
    import ctypes
    from lwsnet_amd import _lib
    dl, drm = maps(2, 16, 100, 3)
    d, r = cu(dl, dev), cu(drm, dev)
    out, mask = torch.empty_like(d), torch.empty(d.shape, dtype=torch.uint8, device=dev)
    arr = ctypes.c_void_p * 4
    with torch.cuda.device(dev):
        _lib.check(hip_lib.lws_lr_check(arr(d.data_ptr()), arr(r.data_ptr()), 1, 2, 16, 100, 1.0, 1, arr(out.data_ptr()),
                                        arr(mask.data_ptr()), arr(), None,
                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "lws_lr_check")
    wo, wm, _, _ = R.lr_check(dl, drm, 1.0, 1)
    assert_bits(out, wo, "out")
    assert_bits(mask, wm, "mask")


@pytest.mark.parametrize("skew", [0, 1], ids=["aligned", "skewed"])
@pytest.mark.parametrize("W", [3, 8, 8189, 8192])
def test_lr_check_row_corners(dev, hip_lib, W, skew):
    """The corners of the row scaffolding, two rows each (the kernel shares nothing between rows): less than one quad (W = 3), a
    thread's eighth quad (W = 8192: bit 31 of its flags word), that quad with a ragged tail (8189), and every base one float past a
    16-byte boundary, where an aligned width (8, 8192) takes the scalar path too; fill off and on, right / row_kept there and not."""
    import ctypes
    from lwsnet_amd import _lib
    B, H = 1, 2
    n = B * H * W
    dl_np, drm_np = maps(B, H, W, W)

    def place(a=None, dtype=torch.float32):
        t = torch.empty(n + 8, dtype=dtype, device=dev)[4 + skew:4 + skew + n].view(B, 1, H, W)
        assert dtype != torch.float32 or t.data_ptr() % 16 == 4 * skew
        return t if a is None else t.copy_(cu(a, dev))

    arr = ctypes.c_void_p * 4
    for fill in (0, 1):
        wo, wm, wr, wk = R.lr_check(dl_np, drm_np, 1.0, fill)
        if W >= 8189:
            assert (wm[..., 7171::4] == 1).any(), "a kept pixel under bit 31 of a thread's flags"
        for optional in (True, False):
            dl, drm, out, mask = place(dl_np), place(drm_np), place(), place(dtype=torch.uint8)
            right = place() if optional else None
            kept = torch.empty((1, B, H), dtype=torch.int32, device=dev) if optional else None
            with torch.cuda.device(dev):
                _lib.check(hip_lib.lws_lr_check(arr(dl.data_ptr()), arr(drm.data_ptr()), 1, B, H, W, 1.0, fill, arr(out.data_ptr()),
                                                arr(mask.data_ptr()), arr(right.data_ptr()) if optional else arr(),
                                                ctypes.c_void_p(kept.data_ptr()) if optional else None,
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "lws_lr_check")
            what = f"W={W} skew={skew} fill={fill} optional={optional}"
            assert_bits(out, wo, what + " out")
            assert_bits(mask, wm, what + " mask")
            if optional:
                assert_bits(right, wr, what + " right")
                assert_bits(kept[0], wk, what + " row_kept")


def test_lr_check_is_batch_independent(dev, hip_lib):
    from lwsnet_amd import ops
    H, W = 63, 255
    dl, drm = maps(3, H, W, 77)
    alone = ops.lr_check([cu(dl[1:2], dev)], [cu(drm[1:2], dev)], 1.0, 1)
    batch = ops.lr_check([cu(dl, dev)], [cu(drm, dev)], 1.0, 1)
    for k, what in ((0, "out"), (1, "mask"), (2, "right")):
        assert_bits(batch[k][0][1:2], alone[k][0].cpu().numpy(), what)
    assert_bits(batch[3][:, 1:2], alone[3].cpu().numpy(), "row_kept")
    # the same image placed first of three, with other content around it
    dl2, drm2 = maps(3, H, W, 78)
    dl2[0], drm2[0] = dl[1], drm[1]
    first = ops.lr_check([cu(dl2, dev)], [cu(drm2, dev)], 1.0, 1)
    assert_bits(first[0][0][0:1], alone[0][0].cpu().numpy(), "out at position 0")


@pytest.mark.parametrize("B,H,W", [(1, 256, 512), (2, 256, 512), (1, 368, 1232)])
def test_forward_lr(dev, model, B, H, W):
    from lwsnet_amd.synth import make_pair
    pairs = [make_pair(H, W, i) for i in range(B)]
    left = np.stack([p[0] for p in pairs])
    right = np.stack([p[1] for p in pairs])
    for tau, fill in ((1.0, True), (3.0, False)):
        res = model.forward_lr(left, right, tau=tau, fill=fill)
        plain = model(left, right)
        mirrored = model(np.ascontiguousarray(right[..., ::-1]), np.ascontiguousarray(left[..., ::-1]))
        assert res.density.shape == (4, B)
        for s in range(4):
            assert type(res.left[s]) is type(plain[s])
            assert_bits(res.left[s], plain[s].numpy(), f"left stage {s + 1}")
            drm = mirrored[s].numpy()
            assert_bits(res.right[s], R.mirror_w(drm), f"right stage {s + 1}")
            wo, wm, _, wk = R.lr_check(plain[s].numpy(), drm, tau, fill)
            assert_bits(res.disp[s], wo, f"disp stage {s + 1}")
            assert_bits(res.mask[s], wm, f"mask stage {s + 1}")
            assert np.array_equal(res.density[s], wk.sum(axis=1) / float(H * W))
        assert 0.0 <= res.density.min() and res.density.max() <= 1.0


def _expected_files(model, left_path, right_path, tau, fill, stages):
    from lwsnet_amd import imageio as io
    l_in = io.to_input(io.crop_bottom_right(io.load_rgb(left_path)))[None]
    r_in = io.to_input(io.crop_bottom_right(io.load_rgb(right_path)))[None]
    res = model.forward_lr(l_in, r_in, tau=tau, fill=fill)
    plain = model(l_in, r_in)
    return [(io.disparity_to_color(res.disp[s].numpy()[0, 0]), io.LR_MASK_GREY[res.mask[s].cpu().numpy()[0, 0]],
             io.disparity_to_color(plain[s].numpy()[0, 0])) for s in stages]


def test_inference_cli_lr_check(dev, model, tmp_path):
    from PIL import Image
    from lwsnet_amd import inference
    src = os.path.join(ROOT, "tests", "golden", "kitti_pair")
    # --left_img mode: 1..4.png from the checked maps and 1_lr..4_lr.png beside them
    for tag in ("lr", "plain"):
        (tmp_path / tag).mkdir()
        for n in ("left_test.png", "right_test.png"):
            shutil.copy(os.path.join(src, n), tmp_path / tag / n)
    written = inference.main(["--left_img", str(tmp_path / "lr" / "left_test.png"), "--synthetic_weights", "--lr_check", "1",
                              "--lr_fill"])
    assert [os.path.basename(p) for p in written] == ["1.png", "1_lr.png", "2.png", "2_lr.png", "3.png", "3_lr.png", "4.png",
                                                      "4_lr.png"]
    plain = inference.main(["--left_img", str(tmp_path / "plain" / "left_test.png"), "--synthetic_weights"])
    assert [os.path.basename(p) for p in plain] == ["1.png", "2.png", "3.png", "4.png"]
    want = _expected_files(model, str(tmp_path / "lr" / "left_test.png"), str(tmp_path / "lr" / "right_test.png"), 1.0, True, range(4))
    for s in range(4):
        color, grey, color_plain = want[s]
        assert np.array_equal(np.asarray(Image.open(written[2 * s])), color)
        g = Image.open(written[2 * s + 1])
        assert g.mode == "L" and np.array_equal(np.asarray(g), grey)
        assert np.array_equal(np.asarray(Image.open(plain[s])), color_plain)
    # directory mode: the stage-4 map and its mask per pair; without the flags the same files as the plain run
    l0 = np.asarray(Image.open(os.path.join(src, "left_test.png")).convert("RGB"))
    r0 = np.asarray(Image.open(os.path.join(src, "right_test.png")).convert("RGB"))
    kdir = tmp_path / "kitti"
    for d in ("image_2", "image_3"):
        (kdir / d).mkdir(parents=True)
    for i in range(2):
        Image.fromarray(np.roll(l0, 11 * i, axis=1)).save(kdir / "image_2" / f"{i:06d}_10.png")
        Image.fromarray(np.roll(r0, 11 * i, axis=1)).save(kdir / "image_3" / f"{i:06d}_10.png")
    out = tmp_path / "out_lr"
    written = inference.main(["--img_path", str(kdir), "--save_path", str(out), "--synthetic_weights", "--lr_check", "1", "--lr_fill"])
    assert sorted(os.listdir(out)) == ["000000_10.png", "000000_10_lr.png", "000001_10.png", "000001_10_lr.png"]
    assert len(written) == 4
    out_plain = tmp_path / "out_plain"
    inference.main(["--img_path", str(kdir), "--save_path", str(out_plain), "--synthetic_weights"])
    assert sorted(os.listdir(out_plain)) == ["000000_10.png", "000001_10.png"]
    for i in range(2):
        name = f"{i:06d}_10.png"
        color, grey, color_plain = _expected_files(model, str(kdir / "image_2" / name), str(kdir / "image_3" / name), 1.0, True, [3])[0]
        assert np.array_equal(np.asarray(Image.open(out / name)), color)
        assert np.array_equal(np.asarray(Image.open(out / f"{i:06d}_10_lr.png")), grey)
        assert np.array_equal(np.asarray(Image.open(out_plain / name)), color_plain)


def test_evaluate_cli_lr_check(dev, model, tmp_path):
    from lwsnet_amd import datasets as D
    from lwsnet_amd import synth
    root = str(tmp_path / "kitti") + "/"
    split = synth.write_kitti_tree(root, 4)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out_json = tmp_path / "lr.json"
    r = subprocess.run([sys.executable, "-m", "lwsnet_amd.evaluate", "--synthetic_weights", "--test_batch_size", "2", "--dataset",
                        "kitti2015", "--datapath", root, "--val_set", split, "--lr_check", "1", "--lr_fill", "--json", str(out_json)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.load(open(out_json))
    ds = D.StereoPairs(*D.kitti2015_lists(root, split)[3:], training=False, kitti_set=True)
    vals, dens = [], []
    for i in range(0, 4, 2):
        items = [ds[j] for j in range(i, i + 2)]
        out = model.forward_lr(np.stack([it[0] for it in items]), np.stack([it[1] for it in items]), tau=1.0, fill=True)
        gt = np.stack([it[2] for it in items]).astype(np.float32)
        row = []
        for s in range(4):
            d = out.disp[s].numpy()[:, 0]
            mask = (gt > 0) & (gt < 192)
            e = np.abs(d - gt)
            row.append(float(((e[mask] > 3.) & (e[mask] / gt[mask] > 0.05)).sum()) / float(mask.sum()))
        vals.append(row)
        dens.append(out.density)
    assert res["per_batch"] == vals
    assert res["lr_tau"] == 1.0
    assert res["lr_density"] == [float(d) for d in np.concatenate(dens, axis=1).mean(axis=1)]
    assert "Average test 3-Pixel Error: Stage 0=" in r.stderr and "LR check (tau = 1, filled): mean density Stage 0=" in r.stderr
