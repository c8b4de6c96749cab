"""The speckle filter on the device: lws_speckle_filter bit for bit against the numpy / Python restatement
(tests/speckle_reference.py) on plateaus with islands and on the adversarial shapes (serpentine, spiral, comb, checkerboard,
constant, components across every tile edge), batch independence, run-to-run identity, the optional arguments of the C ABI, in-place
use, hipGraph capture, the chain forward_lr -> speckle_filter -> point_cloud, and the --speckle flags of the two CLIs."""
import ctypes
import itertools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import geometry_reference as G
import lr_reference as LR
import speckle_inputs as I
import speckle_reference as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MAX_DIFFS = (0.0, 0.5, 1.0)
MAX_SIZES = (0, 1, 50, 10 ** 6)


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


def check(ops, d_np, m_np, d, m, lab, max_diff, max_size, fill, want_labels, what):
    """One ops.speckle_filter call against the reference applied to the labelling `lab` of (d_np, m_np, max_diff)."""
    res = ops.speckle_filter(d, max_size, max_diff, mask=m, fill=bool(fill), want_labels=want_labels)
    wo, wm, wl, wc = R.apply(d_np, m_np, lab, max_size, fill)
    what = f"{what} max_diff={max_diff} max_size={max_size} fill={fill} mask={'on' if m is not None else 'off'}"
    assert_bits(res.disp, wo, what + " out")
    assert_bits(res.mask, wm, what + " mask_out")
    assert (res.labels is None) == (not want_labels)
    if want_labels:
        assert_bits(res.labels, wl, what + " labels")
    assert_bits(res.counts, wc, what + " counts")
    return wm, wc


@pytest.mark.parametrize("kind", I.KINDS)
@pytest.mark.parametrize("B,H,W", [(1, 256, 512), (2, 63, 255), (1, 8, 1), (1, 1, 300)])
def test_speckle_filter_bitexact_small(dev, hip_lib, kind, B, H, W):
    """The full cross product mask x max_diff x max_size x fill x labels; the labelling of the reference is computed once per
    (input, mask, max_diff)."""
    from lwsnet_amd import ops
    d_np = I.make(kind, B, H, W, 3 * H + W)
    mask_np = I.random_mask(B, H, W, H + 7 * W)
    d = cu(d_np, dev)
    for m_np in (None, mask_np):
        m = None if m_np is None else cu(m_np, dev)
        for max_diff in MAX_DIFFS:
            lab = R.labelling(d_np, m_np, max_diff)
            for max_size, fill, want_labels in itertools.product(MAX_SIZES, (0, 1), (False, True)):
                wm, wc = check(ops, d_np, m_np, d, m, lab, max_diff, max_size, fill, want_labels, f"{kind} B={B} {H}x{W}")
                if kind == "plateaus" and m_np is not None and max_diff == 0.5 and max_size == 50 and H * W >= 63 * 255:
                    assert set(np.unique(wm)) == {0, 1, 2, 3}, "the inputs should reach every code"
                    assert (wc[:, 2] > 0).all() and (wc[:, 1] > 0).all(), "the inputs should have removed and kept components"


# (kind, mask, max_diff, max_size, fill, labels): every input kind, mask on and off, fill 0 and 1
LARGE = [("plateaus", True, 0.5, 50, 1, True), ("plateaus", False, 1.0, 50, 0, False), ("plateaus", True, 0.0, 1, 0, True),
         ("serpentine", False, 0.5, 50, 0, True), ("serpentine", True, 1.0, 10 ** 6, 1, False), ("spiral", False, 0.0, 50, 1, True),
         ("spiral", True, 0.5, 1, 0, False), ("comb", False, 1.0, 50, 0, True), ("comb", True, 0.5, 50, 1, True),
         ("checkerboard", False, 1.0, 1, 1, True), ("checkerboard", True, 0.5, 0, 0, False), ("constant", False, 0.0, 10 ** 6, 1, True),
         ("constant", True, 1.0, 50, 0, True)]


@pytest.mark.parametrize("kind,masked,max_diff,max_size,fill,want_labels", LARGE)
def test_speckle_filter_bitexact_large(dev, hip_lib, kind, masked, max_diff, max_size, fill, want_labels):
    from lwsnet_amd import ops
    B, H, W = 3, 368, 1232
    d_np = I.make(kind, B, H, W, 41)
    m_np = I.random_mask(B, H, W, 42) if masked else None
    lab = R.labelling(d_np, m_np, max_diff)
    if kind in ("serpentine", "spiral", "comb", "constant") and not masked:
        assert np.unique(lab[0][1]).tolist() in ([-1, 0], [0]), "one component through the whole image"
    wm, wc = check(ops, d_np, m_np, cu(d_np, dev), None if m_np is None else cu(m_np, dev), lab, max_diff, max_size, fill,
                   want_labels, f"{kind} B={B} {H}x{W}")
    if kind == "plateaus" and masked and max_diff == 0.5:
        assert set(np.unique(wm)) == {0, 1, 2, 3} and (wc[:, 2] > 0).all() and (wc[:, 1] > 0).all()


def test_components_across_every_tile_edge(dev, hip_lib):
    """Pairs and 2 x 2 blocks whose halves lie on both sides of every possible tile border and corner."""
    from lwsnet_amd import ops
    d_np = I.edge_cases()
    d = cu(d_np, dev)
    lab = R.labelling(d_np, None, 1.0)
    for max_size, fill in itertools.product((0, 1, 2, 3, 4, 50), (0, 1)):
        wm, wc = check(ops, d_np, None, d, None, lab, 1.0, max_size, fill, True, "edge cases")
        assert (wc[:2, 1] == (0 if max_size >= 2 else wc[:2, 0])).all() and (wc[2:, 1] == (0 if max_size >= 4 else wc[2:, 0])).all()
    # the same components one pixel further apart in value than max_diff: nothing joins
    check(ops, d_np, None, d, None, R.labelling(d_np, None, 0.0), 0.0, 1, 0, True, "edge cases")


def test_speckle_filter_is_batch_independent(dev, hip_lib):
    from lwsnet_amd import ops
    H, W = 63, 255
    d, m = I.plateaus(3, H, W, 77), I.random_mask(3, H, W, 78)
    kw = dict(max_size=50, max_diff=0.5, fill=True, want_labels=True)
    alone = ops.speckle_filter(cu(d[1:2], dev), mask=cu(m[1:2], dev), **kw)
    batch = ops.speckle_filter(cu(d, dev), mask=cu(m, dev), **kw)
    d2, m2 = I.serpentine(3, H, W, 0), I.random_mask(3, H, W, 79)
    d2[0], m2[0] = d[1], m[1]
    first = ops.speckle_filter(cu(d2, dev), mask=cu(m2, dev), **kw)
    for k, what in enumerate(("out", "mask_out", "labels", "counts")):
        assert_bits(batch[k][1:2], alone[k].cpu().numpy(), what + " in the middle of three")
        assert_bits(first[k][0:1], alone[k].cpu().numpy(), what + " first of three")


@pytest.mark.parametrize("kind", ["serpentine", "plateaus"])
def test_speckle_filter_is_run_to_run_identical(dev, hip_lib, kind):
    from lwsnet_amd import ops
    d = cu(I.make(kind, 2, 368, 1232, 5), dev)
    m = cu(I.random_mask(2, 368, 1232, 6), dev) if kind == "plateaus" else None
    runs = [ops.speckle_filter(d, 50, 0.5, mask=m, fill=True, want_labels=True) for _ in range(5)]
    for r in runs[1:]:
        for k, what in enumerate(("out", "mask_out", "labels", "counts")):
            assert_bits(r[k], runs[0][k].cpu().numpy(), f"{kind} {what}")


def _raw_call(lib, dev, d, m, max_diff, max_size, fill, out, mask_out, labels, counts, work):
    from lwsnet_amd import _lib
    B, _, H, W = d.shape
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(lib.lws_speckle_filter(p(d), p(m), B, H, W, max_diff, max_size, fill, p(work), p(out), p(mask_out), p(labels),
                                          p(counts), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "lws_speckle_filter")


def test_c_abi_optional_arguments_and_in_place(dev, hip_lib):
    """labels = NULL, counts = NULL, mask = NULL; out = disp and mask_out = mask (in place)."""
    B, H, W = 2, 63, 255
    d_np, m_np = I.plateaus(B, H, W, 9), I.random_mask(B, H, W, 10)
    work = torch.empty((int(hip_lib.lws_speckle_workspace(B, H, W)),), dtype=torch.uint8, device=dev)
    d = cu(d_np, dev)
    out, mask_out = torch.empty_like(d), torch.empty(d.shape, dtype=torch.uint8, device=dev)
    _raw_call(hip_lib, dev, d, None, 0.5, 50, 1, out, mask_out, None, None, work)
    wo, wm, _, _ = R.speckle_filter(d_np, None, 0.5, 50, 1)
    assert_bits(out, wo, "out")
    assert_bits(mask_out, wm, "mask_out")
    for fill in (0, 1):
        d2, m2 = cu(d_np, dev), cu(m_np, dev)
        _raw_call(hip_lib, dev, d2, m2, 0.5, 50, fill, d2, m2, None, None, work)
        wo, wm, _, _ = R.speckle_filter(d_np, m_np, 0.5, 50, fill)
        assert_bits(d2, wo, f"in place out fill={fill}")
        assert_bits(m2, wm, f"in place mask_out fill={fill}")


@pytest.mark.parametrize("skew", [0, 1], ids=["aligned", "skewed"])
@pytest.mark.parametrize("W", [3, 8, 8189, 8192])
def test_apply_row_corners(dev, hip_lib, W, skew):
    """The corners of k_sp_apply's row scaffolding, two rows each: less than one quad (W = 3), a thread's eighth quad (W = 8192, the
    widest row the fill takes: bit 31 of its flags word), that quad with a ragged tail (8189), and disp / mask / out / mask_out /
    labels one element past a 16-byte boundary, where an aligned width (8, 8192) takes the scalar path too; fill off and on, labels
    and counts there and not, out of place and in place."""
    B, H = 1, 2
    n = B * H * W
    d_np, m_np = I.plateaus(B, H, W, W), I.random_mask(B, H, W, W + 1)
    work = torch.empty((int(hip_lib.lws_speckle_workspace(B, H, W)),), dtype=torch.uint8, device=dev)

    def place(a=None, dtype=torch.float32):
        t = torch.empty(n + 8, dtype=dtype, device=dev)[4 + skew:4 + skew + n].view(B, 1, H, W)
        return t if a is None else t.copy_(cu(a, dev))

    for fill in (0, 1):
        wo, wm, wl, wc = R.speckle_filter(d_np, m_np, 0.5, 50, fill)
        if W >= 8189:
            assert (wm[..., 7171::4] == 1).any(), "a kept pixel under bit 31 of a thread's flags"
        for optional, in_place in ((True, False), (False, False), (False, True)):
            d, m = place(d_np), place(m_np, torch.uint8)
            assert d.data_ptr() % 16 == 4 * skew
            out, mask_out = (d, m) if in_place else (place(), place(dtype=torch.uint8))
            labels = place(dtype=torch.int32) if optional else None
            counts = torch.empty((B, 3), dtype=torch.int64, device=dev) if optional else None
            _raw_call(hip_lib, dev, d, m, 0.5, 50, fill, out, mask_out, labels, counts, work)
            what = f"W={W} skew={skew} fill={fill} optional={optional} in_place={in_place}"
            assert_bits(out, wo, what + " out")
            assert_bits(mask_out, wm, what + " mask_out")
            if optional:
                assert_bits(labels, wl, what + " labels")
                assert_bits(counts, wc, what + " counts")


def test_rows_wider_than_the_fill_takes_without_fill(dev, hip_lib):
    """fill = 0 has no bound on W: at W = 8200 a thread of k_sp_apply owns a ninth quad, whose kept pixels must still be counted and
    written; every output, with and without a mask."""
    from lwsnet_amd import ops
    B, H, W = 1, 2, 8200
    d_np, m_np = I.plateaus(B, H, W, W), I.random_mask(B, H, W, W + 1)
    for m in (None, m_np):
        wo, wm, wl, wc = R.speckle_filter(d_np, m, 0.5, 50, 0)
        assert (wm[..., 8192:] == 1).any(), "a kept pixel in a thread's ninth quad"
        res = ops.speckle_filter(cu(d_np, dev), 50, 0.5, mask=None if m is None else cu(m, dev), fill=False, want_labels=True)
        for got, want, what in ((res.disp, wo, "out"), (res.mask, wm, "mask_out"), (res.labels, wl, "labels"), (res.counts, wc, "counts")):
            assert_bits(got, want, f"W={W} mask={'on' if m is not None else 'off'} {what}")


def test_graph_capture_replays_the_filter(dev, hip_lib):
    from lwsnet_amd import ops
    B, H, W = 2, 256, 512
    first, second = I.plateaus(B, H, W, 21), I.serpentine(B, H, W, 0)
    m1, m2 = I.random_mask(B, H, W, 22), I.random_mask(B, H, W, 23)
    d, m = cu(first, dev), cu(m1, dev)
    out, mask_out = torch.empty_like(d), torch.empty_like(m)
    labels = torch.empty(d.shape, dtype=torch.int32, device=dev)
    counts = torch.empty((B, 3), dtype=torch.int64, device=dev)
    work = torch.empty((int(hip_lib.lws_speckle_workspace(B, H, W)),), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _raw_call(hip_lib, dev, d, m, 0.5, 50, 1, out, mask_out, labels, counts, work)
    for d_np, m_np in ((first, m1), (second, m2)):
        d.copy_(cu(d_np, dev))
        m.copy_(cu(m_np, dev))
        graph.replay()
        torch.cuda.synchronize(dev)
        eager = ops.speckle_filter(cu(d_np, dev), 50, 0.5, mask=cu(m_np, dev), fill=True, want_labels=True)
        for got, k, what in ((out, 0, "out"), (mask_out, 1, "mask_out"), (labels, 2, "labels"), (counts, 3, "counts")):
            assert_bits(got, eager[k].cpu().numpy(), "replay " + what)
        wo, wm, wl, wc = R.speckle_filter(d_np, m_np, 0.5, 50, 1)
        assert_bits(out, wo, "replay out against the reference")
        assert_bits(counts, wc, "replay counts against the reference")


# The reference chain on synth.make_pair(368, 1232, 0), stage 4, tau = 1, max_diff = 1 leaves 10180 components, none larger than
# 7 pixels (the synthetic weights give a rough map, and the left-right check cuts it up further; the test prints the histogram).
# MAX_SIZE_CHAIN = 2 removes the single pixels and the pairs and keeps the components of 3 .. 7 pixels; the test asserts that the
# reference removes at least one component and keeps at least one, so a choice that no longer fits fails here, not silently.
MAX_SIZE_CHAIN = 2


def test_forward_lr_speckle_point_cloud_chain(dev, model):
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import Camera, camera_rows
    from lwsnet_amd.synth import make_pair
    H, W = 368, 1232
    left, right = make_pair(H, W, 0)[:2]
    left, right = left[None], right[None]
    cam = Camera(721.5, 721.5, 609.5, 172.8, 0.54)
    res = model.forward_lr(left, right, tau=1.0, fill=False)
    plain = model(left, right)
    mirrored = model(np.ascontiguousarray(right[..., ::-1]), np.ascontiguousarray(left[..., ::-1]))
    for s in (3,):
        wo, wm, _, _ = LR.lr_check(plain[s].numpy(), mirrored[s].numpy(), 1.0, 0)
        assert_bits(res.disp[s], wo, f"stage {s + 1} checked map")
        assert_bits(res.mask[s], wm, f"stage {s + 1} LR mask")
        lab = R.labelling(wo, wm, 1.0)
        sizes = np.bincount(lab[0][1][lab[0][1] >= 0])
        sizes = sizes[sizes > 0]
        print(f"stage {s + 1}: {sizes.size} components, sizes 1 .. 8: {np.bincount(sizes, minlength=9)[1:9].tolist()}, largest {sizes.max()}")
        so, sm, sl, sc = R.apply(wo, wm, lab, MAX_SIZE_CHAIN, 0)
        assert sc[0, 2] >= 1 and sc[0, 1] >= 1, "the reference chain must remove a component and keep one"
        sp = ops.speckle_filter(res.disp[s], MAX_SIZE_CHAIN, 1.0, mask=res.mask[s], fill=False, want_labels=True)
        assert_bits(sp.disp, so, f"stage {s + 1} filtered map")
        assert_bits(sp.mask, sm, f"stage {s + 1} codes")
        assert_bits(sp.labels, sl, f"stage {s + 1} labels")
        assert_bits(sp.counts, sc, f"stage {s + 1} counts")
        points, counts = ops.point_cloud(sp.disp, cam, mask=sp.mask)
        clouds, wn = G.point_cloud(so, sm, None, camera_rows(cam, 1), 1.0, float("inf"))
        assert_bits(counts, wn, f"stage {s + 1} point count")
        assert 1 <= int(wn[0]) <= sc[0, 1]
        got = points.cpu().numpy()[0, :len(clouds[0])].reshape(-1).view(clouds[0].dtype)
        assert np.array_equal(got.view(np.uint8), clouds[0].view(np.uint8)), f"stage {s + 1}: points differ"


def _chain(model, left_path, right_path, tau, size, diff, fill, stages):
    """(colour of the filtered map, grey of the speckle codes, grey of the LR mask or None) per stage, through the Python API."""
    from lwsnet_amd import imageio as io
    from lwsnet_amd import ops
    l_in = io.to_input(io.crop_bottom_right(io.load_rgb(left_path)))[None]
    r_in = io.to_input(io.crop_bottom_right(io.load_rgb(right_path)))[None]
    if tau is None:
        disp, masks = model(l_in, r_in), [None] * 4
    else:
        res = model.forward_lr(l_in, r_in, tau=tau, fill=False)
        disp, masks = res.disp, res.mask
    files = []
    for s in stages:
        sp = ops.speckle_filter(disp[s], size, diff, mask=masks[s], fill=fill)
        files.append((io.disparity_to_color(sp.disp.cpu().numpy()[0, 0]), io.LR_MASK_GREY[sp.mask.cpu().numpy()[0, 0]],
                      None if tau is None else io.LR_MASK_GREY[masks[s].cpu().numpy()[0, 0]]))
    return files


def test_inference_cli_speckle(dev, model, tmp_path):
    from PIL import Image
    from lwsnet_amd import inference
    src = os.path.join(ROOT, "tests", "golden", "kitti_pair")
    for tag in ("sp", "splr", "plain"):
        (tmp_path / tag).mkdir()
        for n in ("left_test.png", "right_test.png"):
            shutil.copy(os.path.join(src, n), tmp_path / tag / n)
    lp = lambda tag: str(tmp_path / tag / "left_test.png")      # noqa: E731
    rp = lambda tag: str(tmp_path / tag / "right_test.png")     # noqa: E731
    written = inference.main(["--left_img", lp("sp"), "--synthetic_weights", "--speckle", "60", "--speckle_diff", "0.5"])
    assert [os.path.basename(p) for p in written] == ["1.png", "1_sp.png", "2.png", "2_sp.png", "3.png", "3_sp.png", "4.png", "4_sp.png"]
    want = _chain(model, lp("sp"), rp("sp"), None, 60, 0.5, False, range(4))
    removed = 0
    for s in range(4):
        assert np.array_equal(np.asarray(Image.open(written[2 * s])), want[s][0])
        g = Image.open(written[2 * s + 1])
        assert g.mode == "L" and np.array_equal(np.asarray(g), want[s][1])
        removed += int((want[s][1] == 64).sum())
    assert removed > 0, "the flags should remove something from this pair"
    # with the left-right check: <stem>_lr.png from the LR mask, <stem>_sp.png from the filter behind it, one fill for both
    written = inference.main(["--left_img", lp("splr"), "--synthetic_weights", "--speckle", "60", "--lr_check", "1", "--speckle_fill"])
    assert [os.path.basename(p) for p in written] == [f"{s}{t}.png" for s in (1, 2, 3, 4) for t in ("", "_lr", "_sp")]
    want = _chain(model, lp("splr"), rp("splr"), 1.0, 60, 1.0, True, range(4))
    for s in range(4):
        for k, j in ((0, 0), (1, 2), (2, 1)):               # colour, _lr (LR mask), _sp (codes)
            assert np.array_equal(np.asarray(Image.open(written[3 * s + k])), want[s][j]), (s, k)
    # without the flags: the files of a plain run, unchanged
    plain = inference.main(["--left_img", lp("plain"), "--synthetic_weights"])
    assert [os.path.basename(p) for p in plain] == ["1.png", "2.png", "3.png", "4.png"]
    from lwsnet_amd import imageio as io
    outs = model(io.to_input(io.crop_bottom_right(io.load_rgb(lp("plain"))))[None], io.to_input(io.crop_bottom_right(io.load_rgb(rp("plain"))))[None])
    for s in range(4):
        assert np.array_equal(np.asarray(Image.open(plain[s])), io.disparity_to_color(outs[s].numpy()[0, 0]))
    # directory mode: the stage-4 pair of files per frame
    l0 = np.asarray(Image.open(os.path.join(src, "left_test.png")).convert("RGB"))
    r0 = np.asarray(Image.open(os.path.join(src, "right_test.png")).convert("RGB"))
    kdir = tmp_path / "kitti"
    for d in ("image_2", "image_3"):
        (kdir / d).mkdir(parents=True)
    for i in range(2):
        Image.fromarray(np.roll(l0, 11 * i, axis=1)).save(kdir / "image_2" / f"{i:06d}_10.png")
        Image.fromarray(np.roll(r0, 11 * i, axis=1)).save(kdir / "image_3" / f"{i:06d}_10.png")
    out = tmp_path / "out_sp"
    written = inference.main(["--img_path", str(kdir), "--save_path", str(out), "--synthetic_weights", "--speckle", "60"])
    assert sorted(os.listdir(out)) == ["000000_10.png", "000000_10_sp.png", "000001_10.png", "000001_10_sp.png"] and len(written) == 4
    out_plain = tmp_path / "out_plain"
    inference.main(["--img_path", str(kdir), "--save_path", str(out_plain), "--synthetic_weights"])
    assert sorted(os.listdir(out_plain)) == ["000000_10.png", "000001_10.png"]
    for i in range(2):
        name = f"{i:06d}_10.png"
        color, grey, _ = _chain(model, str(kdir / "image_2" / name), str(kdir / "image_3" / name), None, 60, 1.0, False, [3])[0]
        assert np.array_equal(np.asarray(Image.open(out / name)), color)
        assert np.array_equal(np.asarray(Image.open(out / f"{i:06d}_10_sp.png")), grey)
        outs = model(io.to_input(io.crop_bottom_right(io.load_rgb(str(kdir / "image_2" / name))))[None],
                     io.to_input(io.crop_bottom_right(io.load_rgb(str(kdir / "image_3" / name))))[None])
        assert np.array_equal(np.asarray(Image.open(out_plain / name)), io.disparity_to_color(outs[3].numpy()[0, 0]))


def test_evaluate_cli_speckle(dev, model, tmp_path):
    from lwsnet_amd import datasets as D
    from lwsnet_amd import ops, synth
    root = str(tmp_path / "kitti") + "/"
    split = synth.write_kitti_tree(root, 4)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out_json = tmp_path / "sp.json"
    r = subprocess.run([sys.executable, "-m", "lwsnet_amd.evaluate", "--synthetic_weights", "--test_batch_size", "2", "--dataset",
                        "kitti2015", "--datapath", root, "--val_set", split, "--lr_check", "1", "--speckle", "60", "--speckle_diff",
                        "0.5", "--speckle_fill", "--json", str(out_json)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.load(open(out_json))
    ds = D.StereoPairs(*D.kitti2015_lists(root, split)[3:], training=False, kitti_set=True)
    vals, dens, lr_dens = [], [], []
    for i in range(0, 4, 2):
        items = [ds[j] for j in range(i, i + 2)]
        lr = model.forward_lr(np.stack([it[0] for it in items]), np.stack([it[1] for it in items]), tau=1.0, fill=False)
        gt = np.stack([it[2] for it in items]).astype(np.float32)
        row, drow = [], []
        for s in range(4):
            sp = ops.speckle_filter(lr.disp[s], 60, 0.5, mask=lr.mask[s], fill=True)
            d = sp.disp.cpu().numpy()[:, 0]
            H, W = d.shape[1:]
            mask = (gt > 0) & (gt < 192)
            e = np.abs(d - gt)
            row.append(float(((e[mask] > 3.) & (e[mask] / gt[mask] > 0.05)).sum()) / float(mask.sum()))
            drow.append(sp.counts[:, 1].cpu().numpy() / float(H * W))
        vals.append(row)
        dens.append(np.stack(drow))
        lr_dens.append(lr.density)
    assert res["per_batch"] == vals
    assert res["speckle_size"] == 60 and res["speckle_diff"] == 0.5 and res["lr_tau"] == 1.0
    assert res["speckle_density"] == [float(d) for d in np.concatenate(dens, axis=1).mean(axis=1)]
    assert res["lr_density"] == [float(d) for d in np.concatenate(lr_dens, axis=1).mean(axis=1)]
    assert "Speckle filter (size <= 60, diff <= 0.5, filled): mean kept density Stage 0=" in r.stderr
