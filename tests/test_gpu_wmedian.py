"""The weighted median filter on the device: lws_wmedian_filter bit for bit against the numpy restatement
(tests/wmedian_reference.py) over radius x mask x guide table x fill_min x counts on the shapes below, on every speckle_inputs kind,
batch independence, run-to-run identity, guard bands and poisoned outputs, hipGraph capture, the chain forward_lr -> speckle_filter
-> wmedian_filter -> point_cloud, and the --wmedian flags of the two CLIs.

The kernel's tile is TILE_H x TILE_W = 16 x 64 output pixels per workgroup with a halo of `radius`.  The shapes are the smallest
that reach every path of it: a single pixel; one column and one row (the window clipped to a line, W = 300: five tiles, the last
ragged); 63 x 255 with B = 2 (odd, every row base misaligned, the window clipped on all four sides, ragged tiles in both
directions); 2 x 2 whole tiles plus a remainder in both directions; and an image smaller than the 7 x 7 window."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import geometry_reference as GEO
import guarded as G
import speckle_inputs as I
import wmedian_reference as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILE_H, TILE_W = 16, 64
SHAPES = [(1, 1, 1), (1, 8, 1), (1, 1, 300), (2, 63, 255), (1, 2 * TILE_H + 8, 2 * TILE_W + 22), (1, 3, 5)]
RADII = (1, 2, 3)


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


def noise_map(B, H, W, seed):
    """Uniform noise in 0.5 .. 60 with holes (0.0f on one pixel in six, some of them in blocks), runs of equal values along rows,
    and the values a disparity map must survive: -0.0f, negatives, NaN, +-inf and denormals."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 60.0, (B, 1, H, W)).astype(np.float32)
    flat = d.reshape(-1)
    for _ in range(max(1, flat.size // 400)):               # long runs of equal values (ties)
        i, n = int(rng.integers(0, flat.size)), int(rng.integers(2, 40))
        flat[i:i + n] = flat[i]
    for _ in range(max(1, H * W // 600)):                   # holes of up to 4 x 6 pixels
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        d[:, :, y:y + int(rng.integers(1, 5)), x:x + int(rng.integers(1, 7))] = 0.0
    idx = rng.integers(0, flat.size, (7, max(1, flat.size // 150)))
    for row, v in zip(idx, (0.0, -0.0, -2.5, np.nan, np.inf, -np.inf, 1e-41)):
        flat[row] = np.float32(v)
    flat[rng.integers(0, flat.size, max(1, flat.size // 6))] = 0.0
    return d


def mask_codes(B, H, W, seed):
    """speckle_inputs.random_mask (codes 0, 1, 2) with the speckle filter's code 3 on one pixel in fifty."""
    m = I.random_mask(B, H, W, seed)
    rng = np.random.default_rng(seed + 1)
    m[rng.uniform(size=m.shape) < 0.02] = 3
    return m


def guide(B, H, W, seed):
    """A few constant colour regions, every other one with noise of a few grey levels on half of its pixels: s covers 0 (on whole
    windows inside the quiet regions), values below and values far above the cutoff of a small sigma."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    K = 6
    cy, cx = rng.uniform(0, H, K), rng.uniform(0, W, K)
    region = np.argmin((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2, axis=0)
    colour = rng.integers(0, 256, (K, 3))
    noisy = (rng.uniform(size=(B, H, W, 1)) < 0.5) & (region % 2 == 0)[None, :, :, None]
    g = colour[region][None] + rng.integers(-3, 4, (B, H, W, 3)) * noisy
    return np.clip(g, 0, 255).astype(np.uint8)


def tables():
    from lwsnet_amd import ops
    zero_self = np.full(R.LUT_SIZE, 5, np.uint16)
    zero_self[0] = 0                                        # wlut[0] == 0: a pixel is not its own candidate; T == 0 happens
    return {"none": None, "lut2": ops.wmedian_lut(2.0), "lut40": ops.wmedian_lut(40.0), "ones": np.ones(R.LUT_SIZE, np.uint16),
            "max": np.full(R.LUT_SIZE, 65535, np.uint16), "zero_self": zero_self}


_parts = {}


def parts(key, d, m, rgb, wlut, radius):
    """The reference's window medians, computed once per input and shared (fill_min only enters wmedian_reference.apply)."""
    if key not in _parts:
        _parts[key] = R.window_median(d, m, rgb, wlut, radius)
    return _parts[key]


def raw_call(lib, dev, d, m, rgb, wlut, radius, fill_min, out, counts):
    from lwsnet_amd import _lib
    B, _, H, W = d.shape
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(lib.lws_wmedian_filter(p(d), p(m), p(rgb), p(wlut), B, H, W, radius, fill_min, p(out), p(counts),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "lws_wmedian_filter")


def inputs(B, H, W):
    d = noise_map(B, H, W, 5 * H + W)
    if B > 1:
        d[1] = I.plateaus(1, H, W, H + W)[0]
        d[1].reshape(-1)[np.random.default_rng(W).integers(0, H * W, H * W // 8)] = 0.0
    return d, mask_codes(B, H, W, H + 7 * W), guide(B, H, W, 3 * H + W)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_wmedian_filter_bitexact(dev, hip_lib, B, H, W, radius):
    """mask x guide table x fill_min through ops (counts on), and every (mask, table) once more through ctypes with counts = NULL."""
    from lwsnet_amd import ops
    d_np, m_np, g_np = inputs(B, H, W)
    d, g = cu(d_np, dev), cu(g_np, dev)
    never = (2 * radius + 1) ** 2 + 1
    changed = filled = 0
    for masked in (False, True):
        m = cu(m_np, dev) if masked else None
        for name, wlut in tables().items():
            rgb_np = None if wlut is None else g_np
            pt = parts((B, H, W, radius, masked, name), d_np, m_np if masked else None, rgb_np, wlut, radius)
            wl = cu(wlut, dev)
            for fill_min in (0, 1, 4, never):
                what = f"B={B} {H}x{W} radius={radius} mask={masked} table={name} fill_min={fill_min}"
                want, wc = R.apply(d_np, pt, fill_min)
                res = ops.wmedian_filter(d, radius, rgb=None if wlut is None else g, wlut=wl, mask=m, fill_min=fill_min)
                G.assert_bits(res.disp, want, what + " out")
                G.assert_bits(res.counts, wc, what + " counts")
                if fill_min == never:
                    assert wc[:, 1].sum() == 0
                if fill_min == 4:
                    changed += int(wc[:, 0].sum())
                    filled += int(wc[:, 1].sum())
                    out = torch.full_like(d, -1.0)
                    raw_call(hip_lib, dev, d, m, None if wlut is None else g, wl, radius, fill_min, out, None)
                    G.assert_bits(out, want, what + " out (counts = NULL)")
            if name == "zero_self" and H * W >= 40 * 150:
                assert (pt[3][pt[0]] == 0).any(), "the inputs should reach T == 0 on a valid pixel"
    if H * W >= 40 * 150:
        assert changed > 0 and filled > 0, "the reference must change and fill pixels, or the comparison shows nothing"


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("kind", I.KINDS)
def test_wmedian_filter_bitexact_on_every_kind(dev, hip_lib, kind, radius):
    from lwsnet_amd import ops
    B, H, W = 1, 2 * TILE_H + 8, 2 * TILE_W + 22
    d_np, m_np, g_np = I.make(kind, B, H, W, 3 * H + W), mask_codes(B, H, W, 11), guide(B, H, W, 12)
    d, m, g = cu(d_np, dev), cu(m_np, dev), cu(g_np, dev)
    for name in ("none", "lut2"):
        wlut = tables()[name]
        want, wc = R.wmedian_filter(d_np, radius, None if wlut is None else g_np, wlut, m_np, 4)
        res = ops.wmedian_filter(d, radius, rgb=None if wlut is None else g, wlut=wlut, mask=m, fill_min=4)
        G.assert_bits(res.disp, want, f"{kind} radius={radius} table={name} out")
        G.assert_bits(res.counts, wc, f"{kind} radius={radius} table={name} counts")


def test_wmedian_filter_is_batch_independent(dev, hip_lib):
    from lwsnet_amd import ops
    H, W = 63, 255
    d, m, g = noise_map(3, H, W, 77), mask_codes(3, H, W, 78), guide(3, H, W, 79)
    kw = dict(radius=2, wlut=ops.wmedian_lut(10.0), fill_min=4)
    alone = ops.wmedian_filter(cu(d[1:2], dev), rgb=cu(g[1:2], dev), mask=cu(m[1:2], dev), **kw)
    batch = ops.wmedian_filter(cu(d, dev), rgb=cu(g, dev), mask=cu(m, dev), **kw)
    d2, m2, g2 = noise_map(3, H, W, 80), mask_codes(3, H, W, 81), guide(3, H, W, 82)
    d2[0], m2[0], g2[0] = d[1], m[1], g[1]
    first = ops.wmedian_filter(cu(d2, dev), rgb=cu(g2, dev), mask=cu(m2, dev), **kw)
    for k, what in enumerate(("out", "counts")):
        G.assert_bits(batch[k][1:2], alone[k].cpu().numpy(), what + " in the middle of three")
        G.assert_bits(first[k][0:1], alone[k].cpu().numpy(), what + " first of three")
    assert int(alone.counts.sum()) > 0


def test_wmedian_filter_is_run_to_run_identical(dev, hip_lib):
    from lwsnet_amd import ops
    B, H, W = 2, 63, 255
    d, m, g = cu(noise_map(B, H, W, 5), dev), cu(mask_codes(B, H, W, 6), dev), cu(guide(B, H, W, 7), dev)
    wlut = cu(ops.wmedian_lut(10.0), dev)
    runs = [ops.wmedian_filter(d, 3, rgb=g, wlut=wlut, mask=m, fill_min=1) for _ in range(4)]
    for r in runs[1:]:
        G.assert_bits(r.disp, runs[0].disp.cpu().numpy(), "out")
        G.assert_bits(r.counts, runs[0].counts.cpu().numpy(), "counts")


def test_all_ones_table_equals_no_guide_on_the_device(dev, hip_lib):
    from lwsnet_amd import ops
    B, H, W = 2, 63, 255
    d, m, g = cu(noise_map(B, H, W, 15), dev), cu(mask_codes(B, H, W, 16), dev), cu(guide(B, H, W, 17), dev)
    for radius in RADII:
        a = ops.wmedian_filter(d, radius, rgb=g, wlut=np.ones(R.LUT_SIZE, np.uint16), mask=m, fill_min=4)
        b = ops.wmedian_filter(d, radius, mask=m, fill_min=4)
        G.assert_bits(a.disp, b.disp.cpu().numpy(), f"radius={radius} out")
        G.assert_bits(a.counts, b.counts.cpu().numpy(), f"radius={radius} counts")


@pytest.mark.parametrize("word", G.FLOAT_WORDS, ids=G.word_id)
@pytest.mark.parametrize("B,H,W", [(2, 63, 255), (1, 1, 300), (1, 3, 5)])
def test_guard_bands_and_poisoned_outputs(dev, hip_lib, B, H, W, word):
    """Inputs between poisoned flanks, out and counts between poisoned flanks with poisoned interiors, every base skewed by one
    element: nothing outside an output is written, every output element is, and no halo read reaches past an input."""
    from lwsnet_amd import ops
    d_np, m_np, g_np = inputs(B, H, W)
    wlut = ops.wmedian_lut(10.0)
    for radius in RADII:
        want, wc = R.apply(d_np, parts((B, H, W, radius, True, "lut10"), d_np, m_np, g_np, wlut, radius), 4)
        g = G.Guard(dev, word, skew=1)
        disp, mask = g.place(d_np, name="disp"), g.place(m_np, word=G.MASK_WORD, name="mask")
        rgb, wl = g.place(g_np, plane=3 * H * W, name="rgb"), g.place(wlut, name="wlut")
        out, counts = g.empty((B, 1, H, W), name="out"), g.empty((B, 2), np.int64, align16=True, name="counts")
        raw_call(hip_lib, dev, disp, mask, rgb, wl, radius, 4, out, counts)
        G.assert_bits(out, want, f"radius={radius} out")
        G.assert_bits(counts, wc, f"radius={radius} counts")
        G.assert_bits(disp, d_np, "disp is only read")
        g.check()
        # no optional argument: the unweighted median, every pixel, no counts
        want, _ = R.apply(d_np, parts((B, H, W, radius, False, "none"), d_np, None, None, None, radius), 0)
        g = G.Guard(dev, word, skew=1)
        disp, out = g.place(d_np, name="disp"), g.empty((B, 1, H, W), name="out")
        raw_call(hip_lib, dev, disp, None, None, None, radius, 0, out, None)
        G.assert_bits(out, want, f"radius={radius} out (no optional argument)")
        g.check()


def test_graph_capture_replays_the_filter(dev, hip_lib):
    from lwsnet_amd import ops
    B, H, W = 2, 63, 255
    first, second = noise_map(B, H, W, 21), I.plateaus(B, H, W, 22)
    m1, m2 = mask_codes(B, H, W, 23), mask_codes(B, H, W, 24)
    g1, g2 = guide(B, H, W, 25), guide(B, H, W, 26)
    wlut_np = ops.wmedian_lut(10.0)
    d, m, g, wlut = cu(first, dev), cu(m1, dev), cu(g1, dev), cu(wlut_np, dev)
    out = torch.empty_like(d)
    counts = torch.empty((B, 2), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_call(hip_lib, dev, d, m, g, wlut, 3, 4, out, counts)
    for d_np, m_np, g_np in ((first, m1, g1), (second, m2, g2)):
        d.copy_(cu(d_np, dev))
        m.copy_(cu(m_np, dev))
        g.copy_(cu(g_np, dev))
        graph.replay()
        torch.cuda.synchronize(dev)
        eager = ops.wmedian_filter(cu(d_np, dev), 3, rgb=cu(g_np, dev), wlut=wlut, mask=cu(m_np, dev), fill_min=4)
        G.assert_bits(out, eager.disp.cpu().numpy(), "replay out")
        G.assert_bits(counts, eager.counts.cpu().numpy(), "replay counts")
        want, wc = R.wmedian_filter(d_np, 3, g_np, wlut_np, m_np, 4)
        G.assert_bits(out, want, "replay out against the reference")
        G.assert_bits(counts, wc, "replay counts against the reference")


# The reference chain on synth.make_pair(64, 256, 0), stage 4 (the C oracle's forward, tests/lr_reference.py and
# tests/speckle_reference.py): tau = 2 keeps 363 pixels, the speckle filter at max_size 1 keeps 83 of them (the synthetic weights
# give a rough map), and the 5 x 5 median with fill_min 4 then changes 26 and fills 74.  The test asserts that pixels are kept and
# holes are filled, so a choice that no longer fits fails here, not silently.
def test_forward_lr_speckle_wmedian_point_cloud_chain(dev, model):
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import Camera, camera_rows
    from lwsnet_amd.synth import make_pair, to_rgb8
    H, W = 64, 256
    left, right = make_pair(H, W, 0)[:2]
    left_u8 = to_rgb8(left)                                             # the uint8 image the left input was normalised from
    cam = Camera(721.5, 721.5, 127.5, 31.5, 0.54)
    res = model.forward_lr(left[None], right[None], tau=2.0, fill=False)
    sp = ops.speckle_filter(res.disp[3], 1, 1.0, mask=res.mask[3], fill=False)
    rgb = cu(left_u8[None], dev)
    wlut = ops.wmedian_lut(10.0)
    wm = ops.wmedian_filter(sp.disp, 2, rgb=rgb, wlut=wlut, mask=sp.mask, fill_min=4)
    d_np, m_np = sp.disp.cpu().numpy(), sp.mask.cpu().numpy()
    want, wc = R.wmedian_filter(d_np, 2, left_u8[None], wlut, m_np, 4)
    print(f"chain: kept {int((m_np == 1).sum())} of {H * W}, changed {int(wc[0, 0])}, filled {int(wc[0, 1])}")
    assert (m_np == 1).any() and int(wc[0, 1]) > 0, "the chain must keep pixels and fill holes, or the comparison shows nothing"
    G.assert_bits(wm.disp, want, "filtered map")
    G.assert_bits(wm.counts, wc, "counts")
    points, counts = ops.point_cloud(wm.disp, cam, rgb=rgb)             # a filled map: no mask
    clouds, wn = GEO.point_cloud(want, None, left_u8[None], camera_rows(cam, 1), 1.0, float("inf"))
    G.assert_bits(counts, wn, "point count")
    got = points.cpu().numpy()[0, :len(clouds[0])].reshape(-1).view(clouds[0].dtype)
    assert np.array_equal(got.view(np.uint8), clouds[0].view(np.uint8)), "points differ"


def _run(argv, tmp_path, timeout=300):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m"] + argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]
    return r


def test_inference_cli_wmedian(dev, model, tmp_path):
    from PIL import Image
    from lwsnet_amd import imageio as io
    from lwsnet_amd import ops
    src = os.path.join(ROOT, "tests", "golden", "kitti_pair")
    for tag in ("wm", "lr"):
        (tmp_path / tag).mkdir()
        for n in ("left_test.png", "right_test.png"):
            shutil.copy(os.path.join(src, n), tmp_path / tag / n)
    lp = lambda tag: str(tmp_path / tag / "left_test.png")      # noqa: E731
    r = _run(["lwsnet_amd.inference", "--left_img", lp("wm"), "--synthetic_weights", "--lr_check", "1", "--wmedian", "2",
              "--wmedian_fill", "4"], tmp_path)
    assert "Weighted median (radius 2, sigma 10, fill 4): stage 4 changed = " in r.stderr
    _run(["lwsnet_amd.inference", "--left_img", lp("lr"), "--synthetic_weights", "--lr_check", "1"], tmp_path)
    names = sorted(f"{s}{t}.png" for s in (1, 2, 3, 4) for t in ("", "_lr"))
    for tag in ("wm", "lr"):
        assert sorted(n for n in os.listdir(tmp_path / tag) if n[0].isdigit()) == names, "the filter writes no file of its own"
    left = io.crop_bottom_right(io.load_rgb(lp("wm")))
    right = io.crop_bottom_right(io.load_rgb(str(tmp_path / "wm" / "right_test.png")))
    res = model.forward_lr(io.to_input(left)[None], io.to_input(right)[None], tau=1.0, fill=False)
    rgb, wlut = cu(left[None], dev), ops.wmedian_lut(10.0)
    differ = 0
    for s in range(4):
        wm = ops.wmedian_filter(res.disp[s], 2, rgb=rgb, wlut=wlut, mask=res.mask[s], fill_min=4)
        got = np.asarray(Image.open(tmp_path / "wm" / f"{s + 1}.png"))
        assert np.array_equal(got, io.disparity_to_color(wm.disp.cpu().numpy()[0, 0])), f"stage {s + 1}"
        # without the flags: the files of the checked maps, unchanged
        plain = np.asarray(Image.open(tmp_path / "lr" / f"{s + 1}.png"))
        assert np.array_equal(plain, io.disparity_to_color(res.disp[s].numpy()[0, 0])), f"stage {s + 1} without --wmedian"
        for t in ("wm", "lr"):
            assert np.array_equal(np.asarray(Image.open(tmp_path / t / f"{s + 1}_lr.png")), io.LR_MASK_GREY[res.mask[s].cpu().numpy()[0, 0]])
        differ += int((got != plain).any())
    assert differ > 0, "the flags should change something on this pair"


def test_evaluate_cli_wmedian(dev, model, tmp_path):
    from lwsnet_amd import datasets as D
    from lwsnet_amd import ops, synth
    root = str(tmp_path / "kitti") + "/"
    split = synth.write_kitti_tree(root, 2)
    out_json = tmp_path / "wm.json"
    r = _run(["lwsnet_amd.evaluate", "--synthetic_weights", "--test_batch_size", "2", "--dataset", "kitti2015", "--datapath", root,
              "--val_set", split, "--lr_check", "1", "--wmedian", "1", "--wmedian_sigma", "5", "--wmedian_fill", "3", "--json",
              str(out_json)], tmp_path)
    res = json.load(open(out_json))
    ds = D.StereoPairs(*D.kitti2015_lists(root, split)[3:], training=False, kitti_set=True)
    items, raws = [ds[j] for j in range(2)], [ds.raw(j) for j in range(2)]
    lr = model.forward_lr(np.stack([it[0] for it in items]), np.stack([it[1] for it in items]), tau=1.0, fill=False)
    gt = np.stack([it[2] for it in items]).astype(np.float32)
    rgb, wlut = cu(np.stack([it[0] for it in raws]), dev), ops.wmedian_lut(5.0)
    row, frac = [], []
    for s in range(4):
        wm = ops.wmedian_filter(lr.disp[s], 1, rgb=rgb, wlut=wlut, mask=lr.mask[s], fill_min=3)
        d = wm.disp.cpu().numpy()[:, 0]
        H, W = d.shape[1:]
        mask = (gt > 0) & (gt < 192)
        e = np.abs(d - gt)
        row.append(float(((e[mask] > 3.) & (e[mask] / gt[mask] > 0.05)).sum()) / float(mask.sum()))
        frac.append(wm.counts.sum(dim=1).cpu().numpy() / float(H * W))
    assert res["per_batch"] == [row]
    assert res["wmedian_radius"] == 1 and res["wmedian_sigma"] == 5.0 and res["wmedian_fill"] == 3 and res["lr_tau"] == 1.0
    assert res["wmedian_changed"] == [float(f) for f in np.stack(frac).mean(axis=1)]
    assert all(f > 0 for f in res["wmedian_changed"])
    assert "Weighted median (radius 1, sigma 5, fill 3): mean changed fraction Stage 0=" in r.stderr
