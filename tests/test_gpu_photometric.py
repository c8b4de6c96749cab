"""The photometric reprojection error on the device: lws_photometric bit for bit against the numpy restatement
(tests/photometric_reference.py) -- err, scored, warped and sums -- at every height and width around the kernel's 16 x 64 tile, on
every kind of map and image, with and without the code map and the right valid map, for every subset of the optional outputs,
between poisoned guard bands at odd addresses, in any batch, and replayed from a captured graph; then end to end through
evaluate() and the inference CLI at 64 x 256 with the seeded weights."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import guarded as G
import photometric_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TH, TW = 16, 64                                                     # the shipped tile (lwsnet_amd/csrc/lws_photometric.hip)
HEIGHTS = [1, 2, 3, TH - 1, TH, TH + 1, TH + 2, 2 * TH + 1]
WIDTHS = [1, 2, 3, 4, 5, TW - 1, TW, TW + 1, TW + 2, 2 * TW + 3]
# a sparse cross: every height at a width just past the tile, every width at a height just past it, and the corners
SHAPES = sorted({(h, TW + 2) for h in HEIGHTS} | {(TH + 1, w) for w in WIDTHS} | {(1, 1), (3, 3), (2 * TH + 1, 2 * TW + 3), (TH, TW)})
OPTIONS = [(False, False, 0.85), (True, True, 0.0), (True, False, 1.0), (False, True, 0.85)]     # (mask, rvalid, alpha)
_REF = {}


def ref(key, fn):
    """References and inputs are computed once per case and shared; never modified."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


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


def host(t):
    return t.detach().cpu().numpy()


# ---- inputs ----
def ramps(B, H, W, seed):
    """Smooth ramps with jumps: slanted surfaces and plateaus in front of them."""
    rng = np.random.default_rng(seed)
    slope = rng.uniform(-0.3, 0.6, (B, 1, H, 1))
    d = rng.uniform(0.0, min(40.0, W / 2.0), (B, 1, H, 1)) + slope * np.arange(W) + rng.uniform(-0.2, 0.2, (B, 1, H, W))
    for _ in range(1 + W // 64):
        x0 = int(rng.integers(W))
        d[..., x0:x0 + int(rng.integers(1, max(2, W // 8)))] += rng.uniform(-20.0, 20.0)
    return d.astype(np.float32)


def noise(B, H, W, seed):
    """Far gathers and out-of-view pixels."""
    return np.random.default_rng(seed).uniform(-3.0, W + 3.0, (B, 1, H, W)).astype(np.float32)


def sprinkled(B, H, W, seed):
    d = ramps(B, H, W, seed)
    rng = np.random.default_rng(seed + 1)
    flat = d.reshape(-1)
    for v in (np.nan, np.inf, -np.inf, -0.0, 1e30):
        flat[rng.choice(flat.size, size=max(1, flat.size // 40), replace=False)] = v
    return d


def halves(B, H, W, seed):
    """Integer and half-integer disparities: one-tap warps and weights of exactly 0.5."""
    return (np.round(np.random.default_rng(seed).uniform(-1.0, W / 2.0 + 1.0, (B, 1, H, W)) * 2) / 2).astype(np.float32)


def images(B, H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8), rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)


def code_map(B, H, W, seed):
    """Codes 0..3, mostly 1; every code present once the map has four pixels."""
    rng = np.random.default_rng(seed)
    m = rng.choice(np.array([0, 1, 1, 1, 1, 1, 2, 3], np.uint8), (B, 1, H, W))
    flat = m.reshape(-1)
    flat[:4] = np.arange(4)[:flat.size]
    return m


def valid_map(B, H, W, seed):
    """Mostly 1, some 0 and a few 2 (anything but 1 makes a tap unusable)."""
    return np.random.default_rng(seed).choice(np.array([1, 1, 1, 1, 1, 1, 1, 0, 2], np.uint8), (B, 1, H, W))


def case(B, H, W):
    def make():
        left, right = images(B, H, W, 100 + W)
        return dict(disp=[ramps(B, H, W, W), noise(B, H, W, W + 1), sprinkled(B, H, W, W + 2), halves(B, H, W, W + 3)], left=left, right=right,
                    mask=[code_map(B, H, W, W + 10 + s) for s in range(4)], rvalid=valid_map(B, H, W, W + 20))
    return ref(("case", B, H, W), make)


def want(B, H, W, s, use_mask, use_rvalid, alpha):
    c = case(B, H, W)
    return ref(("want", B, H, W, s, use_mask, use_rvalid, alpha),
               lambda: R.photometric(c["disp"][s], c["left"], c["right"], c["mask"][s] if use_mask else None, c["rvalid"] if use_rvalid else None, alpha))


# ---- the raw call ----
def raw_call(lib, dev, disp, left, right, mask, rvalid, alpha, err, scored, warped, sums):
    """lws_photometric on torch's current stream; mask / err / scored / warped: None, or a list with None for the maps without one."""
    from lwsnet_amd import _lib
    arr = ctypes.c_void_p * 4
    p = lambda ts: arr(*[t.data_ptr() if t is not None else None for t in ts]) if ts is not None else arr()      # noqa: E731
    B, _, H, W = disp[0].shape
    with torch.cuda.device(dev):
        _lib.check(lib.lws_photometric(p(disp), len(disp), left.data_ptr(), right.data_ptr(), p(mask), rvalid.data_ptr() if rvalid is not None else None,
                                       B, H, W, float(alpha), p(err), p(scored), p(warped), sums.data_ptr(),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "lws_photometric")


def check_outputs(what, wants, err, scored, warped, sums):
    for s, w in enumerate(wants):
        if err is not None and err[s] is not None:
            G.assert_bits(err[s], w.err, f"{what} err {s}")
        if scored is not None and scored[s] is not None:
            G.assert_bits(scored[s], w.scored, f"{what} scored {s}")
        if warped is not None and warped[s] is not None:
            G.assert_bits(warped[s], w.warped, f"{what} warped {s}")
        G.assert_bits(sums[s], w.sums, f"{what} sums {s}")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_photometric_bitexact(dev, hip_lib, H, W, B):
    from lwsnet_amd import ops
    c = case(B, H, W)
    disp, left, right = [cu(d, dev) for d in c["disp"]], cu(c["left"], dev), cu(c["right"], dev)
    masks, rvalid = [cu(m, dev) for m in c["mask"]], cu(c["rvalid"], dev)
    n_scored = 0
    for nmaps in (1, 4):
        for use_mask, use_rvalid, alpha in OPTIONS:
            first = (nmaps + int(use_mask)) % 4 if nmaps == 1 else 0            # the single map is not always map 0
            sel = list(range(first, first + nmaps))
            res = ops.photometric([disp[s] for s in sel], left, right, [masks[s] for s in sel] if use_mask else None, rvalid if use_rvalid else None,
                                  alpha, want_err=True, want_scored=True, want_warped=True)
            wants = [want(B, H, W, s, use_mask, use_rvalid, alpha) for s in sel]
            check_outputs(f"B={B} {H}x{W} nmaps={nmaps} mask={use_mask} rvalid={use_rvalid} alpha={alpha}", wants, res.err, res.scored, res.warped,
                          res.sums)
            n_scored += sum(int(w.sums[:, 0].sum()) for w in wants)
    if H < 3 or W < 3:
        assert n_scored == 0
    elif H >= TH and W >= TW:
        assert n_scored > 0, "the inputs should score some pixels"


@pytest.mark.parametrize("kind", ["white", "black", "white-black", "noise-white"])
def test_constant_images(dev, hip_lib, kind):
    """Images that are constant 255 and constant 0: zero variance in every window, and the largest L1 there is."""
    from lwsnet_amd import ops
    B, H, W = 2, TH + 1, TW + 2
    c = case(B, H, W)
    full = lambda v: np.full((B, H, W, 3), v, np.uint8)             # noqa: E731
    left, right = {"white": (full(255), full(255)), "black": (full(0), full(0)), "white-black": (full(255), full(0)),
                   "noise-white": (c["left"], full(255))}[kind]
    sel = [0, 3]
    for alpha in (0.0, 0.85, 1.0):
        res = ops.photometric([cu(c["disp"][s], dev) for s in sel], cu(left, dev), cu(right, dev), alpha=alpha, want_scored=True, want_warped=True)
        wants = [R.photometric(c["disp"][s], left, right, alpha=alpha) for s in sel]
        check_outputs(f"{kind} alpha={alpha}", wants, res.err, res.scored, res.warped, res.sums)
        assert wants[0].sums[:, 0].sum() > 0
        if kind in ("white", "black"):
            assert not res.sums[:, :, 1:].any(), "identical constant images score exactly 0"
        if kind == "white-black" and alpha == 0.0:
            assert int(res.sums[0, 0, 1]) == int(res.sums[0, 0, 0]) << 20, "L1 of white against black is exactly 1"


@pytest.mark.parametrize("subset", list(itertools.product([False, True], repeat=3)), ids=lambda s: "".join("esw"[i] if on else "-" for i, on in enumerate(s)))
def test_every_subset_of_the_optional_outputs(dev, hip_lib, subset):
    from lwsnet_amd import ops
    B, H, W = 3, TH + 1, TW + 2
    c = case(B, H, W)
    e, s_, w = subset
    res = ops.photometric([cu(d, dev) for d in c["disp"]], cu(c["left"], dev), cu(c["right"], dev), [cu(m, dev) for m in c["mask"]], cu(c["rvalid"], dev), 0.85,
                          want_err=e, want_scored=s_, want_warped=w)
    assert (res.err is not None, res.scored is not None, res.warped is not None) == subset
    check_outputs(f"subset {subset}", [want(B, H, W, s, True, True, 0.85) for s in range(4)], res.err, res.scored, res.warped, res.sums)
    one = ops.photometric(cu(c["disp"][1], dev), cu(c["left"], dev), cu(c["right"], dev), cu(c["mask"][1], dev), cu(c["rvalid"], dev), 0.85,
                          want_err=e, want_scored=s_, want_warped=w)                # one tensor in: tensors out
    check_outputs("one map", [want(B, H, W, 1, True, True, 0.85)], *[[v] if v is not None else None for v in (one.err, one.scored, one.warped)], one.sums)


@pytest.mark.parametrize("word", G.FLOAT_WORDS + (G.BYTE_WORD,), ids=G.word_id)
@pytest.mark.parametrize("skew", [0, 1], ids=["aligned", "skewed"])
@pytest.mark.parametrize("optional", ["all", "mixed", "none"])
@pytest.mark.parametrize("B,H,W", [(2, TH + 2, TW + 3), (1, 3, 5)])
def test_memory_contract(dev, hip_lib, B, H, W, optional, skew, word):
    """Inputs between poisoned flanks, outputs between poisoned flanks with a poisoned interior, the uint8 images and maps at odd
    addresses when skewed: no flank changes, no poison is read into a result, and every output element is written."""
    c = case(B, H, W)
    sel = [1, 2]
    with_maps = optional != "none"
    wants = [want(B, H, W, s, with_maps, with_maps, 0.85) for s in sel]
    g = G.Guard(dev, word, skew)
    disp = [g.place(c["disp"][s], name=f"disp{s}") for s in sel]
    left, right = (g.place(c[k], plane=3 * H * W, name=k) for k in ("left", "right"))
    mask = [g.place(c["mask"][s], word=G.MASK_WORD, name=f"mask{s}") for s in sel] if with_maps else None
    rvalid = g.place(c["rvalid"], word=G.MASK_WORD, name="rvalid") if with_maps else None
    if skew:
        assert all(t.data_ptr() % 2 == 1 for t in [left, right] + (mask + [rvalid] if with_maps else []))
    err = [g.empty((B, 1, H, W), name=f"err{k}") for k in range(2)] if optional != "none" else None
    scored = [g.empty((B, 1, H, W), np.uint8, name=f"scored{k}") for k in range(2)] if optional == "all" else None
    warped = [g.empty((B, H, W, 3), np.uint8, plane=3 * H * W, name=f"warped{k}") for k in range(2)] if optional != "none" else None
    if optional == "mixed":                                         # one element NULL among the others
        err[0], warped[1] = None, None
    sums = g.empty((2, B, 4), np.int64, name="sums")
    raw_call(hip_lib, dev, disp, left, right, mask, rvalid, 0.85, err, scored, warped, sums)
    check_outputs("guarded", wants, err, scored, warped, sums)
    for k, s in enumerate(sel):
        G.assert_bits(disp[k], c["disp"][s], f"disp{s} is an input")
    G.assert_bits(left, c["left"], "left is an input")
    G.assert_bits(right, c["right"], "right is an input")
    g.check()


def test_batch_position_and_run_independence(dev, hip_lib):
    from lwsnet_amd import ops
    H, W = TH + 3, 2 * TW + 5
    c = case(3, H, W)
    d, left, right = c["disp"][2].copy(), c["left"].copy(), c["right"].copy()
    for a in (d, left, right):
        a[2] = a[0]                                                 # the same image at positions 0 and 2
    args = ([cu(d, dev), cu(c["disp"][1], dev)], cu(left, dev), cu(right, dev))
    runs = [ops.photometric(*args, want_scored=True, want_warped=True) for _ in range(2)]
    alone = ops.photometric(cu(d[:1], dev), cu(left[:1], dev), cu(right[:1], dev), want_scored=True, want_warped=True)
    for name in ("err", "scored", "warped"):
        a, b = getattr(runs[0], name), getattr(runs[1], name)
        for s in range(2):
            G.assert_bits(a[s], host(b[s]), f"{name}[{s}] across two runs")
        G.assert_bits(a[0][2], host(a[0][0]), f"{name} at positions 0 and 2")
        G.assert_bits(getattr(alone, name)[0], host(a[0][0]), f"{name} alone and in a batch")
    G.assert_bits(runs[0].sums, host(runs[1].sums), "sums across two runs")
    G.assert_bits(runs[0].sums[0, 2], host(runs[0].sums[0, 0]), "sums at positions 0 and 2")
    G.assert_bits(alone.sums[0, 0], host(runs[0].sums[0, 0]), "sums alone and in a batch")
    for s in range(2):                                              # the count and the pe column, per image, from the returned maps
        G.assert_bits(runs[0].sums[s, :, :2], R.sums_from_err(host(runs[0].err[s]), host(runs[0].scored[s])), f"sums[{s}] recomputed from err and scored")
    assert int(runs[0].sums[0, 0, 0]) > 0


def test_graph_capture_replays_the_call(dev, hip_lib):
    from lwsnet_amd import ops
    B, H, W = 2, TH + 1, TW + 2
    sets = [(ramps(B, H, W, 41), noise(B, H, W, 42), *images(B, H, W, 43)), (halves(B, H, W, 44), sprinkled(B, H, W, 45), *images(B, H, W, 46))]
    disp = [cu(sets[0][0], dev), cu(sets[0][1], dev)]
    left, right = cu(sets[0][2], dev), cu(sets[0][3], dev)
    err = [torch.empty_like(d) for d in disp]
    scored = [torch.empty(d.shape, dtype=torch.uint8, device=dev) for d in disp]
    warped = [torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) for _ in disp]
    sums = torch.empty((2, B, 4), dtype=torch.int64, device=dev)
    call = lambda: raw_call(hip_lib, dev, disp, left, right, None, None, 0.85, err, scored, warped, sums)        # noqa: E731
    call()                                                          # the code object is loaded before the capture
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for d0, d1, l, r in reversed(sets):                             # new inputs first
        for t, a in zip(disp + [left, right], (d0, d1, l, r)):
            t.copy_(cu(a, dev))
        for t in err + scored + warped:
            t.zero_()
        sums.fill_(-1)
        graph.replay()
        torch.cuda.synchronize(dev)
        eager = ops.photometric([cu(d0, dev), cu(d1, dev)], cu(l, dev), cu(r, dev), want_scored=True, want_warped=True)
        for s in range(2):
            G.assert_bits(err[s], host(eager.err[s]), "replayed err against the eager call")
            G.assert_bits(scored[s], host(eager.scored[s]), "replayed scored against the eager call")
            G.assert_bits(warped[s], host(eager.warped[s]), "replayed warped against the eager call")
        G.assert_bits(sums, host(eager.sums), "replayed sums against the eager call")
        check_outputs("replay against the reference", [R.photometric(d, l, r) for d in (d0, d1)], err, scored, warped, sums)


def test_ops_validates_its_arguments(dev):
    from lwsnet_amd import ops
    d = torch.zeros((2, 1, 8, 16), device=dev)
    img = torch.zeros((2, 8, 16, 3), dtype=torch.uint8, device=dev)
    m = torch.ones((2, 1, 8, 16), dtype=torch.uint8, device=dev)
    for bad in (lambda: ops.photometric([], img, img), lambda: ops.photometric([d] * 5, img, img), lambda: ops.photometric(d, img[:1], img),
                lambda: ops.photometric(d, img, img.float()), lambda: ops.photometric(d, img, img, alpha=1.5),
                lambda: ops.photometric(d, img, img, alpha=float("nan")), lambda: ops.photometric(d, img, img, mask=m[:1]),
                lambda: ops.photometric([d, d], img, img, mask=[m]), lambda: ops.photometric(d, img, img, rvalid=m.float()),
                lambda: ops.photometric(d.double(), img, img)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        ops.photometric(d.cpu(), img, img)
    res = ops.photometric([d, d], img, img, mask=[m, None], rvalid=m)
    assert res.scored is None and res.warped is None and tuple(res.sums.shape) == (2, 2, 4)
    assert res.sums[:, :, 0].tolist() == [[6 * 14] * 2] * 2 and not res.sums[:, :, 1:].any()


# ---- end to end at 64 x 256, seeded weights ----
EH, EW = 64, 256


@pytest.fixture()
def small_crops(monkeypatch):
    """Both CLIs crop a frame's bottom-right 368 x 1232 window; here 64 x 256."""
    from lwsnet_amd import datasets, imageio
    monkeypatch.setattr(datasets, "KITTI_EVAL_CROP", (EH, EW))
    full = imageio.crop_bottom_right
    monkeypatch.setattr(imageio, "crop_bottom_right", lambda img: full(img, EH, EW))


@pytest.mark.parametrize("chain", [{}, dict(occ_check=1.0)], ids=["plain", "occ_check"])
def test_evaluate_photometric_end_to_end(tmp_path, dev, model, small_crops, chain):
    from lwsnet_amd import datasets as D
    from lwsnet_amd import ops, synth
    from lwsnet_amd.evaluate import evaluate
    from lwsnet_amd.metrics import photometric_means
    from lwsnet_amd.postprocess import Options, run_chain
    root = str(tmp_path / "kitti") + "/"
    split = synth.write_kitti_tree(root, 3, H=EH + 6, W=EW + 10)
    ds = D.StereoPairs(*D.kitti2015_lists(root, split)[3:], training=False, kitti_set=True)
    plain = evaluate(model, ds, "kitti", batch_size=2, **chain)
    res = evaluate(model, ds, "kitti", batch_size=2, photometric=True, photo_alpha=0.7, **chain)
    assert "photometric" not in plain
    assert sorted(set(res) - set(plain)) == ["photometric"]
    for k in plain:
        if k not in ("wall_s", "pairs_per_s"):
            assert res[k] == plain[k], k
    sums = []
    for rng in ([0, 1], [2]):
        items, raws = [ds[i] for i in rng], [ds.raw(i) for i in rng]
        out = run_chain(model, np.stack([t[0] for t in items]), np.stack([t[1] for t in items]), Options.make(**chain))
        assert (out.keep is not None) == bool(chain)
        sums.append(host(ops.photometric(list(out.disp), cu(np.stack([t[0] for t in raws]), dev), cu(np.stack([t[1] for t in raws]), dev), mask=out.keep,
                                         alpha=0.7, want_err=False).sums))
    sums = np.concatenate(sums, axis=1)
    ph = res["photometric"]
    want_m = photometric_means(sums, EH * EW)
    print("photometric:", {k: ph[k] for k in ("pe", "l1", "dssim", "density")})
    assert ph["alpha"] == 0.7 and all(ph[k] == want_m[k] for k in want_m)
    for i in range(3):
        each = photometric_means(sums[:, i:i + 1], EH * EW)
        assert all(ph["per_image"][k][i] == each[k] for k in ("pe", "l1", "dssim", "density"))
    assert all(0.0 < d <= 1.0 for d in ph["density"]) and all(0.0 <= e <= 1.0 for e in ph["pe"])
    if chain:
        assert ph["density"][3] < (EH - 2) * (EW - 2) / (EH * EW), "the codes must drop pixels, or the mask shows nothing"


def test_inference_cli_writes_the_photometric_files(tmp_path, dev, model, small_crops, caplog):
    from PIL import Image

    from lwsnet_amd import imageio as io
    from lwsnet_amd import inference, synth
    root = str(tmp_path / "kitti") + "/"
    synth.write_kitti_tree(root, 1, H=EH + 6, W=EW + 10)
    out = str(tmp_path / "out")
    with caplog.at_level("INFO"):
        written = inference.main(["--synthetic_weights", "--img_path", root, "--save_path", out, "--photometric", "--save_photo"])
    stem = os.path.join(out, "000000_10")
    assert written == [stem + ".png", stem + "_pe.png", stem + "_warp.png"]
    assert "Photometric (alpha = 0.85): Stage 1 = " in caplog.text
    left = io.crop_bottom_right(io.load_rgb(os.path.join(root, "image_2", "000000_10.png")))
    right = io.crop_bottom_right(io.load_rgb(os.path.join(root, "image_3", "000000_10.png")))
    disp = model(io.to_input(left)[None], io.to_input(right)[None])[3].numpy()
    w = R.photometric(disp, left[None], right[None], alpha=0.85)
    assert w.sums[0, 0] > 0
    with open(stem + "_pe.png", "rb") as f:
        assert f.read() == io.encode_png_gray(inference.photo_to_u8(w.err[0, 0]))
    G.assert_bits(np.asarray(Image.open(stem + "_pe.png")), np.rint(w.err[0, 0].astype(np.float64) * 255.0).astype(np.uint8), "<stem>_pe.png")
    G.assert_bits(np.asarray(Image.open(stem + "_warp.png").convert("RGB")), w.warped[0], "<stem>_warp.png")


def test_inference_cli_rectify_photometric(tmp_path, dev, model):
    """--rectify --photometric --save_photo on the golden pair taken as raw frames, in process: the left valid map is the mask, the
    right one is rvalid, and the files of every stage are the restatement's on ops.rectify_pair's crops."""
    import dataclasses
    import shutil

    from PIL import Image

    import rectify_reference as RR
    from conftest import ROOT
    from lwsnet_amd import imageio as io
    from lwsnet_amd import inference, ops
    from lwsnet_amd.geometry import RectifyCalib
    for n in ("left_test.png", "right_test.png"):
        shutil.copy(os.path.join(ROOT, "tests", "golden", "kitti_pair", n), tmp_path / n)
    rig = RR.kitti_like_calib((375, 1242))[0]
    shifted = [p.copy() for p in rig.P_rect]
    for p in shifted:
        p[0, 2] += 200.0                                            # both rectified views look 200 px past the raw images' left edge
    path = RR.write_kitti(tmp_path / "calib_cam_to_cam.txt", dataclasses.replace(rig, P_rect=tuple(shifted)))
    written = inference.main(["--left_img", str(tmp_path / "left_test.png"), "--synthetic_weights", "--rectify", path, "--photometric",
                              "--photo_alpha", "0.5", "--save_photo"])
    assert sorted(os.path.basename(w) for w in written) == sorted(f"{s}{t}" for s in (1, 2, 3, 4) for t in (".png", "_pe.png", "_warp.png"))
    calib = RectifyCalib.from_kitti(path)
    raws = [cu(io.load_rgb(str(tmp_path / n))[None], dev) for n in ("left_test.png", "right_test.png")]
    with torch.cuda.device(dev):
        got = ops.rectify_pair(raws[0], raws[1], calib.params(), (io.CROP_H, io.CROP_W), origin=(375 - io.CROP_H, 1242 - io.CROP_W))
    disp = model(got["input"][0], got["input"][1])
    left, right, valid_l, valid_r = (host(got[k][c]) for k, c in (("rect", 0), ("rect", 1), ("valid", 0), ("valid", 1)))
    assert (valid_l == 0).any() and (valid_r == 0).any(), "the valid maps must drop pixels, or they show nothing"
    for s in range(4):
        w = R.photometric(disp[s].numpy(), left, right, mask=valid_l, rvalid=valid_r, alpha=0.5)
        assert w.sums[0, 0] > 0
        G.assert_bits(np.asarray(Image.open(tmp_path / f"{s + 1}_pe.png")), inference.photo_to_u8(w.err[0, 0]), f"{s + 1}_pe.png")
        G.assert_bits(np.asarray(Image.open(tmp_path / f"{s + 1}_warp.png").convert("RGB")), w.warped[0], f"{s + 1}_warp.png")
