"""The photometric reprojection error without a GPU: the float32 restatement of lws_photometric (tests/photometric_reference.py)
held to an independent float64 evaluation, its exact properties, its ranking of disparity maps on a geometrically consistent pair,
its scoring rules, and the host side: metrics.photometric_means, the CLIs' flags, the header against the ctypes prototype and the
entry point's argument errors."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

import photometric_reference as R
from conftest import ROOT

F = np.float32


# ---- inputs ----
def box_blur(a, k=5):
    """[H,W,3] float64 -> the k x k box mean with edge replication."""
    r = k // 2
    p = np.pad(a, ((r, r), (r, r), (0, 0)), mode="edge")
    return sliding_window_view(p, (k, k), axis=(0, 1)).mean(axis=(-1, -2))


def consistent_pair(H=24, W=160, seed=0):
    """A pair with the geometry of a real rig: R is box-blurred noise, g = 3 + 9 y / H + 2 sin(4 pi x / W), and the left image is
    the right one sampled linearly at x - g (clamped into the row), rounded to bytes.  Returns (left, right uint8 [H,W,3], g)."""
    rng = np.random.default_rng(seed)
    Rf = np.rint(box_blur(rng.uniform(0.0, 255.0, (H, W, 3)))).astype(np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    g = 3.0 + 9.0 * y / H + 2.0 * np.sin(4.0 * np.pi * x / W)
    t = np.clip(x - g, 0.0, W - 1.0)
    i0 = np.floor(t).astype(np.int64)
    i1 = np.minimum(i0 + 1, W - 1)
    a = (t - i0)[..., None]
    r = Rf.astype(np.float64)
    L = np.rint(np.take_along_axis(r, i0[..., None], axis=1) * (1.0 - a) + np.take_along_axis(r, i1[..., None], axis=1) * a)
    return L.astype(np.uint8), Rf, g.astype(F)


def one(disp, left, right, **kw):
    """photometric() of one [H,W] map and one image pair."""
    return R.photometric(np.asarray(disp, F)[None, None], left[None], right[None], **kw)


def mean_pe(p):
    return p.sums[0, 1] / float(1 << 20) / p.sums[0, 0]


# ---- (a) the restatement against float64 ----
def float64_terms(left, w):
    """l1 and dssim of the interior pixels, [H-2,W-2] float64, from the left image and the float32 warped colours w: window means
    and variances through sliding_window_view, not through chained sums."""
    x, y = left.astype(np.float64), w.astype(np.float64)
    win = lambda a: sliding_window_view(a, (3, 3), axis=(0, 1))     # noqa: E731
    mx, my = win(x).mean(axis=(-1, -2)), win(y).mean(axis=(-1, -2))
    vx, vy = (win(x) ** 2).mean(axis=(-1, -2)) - mx ** 2, (win(y) ** 2).mean(axis=(-1, -2)) - my ** 2
    cxy = (win(x) * win(y)).mean(axis=(-1, -2)) - mx * my
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    ssim = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx ** 2 + my ** 2 + c1) * (vx + vy + c2))
    ds = np.clip((1 - ssim) / 2, 0, 1).mean(axis=-1)
    l1 = np.abs(x - y).mean(axis=-1) / 255.0
    return l1[1:-1, 1:-1], ds


def pairs_for_float64():
    rng = np.random.default_rng(11)
    H, W = 20, 70
    near_white = [rng.integers(250, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)]
    full = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)]
    L, Rr, g = consistent_pair(H, W, 5)
    return {"noise 250..255": (*near_white, rng.uniform(0, 6, (H, W))), "full-range noise": (*full, rng.uniform(0, 6, (H, W))),
            "smooth pair": (L, Rr, g + 0.3)}


@pytest.mark.parametrize("name", ["noise 250..255", "full-range noise", "smooth pair"])
def test_restatement_agrees_with_float64(name):
    left, right, d = pairs_for_float64()[name]
    p = one(d, left, right)
    l1_64, ds_64 = float64_terms(left, p.w[0])
    dl1 = np.abs(p.l1[0, 1:-1, 1:-1].astype(np.float64) - l1_64).max()
    dds = np.abs(p.ds[0, 1:-1, 1:-1].astype(np.float64) - ds_64).max()
    print(f"{name}: max |ds32 - ds64| = {dds:.3g}, max |l1_32 - l1_64| = {dl1:.3g}")
    assert dds <= 2e-3 and dl1 <= 1e-6
    assert p.sums[0, 0] > 0


# ---- (b) exact properties ----
def test_identical_images_at_zero_disparity_score_exactly_zero():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (12, 40, 3)).astype(np.uint8)
    p = one(np.zeros((12, 40)), img, img)
    assert p.scored[0, 0, 1:-1, 1:-1].all() and p.sums[0, 0] == 10 * 38
    assert not p.pe.view(np.uint32)[p.scored[:, 0] == 1].any(), "pe must be +0.0 bit for bit"
    assert p.sums[0, 1:].tolist() == [0, 0, 0]
    assert np.array_equal(p.warped[0], img)


def test_a_rolled_image_scores_zero_at_its_shift_and_badly_one_pixel_off():
    rng = np.random.default_rng(2)
    left = rng.integers(0, 256, (16, 64, 3)).astype(np.uint8)
    right = np.roll(left, -7, axis=1)
    p = one(np.full((16, 64), 7.0), left, right)
    sc = p.scored[:, 0] == 1
    assert sc.sum() == 14 * (64 - 7 - 2) and not p.pe.view(np.uint32)[sc].any()
    off = one(np.full((16, 64), 8.0), left, right)
    print("mean pe one pixel off:", mean_pe(off))
    assert mean_pe(off) > 0.3


# ---- (c) ranking ----
def test_ranks_disparity_maps_on_a_consistent_pair():
    L, Rr, g = consistent_pair()
    means = [mean_pe(one(d, L, Rr)) for d in (g, g + F(0.5), g + F(1.0), g + F(3.0), np.zeros_like(g))]
    print("mean pe of g, g+0.5, g+1, g+3, 0:", means)
    assert means[0] < 0.01
    assert means[0] < means[1] < means[2] < means[3] < means[4]


# ---- (d) scoring rules ----
def test_mask_rvalid_and_small_images():
    L, Rr, g = consistent_pair(12, 48, 3)
    base = one(g, L, Rr)
    assert base.sums[0, 0] > 0
    none = one(g, L, Rr, mask=np.zeros((1, 1, 12, 48), np.uint8))
    assert not none.scored.any() and none.sums.tolist() == [[0, 0, 0, 0]] and not none.err.any()
    for code in (0, 2, 3):
        m = np.ones((1, 1, 12, 48), np.uint8)
        m[0, 0, 5, 20] = code
        p = one(g, L, Rr, mask=m)
        assert np.array_equal(p.scored != base.scored, (m != 1) & (base.scored == 1)), "only the pixel's own code counts"
    rv = np.ones((1, 1, 12, 48), np.uint8)
    col = 17
    rv[..., col] = 0
    p = one(g, L, Rr, rvalid=rv)
    t = np.arange(48, dtype=F) - g
    i0 = np.floor(t).astype(np.int64)
    taps = ((i0 == col) | (np.minimum(i0 + 1, 47) == col)) & (t >= 0)
    touched = np.zeros((12, 48), bool)
    touched[1:-1, 1:-1] = sliding_window_view(taps, (3, 3)).any(axis=(-1, -2))
    assert taps.any() and np.array_equal(p.scored[0, 0] == 1, (base.scored[0, 0] == 1) & ~touched)
    assert not p.warped[0][taps].any(), "an unusable pixel warps to 0"
    for H, W in ((2, 9), (9, 2), (1, 1)):
        img = np.full((H, W, 3), 9, np.uint8)
        p = one(np.zeros((H, W)), img, img)
        assert not p.scored.any() and p.sums.tolist() == [[0, 0, 0, 0]] and np.array_equal(p.warped[0], img)


def test_out_of_view_nan_and_infinite_disparities_are_not_warpable():
    img = np.full((5, 8, 3), 200, np.uint8)
    d = np.zeros((5, 8), F)
    d[2, 3], d[2, 4], d[2, 5], d[0, 0], d[4, 7] = np.nan, np.inf, -np.inf, 0.5, -0.5
    w, ok = R.warp(d[None, None], img[None])
    want = np.ones((5, 8), bool)
    want[2, 3:6] = False
    want[0, 0] = want[4, 7] = False                                  # t = -0.5 and t = W - 0.5
    assert np.array_equal(ok[0], want) and not w[0][~want].any()
    assert ok[0, 0, 1] and one(-0.0 * np.ones((5, 8)), img, img).sums[0, 0] == 3 * 6


# ---- (e) host side ----
def test_photometric_means():
    from lwsnet_amd.metrics import photometric_means
    s = np.zeros((3, 2, 4), np.int64)
    s[0, 0], s[0, 1] = (10, 5 << 20, 2 << 20, 1 << 20), (30, 5 << 20, 6 << 20, 3 << 20)
    s[1, 1] = (4, 1 << 19, 0, 1 << 20)
    m = photometric_means(s, pixels=100)
    assert m["scored"] == [40, 4, 0]
    assert m["pe"] == [0.25, 0.125, None] and m["l1"] == [0.2, 0.0, None] and m["dssim"] == [0.1, 0.25, None]
    assert m["density"] == [0.2, 0.02, 0.0]
    assert photometric_means(s)["density"] == [None] * 3
    json.dumps(m)
    torch = pytest.importorskip("torch")
    assert photometric_means(torch.from_numpy(s), 100) == m
    for bad in (s.astype(np.float64), s[0], s[:, :, :3]):
        with pytest.raises(ValueError):
            photometric_means(bad)
    with pytest.raises(ValueError):
        photometric_means(s, pixels=0)


def test_host_accumulator_pools_pixels_and_keeps_per_image_values():
    from lwsnet_amd.evaluate import Photometric
    from lwsnet_amd.metrics import photometric_means
    rng = np.random.default_rng(4)
    batches = [rng.integers(1, 1 << 24, (4, b, 4)).astype(np.int64) for b in (2, 1)]
    batches[0][2, 1] = 0                                            # stage 2 of the second image: nothing scored
    acc = Photometric(0.85)
    for s in batches:
        acc.update(s, 64 * 256)
    res = acc.result()
    allsums = np.concatenate(batches, axis=1)
    want = photometric_means(allsums, 64 * 256)
    assert res["alpha"] == 0.85 and all(res[k] == want[k] for k in want)
    assert res["per_image"]["pe"][1] == photometric_means(allsums[:, 1:2], 64 * 256)["pe"] and res["per_image"]["pe"][1][2] is None
    assert len(res["per_image"]["density"]) == 3
    assert acc.line(res).startswith("Photometric (alpha = 0.85): mean error Stage 0=")
    json.dumps(res)


@pytest.mark.parametrize("kw,msg", [(dict(workers=2), "sequential mode only"), (dict(photo_alpha=1.5), "photo_alpha"),
                                    (dict(photo_alpha=float("nan")), "photo_alpha")])
def test_evaluate_refuses_bad_photometric_arguments(kw, msg):
    from lwsnet_amd import evaluate
    with pytest.raises(ValueError, match=msg):
        evaluate.evaluate(None, [None], "kitti", photometric=True, **kw)


@pytest.mark.parametrize("cli", ["evaluate", "inference"])
@pytest.mark.parametrize("argv,msg", [(["--photometric", "--workers", "2"], "--photometric runs in the sequential mode only"),
                                      (["--photo_alpha", "0.5"], "--photometric\n"), (["--photometric", "--photo_alpha", "1.5"], "must be in [0, 1]"),
                                      (["--photometric", "--photo_alpha", "nan"], "must be in [0, 1]"), (["--save_photo"], "--photometric\n")])
def test_cli_rejects_bad_flags_before_any_model_work(cli, argv, msg, capsys):
    import importlib
    mod = importlib.import_module("lwsnet_amd." + cli)
    with pytest.raises(SystemExit) as e:
        mod.main(["--synthetic_weights", *argv])
    assert e.value.code != 0
    if cli == "evaluate" and "--save_photo" in argv:
        msg = "unrecognized arguments: --save_photo"                # no flag of the evaluate CLI at all
    assert msg in capsys.readouterr().err


@pytest.mark.parametrize("cli,argvs", [("evaluate", [[], ["--workers", "2"], ["--lr_check", "1", "--lr_fill"], ["--sparsification"]]),
                                       ("inference", [[], ["--workers", "2"], ["--occ_check", "1"], ["--save_conf", "--save_ply"]])])
def test_a_command_line_without_the_flags_parses_as_before(cli, argvs):
    import importlib

    from lwsnet_amd import postprocess as post
    mod = importlib.import_module("lwsnet_amd." + cli)
    save = cli == "inference"
    for argv in argvs:
        p = mod.build_parser()
        without = vars(p.parse_args(argv))
        assert not {"photometric", "photo_alpha", "save_photo"} & set(without)
        extra = ["--photometric", "--photo_alpha", "0.5"] + (["--save_photo"] if save else [])
        assert vars(p.parse_args(argv + extra)) == {**without, "photometric": True, "photo_alpha": 0.5, **({"save_photo": True} if save else {})}
        args = p.parse_args(argv)
        post.check_photometric_arguments(p, args, save=save)
        assert vars(args) == {**without, "photometric": False, "photo_alpha": 0.85, **({"save_photo": False} if save else {})}


def test_photo_to_u8():
    from lwsnet_amd.inference import photo_to_u8
    assert photo_to_u8(np.array([0.0, 0.4 / 255, 1.6 / 255, 1.0], F)).tolist() == [0, 0, 2, 255]


_CTYPES = {"int": ctypes.c_int, "float": ctypes.c_float}


def test_prototype_agrees_with_the_header():
    from lwsnet_amd import _lib, build
    txt = open(os.path.join(ROOT, "include", "lwsnet_hip.h")).read()
    m = re.search(r"\bint lws_photometric\((.*?)\);", txt, flags=re.S)
    assert m, "lws_photometric is not declared"
    want = []
    for arg in (" ".join(a.split()) for a in m.group(1).split(",")):
        if arg.endswith("[4]"):
            want.append(ctypes.c_void_p * 4)
        elif "*" in arg:
            want.append(ctypes.c_void_p)
        else:
            want.append(_CTYPES[arg.split()[0]])
    res, args = _lib.PROTOTYPES["lws_photometric"]
    assert res is ctypes.c_int and len(args) == len(want) == 15
    for i, (a, w) in enumerate(zip(args, want)):
        assert a is w or (a._length_ == 4 and w._length_ == 4 and a._type_ is w._type_), (i, a, w)
    assert "lws_photometric.hip" in build.SOURCES
    assert "#define LWS_ABI_VERSION 8" in txt


def test_entry_point_rejects_bad_arguments_on_the_host(hip_lib):
    """Every argument error returns LWS_ERR_INVALID before any GPU call: host memory stands in for the device buffers."""
    from lwsnet_amd import _lib
    B, H, W = 2, 5, 7
    n = B * H * W
    disp = [np.zeros(n, F) for _ in range(2)]
    left, right, rvalid = np.zeros(3 * n, np.uint8), np.zeros(3 * n, np.uint8), np.zeros(n, np.uint8)
    mask = [np.zeros(n, np.uint8) for _ in range(2)]
    err = [np.zeros(n, F) for _ in range(2)]
    scored = [np.zeros(n, np.uint8) for _ in range(2)]
    warped = [np.zeros(3 * n, np.uint8) for _ in range(2)]
    sums = np.zeros(2 * B * 4 + 4, np.int64)
    arr = ctypes.c_void_p * 4
    ptrs = lambda xs: arr(*[x.ctypes.data if x is not None else None for x in xs])      # noqa: E731

    def call(msg, **kw):
        a = dict(disp=ptrs(disp), nmaps=2, left=left.ctypes.data, right=right.ctypes.data, mask=ptrs(mask), rvalid=rvalid.ctypes.data, B=B, H=H,
                 W=W, alpha=0.85, err=ptrs(err), scored=ptrs(scored), warped=ptrs(warped), sums=sums.ctypes.data)
        a.update(kw)
        rc = hip_lib.lws_photometric(a["disp"], a["nmaps"], a["left"], a["right"], a["mask"], a["rvalid"], a["B"], a["H"], a["W"], a["alpha"],
                                     a["err"], a["scored"], a["warped"], a["sums"], None)
        assert rc == _lib.LWS_ERR_INVALID, (msg, rc)
        assert msg.encode() in hip_lib.lws_last_error(), (msg, hip_lib.lws_last_error())

    call("disp[0] is null", disp=arr())
    call("must not be null", left=None)
    call("must not be null", right=None)
    call("must not be null", sums=None)
    call("disp[1] is null", disp=ptrs([disp[0], None]))
    call("nmaps 0 outside 1..4", nmaps=0)
    call("nmaps 5 outside 1..4", nmaps=5)
    for alpha in (-0.01, 1.01, float("nan"), float("inf")):
        call("alpha must be in [0, 1]", alpha=alpha)
    call("bad shape", B=0)
    call("bad shape", H=0)
    call("bad shape", W=-1)
    call("must be < 2^31", B=1, H=65536, W=32768)
    call("exceeds 65535", B=32768)
    call("8-byte aligned", sums=sums.ctypes.data + 4)
    call("4-byte aligned", err=ptrs([err[0], err[1][1:].view(np.uint8)[1:]]))
    call("disp[0] and err[0] overlap", err=ptrs([disp[0], err[1]]))
    call("err[1] and err[0] overlap", err=ptrs([err[0], err[0]]))
    call("left and warped[1] overlap", warped=ptrs([warped[0], left]))
    call("right and warped[0] overlap", warped=ptrs([right, warped[1]]))
    call("mask[1] and scored[0] overlap", scored=ptrs([mask[1], scored[1]]))
    call("rvalid and scored[1] overlap", scored=ptrs([scored[0], rvalid]))
    both = np.zeros(2 * n, F)                                        # a partial overlap: the second half of err[0] is disp[1]
    call("disp[1] and err[0] overlap", err=ptrs([both[n // 2:n // 2 + n], err[1]]), disp=ptrs([disp[0], both[n:]]))
    call("sums and err[0] overlap", err=ptrs([sums[:n // 2 + 1].view(F), err[1]]))
