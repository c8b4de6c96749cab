"""The ground pipeline on the device: lws_vdisparity, lws_ground_fit, lws_ground_classify and lws_bev_grid bit for bit against the
numpy restatement (tests/ground_reference.py) at the smallest shapes that reach each path; views one element past a 16-byte
boundary, batch independence, poisoned guard bands, a captured graph, real maps of the model and the inference CLI's files."""
import ctypes
import os

import numpy as np
import pytest

import ground_reference as G
import guarded

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_geometry import KITTI15_CALIB, assert_bits, cam_rows, cu, misaligned  # noqa: E402

F = np.float32
INF = float("inf")
SPECIAL = np.array([np.nan, np.inf, -np.inf, -3.0, 0.0, 0.5, 1e30, 0.999], F)       # 0.5, 0.999: below min_disp = 1
# the parameters of the 96 x 160 road scenes
ROAD = dict(min_disp=1.0, max_depth=INF, sub=4, nbins=128, yh=(24, 72), qb=(42, 127), tol_bins=1, min_score=1, tol0=1.0, tol=1.0, iters=3,
            ground_tol=0.2, max_height=3.0, code_bits=1 << 2, x_min=-8.0, cell=0.2, grid=(80, 100))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, hip_lib):
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    return LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()


def road_cameras(B):
    from lwsnet_amd.geometry import Camera
    return [Camera(120.0 + 2 * b, 120.0 - b, 79.5 - 3 * b, 47.5 + b, 0.54 + 0.01 * b) for b in range(B)]


def roads(B, seed, plain=False):
    """B road scenes with boxes (pitch and roll differ per image), about 2.5 % special values planted and a code map with about 25 %
    non-1 codes.  plain: neither.  -> (disp [B,1,96,160], mask, cameras)."""
    rng = np.random.default_rng(seed)
    cams = road_cameras(B)
    d = np.concatenate([G.road_scene(pitch_deg=1.0 + 0.3 * b, roll_deg=0.7 * b, cam=cams[b].row())[0] for b in range(B)])
    mask = rng.choice(np.array([0, 1, 1, 1, 1, 1, 1, 2], np.uint8), size=d.shape)
    if plain:
        mask[:] = 1
    else:
        flat = d.reshape(-1)
        idx = rng.choice(flat.size, size=flat.size // 40, replace=False)
        flat[idx] = SPECIAL[np.arange(len(idx)) % len(SPECIAL)]
    return d, mask, cams


def reference(d, mask, rows, p):
    """The restatement of the four calls with the parameters p."""
    out = {"hist": G.vdisparity(d, mask, p["min_disp"], p["sub"], p["nbins"])}
    out["plane"], out["info"] = G.ground_fit(d, mask, out["hist"], p["min_disp"], p["sub"], *p["yh"], *p["qb"], p["tol_bins"], p["min_score"],
                                             p["tol0"], p["tol"], p["iters"])
    out["height"], out["codes"], out["counts"] = G.ground_classify(d, mask, rows, out["plane"], p["min_disp"], p["max_depth"], p["ground_tol"],
                                                                   p["max_height"])
    out["count"], out["hmax"] = G.bev_grid(d, rows, out["codes"], out["height"], p["min_disp"], p["max_depth"], p["code_bits"], p["x_min"],
                                           p["cell"], *p["grid"])
    return out


def run_ops(d, mask, cams, p, dev):
    from lwsnet_amd import ops
    return ops.ground(cu(d, dev), cams, None if mask is None else cu(mask, dev), p["min_disp"], p["max_depth"], sub=p["sub"], nbins=p["nbins"],
                      yh_range=p["yh"], qb_range=p["qb"], tol_bins=p["tol_bins"], min_score=p["min_score"], tol0=p["tol0"], tol=p["tol"],
                      iters=p["iters"], ground_tol=p["ground_tol"], max_height=p["max_height"], code_bits=p["code_bits"], x_min=p["x_min"],
                      cell=p["cell"], grid=p["grid"])


NAMES = (("hist", "hist"), ("plane", "plane"), ("info", "info"), ("height", "height"), ("codes", "codes"), ("counts", "counts"),
         ("bev_count", "count"), ("bev_hmax", "hmax"))


def check_result(res, want, what):
    for field, key in NAMES:
        if key in want:
            assert_bits(getattr(res, field), want[key], f"{what} {key}")


# ---- lws_vdisparity ----
def hist_maps(B, H, W, sub, nbins, seed):
    """Disparities from 0 to a fifth past the last bin, the specials planted, row 0 of every image in one bin, and a code map."""
    rng = np.random.default_rng(seed)
    top = nbins / sub
    d = (rng.random((B, 1, H, W)) * 1.2 * top).astype(F)
    flat = d.reshape(-1)
    idx = rng.choice(flat.size, size=max(1, flat.size // 20), replace=False)
    flat[idx] = np.concatenate([SPECIAL, [F(top), np.nextafter(F(top), F(0))]]).astype(F)[np.arange(len(idx)) % (len(SPECIAL) + 2)]
    d[:, 0, 0, :] = F(min(1.3, 0.9 * top)) if top > 1.0 else F(0.5 * top)
    mask = rng.choice(np.array([0, 1, 1, 1, 2, 3], np.uint8), size=d.shape)
    return d, mask


@pytest.mark.parametrize("B,H,W,sub,nbins,min_disp", [
    (1, 1, 1, 4, 1, 0.125),                 # one pixel, one bin
    (2, 300, 5, 4, 70, 1.0),                # a partial quad; rows not 16-byte aligned
    (1, 3, 1030, 16, 4096, 1.0),            # more than one 256-quad chunk per row; the largest histogram
    (3, 5, 1030, 1, 70, 1.0),
    (2, 1, 5, 3, 1, 0.01)])
def test_vdisparity_bitexact(dev, hip_lib, B, H, W, sub, nbins, min_disp):
    from lwsnet_amd import ops
    d, mask = hist_maps(B, H, W, sub, nbins, 3 * H + W + nbins)
    for m in (None, mask):
        want = G.vdisparity(d, m, min_disp, sub, nbins)
        got = ops.vdisparity(cu(d, dev), None if m is None else cu(m, dev), min_disp, sub, nbins)
        assert_bits(got, want, f"B={B} {H}x{W} sub={sub} nbins={nbins} mask={m is not None}")
        # a view one element past a 16-byte boundary
        got = ops.vdisparity(misaligned(d, dev), None if m is None else misaligned(m, dev), min_disp, sub, nbins)
        assert_bits(got, want, f"misaligned B={B} {H}x{W} sub={sub} nbins={nbins} mask={m is not None}")
    if W > 1 and nbins > 1:
        row0 = G.vdisparity(d, None, min_disp, sub, nbins)[0, 0]
        assert row0.max() == W and (row0 > 0).sum() == 1, "row 0 should sit in one bin"
        c, _ = G.counted(d, mask, min_disp, sub, nbins)
        assert 0 < c.sum() < c.size


# ---- the C ABI with the caller's buffers ----
def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_hist(lib, dev, b, shape, p):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_vdisparity(P(b["disp"]), P(b.get("mask")), *shape, p["min_disp"], p["sub"], p["nbins"], P(b["hist"]), stream()),
                   "lws_vdisparity")


def raw_fit(lib, dev, b, shape, p):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_ground_fit(P(b["disp"]), P(b.get("mask")), P(b["hist"]), *shape, p["min_disp"], p["sub"], p["nbins"], *p["yh"], *p["qb"],
                                      p["tol_bins"], p["min_score"], p["tol0"], p["tol"], p["iters"], P(b["work"]), P(b["plane"]), P(b["info"]),
                                      stream()), "lws_ground_fit")


def raw_classify(lib, dev, b, shape, p):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_ground_classify(P(b["disp"]), P(b.get("mask")), P(b["cam"]), P(b["plane"]), *shape, p["min_disp"], p["max_depth"],
                                           p["ground_tol"], p["max_height"], P(b.get("height")), P(b.get("codes")), P(b.get("counts")), stream()),
                   "lws_ground_classify")


def raw_bev(lib, dev, b, shape, p):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_bev_grid(P(b["disp"]), P(b["cam"]), P(b["codes"]), P(b.get("height")), *shape, p["min_disp"], p["max_depth"],
                                    p["code_bits"], p["x_min"], p["cell"], *p["grid"], P(b.get("count")), P(b.get("hmax")), stream()),
                   "lws_bev_grid")


def fit_buffers(lib, dev, B, H, nbins):
    return dict(work=torch.empty((int(lib.lws_ground_workspace(B, H, nbins)),), dtype=torch.uint8, device=dev),
                plane=torch.empty((B, 4), dtype=torch.float32, device=dev), info=torch.empty((B, 8), dtype=torch.int32, device=dev))


# ---- lws_ground_fit: the vote ----
def vote(lib, dev, hist, p, W=4):
    """lws_ground_fit on a given histogram and a map without a valid pixel, against the restatement: (plane, info) of the device."""
    B, H, nbins = hist.shape
    d = np.zeros((B, 1, H, W), F)
    q = {**ROAD, **p, "nbins": nbins}
    b = dict(disp=cu(d, dev), hist=cu(hist, dev), **fit_buffers(lib, dev, B, H, nbins))
    raw_fit(lib, dev, b, (B, H, W), q)
    plane, info = G.ground_fit(d, None, hist, q["min_disp"], q["sub"], *q["yh"], *q["qb"], q["tol_bins"], q["min_score"], q["tol0"], q["tol"],
                               q["iters"])
    assert_bits(b["plane"], plane, f"vote {p} plane")
    assert_bits(b["info"], info, f"vote {p} info")
    return plane, info


def test_hough_tie_rule_and_edges(dev, hip_lib):
    hist = np.zeros((1, 6, 8), np.uint32)
    hist[0, 5, 3] = hist[0, 5, 5] = 7                       # two bottom bins with equal support: every yh scores 7 with either
    _, info = vote(hip_lib, dev, hist, dict(yh=(0, 3), qb=(1, 7), tol_bins=0, min_score=0))
    assert info[0, :5].tolist() == [G.DEGENERATE, 0, 3, 7, 0]                   # the smaller qB, then the smaller yh; no pixel to fit
    _, info = vote(hip_lib, dev, hist, dict(yh=(2, 3), qb=(4, 7), tol_bins=0, min_score=0))
    assert info[0, 1:4].tolist() == [2, 5, 7]
    _, info = vote(hip_lib, dev, hist, dict(yh=(-4, -4), qb=(1, 7), tol_bins=1, min_score=0))
    assert info[0, 1:4].tolist() == [-4, 4, 14]                                 # yh < 0; one bin of tolerance around 4 reaches both
    _, info = vote(hip_lib, dev, hist, dict(yh=(4, 4), qb=(1, 7), tol_bins=0, min_score=0))   # yh = H - 2: the bottom row alone
    assert info[0, 1:4].tolist() == [4, 3, 7]
    rng = np.random.default_rng(5)
    hist = rng.integers(0, 50, (2, 9, 8)).astype(np.uint32)                     # windows clipped at bin 0 and at nbins - 1
    vote(hip_lib, dev, hist, dict(yh=(-3, 7), qb=(1, 7), tol_bins=8, min_score=0))
    vote(hip_lib, dev, hist, dict(yh=(-65536, -65530), qb=(6, 7), tol_bins=2, min_score=0))
    # no ground: min_score above the best, and an empty histogram
    plane, info = vote(hip_lib, dev, hist, dict(yh=(0, 7), qb=(1, 7), tol_bins=1, min_score=10 ** 6))
    assert info[:, 0].tolist() == [G.NO_GROUND] * 2 and np.isnan(plane).all() and (info[:, 3] > 0).all()
    plane, info = vote(hip_lib, dev, np.zeros((1, 9, 8), np.uint32), dict(yh=(0, 7), qb=(2, 7), tol_bins=1, min_score=1))
    assert info[0, :5].tolist() == [G.NO_GROUND, 0, 2, 0, 0] and np.isnan(plane).all()


def test_hough_ragged_candidate_count(dev, hip_lib):
    """300 bottom bins: two workgroups of candidates per horizon row, the second with 44 of 256 threads at work; 3600 candidates."""
    rng = np.random.default_rng(9)
    hist = rng.integers(0, 9, (2, 20, 400)).astype(np.uint32)
    hist[0, np.arange(20), (np.arange(20) * 330) // 19] += 40                   # a line to find
    _, info = vote(hip_lib, dev, hist, dict(yh=(-2, 9), qb=(50, 349), tol_bins=1, min_score=0))
    assert 320 <= info[0, 2] <= 340
    vote(hip_lib, dev, hist, dict(yh=(-2, 9), qb=(1, 399), tol_bins=3, min_score=0))


# ---- lws_ground_fit: the passes ----
@pytest.mark.parametrize("iters", [0, 3])
def test_fit_of_road_scenes_bitexact(dev, hip_lib, iters):
    B = 2
    d, mask, cams = roads(B, 4)
    p = {**ROAD, "iters": iters}
    for m in (None, mask):
        want = reference(d, m, cam_rows(cams), p)
        assert want["info"][:, 0].tolist() == [G.OK] * B and (want["info"][:, 4] > 3000).all(), want["info"]
        check_result(run_ops(d, m, cams, p, dev), want, f"roads iters={iters} mask={m is not None}")


def test_fit_degenerate_cases(dev, hip_lib):
    from lwsnet_amd import ops
    # fewer than 3 inliers: two valid pixels on the voted line
    d = np.zeros((1, 1, 8, 16), F)
    d[0, 0, 7, 3] = d[0, 0, 7, 9] = 8.1
    hist = ops.vdisparity(cu(d, dev), None, 1.0, 4, 64)
    assert_bits(hist, G.vdisparity(d, None, 1.0, 4, 64), "two pixels hist")
    want = G.ground_fit(d, None, hist.cpu().numpy(), 1.0, 4, 0, 6, 1, 63, 1, 1, 1.0, 1.0, 3)
    got = ops.ground_fit(cu(d, dev), hist, None, 1.0, 4, (0, 6), (1, 63), 1, 1, 1.0, 1.0, 3)
    assert_bits(got[0], want[0], "two pixels plane")
    assert_bits(got[1], want[1], "two pixels info")
    assert want[1][0, :5].tolist() == [G.DEGENERATE, 0, 31, 2, 2] and np.isnan(want[0]).all()     # bins 31..33 reach the two: the smaller qB
    # W = 1: every pixel on one column, det = 0
    d = (2.0 + 1.5 * np.arange(12, dtype=F)).reshape(1, 1, 12, 1)
    hist = ops.vdisparity(cu(d, dev), None, 1.0, 4, 128)
    want = G.ground_fit(d, None, hist.cpu().numpy(), 1.0, 4, -4, 4, 40, 100, 1, 1, 2.0, 1.0, 2)
    got = ops.ground_fit(cu(d, dev), hist, None, 1.0, 4, (-4, 4), (40, 100), 1, 1, 2.0, 1.0, 2)
    assert_bits(got[0], want[0], "column plane")
    assert_bits(got[1], want[1], "column info")
    assert want[1][0, 0] == G.DEGENERATE and want[1][0, 4] >= 3 and np.isnan(want[0]).all()


def test_fit_sums_past_32_bits(dev, hip_lib):
    """8 x 1030 near 80 px: SxQ of the inliers passes 2^32, so a sum kept in 32 bits anywhere would show."""
    H, W = 8, 1030
    y, x = np.mgrid[0:H, 0:W]
    d = (80.0 + 0.0007 * x + 0.05 * (y - 7)).astype(F)[None, None]
    p = {**ROAD, "nbins": 400, "yh": (-65536, -65533), "qb": (300, 340), "iters": 3}
    want = reference(d, None, cam_rows(road_cameras(1)), p)
    assert want["info"][0, 0] == G.OK and want["info"][0, 4] > 8000
    cnt, _ = G.counted(d, None, 1.0, 4, 400)
    sums = G.fit_sums(G.u16(d[0, 0]), cnt[0, 0], tuple(256.0 * float(v) for v in want["plane"][0, :3]), 1.0)
    assert sums[7] > 2 ** 32, sums
    check_result(run_ops(d, None, road_cameras(1), p, dev), want, "8x1030")


# ---- lws_ground_classify ----
def test_classify_outputs_alone_nan_plane_and_misaligned(dev, hip_lib):
    from lwsnet_amd import ops
    B = 2
    d, mask, cams = roads(B, 6)
    rows = cam_rows(cams)
    want = reference(d, mask, rows, ROAD)
    assert all((want["codes"] == c).any() for c in (0, 1, 2)), "the scene should hold invalid, ground and obstacle pixels"
    dm, mm, plane = cu(d, dev), cu(mask, dev), cu(want["plane"], dev)
    args = (1.0, INF, 0.2, 3.0)
    for h, c, n in ((True, False, False), (False, True, False), (True, True, True), (False, True, True)):
        got = ops.ground_classify(dm, cams, plane, mm, *args, height=h, codes=c, counts=n)
        assert [g is not None for g in got] == [h, c, n]
        for g, key in zip(got, ("height", "codes", "counts")):
            if g is not None:
                assert_bits(g, want[key], f"classify {key} of {(h, c, n)}")
    # a plane that puts pixels below the road and overhead
    tilted = want["plane"].copy()
    tilted[:, 0] += F(0.02)
    tilted[:, 2] -= F(1.5)
    w2 = G.ground_classify(d, mask, rows, tilted, 1.0, 40.0, 0.05, 0.4)
    assert all((w2[1] == c).any() for c in (0, 1, 2, 3, 4)), np.unique(w2[1])
    got = ops.ground_classify(dm, cams, cu(tilted, dev), mm, 1.0, 40.0, 0.05, 0.4)
    for g, w, key in zip(got, w2, ("height", "codes", "counts")):
        assert_bits(g, w, f"tilted {key}")
    # a NaN plane (image 0) and an infinite one (image 1): code 5 wherever the pixel is valid
    bad = np.array([[np.nan] * 4, [0.0, np.inf, 1.0, 0.0]], F)
    w3 = G.ground_classify(d, mask, rows, bad, *args)
    assert set(np.unique(w3[1])) == {0, 5} and (w3[0] == 0).all()
    got = ops.ground_classify(dm, cams, cu(bad, dev), mm, *args)
    for g, w, key in zip(got, w3, ("height", "codes", "counts")):
        assert_bits(g, w, f"no plane {key}")
    # every map one element past a 16-byte boundary, the outputs too
    b = dict(disp=misaligned(d, dev), mask=misaligned(mask, dev), cam=misaligned(rows, dev), plane=misaligned(want["plane"], dev),
             height=misaligned(np.zeros(d.shape, F), dev), codes=misaligned(np.zeros(d.shape, np.uint8), dev),
             counts=torch.empty((B, 6), dtype=torch.int64, device=dev))
    raw_classify(hip_lib, dev, b, d.shape[:1] + d.shape[2:], ROAD)
    for key in ("height", "codes", "counts"):
        assert_bits(b[key], want[key], f"misaligned classify {key}")
    b.update(count=misaligned(np.zeros((B, 100, 80), np.uint32), dev), hmax=misaligned(np.zeros((B, 100, 80), F), dev))
    raw_bev(hip_lib, dev, b, d.shape[:1] + d.shape[2:], ROAD)
    assert_bits(b["count"], want["count"], "misaligned bev count")
    assert_bits(b["hmax"], want["hmax"], "misaligned bev hmax")


# ---- lws_bev_grid ----
def test_bev_grid_cases(dev, hip_lib):
    from lwsnet_amd import ops
    B = 2
    d, mask, cams = roads(B, 7)
    rows = cam_rows(cams)
    base = reference(d, mask, rows, ROAD)
    dm, codes, height = cu(d, dev), cu(base["codes"], dev), cu(base["height"], dev)
    cases = [dict(grid=(1, 1), x_min=-50.0, cell=100.0),                        # one cell holds every obstacle pixel
             dict(grid=(2, 3), x_min=-1.0, cell=3.0),                           # points outside to the left and beyond, many per cell
             dict(grid=(7, 20), x_min=1.0, cell=0.3, code_bits=(1 << 2) | (1 << 3)),    # ... to the right and nearer as well
             dict(code_bits=1 << 3),                                            # selects nothing: the scene has no overhead pixel
             dict(code_bits=0)]
    for c in cases:
        p = {**ROAD, **c}
        count, hmax = G.bev_grid(d, rows, base["codes"], base["height"], 1.0, INF, p["code_bits"], p["x_min"], p["cell"], *p["grid"])
        got = ops.bev_grid(dm, cams, codes, height, 1.0, INF, p["code_bits"], p["x_min"], p["cell"], p["grid"])
        assert_bits(got[0], count, f"bev {c} count")
        assert_bits(got[1], hmax, f"bev {c} hmax")
        n_obstacles = int(base["counts"][:, 2].sum())
        if c.get("grid") == (1, 1):
            top = [base["height"][i][base["codes"][i] == G.OBSTACLE].max() for i in range(B)]
            assert count.sum() == n_obstacles and count.min() > 100 and hmax.reshape(-1).tolist() == top
        elif "grid" in c:
            assert 0 < count.sum() < n_obstacles and count.max() > 1
        else:
            assert count.sum() == 0 and (hmax.view(np.uint32) == 0).all()
    # every code counted, no maximum: the count alone
    count, _ = G.bev_grid(d, rows, base["codes"], base["height"], 1.0, INF, 63, -8.0, 0.5, 32, 40)
    got = ops.bev_grid(dm, cams, codes, None, 1.0, INF, 63, -8.0, 0.5, (32, 40), hmax=False)
    assert got[1] is None
    assert_bits(got[0], count, "bev of every code")
    got = ops.bev_grid(dm, cams, codes, height, 1.0, INF, 4, -8.0, 0.5, (32, 40), count=False)
    assert got[0] is None
    assert_bits(got[1], G.bev_grid(d, rows, base["codes"], base["height"], 1.0, INF, 4, -8.0, 0.5, 32, 40)[1], "bev hmax alone")


# ---- across the four ----
def test_ground_is_batch_independent(dev, hip_lib):
    B = 3
    d, mask, cams = roads(B, 11)
    batch = run_ops(d, mask, cams, ROAD, dev)
    assert batch.info[:, 0].cpu().tolist() == [0, 0, 0]

    def same(got, b, rb, what):
        for field, _ in NAMES:
            g, r = getattr(got, field)[b].cpu().numpy(), getattr(batch, field)[rb].cpu().numpy()
            assert np.array_equal(guarded.as_bits(g), guarded.as_bits(r)), f"{what} {field}"

    for b in range(B):
        same(run_ops(d[b:b + 1], mask[b:b + 1], [cams[b]], ROAD, dev), 0, b, f"image {b} alone")
    d2, m2, _ = roads(B, 12)
    d2[0], m2[0] = d[2], mask[2]
    same(run_ops(d2, m2, [cams[2]] + cams[1:], ROAD, dev), 0, 2, "image 2 moved to the front")


WORDS = pytest.mark.parametrize("word", guarded.FLOAT_WORDS, ids=guarded.word_id)


def all_buffers(dev, lib, B, H, W, p, d, mask, rows, guard=None):
    """The buffers of the four calls: in a Guard (inputs placed, outputs and workspace poisoned) or plain device tensors."""
    Gx, Gz = p["grid"]
    nbytes = int(lib.lws_ground_workspace(B, H, p["nbins"]))
    assert nbytes > 0
    if guard is not None:
        g = guard
        return dict(disp=g.place(d, name="disp"), mask=None if mask is None else g.place(mask, word=guarded.MASK_WORD, name="mask"),
                    cam=g.place(rows, name="cam"), hist=g.empty((B, H, p["nbins"]), np.uint32, name="hist"),
                    work=g.empty((nbytes,), np.uint8, align16=True, word=g.word, name="workspace"), plane=g.empty((B, 4), F, name="plane"),
                    info=g.empty((B, 8), np.int32, name="info"), height=g.empty((B, 1, H, W), F, name="height"),
                    codes=g.empty((B, 1, H, W), np.uint8, name="codes"), counts=g.empty((B, 6), np.int64, align16=True, name="counts"),
                    count=g.empty((B, Gz, Gx), np.uint32, name="count"), hmax=g.empty((B, Gz, Gx), F, name="hmax"))
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)                # noqa: E731
    return dict(disp=cu(d, dev), mask=None if mask is None else cu(mask, dev), cam=cu(rows, dev), hist=e((B, H, p["nbins"]), torch.uint32),
                work=e((nbytes,), torch.uint8), plane=e((B, 4), torch.float32), info=e((B, 8), torch.int32), height=e((B, 1, H, W), torch.float32),
                codes=e((B, 1, H, W), torch.uint8), counts=e((B, 6), torch.int64), count=e((B, Gz, Gx), torch.uint32),
                hmax=e((B, Gz, Gx), torch.float32))


def run_raw(lib, dev, b, shape, p):
    raw_hist(lib, dev, b, shape, p)
    raw_fit(lib, dev, b, shape, p)
    raw_classify(lib, dev, b, shape, p)
    raw_bev(lib, dev, b, shape, p)


RAW_KEYS = ("hist", "plane", "info", "height", "codes", "counts", "count", "hmax")


@WORDS
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "plain"])
def test_memory_contract(dev, hip_lib, with_mask, word):
    """Inputs and outputs between poisoned flanks, every output and the workspace poisoned inside: nothing outside the outputs
    changes and every element the header promises is written -- the histogram's zeros and the grids' empty cells included."""
    B = 2
    d, mask, cams = roads(B, 8)
    H, W = d.shape[2:]
    rows = cam_rows(cams)
    m = mask if with_mask else None
    want = reference(d, m, rows, ROAD)
    g = guarded.Guard(dev, word, skew=1)
    b = all_buffers(dev, hip_lib, B, H, W, ROAD, d, m, rows, guard=g)
    run_raw(hip_lib, dev, b, (B, H, W), ROAD)
    for key in RAW_KEYS:
        guarded.assert_bits(b[key], want[key], f"guarded {key}")
    g.check()


def test_graph_capture_replays_the_four_calls(dev, hip_lib):
    B = 2
    first, second = roads(B, 21), roads(B, 22, plain=True)
    H, W = first[0].shape[2:]
    rows = cam_rows(first[2])
    b = all_buffers(dev, hip_lib, B, H, W, ROAD, first[0], first[1], rows)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                           # one stream: the capture stream
        run_raw(hip_lib, dev, b, (B, H, W), ROAD)
    for d_np, m_np, _ in (first, second):
        b["disp"].copy_(cu(d_np, dev))
        b["mask"].copy_(cu(m_np, dev))
        graph.replay()
        torch.cuda.synchronize(dev)
        want = reference(d_np, m_np, rows, ROAD)
        for key in RAW_KEYS:
            assert_bits(b[key], want[key], f"replay {key}")


def test_ground_of_model_maps(dev, model):
    """Real maps: the seeded model at 64 x 256 behind forward_occ, each stage with its code map -- bit-equal whatever the status."""
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import Camera
    from lwsnet_amd.synth import make_pair
    H, W = 64, 256
    left, right = (a[None] for a in make_pair(H, W, 0)[:2])
    cams = [Camera(721.5, 721.5, 127.5, 31.5, 0.54)]
    rows = cam_rows(cams)
    res = model.forward_occ(left, right, tau=1.0, fill=False)
    p = {**ROAD, "nbins": 768, "yh": (H // 4, 3 * H // 4), "qb": (256, 767), "min_score": 0, "x_min": -20.0, "grid": (200, 300)}
    for s in range(4):
        d, m = res.disp[s].numpy(), res.mask[s].cpu().numpy()
        want = reference(d, m, rows, p)
        got = ops.ground(res.disp[s], cams, res.mask[s])    # the defaults are these parameters
        check_result(got, want, f"forward_occ stage {s + 1}")
        print(f"forward_occ stage {s + 1}: info = {want['info'][0, :5].tolist()}, counts = {want['counts'][0].tolist()}")


def test_inference_cli_ground_files(dev, model, tmp_path):
    from PIL import Image
    from lwsnet_amd import imageio as io
    from lwsnet_amd import inference, ops, synth
    from lwsnet_amd.geometry import Camera
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, 1)
    calib = tmp_path / "000000.txt"
    calib.write_text(KITTI15_CALIB.format(fx=721.5377, cx=609.5593, cy=172.854, t3=44.85728 - 0.54 * 721.5377))
    out = tmp_path / "out"
    written = inference.main(["--img_path", root + "/", "--synthetic_weights", "--calib", str(calib), "--occ_check", "1", "--save_path",
                              str(out), "--save_ground", "--ground_tol", "0.3", "--max_height", "2.5"])
    stem = "000000_10"
    assert sorted(os.listdir(out)) == sorted(stem + s for s in (".png", "_occ.png", "_ground.png", "_bev.png"))
    assert len(written) == 4
    full = io.load_rgb(os.path.join(root, "image_2", stem + ".png"))
    left = io.crop_bottom_right(full)
    l_in = io.to_input(left)[None]
    r_in = io.to_input(io.crop_bottom_right(io.load_rgb(os.path.join(root, "image_3", stem + ".png"))))[None]
    cam = Camera.from_kitti(str(calib)).crop_bottom_right(*full.shape[:2])
    res = model.forward_occ(l_in, r_in, tau=1.0, fill=False)
    g = ops.ground(res.disp[3], cam, res.mask[3], ground_tol=0.3, max_height=2.5)
    assert np.array_equal(np.asarray(Image.open(out / (stem + "_ground.png"))), inference.ground_to_rgb(g.codes[0, 0].cpu().numpy(), left))
    bev = np.asarray(Image.open(out / (stem + "_bev.png")))
    assert bev.shape == (300, 200) and np.array_equal(bev, inference.bev_to_u8(g.bev_hmax[0].cpu().numpy(), 2.5))
