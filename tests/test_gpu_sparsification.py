"""lws_sparsification on the device against its numpy restatement (tests/sparsification_reference.py), bit for bit: random and
planted inputs, the hot bin and the widths of the sums, determinism and batch independence, guard bands, hipGraph capture, the
argument errors, and `python -m lwsnet_amd.evaluate --sparsification` end to end on a generated KITTI tree."""
import ctypes

import numpy as np
import pytest

import guarded as G
import sparsification_reference as REF
from test_gpu_evaluate import _cli, make

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WORDS = pytest.mark.parametrize("word", G.FLOAT_WORDS, ids=G.word_id)
KINDS = pytest.mark.parametrize("kind", [0, 1], ids=["sigma", "conf"])
MODES = pytest.mark.parametrize("mode", [0, 1], ids=["kitti", "epe"])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def make_inputs(B, Hg, W, off, kind, seed):
    """preds and gt as make() of test_gpu_evaluate.py builds them (gt in [-15, 215)); unc log-uniform over 2^-30..2^10 for sigma,
    uniform over [-0.1, 1.1] for conf; the padded rows of every map hold 1000 and must never be read."""
    preds, gt = make(B, Hg, W, off, seed)
    rng = np.random.default_rng(seed + 77)
    unc = []
    for s in range(4):
        u = np.full((B, 1, Hg + off, W), 1000.0, np.float32)
        if kind == 0:
            u[:, 0, off:] = np.exp2(rng.uniform(-30.0, 10.0, (B, Hg, W))).astype(np.float32)
        else:
            u[:, 0, off:] = rng.uniform(-0.1, 1.1, (B, Hg, W)).astype(np.float32)
        unc.append(u)
    return preds, unc, gt


def run(dev, preds, unc, gt, off, maxdisp, mode, kind):
    from lwsnet_amd import ops
    h = ops.sparsification([torch.from_numpy(p).to(dev) for p in preds], [torch.from_numpy(u).to(dev) for u in unc],
                           torch.from_numpy(gt).to(dev), off, maxdisp, mode, kind)
    assert h.dtype == torch.int64 and tuple(h.shape) == (len(preds), gt.shape[0], 2, 1026, 3)
    return h.cpu().numpy()


def assert_hist(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


@pytest.mark.parametrize("B,Hg,W,off", [(3, 5, 7, 4), (2, 37, 61, 0), (2, 37, 61, 3), (1, 64, 300, 0)])
@pytest.mark.parametrize("nmaps", [1, 4])
@MODES
@KINDS
def test_histograms_match_numpy_float32(dev, B, Hg, W, off, nmaps, mode, kind):
    preds, unc, gt = make_inputs(B, Hg, W, off, kind, seed=B * 1000 + Hg + W + off)
    preds, unc = preds[:nmaps], unc[:nmaps]
    want = REF.histogram(preds, unc, gt, off, 192, mode, kind)
    got = run(dev, preds, unc, gt, off, 192, mode, "sigma" if kind == 0 else "conf")
    assert_hist(got, want)
    assert want[:, :, 0, :, 0].sum() > 0 and (want[:, :, 0, 1:1025, 0] > 0).sum() > 20      # the ranking spreads over many bins


def planted(kind, seed=7):
    """B, Hg, W, off = 2, 37, 61, 4 with every bin rule's edge in unc, NaN / inf predictions and the ground-truth edge values."""
    B, Hg, W, off = 2, 37, 61, 4
    preds, unc, gt = make_inputs(B, Hg, W, off, kind, seed)
    lo = np.float32(2.0 ** -24)
    edge = [np.nan, np.inf, -np.inf, -0.0, 0.0, lo, np.nextafter(lo, np.float32(0)), np.nextafter(lo, np.float32(1)),
            np.float32(255.99998), 256.0, 1.5, -2.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), np.float32(1) - lo, 1e30]
    cells = [(50.0, 53.5, u) for u in edge]                                     # (gt, pred, unc): a valid pixel per edge value
    cells += [(30.0, np.nan, 0.25), (30.0, np.inf, 0.25), (30.0, -np.inf, 0.25), (30.0, 70000.0, 0.25), (30.0, 3.0e38, 0.25),
              (80.0, 84.0, 0.25), (80.0, np.nextafter(np.float32(84), np.float32(100)), 0.25),   # e / g == 0.05f, and the next float up
              (30.0, 30.0, 0.25), (30.0, np.float32(30) + np.float32(2.0 ** -18), 0.25)]        # e == 0 and a tiny e
    cells += [(g, 20.0, 0.25) for g in (np.nan, np.inf, -np.inf, 0.0, -0.0, 192.0, 49151 / 256, -3.0)]
    for k, (g, p, u) in enumerate(cells):
        for b in range(B):
            y, x = 1 + k + b, (5 + 7 * k) % W
            gt[b, y, x] = g
            for s in range(4):
                preds[s][b, 0, off + y, x] = p
                unc[s][b, 0, off + y, x] = u
    return preds, unc, gt, off


@MODES
@KINDS
def test_planted_edge_values(dev, mode, kind):
    preds, unc, gt, off = planted(kind)
    want = REF.histogram(preds, unc, gt, off, 192, mode, kind)
    assert_hist(run(dev, preds, unc, gt, off, 192, mode, kind), want)
    assert want[0, 0, 0, 0, 0] > 0 and want[0, 0, 0, 1025, 0] > 0 and want[0, 0, 1, 0, 0] > 0 and want[0, 0, 1, 1025, 0] >= 5
    assert want[0, 0, 1, 1025, 2] >= 3 * 2 ** 26                                # the NaN and inf predictions count as 65536 px


@MODES
@KINDS
def test_bin_sums_equal_stage_metrics(dev, mode, kind):
    from lwsnet_amd import ops
    preds, unc, gt, off = planted(kind)
    counts, _ = ops.stage_metrics([torch.from_numpy(p).to(dev) for p in preds], torch.from_numpy(gt).to(dev), off, 192, mode)
    got = run(dev, preds, unc, gt, off, 192, mode, kind)
    for r in range(2):
        assert np.array_equal(got[:, :, r, :, :2].sum(axis=2), counts.cpu().numpy()), r
    assert np.array_equal(got[:, :, 0, :, 2].sum(axis=2), got[:, :, 1, :, 2].sum(axis=2))      # one q sum, binned twice


def test_hot_bin_and_the_widths_of_the_sums(dev):
    """Every pixel of one 300 x 300 image in one bin with the largest q: lost LDS atomics, 16-bit counts and 32-bit sums show."""
    n = 300
    gt = np.full((1, n, n), 50.0, np.float32)
    preds = [np.full((1, 1, n, n), np.nan, np.float32)]
    unc = [np.zeros((1, 1, n, n), np.float32)]
    got = run(dev, preds, unc, gt, 0, 192, 0, 0)
    want = np.zeros((1, 1, 2, 1026, 3), np.int64)
    want[0, 0, 0, 0] = want[0, 0, 1, 1025] = (n * n, 0, n * n * 2 ** 26)
    assert_hist(got, want)
    assert_hist(got, REF.histogram(preds, unc, gt, 0, 192, 0, 0))
    # a few lanes per wave elsewhere: the wave-level add and the lanes' own adds side by side, bad pixels in both
    preds[0][0, 0, :, ::9] = 70.0
    unc[0][0, 0, :, ::5] = 3.0
    assert_hist(run(dev, preds, unc, gt, 0, 192, 0, 0), REF.histogram(preds, unc, gt, 0, 192, 0, 0))


@pytest.mark.parametrize("Hg,W,off", [(37, 61, 4), (64, 300, 0)])
def test_deterministic_and_batch_independent(dev, Hg, W, off):
    preds, unc, gt = make_inputs(3, Hg, W, off, 1, seed=11)
    preds[1][2, 0, off + 1, 2] = np.nan
    one = run(dev, [p[2:3] for p in preds], [u[2:3] for u in unc], gt[2:3], off, 192, 1, 1)
    three = run(dev, preds, unc, gt, off, 192, 1, 1)
    again = run(dev, preds, unc, gt, off, 192, 1, 1)
    assert one.tobytes() == three[:, 2:3].tobytes()
    assert three.tobytes() == again.tobytes()


@WORDS
@KINDS
def test_guard_bands(dev, hip_lib, kind, word):
    """Skewed, element-aligned pointers and a poisoned hist: every element is written, nothing outside is touched or read."""
    B, Hg, W, off, mode = 2, 37, 61, 3, 0
    preds_np, unc_np, gt_np = make_inputs(B, Hg, W, off, kind, seed=21)
    want = REF.histogram(preds_np, unc_np, gt_np, off, 192, mode, kind)
    g = G.Guard(dev, word, skew=1)
    preds = [g.place(p, name=f"pred{s}") for s, p in enumerate(preds_np)]
    unc = [g.place(u, name=f"unc{s}") for s, u in enumerate(unc_np)]
    gt = g.place(gt_np, name="gt")
    hist = g.empty((4, B, 2, 1026, 3), np.int64, name="hist")
    assert hist.data_ptr() % 16 == 8 and gt.data_ptr() % 16 == 4
    arr = lambda ts: (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ts])     # noqa: E731
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(hip_lib.lws_sparsification(arr(preds), arr(unc), 4, kind, B, Hg + off, W, off, gt.data_ptr(), Hg, 192.0, mode,
                                              hist.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "lws_sparsification")
    G.assert_bits(hist, want, "hist")
    g.check()


def test_graph_capture_replays_the_call(dev, hip_lib):
    """The memset and the kernel are two nodes of a captured graph: every replay clears hist before it counts."""
    from lwsnet_amd import _lib
    B, Hg, W, off, mode, kind = 2, 37, 61, 3, 1, 1
    first, second = make_inputs(B, Hg, W, off, kind, seed=31), make_inputs(B, Hg, W, off, kind, seed=32)
    preds = [torch.from_numpy(p).to(dev) for p in first[0]]
    unc = [torch.from_numpy(u).to(dev) for u in first[1]]
    gt = torch.from_numpy(first[2]).to(dev)
    hist = torch.full((4, B, 2, 1026, 3), -1, device=dev, dtype=torch.int64)
    arr = lambda ts: (ctypes.c_void_p * 4)(*[t.data_ptr() for t in ts])     # noqa: E731
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.device(dev), torch.cuda.graph(graph):
        _lib.check(hip_lib.lws_sparsification(arr(preds), arr(unc), 4, kind, B, Hg + off, W, off, gt.data_ptr(), Hg, 192.0, mode,
                                              hist.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "lws_sparsification")
    for p_np, u_np, g_np in (first, second, first):
        for dst, src in zip(preds + unc + [gt], p_np + u_np + [g_np]):
            dst.copy_(torch.from_numpy(src))
        graph.replay()
        torch.cuda.synchronize(dev)
        assert_hist(hist.cpu().numpy(), REF.histogram(p_np, u_np, g_np, off, 192, mode, kind))


def test_argument_errors_leave_hist_untouched(dev, hip_lib):
    from lwsnet_amd import _lib
    B, Hg, W = 1, 8, 16
    maps = [torch.zeros((B, 1, Hg, W), device=dev) for _ in range(8)]
    gt = torch.ones((B, Hg, W), device=dev)
    hist = torch.full((4, B, 2, 1026, 3), 0x5A5A5A5A5A5A5A5A, device=dev, dtype=torch.int64)
    before = hist.cpu().numpy().copy()
    arr = lambda ts, n=4: (ctypes.c_void_p * 4)(*([t.data_ptr() for t in ts[:n]] + [None] * (4 - n)))     # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(pred=None, unc=None, nmaps=4, kind=0, B=B, Hp=Hg, off=0, gt=gt.data_ptr(), maxdisp=192.0, mode=0, hist=hist.data_ptr()):
        return hip_lib.lws_sparsification(pred if pred is not None else arr(maps[:4]), unc if unc is not None else arr(maps[4:]), nmaps,
                                          kind, B, Hp, W, off, gt, Hg, maxdisp, mode, hist, st)

    inside = (ctypes.c_void_p * 4)(*[hist.data_ptr() + 4 * k for k in range(4)])
    cases = [dict(pred=arr(maps[:4], 3)), dict(unc=arr(maps[4:], 0)), dict(gt=None), dict(hist=None), dict(nmaps=0), dict(nmaps=5),
             dict(kind=2), dict(kind=-1), dict(mode=2), dict(mode=-1), dict(off=-1, Hp=Hg - 1), dict(Hp=Hg + 1), dict(off=1),
             dict(maxdisp=0.0), dict(maxdisp=float("nan")), dict(B=0), dict(B=65536), dict(gt=hist.data_ptr() + 8), dict(pred=inside),
             dict(unc=inside), dict(hist=gt.data_ptr()), dict(hist=maps[5].data_ptr() - 8)]
    with torch.cuda.device(dev):
        for kw in cases:
            assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        torch.cuda.synchronize()
        assert np.array_equal(hist.cpu().numpy(), before)
        assert all(float(m.abs().sum()) == 0 for m in maps) and float(gt.sum()) == B * Hg * W
        assert call() == 0                                                      # and the same call without an error runs
    got = hist.cpu().numpy()
    assert got[:, 0, 0, 1025, 0].tolist() == [0] * 4 and got[:, 0, 0, 0].tolist() == [[Hg * W, 0, Hg * W * 1024]] * 4


def test_ops_validates_shapes_and_names(dev):
    from lwsnet_amd import ops
    g = torch.zeros((2, 8, 16), device=dev)
    p = [torch.zeros((2, 1, 8, 16), device=dev)] * 4
    for bad in (lambda: ops.sparsification(p, p, g, 4, 192, 0, 0),              # Hp must be Hg + row_offset
                lambda: ops.sparsification(p, p[:3], g, 0, 192, 0, 0), lambda: ops.sparsification([], [], g, 0, 192, 0, 0),
                lambda: ops.sparsification(p, p, g, 0, 192, 2, 0), lambda: ops.sparsification(p, p, g, 0, 192, 0, "entropy"),
                lambda: ops.sparsification(p, p, g.double(), 0, 192, 0, 0), lambda: ops.sparsification(p, p, g, 0, 0.0, 0, 0)):
        with pytest.raises(ValueError):
            bad()
    assert tuple(ops.sparsification(p[:2], p[:2], g, 0, 192, "epe", "conf").shape) == (2, 2, 2, 1026, 3)


def test_cli_sparsification_end_to_end(tmp_path, dev):
    from lwsnet_amd import datasets as D
    from lwsnet_amd import synth
    from lwsnet_amd.evaluate import build_parser
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import make_state_dict
    root = str(tmp_path / "kitti") + "/"
    split = synth.write_kitti_tree(root, 3)
    common = ["--dataset", "kitti2015", "--datapath", root, "--val_set", split]
    plain, _ = _cli(common, tmp_path / "plain.json")
    res, log = _cli(common + ["--sparsification"], tmp_path / "spars.json")
    assert "sparsification" not in plain
    for k in ("average", "per_batch", "per_image"):
        assert res[k] == plain[k], k
    sp = res["sparsification"]
    assert "Sparsification (conf): AUSE Stage 0=" in log and "Sparsification (sigma): AUSE Stage 0=" in log
    assert log.index("Average test 3-Pixel Error") < log.index("Sparsification (conf)") < log.index("Sparsification (sigma)")
    F = len(sp["fractions"])
    assert F == 100 and sp["fractions"][0] == 0 and sp["fractions"][-1] == 0.99
    for kind in ("conf", "sigma"):
        assert len(sp[kind]["ause"]) == len(sp[kind]["ause_rel"]) == 4 and np.shape(sp[kind]["curve"]) == (4, F)
        assert np.shape(sp["per_image_ause"][kind]) == (3, 4)
        assert [c[0] for c in sp[kind]["curve"]] == sp["all"]
    assert np.shape(sp["oracle"]["curve"]) == (4, F) and len(sp["all"]) == 4
    # the same numbers from the maps model.forward_conf returns, through the numpy restatement; the histograms are integers, so the
    # only float arithmetic is the host's
    ds = D.StereoPairs(*D.kitti2015_lists(root, split)[3:], training=False, kitti_set=True)
    args = build_parser().parse_args([])
    model = LWSNet(args, device=dev)
    model.set_state_dict(make_state_dict(7, args))
    model.eval()
    pooled = {"conf": 0, "sigma": 0}
    per_image = {"conf": [], "sigma": []}
    for i in range(0, len(ds), 2):
        items = [ds[j] for j in range(i, min(i + 2, len(ds)))]
        r = model.forward_conf(np.stack([t[0] for t in items]), np.stack([t[1] for t in items]))
        gt = np.stack([t[2] for t in items]).astype(np.float32)
        preds = [p.cpu().numpy() for p in r.preds]
        off = preds[0].shape[2] - gt.shape[1]
        for kind, maps in (("conf", r.conf), ("sigma", r.sigma)):
            u = [m.cpu().numpy() for m in maps]
            h = REF.histogram(preds, u + [u[2]], gt, off, 192, 0, 1 if kind == "conf" else 0)
            pooled[kind] = pooled[kind] + h.sum(axis=1)
            per_image[kind] += [[REF.ause_loop(h[s, b], "kitti") for s in range(4)] for b in range(h.shape[1])]
    for kind in ("conf", "sigma"):
        want = [REF.ause_loop(pooled[kind][s], "kitti") for s in range(4)]
        print(kind, "ause", sp[kind]["ause"], "restated", want)
        np.testing.assert_allclose(sp[kind]["ause"], want, rtol=1e-12)
        np.testing.assert_allclose(sp["per_image_ause"][kind], per_image[kind], rtol=1e-12)
    want_all = [int(pooled["conf"][s][0, :, 1].sum()) / int(pooled["conf"][s][0, :, 0].sum()) for s in range(4)]
    assert sp["all"] == want_all
