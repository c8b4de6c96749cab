"""Dataset evaluation on the device: lws_stage_metrics against the reference's float32 numpy formulas (finetune.py:212-219
error_estimating, train.py:180,189-190 EPE), its determinism and batch independence, StereoPairs.raw + lws_preprocess_rgb8 against
StereoPairs[i], and the `python -m lwsnet_amd.evaluate` CLI end to end on generated KITTI / SceneFlow trees (both modes)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def expected(preds, gt, row_offset, maxdisp, mode):
    """numpy float32: counts [4,B,2], abs_sum [4,B] (fp64 sum of the float32 e over the mask)."""
    B = gt.shape[0]
    counts = np.zeros((4, B, 2), np.int64)
    sums = np.zeros((4, B), np.float64)
    md = np.float32(maxdisp)
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in range(4):
            for b in range(B):
                g = gt[b]
                e = np.abs(preds[s][b, 0, row_offset:] - g)
                mask = (g < md) & ((g > 0) if mode == 0 else True)
                bad = mask & (e > np.float32(3.0)) & (e / g > np.float32(0.05))
                counts[s, b] = mask.sum(), bad.sum()
                sums[s, b] = e[mask].astype(np.float64).sum()
    return counts, sums


def run(preds, gt, row_offset, maxdisp, mode):
    from lwsnet_amd import ops
    dev = _dev()
    counts, sums = ops.stage_metrics([torch.from_numpy(p).to(dev) for p in preds], torch.from_numpy(gt).to(dev), row_offset,
                                     maxdisp, mode)
    return counts.cpu().numpy(), sums.cpu().numpy()


def make(B, Hg, W, row_offset, seed):
    rng = np.random.default_rng(seed)
    gt = (rng.random((B, Hg, W)) * 230 - 15).astype(np.float32)
    preds = []
    for s in range(4):
        p = np.zeros((B, 1, Hg + row_offset, W), np.float32)
        p[:, 0, row_offset:] = gt + (rng.standard_normal((B, Hg, W)) * 4 * (s + 1)).astype(np.float32)
        p[:, 0, :row_offset] = 1000.0                        # the padded rows must never be read
        preds.append(p)
    return preds, gt


def check(preds, gt, row_offset, maxdisp, mode):
    got_c, got_s = run(preds, gt, row_offset, maxdisp, mode)
    want_c, want_s = expected(preds, gt, row_offset, maxdisp, mode)
    assert np.array_equal(got_c, want_c), (mode, np.argwhere(got_c != want_c)[:5])
    finite = np.isfinite(want_s)
    assert np.array_equal(np.isnan(got_s), np.isnan(want_s)) and np.array_equal(got_s[~finite & ~np.isnan(want_s)],
                                                                               want_s[~finite & ~np.isnan(want_s)])
    np.testing.assert_allclose(got_s[finite], want_s[finite], rtol=1e-9)
    return got_c, got_s


@pytest.mark.parametrize("B,Hg,W,off", [(1, 368, 1232, 0), (3, 540, 960, 4), (2, 37, 61, 0), (2, 37, 61, 3), (3, 5, 7, 4)])
@pytest.mark.parametrize("mode", [0, 1])
def test_stage_metrics_match_numpy_float32(B, Hg, W, off, mode):
    preds, gt = make(B, Hg, W, off, seed=B * 1000 + Hg + W + off)
    counts, sums = check(preds, gt, off, 192, mode)
    # the per-batch EPE against numpy's own float32 mean (train.py:190)
    mask = (gt < 192) & ((gt > 0) if mode == 0 else True)
    for s in range(4):
        ref = float(np.mean(np.abs(preds[s][:, 0, off:][mask] - gt[mask])))
        np.testing.assert_allclose(sums[s].sum() / counts[s, :, 0].sum(), ref, rtol=1e-5)


@pytest.mark.parametrize("mode", [0, 1])
def test_stage_metrics_planted_boundary_values(mode):
    B, Hg, W, off = 2, 37, 61, 4
    preds, gt = make(B, Hg, W, off, seed=7)
    d84n = np.nextafter(np.float32(84), np.float32(100))
    assert np.float32(4) / np.float32(80) == np.float32(0.05) and (d84n - np.float32(80)) / np.float32(80) > np.float32(0.05)
    planted = [  # (gt, pred for every stage)
        (50.0, 53.0),                 # e == 3: not bad
        (80.0, 84.0),                 # e / g rounds to exactly 0.05f: not bad
        (80.0, d84n),                 # next float up: bad
        (0.0, 10.0), (192.0, 1.0), (49151 / 256, 1.0), (-3.0, 20.0), (-0.0, 5.0),
        (np.nan, 5.0), (np.inf, 5.0), (-np.inf, 5.0),
        (30.0, np.nan),               # NaN prediction: never bad, abs_sum NaN where valid
    ]
    for k, (g, p) in enumerate(planted):
        for b in range(B):
            y, x = 3 + 2 * k + b, 5 + 3 * k
            gt[b, y, x] = g
            for s in range(4):
                preds[s][b, 0, off + y, x] = p
    counts, sums = check(preds, gt, off, 192, mode)
    assert np.isnan(sums).all()                              # the NaN prediction sits on a valid pixel in both modes
    # image 0 without the -inf and NaN-prediction pixels: finite, still exact
    gt2 = gt.copy()
    for b in range(B):
        for k in (10, 11):
            gt2[b, 3 + 2 * k + b, 5 + 3 * k] = 500.0
    check(preds, gt2, off, 192, mode)


def test_stage_metrics_are_deterministic_and_batch_independent():
    from lwsnet_amd import ops
    dev = _dev()
    for B, Hg, W, off in ((8, 368, 1232, 0), (8, 37, 61, 4)):         # W = 61: every other image of the batch is misaligned
        preds, gt = make(B, Hg, W, off, seed=11)
        preds[0][3, 0, off + 1, 2] = np.nan
        P = [torch.from_numpy(p).to(dev) for p in preds]
        G = torch.from_numpy(gt).to(dev)
        c1, s1 = ops.stage_metrics(P, G, off, 192, 1)
        c2, s2 = ops.stage_metrics(P, G, off, 192, 1)
        assert torch.equal(c1, c2) and np.array_equal(s1.cpu().numpy().view(np.int64), s2.cpu().numpy().view(np.int64))
        for b in range(B):
            cb, sb = ops.stage_metrics([p[b:b + 1].clone() for p in P], G[b:b + 1].clone(), off, 192, 1)
            assert torch.equal(cb[:, 0], c1[:, b])
            assert np.array_equal(sb[:, 0].cpu().numpy().view(np.int64), s1[:, b].cpu().numpy().view(np.int64)), (B, W, b)


@pytest.mark.parametrize("B,Hg,W,off", [(2, 3, 5, 0),          # one partial quad at the end of each image, one workgroup
                                        (2, 37, 61, 3),        # misaligned images: the scalar loads
                                        (1, 33, 125, 0),       # 4125 pixels: two workgroups, the second nearly empty
                                        (1, 1025, 1024, 0)])   # 257 workgroups: the second launch's strided loop steps twice
@pytest.mark.parametrize("mode", [0, 1])
def test_stage_metrics_keep_the_documented_summation_order(B, Hg, W, off, mode):
    """abs_sum bit for bit against tests/metrics_reference.py, which restates the order of float64 additions written in the header
    of lws_metrics.hip: a sum in any other order passes check()'s rtol, this does not."""
    import metrics_reference as REF
    preds, gt = make(B, Hg, W, off, seed=B * 1000 + Hg + W + off)
    got_c, got_s = run(preds, gt, off, 192, mode)
    want_c, want_s = REF.stage_metrics(preds, gt, off, 192, mode)
    assert np.array_equal(got_c, want_c), (mode, np.argwhere(got_c != want_c)[:5])
    assert np.isfinite(want_s).all()
    assert np.array_equal(got_s.view(np.int64), want_s.view(np.int64)), (mode, got_s, want_s)
    np.testing.assert_allclose(want_s, expected(preds, gt, off, 192, mode)[1], rtol=1e-12)    # the restatement sums the same terms


def test_stage_metrics_validate_shapes():
    from lwsnet_amd import ops
    dev = _dev()
    g = torch.zeros((2, 8, 16), device=dev)
    p = [torch.zeros((2, 1, 8, 16), device=dev)] * 4
    with pytest.raises(ValueError):
        ops.stage_metrics(p, g, 4, 192, 0)                   # Hp must be Hg + row_offset
    with pytest.raises(ValueError):
        ops.stage_metrics(p[:3], g, 0, 192, 0)
    with pytest.raises(ValueError):
        ops.stage_metrics(p, g, 0, 192, 2)
    with pytest.raises(ValueError):
        ops.stage_metrics(p, g.double(), 0, 192, 0)


def test_raw_plus_device_preprocess_equals_getitem(tmp_path):
    from lwsnet_amd import datasets as D
    from lwsnet_amd import ops, synth
    dev = _dev()
    split = synth.write_kitti_tree(str(tmp_path / "kitti"), 2)
    synth.write_sceneflow_tree(str(tmp_path / "sf"), 2)
    kl = D.kitti2015_lists(str(tmp_path / "kitti") + "/", split)[3:]
    sl = D.sceneflow_lists(str(tmp_path / "sf"))[3:]
    for lists, kitti in ((kl, True), (sl, False)):
        ds = D.StereoPairs(*lists, training=False, kitti_set=kitti)
        for i in range(len(ds)):
            left, right, gt = ds.raw(i)
            want = ds[i]
            assert left.dtype == np.uint8 and np.array_equal(gt, want[2])
            if not kitti:
                assert left.shape == (544, 960, 3) and not left[:4].any()          # PIL's zero padding
            x = ops.preprocess_rgb8(torch.from_numpy(np.stack([left, right])).to(dev)).cpu().numpy()
            assert np.array_equal(x[0], want[0]) and np.array_equal(x[1], want[1])


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _cli(args, out_json, timeout=600):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "lwsnet_amd.evaluate", "--synthetic_weights", "--test_batch_size", "2",
                        "--json", str(out_json), *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]
    with open(out_json) as f:
        return json.load(f), r.stderr


def _restated(ds, metric, bs, maxdisp=192):
    """model(left, right) on the same batches, the float32 formulas of the reference on the host."""
    from lwsnet_amd.evaluate import build_parser
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import make_state_dict
    args = build_parser().parse_args([])
    model = LWSNet(args, device=_dev())
    model.set_state_dict(make_state_dict(7, args))
    model.eval()
    vals = []
    for i in range(0, len(ds), bs):
        items = [ds[j] for j in range(i, min(i + bs, len(ds)))]
        outs = model(np.stack([t[0] for t in items]), np.stack([t[1] for t in items]))
        gt = np.stack([t[2] for t in items])
        row = []
        for s in range(4):
            out = outs[s].cpu().numpy()[:, 0]
            if metric == "kitti":
                mask = (gt > 0) & (gt < maxdisp)
                err = np.abs(out - gt)
                row.append(float(((err[mask] > 3.) & (err[mask] / gt[mask] > 0.05)).sum()) / float(mask.sum()))
            else:
                mask = gt < maxdisp
                row.append(float(np.mean(np.abs(out[:, 4:, :][mask] - gt[mask]))))
        vals.append(row)
    return vals, [float(np.mean([v[s] for v in vals])) for s in range(4)]


def test_cli_kitti_end_to_end(tmp_path):
    from lwsnet_amd import datasets as D
    from lwsnet_amd import synth
    root = str(tmp_path / "kitti") + "/"
    split = synth.write_kitti_tree(root, 5)
    res0, log = _cli(["--dataset", "kitti2015", "--datapath", root, "--val_set", split], tmp_path / "w0.json")
    res2, _ = _cli(["--dataset", "kitti2015", "--datapath", root, "--val_set", split, "--workers", "2"], tmp_path / "w2.json")
    ds = D.StereoPairs(*D.kitti2015_lists(root, split)[3:], training=False, kitti_set=True)
    vals, _ = _restated(ds, "kitti", 2)
    assert res0["pairs"] == 5 and res0["batches"] == 3 and res0["per_batch"] == vals
    meters = [0.0] * 4
    for v in vals:                                            # AverageMeter: sum in batch order, / count
        meters = [meters[s] + v[s] for s in range(4)]
    assert res0["average"] == [m / 3 for m in meters]
    for k in ("average", "per_batch", "per_image"):
        assert res2[k] == res0[k], k
    assert "Test [0/3] Stage 0 = " in log and "Average test 3-Pixel Error: Stage 0=" in log


def test_cli_sceneflow_end_to_end(tmp_path):
    from lwsnet_amd import datasets as D
    from lwsnet_amd import synth
    root = str(tmp_path / "sf")
    synth.write_sceneflow_tree(root, 3)
    res0, log = _cli(["--dataset", "sceneflow", "--datapath", root], tmp_path / "w0.json")
    res2, _ = _cli(["--dataset", "sceneflow", "--datapath", root, "--workers", "2"], tmp_path / "w2.json")
    ds = D.StereoPairs(*D.sceneflow_lists(root)[3:], training=False, kitti_set=False)
    vals, avg = _restated(ds, "epe", 2)
    assert res0["pairs"] == 3 and res0["batches"] == 2
    np.testing.assert_allclose(res0["per_batch"], vals, rtol=1e-5)
    np.testing.assert_allclose(res0["average"], avg, rtol=1e-5)
    for k in ("average", "per_batch", "per_image"):
        assert res2[k] == res0[k], k
    assert "Test: [0/2] Stage 0 = " in log and "Average test EPE = Stage 0=" in log
