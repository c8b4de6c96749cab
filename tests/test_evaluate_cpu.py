"""Evaluation bookkeeping (lwsnet_amd/evaluate.py) against a float32 numpy restatement of the reference's two test loops
(finetune.py:184-219 test + error_estimating; train.py:169-199 test), and the host-side argument checks of lws_stage_metrics.
No GPU: the per-image sums are computed here in numpy and fed to `aggregate` as the kernel would return them."""
import ctypes

import numpy as np
import pytest

from lwsnet_amd import _lib
from lwsnet_amd import evaluate as E


# ---- the reference, restated in float32 ------------------------------------------------------------------------------------
def error_estimating32(disp, gt, maxdisp=192):
    disp, gt = np.asarray(disp, np.float32), np.asarray(gt, np.float32)
    mask = (gt > 0) & (gt < maxdisp)
    err = np.abs(disp - gt)
    err3 = ((err[mask] > 3.) & (err[mask] / gt[mask] > 0.05)).sum()
    return float(err3) / float(mask.sum())


class _Meter:
    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def reference_kitti(preds, gts, bs):
    """preds[s]: [N,H,W], gts [N,H,W] -> (per-batch values, averages)"""
    meters, vals = [_Meter() for _ in range(4)], []
    for i in range(0, len(gts), bs):
        row = []
        for s in range(4):
            meters[s].update(error_estimating32(preds[s][i:i + bs], gts[i:i + bs]))
            row.append(meters[s].val)
        vals.append(row)
    return vals, [m.avg for m in meters]


def reference_epe(preds, gts, bs, maxdisp=192):
    """preds[s]: [N,H+4,W] (544-row crop), gts [N,H,W]"""
    meters, vals = [_Meter() for _ in range(4)], []
    for i in range(0, len(gts), bs):
        gt = gts[i:i + bs]
        mask = gt < maxdisp
        row = []
        for s in range(4):
            if len(gt[mask]) == 0:
                row.append(None)
                continue
            out = preds[s][i:i + bs][:, 4:, :]
            meters[s].update(float(np.mean(np.abs(out[mask] - gt[mask]))))
            row.append(meters[s].val)
        vals.append(row)
    return vals, [m.avg for m in meters]


def per_image_sums(preds, gts, mode, maxdisp=192, row_offset=0):
    """What lws_stage_metrics returns, computed in numpy: counts [4,N,2], abs_sum [4,N]."""
    N = len(gts)
    counts = np.zeros((4, N, 2), np.int64)
    sums = np.zeros((4, N), np.float64)
    for s in range(4):
        for n in range(N):
            g = gts[n]
            p = preds[s][n][row_offset:]
            mask = (g < np.float32(maxdisp)) & ((g > 0) if mode == 0 else True)
            e = np.abs(p - g)
            with np.errstate(divide="ignore", invalid="ignore"):
                bad = mask & (e > 3.) & (e / g > 0.05)
            counts[s, n] = (mask.sum(), bad.sum())
            sums[s, n] = e[mask].astype(np.float64).sum()
    return counts, sums


def _batches(counts, sums, bs):
    return [(counts[:, i:i + bs], sums[:, i:i + bs]) for i in range(0, counts.shape[1], bs)]


def _data(N, H, W, seed, pad=0):
    rng = np.random.default_rng(seed)
    gts = (rng.random((N, H, W)) * 220 - 10).astype(np.float32)              # some gt <= 0 and >= 192
    preds = [np.concatenate([np.zeros((N, pad, W), np.float32), gts + (rng.standard_normal((N, H, W)) * 6 * (s + 1)).astype(np.float32)], 1)
             for s in range(4)]
    return preds, gts


# ---- 1. aggregate == the reference loops ---------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [1, 3, 8])
def test_aggregate_kitti_matches_reference(bs):
    preds, gts = _data(11, 9, 13, bs)                       # 11 images: a partial last batch for bs 3 and 8
    counts, sums = per_image_sums(preds, gts, 0)
    avg, vals, lines = E.aggregate(_batches(counts, sums, bs), "kitti")
    want_vals, want_avg = reference_kitti(preds, gts, bs)
    assert vals == want_vals and avg == want_avg           # exact: ratios of the same integers, averaged in the same order
    assert len(vals) == -(-11 // bs) and len(lines) == len(vals) + 1


@pytest.mark.parametrize("bs", [1, 3, 8])
def test_aggregate_epe_matches_reference(bs):
    preds, gts = _data(11, 9, 13, 10 + bs, pad=4)
    counts, sums = per_image_sums(preds, gts, 1, row_offset=4)
    avg, vals, _ = E.aggregate(_batches(counts, sums, bs), "epe")
    want_vals, want_avg = reference_epe(preds, gts, bs)
    assert len(vals) == len(want_vals)
    for got, want in zip(vals, want_vals):
        np.testing.assert_allclose(got, want, rtol=1e-5)
    np.testing.assert_allclose(avg, want_avg, rtol=1e-5)


def test_aggregate_epe_skips_a_batch_without_valid_pixels():
    preds, gts = _data(5, 6, 7, 3, pad=4)
    gts[2:4] = 500.0                                        # batch 1 (images 2, 3 at bs 2): no gt < 192
    counts, sums = per_image_sums(preds, gts, 1, row_offset=4)
    avg, vals, _ = E.aggregate(_batches(counts, sums, 2), "epe")
    want_vals, want_avg = reference_epe(preds, gts, 2)
    assert vals[1] == [None] * 4 and want_vals[1] == [None] * 4
    np.testing.assert_allclose(avg, want_avg, rtol=1e-5)     # the skipped batch does not count in the average
    np.testing.assert_allclose(avg, [(vals[0][s] + vals[2][s]) / 2 for s in range(4)], rtol=1e-12)


def test_aggregate_kitti_empty_batch_raises_naming_its_files():
    preds, gts = _data(4, 5, 6, 4)
    gts[2:] = 0.0
    counts, sums = per_image_sums(preds, gts, 0)
    with pytest.raises(ZeroDivisionError):
        reference_kitti(preds, gts, 2)
    with pytest.raises(ValueError, match="c.png, d.png"):
        E.aggregate(_batches(counts, sums, 2), "kitti", batch_files=[["a.png", "b.png"], ["c.png", "d.png"]])


def test_batch_ranges_are_in_order_and_keep_the_last_partial_batch():
    assert [list(r) for r in E.batch_ranges(5, 2)] == [[0, 1], [2, 3], [4]]
    assert [list(r) for r in E.batch_ranges(3, 8)] == [[0, 1, 2]]


# ---- 2. log lines -------------------------------------------------------------------------------------------------------
def test_log_lines_follow_the_reference():
    counts = np.zeros((4, 1, 2), np.int64)
    counts[:, 0] = (8, 1)
    sums = np.full((4, 1), 12.0)
    _, _, lines = E.aggregate([(counts, sums)] * 3, "kitti")
    assert lines[0] == "Test [0/3] " + "\t".join(f"Stage {s} = 0.1250(0.1250)" for s in range(4))
    assert len(lines) == 4 and lines[2].startswith("Test [2/3] Stage 0 = 0.1250(0.1250)\t")
    assert lines[-1] == "Average test 3-Pixel Error: Stage 0=0.1250, Stage 1=0.1250, Stage 2=0.1250, Stage 3=0.1250"
    _, _, lines = E.aggregate([(counts, sums)] * 12, "epe")    # every 5th batch: 0, 5, 10
    assert [ln.split(" Stage")[0] for ln in lines[:-1]] == ["Test: [0/12]", "Test: [5/12]", "Test: [10/12]"]
    assert lines[0] == "Test: [0/12] " + "\t".join(f"Stage {s} = 1.50(1.50)" for s in range(4))
    assert lines[-1] == "Average test EPE = Stage 0=1.50, Stage 1=1.50, Stage 2=1.50, Stage 3=1.50"


# ---- 3. CLI defaults ----------------------------------------------------------------------------------------------------
def test_cli_defaults_match_the_reference():
    a = E.build_parser().parse_args([])
    assert a.test_batch_size == 8 and a.maxdisp == 192 and a.val_set == "val_set.txt"       # finetune.py:20,33,39; train.py:21,34
    assert a.maxdisplist == [24, 5, 5] and a.channels_3d == 8 and a.layers_3d == 4 and a.growth_rate == [4, 1, 1]
    assert a.workers == 0 and a.dataset == "kitti2015" and a.json is None


def test_cli_refuses_a_missing_val_set(tmp_path):
    args = E.build_parser().parse_args(["--datapath", str(tmp_path), "--val_set", str(tmp_path / "absent.txt")])
    with pytest.raises(FileNotFoundError, match="absent.txt"):
        E.load_dataset(args)


# ---- 4. C ABI argument checks -------------------------------------------------------------------------------------------
def test_stage_metrics_validates_on_host(hip_lib):
    L = hip_lib
    assert L.lws_stage_metrics_workspace(2, 368, 1232) > 0
    assert L.lws_stage_metrics_workspace(2, 368, 1232) == 2 * L.lws_stage_metrics_workspace(1, 368, 1232)
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0)):
        assert L.lws_stage_metrics_workspace(*bad) == _lib.LWS_ERR_INVALID
        assert b"stage_metrics_workspace: bad shape" in L.lws_last_error()
    nz = ctypes.c_void_p(16)                                # never dereferenced: validation fails before any HIP call
    preds = (ctypes.c_void_p * 4)(16, 16, 16, 16)

    def call(pred=preds, B=1, Hp=8, W=8, off=0, gt=nz, Hg=8, md=192.0, mode=0, ws=nz, counts=nz, sums=nz):
        return L.lws_stage_metrics(pred, B, Hp, W, off, gt, Hg, md, mode, ws, counts, sums, None)

    cases = [(dict(pred=(ctypes.c_void_p * 4)(16, 16, 0, 16)), b"pred[2] is null"),
             (dict(gt=None), b"null pointer"), (dict(ws=None), b"null pointer"), (dict(counts=None), b"null pointer"),
             (dict(sums=None), b"null pointer"), (dict(B=0), b"bad shape"), (dict(Hg=0, Hp=0), b"bad shape"),
             (dict(W=0), b"bad shape"), (dict(off=-1, Hp=7), b"row_offset -1"), (dict(Hp=9), b"Hg + row_offset"),
             (dict(mode=2), b"mode 2"), (dict(mode=-1), b"mode -1"), (dict(md=0.0), b"maxdisp must be > 0"),
             (dict(md=-5.0), b"maxdisp must be > 0"), (dict(md=float("nan")), b"maxdisp must be > 0")]
    for kw, msg in cases:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert msg in L.lws_last_error(), (kw, L.lws_last_error())
    # the ground-truth checks shared with lws_sparsification and the workspace query: the whole text
    texts = [(dict(B=0), b"stage_metrics: bad shape B=0 Hg=8 W=8"), (dict(B=65536), b"stage_metrics: bad shape B=65536 Hg=8 W=8"),
             (dict(Hg=0, Hp=0), b"stage_metrics: bad shape B=1 Hg=0 W=8"), (dict(W=-1), b"stage_metrics: bad shape B=1 Hg=8 W=-1"),
             (dict(off=-1, Hp=7), b"stage_metrics: row_offset -1 < 0"),
             (dict(Hp=9), b"stage_metrics: Hp=9 must be Hg + row_offset = 8 + 0"),
             (dict(off=2), b"stage_metrics: Hp=8 must be Hg + row_offset = 8 + 2"),
             (dict(mode=2), b"stage_metrics: mode 2 (0 = KITTI 3-px, 1 = EPE)"),
             (dict(md=0.0), b"stage_metrics: maxdisp must be > 0, got 0"),
             (dict(md=float("nan")), b"stage_metrics: maxdisp must be > 0, got nan"),
             (dict(Hg=1048577, Hp=1048577, W=1048576), b"stage_metrics: 1048577x1048576 is too large"),
             (dict(gt=None), b"stage_metrics: null pointer"), (dict(pred=(ctypes.c_void_p * 4)(16, 16, 0, 16)), b"stage_metrics: pred[2] is null")]
    for kw, msg in texts:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert L.lws_last_error() == msg, kw
    for shape, msg in (((0, 4, 4), b"stage_metrics_workspace: bad shape B=0 4x4"), ((65536, 4, 4), b"stage_metrics_workspace: bad shape B=65536 4x4"),
                       ((1, 0, 4), b"stage_metrics_workspace: bad shape B=1 0x4"), ((1, 4, -1), b"stage_metrics_workspace: bad shape B=1 4x-1"),
                       ((1, 1048577, 1048576), b"stage_metrics_workspace: 1048577x1048576 is too large")):
        assert L.lws_stage_metrics_workspace(*shape) == _lib.LWS_ERR_INVALID
        assert L.lws_last_error() == msg
    assert L.lws_stage_metrics_workspace(1, 1048576, 1048576) == (1 << 28) * 4 * 24      # 2^40 pixels are still allowed
