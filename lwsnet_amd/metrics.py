"""Evaluation metrics of the reference."""
import numpy as np


def error_3px(disp, gt, maxdisp=192):
    """KITTI 3-pixel error, /root/reference/finetune.py:212-219: over 0 < gt < maxdisp, the fraction of pixels with
    |d - gt| > 3 and |d - gt| / gt > 0.05."""
    disp = np.asarray(disp, dtype=np.float64)
    gt = np.asarray(gt, dtype=np.float64)
    mask = (gt > 0) & (gt < maxdisp)
    err = np.abs(disp - gt)
    bad = (err[mask] > 3.0) & (err[mask] / gt[mask] > 0.05)
    return float(bad.sum()) / float(mask.sum())


def end_point_error(disp, gt, maxdisp=192):
    """SceneFlow EPE, /root/reference/train.py:179 (mask = gt < maxdisp) and :190 (mean |d - gt| over the mask)."""
    disp = np.asarray(disp, dtype=np.float64)
    gt = np.asarray(gt, dtype=np.float64)
    mask = gt < maxdisp
    return float(np.abs(disp[mask] - gt[mask]).mean())


# ---- sparsification curves and AUSE (Ilg et al. 2018) from the integer histograms of lws_sparsification ----
SPARS_BINS = 1026


def spars_bin(v):
    """The histogram bin of lws_sparsification (include/lwsnet_hip.h) for float32 values: 1025 for NaN and v >= 256, 0 for
    v < 2**-24 (negatives and both zeros), otherwise 1 + ((bits >> 18) - 3296): 32 logarithmic bins per octave over
    [2**-24, 2**8).  Returns int64 of v's shape."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        top = ~(v < np.float32(256.0))
        low = v < np.float32(2.0 ** -24)
    mid = (np.ascontiguousarray(v).view(np.uint32) >> np.uint32(18)).astype(np.int64) - 3295
    return np.where(top, SPARS_BINS - 1, np.where(low, 0, mid)).astype(np.int64)


def spars_bin_edges():
    """The float64 lower edges of bins 1..1025: 2**(-24 + j // 32) * (1 + (j % 32) / 32) for j = 0..1024; the last one is 256."""
    j = np.arange(SPARS_BINS - 1)
    return np.ldexp(1.0 + (j % 32) / 32.0, -24 + j // 32)


def sparsification_curves(hist, metric, fractions=None):
    """The sparsification curves of one map from its [2,1026,3] histogram (ranking under test / oracle ranking; per bin
    {pixels, bad pixels, error sum in 1/1024 px}), pooled over whatever the caller likes.  Per ranking: with the cumulative sums
    n_j and num_j over ascending bins (num: the bad pixels for metric "kitti", the error sum / 1024 for "epe"), every non-empty
    bin gives the exact curve point x_j = 1 - n_j / N (the fraction removed when bins above j go), y_j = num_j / n_j (the error of
    the rest); the curve is np.interp over the points sorted by x.  Returns a dict: fractions, unc and oracle (the two curves at
    the fractions), all (= y(0), the error of all pixels), ause (the mean over the fractions of unc - oracle) and ause_rel
    (ause / all, None when all is 0).  No valid pixel: ValueError."""
    if metric not in ("kitti", "epe"):
        raise ValueError(f"metric must be 'kitti' or 'epe', got {metric!r}")
    hist = np.asarray(hist)
    if hist.shape != (2, SPARS_BINS, 3) or hist.dtype.kind not in "iu":
        raise ValueError(f"hist must be an integer [2,{SPARS_BINS},3] array; got {hist.dtype} {hist.shape}")
    fractions = np.linspace(0, 0.99, 100) if fractions is None else np.asarray(fractions, dtype=np.float64)
    curves = []
    for r in range(2):
        cnt = hist[r, :, 0].astype(np.int64)
        n = np.cumsum(cnt)
        if n[-1] == 0:
            raise ValueError("the histogram has no valid pixel")
        if metric == "kitti":
            num = np.cumsum(hist[r, :, 1].astype(np.int64)).astype(np.float64)
        else:
            num = np.cumsum(hist[r, :, 2].astype(np.int64)).astype(np.float64) / 1024.0
        keep = cnt > 0
        x = 1.0 - n[keep].astype(np.float64) / float(n[-1])
        y = num[keep] / n[keep].astype(np.float64)
        curves.append(np.interp(fractions, x[::-1], y[::-1]))       # n ascends, so x descends
        if r == 0:
            total = float(y[-1])                                    # the last non-empty bin: x = 0, every pixel kept
    ause = float(np.mean(curves[0] - curves[1]))
    return {"fractions": fractions, "unc": curves[0], "oracle": curves[1], "all": total, "ause": ause,
            "ause_rel": ause / total if total != 0 else None}
