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


# ---- the photometric reprojection error from the integer sums of lws_photometric ----
PHOTO_SCALE = 1 << 20


def photometric_means(sums, pixels=None):
    """The per-map means of ops.photometric's sums, an integer [nmaps,B,4] array (or tensor) {scored pixels, sum q(pe), sum q(l1),
    sum q(dssim)} with q(v) = rint(v * 2**20), pooled over the PIXELS of the B images: sum q / (2**20 * sum count).  Returns a dict
    of lists with one entry per map: "pe", "l1", "dssim" (None for a map without a scored pixel), "scored" (the pixel count) and
    "density" = scored / (B * pixels), pixels = H * W of one image (None when pixels is not given)."""
    if hasattr(sums, "detach"):
        sums = sums.detach().cpu().numpy()
    sums = np.asarray(sums)
    if sums.ndim != 3 or sums.shape[2] != 4 or sums.dtype.kind not in "iu":
        raise ValueError(f"sums must be an integer [nmaps,B,4] array; got {sums.dtype} {sums.shape}")
    if pixels is not None and (int(pixels) != pixels or pixels < 1):
        raise ValueError(f"pixels must be a positive integer, got {pixels!r}")
    tot = [[int(v) for v in row] for row in sums.astype(np.int64).sum(axis=1)]          # python integers: exact
    res = {"scored": [t[0] for t in tot]}
    for k, name in ((1, "pe"), (2, "l1"), (3, "dssim")):
        res[name] = [t[k] / (PHOTO_SCALE * t[0]) if t[0] > 0 else None for t in tot]
    res["density"] = [t[0] / (sums.shape[1] * int(pixels)) if pixels is not None else None for t in tot]
    return res
