"""Restatement of lws_sparsification (include/lwsnet_hip.h) and of the sparsification curves in numpy, independent of
lwsnet_amd.metrics: the bin of a value from np.frexp instead of its bits, the histogram from float32 numpy arrays, the curves from
explicit loops.  Shared by tests/test_sparsification_cpu.py and tests/test_gpu_sparsification.py."""
import numpy as np

BINS = 1026
F32 = np.float32


def bin_frexp(v):
    """The bin of float32 values by value, not by bits: v = m * 2**ex with m in [0.5, 1) puts v into octave ex - 1 and into the
    sub-bin floor((2 m - 1) * 32) of its 32; octave -24 starts at bin 1.  All of it is exact in float64."""
    v = np.asarray(v, dtype=np.float32)
    out = np.empty(v.shape, np.int64)
    flat, o = v.reshape(-1), out.reshape(-1)
    with np.errstate(invalid="ignore"):
        m, ex = np.frexp(flat.astype(np.float64))
    for i in range(flat.size):
        x = flat[i]
        if np.isnan(x) or x >= 256.0:
            o[i] = BINS - 1
        elif x < 2.0 ** -24:
            o[i] = 0
        else:
            o[i] = 1 + (int(ex[i]) - 1 + 24) * 32 + int(np.floor((2.0 * m[i] - 1.0) * 32.0))
    return out


def bin_frexp_fast(v):
    """bin_frexp without the loop (the same formulation, vectorised), for whole images."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        m, ex = np.frexp(v.astype(np.float64))
        mid = 1 + (ex.astype(np.int64) - 1 + 24) * 32 + np.floor((2.0 * np.where(np.isfinite(m), m, 0.5) - 1.0) * 32.0).astype(np.int64)
        return np.where(np.isnan(v) | (v >= 256.0), BINS - 1, np.where(v < 2.0 ** -24, 0, mid)).astype(np.int64)


def histogram(preds, unc, gt, row_offset, maxdisp, mode, kind):
    """int64 [nmaps,B,2,1026,3]: per map, image and ranking (0: by the uncertainty, 1: by the error) the {pixels, bad pixels,
    q sum} of every bin, every step one float32 numpy operation.  The sums go through np.bincount, whose float64 weights are exact
    here: every partial sum is an integer below 2**53 (q <= 2**26 per pixel, fewer than 2**26 pixels per image)."""
    nmaps, B = len(preds), gt.shape[0]
    hist = np.zeros((nmaps, B, 2, BINS, 3), np.int64)
    md = F32(maxdisp)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for s in range(nmaps):
            for b in range(B):
                g = gt[b]
                p, un = preds[s][b, 0, row_offset:], unc[s][b, 0, row_offset:]
                assert g.size < 2 ** 26
                e = np.abs(p - g)
                valid = (g < md) & ((g > 0) if mode == 0 else True)
                bad = valid & (e > F32(3.0)) & (e / g > F32(0.05))
                ec = np.fmin(e, F32(65536.0))                       # fmin: a NaN e gives 65536
                q = np.rint(ec * F32(1024.0)).astype(np.int64)
                u = un if kind == 0 else F32(1.0) - un
                for r, key in enumerate((u, e)):
                    bins = bin_frexp_fast(key)[valid]
                    hist[s, b, r, :, 0] = np.bincount(bins, minlength=BINS)
                    hist[s, b, r, :, 1] = np.bincount(bins, weights=bad[valid].astype(np.float64), minlength=BINS).astype(np.int64)
                    hist[s, b, r, :, 2] = np.bincount(bins, weights=q[valid].astype(np.float64), minlength=BINS).astype(np.int64)
    return hist


def curve_loop(rows, metric, fractions):
    """One ranking's curve from its [1026,3] rows with explicit loops: the exact points of the non-empty bins, then linear
    interpolation by hand (clamped outside the points, as np.interp clamps)."""
    N = int(rows[:, 0].sum())
    if N == 0:
        raise ValueError("no valid pixel")
    pts, n, num = [], 0, 0
    for j in range(BINS):
        c = int(rows[j, 0])
        n += c
        num += int(rows[j, 1]) if metric == "kitti" else int(rows[j, 2])
        if c:
            pts.append((1.0 - n / N, (num if metric == "kitti" else num / 1024.0) / n))
    pts.sort()
    out = []
    for f in fractions:
        if f <= pts[0][0]:
            out.append(pts[0][1])
        elif f >= pts[-1][0]:
            out.append(pts[-1][1])
        else:
            for (x0, y0), (x1, y1) in zip(pts[:-1], pts[1:]):
                if x0 <= f < x1:
                    out.append((y1 - y0) / (x1 - x0) * (f - x0) + y0)
                    break
    return np.array(out)


def ause_loop(hist, metric, fractions=None):
    """AUSE of a [2,1026,3] histogram: the mean over the fractions of curve(ranking) - curve(oracle)."""
    fractions = np.linspace(0, 0.99, 100) if fractions is None else fractions
    return float(np.mean(curve_loop(hist[0], metric, fractions) - curve_loop(hist[1], metric, fractions)))
