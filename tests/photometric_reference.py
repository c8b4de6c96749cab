"""lws_photometric (include/lwsnet_hip.h) restated in float32 numpy: every step one float32 operation in the contract's order, the
3 x 3 window by vectorised shifts (horizontally first, then vertically), the sums from the rounded values in numpy int64.  The
device outputs must equal these bit for bit (tests/test_gpu_photometric.py); tests/test_photometric_cpu.py holds the restatement
itself to an independent float64 evaluation."""
from collections import namedtuple

import numpy as np

F = np.float32
C1, C2 = F(6.5025), F(58.5225)
Q = F(1048576.0)

Photo = namedtuple("Photo", ["err", "scored", "warped", "sums", "pe", "l1", "ds", "w"])
Photo.__doc__ = """err float32 [B,1,H,W], scored uint8 [B,1,H,W], warped uint8 [B,H,W,3], sums int64 [B,4]: the outputs of one map.  Behind
them, for the CPU tests: pe, l1, ds float32 [B,H,W] (0 outside the image's interior, otherwise the value whether scored or not)
and w float32 [B,H,W,3], the warped colours before rounding (0 where not warpable)."""


def warp(disp, right, rvalid=None):
    """disp [B,1,H,W] float32, right [B,H,W,3] uint8, rvalid None or [B,1,H,W] uint8 -> (w float32 [B,H,W,3], warpable bool [B,H,W])."""
    d = np.asarray(disp, dtype=F)[:, 0]
    B, H, W = d.shape
    with np.errstate(invalid="ignore"):
        t = np.arange(W, dtype=F) - d
        ok = ~np.isnan(d) & (t >= F(0)) & (t <= F(W - 1))
    ts = np.where(ok, t, F(0)).astype(F)
    fl = np.floor(ts)
    i0 = fl.astype(np.int64)
    i1 = np.minimum(i0 + 1, W - 1)
    if rvalid is not None:
        rv = np.asarray(rvalid)[:, 0]
        ok = ok & (np.take_along_axis(rv, i0, axis=2) == 1) & (np.take_along_axis(rv, i1, axis=2) == 1)
    a = (ts - fl).astype(F)
    r = np.asarray(right).astype(F)
    r0 = np.take_along_axis(r, i0[..., None], axis=2)
    r1 = np.take_along_axis(r, i1[..., None], axis=2)
    w = r0 + a[..., None] * (r1 - r0)
    return np.where(ok[..., None], w, F(0)).astype(F), ok


def _window(v):
    """[B,H,W,...] -> [B,H-2,W-2,...]: the 3 x 3 sums, horizontally first (H, W >= 3)."""
    h = (v[:, :, :-2] + v[:, :, 1:-1]) + v[:, :, 2:]
    return (h[:, :-2] + h[:, 1:-1]) + h[:, 2:]


def photometric(disp, left, right, mask=None, rvalid=None, alpha=0.85):
    """One map: disp [B,1,H,W] float32, left / right [B,H,W,3] uint8, mask / rvalid None or [B,1,H,W] uint8.  Returns a Photo."""
    alpha = F(alpha)
    w, ok = warp(disp, right, rvalid)
    B, H, W = ok.shape
    warped = np.rint(w).astype(np.uint8)
    pe, l1, ds = (np.zeros((B, H, W), F) for _ in range(3))
    scored = np.zeros((B, H, W), bool)
    if H >= 3 and W >= 3:
        x = np.asarray(left).astype(F)
        y = w
        a = np.abs(x - y)
        l1 = (((a[..., 0] + a[..., 1]) + a[..., 2]) / F(3.0)) / F(255.0)
        Sx, Sy, Sxx, Syy, Sxy = _window(x), _window(y), _window(x * x), _window(y * y), _window(x * y)
        mx, my = Sx / F(9.0), Sy / F(9.0)
        vx, vy, cxy = Sxx / F(9.0) - mx * mx, Syy / F(9.0) - my * my, Sxy / F(9.0) - mx * my
        n = ((F(2.0) * mx) * my + C1) * (F(2.0) * cxy + C2)
        m = ((mx * mx + my * my) + C1) * ((vx + vy) + C2)
        dsc = np.minimum(np.maximum((F(1.0) - n / m) * F(0.5), F(0.0)), F(1.0))
        ds[:, 1:-1, 1:-1] = ((dsc[..., 0] + dsc[..., 1]) + dsc[..., 2]) / F(3.0)
        l1[:, 0], l1[:, -1], l1[:, :, 0], l1[:, :, -1] = 0, 0, 0, 0
        pe = alpha * ds + (F(1.0) - alpha) * l1
        pe[:, 0], pe[:, -1], pe[:, :, 0], pe[:, :, -1] = 0, 0, 0, 0
        scored[:, 1:-1, 1:-1] = _window(ok.astype(np.int64)) == 9
        if mask is not None:
            scored &= np.asarray(mask)[:, 0] == 1
    assert pe.dtype == F and l1.dtype == F and ds.dtype == F
    err = np.where(scored, pe, F(0)).astype(F)
    q = [np.where(scored, np.rint(v * Q), F(0)).astype(np.int64) for v in (pe, l1, ds)]
    sums = np.stack([scored.sum(axis=(1, 2), dtype=np.int64)] + [v.sum(axis=(1, 2), dtype=np.int64) for v in q], axis=1)
    return Photo(err[:, None], scored.astype(np.uint8)[:, None], warped, sums, pe, l1, ds, w)


def sums_from_err(err, scored):
    """The first two columns of sums, recomputed per image from returned err and scored maps [B,1,H,W]: {count, sum q(pe)}."""
    sc = np.asarray(scored)[:, 0] == 1
    q = np.where(sc, np.rint(np.asarray(err, dtype=F)[:, 0] * Q), F(0)).astype(np.int64)
    return np.stack([sc.sum(axis=(1, 2), dtype=np.int64), q.sum(axis=(1, 2), dtype=np.int64)], axis=1)
