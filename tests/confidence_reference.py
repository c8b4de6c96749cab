"""numpy float32 restatement of the confidence contract (include/lwsnet_hip.h: lws_softargmin_conf), one float32 operation per step,
the sums explicit ascending loops over k.  Beyond numpy it uses only the C oracle's expf (the library's polynomial, restated in
oracle/lws_oracle.c) and its two resizes, which follow oracle.lws_oracle.VARIANT["align_mode"]."""
import numpy as np

from oracle import c_oracle as C

F = np.float32


def low_maps(cost, start):
    """cost [B,D,h,w] float32 -> (d, peak, sig), each [B,h,w] float32."""
    cost = np.ascontiguousarray(cost, dtype=F)
    D = cost.shape[1]
    neg = -cost
    m = neg[:, 0].copy()
    for k in range(1, D):
        m = np.maximum(m, neg[:, k])
    e = [C.expf(neg[:, k] - m) for k in range(D)]
    S = np.zeros_like(m)
    for k in range(D):
        S = S + e[k]
    p = [e[k] / S for k in range(D)]
    v = [F(start) + F(k) for k in range(D)]
    d = np.zeros_like(m)
    for k in range(D):
        d = d + p[k] * v[k]
    peak = np.zeros_like(m)
    var = np.zeros_like(m)
    for k in range(D):
        t = v[k] - d
        peak = np.where(np.abs(t) <= F(1.0), peak + p[k], peak)
        var = var + p[k] * (t * t)
    sig = np.sqrt(var)
    for a in (d, peak, sig):
        assert a.dtype == F
    return d, peak, sig


def full_maps(peak, sig, H, W):
    """(peak, sig) [B,h,w] -> (conf, sigma) [B,1,H,W]: the resize of peak, and of sig in full-resolution pixels."""
    return C.resize_bilinear(peak, H, W)[:, None], C.upsample_add(sig, None, H, W)


def softargmin_conf(cost, start, H, W):
    """-> dict of the five outputs of lws_softargmin_conf."""
    d, peak, sig = low_maps(cost, start)
    conf, sigma = full_maps(peak, sig, H, W)
    return {"disp_low": d, "peak_low": peak, "sigma_low": sig, "conf": conf, "sigma": sigma}


def low_maps_f64(cost, start, d32):
    """peak and sig of the same formulas evaluated in float64 (numpy's exp), the |t| <= 1 window taken from the float32 d32 so that
    a boundary cannot flip."""
    c = np.asarray(cost, np.float64)
    D = c.shape[1]
    e = np.exp(-c - (-c).max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    v = (np.float64(start) + np.arange(D, dtype=np.float64))[None, :, None, None]
    d = (p * v).sum(axis=1)
    inside = np.abs((F(start) + np.arange(D, dtype=F))[None, :, None, None] - d32[:, None]) <= F(1.0)
    peak = (p * inside).sum(axis=1)
    sig = np.sqrt((p * (v - d[:, None]) ** 2).sum(axis=1))
    return peak, sig
