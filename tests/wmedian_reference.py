"""numpy restatement of lws_wmedian_filter (include/lwsnet_hip.h), written differently from the kernel: per pixel the window is
gathered (one plane per window offset), the candidates are stable-sorted by value, their int64 weights are summed cumulatively and
the first value whose doubled sum reaches the total is taken.  The kernel counts instead of sorting and never orders anything."""
import numpy as np

LUT_SIZE = 766


def valid_pixels(d, mask):
    """valid(q) = (mask is None or mask[q] == 1) and isfinite(d_q) and d_q > 0."""
    with np.errstate(invalid="ignore"):
        v = np.isfinite(d) & (d > np.float32(0.0))
    return v if mask is None else v & (mask == 1)


def window_median(disp, mask, rgb, wlut, radius):
    """disp [B,1,H,W] float32, mask None or uint8 [B,1,H,W], rgb None or uint8 [B,H,W,3], wlut None or uint16 [766].  Returns
    (valid [B,H,W] bool, m [B,H,W] float32 (0 where there is no candidate), n [B,H,W] int64, T [B,H,W] int64): everything the
    output rule needs, whatever fill_min is."""
    disp = np.asarray(disp)
    assert disp.dtype == np.float32 and disp.ndim == 4 and disp.shape[1] == 1 and radius in (1, 2, 3)
    B, _, H, W = disp.shape
    d = disp[:, 0]
    valid = valid_pixels(d, None if mask is None else np.asarray(mask)[:, 0])
    r = radius
    K = (2 * r + 1) ** 2
    val = np.full((B, H, W, K), np.inf, np.float32)         # +inf: sorts behind every candidate
    wgt = np.zeros((B, H, W, K), np.int64)
    if rgb is not None:
        assert wlut is not None and wlut.dtype == np.uint16 and wlut.shape == (LUT_SIZE,)
        assert rgb.dtype == np.uint8 and rgb.shape == (B, H, W, 3)
        col = rgb.astype(np.int64)
        lut = wlut.astype(np.int64)
    k = 0
    for oy in range(-r, r + 1):
        for ox in range(-r, r + 1):
            # the pixels p = (y, x) whose neighbour q = (y + oy, x + ox) lies inside the image
            py = slice(max(0, -oy), min(H, H - oy))
            px = slice(max(0, -ox), min(W, W - ox))
            qy = slice(max(0, -oy) + oy, min(H, H - oy) + oy)
            qx = slice(max(0, -ox) + ox, min(W, W - ox) + ox)
            if py.start < py.stop and px.start < px.stop:
                if rgb is None:
                    w = np.ones((B, py.stop - py.start, px.stop - px.start), np.int64)
                else:
                    w = lut[np.abs(col[:, py, px] - col[:, qy, qx]).sum(axis=-1)]
                cand = valid[:, qy, qx] & (w > 0)
                val[:, py, px, k] = np.where(cand, d[:, qy, qx], np.float32(np.inf))
                wgt[:, py, px, k] = np.where(cand, w, 0)
            k += 1
    order = np.argsort(val, axis=-1, kind="stable")
    sv = np.take_along_axis(val, order, axis=-1)
    cum = np.cumsum(np.take_along_axis(wgt, order, axis=-1), axis=-1)
    T = cum[..., -1]
    n = (wgt > 0).sum(axis=-1)
    first = np.argmax(2 * cum >= T[..., None], axis=-1)     # the first sorted value that meets the threshold
    m = np.take_along_axis(sv, first[..., None], axis=-1)[..., 0]
    m = np.where(n > 0, m, np.float32(0.0)).astype(np.float32)
    return valid, m, n, T


def apply(disp, parts, fill_min):
    """The output rule on what window_median returned: (out [B,1,H,W] float32, counts [B,2] int64)."""
    valid, m, n, T = parts
    d = np.asarray(disp)[:, 0]
    fill = ~valid & (fill_min > 0) & (n >= fill_min)
    out = np.where(valid, np.where(T == 0, d, m), np.where(fill, m, np.float32(0.0))).astype(np.float32)
    changed = valid & (out.view(np.uint32) != np.ascontiguousarray(d).view(np.uint32))
    counts = np.stack([changed.sum(axis=(1, 2)), fill.sum(axis=(1, 2))], axis=1).astype(np.int64)
    return out[:, None], counts


def wmedian_filter(disp, radius, rgb=None, wlut=None, mask=None, fill_min=0):
    """lws_wmedian_filter: (out, counts)."""
    return apply(disp, window_median(disp, mask, rgb, wlut, radius), fill_min)
