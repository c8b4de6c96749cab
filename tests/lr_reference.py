"""numpy restatement of the left-right consistency check (include/lwsnet_hip.h: lws_lr_pairs, lws_lr_check), one float32
operation per step as the kernel computes it, so the GPU tests compare bit for bit."""
import numpy as np


def mirror_w(t):
    return np.ascontiguousarray(np.asarray(t)[..., ::-1])


def lr_pairs(left, right):
    """left, right [B,3,H,W] -> left2 = [left; mirror_w(right)], right2 = [right; mirror_w(left)]."""
    return np.concatenate([left, mirror_w(right)]), np.concatenate([right, mirror_w(left)])


def lr_codes(dl, drm, tau):
    """dl, drm [..., W] float32 (the left-view map and the mirrored right-view map) -> uint8 codes: 1 consistent, 0 inconsistent
    (or NaN d), 2 out of the right camera's view."""
    dl = np.asarray(dl, np.float32)
    drm = np.asarray(drm, np.float32)
    W = dl.shape[-1]
    x = np.arange(W, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (W - 1 - x).astype(np.float32) + dl
        inview = (t >= np.float32(0)) & (t <= np.float32(W - 1))
        ts = np.where(inview, t, np.float32(0))
        i0 = np.floor(ts).astype(np.int64)
        i1 = np.minimum(i0 + 1, W - 1)
        a = ts - i0.astype(np.float32)
        r0 = np.take_along_axis(drm, i0, axis=-1)
        r1 = np.take_along_axis(drm, i1, axis=-1)
        r = r0 + a * (r1 - r0)
        ok = np.abs(dl - r) <= np.float32(tau)
    code = np.where(inview, np.where(ok, 1, 0), 2)
    code = np.where(np.isnan(dl), 0, code)
    return code.astype(np.uint8)


def background_fill(dl, code):
    """code-1 pixels keep d; the others min(d at the nearest code-1 pixel on the left, on the right) of their row (the left value
    on a tie), one side's value if only that side has one, 0 if the row has none."""
    dl = np.asarray(dl, np.float32)
    rows = dl.reshape(-1, dl.shape[-1])
    ok = (np.asarray(code) == 1).reshape(rows.shape)
    W = rows.shape[1]
    idx = np.arange(W)
    last = np.maximum.accumulate(np.where(ok, idx, -1), axis=1)
    nxt = np.minimum.accumulate(np.where(ok, idx, W)[:, ::-1], axis=1)[:, ::-1]
    vl = np.take_along_axis(rows, np.maximum(last, 0), axis=1)
    vr = np.take_along_axis(rows, np.minimum(nxt, W - 1), axis=1)
    hl, hr = last >= 0, nxt < W
    both = np.where(vr < vl, vr, vl)
    out = np.where(hl & hr, both, np.where(hl, vl, np.where(hr, vr, np.float32(0))))
    out = np.where(ok, rows, out).astype(np.float32)
    return out.reshape(dl.shape)


def lr_check(dl, drm, tau, fill):
    """One stage: dl, drm [B,1,H,W] -> (out, mask, right, row_kept [B,H])."""
    dl = np.asarray(dl, np.float32)
    drm = np.asarray(drm, np.float32)
    code = lr_codes(dl, drm, tau)
    if fill:
        out = background_fill(dl, code)
    else:
        out = np.where(code == 1, dl, np.float32(0)).astype(np.float32)
    right = mirror_w(drm)
    row_kept = (code == 1).sum(axis=-1, dtype=np.int32)[:, 0]
    return out, code, right, row_kept
