"""numpy restatement of the one-forward occlusion check (include/lwsnet_hip.h: lws_occlusion_check), one float32 operation per
step as the contract states it, so the GPU tests compare bit for bit.  Nothing like the kernel: whole-array operations, the
z-buffer by np.maximum.at on the key words, the fill by lr_reference.background_fill."""
import numpy as np

import lr_reference as LR


def key(d):
    """The order-preserving uint32 word of float32 values: bits ^ (sign ? 0xffffffff : 0x80000000)."""
    u = np.ascontiguousarray(d, np.float32).view(np.uint32)
    return u ^ np.where(u >> np.uint32(31), np.uint32(0xffffffff), np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.ascontiguousarray(k, np.uint32)
    return (k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xffffffff)).astype(np.uint32)).view(np.float32)


def targets(dl):
    """dl [..., W] -> (t = x - d as float32, inview = d is no NaN and 0 <= t <= W-1)."""
    W = dl.shape[-1]
    x = np.arange(W, dtype=np.int64).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x - dl).astype(np.float32)
        inview = ~np.isnan(dl) & (t >= np.float32(0)) & (t <= np.float32(W - 1))
    return t, inview


def splat(dl):
    """dl [R, W] float32 -> Z [R, W] uint32: per row the largest key that landed on each column, 0 where nothing did."""
    R, W = dl.shape
    t, inview = targets(dl)
    ts = np.where(inview, t, np.float32(0))
    lo, hi = np.floor(ts), np.ceil(ts)
    k = key(dl)
    rows = np.broadcast_to(np.arange(R)[:, None], dl.shape)
    Z = np.zeros((R, W), np.uint32)
    np.maximum.at(Z, (rows[inview], lo.astype(np.int64)[inview]), k[inview])
    two = inview & (hi != lo)
    np.maximum.at(Z, (rows[two], lo.astype(np.int64)[two] + 1), k[two])
    return Z


def occ_codes(dl, Z, tau):
    """uint8 codes of dl [R, W] against its z-buffer: 1 visible, 0 occluded by a nearer surface (or NaN d), 2 out of view."""
    t, inview = targets(dl)
    j = np.rint(np.where(inview, t, np.float32(0))).astype(np.int64)
    z = unkey(np.take_along_axis(Z, j, axis=-1))
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (z - dl).astype(np.float32) <= np.float32(tau)
    code = np.where(inview, np.where(ok, 1, 0), 2)
    return np.where(np.isnan(dl), 0, code).astype(np.uint8)


def occlusion_check(dl, tau, fill):
    """One stage: dl [B,1,H,W] -> (out, mask, right, row_kept [B,H])."""
    dl = np.ascontiguousarray(dl, np.float32)
    rows = dl.reshape(-1, dl.shape[-1])
    Z = splat(rows)
    code = occ_codes(rows, Z, tau).reshape(dl.shape)
    if fill:
        out = LR.background_fill(dl, code)
    else:
        out = np.where(code == 1, dl, np.float32(0)).astype(np.float32)
    right = np.where(Z == 0, np.float32(0), unkey(Z)).astype(np.float32).reshape(dl.shape)
    row_kept = (code == 1).sum(axis=-1, dtype=np.int32)[:, 0]
    return out, code, right, row_kept
