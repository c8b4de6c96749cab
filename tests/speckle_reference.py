"""numpy / Python restatement of the speckle filter (include/lwsnet_hip.h: lws_speckle_filter), so the GPU tests compare bit for
bit.  It knows nothing of the kernel's tiles: validity and the two planes of join bits come from float32 numpy arithmetic, the
horizontal runs are collapsed with numpy, and a union-find (path halving, the smaller raster index as the root) walks the distinct
vertical edges between runs in plain Python.  tests/test_speckle_cpu.py holds it to an independent flood fill."""
import numpy as np

import lr_reference


def valid_pixels(d, mask):
    d = np.asarray(d, np.float32)
    v = np.isfinite(d) & (d > np.float32(0))
    if mask is not None:
        v &= np.asarray(mask) == 1
    return v


def join_bits(d, valid, max_diff):
    """(right [H,W-1], down [H-1,W]) booleans: the pixel is joined to its right / lower neighbour."""
    d = np.asarray(d, np.float32)
    md = np.float32(max_diff)
    with np.errstate(invalid="ignore", over="ignore"):
        right = valid[:, :-1] & valid[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= md)
        down = valid[:-1, :] & valid[1:, :] & (np.abs(d[:-1, :] - d[1:, :]) <= md)
    return right, down


def label_image(d, mask, max_diff):
    """One image d [H,W] (mask [H,W] uint8 or None) -> (valid [H,W] bool, labels [H,W] int32: the raster index of the first pixel of
    the pixel's component, -1 where invalid, size [H,W] int64: the pixels of the pixel's component, 0 where invalid)."""
    d = np.asarray(d, np.float32)
    H, W = d.shape
    valid = valid_pixels(d, mask)
    right, down = join_bits(d, valid, max_diff)
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    # horizontal runs: a pixel's run starts at the last pixel at or before it that is not joined to its left neighbour
    start = np.ones((H, W), bool)
    start[:, 1:] = ~right
    run = np.maximum.accumulate(np.where(start, idx, -1), axis=1).reshape(-1)
    # the distinct vertical edges between runs
    a, b = run[idx[:-1, :][down]], run[idx[1:, :][down]]
    key = np.unique(a * (H * W) + b)                        # (a, b) as one int64: H*W < 2^31
    edges = np.stack([key // (H * W), key % (H * W)], axis=1)
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]                   # path halving
            i = parent[i]
        return i

    for u, v in edges.tolist():
        ru, rv = find(u), find(v)
        if ru != rv:
            if ru < rv:
                parent[rv] = ru
            else:
                parent[ru] = rv
    par = np.asarray(parent, np.int64)
    while True:                                             # pointer jumping to the roots
        nxt = par[par]
        if np.array_equal(nxt, par):
            break
        par = nxt
    lab = par[run]
    lab = np.where(valid.reshape(-1), lab, -1)
    sizes = np.bincount(lab[lab >= 0], minlength=H * W)
    size = np.where(lab >= 0, sizes[np.maximum(lab, 0)], 0)
    return valid, lab.astype(np.int32).reshape(H, W), size.reshape(H, W)


def apply_image(d, mask, valid, lab, size, max_size, fill):
    """-> (out float32 [H,W], mask_out uint8 [H,W], counts int64 [3] = {valid, kept, removed components})."""
    d = np.asarray(d, np.float32)
    speckle = valid & (size <= max_size)
    invalid_code = np.zeros(d.shape, np.uint8) if mask is None else np.where(np.asarray(mask) != 1, mask, 0).astype(np.uint8)
    code = np.where(valid, np.where(speckle, 3, 1), invalid_code).astype(np.uint8)
    if fill:
        out = lr_reference.background_fill(d, code)
    else:
        out = np.where(code == 1, d, np.float32(0)).astype(np.float32)
    removed = np.unique(lab[speckle]).size
    return out, code, np.array([valid.sum(), (code == 1).sum(), removed], np.int64)


def labelling(disp, mask, max_diff):
    """disp [B,1,H,W], mask the same shape or None -> a list of label_image results, one per image (the part of the filter that
    depends on (disp, mask, max_diff) only: compute it once, then `apply` for every max_size / fill)."""
    disp = np.asarray(disp, np.float32)
    return [label_image(disp[b, 0], None if mask is None else mask[b, 0], max_diff) for b in range(disp.shape[0])]


def apply(disp, mask, lab, max_size, fill):
    """-> (out [B,1,H,W] float32, mask_out uint8, labels int32, counts [B,3] int64)."""
    disp = np.asarray(disp, np.float32)
    outs = [apply_image(disp[b, 0], None if mask is None else mask[b, 0], *lab[b], max_size, fill) for b in range(disp.shape[0])]
    return (np.stack([o[0] for o in outs])[:, None], np.stack([o[1] for o in outs])[:, None],
            np.stack([l[1] for l in lab])[:, None], np.stack([o[2] for o in outs]))


def speckle_filter(disp, mask, max_diff, max_size, fill):
    return apply(disp, mask, labelling(disp, mask, max_diff), max_size, fill)
