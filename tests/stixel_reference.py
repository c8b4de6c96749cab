"""numpy restatement of lws_stixels (include/lwsnet_hip.h): float32 steps as float32 values, one numpy operation per step of the
contract in its order; the sums as Python integers, the mean disparity in Python floats (float64); the walk for y_top as the
loop the header writes.  Builds on ground_reference.valid_z and ground_reference.u16.  Written for clarity, not speed."""
import numpy as np

import ground_reference as G

F = np.float32


def taking(d, cam, codes, min_disp, max_depth, code_bits, sub, nbins):
    """take(p) and the bins: (bool [B,1,H,W], int64 [B,1,H,W], 0 where the pixel takes no part)."""
    d = np.asarray(d, F)
    valid, _ = G.valid_z(d, None, cam, min_disp, max_depth)
    code = np.asarray(codes).astype(np.int64)
    with np.errstate(all="ignore"):
        t = np.floor(d * F(sub))
        take = valid & (code < 6) & (((code_bits >> np.minimum(code, 6)) & 1) == 1) & (t < F(nbins))
    return take, np.where(take, t, F(0)).astype(np.int64)


def walk(flag, y_base, max_gap):
    """y_top of the header: up from y_base over gaps of at most max_gap unflagged rows."""
    y_top, gap = y_base, 0
    for y in range(y_base - 1, -1, -1):
        if flag[y]:
            y_top, gap = y, 0
        else:
            gap += 1
            if gap > max_gap:
                break
    return y_top


def strip_layers(take, q, Q, hbits, cam, x0, x1, nbins, tol_bins, min_count, min_row, max_gap, layers):
    """One strip ([H, ws] arrays; cam: the image's row) -> (U int64 [nbins], rows int32 [layers,4], vals uint32 bit patterns [layers,4])."""
    U = np.bincount(q[take], minlength=nbins).astype(np.int64)
    rows = np.zeros((layers, 4), np.int32)
    rows[:, 1:] = -1
    vals = np.zeros((layers, 4), np.uint32)
    fx, cx, fb = F(cam[0]), F(cam[2]), F(cam[4])
    pre = np.concatenate([[0], np.cumsum(U)])
    kmax = nbins - 1
    for j in range(layers):
        if kmax < 0:
            break
        k = np.arange(kmax + 1)
        wn = pre[np.minimum(k + tol_bins, kmax) + 1] - pre[np.maximum(k - tol_bins, 0)]
        near = np.flatnonzero(wn >= min_count)
        if near.size == 0:
            break
        k_near = int(near[-1])
        lo, hi = max(k_near - tol_bins, 0), min(k_near + tol_bins, kmax)
        win = U[lo:hi + 1]
        k_peak = lo + int(np.flatnonzero(win == win.max())[-1])         # the larger bin wins a tie
        member = take & (np.abs(q - k_peak) <= tol_bins) & (q <= kmax)
        kmax = k_peak - tol_bins - 1
        rows[j, 3] = k_peak
        flag = member.sum(axis=1) >= min_row
        if not flag.any():
            continue                                                    # a hole
        y_base = int(np.flatnonzero(flag)[-1])
        y_top = walk(flag, y_base, max_gap)
        m = member[y_top:y_base + 1]
        n, sq = int(m.sum()), int(Q[y_top:y_base + 1][m].astype(np.int64).sum())
        hb = int(hbits[y_top:y_base + 1][m].max())
        with np.errstate(all="ignore"):
            d_st = F((float(sq) / float(n)) / 256.0)
            z = fb / d_st
            xc = F(x0 + x1) * F(0.5)
            X = ((xc - cx) * z) / fx
        rows[j, :3] = n, y_top, y_base
        vals[j] = np.array([d_st, z, X], F).view(np.uint32).tolist() + [hb]
    return U, rows, vals


def stixels(d, cam, codes, height, min_disp, max_depth, code_bits, width, sub, nbins, tol_bins, min_count, min_row, max_gap, layers):
    """-> (rows int32 [B,S,layers,4], vals float32 [B,S,layers,4], udisp uint32 [B,S,nbins]); cam float32 [B,5]."""
    d, cam = np.asarray(d, F), np.asarray(cam, F)
    B, _, H, W = d.shape
    S = -(-W // width)
    take, q = taking(d, cam, codes, min_disp, max_depth, code_bits, sub, nbins)
    Q = G.u16(d).astype(np.int64)
    hbits = np.ascontiguousarray(np.asarray(height, F)).view(np.uint32)
    rows, vals = np.zeros((B, S, layers, 4), np.int32), np.zeros((B, S, layers, 4), np.uint32)
    udisp = np.zeros((B, S, nbins), np.uint32)
    for b in range(B):
        for s in range(S):
            x0 = s * width
            x1 = min(x0 + width, W) - 1
            cols = slice(x0, x1 + 1)
            U, rows[b, s], vals[b, s] = strip_layers(take[b, 0, :, cols], q[b, 0, :, cols], Q[b, 0, :, cols], hbits[b, 0, :, cols], cam[b], x0,
                                                     x1, nbins, tol_bins, min_count, min_row, max_gap, layers)
            udisp[b, s] = U
    return rows, vals.view(F), udisp


def column_map(H, W, width, strips, background=0.0):
    """A hand-made map for the tests: `strips` = {strip index: [(y0, y1, disparity), ..]} fills the rows y0 .. y1 of every column of
    the strip.  Returns (disp [1,1,H,W], codes (2 where a disparity was set, else 0), height (row-dependent, positive))."""
    d = np.full((1, 1, H, W), background, F)
    codes = np.zeros((1, 1, H, W), np.uint8)
    for s, spans in strips.items():
        for y0, y1, v in spans:
            d[0, 0, y0:y1 + 1, s * width:(s + 1) * width] = v
            codes[0, 0, y0:y1 + 1, s * width:(s + 1) * width] = 2
    height = np.broadcast_to((0.05 * (H - np.arange(H, dtype=F)))[None, None, :, None], d.shape).astype(F)
    return d, codes, height
