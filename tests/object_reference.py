"""numpy restatement of lws_objects (include/lwsnet_objects.h): the occupied cells of the u-disparity image, their 8-connected
components by a flood fill of its own (in the order of the cell index c, so that the components come out by increasing root), the member pixels,
and per component the sums as Python integers, the mean disparity in Python floats (float64) and the float32 X, Y, Z one numpy
operation per step of the contract in its order.  Builds on stixel_reference.taking and ground_reference.valid_z / u16.  Written
for clarity, not speed.  Also the hand-made cell patterns the CPU and GPU tests share."""
import numpy as np

import ground_reference as G
import stixel_reference as X

F = np.float32
EMPTY_ROW = [0, -1, -1, -1, -1, -1, -1, 0]


def components(occ):
    """occ bool [S,nbins] -> (comp int64 [S,nbins]: the component of each occupied cell, numbered by increasing root, -1 elsewhere;
    the roots' (s, k)).  The root of a component is its smallest c = (nbins - 1 - k) * S + s."""
    S, nbins = occ.shape
    comp = np.full((S, nbins), -1, np.int64)
    roots = []
    for kr in range(nbins):                                 # c order: the nearest bin first, then left to right
        k = nbins - 1 - kr
        for s in np.flatnonzero(occ[:, k] & (comp[:, k] < 0)):
            if comp[s, k] >= 0:
                continue
            comp[s, k] = len(roots)
            stack = [(int(s), k)]
            while stack:
                cs, ck = stack.pop()
                for ns in range(max(cs - 1, 0), min(cs + 2, S)):
                    for nk in range(max(ck - 1, 0), min(ck + 2, nbins)):
                        if occ[ns, nk] and comp[ns, nk] < 0:
                            comp[ns, nk] = len(roots)
                            stack.append((ns, nk))
            roots.append((int(s), k))
    return comp, roots


def ordered_min(v):
    """The minimum of float32 values in the order -0.0 < +0.0."""
    m = v.min()
    return (F(-0.0) if np.signbit(v[v == 0]).any() else F(0.0)) if m == 0 else m


def ordered_max(v):
    m = v.max()
    return (F(0.0) if (~np.signbit(v[v == 0])).any() else F(-0.0)) if m == 0 else m


def objects(d, cam, codes, udisp, min_disp, max_depth, code_bits, width, sub, nbins, min_count, min_pixels, max_objects):
    """-> (rows int32 [B,max_objects,8], vals float32 [B,max_objects,8], labels int32 [B,1,H,W], info int32 [B,4]); cam float32 [B,5]."""
    d, cam, udisp = np.asarray(d, F), np.asarray(cam, F), np.asarray(udisp)
    B, _, H, W = d.shape
    S = -(-W // width)
    assert udisp.shape == (B, S, nbins)
    take, q = X.taking(d, cam, codes, min_disp, max_depth, code_bits, sub, nbins)
    _, z = G.valid_z(d, None, cam, min_disp, max_depth)
    Q = G.u16(d).astype(np.int64)
    rows = np.tile(np.array(EMPTY_ROW, np.int32), (B, max_objects, 1))
    vals = np.zeros((B, max_objects, 8), F)
    labels = np.full((B, 1, H, W), -1, np.int32)
    info = np.zeros((B, 4), np.int32)
    xi, yi = np.broadcast_to(np.arange(W)[None, :], (H, W)), np.broadcast_to(np.arange(H)[:, None], (H, W))
    for b in range(B):
        occ = udisp[b].astype(np.int64) >= min_count
        comp, roots = components(occ)
        fx, fy, cx, cy, fb = (F(v) for v in cam[b])
        with np.errstate(all="ignore"):
            Xm = ((xi.astype(F) - cx) * z[b, 0]) / fx
            Ym = ((yi.astype(F) - cy) * z[b, 0]) / fy
        of_pixel = np.where(take[b, 0], comp[xi // width, q[b, 0]], -1)     # a taking pixel in a cell that is not occupied: -1
        n_of = np.bincount(of_pixel[of_pixel >= 0], minlength=len(roots))
        kept = [i for i in range(len(roots)) if n_of[i] >= min_pixels]
        info[b] = occ.sum(), len(roots), len(kept), sum(int(n_of[i]) for i in kept)
        for j, i in enumerate(kept[:max_objects]):
            m = of_pixel == i
            labels[b, 0][m] = j
            cells_s, cells_k = np.nonzero(comp == i)
            n, sq = int(m.sum()), int(Q[b, 0][m].sum())
            rows[b, j] = n, xi[m].min(), xi[m].max(), yi[m].min(), yi[m].max(), cells_k.min(), cells_k.max(), len(cells_k)
            with np.errstate(all="ignore"):
                d_ob = F((float(sq) / float(n)) / 256.0)
                vals[b, j, :2] = d_ob, fb / d_ob
            for at, v in ((2, Xm[m]), (4, Ym[m]), (6, z[b, 0][m])):
                vals[b, j, at], vals[b, j, at + 1] = ordered_min(v), ordered_max(v)
    return rows, vals, labels, info


def cell_map(H, W, width, sub, cells, background=0.0):
    """A hand-made map for the tests: `cells` = {(strip, bin): pixels} puts that many pixels of disparity (bin + 0.5) / sub into the
    strip, row by row from the top, one cell after the other in the order of the dict.  Returns (disp [1,1,H,W], codes: 2 where a
    disparity was set, else 0)."""
    d = np.full((1, 1, H, W), background, F)
    codes = np.zeros((1, 1, H, W), np.uint8)
    used = {}
    for (s, k), count in cells.items():
        x0 = s * width
        ws = min(x0 + width, W) - x0
        i = np.arange(used.get(s, 0), used.get(s, 0) + count)
        assert ws > 0 and (i.size == 0 or i[-1] // ws < H), f"cell {(s, k)} does not fit {H} rows"
        d[0, 0, i // ws, x0 + i % ws] = F((k + 0.5) / sub)
        codes[0, 0, i // ws, x0 + i % ws] = 2
        used[s] = used.get(s, 0) + count
    return d, codes


def udisp_of(d, cam, codes, p):
    """The histogram lws_stixels writes for the map: uint32 [B,S,nbins]."""
    take, q = X.taking(d, cam, codes, p["min_disp"], p["max_depth"], p["code_bits"], p["sub"], p["nbins"])
    B, _, H, W = take.shape
    S = -(-W // p["width"])
    u = np.zeros((B, S, p["nbins"]), np.uint32)
    s_of = np.broadcast_to(np.arange(W)[None, :] // p["width"], (H, W))
    for b in range(B):
        np.add.at(u[b], (s_of[take[b, 0]], q[b, 0][take[b, 0]]), 1)
    return u


def run(d, cam, codes, udisp, p):
    return objects(d, cam, codes, udisp, p["min_disp"], p["max_depth"], p["code_bits"], p["width"], p["sub"], p["nbins"], p["min_count"],
                   p["min_pixels"], p["max_objects"])
