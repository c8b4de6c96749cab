"""Restatement of lws_stage_metrics (include/lwsnet_hip.h) in numpy that keeps the ORDER of the float64 additions the header of
lwsnet_amd/csrc/lws_metrics.hip promises, so that abs_sum can be compared bit for bit (a sum in any other order passes a relative
tolerance and says nothing about the order):
  1. a workgroup owns 1024 consecutive quads (4096 pixels) of an image; its thread t adds the e of its quads t, t + 256, t + 512,
     t + 768 in that order, the pixels of a quad as x, y, z, w, starting from 0.0
  2. a wave's 64 sums go through the shuffle tree o = 32, 16, .., 1 (lane l takes lane l + o's value): lane 0 holds the result
  3. the four waves combine as (w0 + w1) + (w2 + w3): one partial per workgroup
  4. the second launch: thread t adds the partials t, t + 256, ... of the image in that order, starting from 0.0; then 2. and 3.
For finite inputs only: an invalid pixel is restated as the addition of +0.0, which leaves a sum of non-negative terms as it is.
Used by tests/test_gpu_evaluate.py."""
import numpy as np

THREADS = 256
STEPS = 4
PIXELS_PER_BLOCK = 4 * THREADS * STEPS


def _wave_tree(v):
    """[..., 64] -> [...]: what lane 0 holds after v += shfl_down(v, o) for o = 32 .. 1."""
    o = 32
    while o > 0:
        v = v[..., :o] + v[..., o:2 * o]
        o >>= 1
    return v[..., 0]


def _block_tree(v):
    """[..., 256] per-thread sums -> [...]: the wave trees, then (w0 + w1) + (w2 + w3)."""
    w = _wave_tree(v.reshape(v.shape[:-1] + (THREADS // 64, 64)))
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def ordered_sum(terms):
    """The float64 sum of one image's per-pixel terms (flat, raster order, 0.0 where the pixel is not valid) in the kernel's order."""
    terms = np.asarray(terms, np.float64).reshape(-1)
    nblk = -(-terms.size // PIXELS_PER_BLOCK)
    a = np.zeros(nblk * PIXELS_PER_BLOCK, np.float64)
    a[:terms.size] = terms
    a = a.reshape(nblk, STEPS, THREADS, 4)                   # pixel 4 * (j * 1024 + k * 256 + t) + c
    acc = np.zeros((nblk, THREADS), np.float64)
    for k in range(STEPS):
        for c in range(4):
            acc = acc + a[:, k, :, c]
    part = _block_tree(acc)                                 # [nblk]
    rounds = -(-nblk // THREADS)
    p = np.zeros(rounds * THREADS, np.float64)
    p[:nblk] = part
    p = p.reshape(rounds, THREADS)
    acc = np.zeros(THREADS, np.float64)
    for r in range(rounds):
        acc = acc + p[r]
    return _block_tree(acc)


def stage_metrics(preds, gt, row_offset, maxdisp, mode):
    """counts [4,B,2] int64 = {valid, bad} and abs_sum [4,B] float64 of lws_stage_metrics: every per-pixel step one float32 numpy
    operation, abs_sum added in the kernel's order.  preds: four [B,1,Hg + row_offset,W] float32 arrays, gt [B,Hg,W] float32."""
    B = gt.shape[0]
    counts = np.zeros((4, B, 2), np.int64)
    sums = np.zeros((4, B), np.float64)
    md = np.float32(maxdisp)
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in range(4):
            for b in range(B):
                g = gt[b]
                e = np.abs(preds[s][b, 0, row_offset:] - g)
                assert e.dtype == np.float32 and np.isfinite(e).all() and np.isfinite(g).all()
                valid = (g < md) & ((g > np.float32(0)) if mode == 0 else True)
                bad = valid & (e > np.float32(3.0)) & (e / g > np.float32(0.05))
                counts[s, b] = valid.sum(), bad.sum()
                sums[s, b] = ordered_sum(np.where(valid, e, np.float32(0)))
    return counts, sums
