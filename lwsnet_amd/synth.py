"""Seeded synthetic stereo pairs (numpy only; no datasets travel to the GPU box).

``make_pair`` builds a band-limited left image, a smooth ground-truth disparity
field inside 0..192 px, and the right image as the left one resampled along x,
then normalises both like the reference input pipeline
(/root/reference/inference.py:83-85,102-103; dataloader/dataloader.py:10-11).
``make_noise_pair`` is the adversarial-numerics case (white noise).
"""
from __future__ import annotations

import numpy as np

IMAGENET_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
IMAGENET_STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def check_size(H, W, maxdisp0=24):
    """Sizes the network accepts: the 2D hourglass skip-adds
    (/root/reference/models/submodules.py:103,182) need ceil(H/2), ceil(W/2)
    divisible by 4 (so H = 8k or 8k-1: the stem convolution, submodules.py:118-125,
    gives ceil(H/2)), and the stage-1 volume (models/models.py:72) needs the 1/8 map
    to be at least maxdisplist[0] wide."""
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    if H <= 0 or W <= 0 or h2 % 4 or w2 % 4:
        raise ValueError(f"unsupported input size {H}x{W}: ceil(H/2) and ceil(W/2) must be divisible by 4")
    if w2 // 4 < maxdisp0:
        raise ValueError(f"unsupported input size {H}x{W}: the 1/8 map is {w2 // 4} wide, must be >= maxdisplist[0]={maxdisp0}")


def _box_blur(a, k=9):
    """Separable k x k box blur with edge replication, float64, along the last two axes."""
    r = k // 2
    for axis in (-1, -2):
        pad = [(0, 0)] * a.ndim
        pad[axis] = (r, r)
        p = np.pad(a, pad, mode="edge")
        c = np.cumsum(p, axis=axis)
        z = np.zeros_like(np.take(c, [0], axis=axis))
        c = np.concatenate([z, c], axis=axis)
        n = a.shape[axis]
        hi = np.take(c, np.arange(k, k + n), axis=axis)
        lo = np.take(c, np.arange(0, n), axis=axis)
        a = (hi - lo) / k
    return a


def gt_disparity(H, W):
    y = np.arange(H, dtype=np.float64)[:, None]
    x = np.arange(W, dtype=np.float64)[None, :]
    return 10.0 + 60.0 * y / H + 6.0 * np.sin(2.0 * np.pi * x / W * 3.0)


def _normalise(img01):
    return ((img01.astype(np.float32) - IMAGENET_MEAN[:, None, None]) / IMAGENET_STD[:, None, None]).astype(np.float32)


def make_pair(H, W, index=0):
    """Returns (left, right, gt) float32: [3,H,W], [3,H,W], [H,W]."""
    rng = np.random.default_rng(1234 + int(index))
    f = rng.random((3, H, W))
    f = _box_blur(_box_blur(f))
    lo, hi = f.min(), f.max()
    left = (f - lo) / (hi - lo)
    g = gt_disparity(H, W)
    xs = np.arange(W, dtype=np.float64)[None, :] - g          # sample left at x - g
    x0 = np.floor(xs)
    lam = xs - x0
    x0 = x0.astype(np.int64)
    x1 = x0 + 1
    rows = np.arange(H)[:, None]

    def tap(xi):
        ok = (xi >= 0) & (xi < W)
        v = left[:, rows, np.clip(xi, 0, W - 1)]
        return np.where(ok[None], v, 0.0)

    right = tap(x0) * (1.0 - lam)[None] + tap(x1) * lam[None]
    return (np.ascontiguousarray(_normalise(left)), np.ascontiguousarray(_normalise(right)),
            np.ascontiguousarray(g, dtype=np.float32))


def make_noise_pair(H, W, index=0):
    rng = np.random.default_rng(4321 + int(index))
    left = rng.standard_normal((3, H, W)).astype(np.float32)
    right = rng.standard_normal((3, H, W)).astype(np.float32)
    return left, right


def make_batch(B, H, W, first_index=0):
    """[B,3,H,W] left/right float32 batches of seeded synthetic pairs."""
    ls, rs = [], []
    for i in range(B):
        l, r, _ = make_pair(H, W, first_index + i)
        ls.append(l)
        rs.append(r)
    return np.ascontiguousarray(np.stack(ls)), np.ascontiguousarray(np.stack(rs))


def to_rgb8(img):
    """Inverse of the normalisation: [3,H,W] normalised float32 -> [H,W,3] uint8 RGB (rounded, clipped)."""
    x = img.astype(np.float64) * IMAGENET_STD[:, None, None] + IMAGENET_MEAN[:, None, None]
    return np.ascontiguousarray(np.clip(np.rint(x * 255.0), 0, 255).astype(np.uint8).transpose(1, 2, 0))


def write_kitti_tree(root, n, H=375, W=1242):
    """A miniature KITTI 2015 training tree (image_2/, image_3/, disp_occ_0/ with n `*_10.png` frames; ground truth as 16-bit
    PNG x 256, 0 = no measurement in the top rows) and its split file root/val_set.txt listing all n frames.  Returns the split path."""
    import os

    from PIL import Image
    for d in ("image_2", "image_3", "disp_occ_0"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for i in range(n):
        left, right, gt = make_pair(H, W, i)
        name = f"{i:06d}_10.png"
        Image.fromarray(to_rgb8(left)).save(os.path.join(root, "image_2", name))
        Image.fromarray(to_rgb8(right)).save(os.path.join(root, "image_3", name))
        g16 = np.rint(gt.astype(np.float64) * 256).astype(np.uint16)
        g16[: H // 3] = 0                                    # KITTI's sparse ground truth: no value in the sky
        Image.fromarray(g16).save(os.path.join(root, "disp_occ_0", name))
    split = os.path.join(root, "val_set.txt")
    with open(split, "w") as f:
        f.write("".join(f"{i}\n" for i in range(n)))
    return split


def write_sceneflow_tree(root, n, H=540, W=960):
    """A miniature SceneFlow tree in the layout lwsnet_amd.datasets.sceneflow_lists reads: n flyingthings3d TEST frames of H x W
    (clean pass PNGs, ground truth PFM), empty monkaa / TRAIN / driving folders."""
    import os

    from PIL import Image

    def mk(*p):
        os.makedirs(os.path.join(root, *p), exist_ok=True)
        return os.path.join(root, *p)

    mk("monkaa_frames_cleanpass")
    mk("monkaa_disparity")
    for part in ("A", "B", "C"):
        mk("frames_cleanpass", "TRAIN", part)
        mk("frames_cleanpass", "TEST", part)
        mk("frames_disparity", "TEST", part)
    for direction in ("scene_backwards", "scene_forwards"):
        for speed in ("fast", "slow"):
            mk("driving_frames_cleanpass", "15mm_focallength", direction, speed, "left")
            mk("driving_disparity", "15mm_focallength", direction, speed, "left")
    for i in range(n):
        left, right, gt = make_pair(H, W, 100 + i)
        seq = f"{i:04d}"
        Image.fromarray(to_rgb8(left)).save(os.path.join(mk("frames_cleanpass", "TEST", "A", seq, "left"), "0006.png"))
        Image.fromarray(to_rgb8(right)).save(os.path.join(mk("frames_cleanpass", "TEST", "A", seq, "right"), "0006.png"))
        gt = gt.copy()
        gt[:, : W // 8] += 200.0                             # a band outside gt < maxdisp
        with open(os.path.join(mk("frames_disparity", "TEST", "A", seq, "left"), "0006.pfm"), "wb") as f:
            f.write(b"Pf\n" + f"{W} {H}\n".encode() + b"-1.0\n")
            f.write(np.flipud(gt).astype("<f4").tobytes())
