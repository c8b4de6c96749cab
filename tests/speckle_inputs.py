"""Seeded inputs of the speckle-filter tests: every generator returns float32 maps [B,1,H,W] for any H, W >= 1 (the GPU tests
use them from 8 x 1 to 368 x 1232), independent of how the kernels tile the image."""
import numpy as np

KINDS = ("plateaus", "serpentine", "spiral", "comb", "checkerboard", "constant")


def plant_specials(a, rng):
    """NaN, +inf, -inf, 0 and negative values, each on about 1 pixel in 500 (as test_gpu_lrcheck.maps plants its NaN / inf)."""
    flat = a.reshape(-1)
    idx = rng.choice(flat.size, size=min(flat.size, 5 * max(1, flat.size // 500)), replace=False)
    k = len(idx) // 5
    flat[idx[:k]] = np.nan
    flat[idx[k:2 * k]] = np.inf
    flat[idx[2 * k:3 * k]] = -np.inf
    flat[idx[3 * k:4 * k]] = 0.0
    flat[idx[4 * k:]] = -3.5
    return a


def plateaus(B, H, W, seed):
    """Piecewise-constant regions of a Voronoi-like partition; half of them with noise of amplitude 0.2 (below every max_diff > 0
    the tests use), half with amplitude 3 (above them all); islands of 1 .. 120 pixels 10 above their surroundings; specials."""
    rng = np.random.default_rng(seed)
    out = np.empty((B, 1, H, W), np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        K = 24
        cy, cx = rng.uniform(0, H, K), rng.uniform(0, W, K)
        region = np.argmin((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2, axis=0)
        level = rng.uniform(5.0, 60.0, K)
        amp = np.where(np.arange(K) % 2 == 0, 0.2, 3.0)
        d = level[region] + amp[region] * rng.uniform(-0.5, 0.5, (H, W))
        for _ in range(max(1, H * W // 1500)):              # islands: h x w rectangles of 1 .. 120 pixels, quiet inside
            h = int(rng.integers(1, 11))
            w = int(rng.integers(1, 13))
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            d[y:y + h, x:x + w] = level[region[y, x]] + 10.0 + 0.1 * rng.uniform(-0.5, 0.5, d[y:y + h, x:x + w].shape)
        out[b, 0] = plant_specials(d.astype(np.float32), rng)
    return out


def serpentine(B, H, W, seed):
    """One component that winds through the whole image: the even rows, joined alternately at the right and the left end."""
    d = np.zeros((B, 1, H, W), np.float32)
    d[:, :, 0::2, :] = 10.0
    d[:, :, 1::4, W - 1] = 10.0
    d[:, :, 3::4, 0] = 10.0
    return d


def spiral(B, H, W, seed):
    """A path of width 1 from the top-left corner inwards to the centre, a gap of one pixel between its turns."""
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True

    def free(py, px):
        return 0 <= py < H and 0 <= px < W and not m[py, px]

    turns = 0
    while turns < 2:
        ny, nx = y + dy, x + dx
        ay, ax = ny + dy, nx + dx                           # stop one short of an earlier turn of the path
        if free(ny, nx) and not (0 <= ay < H and 0 <= ax < W and m[ay, ax]):
            y, x = ny, nx
            m[y, x] = True
            turns = 0
        else:
            dy, dx = dx, -dy                                # right -> down -> left -> up
            turns += 1
    d = np.where(m, np.float32(10.0), np.float32(0.0)).astype(np.float32)
    return np.broadcast_to(d, (B, 1, H, W)).copy()


def comb(B, H, W, seed):
    """Vertical teeth (every other column) joined by the bottom row only."""
    d = np.zeros((B, 1, H, W), np.float32)
    d[:, :, :, 0::2] = 10.0
    d[:, :, H - 1, :] = 10.0
    return d


def checkerboard(B, H, W, seed):
    """Two values further apart than every max_diff of the tests: H*W components of one pixel."""
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.where((yy + xx) % 2 == 0, np.float32(10.0), np.float32(20.0)).astype(np.float32)
    return np.broadcast_to(d, (B, 1, H, W)).copy()


def constant(B, H, W, seed):
    """One component of H*W pixels."""
    return np.full((B, 1, H, W), 7.5, np.float32)


def make(kind, B, H, W, seed):
    return globals()[kind](B, H, W, seed)


def random_mask(B, H, W, seed):
    """The lws_lr_check code map: mostly 1, some 0 and 2."""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 1, 2], np.uint8), size=(B, 1, H, W), p=[0.03, 0.94, 0.03])


def edge_cases(H=70, W=135):
    """Components of 2 and 4 pixels across every possible tile border and corner, whatever the tile shape (up to 64 x 128): image
    0 holds horizontal pairs starting at every column, image 1 vertical pairs starting at every row, images 2 .. 10 blocks of
    2 x 2 pixels on a lattice of period 3 shifted by (sy, sx) in 0..2 x 0..2, so that a block's corner falls on every (y, x).
    Neighbouring components are a pixel apart and never join."""
    d = np.zeros((11, 1, H, W), np.float32)
    for j, y in enumerate(range(0, H, 2)):
        for x in range(j % 3, W - 1, 3):
            d[0, 0, y, x:x + 2] = 10.0 + (x % 7)
    for j, x in enumerate(range(0, W, 2)):
        for y in range(j % 3, H - 1, 3):
            d[1, 0, y:y + 2, x] = 10.0 + (y % 7)
    for sy in range(3):
        for sx in range(3):
            for y in range(sy, H - 1, 3):
                for x in range(sx, W - 1, 3):
                    d[2 + 3 * sy + sx, 0, y:y + 2, x:x + 2] = 10.0 + ((x + y) % 7) * 0.25
    return d
