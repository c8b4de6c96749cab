"""lws_tsdf_window (include/lwsnet_tsdf_window.h) restated in numpy: a volume seen through an integer offset.  The rule moves bits
and compares Wt with zero, so the restatement works on the uint32 words of T and Wt and no float is ever rounded; and the volumes
the window's tests share."""
import numpy as np

F = np.float32
POISON_T = np.array([0x7FC0BEEF], np.uint32).view(F)[0]    # a NaN with a payload: what an unobserved voxel's T holds in the tests


def window(T, Wt, C, shift, dims=None):
    """T, Wt float32 [Gz,Gy,Gx], C uint8 [Gz,Gy,Gx,4] or None; shift = (sx, sy, sz); dims = (Dx, Dy, Dz), default the source's.
    -> (T2, Wt2, C2, (live, not live)): destination voxel i takes source voxel i + shift where that lies inside the source and its
    Wt is not equal to zero (NaN is not), bit for bit; everything else is +0.0 / {0, 0, 0, 0}."""
    T, Wt = np.ascontiguousarray(T, F), np.ascontiguousarray(Wt, F)
    G = T.shape[::-1]
    D = tuple(G if dims is None else dims)
    T2, Wt2 = np.zeros(D[::-1], np.uint32), np.zeros(D[::-1], np.uint32)
    C2 = None if C is None else np.zeros((*D[::-1], 4), np.uint8)
    lo = [max(0, -shift[e]) for e in range(3)]              # the destination indices whose source is inside: lo <= i < hi
    hi = [min(D[e], G[e] - shift[e]) for e in range(3)]
    live_n = 0
    if all(h > l for l, h in zip(lo, hi)):
        dst = tuple(slice(lo[e], hi[e]) for e in (2, 1, 0))
        src = tuple(slice(lo[e] + shift[e], hi[e] + shift[e]) for e in (2, 1, 0))
        with np.errstate(invalid="ignore"):
            live = ~(Wt[src] == 0)                          # -0.0 == 0: dead; NaN == 0 is false: live
        T2[dst] = np.where(live, T.view(np.uint32)[src], 0)
        Wt2[dst] = np.where(live, Wt.view(np.uint32)[src], 0)
        if C is not None:
            C2[dst] = np.where(live[..., None], np.ascontiguousarray(C)[src], 0)
        live_n = int(live.sum())
    return T2.view(F), Wt2.view(F), C2, (live_n, D[0] * D[1] * D[2] - live_n)


def window_by_voxel(T, Wt, C, shift, dims=None):
    """The same rule one voxel at a time, as the header words it: the check of window()'s slices."""
    Gz, Gy, Gx = T.shape
    Dx, Dy, Dz = (Gx, Gy, Gz) if dims is None else dims
    T2, Wt2, C2 = np.zeros((Dz, Dy, Dx), np.uint32), np.zeros((Dz, Dy, Dx), np.uint32), None if C is None else np.zeros((Dz, Dy, Dx, 4), np.uint8)
    Tb, Wb = np.ascontiguousarray(T, F).view(np.uint32), np.ascontiguousarray(Wt, F).view(np.uint32)
    n = 0
    for iz in range(Dz):
        for iy in range(Dy):
            for ix in range(Dx):
                jx, jy, jz = ix + shift[0], iy + shift[1], iz + shift[2]
                if not (0 <= jx < Gx and 0 <= jy < Gy and 0 <= jz < Gz):
                    continue
                w = Wt[jz, jy, jx]
                if w == 0:
                    continue
                n += 1
                T2[iz, iy, ix], Wt2[iz, iy, ix] = Tb[jz, jy, jx], Wb[jz, jy, jx]
                if C is not None:
                    C2[iz, iy, ix] = C[jz, jy, jx]
    return T2.view(F), Wt2.view(F), C2, (n, Dx * Dy * Dz - n)


def same_bits(a, b):
    return a is b or (a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes())


def noise_volume(dims, seed, holes=0.05, special=False):
    """T uniform noise with exact zeros, weights 1 and 2, a fraction `holes` unobserved with a poisoned T and C = 0xA5; `special`
    adds weights of NaN, +inf, -0.0 and a negative one.  vs = 0.25 and an origin in multiples of 0.25: every voxel centre is an
    exact float32, whatever integer offset the origin has moved by.  -> (T, Wt, C, origin, vs)"""
    rng = np.random.default_rng(seed)
    shape = tuple(dims)[::-1]
    Wt = rng.choice(np.array([1.0, 2.0], F), size=shape)
    Wt[rng.random(shape) < holes] = 0
    T = rng.uniform(-1, 1, shape).astype(F)
    T[rng.random(shape) < 0.05] = 0.0
    C = rng.integers(0, 256, (*shape, 4), dtype=np.uint8)
    if special:
        flat = Wt.reshape(-1)
        pick = rng.choice(flat.size, size=min(16, flat.size // 4), replace=False)
        flat[pick] = np.array([np.nan, np.inf, -0.0, -1.5], F)[np.arange(len(pick)) % 4]
    with np.errstate(invalid="ignore"):
        dead = Wt == 0
    T[dead] = POISON_T
    C[dead] = 0xA5
    return T, Wt, C, (-1.0, 0.5, 2.0), 0.25


def moved_origin(origin, shift, vs):
    """The origin of the window `shift` voxels on: exact for the volumes of noise_volume."""
    return tuple(float(F(np.float64(o) + s * np.float64(vs))) for o, s in zip(origin, shift))


def triangles(records, faces):
    """The triangles of a mesh as a sorted list of 48-byte strings, the three 16-byte vertex records of each in the face's order: a
    multiset that does not know of vertex indices."""
    rec = np.ascontiguousarray(records, np.uint8).reshape(-1, 16)
    return sorted(rec[f].tobytes() for f in np.asarray(faces).reshape(-1, 3))
