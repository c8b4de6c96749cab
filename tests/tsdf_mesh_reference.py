"""lws_tsdf_mesh (include/lwsnet_tsdf_mesh.h) restated in numpy: the case table built from the header's rule, and the mesh of a volume
with the vertices of tsdf_reference.points.  The table is built here by walking each face's corners counter-clockwise as seen from
outside the cube -- a segment starts on the edge where that walk goes from a positive corner to a non-positive one and ends on the
edge where it comes back to the same run of positive corners -- which is another way to the header's "positive corners on the
left" than the cross products of tools/make_tsdf_mesh_table.py.  Nothing here modifies its arguments."""
import numpy as np

import tsdf_reference as R

F = np.float32
AXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1))


def corner_of(k):
    return (k & 1, (k >> 1) & 1, (k >> 2) & 1)


def corner_index(c):
    return c[0] + 2 * c[1] + 4 * c[2]


def edge_between(a, b):
    """The id 4 * e + j of the edge between two neighbouring corners (given as coordinates)."""
    e = next(i for i in range(3) if a[i] != b[i])
    owner = a if a[e] == 0 else b
    j = {0: owner[1] + 2 * owner[2], 1: owner[0] + 2 * owner[2], 2: owner[0] + 2 * owner[1]}[e]
    return 4 * e + j


def edge_owner(eid):
    """-> (the owner corner's offsets (dx, dy, dz), the axis e) of edge id 4 * e + j."""
    e, j = eid >> 2, eid & 3
    lo, hi = j & 1, j >> 1
    return {0: (0, lo, hi), 1: (lo, 0, hi), 2: (lo, hi, 0)}[e], e


def edge_corners(eid):
    a, e = edge_owner(eid)
    b = tuple(a[i] + AXES[e][i] for i in range(3))
    return corner_index(a), corner_index(b)


def face_walks():
    """The six faces, each as its four corners in counter-clockwise order seen from outside the cube."""
    walks = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3               # u x v = +axis
        for side in (0, 1):
            ring = [(0, 0), (1, 0), (1, 1), (0, 1)]          # counter-clockwise seen from +axis
            if side == 0:
                ring.reverse()                              # the outside of this face is -axis
            walk = []
            for cu, cv in ring:
                c = [0, 0, 0]
                c[axis], c[u], c[v] = side, cu, cv
                walk.append(tuple(c))
            walks.append(walk)
    return walks


def face_segments(case):
    """The directed segments (from edge id, to edge id) of a case on all six faces, by the rule."""
    segments = []
    for walk in face_walks():
        pos = [bool((case >> corner_index(c)) & 1) for c in walk]
        for i in range(4):
            if pos[i] and not pos[(i + 1) % 4]:             # the walk leaves a run of positive corners: a segment starts here ...
                k = i
                while pos[(k - 1) % 4]:                     # ... and ends where the walk entered that run
                    k -= 1
                segments.append((edge_between(walk[i], walk[(i + 1) % 4]), edge_between(walk[(k - 1) % 4], walk[k % 4])))
    return segments


def triangles(case):
    follow = dict(face_segments(case))
    out, todo = [], sorted(follow)
    while todo:
        loop = [todo[0]]
        while follow[loop[-1]] != loop[0]:
            loop.append(follow[loop[-1]])
        todo = [e for e in todo if e not in loop]
        out.extend((loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1))
    return out


_TABLE = []


def table():
    """uint8 [256,32]: row c = (n, the 3n edge ids, 255 ...)."""
    if not _TABLE:
        t = np.full((256, 32), 255, np.uint8)
        for case in range(256):
            tris = triangles(case)
            t[case, 0] = len(tris)
            t[case, 1:1 + 3 * len(tris)] = [e for tri in tris for e in tri]
        t.setflags(write=False)
        _TABLE.append(t)
    return _TABLE[0]


def mesh(T, Wt, C, origin, vs, w_min=0.0):
    """-> (records uint8 [n,16], normals float32 [n,4], faces int32 [m,3]): the vertices are tsdf_reference.points in its order, the
    faces go cube by cube in raster order (z, y, x) and in the table's order inside a cube."""
    T, Wt = np.asarray(T, F), np.asarray(Wt, F)
    Gz, Gy, Gx = T.shape
    xyz, rgba, nrm, _, _ = R.points(T, Wt, C, origin, vs, w_min)
    with np.errstate(all="ignore"):
        obs = (Wt > 0) & (Wt >= F(w_min))
        pos = T > 0
        cross = np.zeros((Gz, Gy, Gx, 3), bool)             # the crossing on the edge that leaves (iz, iy, ix) towards +e
        cross[:, :, :-1, 0] = obs[:, :, :-1] & obs[:, :, 1:] & (((T[:, :, :-1] > 0) & (T[:, :, 1:] <= 0)) | ((T[:, :, :-1] <= 0) & (T[:, :, 1:] > 0)))
        cross[:, :-1, :, 1] = obs[:, :-1] & obs[:, 1:] & (((T[:, :-1] > 0) & (T[:, 1:] <= 0)) | ((T[:, :-1] <= 0) & (T[:, 1:] > 0)))
        cross[:-1, :, :, 2] = obs[:-1] & obs[1:] & (((T[:-1] > 0) & (T[1:] <= 0)) | ((T[:-1] <= 0) & (T[1:] > 0)))
    index = (np.cumsum(cross.reshape(-1)) - 1).reshape(cross.shape)      # the rank in the order (z, y, x, axis)
    assert int(cross.sum()) == len(xyz)
    ok = obs & ~np.isnan(T)
    valid = np.ones((Gz - 1, Gy - 1, Gx - 1), bool)
    case = np.zeros((Gz - 1, Gy - 1, Gx - 1), np.int64)
    for k in range(8):
        dx, dy, dz = corner_of(k)
        sl = (slice(dz, Gz - 1 + dz), slice(dy, Gy - 1 + dy), slice(dx, Gx - 1 + dx))
        valid &= ok[sl]
        case |= pos[sl].astype(np.int64) << k
    tab = table()
    faces = []
    for iz, iy, ix in zip(*np.nonzero(valid & (tab[case, 0] > 0))):
        row = tab[case[iz, iy, ix]]
        for eid in row[1:1 + 3 * row[0]]:
            (dx, dy, dz), e = edge_owner(int(eid))
            assert cross[iz + dz, iy + dy, ix + dx, e], "a valid cube's table edge is a crossing of the points"
            faces.append(index[iz + dz, iy + dy, ix + dx, e])
    return R.records(xyz, rgba), nrm, np.array(faces, np.int32).reshape(-1, 3)


def positions(records):
    """float32 [n,3] of the records' X, Y, Z."""
    return np.ascontiguousarray(records[:, :12]).view(F).reshape(-1, 3)


def directed_edges(faces):
    """{(a, b): how many faces hold the directed edge a -> b}."""
    count = {}
    for f in np.asarray(faces).reshape(-1, 3):
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            count[int(a), int(b)] = count.get((int(a), int(b)), 0) + 1
    return count


def euler(faces):
    """V - E + F over the vertices the faces use."""
    faces = np.asarray(faces).reshape(-1, 3)
    d = directed_edges(faces)
    undirected = {(min(a, b), max(a, b)) for a, b in d}
    return len(np.unique(faces)) - len(undirected) + len(faces)


def signed_volume(xyz, faces):
    p = np.asarray(xyz, np.float64)[np.asarray(faces).reshape(-1, 3)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


# ---- the analytic volumes of tests/test_tsdf_mesh_cpu.py: fully observed, T the distance to the shape in metres, vs = 0.25 ----
VS = 0.25


def lattice(dims):
    """The voxel coordinates (x [1,1,Gx], y [1,Gy,1], z [Gz,1,1]) of a volume of dims = (Gx, Gy, Gz) with its origin at 0, in voxels."""
    return (np.arange(dims[0], dtype=np.float64)[None, None, :], np.arange(dims[1], dtype=np.float64)[None, :, None],
            np.arange(dims[2], dtype=np.float64)[:, None, None])


def sphere_volume(dims=(16, 16, 16), centre=(7.3, 7.6, 7.45), radius=5.0):
    x, y, z = lattice(dims)
    T = (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius) * VS
    return T.astype(F), np.ones(dims[::-1], F)


def two_spheres_volume(dims=(24, 12, 12), centres=((5.3, 5.6, 5.45), (17.4, 5.7, 5.55)), radius=4.0):
    x, y, z = lattice(dims)
    d = [np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - radius for c in centres]
    return (np.minimum(*d) * VS).astype(F), np.ones(dims[::-1], F)


def torus_volume(dims=(20, 20, 10), centre=(9.3, 9.6, 4.45), ring=5.5, tube=2.2):
    x, y, z = lattice(dims)
    q = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2) - ring
    return ((np.sqrt(q ** 2 + (z - centre[2]) ** 2) - tube) * VS).astype(F), np.ones(dims[::-1], F)


def all_cases_volume():
    """-> T float32 [256,2,2,2]: volume c is one cube of case c, T = +-1 with no zero."""
    T = np.empty((256, 2, 2, 2), F)
    for c in range(256):
        for k in range(8):
            dx, dy, dz = corner_of(k)
            T[c, dz, dy, dx] = 1.0 if (c >> k) & 1 else -1.0
    return T
