#!/usr/bin/env python3
"""Prints the marching-cubes case table of lws_tsdf_mesh (include/lwsnet_tsdf_mesh.h states the rule) as the rows of
lwsnet_amd/csrc/lws_tsdf_mesh_table.h.

    python tools/make_tsdf_mesh_table.py > lwsnet_amd/csrc/lws_tsdf_mesh_table.h
    python tools/make_tsdf_mesh_table.py --max          # LWS_TSDF_MESH_MAX_TRIS

The table is made by construction, with vectors: corner k = dx + 2 * dy + 4 * dz of the unit cube is positive where bit k of the case
is set; an edge leaves its owner corner towards +e and has the id 4 * e + j; on each of the six faces the crossing edges are joined
by segments between their midpoints, two crossings by one segment, four by two segments that each cut off one positive corner; a
segment from p to q on a face with the outward normal n is directed so that n x (q - p) points to its positive corner; the directed
segments close into loops, a loop starts at its smallest edge id and is fanned from there, the loops of a case in the order of their
smallest edge ids.  Row c: byte 0 the number of triangles, then three edge ids per triangle, then 255 up to 32 bytes.
tests/tsdf_mesh_reference.py builds the same table another way, and tests/test_tsdf_mesh_cpu.py holds both to the rule's properties."""
import sys

import numpy as np


def corner(k):
    return np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1])


def edge_id(owner, e):
    j = [owner[i] for i in range(3) if i != e]
    return 4 * e + int(j[0]) + 2 * int(j[1])


def face_segments(case, axis, side):
    """The directed segments (from edge id, to edge id) of the face `axis` = `side`."""
    n = np.zeros(3)
    n[axis] = 1.0 if side else -1.0
    corners = [k for k in range(8) if corner(k)[axis] == side]
    pos = {k: bool((case >> k) & 1) for k in corners}
    crossing = {}                                           # edge id -> (midpoint, its two corners)
    for a in corners:
        for b in corners:
            d = corner(b) - corner(a)
            if d.sum() == 1 and np.abs(d).sum() == 1 and pos[a] != pos[b]:      # b = a + one axis
                crossing[edge_id(corner(a), int(np.argmax(d)))] = (corner(a) + 0.5 * d, (a, b))
    def directed(e0, e1, c):
        p, q = crossing[e0][0], crossing[e1][0]
        return (e0, e1) if np.dot(np.cross(n, q - p), corner(c) - p) > 0 else (e1, e0)
    if len(crossing) == 2:
        e0, e1 = sorted(crossing)
        return [directed(e0, e1, next(k for k in corners if pos[k]))]
    segments = []
    if len(crossing) == 4:
        for c in corners:
            if pos[c]:
                e0, e1 = sorted(e for e, (_, ends) in crossing.items() if c in ends)
                segments.append(directed(e0, e1, c))
    return segments


def case_triangles(case):
    nxt = {}
    for axis in range(3):
        for side in (0, 1):
            for e0, e1 in face_segments(case, axis, side):
                assert e0 not in nxt
                nxt[e0] = e1
    assert sorted(nxt) == sorted(nxt.values())
    tris, left = [], set(nxt)
    while left:
        loop = [min(left)]
        while nxt[loop[-1]] != loop[0]:
            loop.append(nxt[loop[-1]])
        left -= set(loop)
        tris += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    return tris


def table():
    rows = np.full((256, 32), 255, np.uint8)
    for case in range(256):
        tris = case_triangles(case)
        rows[case, 0] = len(tris)
        rows[case, 1:1 + 3 * len(tris)] = np.array(tris, np.uint8).reshape(-1)
    return rows


def main():
    rows = table()
    if "--max" in sys.argv:
        print(int(rows[:, 0].max()))
        return
    print("// The case table of lws_tsdf_mesh, [256][32] bytes: printed by tools/make_tsdf_mesh_table.py, not edited by hand.")
    print("// Row c: the triangles of case c, three edge ids each, 255 behind them.")
    for case in range(256):
        print("{" + ", ".join(f"{v:3d}" for v in rows[case]) + "},")


if __name__ == "__main__":
    main()
