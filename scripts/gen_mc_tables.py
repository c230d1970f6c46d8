#!/usr/bin/env python3
"""Generator of ``intrinsicnerf_amd/csrc/mc_tables.h``: the marching-cubes case table of inerf_mc_count / inerf_mc_emit.

The table is derived, not remembered.  Numbering:
  corner  c = di | dj << 1 | dk << 2            the lattice point (i + di, j + dj, k + dk) of cube (i, j, k)
  edge    e = 4 * axis + rank                   axis 0 = i, 1 = j, 2 = k; rank = the position of the edge's low corner among the four
                                                corners whose offset along ``axis`` is 0, in ascending corner number
  case    bit c set  <=>  occ[corner c] > level (a NaN is outside)
Rule per case:
  * on each of the six faces, marching squares on the face's four corner states alone;
  * a face with two diagonal inside corners cuts each of them off on its own - a function of the face alone, so the two cubes that
    share a face draw the same segments on it;
  * every segment is directed so that the inside corners lie on its RIGHT seen from outside the cube (on its left seen from within);
    the two cubes that share a face see it from opposite sides, so they direct its segments oppositely;
  * the directed segments chain into closed loops (every active edge has one incoming and one outgoing segment);
  * every loop is fan-triangulated in the loop's direction, from its lowest-numbered edge among those from which no diagonal of the
    fan joins two edges of one cube face (such a diagonal lies in that face, where the neighbouring cube may draw it too: four
    triangles would meet in one mesh edge; the plain "lowest edge" fan does that on 38 edges of a 16^3 noise field).  Every loop
    has such an edge (asserted).
With this direction the geometric normal (b - a) x (c - a) of every triangle points towards the outside corners, that is towards
lower values: outward for an occupancy (asserted below on the cases with one inside corner).

``python scripts/gen_mc_tables.py`` prints the header; ``--write`` replaces the committed file; ``--check`` compares.
"""
import os
import sys

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "intrinsicnerf_amd", "csrc", "mc_tables.h")


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def corner_of(offset):
    return offset[0] | offset[1] << 1 | offset[2] << 2


def edge_list():
    """[(axis, low corner, high corner)] in edge order"""
    edges = []
    for axis in range(3):
        for c in range(8):
            if corner_offset(c)[axis] == 0:
                edges.append((axis, c, c | 1 << axis))
    return edges


EDGES = edge_list()
EDGE_OF = {frozenset((lo, hi)): e for e, (_, lo, hi) in enumerate(EDGES)}


def faces():
    """[(axis, side, [four corners, counter-clockwise seen from outside the cube])]"""
    out = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3              # (axis, u, v) is a right-handed triple
        for side in (0, 1):
            ring = []
            for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):    # counter-clockwise seen from +axis
                off = [0, 0, 0]
                off[axis], off[u], off[v] = side, du, dv
                ring.append(corner_of(off))
            if side == 0:                                      # outside is -axis: the other way round
                ring.reverse()
            out.append((axis, side, ring))
    return out


FACES = faces()


def face_segments(case, ring):
    """directed segments (edge from, edge to) of marching squares on one face: per maximal run of inside corners p_a .. p_b of the
    counter-clockwise ring, from the crossing before p_a to the crossing after p_b (the run lies on the right, seen from outside)"""
    inside = [bool(case >> c & 1) for c in ring]
    if all(inside) or not any(inside):
        return []
    segs = []
    for a in range(4):
        if inside[a] and not inside[a - 1]:
            b = a
            while inside[(b + 1) % 4]:
                b += 1
            first = EDGE_OF[frozenset((ring[a - 1], ring[a]))]
            last = EDGE_OF[frozenset((ring[b % 4], ring[(b + 1) % 4]))]
            segs.append((first, last))
    return segs


def case_loops(case):
    nxt = {}
    for _, _, ring in FACES:
        for a, b in face_segments(case, ring):
            assert a not in nxt, (case, a)
            nxt[a] = b
    active = {e for e, (_, lo, hi) in enumerate(EDGES) if (case >> lo & 1) != (case >> hi & 1)}
    assert set(nxt) == active and set(nxt.values()) == active, case
    loops, seen = [], set()
    for start in sorted(active):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3, (case, loop)
        loops.append(loop)                                     # starts at its lowest-numbered edge: ``start`` ascends
    return loops


def edge_faces(e):
    """the two cube faces (axis, side) edge e lies in"""
    axis, lo, _ = EDGES[e]
    return {(a, (lo >> a) & 1) for a in range(3) if a != axis}


def fan(loop):
    """the fan of a loop that no diagonal of which lies in a face of the cube: from the lowest-numbered edge that allows it.  (A
    diagonal between two edges of one face would lie IN that face; the cube beyond the face may draw the same diagonal, and the mesh
    edge would then carry four triangles.  Diagonals through the cube's interior belong to this cube alone.)"""
    n = len(loop)
    for apex in sorted(loop):
        at = loop.index(apex)
        rot = loop[at:] + loop[:at]                            # the loop's direction is kept
        if all(not (edge_faces(rot[0]) & edge_faces(rot[k])) for k in range(2, n - 1)):
            return [(rot[0], rot[k], rot[k + 1]) for k in range(1, n - 1)]
    raise AssertionError(f"no fan of {loop} stays out of the cube's faces")


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        tris += fan(loop)
    return tris


def midpoint(e):
    _, lo, hi = EDGES[e]
    a, b = corner_offset(lo), corner_offset(hi)
    return tuple((x + y) / 2.0 for x, y in zip(a, b))


def build():
    table = [case_triangles(case) for case in range(256)]
    # the winding: with one inside corner the triangle's normal points away from that corner
    for c in range(8):
        (t,) = table[1 << c]
        a, b, d = (midpoint(e) for e in t)
        u, v = [b[i] - a[i] for i in range(3)], [d[i] - a[i] for i in range(3)]
        n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
        cen = [(a[i] + b[i] + d[i]) / 3.0 - corner_offset(c)[i] for i in range(3)]
        assert sum(n[i] * cen[i] for i in range(3)) > 0, c
    max_tris = max(len(t) for t in table)
    max_edge_tris = max(sum(e in t for t in tris) for tris in table for e in range(12))
    return table, max_tris, max_edge_tris


def render():
    table, max_tris, max_edge_tris = build()
    lines = [
        "// mc_tables.h - the marching-cubes case table of mcubes.hip.  GENERATED by scripts/gen_mc_tables.py: do not edit; the rule",
        "// (marching squares per face, diagonal inside corners cut off separately, loops fanned without a diagonal in a cube face) is stated there.",
        "//   corner c = di | dj << 1 | dk << 2;  edge e = 4 * axis + rank of its low corner;  case bit c <=> occ[corner c] > level.",
        "// kMcTriangles[case] holds kMcCount[case] triangles of three edge numbers each, normals towards the lower values.",
        "#pragma once",
        "",
        "#if defined(__HIPCC__)",
        "#define INERF_MC_TABLE __device__ constexpr          // indexed at run time inside the kernels",
        "#else",
        "#define INERF_MC_TABLE constexpr",
        "#endif",
        "",
        "namespace inerf {",
        "",
        f"constexpr int kMcMaxTriangles = {max_tris};          // most triangles of one cube",
        f"constexpr int kMcMaxEdgeTriangles = {max_edge_tris};      // most triangles of one cube that meet at one of its edges",
        "",
        "// low corner of edge e, and its axis is e / 4",
        "INERF_MC_TABLE unsigned char kMcEdgeCorner[12] = {" + ", ".join(str(lo) for _, lo, _ in EDGES) + "};",
        "",
        "INERF_MC_TABLE unsigned char kMcCount[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(table[c])) for c in range(r, r + 32)) + ",")
    lines += ["};", "", f"INERF_MC_TABLE unsigned char kMcTriangles[256][{3 * max_tris}] = {{"]
    for case, tris in enumerate(table):
        flat = [e for t in tris for e in t]
        flat += [0] * (3 * max_tris - len(flat))
        lines.append("    {" + ", ".join(f"{e:2d}" for e in flat) + "},   // %3d" % case)
    lines += ["};", "", "}  // namespace inerf", ""]
    return "\n".join(lines), max_tris, max_edge_tris


def main(argv):
    text, max_tris, max_edge_tris = render()
    if "--write" in argv:
        with open(HEADER, "w") as fh:
            fh.write(text)
    elif "--check" in argv:
        with open(HEADER) as fh:
            if fh.read() != text:
                print("mc_tables.h differs from what this generator writes", file=sys.stderr)
                return 1
    else:
        sys.stdout.write(text)
    print(f"max triangles per cube: {max_tris}; max triangles at one edge of one cube: {max_edge_tris}", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
