#!/usr/bin/env python3
"""Generates mesh_to_sdf_amd/csrc/isosurface_table.h, the marching-cubes table of m2s_grid_isosurface (include/m2s.h).

Nothing is copied from an outside table: the 256 cases follow from the rule below.

Cube: corner c = 4*dx + 2*dy + dz (the bit of the case).  Local edge e = 4*a + r joins the corner at offset o and o + e_a, where
a = 0 (x): o = (0, dy, dz), r = 2*dy + dz;  a = 1 (y): o = (dx, 0, dz), r = 2*dx + dz;  a = 2 (z): o = (dx, dy, 0), r = 2*dx + dy.
1. On each of the six faces, the crossing edges (one end inside, one outside) are paired into isoline segments.  An ambiguous face
   (four crossings: the two inside corners on a diagonal) keeps its inside corners SEPARATED: each inside corner is cut off by the
   segment between its two face edges.  The pairing depends on that face's four signs only, so the two cells sharing a face agree.
2. A segment is directed so that, seen from outside the cube, the inside corners lie on its right.  The neighbour sees the face from
   the other side, so it directs the same segment the other way: the mesh is closed across cells.
3. Every crossing edge lies on two faces and ends one segment on one and starts one on the other, so the segments of a cell form
   disjoint closed loops.  Each loop is rotated to start at its lowest edge id and fanned: (l0, l_i, l_i+1).  Loops are emitted in
   order of their lowest edge id.  The right-hand normal of a triangle then points from inside to outside (checked below).

Usage: python tools/gen_isosurface_table.py [--check]   (--check: exit 1 if the committed header differs)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mesh_to_sdf_amd", "csrc", "isosurface_table.h")


def corner(dx, dy, dz):
    return 4 * dx + 2 * dy + dz


def corner_pos(c):
    return ((c >> 2) & 1, (c >> 1) & 1, c & 1)


def _edges():
    out = []
    for a in range(3):
        for r in range(4):
            hi, lo = (r >> 1) & 1, r & 1
            o = [0, 0, 0]
            others = [k for k in range(3) if k != a]
            o[others[0]], o[others[1]] = hi, lo
            out.append((tuple(o), a))
    return out


EDGES = _edges()   # local edge id -> (offset of its lower corner, axis)


def edge_corners(e):
    o, a = EDGES[e]
    p = list(o)
    p[a] = 1
    return corner(*o), corner(*p)


def edge_mid(e):
    o, a = EDGES[e]
    return tuple(o[k] + (0.5 if k == a else 0.0) for k in range(3))


# faces: (axis f, side s): the corners with coordinate f == s; its edges run along the other two axes
FACES = [(f, s) for f in range(3) for s in range(2)]


def face_corners(face):
    f, s = face
    return [c for c in range(8) if corner_pos(c)[f] == s]


def face_edges(face):
    f, s = face
    return [e for e in range(12) if EDGES[e][1] != f and EDGES[e][0][f] == s]


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _sub(u, v):
    return tuple(a - b for a, b in zip(u, v))


def _dot(u, v):
    return sum(a * b for a, b in zip(u, v))


def _directed(face, ea, eb, inside_corner):
    """(ea, eb) or (eb, ea): the direction with `inside_corner` on the right, seen from outside the cube."""
    f, s = face
    n = [0, 0, 0]
    n[f] = 1 if s else -1
    ma, mb = edge_mid(ea), edge_mid(eb)
    side = _dot(_cross(tuple(n), _sub(mb, ma)), _sub(corner_pos(inside_corner), ma))
    assert side != 0
    return (ea, eb) if side < 0 else (eb, ea)


def face_segments(case, face):
    """The directed segments (edge, edge) of one face of a cell with this case: depends on the face's four signs only."""
    inside = lambda c: (case >> c) & 1
    cs = face_corners(face)
    crossing = [e for e in face_edges(face) if inside(edge_corners(e)[0]) != inside(edge_corners(e)[1])]
    ins = [c for c in cs if inside(c)]
    if not crossing:
        return []
    if len(crossing) == 2:
        return [_directed(face, crossing[0], crossing[1], ins[0])]
    assert len(crossing) == 4 and len(ins) == 2
    segs = []
    for c in ins:   # separated: each inside corner is cut off by its own segment
        es = [e for e in crossing if c in edge_corners(e)]
        segs.append(_directed(face, es[0], es[1], c))
    return segs


def loops(case):
    nxt = {}
    for face in FACES:
        for a, b in face_segments(case, face):
            assert a not in nxt, (case, a)
            nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values())   # every crossing edge starts one segment and ends one
    out, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        out.append(loop)   # started at its lowest id, since starts are visited in ascending order
    return out


def triangles(case):
    tris = []
    for loop in loops(case):
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


TABLE = [triangles(c) for c in range(256)]
MAX_TRIS = max(len(t) for t in TABLE)


def _check_orientation():
    # one inside corner (corner 0): the triangle's normal must point away from it, towards the outside
    (t,) = TABLE[1]
    p = [edge_mid(e) for e in t]
    n = _cross(_sub(p[1], p[0]), _sub(p[2], p[0]))
    assert all(x > 0 for x in n), n


_check_orientation()


def render():
    lines = [
        "// isosurface_table.h — GENERATED by tools/gen_isosurface_table.py; do not edit.  The rule is stated there and in include/m2s.h.",
        "// Corner c = 4*dx + 2*dy + dz; case bit c set = that corner is inside (d < iso).",
        "// Local edge e = 4*a + r along axis a from the corner at kIsoEdgeOffset[e] (dx, dy, dz).",
        "// kIsoTris[case]: kIsoTriCount[case] triangles of three local edges, in emission order; unused slots are -1.",
        "// M2S_ISO_TABLE qualifies the arrays (isosurface.hip: __constant__); plain `static const` by default.",
        "#pragma once",
        "#include <stdint.h>",
        "",
        "#ifndef M2S_ISO_TABLE",
        "#define M2S_ISO_TABLE static const",
        "#endif",
        "",
        f"#define M2S_ISO_MAX_TRIS {MAX_TRIS}   /* the most triangles any cell emits */",
        "",
        "M2S_ISO_TABLE uint8_t kIsoEdgeOffset[12][3] = {",
    ]
    lines += ["  {%d, %d, %d},   // e%d, axis %d" % (o[0], o[1], o[2], e, a) for e, (o, a) in enumerate(EDGES)]
    lines += ["};", "", "M2S_ISO_TABLE uint8_t kIsoTriCount[256] = {"]
    for r in range(0, 256, 32):
        lines.append("  " + ", ".join(str(len(TABLE[c])) for c in range(r, r + 32)) + ",")
    lines += ["};", "", f"M2S_ISO_TABLE int8_t kIsoTris[256][{3 * MAX_TRIS}] = {{"]
    for c in range(256):
        flat = [e for t in TABLE[c] for e in t]
        flat += [-1] * (3 * MAX_TRIS - len(flat))
        lines.append("  {" + ", ".join(str(v) for v in flat) + "},   // %d" % c)
    lines += ["};", ""]
    return "\n".join(lines)


def main(argv):
    text = render()
    if "--check" in argv:
        with open(HEADER) as f:
            return 0 if f.read() == text else 1
    with open(HEADER, "w") as f:
        f.write(text)
    print(f"wrote {HEADER}: max {MAX_TRIS} triangles per cell")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
