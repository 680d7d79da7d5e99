"""Generate the marching-cubes tables of myslam_amd/csrc/eslam_mc_tables.h from one face rule.

    python tools/gen_mc_tables.py            # rewrites the header
    python tools/gen_mc_tables.py --check    # exit 1 if the committed header differs

Cube conventions (shared with eslam_mesh.hip and tests/mesh_ref.py):
  corner k sits at (k & 1, (k >> 1) & 1, (k >> 2) & 1) in (x, y, z); bit k of the case index is set when corner k's
  value is below the level.  Edge e = 4 * axis + j runs along `axis` (0 x, 1 y, 2 z) from its lower corner, whose two
  other coordinates are (j & 1, j >> 1) in axis order (x-edges: (y, z); y-edges: (x, z); z-edges: (x, y)).

Face rule: on each of the six faces the crossing edges (one end below, one not) are joined by segments.  Two crossings
give one segment.  Four crossings (the two below corners are diagonal) give two segments, each cutting off one below
corner.  A face is shared by two cubes that see the same four corner values, so both emit the same segments: the mesh
has no cracks.  Every segment (from, to) is oriented so that (to - from) x n, n the face's outward normal, points toward
the below corners it cuts off; each crossing edge then starts one segment and ends another, the segments chain into
closed polygons, and each polygon is fan-triangulated from its first vertex.  Triangles (v0, v1, v2) then have (v1 - v0) x (v2 - v0) pointing
away from the below corners.
"""
import os
import sys

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "myslam_amd", "csrc", "eslam_mc_tables.h")


def corner_pos(k):
    return np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1], dtype=np.int64)


def edge_ends(e):
    """(lower corner, upper corner) of edge e."""
    axis, j = divmod(e, 4)
    other = [a for a in range(3) if a != axis]
    lo = np.zeros(3, dtype=np.int64)
    lo[other[0]] = j & 1
    lo[other[1]] = j >> 1
    hi = lo.copy()
    hi[axis] = 1
    idx = lambda p: int(p[0] + 2 * p[1] + 4 * p[2])
    return idx(lo), idx(hi)


EDGES = [edge_ends(e) for e in range(12)]


def edge_mid(e):
    a, b = EDGES[e]
    return (corner_pos(a) + corner_pos(b)) / 2.0


def edge_of(c0, c1):
    for e, (a, b) in enumerate(EDGES):
        if {a, b} == {c0, c1}:
            return e
    raise KeyError((c0, c1))


def faces():
    """The six faces: (outward normal, corners in cyclic order)."""
    out = []
    for axis in range(3):
        for side in (0, 1):
            n = np.zeros(3)
            n[axis] = 1.0 if side else -1.0
            cs = [k for k in range(8) if corner_pos(k)[axis] == side]
            # cyclic order: sort by angle around the face centre
            ctr = np.mean([corner_pos(k) for k in cs], axis=0)
            u, v = [a for a in range(3) if a != axis]
            cs.sort(key=lambda k: np.arctan2(corner_pos(k)[v] - ctr[v], corner_pos(k)[u] - ctr[u]))
            out.append((n, cs))
    return out


FACES = faces()


def face_segments(case, face):
    """Oriented segments (edge_from, edge_to) the face rule puts on one face of a cube of this case."""
    n, cs = face
    below = [(case >> k) & 1 for k in cs]
    ring = [edge_of(cs[i], cs[(i + 1) % 4]) for i in range(4)]          # ring[i] joins cs[i] and cs[i+1]
    crossing = [below[i] != below[(i + 1) % 4] for i in range(4)]
    segs = []
    if sum(crossing) == 2:
        a, b = [ring[i] for i in range(4) if crossing[i]]
        segs.append((a, b, [cs[i] for i in range(4) if below[i]]))
    elif sum(crossing) == 4:
        for i in range(4):
            if below[i]:       # cut off below corner cs[i]: its two ring edges are ring[i - 1] and ring[i]
                segs.append((ring[(i - 1) % 4], ring[i], [cs[i]]))
    out = []
    for a, b, cut in segs:
        pa, pb = edge_mid(a), edge_mid(b)
        m = (pa + pb) / 2.0
        side = np.dot(np.cross(pb - pa, n), np.mean([corner_pos(k) for k in cut], axis=0) - m)
        assert abs(side) > 1e-9
        out.append((a, b) if side > 0 else (b, a))
    return out


def case_polygons(case):
    nxt = {}
    for f in FACES:
        for a, b in face_segments(case, f):
            assert a not in nxt, (case, a)
            nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), case          # every crossing edge starts one segment and ends one
    polys, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        poly, e = [], start
        while e not in seen:
            seen.add(e)
            poly.append(e)
            e = nxt[e]
        assert e == start
        polys.append(poly)
    return polys


def case_triangles(case):
    tris = []
    for poly in case_polygons(case):
        for k in range(1, len(poly) - 1):
            tris.append((poly[0], poly[k], poly[k + 1]))
    return tris


def build_tables():
    tris = [case_triangles(c) for c in range(256)]
    return tris, max(len(t) for t in tris)


def render_header():
    tris, max_tris = build_tables()
    lines = [
        "// Generated by tools/gen_mc_tables.py - do not edit.  Marching-cubes tables derived from one face rule (see there).",
        "// corner k = (k & 1, (k >> 1) & 1, (k >> 2) & 1); case bit k set when corner k < level;",
        "// edge e = 4 * axis + j from its lower corner, whose other two coordinates are (j & 1, j >> 1) in axis order.",
        "// MC_TABLE: the storage of the tables; a device translation unit defines it as `__constant__ static const`.",
        "#pragma once",
        "",
        "#ifndef MC_TABLE",
        "#define MC_TABLE static const",
        "#endif",
        f"#define MC_MAX_TRIS {max_tris}",
        "",
        "// triangles of each case",
        "MC_TABLE unsigned char MC_NTRI[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(tris[c])) for c in range(r, r + 32)) + ",")
    lines.append("};")
    lines.append("")
    lines.append("// the edges of each triangle, in table order (unused entries -1)")
    lines.append("MC_TABLE signed char MC_TRI[256][3 * MC_MAX_TRIS] = {")
    for c in range(256):
        flat = [e for t in tris[c] for e in t] + [-1] * (3 * (max_tris - len(tris[c])))
        lines.append("    {" + ", ".join(str(e) for e in flat) + "},")
    lines.append("};")
    lines.append("")
    return "\n".join(lines)


def main(argv):
    text = render_header()
    if "--check" in argv:
        with open(HEADER) as f:
            same = f.read() == text
        print("up to date" if same else "differs")
        return 0 if same else 1
    with open(HEADER, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
