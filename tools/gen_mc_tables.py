#!/usr/bin/env python3
"""Derive the 256-case marching-cubes tables procedurally and write csrc/mc_tables.h.

    python tools/gen_mc_tables.py            # rewrites the header
    python tools/gen_mc_tables.py --check    # exit 1 if the committed header differs

Numbering (the kernels, mesh.py and this file share it):
  corner c = dx | dy << 1 | dz << 2 (dx, dy, dz in {0,1}: offsets along array axes 0, 1, 2); case bit c is set iff that
  corner is inside (v > level).
  edge e = 4 * a + (o1 | o2 << 1): the edge along axis a whose offsets on the other two axes (in increasing axis order)
  are o1, o2.  Its low end is the grid point that owns it.

Face rule.  On each of the cube's 6 faces the surface crosses the face in segments joining cut edges:
  1 or 3 inside corners: one segment cuts off the odd corner;
  2 adjacent inside corners: one segment parallel to them;
  2 diagonal inside corners (the ambiguous face): two segments, each cutting off one INSIDE corner -- inside corners are
  never joined across the face diagonal.
The rule depends only on the 4 corners of the face, so the two cells sharing a face draw the same segments: the surface of
a closed field is watertight.  Each segment is oriented so that, seen from outside the cube, the outside (v <= level)
side of the face is on its left; then the segments chain into closed loops around the cube and a loop read in order
has its right-hand normal pointing toward decreasing v.

Triangulation.  Each loop becomes a fan from one of its vertices.  Among the apices, the one whose fan draws the fewest
diagonals between two cut edges of a common cube face is taken (such a diagonal could also be drawn by the neighbouring
cell, giving an edge with four triangles); ties go to the lowest edge number.  The choice depends on the loop as an
unoriented cycle only, so complementary cases that share their face segments get the same triangles, reversed.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "learning-implicitly-from-spatial-transformers-network_amd", "csrc", "mc_tables.h")
MAX_TRIS = 5


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_id(c1, c2):
    """Edge between two corners that differ in exactly one axis."""
    d = c1 ^ c2
    assert d in (1, 2, 4), (c1, c2)
    a = d.bit_length() - 1
    p = corner_pos(c1)
    o = [p[b] for b in range(3) if b != a]
    return 4 * a + (o[0] | (o[1] << 1))


def edge_corners(e):
    a, r = divmod(e, 4)
    others = [b for b in range(3) if b != a]
    lo = ((r & 1) << others[0]) | (((r >> 1) & 1) << others[1])
    return lo, lo | (1 << a)


def edge_mid(e):
    c0, c1 = edge_corners(e)
    return tuple((u + v) / 2 for u, v in zip(corner_pos(c0), corner_pos(c1)))


def faces():
    """(outward normal, 4 corners in cyclic order) for each of the 6 faces."""
    out = []
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        for s in (0, 1):
            base = s << a
            ring = [base, base | (1 << b), base | (1 << b) | (1 << c), base | (1 << c)]
            n = [0, 0, 0]
            n[a] = 1 if s else -1
            out.append((tuple(n), ring))
    return out


FACES = faces()


def _sub(u, v):
    return tuple(x - y for x, y in zip(u, v))


def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _dot(u, v):
    return sum(x * y for x, y in zip(u, v))


def face_segments(ring, inside):
    """Unoriented segments (edge pairs) the face rule draws on a face with corners `ring` (cyclic) and `inside` flags."""
    fl = [inside[c] for c in ring]
    n_in = sum(fl)
    if n_in in (0, 4):
        return []
    e = [edge_id(ring[i], ring[(i + 1) % 4]) for i in range(4)]      # e[i] joins ring[i] and ring[i+1]
    if n_in == 2 and fl[0] == fl[2]:                                   # ambiguous: cut off each inside corner
        return [(e[(i - 1) % 4], e[i]) for i in range(4) if fl[i]]
    cut = [e[i] for i in range(4) if fl[i] != fl[(i + 1) % 4]]
    assert len(cut) == 2
    return [tuple(cut)]


def oriented_face_segments(n, ring, inside):
    """The face's segments oriented with the outside of the face on their left, seen along -n."""
    out = []
    for a, b in face_segments(ring, inside):
        pa, pb = edge_mid(a), edge_mid(b)
        mid = tuple((x + y) / 2 for x, y in zip(pa, pb))
        # the corner nearest the segment lies on its side; n x (b - a) must point away from the inside
        q = min(ring, key=lambda c: sum((x - y) ** 2 for x, y in zip(corner_pos(c), mid)))
        s = _dot(_cross(n, _sub(pb, pa)), _sub(corner_pos(q), mid))
        assert s != 0
        if (s < 0) != bool(inside[q]):
            a, b = b, a
        out.append((a, b))
    return out


def case_segments(case):
    inside = [(case >> c) & 1 for c in range(8)]
    return [(fi, s) for fi, (n, ring) in enumerate(FACES) for s in oriented_face_segments(n, ring, inside)]


def loops(case):
    nxt = {}
    for _, (a, b) in case_segments(case):
        assert a not in nxt
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values())
    out, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        out.append(loop)
    return out


def edge_faces(e):
    """The two cube faces (indices into FACES) that contain edge e."""
    c0, c1 = edge_corners(e)
    return {fi for fi, (_, ring) in enumerate(FACES) if c0 in ring and c1 in ring}


def triangulate(loop):
    n = len(loop)
    best = None
    for k in range(n):
        r = loop[k:] + loop[:k]
        bad = sum(1 for i in range(2, n - 1) if edge_faces(r[0]) & edge_faces(r[i]))
        key = (bad, r[0])
        if best is None or key < best[0]:
            best = (key, r)
    r = best[1]
    return [(r[0], r[i], r[i + 1]) for i in range(1, n - 1)]


def tables():
    edge_mask, tris = [], []
    for case in range(256):
        m = 0
        for e in range(12):
            c0, c1 = edge_corners(e)
            if ((case >> c0) & 1) != ((case >> c1) & 1):
                m |= 1 << e
        edge_mask.append(m)
        t = [tri for loop in loops(case) for tri in triangulate(loop)]
        assert len(t) <= MAX_TRIS, (case, len(t))
        tris.append(t)
    return edge_mask, tris


def render():
    edge_mask, tris = tables()
    lines = [
        "// GENERATED by tools/gen_mc_tables.py -- do not edit; rerun the generator.",
        "// Marching-cubes case tables derived from the face rule documented in the generator: inside corners are never",
        "// joined across a face diagonal, so the cells on both sides of a face draw the same segments on it.",
        "// corner c = dx | dy << 1 | dz << 2 (offsets along array axes 0, 1, 2); case bit c set iff corner c is inside",
        "// (v > level).  edge e = 4 * axis + (o1 | o2 << 1), o1 / o2 the offsets on the other two axes in increasing",
        "// order; the low end of the edge owns it.  Triangles have their right-hand normal toward decreasing v.",
        "#ifndef LIST_MC_TABLES_H",
        "#define LIST_MC_TABLES_H",
        "",
        "#include <stdint.h>",
        "",
        "// device constants in a HIP translation unit, plain constants elsewhere",
        "#if defined(__HIPCC__)",
        "#define LIST_MC_TABLE static __constant__ const",
        "#else",
        "#define LIST_MC_TABLE static const",
        "#endif",
        "",
        f"#define LIST_MC_MAX_TRIS {MAX_TRIS}",
        "",
        "// bit e set iff edge e changes sign",
        "LIST_MC_TABLE uint16_t kMcEdgeMask[256] = {",
    ]
    for r in range(0, 256, 12):
        lines.append("    " + " ".join(f"0x{m:03x}," for m in edge_mask[r:r + 12]))
    lines += ["};", "", "// number of triangles of each case", "LIST_MC_TABLE uint8_t kMcTriCount[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    " + " ".join(f"{len(t)}," for t in tris[r:r + 32]))
    lines += ["};", "", "// the triangles of each case as edge triples, -1 after the last",
              f"LIST_MC_TABLE int8_t kMcTriEdges[256][{3 * MAX_TRIS}] = {{"]
    for case, t in enumerate(tris):
        flat = [e for tri in t for e in tri]
        flat += [-1] * (3 * MAX_TRIS - len(flat))
        lines.append("    {" + ", ".join(f"{e:2d}" for e in flat) + f"}},  // {case}")
    lines += ["};", "", "#endif  // LIST_MC_TABLES_H", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with the committed header instead of writing it")
    ap.add_argument("--out", default=HEADER)
    args = ap.parse_args()
    text = render()
    if args.check:
        with open(args.out) as f:
            same = f.read() == text
        print("up to date" if same else f"{args.out} differs from the generator's output")
        return 0 if same else 1
    with open(args.out, "w") as f:
        f.write(text)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
