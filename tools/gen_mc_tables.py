#!/usr/bin/env python3
"""Generate openobj_amd/csrc/objnerf_mc_tables.h: the marching-cubes case table of objnerf_mesh.hip.

    python tools/gen_mc_tables.py            # rewrites the header
    python tools/gen_mc_tables.py --check    # exits 1 if the committed header differs

The table is derived here from one face-local rule; nothing is copied from another implementation.

Cube convention (index space, axis 0 / 1 / 2 of a [d][d][d] volume):
  corner c in 0..7 sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1);
  edge e = 4 * axis + j joins corner EDGE_C0[e] and EDGE_C0[e] | (1 << axis), where EDGE_C0[e] is the j-th corner
  (in increasing order) whose bit `axis` is clear.  The vertex on edge e is owned by lattice point
  cell + offset(EDGE_C0[e]) along `axis`.
  case bit c is set when corner c is ABOVE the level (value > level; a value equal to the level counts as below).

Surface of one case: on each of the 6 faces, walk the 4 corners counter-clockwise as seen from outside the cube.
The crossing edges alternate between "leaving" the above region (above -> below) and "entering" it.  Every leaving
crossing is joined to the crossing before it in that walk.  With 2 crossings this is the only segment; with 4 (the
ambiguous face) it separates the two above corners.  The rule reads only the face's 4 corner bits, so the two
cells that share a face cut it identically (no cracks), and the table is deliberately not complement-symmetric.
Every crossing edge lies on two faces and is leaving on one, entering on the other, so the segments close into
directed loops.  Each loop is fanned into triangles; the apex is the first loop vertex (lowest edge id first)
whose fan diagonals do not lie in a cube face.  The resulting triangle winding is then fixed so that it matches
skimage.measure.marching_cubes(..., gradient_direction='ascent') (right-handed: the face normal by the right-hand
rule points from the above side to the below side, i.e. down the gradient).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "openobj_amd", "csrc", "objnerf_mc_tables.h")


def corner_off(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edges():
    out = []
    for a in range(3):
        for c in range(8):
            if not (c >> a) & 1:
                out.append((c, a))
    return out                                   # e = 4 * a + j


EDGES = edges()
EDGE_ID = {(c, c | (1 << a)): e for e, (c, a) in enumerate(EDGES)}


def edge_between(c0, c1):
    return EDGE_ID[(min(c0, c1), max(c0, c1))]


def faces():
    """6 faces as the corner walk counter-clockwise seen from outside: (axis, side, [4 corners])."""
    out = []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        for s in range(2):
            ring = []
            for (pu, pv) in [(0, 0), (1, 0), (1, 1), (0, 1)]:      # CCW about +e_a (e_u x e_v = e_a)
                ring.append((s << a) | (pu << u) | (pv << v))
            if s == 0:
                ring = ring[::-1]                                   # outward normal is -e_a
            out.append((a, s, ring))
    return out


FACES = faces()


def face_segments(case, ring):
    """Directed segments (edge_from, edge_to) the rule draws on one face."""
    above = [(case >> c) & 1 for c in ring]
    cross = []                                    # (edge, leaving?) in walk order
    for i in range(4):
        c0, c1 = ring[i], ring[(i + 1) % 4]
        if above[i] != above[(i + 1) % 4]:
            cross.append((edge_between(c0, c1), above[i] == 1))
    segs = []
    for i, (e, leaving) in enumerate(cross):
        if leaving:
            segs.append((e, cross[i - 1][0]))
    return segs


def edge_faces(e):
    c, a = EDGES[e]
    return {f for f, (fa, fs, ring) in enumerate(FACES) if c in ring and (c | (1 << a)) in ring}


def case_triangles(case):
    nxt = {}
    for (_, _, ring) in FACES:
        for e0, e1 in face_segments(case, ring):
            assert e0 not in nxt
            nxt[e0] = e1
    tris = []
    seen = set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop = [start]
        seen.add(start)
        e = nxt[start]
        while e != start:
            loop.append(e)
            seen.add(e)
            e = nxt[e]
        n = len(loop)
        best = 0
        for k in range(n):                        # apex whose diagonals stay off the cube faces
            rot = loop[k:] + loop[:k]
            ok = all(not (edge_faces(rot[0]) & edge_faces(rot[j])) for j in range(2, n - 1))
            if ok:
                best = k
                break
        rot = loop[best:] + loop[:best]
        for j in range(1, n - 1):
            # the walk keeps the above region on the left seen from outside: reversed, the right-hand normal points
            # from above to below, skimage's 'ascent' winding
            tris.append((rot[0], rot[j + 1], rot[j]))
    return tris


def build():
    return [case_triangles(c) for c in range(256)]


def render(table):
    maxt = max(len(t) for t in table)
    lines = [
        "// Generated by tools/gen_mc_tables.py -- do not edit.  Marching-cubes case table of objnerf_mesh.hip:",
        "// corner c at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) in (axis 0, 1, 2); case bit c = corner c above the level;",
        "// edge e = 4 * axis + j starts at corner MC_EDGE_C0[e] and runs along `axis`; triangles are edge triples, wound",
        "// like skimage's marching_cubes(gradient_direction='ascent').  Ambiguous faces: the two above corners are",
        "// separated (face-local, so neighbouring cells agree; not complement-symmetric).",
        "// Included twice by objnerf_mesh.hip, into a host and a device namespace: no include guard, no includes; the",
        "// includer defines OBJNERF_MC_QUAL (the storage of the arrays) and has <stdint.h>.",
        "#ifndef OBJNERF_MC_MAX_TRIS",
        f"#define OBJNERF_MC_MAX_TRIS {maxt}",
        "#endif",
        "",
        "OBJNERF_MC_QUAL uint8_t MC_EDGE_C0[12] = {" + ", ".join(str(c) for c, _ in EDGES) + "};",
        "OBJNERF_MC_QUAL uint8_t MC_EDGE_AXIS[12] = {" + ", ".join(str(a) for _, a in EDGES) + "};",
        "",
        "OBJNERF_MC_QUAL uint8_t MC_NTRI[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("  " + ", ".join(str(len(table[c])) for c in range(r, min(256, r + 32))) + ",")
    lines.append("};")
    lines.append("")
    lines.append(f"OBJNERF_MC_QUAL uint8_t MC_TRI[256][{3 * maxt}] = {{   // unused slots: 0xff")
    for c, t in enumerate(table):
        flat = [e for tri in t for e in tri] + [255] * (3 * maxt - 3 * len(t))
        lines.append("  {" + ", ".join(str(x) for x in flat) + "},")
    lines.append("};")
    return "\n".join(lines) + "\n"


def main():
    text = render(build())
    if "--check" in sys.argv:
        ok = os.path.exists(OUT) and open(OUT).read() == text
        print("objnerf_mc_tables.h up to date" if ok else "objnerf_mc_tables.h differs from the generator")
        sys.exit(0 if ok else 1)
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
