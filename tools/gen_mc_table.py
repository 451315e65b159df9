#!/usr/bin/env python3
"""Generates cuda-slam_amd/csrc/tsdf_mesh_table.hpp: the marching-cubes triangle table of mi_tsdf_mesh (include/mi_slam.h states the rules;
DESIGN.md, "The mesh", says why they are these).  Nothing is copied from a published table: the 256 rows follow from the cube's geometry.

  corners   corner c of a cube is its origin + (c & 1, (c >> 1) & 1, (c >> 2) & 1); the case is the OR of 1 << c over the positive corners
  edges     edge e = 4 axis + 2 hi + lo runs along `axis` from its owner corner, whose offset has `lo` on the lower and `hi` on the higher
            of the two other axes
  segments  on each of the six faces the crossed edges (ends of different sign) are two or four; two are joined by one segment, four by
            two, each cutting off one positive corner -- a rule of the face's four signs alone, so the two cubes on a face agree
  direction seen from outside the cube the positive corner lies to the left of the segment: a -> b when
            n . ((m_b - m_a) x (p - m_a)) > 0 with n the face's outward normal, m the edge midpoints and p the positive corner
  loops     every crossed edge has one successor; loops are followed from the lowest unvisited edge
  fan       the loop is rotated to the first start, counted from its lowest edge, whose fan has no diagonal between two edges of one cube
            face (a neighbouring cube could produce the same diagonal again); the triangles are (r0, rk, rk+1)

Usage: python tools/gen_mc_table.py [--check]      (--check: compare with the committed header, write nothing)"""
import itertools
import os
import sys

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cuda-slam_amd", "csrc", "tsdf_mesh_table.hpp")
MAX_TRIANGLES = 5


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edge_owner(e):
    """(axis, owner corner's offset) of edge e"""
    axis, hi, lo = e >> 2, (e >> 1) & 1, e & 1
    off = [0, 0, 0]
    others = [a for a in range(3) if a != axis]
    off[others[0]], off[others[1]] = lo, hi
    return axis, tuple(off)


def edge_ends(e):
    axis, off = edge_owner(e)
    end = list(off)
    end[axis] = 1
    return off, tuple(end)


def corner_index(off):
    return off[0] | off[1] << 1 | off[2] << 2


def faces():
    """[(axis, side, outward normal, the face's 4 edges)]"""
    out = []
    for axis in range(3):
        for side in (0, 1):
            n = [0, 0, 0]
            n[axis] = 1 if side else -1
            on = [e for e in range(12) if edge_owner(e)[0] != axis and edge_owner(e)[1][axis] == side]
            assert len(on) == 4
            out.append((axis, side, tuple(n), on))
    return out


FACES = faces()


def share_a_face(e0, e1):
    return any(e0 in on and e1 in on for _, _, _, on in FACES)


def cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def sub(u, v):
    return tuple(a - b for a, b in zip(u, v))


def midpoint(e):
    a, b = edge_ends(e)
    return tuple((x + y) / 2 for x, y in zip(a, b))


def directed(n, ea, eb, p):
    """the segment between the edges ea and eb, as (from, to): the positive corner p to its left, seen from outside"""
    ma, mb = midpoint(ea), midpoint(eb)
    s = sum(x * y for x, y in zip(n, cross(sub(mb, ma), sub(p, ma))))
    assert s != 0
    return (ea, eb) if s > 0 else (eb, ea)


def case_loops(case):
    positive = lambda off: bool(case >> corner_index(off) & 1)
    crossed = [e for e in range(12) if positive(edge_ends(e)[0]) != positive(edge_ends(e)[1])]
    successor = {}
    for axis, side, n, on in FACES:
        cut = [e for e in on if e in crossed]
        corners = [corner_offset(c) for c in range(8) if corner_offset(c)[axis] == side]
        assert len(cut) in (0, 2, 4)
        if len(cut) == 2:
            p = next(c for c in corners if positive(c))
            segments = [directed(n, cut[0], cut[1], p)]
        else:
            segments = []
            for p in corners:
                if len(cut) == 4 and positive(p):        # the two face edges that meet at the corner cut off
                    ea, eb = [e for e in cut if p in edge_ends(e)]
                    segments.append(directed(n, ea, eb, p))
        for a, b in segments:
            assert a not in successor, "edge %d of case %d has two successors" % (a, case)
            successor[a] = b
    assert sorted(successor) == crossed and sorted(successor.values()) == crossed
    loops, seen = [], set()
    for e in crossed:                                    # ascending: a loop starts at its lowest edge, loops come by their lowest edge
        if e in seen:
            continue
        loop = [e]
        while successor[loop[-1]] != e:
            loop.append(successor[loop[-1]])
        seen.update(loop)
        loops.append(loop)
    return loops


def fan(loop):
    for start in range(len(loop)):
        r = loop[start:] + loop[:start]
        if not any(share_a_face(r[0], r[k]) for k in range(2, len(r) - 1)):
            return [(r[0], r[k], r[k + 1]) for k in range(1, len(r) - 1)]
    raise AssertionError("no start of loop %s has a fan free of in-face diagonals" % loop)


def table():
    """256 rows, each a list of at most 5 triangles of three edge numbers"""
    rows = [[t for loop in case_loops(case) for t in fan(loop)] for case in range(256)]
    assert max(len(r) for r in rows) <= MAX_TRIANGLES
    return rows


def pack(row):
    """one 64-bit word: edge v of triangle t in bits 4 (3 t + v) .. + 3, the number of triangles in bits 60 .. 63"""
    word = len(row) << 60
    for i, e in enumerate(itertools.chain.from_iterable(row)):
        word |= e << 4 * i
    return word


def unpack(word):
    return [tuple(word >> 4 * (3 * t + v) & 15 for v in range(3)) for t in range(word >> 60)]


def header_text(rows):
    out = ["// Generated by tools/gen_mc_table.py -- do not edit; tests/test_tsdf_mesh_reference.py compares this file with a fresh run.",
           "// The marching-cubes table of mi_tsdf_mesh (K78): row = the cube's case, the OR of 1 << c over its positive corners.  A row is one",
           "// 64-bit word: edge v (0 .. 11) of triangle t in bits 4 (3 t + v) .. + 3, the number of triangles (0 .. 5) in bits 60 .. 63.",
           "#pragma once", "", "namespace mislam {", "",
           "constexpr int TSDF_MESH_CASES = 256;",
           "constexpr int TSDF_MESH_MAX_TRIANGLES = %d;" % MAX_TRIANGLES,
           "constexpr int TSDF_MESH_TABLE_TRIANGLES = %d;      // over all rows" % sum(len(r) for r in rows),
           "constexpr unsigned long long TSDF_MESH_TABLE[TSDF_MESH_CASES] = {"]
    for at in range(0, 256, 4):
        out.append("    " + " ".join("0x%016xull," % pack(r) for r in rows[at:at + 4]) + "   // 0x%02x" % at)
    out += ["};", "", "}  // namespace mislam", ""]
    return "\n".join(out)


def main(argv):
    text = header_text(table())
    if "--check" in argv:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("%s: %s" % (HEADER, "up to date" if same else "DIFFERS from a fresh run"))
        return 0 if same else 1
    with open(HEADER, "w") as fh:
        fh.write(text)
    print("wrote %s: %d triangles" % (HEADER, sum(len(r) for r in table())))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
