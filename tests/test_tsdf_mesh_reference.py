"""CPU suite: the triangle table of mi_tsdf_mesh and its numpy twin (tests/tsdf_mesh_reference.py).  The table's stated facts, from the
twin's own generator, from tools/gen_mc_table.py and from the committed header, which must be the generator's output byte for byte; then the
meshes of a noise lattice (every ambiguous face) and of a sphere: every directed edge once, its reverse once where the cube behind it
exists, the winding towards the positive side, the vertices a bitwise subsequence of extract(), every vertex referenced."""
import collections
import importlib.util
import os
import re

import numpy as np

import tsdf_mesh_reference as M
import tsdf_reference as R
from conftest import ROOT

ORIGIN = np.array([-0.35, 0.2, 0.05], np.float32)
VOXEL = 0.1
# rows of sphere_map(12, 4) to leave unobserved: (9, 4, 5) and (9, 6, 5), on either side of the crossing between (9, 5, 5) and (10, 5, 5) --
# each of the four cubes round that edge holds one of them, so the crossing stays in extract() and no triangle uses it -- and (2, 5, 5)
HOLES = [9 + 12 * (4 + 12 * 5), 9 + 12 * (6 + 12 * 5), 2 + 12 * (5 + 12 * 5)]


def generator():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def header_rows(gen):
    text = open(gen.HEADER).read()
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{16})ull", text)]
    assert len(words) == 256
    return text, [gen.unpack(w) for w in words]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_tables_facts():
    gen = generator()
    text, committed = header_rows(gen)
    for name, rows in (("twin", M.TABLE), ("generator", gen.table()), ("header", committed)):
        rows = [[tuple(t) for t in r] for r in rows]
        assert sum(len(r) for r in rows) == 820 and max(len(r) for r in rows) == 5, name
        hist = collections.Counter(len(r) for r in rows)
        assert [hist[k] for k in range(6)] == [2, 16, 50, 80, 76, 32], name
        assert rows[0x00] == [] and rows[0xff] == [], name
        assert rows[0x01] == [(0, 8, 4)], name
        assert rows[0x03] == [(4, 5, 9), (4, 9, 8)], name
        assert rows[0x5a] == [(0, 1, 11), (0, 11, 9), (2, 3, 10), (2, 10, 8)], name
        assert rows[0x69] == [(0, 8, 4), (1, 11, 5), (2, 9, 7), (3, 10, 6)], name
        assert rows == [[tuple(t) for t in r] for r in M.TABLE], name       # two generators, written apart, and the header: one table
    assert max(len(loop) for case in range(256) for loop in M.case_loops(case)) == 7
    assert max(len(loop) for case in range(256) for loop in gen.case_loops(case)) == 7
    assert "TSDF_MESH_TABLE_TRIANGLES = 820" in text


def test_the_committed_header_is_a_fresh_run_of_the_generator():
    gen = generator()
    assert open(gen.HEADER).read() == gen.header_text(gen.table())
    for row in gen.table():
        assert gen.unpack(gen.pack(row)) == row


def test_every_row_uses_each_crossed_edge_and_no_in_face_diagonal():
    for case, row in enumerate(M.TABLE):
        crossed = {e for e in range(12) if (case >> M.edge_corners(e)[0] & 1) != (case >> M.edge_corners(e)[1] & 1)}
        assert {e for t in row for e in t} == crossed, case
        sides = collections.Counter()
        for t in row:
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                sides[(a, b)] += 1
        assert set(sides.values()) <= {1}, case
        for (a, b) in sides:
            if (b, a) in sides:              # a fan's diagonal, inside the cube: never in a face, where the neighbour could repeat it
                assert not M.in_one_face(a, b), (case, a, b)
            else:                            # a side of a loop: a segment in one face
                assert M.in_one_face(a, b), (case, a, b)


def test_every_table_triangle_faces_the_positive_side():
    """vertices at the edges' midpoints: the geometric normal agrees with the sum of the three edges' directions towards their positive ends"""
    for case, row in enumerate(M.TABLE):
        for t in row:
            p, towards = [], np.zeros(3)
            for e in t:
                c0, c1 = M.edge_corners(e)
                p.append((M.corner_offset(c0) + M.corner_offset(c1)) / 2.0)
                towards[M.edge_axis(e)] += -1.0 if case >> c0 & 1 else 1.0
            assert np.cross(p[1] - p[0], p[2] - p[0]) @ towards > 0, (case, t)
    n = np.cross(np.array([0, 0, .5]) - np.array([.5, 0, 0]), np.array([0, .5, 0]) - np.array([.5, 0, 0]))
    assert (n < 0).all()                     # row 0x01 = (0, 8, 4): towards corner 0, the positive one


def check_mesh(mp, m):
    xyz, normals = R.extract(mp, ORIGIN, VOXEL)
    keys = M.crossing_keys(np.asarray(mp[0], np.int64), np.asarray(mp[1], np.float32), np.asarray(mp[2], np.float32) >= 1, R._Table(np.asarray(mp[0], np.int64), np.asarray(mp[2]) >= 1))
    at = np.searchsorted(keys, m.vert_key)
    assert (keys[at] == m.vert_key).all() and (np.diff(at) > 0).all()                 # a subsequence of extract() ...
    assert np.array_equal(bits(m.xyz), bits(xyz[at])) and np.array_equal(bits(m.normals), bits(normals[at]))    # ... with its bits
    assert m.tri.min() == 0 and m.tri.max() == len(m.xyz) - 1
    assert len(np.unique(m.tri)) == len(m.xyz)                                        # every vertex is referenced
    assert (m.tri[:, 0] != m.tri[:, 1]).all() and (m.tri[:, 1] != m.tri[:, 2]).all() and (m.tri[:, 0] != m.tri[:, 2]).all()
    assert (np.diff(m.tri_cube) >= 0).all()                                           # by cube in row order
    return at


def test_the_noise_lattice_is_closed_wherever_a_cube_lies_behind():
    mp = M.noise_map(12, 1)
    assert (np.abs(mp[1]) < 0.9).all() and (mp[1] != 0).all()
    m = M.mesh(mp, ORIGIN, VOXEL)
    cubes = (np.asarray(mp[0]) < 11).all(axis=1)
    assert np.array_equal(m.meshed, cubes)                                            # fully observed, nothing saturated: all 11^3 cubes
    assert len(set(m.case[m.meshed])) > 200                                           # (nearly) every case, the ambiguous ones among them
    check_mesh(mp, m)
    edges, open_edges = M.check_shared_edges(mp, 1.0, m)
    assert edges == 3 * len(m.tri) and 0 < open_edges < edges // 10                   # open on the lattice's own boundary alone
    # away from the boundary nothing is open: the inner 9^3 block of cubes has every neighbour
    a, b = M.directed_edges(m.tri)
    inner = np.repeat(((np.asarray(mp[0])[m.tri_cube] >= 1) & (np.asarray(mp[0])[m.tri_cube] <= 9)).all(axis=1), 3)
    code = set((a * len(m.xyz) + b).tolist())
    assert all((y * len(m.xyz) + x) in code for x, y in zip(a[inner].tolist(), b[inner].tolist()))


def test_a_sphere_is_a_closed_surface_facing_outwards():
    mp = M.sphere_map(12, 4.0)
    m = M.mesh(mp, ORIGIN, VOXEL)
    check_mesh(mp, m)
    edges, open_edges = M.check_shared_edges(mp, 1.0, m)
    assert open_edges == 0 and M.euler(m.tri, len(m.xyz)) == 2
    a, b = M.directed_edges(m.tri)
    assert (np.unique(np.minimum(a, b) * len(m.xyz) + np.maximum(a, b), return_counts=True)[1] == 2).all()
    assert (M.check_positive_side(mp, m) > 0).all()
    g = M.geometric_normals(m.xyz, m.tri)
    assert ((g[:, None, :] * m.normals[m.tri].astype(np.float64)).sum(axis=2) > 0).all()       # the winding agrees with the vertex normals
    centre = ORIGIN.astype(np.float64) + (5.5 + 0.5) * VOXEL
    radii = np.linalg.norm(m.xyz.astype(np.float64) - centre, axis=1)
    assert np.abs(radii - 4.0 * VOXEL).max() < 0.1 * VOXEL
    p = m.xyz.astype(np.float64)[m.tri]
    assert ((g * (p.mean(axis=1) - centre)).sum(axis=1) > 0).all()                    # outwards: the positive side


def test_holes_and_saturated_steps_give_no_triangle():
    coord, tsdf, weight = M.sphere_map(12, 4.0)
    weight = weight.copy()
    weight[HOLES] = 0.5
    mp = (coord, tsdf, weight)
    whole, holed = M.mesh((coord, tsdf, np.ones_like(weight)), ORIGIN, VOXEL), M.mesh(mp, ORIGIN, VOXEL)
    assert 0 < len(holed.tri) < len(whole.tri) and 0 < holed.meshed.sum() < whole.meshed.sum()
    at = check_mesh(mp, holed)
    assert len(at) < len(R.extract(mp, ORIGIN, VOXEL)[0])                             # a strict subset: crossings beside a hole go unused
    edges, open_edges = M.check_shared_edges(mp, 1.0, holed)
    assert open_edges > 0
    # a saturated step: +1 beside -1 is the back of the band, no crossing, and its cubes are not meshed
    z, y, x = np.meshgrid(np.arange(3), np.arange(3), np.arange(4), indexing="ij")
    c = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.int32)
    f = np.where(c[:, 0] < 2, 1.0, -1.0).astype(np.float32)
    flat = M.mesh((c, f, np.ones(len(c), np.float32)), ORIGIN, VOXEL)
    assert len(flat.tri) == 0 and len(flat.xyz) == 0 and not flat.meshed[(c[:, 0] == 1)].any() and flat.meshed[(c[:, 0] == 0) & (c[:, 1] < 2) & (c[:, 2] < 2)].all()
    f2 = np.where(c[:, 0] < 2, 1.0, -0.5).astype(np.float32)
    wall = M.mesh((c, f2, np.ones(len(c), np.float32)), ORIGIN, VOXEL)
    assert len(wall.tri) == 2 * 4 and len(wall.xyz) == 9


def test_empty_maps_and_maps_without_a_surface():
    none = M.mesh((np.zeros((0, 3), np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32)), ORIGIN, VOXEL)
    assert none.xyz.shape == (0, 3) and none.tri.shape == (0, 3)
    coord, tsdf, weight = M.sphere_map(6, 1.5)
    assert len(M.mesh((coord, np.minimum(np.abs(tsdf) + np.float32(0.1), np.float32(1)), weight), ORIGIN, VOXEL).tri) == 0
    assert len(M.mesh((coord, tsdf, weight * np.float32(0.5)), ORIGIN, VOXEL).tri) == 0
