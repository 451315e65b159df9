"""The numpy twin of mi_tsdf_mesh, written from the rules of include/mi_slam.h alone, over tsdf_reference.py's table, gradient and crossing
(extract() gives the vertices' bits).  The triangle table is generated here, independently of csrc/tsdf_mesh_table.hpp and of
tools/gen_mc_table.py, and in other words: a face's corners are walked counter-clockwise as seen from outside, and every run of positive
corners sends the face edge behind its last corner to the face edge in front of its first -- which is "the positive corner lies to the
left" without a cross product.  tests/test_tsdf_mesh_reference.py pins the properties on the CPU, tests/test_gpu_tsdf_mesh.py compares the
device against mesh() bit for bit."""
import collections

import numpy as np

import tsdf_reference as R

F32, F64 = np.float32, np.float64


def corner_offset(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], np.int64)


def edge_axis(e):
    return e >> 2


def edge_offset(e):
    """the owner corner's offset: lo on the lower, hi on the higher of the two other axes"""
    axis, hi, lo = e >> 2, (e >> 1) & 1, e & 1
    u, v = [a for a in range(3) if a != axis]
    off = np.zeros(3, np.int64)
    off[u], off[v] = lo, hi
    return off


def edge_corners(e):
    """(owner corner, the corner at the other end)"""
    off = edge_offset(e)
    c0 = int(off[0] | off[1] << 1 | off[2] << 2)
    return c0, c0 | 1 << edge_axis(e)


EDGE_OF = {frozenset(edge_corners(e)): e for e in range(12)}


def _face_cycles():
    """per face: its four corners counter-clockwise as seen from outside the cube"""
    out = []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3                   # e_u x e_v = e_a: counter-clockwise as seen from +a
        for side in (0, 1):
            ring = []
            for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                off = [0, 0, 0]
                off[a], off[u], off[v] = side, du, dv
                ring.append(off[0] | off[1] << 1 | off[2] << 2)
            out.append(ring if side else ring[::-1])
    return out


FACE_CYCLES = _face_cycles()
FACE_EDGES = [{EDGE_OF[frozenset((ring[k], ring[(k + 1) % 4]))] for k in range(4)} for ring in FACE_CYCLES]


def in_one_face(e0, e1):
    return any(e0 in f and e1 in f for f in FACE_EDGES)


def case_loops(case):
    succ = {}
    for ring in FACE_CYCLES:
        pos = [bool(case >> c & 1) for c in ring]
        if all(pos) or not any(pos):
            continue
        for k in range(4):
            if pos[k] and not pos[k - 1]:                 # a run of positive corners starts at k ...
                j = k
                while pos[(j + 1) % 4]:
                    j += 1                                # ... and ends at j
                a = EDGE_OF[frozenset((ring[j % 4], ring[(j + 1) % 4]))]
                b = EDGE_OF[frozenset((ring[k - 1], ring[k]))]
                assert a not in succ
                succ[a] = b
    loops, seen = [], set()
    for e in sorted(succ):
        if e in seen:
            continue
        loop = [e]
        while succ[loop[-1]] != e:
            loop.append(succ[loop[-1]])
        seen.update(loop)
        loops.append(loop)
    assert len(seen) == len(succ)
    return loops


def fan(loop):
    for s in range(len(loop)):
        r = loop[s:] + loop[:s]
        if all(not in_one_face(r[0], r[k]) for k in range(2, len(r) - 1)):
            return [(r[0], r[k], r[k + 1]) for k in range(1, len(r) - 1)]
    raise AssertionError("loop %s: every start has an in-face diagonal" % (loop,))


def make_table():
    return [[t for loop in case_loops(case) for t in fan(loop)] for case in range(256)]


TABLE = make_table()

Mesh = collections.namedtuple("Mesh", "xyz normals tri vert_key tri_cube meshed case")


def crossing_keys(coord, tsdf, observed, table):
    """3 row + axis of every crossing of extract(), ascending: extract()'s own order"""
    rows = np.nonzero(observed)[0]
    keys = []
    for a in range(3):
        e = np.zeros(3, np.int64)
        e[a] = 1
        j = table(coord[rows] + e)
        i, j = rows[j >= 0], j[j >= 0]
        f0, f1 = tsdf[i].astype(F64), tsdf[j].astype(F64)
        cross = ((f0 > 0) != (f1 > 0)) & ~((np.abs(f0) >= 1) & (np.abs(f1) >= 1))
        keys.append(3 * i[cross] + a)
    return np.sort(np.concatenate(keys))


def mesh(map, origin, voxel, min_weight=1.0):
    """Mesh(xyz [nv, 3] float32, normals [nv, 3] float32, tri [nt, 3] int32, and what the checks want: vert_key [nv] = 3 row + axis of every
    vertex, tri_cube [nt] the row of every triangle's cube, meshed [rows] bool, case [rows])"""
    coord, tsdf, weight = np.asarray(map[0], np.int64).reshape(-1, 3), np.asarray(map[1], F32), np.asarray(map[2], F32)
    nrows = len(coord)
    none = Mesh(np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64),
                np.zeros(nrows, bool), np.zeros(nrows, np.int64))
    if nrows == 0:
        return none
    R.check_map(coord, tsdf, weight)
    observed = weight >= F32(min_weight)
    if not observed.any():
        return none
    table = R._Table(coord, observed)
    corner_row = np.stack([np.where(observed, table(coord + corner_offset(c)), -1) for c in range(8)], axis=1)
    f = tsdf[np.maximum(corner_row, 0)].astype(F64)
    positive, saturated = f > 0, np.abs(f) >= 1
    meshed = (corner_row >= 0).all(axis=1)
    for e in range(12):
        c0, c1 = edge_corners(e)
        meshed &= ~((positive[:, c0] != positive[:, c1]) & saturated[:, c0] & saturated[:, c1])
    case = np.where(meshed, (positive << np.arange(8)).sum(axis=1), 0)
    tri_key, tri_cube = [], []
    for i in np.nonzero(meshed)[0]:                       # by cube in row order, then in table order
        for t in TABLE[case[i]]:
            tri_key.append([3 * corner_row[i, edge_corners(e)[0]] + edge_axis(e) for e in t])
            tri_cube.append(i)
    if not tri_key:
        return none._replace(meshed=meshed, case=case)
    tri_key, tri_cube = np.array(tri_key, np.int64), np.array(tri_cube, np.int64)
    keys = crossing_keys(coord, tsdf, observed, table)
    xyz, normals = R.extract(map, origin, voxel, min_weight)
    assert len(keys) == len(xyz) and (np.diff(keys) > 0).all()
    used = np.unique(tri_key)
    assert np.isin(used, keys).all(), "a triangle uses an edge that is no crossing of extract()"
    keep = np.isin(keys, used)
    return Mesh(xyz[keep], normals[keep], np.searchsorted(used, tri_key).astype(np.int32), used, tri_cube, meshed, case)


# ---- what a mesh must satisfy (the CPU test asks it of mesh(), the GPU tests of the device's arrays with mesh()'s side facts)
def directed_edges(tri):
    tri = np.asarray(tri, np.int64)
    return tri[:, [0, 1, 2]].ravel(), tri[:, [1, 2, 0]].ravel()


def check_shared_edges(map, min_weight, m, tri=None):
    """Every directed edge occurs once; its reverse occurs once exactly where it must: always for an edge inside a cube, and for an edge in
    a cube's face where the cube on the other side of that face is meshed.  Returns (edges, edges without a reverse)."""
    coord, weight = np.asarray(map[0], np.int64).reshape(-1, 3), np.asarray(map[2], F32)
    tri = m.tri if tri is None else tri
    table = R._Table(coord, weight >= F32(min_weight))
    nvert = len(m.vert_key)
    a, b = directed_edges(tri)
    cube = np.repeat(m.tri_cube, 3)
    code, counts = np.unique(a * nvert + b, return_counts=True)
    assert (counts == 1).all(), "%d directed edges occur more than once" % (counts > 1).sum()
    has_reverse = np.isin(b * nvert + a, code)
    row, axis = m.vert_key // 3, m.vert_key % 3
    pos2 = 2 * coord[row]                                 # the lattice edge's midpoint, doubled
    pos2[np.arange(nvert), axis] += 1
    pa, pb, c2 = pos2[a], pos2[b], 2 * coord[cube]
    must, inside = np.zeros(len(a), bool), np.ones(len(a), bool)
    for d in range(3):
        in_face = (pa[:, d] == pb[:, d]) & (pa[:, d] % 2 == 0)
        beyond = coord[cube].copy()
        beyond[:, d] += np.where(pa[:, d] > c2[:, d], 1, -1)
        other = table(beyond)
        must |= in_face & (other >= 0) & m.meshed[np.maximum(other, 0)]
        inside &= ~in_face
    must |= inside
    assert (has_reverse == must).all(), "%d edges lack a reverse they must have, %d have one they cannot" % (
        (must & ~has_reverse).sum(), (has_reverse & ~must).sum())
    return len(a), int((~has_reverse).sum())


def geometric_normals(xyz, tri):
    p = np.asarray(xyz, F64)[np.asarray(tri, np.int64)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])


def check_positive_side(map, m, xyz=None, tri=None):
    """The geometric normal of every triangle points to the positive side: the positive end of the lattice edge under each of its vertices
    lies in front of the triangle's plane (or the normal is zero: a triangle folded onto a voxel centre by an exact 0)."""
    coord, tsdf = np.asarray(map[0], np.int64).reshape(-1, 3), np.asarray(map[1], F32)
    xyz, tri = (m.xyz if xyz is None else xyz), (m.tri if tri is None else tri)
    g = geometric_normals(xyz, tri)
    row, axis = m.vert_key // 3, m.vert_key % 3
    towards = np.where(tsdf[row] > 0, -1.0, 1.0)          # the owner is positive: the positive end is behind the vertex along the axis
    t = np.asarray(tri, np.int64)
    return np.take_along_axis(g, axis[t], axis=1) * towards[t]        # [nt, 3]: > 0 (or all 0) for every vertex of every triangle


def euler(tri, nvert):
    a, b = directed_edges(tri)
    undirected = np.unique(np.minimum(a, b) * nvert + np.maximum(a, b))
    return nvert - len(undirected) + len(tri)


def sphere_map(n=12, radius=4.0, band=3.0, centre=None):
    """a fully observed n^3 lattice of the clipped signed distance to a sphere, positive outside: (coord, tsdf, weight), rows by (cz, cy, cx)"""
    centre = np.full(3, (n - 1) / 2.0) if centre is None else np.asarray(centre, F64)
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    coord = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.int32)
    d = np.linalg.norm(coord.astype(F64) - centre, axis=1) - radius
    return coord, np.clip(d / band, -1.0, 1.0).astype(F32), np.ones(len(coord), F32)


def noise_map(n=12, seed=1):
    """a fully observed n^3 lattice of values in (-0.9, 0.9), none 0: every ambiguous face occurs"""
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    coord = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.int32)
    v = np.random.default_rng(seed).uniform(-0.9, 0.9, len(coord)).astype(F32)
    v[v == 0] = F32(0.5)
    return coord, v, np.ones(len(coord), F32)
