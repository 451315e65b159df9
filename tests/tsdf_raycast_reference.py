"""The float64 twin of mi_tsdf_raycast, written from the rules of include/mi_slam.h alone: numpy, one IEEE operation per step in the stated
order (fp32 where the header says fp32, fp64 on promoted operands elsewhere).  Vectorised over the rays, a loop over the samples, look-ups
by searchsorted on packed keys (tsdf_reference's table).  It visits every sample: no empty-space skipping.  No library call;
tests/test_tsdf_raycast_reference.py pins it on cases with known answers, tests/test_tsdf_cast.py compares the shared header against it and
tests/test_gpu_tsdf_raycast.py the device, bit for bit."""
import numpy as np

from tsdf_reference import _gradient, _Table, check_map, move, voxel_of

F32, F64 = np.float32, np.float64
MAX_STEPS = 65536
LIMIT = 2.0 ** 30


def steps(voxel, min_range, max_range):
    return int(np.floor((F64(F32(max_range)) - F64(F32(min_range))) / (F64(F32(voxel)) / F64(2)))) + 1


def directions(pose, dirs):
    """(o [3] float64, d [n, 3] float64, live [n]): rule 1"""
    T = np.eye(4, dtype=F32) if pose is None else np.asarray(pose, F32)
    p = np.asarray(dirs, F32).reshape(-1, 3)
    _, o = move(T, np.zeros((1, 3), F32))                      # the translation column
    with np.errstate(all="ignore"):
        u = np.empty((len(p), 3), F64)
        for i in range(3):
            u[:, i] = ((T[i, 0] * p[:, 0] + T[i, 1] * p[:, 1]) + T[i, 2] * p[:, 2]).astype(F64)       # fp32, every operation rounded
        length = np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])
        live = (length > 0) & np.isfinite(length)
        d = u / np.where(live, length, 1.0)[:, None]
    return o.astype(F64), np.where(live[:, None], d, 0.0), live


def sample_voxels(o, d, s, origin, voxel):
    """(coord [m, 3] int64, in_range [m]) of the samples at depth s along the rays (o, d): rule 2"""
    with np.errstate(all="ignore"):
        x = (o[None, :] + s * d).astype(F32)
        q = np.floor((x - np.asarray(origin, F32)) / F32(voxel))
    ok = ((q >= -LIMIT) & (q < LIMIT)).all(axis=1)
    c = np.zeros((len(x), 3), np.int64)
    if ok.any():
        c[ok] = voxel_of(x[ok], origin, voxel)
    return c, ok


def field(table, tsdf, o, d, s, origin, voxel):
    """(available [m], F [m]) of the trilinear field at the depths s [m] of the rays (o, d [m, 3]): rule 4"""
    p = o[None, :] + s[:, None] * d
    q = (p - np.asarray(origin, F32).astype(F64)) / F64(F32(voxel)) - 0.5
    ok = ((q >= -LIMIT) & (q < LIMIT)).all(axis=1)
    i = np.floor(np.where(ok[:, None], q, 0.0))
    w = np.where(ok[:, None], q, 0.0) - i
    i = i.astype(np.int64)
    f = {}
    for z in (0, 1):
        for y in (0, 1):
            for x in (0, 1):
                row = table(i + np.array([x, y, z], np.int64))
                ok = ok & (row >= 0)
                f[x, y, z] = tsdf[np.maximum(row, 0)].astype(F64)
    c = {(y, z): f[0, y, z] + w[:, 0] * (f[1, y, z] - f[0, y, z]) for y in (0, 1) for z in (0, 1)}
    c0 = c[0, 0] + w[:, 1] * (c[1, 0] - c[0, 0])
    c1 = c[0, 1] + w[:, 1] * (c[1, 1] - c[0, 1])
    return ok, c0 + w[:, 2] * (c1 - c0)


def raycast(map, origin, voxel, max_range, pose, dirs, min_weight=1.0, min_range=0.0, details=False):
    """(depth [n] float32, xyz [n, 3] float32, normals [n, 3] float32, hits); with details a dict beside them: d [n, 3], end_k [n] (K: the
    march ran out), and for the hits trilinear [n] and r [n]"""
    dirs = np.asarray(dirs, F32).reshape(-1, 3)
    n = len(dirs)
    K = steps(voxel, min_range, max_range)
    assert 1 <= K <= MAX_STEPS
    depth, xyz, normals = np.zeros(n, F32), np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    o, d, live = directions(pose, dirs)
    info = {"d": d, "end_k": np.full(n, K, np.int64), "trilinear": np.zeros(n, np.int64), "r": np.zeros(n, F64), "K": K}
    coord = np.zeros((0, 3), np.int64) if map is None else np.asarray(map[0], np.int64).reshape(-1, 3)
    if len(coord) == 0:
        return (depth, xyz, normals, 0) + ((info,) if details else ())
    tsdf, weight = np.asarray(map[1], F32), np.asarray(map[2], F32)
    check_map(coord, tsdf, weight)
    table = _Table(coord, weight >= F32(min_weight))
    h, lo = F64(F32(voxel)) / F64(2), F64(F32(min_range))

    active = live.copy()
    prev_observed, prev_g, prev_row = np.zeros(n, bool), np.zeros(n, F64), np.zeros(n, np.int64)
    hit_ray, hit_k, hit_prev, hit_row = [], [], [], []
    for k in range(K):                                         # rule 3
        idx = np.nonzero(active)[0]
        if len(idx) == 0:
            break
        c, ok = sample_voxels(o, d[idx], lo + F64(k) * h, origin, voxel)
        row = np.where(ok, table(c), -1)
        g = tsdf[np.maximum(row, 0)].astype(F64)
        positive = (row >= 0) & (g > 0)
        ends = (row >= 0) & ~positive
        hits = ends & prev_observed[idx] & (k >= 1)
        hit_ray.append(idx[hits]); hit_k.append(np.full(hits.sum(), k)); hit_prev.append(prev_row[idx[hits]]); hit_row.append(row[hits])
        info["end_k"][idx[ends]] = k
        active[idx[ends]] = False
        prev_observed[idx] = positive
        prev_g[idx[positive]] = g[positive]
        prev_row[idx[positive]] = row[positive]

    ray, k, ri, rj = (np.concatenate(a) if a else np.zeros(0, np.int64) for a in (hit_ray, hit_k, hit_prev, hit_row))
    if len(ray) == 0:
        return (depth, xyz, normals, 0) + ((info,) if details else ())
    a, b = lo + (k - 1).astype(F64) * h, lo + k.astype(F64) * h           # rule 4
    gi, gj = tsdf[ri].astype(F64), tsdf[rj].astype(F64)
    with np.errstate(all="ignore"):
        ok_a, Fa = field(table, tsdf, o, d[ray], a, origin, voxel)
        ok_b, Fb = field(table, tsdf, o, d[ray], b, origin, voxel)
        tri = ok_a & ok_b & (Fa > 0) & (0 >= Fb)
        r = np.where(tri, Fa / np.where(tri, Fa - Fb, 1.0), gi / (gi - gj))
        t = a + r * h
        dep = t.astype(F32)
        point = (o[None, :] + t[:, None] * d[ray]).astype(F32)
        v = (1.0 - r)[:, None] * _gradient(table, coord, tsdf, ri) + r[:, None] * _gradient(table, coord, tsdf, rj)      # rule 5
        norm = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        nrm = np.where((norm > 0)[:, None], v / np.where(norm > 0, norm, 1.0)[:, None], 0.0).astype(F32)
    good = dep > 0                                             # a depth that rounds to 0 is a miss
    ray, dep, point, nrm, tri, r = ray[good], dep[good], point[good], nrm[good], tri[good], r[good]
    depth[ray], xyz[ray], normals[ray] = dep, point, nrm
    info["trilinear"][ray], info["r"][ray] = tri, r
    return (depth, xyz, normals, len(ray)) + ((info,) if details else ())


def slab(plane_x=5.25, lo=(0, 0, 0), hi=(12, 8, 8), tau=2.0, voxel=1.0, origin=(0.0, 0.0, 0.0), band=3):
    """A hand-made map: a wall at x = plane_x seen from the low-x side, the values linear in x across it -- f = (plane_x - centre_x) / tau,
    clipped to [-1, 1] -- on the voxels whose centre is within `band` voxels of the plane, weight 1, over lo .. hi (voxel coordinates,
    hi exclusive).  Rows ascending by (cz, cy, cx)."""
    cz, cy, cx = np.meshgrid(np.arange(lo[2], hi[2]), np.arange(lo[1], hi[1]), np.arange(lo[0], hi[0]), indexing="ij")
    coord = np.stack([cx.ravel(), cy.ravel(), cz.ravel()], axis=1).astype(np.int32)
    centre = F64(F32(origin[0])) + (coord[:, 0].astype(F64) + 0.5) * F64(F32(voxel))
    keep = np.abs(centre - plane_x) <= band * F64(F32(voxel))
    f = np.clip((plane_x - centre[keep]) / tau, -1, 1).astype(F32)
    return coord[keep], f, np.ones(keep.sum(), F32)
