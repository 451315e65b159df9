"""The float64 twin of mi_tsdf_integrate and mi_tsdf_extract, written from the rules of include/mi_slam.h alone: numpy, one IEEE operation per
step in the stated order (fp32 where the header says fp32, fp64 on promoted operands elsewhere), sums taken one term after the other.  No
library call; tests/test_tsdf_reference.py pins its properties on the CPU, tests/test_gpu_tsdf.py compares the device against it bit for bit."""
import numpy as np

F32, F64 = np.float32, np.float64
MAX_HALF_STEPS = 16


def half_steps(voxel, tau):
    return int(np.floor(F64(F32(tau)) / (F64(F32(voxel)) / F64(2))))


def move(T, p):
    """w = ((R0 p_x + R1 p_y) + R2 p_z) + t in fp32, and o = t; T: the 4 x 4 matrix (sensor to world) or None: the identity"""
    T = np.eye(4, dtype=F32) if T is None else np.asarray(T, F32)
    p = np.asarray(p, F32).reshape(-1, 3)
    w = np.empty_like(p)
    for i in range(3):
        w[:, i] = ((T[i, 0] * p[:, 0] + T[i, 1] * p[:, 1]) + T[i, 2] * p[:, 2]) + T[i, 3]
    return w, T[:3, 3].copy()


def voxel_of(x, origin, voxel):
    """mi_voxel_index: floor((p - o) / v), one fp32 subtraction and one fp32 division"""
    q = np.floor((np.asarray(x, F32) - np.asarray(origin, F32)) / F32(voxel))
    assert np.all((q >= -2.0 ** 30) & (q < 2.0 ** 30)), "a voxel coordinate outside [-2^30, 2^30)"
    return q.astype(np.int64)


def centre_of(c, origin, voxel):
    return np.asarray(origin, F32).astype(F64) + (np.asarray(c).astype(F64) + 0.5) * F64(F32(voxel))


def samples(scans, poses, origin, voxel, tau, min_range=0.0, max_range=np.inf):
    """Every surviving sample in ascending (scan, point, k): (coord [m, 3] int64, f [m] float64, scan [m], point [m], k [m])"""
    S = half_steps(voxel, tau)
    assert S <= MAX_HALF_STEPS
    h, tau64 = F64(F32(voxel)) / F64(2), F64(F32(tau))
    out = [[], [], [], [], []]
    with np.errstate(all="ignore"):
        for s, scan in enumerate(scans):
            w32, o32 = move(None if poses is None else poses[s], scan)
            n = len(w32)
            if n == 0:
                continue
            w, o = w32.astype(F64), o32.astype(F64)
            e = w - o
            rho = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
            live = (rho > 0) & np.isfinite(rho) & ~(rho < F64(F32(min_range))) & ~(rho > F64(F32(max_range)))
            d = e / np.where(live, rho, 1.0)[:, None]
            keep = np.zeros((n, 2 * S + 1), bool)
            coord = np.zeros((n, 2 * S + 1, 3), np.int64)
            f = np.zeros((n, 2 * S + 1), F64)
            have_prev, prev = np.zeros(n, bool), np.zeros((n, 3), np.int64)
            for col, k in enumerate(range(-S, S + 1)):
                depth = rho + F64(k) * h
                exists = live & (depth > 0)
                x = (o[None, :] + depth[:, None] * d).astype(F32)
                c = np.zeros((n, 3), np.int64)
                c[exists] = voxel_of(x[exists], origin, voxel)
                same = have_prev & (c == prev).all(axis=1)
                prev = np.where(exists[:, None], c, prev)
                have_prev = have_prev | exists
                cen = centre_of(c, origin, voxel)
                sdf = (d[:, 0] * (w[:, 0] - cen[:, 0]) + d[:, 1] * (w[:, 1] - cen[:, 1])) + d[:, 2] * (w[:, 2] - cen[:, 2])
                q = sdf / tau64
                keep[:, col] = exists & ~same & ~(sdf < -tau64)
                coord[:, col] = c
                f[:, col] = np.where(q < 1.0, q, 1.0)
            pt, col = np.nonzero(keep)                    # row-major: ascending (point, k)
            out[0].append(coord[pt, col]); out[1].append(f[pt, col]); out[2].append(np.full(len(pt), s)); out[3].append(pt); out[4].append(col - S)
    if not out[0]:
        return np.zeros((0, 3), np.int64), np.zeros(0, F64), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    return tuple(np.concatenate(a) for a in out)


def check_map(coord, tsdf, weight):
    coord = np.asarray(coord, np.int64).reshape(-1, 3)
    if len(coord) > 1:
        a, b = coord[:-1], coord[1:]
        above = np.where(a[:, 2] != b[:, 2], b[:, 2] > a[:, 2], np.where(a[:, 1] != b[:, 1], b[:, 1] > a[:, 1], b[:, 0] > a[:, 0]))
        assert above.all(), "rows not strictly ascending by (cz, cy, cx)"
    assert (np.isfinite(weight) & (np.asarray(weight) > 0)).all() and (np.abs(tsdf) <= 1).all()


def integrate(scans, poses, origin, voxel, tau, min_range=0.0, max_range=np.inf, max_weight=np.inf, map=None):
    """(coord [nv, 3] int32, tsdf [nv] float32, weight [nv] float32), ascending by (cz, cy, cx)"""
    coord, f, _, _, _ = samples(scans, poses, origin, voxel, tau, min_range, max_range)
    if map is None:
        in_coord, in_d, in_w = np.zeros((0, 3), np.int64), np.zeros(0, F32), np.zeros(0, F32)
    else:
        in_coord, in_d, in_w = np.asarray(map[0], np.int64).reshape(-1, 3), np.asarray(map[1], F32), np.asarray(map[2], F32)
        check_map(in_coord, in_d, in_w)
    nin = len(in_coord)
    allc = np.concatenate([in_coord, coord])
    if len(allc) == 0:
        return np.zeros((0, 3), np.int32), np.zeros(0, F32), np.zeros(0, F32)
    order = np.lexsort((allc[:, 0], allc[:, 1], allc[:, 2]))          # stable: an input row first, then the samples as numbered
    sc = allc[order]
    head = np.concatenate([[True], (sc[1:] != sc[:-1]).any(axis=1)])
    start = np.nonzero(head)[0]
    end = np.concatenate([start[1:], [len(sc)]])
    stored = order[start] < nin
    first = start + stored                                             # the first sample of the run
    count = end - first
    F = np.zeros(len(start), F64)
    vals = np.concatenate([np.zeros(nin, F64), f])[order]
    for t in range(int(count.max()) if len(count) else 0):             # one term after the other, in the run's order
        rows = np.nonzero(count > t)[0]
        F[rows] = F[rows] + vals[first[rows] + t]
    D = np.where(stored, in_d[np.where(stored, order[start], 0)] if nin else 0.0, 0.0).astype(F64)
    W = np.where(stored, in_w[np.where(stored, order[start], 0)] if nin else 0.0, 0.0).astype(F64)
    C = count.astype(F64)
    with np.errstate(all="ignore"):
        total = W + C
        out_d = ((W * D + F) / total).astype(F32)
        out_w = np.where(total < F64(F32(max_weight)), total, F64(F32(max_weight))).astype(F32)
    untouched = count == 0
    if nin:
        rows_in = np.where(stored, order[start], 0)
        out_d = np.where(untouched, in_d[rows_in], out_d).astype(F32)
        out_w = np.where(untouched, in_w[rows_in], out_w).astype(F32)
    return sc[start].astype(np.int32), out_d, out_w


class _Table:
    """row of an observed voxel by coordinate, or -1"""

    def __init__(self, coord, observed):
        self.lo = coord.min(axis=0) - 1
        self.ext = coord.max(axis=0) - self.lo + 2
        rows = np.nonzero(observed)[0]
        keys = self._key(coord[rows])
        order = np.argsort(keys, kind="stable")
        self.keys, self.rows = keys[order], rows[order]

    def _key(self, c):
        r = c - self.lo
        return (r[:, 2] * self.ext[1] + r[:, 1]) * self.ext[0] + r[:, 0]

    def __call__(self, c):
        inside = ((c >= self.lo) & (c < self.lo + self.ext)).all(axis=1)
        k = self._key(np.where(inside[:, None], c, self.lo))
        at = np.minimum(np.searchsorted(self.keys, k), max(len(self.keys) - 1, 0))
        hit = inside & (len(self.keys) > 0) & (self.keys[at] == k if len(self.keys) else False)
        return np.where(hit, self.rows[at] if len(self.keys) else -1, -1)


def _gradient(table, coord, tsdf, rows):
    f0 = tsdf[rows].astype(F64)
    g = np.zeros((len(rows), 3), F64)
    for a in range(3):
        e = np.zeros(3, np.int64)
        e[a] = 1
        m, p = table(coord[rows] - e), table(coord[rows] + e)
        fm, fp = tsdf[np.maximum(m, 0)].astype(F64), tsdf[np.maximum(p, 0)].astype(F64)
        g[:, a] = np.where((m >= 0) & (p >= 0), (fp - fm) / 2.0, np.where(p >= 0, fp - f0, np.where(m >= 0, f0 - fm, 0.0)))
    return g


def extract(map, origin, voxel, min_weight=1.0):
    """(xyz [n, 3] float32, normals [n, 3] float32), by row, then axis"""
    coord, tsdf, weight = np.asarray(map[0], np.int64).reshape(-1, 3), np.asarray(map[1], F32), np.asarray(map[2], F32)
    empty = np.zeros((0, 3), F32)
    if len(coord) == 0:
        return empty, empty.copy()
    check_map(coord, tsdf, weight)
    observed = weight >= F32(min_weight)
    table = _Table(coord, observed)
    v64 = F64(F32(voxel))
    pts, nrm, key = [], [], []
    rows = np.nonzero(observed)[0]
    for a in range(3):
        e = np.zeros(3, np.int64)
        e[a] = 1
        j = table(coord[rows] + e)
        i, j = rows[j >= 0], j[j >= 0]
        f0, f1 = tsdf[i].astype(F64), tsdf[j].astype(F64)
        cross = ((f0 > 0) != (f1 > 0)) & ~((np.abs(f0) >= 1) & (np.abs(f1) >= 1))
        i, j, f0, f1 = i[cross], j[cross], f0[cross], f1[cross]
        r = f0 / (f0 - f1)
        cen = centre_of(coord[i], origin, voxel)
        cen[:, a] = cen[:, a] + r * v64
        gi, gj = _gradient(table, coord, tsdf, i), _gradient(table, coord, tsdf, j)
        v = (1.0 - r)[:, None] * gi + r[:, None] * gj
        norm = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        with np.errstate(all="ignore"):
            n = np.where((norm > 0)[:, None], v / np.where(norm > 0, norm, 1.0)[:, None], 0.0)
        pts.append(cen.astype(F32)); nrm.append(n.astype(F32)); key.append(3 * i + a)
    order = np.argsort(np.concatenate(key), kind="stable")
    return np.concatenate(pts)[order], np.concatenate(nrm)[order]
