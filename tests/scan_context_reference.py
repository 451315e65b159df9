"""The contracts of mi_scan_context and mi_scan_context_search (include/mi_slam.h) restated in numpy, bit for bit, and beside the restatement
an independent plain-float64 twin (arctan2, sqrt, np.dot) that checks the restatement itself (tests/test_scan_context_reference.py).

The restatement bins with the very doubles the library bins with: the caller passes the tables of capi.scan_context_tables(params).  numpy
never fuses a product into a sum, so `a * b - c * d` below is two rounded products and one rounded difference, as the header says.  The
fp32 fmaf chain of the cosines is match_reference.fmaf, exact."""
import numpy as np

from match_reference import fmaf


# ---- mi_scan_context
def bins(xyz, centre, edge2, dirs):
    """(ring int [n], sector int [n]) of every point by the header's rule; ring -1: the point belongs to no bin.  edge2 [rings + 1],
    dirs [sectors, 2]: capi.scan_context_tables."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    c = np.zeros(3, np.float32) if centre is None else np.asarray(centre, np.float32)
    rings, sectors = len(edge2) - 1, len(dirs)
    dx = xyz[:, 0].astype(np.float64) - np.float64(c[0])
    dy = xyz[:, 1].astype(np.float64) - np.float64(c[1])
    xx, yy = dx * dx, dy * dy
    d2 = xx + yy
    ring = np.zeros(len(xyz), np.int64)
    for e in range(1, rings):
        ring += edge2[e] <= d2
    ring[~(d2 < edge2[rings])] = -1
    upper = (dy > 0) | ((dy == 0) & (dx > 0))
    lower = (dy < 0) | ((dy == 0) & (dx < 0))
    first_lower = (sectors + 1) // 2
    passed = np.zeros(len(xyz), np.int64)
    for j in range(sectors):
        a, b = dirs[j, 0] * dy, dirs[j, 1] * dx
        own = upper if j < first_lower else lower
        passed += own & ((a - b) >= 0)
    sector = np.where(upper, passed - 1, first_lower - 1 + passed)
    sector[~(upper | lower)] = 0
    return ring, np.maximum(sector, 0)


def descriptor(xyz, centre, z_offset, edge2, dirs):
    """[rings, sectors] float32: the largest z + z_offset (one fp32 addition) of every bin where that is positive, else +0."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rings, sectors = len(edge2) - 1, len(dirs)
    ring, sector = bins(xyz, centre, edge2, dirs)
    v = xyz[:, 2] + np.float32(z_offset)
    keep = (ring >= 0) & (v > 0)
    out = np.zeros((rings, sectors), np.float32)
    np.maximum.at(out, (ring[keep], sector[keep]), v[keep])
    return out


def descriptors(clouds, centres, params, tables):
    return np.stack([descriptor(c, None if centres is None else centres[i], params.z_offset, *tables) for i, c in enumerate(clouds)])


def bins_twin(xyz, centre, rings, sectors, max_radius):
    """The same bins from the definition: the ring from the distance's square root, the sector from the angle.  Agrees with bins() away from
    the edges and boundaries (boundary_margin)."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    c = np.zeros(3) if centre is None else np.asarray(centre, np.float64)
    rho = np.sqrt((xyz[:, 0] - c[0]) ** 2 + (xyz[:, 1] - c[1]) ** 2)
    ang = np.mod(np.arctan2(xyz[:, 1] - c[1], xyz[:, 0] - c[0]), 2 * np.pi)
    ring = np.floor(rho / max_radius * rings).astype(np.int64)
    ring[rho >= max_radius] = -1
    return ring, np.minimum(np.floor(ang / (2 * np.pi) * sectors).astype(np.int64), sectors - 1)


def boundary_margin(xyz, centre, rings, sectors, max_radius):
    """The smallest relative distance of any point from a ring edge (in units of the ring's width) or a sector boundary (in units of the
    sector's width): what a test asserts to be large before it compares bins() with bins_twin()."""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    c = np.zeros(3) if centre is None else np.asarray(centre, np.float64)
    u = np.sqrt((xyz[:, 0] - c[0]) ** 2 + (xyz[:, 1] - c[1]) ** 2) / max_radius * rings
    w = np.mod(np.arctan2(xyz[:, 1] - c[1], xyz[:, 0] - c[0]), 2 * np.pi) / (2 * np.pi) * sectors
    return min(np.abs(u - np.rint(u)).min(), np.abs(w - np.rint(w)).min())


def descriptor_twin(xyz, centre, rings, sectors, max_radius, z_offset):
    xyz32 = np.asarray(xyz, np.float32).reshape(-1, 3)
    ring, sector = bins_twin(xyz32, centre, rings, sectors, max_radius)
    v = xyz32[:, 2] + np.float32(z_offset)
    out = np.zeros((rings, sectors), np.float32)
    for r, s, h in zip(ring, sector, v):
        if r >= 0 and h > out[r, s]:
            out[r, s] = h
    return out


# ---- mi_scan_context_search
def unit_columns(desc):
    """(unit float32 [rows, rings, sectors], nonempty bool [rows, sectors]): every column over the fp64 root of its fp64 sum of squares, rings
    ascending, each component rounded to fp32 once; an empty column stays +0."""
    d = np.asarray(desc, np.float32).astype(np.float64)
    ss = np.zeros((d.shape[0], d.shape[2]))
    for r in range(d.shape[1]):
        ss = ss + d[:, r, :] * d[:, r, :]
    norm = np.sqrt(ss)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(ss[:, None, :] > 0, d / norm[:, None, :], 0.0).astype(np.float32)
    return u, ss > 0


def shift_distances(uq, mq, uc, mc):
    """float32 [nd, sectors]: d_s of one query (unit columns uq [rings, sectors], mask mq [sectors]) against every row of uc, mc."""
    rings, sectors = uq.shape
    G = np.zeros((uc.shape[0], sectors, sectors), np.float32)          # [row, j, k]
    for r in range(rings):
        G = fmaf(uq[r][None, :, None], uc[:, r, None, :], G)
    j = np.arange(sectors)[None, :]
    k = (j + np.arange(sectors)[:, None]) % sectors                     # [s, j]
    valid = mq[None, None, :] & mc[:, k]                                # [row, s, j]
    term = np.where(valid, 1.0 - G[:, j, k].astype(np.float64), 0.0)
    # np.cumsum adds one element after the other, j ascending; a term that is left out adds 0.0, which changes no bit of a sum that is never -0
    total = np.cumsum(term, axis=2)[:, :, -1]
    cnt = valid.sum(axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, (total / cnt).astype(np.float32), np.float32(1.0))


def search(query, db, limit=None):
    """(idx int32 [nq], dist float32 [nq], shift int32 [nq], second float32 [nq]): the contract's outputs.  np.argmin returns the first of
    equal minima: the lowest shift, then the lowest row."""
    uq, mq = unit_columns(query)
    uc, mc = unit_columns(db)
    nq, nd = len(uq), len(uc)
    idx, dist, shift, second = np.full(nq, -1, np.int32), np.full(nq, np.inf, np.float32), np.zeros(nq, np.int32), np.full(nq, np.inf, np.float32)
    for i in range(nq):
        lim = nd if limit is None else min(int(limit[i]), nd)
        if lim <= 0:
            continue
        d = shift_distances(uq[i], mq[i], uc[:lim], mc[:lim])
        per_row, per_shift = d.min(axis=1), d.argmin(axis=1)
        idx[i] = per_row.argmin()
        dist[i], shift[i] = per_row[idx[i]], per_shift[idx[i]]
        if lim > 1:
            second[i] = np.delete(per_row, idx[i]).min()
    return idx, dist, shift, second


def shift_distances_twin(q, db):
    """float64 [nd, sectors]: the same distances in plain float64 -- np.dot of columns normalised in float64."""
    def unit(d):
        d = np.asarray(d, np.float64)
        n = np.sqrt((d * d).sum(axis=-2, keepdims=True))
        return np.where(n > 0, d / np.where(n > 0, n, 1.0), 0.0), n[..., 0, :] > 0
    uq, mq = unit(q)
    uc, mc = unit(db)
    sectors = uq.shape[1]
    G = np.einsum("rj,nrk->njk", uq, uc)
    j = np.arange(sectors)
    out = np.ones((len(uc), sectors))
    for s in range(sectors):
        k = (j + s) % sectors
        valid = mq[None, :] & mc[:, k]
        cnt = valid.sum(axis=1)
        tot = np.where(valid, 1.0 - G[:, j, k], 0.0).sum(axis=1)
        out[:, s] = np.where(cnt > 0, tot / np.maximum(cnt, 1), 1.0)
    return out


# ---- the same search at pair counts where emulating every fmaf of every pair is not affordable
def e_bound(rings):
    """An upper bound of |d - t| for any one (query, row, shift): d the contract's fp32 distance (shift_distances), t the plain-float64
    twin's (shift_distances_twin, row_minima_twin).  Derived, with u = 2^-24 the unit roundoff of fp32; nothing here is measured.

    1. The components.  A unit component is x = v / norm formed in fp64 (relative error below 3 * 2^-53) and rounded to fp32 once: x(1 + a),
       |a| <= u.  (Below fp32's normal range the error is absolute, at most 2^-150, and never counts.)  The product of two rounded
       components is exact inside the fmaf and equals x y (1 + a)(1 + b); the columns have unit length, so by Cauchy-Schwarz the absolute
       exact products of one G(j, k) sum to at most 1, the rounded ones to at most (1 + u)^2, and the two sums differ by at most 2u + u^2.
    2. The chain.  G is `rings` fmafs, c <- fl(c + p), the first of them onto 0: `rings` roundings, each a relative error of at most u
       on a partial sum.  The standard bound is gamma |p|_1 with gamma = rings u / (1 - rings u), at most rings u (1 + u)^2 / (1 - rings u)
       here.  With rings <= 32 everything of second order in 1. and 2. together is below 2^-38 < 0.0001 u.
    3. The mean.  1 - G, the sum of at most 64 such terms and the division are fp64 on both sides: below 70 * 2^-53 < 2^-46 each; the twin's
       own matrix product, whatever the order of its sums, is within rings * 2^-53 of the exact one.  A mean of terms moves by no more than
       its terms do.
    4. The distance.  |G| <= 1 + 2^-19, so the mean lies in [-2^-19, 2 + 2^-19], and its one rounding to fp32 is at most half a unit in the
       last place of a number below 2 (2 itself is representable): 2^-24 = u.

    Together: 2u + rings u + u + less than 0.001 u = (rings + 3.001) u.  (rings + 5) u, the estimate this bound was first stated with,
    holds with 2u to spare and is what is returned: it is used as a margin, where more is safe.  The minimum over the shifts of a row obeys
    the same bound as each shift does."""
    return (rings + 5) * 2.0 ** -24


def row_minima_twin(query, db, block=1 << 16):
    """float64 [nq, nd]: every row's smallest twin distance over the shifts.  The arithmetic of shift_distances_twin, but G of a block of
    queries against a block of rows is one matrix product ([queries x sectors, rings] by [rings, rows x sectors]: BLAS does the
    nq * nd * sectors^2 * rings work), and shift s reads its wrapped diagonal G(j, (j + s) mod sectors) through a strided view of G laid
    beside itself.  The number of pairs under a shift is a matrix product of the masks, exact in float64.  block: elements of G per product:
    small enough for the block's temporaries to stay in the cache."""
    from numpy.lib.stride_tricks import as_strided

    def unit(d):
        d = np.asarray(d, np.float64)
        n = np.sqrt((d * d).sum(axis=-2, keepdims=True))
        return np.where(n > 0, d / np.where(n > 0, n, 1.0), 0.0), n[..., 0, :] > 0
    uq, mq = unit(query)
    uc, mc = unit(db)
    (nq, rings, sectors), nd = uq.shape, uc.shape[0]
    rb = min(nd, max(1, block // sectors ** 2))
    qb = min(nq, max(1, block // (rb * sectors ** 2)))
    out = np.empty((nq, nd))
    for r0 in range(0, nd, rb):
        n = min(rb, nd - r0)
        B = np.ascontiguousarray(uc[r0:r0 + n].transpose(1, 0, 2)).reshape(rings, n * sectors)
        mc2 = np.concatenate([mc[r0:r0 + n]] * 2, axis=1)
        # rot[j, row, s] = the row's mask at column (j + s) mod sectors
        rot = as_strided(mc2, (sectors, n, sectors), (mc2.strides[1], mc2.strides[0], mc2.strides[1]), writeable=False)
        rot_count = rot.astype(np.float64).reshape(sectors, n * sectors)
        for q0 in range(0, nq, qb):
            b = min(qb, nq - q0)
            A = np.ascontiguousarray(uq[q0:q0 + b].transpose(0, 2, 1)).reshape(b * sectors, rings)
            G = np.matmul(A, B).reshape(b, sectors, n, sectors)         # [query, j, row, k]
            G2 = np.concatenate([G, G], axis=3)
            st = G2.strides
            diag = as_strided(G2, G.shape, (st[0], st[1] + st[3], st[2], st[3]), writeable=False)      # [query, j, row, s]
            valid = mq[q0:q0 + b][:, :, None, None] & rot[None]
            tot = np.where(valid, 1.0 - diag, 0.0).sum(axis=1)          # [query, row, s]
            cnt = np.matmul(mq[q0:q0 + b].astype(np.float64), rot_count).reshape(b, n, sectors)
            out[q0:q0 + b, r0:r0 + n] = np.where(cnt > 0, tot / np.maximum(cnt, 1), 1.0).min(axis=2)
    return out


def search_pruned(query, db, limit=None, stats=None):
    """search(), bit for bit, at a cost that many pairs allow.  Every row's smallest distance is known from row_minima_twin to within
    e = e_bound(rings).  Let T2 be the second smallest twin minimum among a query's admitted rows: two rows have an fp32 minimum of at most
    T2 + e, so the winner and the runner-up of the contract, and every row that ties with either, have a twin minimum of at most T2 + 2e.
    The rows within 4e of T2 are kept -- twice what the argument needs -- and shift_distances, every fmaf of it, runs over them alone, in
    ascending row order; fewer than two admitted rows are all kept.  The ties fall as in search(): the lowest row, then the lowest shift.
    stats: a dict that receives `kept` (rows kept, per query with a row) and `worst` (the largest |fp32 minimum - twin minimum| seen on a
    kept row), for the tests of the bound."""
    uq, mq = unit_columns(query)
    uc, mc = unit_columns(db)
    nq, nd, rings = len(uq), len(uc), uq.shape[1]
    twin = row_minima_twin(query, db)
    margin = 4 * e_bound(rings)
    idx, dist, shift, second = np.full(nq, -1, np.int32), np.full(nq, np.inf, np.float32), np.zeros(nq, np.int32), np.full(nq, np.inf, np.float32)
    kept_counts, worst = [], 0.0
    for i in range(nq):
        lim = nd if limit is None else min(int(limit[i]), nd)
        if lim <= 0:
            continue
        t = twin[i, :lim]
        kept = np.arange(lim) if lim < 2 else np.nonzero(t <= np.partition(t, 1)[1] + margin)[0]
        d = shift_distances(uq[i], mq[i], uc[kept], mc[kept])
        per_row, per_shift = d.min(axis=1), d.argmin(axis=1)
        w = per_row.argmin()
        idx[i], dist[i], shift[i] = kept[w], per_row[w], per_shift[w]
        if lim > 1:
            second[i] = np.delete(per_row, w).min()
        kept_counts.append(len(kept))
        worst = max(worst, float(np.abs(per_row.astype(np.float64) - t[kept]).max()))
    if stats is not None:
        stats["kept"], stats["worst"] = np.array(kept_counts, np.int64), worst
    return idx, dist, shift, second


# ---- the planted places of the tests: a ground plane with boxes and pillars on it, and the same place seen again
def place(rng, n_points=2000, extent=60.0):
    """[n, 3] float32: about n_points points of a ground plane at z = -2 (a sensor two units above it) and a few dozen boxes and pillars."""
    n_ground = n_points // 2
    rho, phi = extent * np.sqrt(rng.uniform(0, 1, n_ground)), rng.uniform(0, 2 * np.pi, n_ground)
    parts = [np.stack([rho * np.cos(phi), rho * np.sin(phi), -2.0 + 0.02 * rng.normal(size=n_ground)], axis=1)]
    n_obj = int(rng.integers(24, 48))
    per = max((n_points - n_ground) // n_obj, 4)
    for _ in range(n_obj):
        r0, a0 = extent * np.sqrt(rng.uniform(0.01, 1)), rng.uniform(0, 2 * np.pi)
        size = rng.uniform(0.3, 4.0, 2) if rng.uniform() < 0.7 else np.full(2, 0.3)        # a box, or a pillar
        height = rng.uniform(0.5, 12.0)
        p = np.stack([r0 * np.cos(a0) + size[0] * rng.uniform(-1, 1, per), r0 * np.sin(a0) + size[1] * rng.uniform(-1, 1, per),
                      -2.0 + height * rng.uniform(0, 1, per) ** 0.3], axis=1)
        parts.append(p)
    return np.concatenate(parts).astype(np.float32)


def revisit(rng, cloud, sectors, k, shift_xy=0.5, noise=0.02):
    """The place seen again: turned counter-clockwise about z by k + 1/3 sectors, moved by shift_xy in a random planar direction, 2 cm of
    noise on every coordinate."""
    ang = (k + 1.0 / 3.0) * 2 * np.pi / sectors
    c, s = np.cos(ang), np.sin(ang)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    d = rng.uniform(0, 2 * np.pi)
    t = np.array([shift_xy * np.cos(d), shift_xy * np.sin(d), 0.0])
    return (np.asarray(cloud, np.float64) @ R.T + t + noise * rng.normal(size=cloud.shape)).astype(np.float32)
