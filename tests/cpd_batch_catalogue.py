"""The problems the batched-CPD suites run, generated from seeds: no fixture files.

A problem is a pair (moving cloud, fixed cloud) of icp_batch_catalogue.pair: two independent samples of one smooth seeded surface, the
moving one displaced by a small rigid motion and perturbed by noise.  Under the default CPD rules such a pair of 200 to 1 024 points stops
on sigma^2 <= eps = 1e-3 after 15 to 19 EM iterations (checked on the CPU oracle), all values finite."""
import numpy as np

from icp_batch_catalogue import ill_posed as icp_ill_posed
from icp_batch_catalogue import pair

SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1000, 1024)


def sizes_batch(seed=21000):
    """All 196 moving x fixed size combinations of SIZES."""
    return [pair(seed + 20 * i + j, m, n) for i, m in enumerate(SIZES) for j, n in enumerate(SIZES)]


def chunk_edge_sizes(edge):
    """The sizes on both sides of every change of the single path's chunk count (one chunk per 64 streamed points) up to the routing edge."""
    return [s for k in range(1, edge // 64 + 1) for s in (64 * k - 1, 64 * k)]


def chunk_edge_batch(edge, seed=23000):
    """Each edge size against itself, against a small and against a mid-sized cloud on the other side (the chunk counts of the two passes
    depend on one side each)."""
    out = []
    for j, s in enumerate(chunk_edge_sizes(edge)):
        other = (s, 100, 700)[j % 3]
        out.append(pair(seed + 2 * j, s, other))
        out.append(pair(seed + 2 * j + 1, other, s))
    return out


def rules_batch(seed=25000, count=40):
    """40 problems of mixed sizes between 200 and 1 024 points that converge under the default rules."""
    rng = np.random.default_rng(seed)
    return [pair(seed + 1 + k, int(rng.integers(200, 1025)), int(rng.integers(200, 1025))) for k in range(count)]


def small_batch(seed=27000, count=1500, lo=1, hi=256):
    rng = np.random.default_rng(seed)
    return [pair(seed + 1 + k, int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))) for k in range(count)]


def ill_posed():
    """(name, moving, fixed) within 1 024 points: planar, collinear, all points equal on one or both sides, offset 1e3."""
    keep = ("planar", "collinear", "collinear_moving_only", "all_equal", "all_equal_both", "offset_1e3")
    return [(name, b[:1024].copy(), a[:1024].copy()) for name, b, a in icp_ill_posed() if name in keep]
