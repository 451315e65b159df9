"""What tests/test_gpu_mls.py and tests/test_mls_bound.py share: the main clouds of mi_mls_smooth's suite (the "surface", "volume" and
"offset" recipes of tests/test_gpu_iss.py), their radii, their separate query sets, the restatement of every main case (built once per
case, frozen, shared) and the constant K of the coordinate bound."""
import functools

import numpy as np

import mls_reference as M
from test_gpu_iss import clouds, frozen

RADIUS = {"surface": 0.9, "volume": 1.6, "offset": 0.9}
QUERIES = 500
PIVOT_CHECKED = 1e-6              # a query whose conditioning is below this is left out of the coordinate check
LEFT_OUT_SHARE = 0.01             # ... and at most this share of a main cloud's queries may be
# The coordinate bound is half an fp32 ulp of the reference value plus K (c + 8) 2^-53 radius / conditioning.  K = 4 x the worst ratio of
# the restatement's own spread between ascending and descending summation to that formula at K = 1 over every main case, which
# tests/test_mls_bound.py measures (1.41, on the volume cloud's normals) and holds K to; the factor 4 because the device's walk order is a third order.
K_BOUND = 5.7


@functools.lru_cache(maxsize=None)
def queries(name):
    """500 queries of their own: points of the cloud moved off it by a Gaussian of sigma 0.05"""
    rng = np.random.default_rng(211)
    cloud = clouds()[name]
    return frozen((cloud[rng.permutation(len(cloud))[:QUERIES]] + rng.normal(scale=0.05, size=(QUERIES, 3))).astype(np.float32))


@functools.lru_cache(maxsize=None)
def reference(name, separate, mode, order, descending=False):
    ref = M.smooth(clouds()[name], RADIUS[name], mode, queries=queries(name) if separate else None, order=order, descending=descending)
    return {k: frozen(v) for k, v in ref.items()}


def checked(ref, radius):
    """the queries of the coordinate check: fitted, and conditioned at or above PIVOT_CHECKED"""
    return (ref["status"] != M.UNTOUCHED) & (M.conditioning(ref, radius) >= PIVOT_CHECKED)
