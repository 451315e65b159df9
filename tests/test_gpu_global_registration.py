"""GPU suite, end to end: a start pose from descriptors alone.  A bumpy closed surface with analytic normals and a rotated, translated,
re-ordered copy of it go through mi_fpfh_features (k = 16), mi_feature_match (mutual) and mi_ransac_register; the pose must bring every
point to within max_distance of its true image."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, MAXD = 3000, 0.01


def bumpy(n):
    """(points, unit normals) float64 [n, 3]: the surface |p| = g(p / |p|), g(u) = 1 + 0.15 sin(3 ux + 1) + 0.1 cos(4 uy uz + 2 ux) + 0.08 sin(5 uz),
    sampled along a Fibonacci spiral of directions.  With F(p) = |p| - g(p / |p|) the normal is grad F = u - (I - u u^T) grad g(u) / |p|."""
    k = np.arange(n) + 0.5
    z = 1 - 2 * k / n
    phi = np.pi * (1 + 5 ** 0.5) * k
    u = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=1)
    ux, uy, uz = u.T
    g = 1 + 0.15 * np.sin(3 * ux + 1) + 0.1 * np.cos(4 * uy * uz + 2 * ux) + 0.08 * np.sin(5 * uz)
    s = -0.1 * np.sin(4 * uy * uz + 2 * ux)
    grad = np.stack([0.45 * np.cos(3 * ux + 1) + 2 * s, 4 * uz * s, 4 * uy * s + 0.4 * np.cos(5 * uz)], axis=1)
    tangential = grad - u * (grad * u).sum(axis=1, keepdims=True)
    nrm = u - tangential / g[:, None]
    return u * g[:, None], nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def test_a_pose_from_descriptors_alone(ctx, capi):
    """Measured on an MI355X (printed by the test): 2 832 of the 3 000 points are kept by the mutual filter and 2 762 of them, 97.5 %, are
    matched to their own image; 3 860 of 4 096 hypotheses are valid; 2 762 inliers, rmse 1.9e-7, the worst point 3.3e-7 from its true image
    against max_distance 0.01.  The wrong 2.5 % lie far from any consistent pose and are no inliers."""
    p, nr = bumpy(N)
    rng = np.random.default_rng(11)
    a = np.deg2rad(100.0)
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R0, t0 = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K, np.array([0.5, -1.0, 2.0])
    perm = rng.permutation(N)
    src, src_n = p.astype(np.float32), nr.astype(np.float32)
    tgt, tgt_n = (p @ R0.T + t0)[perm].astype(np.float32), (nr @ R0.T)[perm].astype(np.float32)
    inverse = np.argsort(perm)                            # source point i is target row inverse[i]
    fs, ft = ctx.fpfh_features(src, src_n, 16), ctx.fpfh_features(tgt, tgt_n, 16)
    idx = ctx.feature_match(fs, ft, mutual=True)
    kept = idx >= 0
    correct = kept & (idx == inverse)
    Rr, tr, inl, rmse, best, nvalid, mask = ctx.ransac_register(src, tgt, idx, capi.ransac_params(MAXD, hypotheses=4096, seed=3), want_mask=True)
    err = np.linalg.norm(src.astype(np.float64) @ Rr.astype(np.float64).T + tr - (src.astype(np.float64) @ R0.T + t0), axis=1)
    print("end to end: %d of %d points kept by the mutual filter, %d of them correct (%.1f %%); %d valid hypotheses of 4096, %d inliers, rmse %.2e, "
          "worst point %.2e against max_distance %g" % (kept.sum(), N, correct.sum(), 100.0 * correct.sum() / max(kept.sum(), 1), nvalid, inl, rmse, err.max(), MAXD))
    assert nvalid > 0 and inl >= 3
    assert err.max() <= MAXD
    assert (mask[correct] != 0).all()                     # every correct match is explained by the pose
