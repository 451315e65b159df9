"""ctypes binding of libmislam.so -- the C ABI declared in include/mi_slam.h.

This module is plumbing for the Python-side callers in this repository (tests, bench.py, __graft_entry__): it passes host
numpy buffers straight through to the C entry points and adds nothing of its own.  There is deliberately no fallback: if
the shared library is missing, or no HIP device is usable, the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MISLAM_LIB") or os.path.join(_HERE, "libmislam.so")   # MISLAM_LIB: developer override (variant builds)

MI_OK = 0
MI_ERR_INVALID_ARG, MI_ERR_NO_DEVICE, MI_ERR_HIP, MI_ERR_RCCL, MI_ERR_STATE = -1, -2, -3, -4, -5
DIST_CPU_ROUNDING, DIST_FMA = 0, 1
COMPOSE_CPU_ADDITIVE, COMPOSE_EXACT = 0, 1
NN_AUTO, NN_BRUTEFORCE, NN_TREE, NN_GRID = 0, 1, 2, 3
SHARD_AUTO, SHARD_TARGET, SHARD_SOURCE = 0, 1, 2
SUM_EXACT, SUM_CPU_SEQUENTIAL = 0, 1
SIGMA2_EXACT, SIGMA2_CPU_SEQUENTIAL = 0, 1
ESTEP_DEFAULT, ESTEP_CPU_SEQUENTIAL = 0, 1
NN_INDEX_MIN_POINTS = 10000         # MI_NN_AUTO switches to the cell grid at this many fixed points (mi_slam.h MI_NN_INDEX_MIN_POINTS)
STOP_RUNNING, STOP_CONVERGED, STOP_MAX_ITERATIONS, STOP_NO_PAIRS, STOP_ERROR_INCREASED, STOP_TOLERANCE, STOP_SIGMA = range(7)
STOP_DEGENERATE = 7                 # MI_STOP_DEGENERATE (mi_icp_plane_register)
(KERNEL_NN, KERNEL_MOMENTS, KERNEL_SOLVE, KERNEL_TRANSFORM, KERNEL_FINALIZE, KERNEL_ALLREDUCE, KERNEL_CPD_DENOM,
 KERNEL_CPD_CONTRACT, KERNEL_CPD_MSTEP, KERNEL_CPD_FGT) = range(10)
KERNEL_NAMES = ["nn", "moments", "solve", "transform", "finalize", "allreduce", "cpd_denom", "cpd_contract", "cpd_mstep", "cpd_fgt"]
CPD_APPROX_NONE, CPD_APPROX_FULL, CPD_APPROX_HYBRID = 0, 1, 2
(CPD_ROUTE_EXACT_MFMA, CPD_ROUTE_EXACT_VALU, CPD_ROUTE_SEQUENTIAL, CPD_ROUTE_TRUNC_CULLED, CPD_ROUTE_TRUNC_EVERY_PAIR, CPD_ROUTE_FGT) = range(6)
UNIQUE_ID_BYTES = 128
EXCHANGE_MIN_U64, EXCHANGE_SUM_F64 = 0, 1
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int)      # mi_exchange_fn

# every symbol include/mi_slam.h declares (tests check that the library exports each of them)
EXPORTS = [
    "mi_abi_version", "mi_last_error", "mi_device_count", "mi_ctx_create", "mi_dist_unique_id", "mi_ctx_create_dist",
    "mi_ctx_create_exchange", "mi_runtime_info", "mi_ctx_preload", "mi_ctx_rank", "mi_dist_info", "mi_shard_range", "mi_source_share", "mi_pack_key", "mi_unpack_key", "mi_ctx_destroy", "mi_ctx_synchronize", "mi_icp_params_default", "mi_icp_params_cuda_slam",
    "mi_icp_register", "mi_icp_load", "mi_icp_reset", "mi_icp_run", "mi_icp_auto_batch", "mi_icp_result", "mi_icp_batch_route", "mi_icp_register_batch", "mi_nn_search", "mi_nn_search_ex", "mi_cross_moments", "mi_kabsch",
    "mi_transform_mse", "mi_cpd_params_default", "mi_cpd_register", "mi_cpd_batch_route", "mi_cpd_register_batch", "mi_cpd_sigma_squared", "mi_cpd_sigma_squared_mode", "mi_cpd_estep",
    "mi_cpd_estep_truncated", "mi_cpd_estep_fgt", "mi_fgt_kcenter", "mi_fgt_kcenter_guided", "mi_fgt_tables", "mi_nicp_params_default", "mi_nicp_register",
    "mi_prepare_params_default", "mi_prepare_cloud", "mi_voxel_index", "mi_voxel_downsample", "mi_voxel_downsample_times",
    "mi_knn_search", "mi_knn_search_times", "mi_estimate_normals", "mi_estimate_normals_times",
    "mi_outlier_params_default", "mi_remove_outliers", "mi_remove_outliers_times",
    "mi_iss_params_default", "mi_iss_keypoints", "mi_iss_keypoints_times",
    "mi_cluster_params_default", "mi_cluster_dbscan", "mi_cluster_dbscan_times",
    "mi_plane_params_default", "mi_icp_plane_register", "mi_plane_system", "mi_icp_plane_times",
    "mi_estimate_covariances", "mi_icp_gicp_register", "mi_gicp_system", "mi_icp_gicp_times",
    "mi_fpfh_features", "mi_fpfh_features_times",
    "mi_feature_match", "mi_feature_match_times",
    "mi_ransac_params_default", "mi_ransac_register", "mi_ransac_hypotheses", "mi_ransac_register_times",
    "mi_ndt_constants", "mi_ndt_voxels", "mi_ndt_params_default", "mi_ndt_register", "mi_ndt_system", "mi_ndt_times",
    "mi_cpd_mstep", "mi_profile_enable", "mi_profile_select", "mi_profile_reset", "mi_profile_get", "mi_icp_load_times", "mi_profile_search_stats", "mi_profile_search_phases", "mi_selftest_sort_pairs", "mi_selftest_cloud_range", "mi_selftest_fail_loads", "mi_selftest_live_buffers", "mi_selftest_icp_schedule", "mi_selftest_cpd_last", "mi_selftest_nicp_candidates", "mi_nn_kernel_name",
]


class IcpParams(C.Structure):
    _fields_ = [("eps", C.c_float), ("max_iterations", C.c_int), ("max_distance_squared", C.c_float),
                ("dist_mode", C.c_int), ("compose_mode", C.c_int), ("filter_pairs", C.c_int),
                ("abort_on_increase", C.c_int), ("sync_every", C.c_int), ("verbose", C.c_int), ("nn_mode", C.c_int),
                ("shard_mode", C.c_int), ("sum_mode", C.c_int), ("reserved", C.c_int * 4)]


class CpdParams(C.Structure):
    _fields_ = [("eps", C.c_float), ("weight", C.c_float), ("const_scale", C.c_int), ("max_iterations", C.c_int),
                ("tolerance", C.c_float), ("sigma2_init", C.c_float), ("sync_every", C.c_int), ("verbose", C.c_int),
                ("approximation", C.c_int), ("fgt_ratio_of_far_field", C.c_float), ("fgt_order_of_truncation", C.c_int),
                ("sigma2_mode", C.c_int), ("estep_mode", C.c_int), ("reserved", C.c_int * 3)]


class NicpParams(C.Structure):
    _fields_ = [("eps", C.c_float), ("max_repetitions", C.c_int), ("approximation", C.c_int), ("verbose", C.c_int),
                ("reserved", C.c_int * 4)]


class PrepareParams(C.Structure):
    _fields_ = [("has_spread", C.c_int), ("spread", C.c_float), ("noise_intensity", C.c_float), ("has_transform", C.c_int),
                ("rotation", C.c_float * 9), ("translation", C.c_float * 3), ("reserved", C.c_int * 4)]


class OutlierParams(C.Structure):
    _fields_ = [("method", C.c_int), ("dist_mode", C.c_int), ("k", C.c_int), ("std_ratio", C.c_float), ("radius", C.c_float),
                ("min_neighbours", C.c_int), ("reserved", C.c_int * 6)]


class OutlierStats(C.Structure):
    _fields_ = [("mean", C.c_double), ("stddev", C.c_double), ("threshold", C.c_double), ("kept", C.c_longlong), ("reserved", C.c_int * 4)]


class IssParams(C.Structure):
    _fields_ = [("salient_radius", C.c_float), ("non_max_radius", C.c_float), ("gamma_21", C.c_float), ("gamma_32", C.c_float),
                ("min_neighbours", C.c_int), ("dist_mode", C.c_int), ("reserved", C.c_int * 10)]


class ClusterParams(C.Structure):
    _fields_ = [("radius", C.c_float), ("min_points", C.c_int), ("min_cluster_size", C.c_int), ("max_cluster_size", C.c_int),
                ("dist_mode", C.c_int), ("reserved", C.c_int * 11)]


class PlaneParams(C.Structure):
    _fields_ = [("eps_rotation", C.c_float), ("eps_translation", C.c_float), ("max_iterations", C.c_int), ("max_distance_squared", C.c_float),
                ("dist_mode", C.c_int), ("sync_every", C.c_int), ("verbose", C.c_int), ("reserved", C.c_int * 9)]


class NdtParams(C.Structure):
    _fields_ = [("eps_rotation", C.c_float), ("eps_translation", C.c_float), ("max_iterations", C.c_int), ("neighbourhood", C.c_int),
                ("outlier_ratio", C.c_float), ("sync_every", C.c_int), ("verbose", C.c_int), ("reserved", C.c_int * 9)]


class MiSlamError(RuntimeError):
    pass


_lib = None
_f = C.POINTER(C.c_float)
_i = C.POINTER(C.c_int)
_u8 = C.POINTER(C.c_ubyte)


def lib():
    """Load libmislam.so (raises if it has not been built -- run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MiSlamError("libmislam.so not built at %s: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        _lib.mi_last_error.restype = C.c_char_p
        _lib.mi_ctx_destroy.restype = None
        _lib.mi_icp_params_default.restype = None
        _lib.mi_icp_params_cuda_slam.restype = None
        _lib.mi_cpd_params_default.restype = None
        _lib.mi_prepare_params_default.restype = None
        _lib.mi_pack_key.restype = C.c_ulonglong
        _lib.mi_pack_key.argtypes = [C.c_float, C.c_int]
        _lib.mi_unpack_key.restype = None
        _lib.mi_unpack_key.argtypes = [C.c_ulonglong, _f, _i]
    return _lib


def _check(rc):
    if rc != MI_OK:
        raise MiSlamError("libmislam error %d: %s" % (rc, lib().mi_last_error().decode()))


def _fp(a):
    return a.ctypes.data_as(_f)


def _cloud(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("cloud must be [n,3] float32")
    return a


def device_count():
    c = C.c_int(0)
    _check(lib().mi_device_count(C.byref(c)))
    return c.value


def icp_params(cuda_slam=False, **kw):
    p = IcpParams()
    (lib().mi_icp_params_cuda_slam if cuda_slam else lib().mi_icp_params_default)(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def cpd_params(**kw):
    p = CpdParams()
    lib().mi_cpd_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def nicp_params(**kw):
    p = NicpParams()
    lib().mi_nicp_params_default.restype = None
    lib().mi_nicp_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def fgt_tables(order):
    """Host-only: exponents (a, b, c) per monomial in the reference's graded order, C_k and the Horner slot (mi_fgt_tables)."""
    pd = C.c_int(0)
    _check(lib().mi_fgt_tables(int(order), None, None, None, C.byref(pd)))
    mono = np.empty(pd.value, np.uint32)
    ck = np.empty(pd.value, np.float32)
    slot = np.empty(pd.value, np.int32)
    _check(lib().mi_fgt_tables(int(order), mono.ctypes.data_as(C.POINTER(C.c_uint)), _fp(ck), slot.ctypes.data_as(_i), C.byref(pd)))
    exps = np.stack([mono & 0xff, (mono >> 8) & 0xff, (mono >> 16) & 0xff], axis=1).astype(np.int32)
    return exps, ck, slot


def shard_range(m_total, rank, world):
    lo, hi = C.c_int(0), C.c_int(0)
    _check(lib().mi_shard_range(m_total, rank, world, C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


class IcpBatchInfo(C.Structure):
    _fields_ = [("problems_batched", C.c_int), ("problems_fallback", C.c_int), ("launches", C.c_int), ("reserved", C.c_int * 5)]


def icp_batch_route(n_before, n_after, params):
    """1 if mi_icp_register_batch carries a problem of these sizes under these rules on the batched kernel, 0 if it takes the existing path."""
    f = lib().mi_icp_batch_route
    f.argtypes = [C.c_int, C.c_int, C.POINTER(IcpParams)]
    f.restype = C.c_int
    return f(int(n_before), int(n_after), C.byref(params))


def icp_register_batch_raw(handle, n_problems, before, before_range, after, after_range, params, out_T, iterations, error, stop_reason, info):
    """mi_icp_register_batch with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_icp_register_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    return f(handle, n_problems, before, before_range, after, after_range, params, out_T, iterations, error, stop_reason, info)


class CpdBatchInfo(C.Structure):
    _fields_ = [("problems_batched", C.c_int), ("problems_fallback", C.c_int), ("launches", C.c_int), ("reserved", C.c_int * 5)]


def cpd_batch_route(m_before, n_after, params):
    """1 if mi_cpd_register_batch carries a problem of these sizes under these rules on the batched kernel, 0 if it takes the existing path."""
    f = lib().mi_cpd_batch_route
    f.argtypes = [C.c_int, C.c_int, C.POINTER(CpdParams)]
    f.restype = C.c_int
    return f(int(m_before), int(n_after), C.byref(params))


def cpd_register_batch_raw(handle, n_problems, before, before_range, after, after_range, params, out_sR_t, out_scale, iterations, error, stop_reason,
                           info):
    """mi_cpd_register_batch with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_cpd_register_batch
    f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 11
    f.restype = C.c_int
    return f(handle, n_problems, before, before_range, after, after_range, params, out_sR_t, out_scale, iterations, error, stop_reason, info)


def _batch_arrays(befores, afters, before_range, after_range):
    """The two concatenated clouds and (B, 2) range tables of a batched call, from lists of clouds or from arrays plus ranges; checks
    that no range runs past its array (the C interface trusts the arrays to reach as far as the ranges say)."""
    if before_range is None:
        counts = [len(b) for b in befores]
        before_range = np.stack([np.cumsum([0] + counts[:-1]), counts], axis=1) if counts else np.zeros((0, 2))
        befores = np.concatenate([_cloud(b) for b in befores]) if counts else np.zeros((0, 3), np.float32)
    if after_range is None:
        counts = [len(a) for a in afters]
        after_range = np.stack([np.cumsum([0] + counts[:-1]), counts], axis=1) if counts else np.zeros((0, 2))
        afters = np.concatenate([_cloud(a) for a in afters]) if counts else np.zeros((0, 3), np.float32)
    before, after = _cloud(befores), _cloud(afters)
    br = np.ascontiguousarray(before_range, np.int32).reshape(-1, 2)
    ar = np.ascontiguousarray(after_range, np.int32).reshape(-1, 2)
    if len(br) != len(ar):
        raise ValueError("before_range and after_range must name the same number of problems")
    for name, r, n in (("before", br, len(before)), ("after", ar, len(after))):
        for k in range(len(br)):
            if r[k, 0] >= 0 and r[k, 1] >= 0 and int(r[k, 0]) + int(r[k, 1]) > n:
                raise MiSlamError("libmislam error %d: problem %d: %s range %d + %d runs past the array (%d points)"
                                  % (MI_ERR_INVALID_ARG, k, name, r[k, 0], r[k, 1], n))
    return before, br, after, ar


def voxel_index_raw(p, origin, voxel, out):
    """mi_voxel_index with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_voxel_index
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    f.restype = C.c_int
    return f(p, origin, voxel, out)


def voxel_index(p, origin, voxel):
    """The voxel a point falls in (mi_voxel_index, host only): int32 [3] = floor((p - origin) / voxel) in fp32."""
    p = np.ascontiguousarray(p, np.float32).reshape(3)
    origin = np.ascontiguousarray(origin, np.float32).reshape(3)
    out = np.zeros(3, np.int32)
    _check(voxel_index_raw(p.ctypes.data, origin.ctypes.data, float(voxel), out.ctypes.data))
    return out


def voxel_downsample_raw(handle, xyz, n, voxel, origin, out_xyz, out_n, out_count, out_coord, voxel_of_point):
    """mi_voxel_downsample with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_voxel_downsample
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float] + [C.c_void_p] * 6
    f.restype = C.c_int
    return f(handle, xyz, n, voxel, origin, out_xyz, out_n, out_count, out_coord, voxel_of_point)


KNN_MAX_K = 32                      # MI_KNN_MAX_K


def knn_search_raw(handle, query, n, cloud, m, k, dist_mode, max_d2, idx, d2, count):
    """mi_knn_search with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_knn_search
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    return f(handle, query, n, cloud, m, k, dist_mode, max_d2, idx, d2, count)


def estimate_normals_raw(handle, cloud, n, k, dist_mode, max_d2, viewpoint, normals, curvature, count):
    """mi_estimate_normals with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_estimate_normals
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    return f(handle, cloud, n, k, dist_mode, max_d2, viewpoint, normals, curvature, count)


OUTLIER_STATISTICAL, OUTLIER_RADIUS = 0, 1     # MI_OUTLIER_*


def outlier_params(**kw):
    """mi_outlier_params at its defaults (statistical, k = 16, std_ratio = 2, CPU rounding) with the given fields set."""
    p = OutlierParams()
    lib().mi_outlier_params_default.restype = None
    lib().mi_outlier_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def remove_outliers_raw(handle, cloud, n, params, out_xyz, out_index, out_n, keep, mean_distance, neighbours, stats):
    """mi_remove_outliers with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_remove_outliers
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8
    f.restype = C.c_int
    return f(handle, cloud, n, params, out_xyz, out_index, out_n, keep, mean_distance, neighbours, stats)


def iss_params(**kw):
    """mi_iss_params at its defaults (gamma 0.975 and 0.975, min_neighbours 5, CPU rounding; both radii 0: set them) with the given fields set."""
    p = IssParams()
    lib().mi_iss_params_default.restype = None
    lib().mi_iss_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def iss_keypoints_raw(handle, cloud, n, params, out_xyz, out_index, out_n, is_keypoint, saliency, eigenvalues, neighbours):
    """mi_iss_keypoints with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_iss_keypoints
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8
    f.restype = C.c_int
    return f(handle, cloud, n, params, out_xyz, out_index, out_n, is_keypoint, saliency, eigenvalues, neighbours)


def cluster_params(**kw):
    """mi_cluster_params at its defaults (min_points 1, min_cluster_size 1, no upper limit, CPU rounding; radius 0: set it) with the given fields set."""
    p = ClusterParams()
    lib().mi_cluster_params_default.restype = None
    lib().mi_cluster_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def cluster_dbscan_raw(handle, cloud, n, params, labels, n_clusters, cluster_sizes, cluster_cap, is_core, grouped_index, n_grouped):
    """mi_cluster_dbscan with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_cluster_dbscan
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3
    f.restype = C.c_int
    return f(handle, cloud, n, params, labels, n_clusters, cluster_sizes, cluster_cap, is_core, grouped_index, n_grouped)


def plane_params(**kw):
    """mi_plane_params at its defaults (eps 1e-6 and 1e-6, 50 iterations, no distance limit, CPU rounding) with the given fields set."""
    p = PlaneParams()
    lib().mi_plane_params_default.restype = None
    lib().mi_plane_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def icp_plane_register_raw(handle, before, n, after, normals, m, params, init_T, out_T, iterations, error, stop_reason):
    """mi_icp_plane_register with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_icp_plane_register
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    f.restype = C.c_int
    return f(handle, before, n, after, normals, m, params, init_T, out_T, iterations, error, stop_reason)


def plane_system_raw(handle, before, n, after, normals, m, T, dist_mode, max_d2, out_sums, out_centre, out_idx):
    """mi_plane_system with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_plane_system
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    return f(handle, before, n, after, normals, m, T, dist_mode, max_d2, out_sums, out_centre, out_idx)


COV_RAW, COV_PLANE = 0, 1     # MI_COV_*


def estimate_covariances_raw(handle, cloud, n, k, dist_mode, max_d2, mode, epsilon, cov6, count):
    """mi_estimate_covariances with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_estimate_covariances
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    return f(handle, cloud, n, k, dist_mode, max_d2, mode, epsilon, cov6, count)


def icp_gicp_register_raw(handle, before, before_cov, n, after, after_cov, m, params, init_T, out_T, iterations, error, stop_reason):
    """mi_icp_gicp_register with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_icp_gicp_register
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    f.restype = C.c_int
    return f(handle, before, before_cov, n, after, after_cov, m, params, init_T, out_T, iterations, error, stop_reason)


def gicp_system_raw(handle, before, before_cov, n, after, after_cov, m, T, dist_mode, max_d2, out_sums, out_centre, out_idx):
    """mi_gicp_system with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_gicp_system
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    return f(handle, before, before_cov, n, after, after_cov, m, T, dist_mode, max_d2, out_sums, out_centre, out_idx)


def icp_gicp_times_raw(handle, out_ms):
    """mi_icp_gicp_times with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_icp_gicp_times
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p], C.c_int
    return f(handle, out_ms)


def ndt_params(**kw):
    """mi_ndt_params with the library's defaults, then the given fields"""
    p = NdtParams()
    lib().mi_ndt_params_default.restype = None
    lib().mi_ndt_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def ndt_constants_raw(voxel, outlier_ratio, out):
    """mi_ndt_constants with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_ndt_constants
    f.argtypes, f.restype = [C.c_float, C.c_float, C.c_void_p], C.c_int
    return f(voxel, outlier_ratio, out)


def ndt_constants(voxel, outlier_ratio=0.55):
    """(d1, d2, h, k) of the NDT score as float64 [4] (mi_ndt_constants, host only)"""
    out = np.zeros(4, np.float64)
    _check(ndt_constants_raw(float(voxel), float(outlier_ratio), out.ctypes.data))
    return out


def ndt_voxels_raw(handle, xyz, n, voxel, origin, min_points, eig_ratio, out_coord, out_mean, out_icov, out_n, out_count, out_cov, out_origin):
    """mi_ndt_voxels with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_ndt_voxels
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_float] + [C.c_void_p] * 7
    f.restype = C.c_int
    return f(handle, xyz, n, voxel, origin, min_points, eig_ratio, out_coord, out_mean, out_icov, out_n, out_count, out_cov, out_origin)


def ndt_register_raw(handle, before, n, coord, mean, icov, nv, voxel, origin, params, init_T, out_T, iterations, score, stop_reason):
    """mi_ndt_register with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_ndt_register
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float] + [C.c_void_p] * 7
    f.restype = C.c_int
    return f(handle, before, n, coord, mean, icov, nv, voxel, origin, params, init_T, out_T, iterations, score, stop_reason)


def ndt_system_raw(handle, before, n, coord, mean, icov, nv, voxel, origin, T, neighbourhood, outlier_ratio, out_sums, out_centre, out_idx, out_terms):
    """mi_ndt_system with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_ndt_system
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_float] + [C.c_void_p] * 4
    f.restype = C.c_int
    return f(handle, before, n, coord, mean, icov, nv, voxel, origin, T, neighbourhood, outlier_ratio, out_sums, out_centre, out_idx, out_terms)


def ndt_times_raw(handle, out_ms):
    """mi_ndt_times with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_ndt_times
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p], C.c_int
    return f(handle, out_ms)


FPFH_BINS, FPFH_DIM = 11, 33     # MI_FPFH_BINS, MI_FPFH_DIM


def fpfh_features_raw(handle, cloud, normals, n, k, dist_mode, max_d2, fpfh, counts, count):
    """mi_fpfh_features with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_fpfh_features
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    return f(handle, cloud, normals, n, k, dist_mode, max_d2, fpfh, counts, count)


def fpfh_features_times_raw(handle, out_ms):
    """mi_fpfh_features_times with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_fpfh_features_times
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p], C.c_int
    return f(handle, out_ms)


FEATURE_MAX_DIM = 64             # MI_FEATURE_MAX_DIM


def feature_match_raw(handle, query, n, target, m, dim, mutual, idx, d2):
    """mi_feature_match with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_feature_match
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    return f(handle, query, n, target, m, dim, mutual, idx, d2)


def feature_match_times_raw(handle, out_ms):
    """mi_feature_match_times with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_feature_match_times
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p], C.c_int
    return f(handle, out_ms)


class RansacParams(C.Structure):
    _fields_ = [("hypotheses", C.c_int), ("seed", C.c_ulonglong), ("max_distance", C.c_float), ("edge_similarity", C.c_float),
                ("refine_iterations", C.c_int), ("reserved", C.c_int * 8)]


def ransac_params(max_distance, **kw):
    """mi_ransac_params_default with max_distance and any other field set: hypotheses, seed, edge_similarity, refine_iterations."""
    p = RansacParams()
    f = lib().mi_ransac_params_default
    f.argtypes, f.restype = [C.c_void_p], None
    f(C.byref(p))
    p.max_distance = max_distance
    for k, v in kw.items():
        if k not in ("hypotheses", "seed", "edge_similarity", "refine_iterations"):
            raise TypeError("mi_ransac_params has no field %r" % k)
        setattr(p, k, v)
    return p


def ransac_register_raw(handle, src, n, tgt, m, idx, params, R9, t3, inliers, rmse, best, nvalid, mask):
    """mi_ransac_register with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_ransac_register
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 9
    f.restype = C.c_int
    return f(handle, src, n, tgt, m, idx, params, R9, t3, inliers, rmse, best, nvalid, mask)


def ransac_hypotheses_raw(handle, src, n, tgt, m, idx, params, first, count, triples, valid, pose12, inlier_count):
    """mi_ransac_hypotheses with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_ransac_hypotheses
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
    f.restype = C.c_int
    return f(handle, src, n, tgt, m, idx, params, first, count, triples, valid, pose12, inlier_count)


def ransac_register_times_raw(handle, out_ms):
    """mi_ransac_register_times with ctypes pointers (or None) as given: returns the error code, raises nothing."""
    f = lib().mi_ransac_register_times
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p], C.c_int
    return f(handle, out_ms)


def _cov6(a, points):
    a = np.ascontiguousarray(a, np.float32)
    if a.shape != (points, 6):
        raise ValueError("covariances are [points, 6]: xx, xy, xz, yy, yz, zz per point")
    return a


def _T16(T):
    """A transform as the C interface takes it: None, or 16 float32 column-major from a [4, 4] array indexed [row, col]."""
    if T is None:
        return None
    T = np.asarray(T, np.float32)
    if T.shape != (4, 4):
        raise ValueError("a transform is a [4, 4] array indexed [row, col]")
    return np.ascontiguousarray(T.T).reshape(16)


def icp_auto_batch(n_moving_total, m_fixed_total, world, source_sharded, every_pair_search):
    """Iterations mi_icp_run enqueues between host checks with sync_every = 0: a function of global sizes only."""
    f = lib().mi_icp_auto_batch
    f.argtypes = [C.c_longlong, C.c_longlong, C.c_int, C.c_int, C.c_int]
    return int(f(n_moving_total, m_fixed_total, world, 1 if source_sharded else 0, 1 if every_pair_search else 0))


def source_share(n_total, rank, world):
    """Moving points rank `rank` works on under SHARD_SOURCE."""
    cnt = C.c_int(0)
    _check(lib().mi_source_share(n_total, rank, world, C.byref(cnt)))
    return cnt.value


def pack_key(d2, index):
    return int(lib().mi_pack_key(float(d2), int(index)))


def unpack_key(key):
    d2, idx = C.c_float(0), C.c_int(0)
    lib().mi_unpack_key(C.c_ulonglong(key), C.byref(d2), C.byref(idx))
    return d2.value, idx.value


def selftest_cloud_range_raw(ctx, xyz, n, check, out_lo_hi, out_first_bad):
    """mi_selftest_cloud_range with raw pointers -> its return code."""
    f = lib().mi_selftest_cloud_range
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    return f(ctx, xyz, n, check, out_lo_hi, out_first_bad)


def selftest_live_buffers():
    """Device buffers of the library alive in this process (mi_selftest_live_buffers)."""
    n = C.c_longlong(0)
    _check(lib().mi_selftest_live_buffers(C.byref(n)))
    return n.value


def dist_unique_id():
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    _check(lib().mi_dist_unique_id(buf))
    return buf.raw


def runtime_info():
    """{hip_path, rccl_path, hip_runtime_version, rccl_version}: the shared objects libmislam.so's HIP / RCCL calls bind to in this
    process (mi_runtime_info; no device touched)."""
    hip, rccl = C.create_string_buffer(1024), C.create_string_buffer(1024)
    hv, rv = C.c_int(0), C.c_int(0)
    _check(lib().mi_runtime_info(hip, rccl, 1024, C.byref(hv), C.byref(rv)))
    return {"hip_path": hip.value.decode(), "rccl_path": rccl.value.decode(), "hip_runtime_version": hv.value, "rccl_version": rv.value}


def _T_to_Rt(T):
    M = np.array(T, dtype=np.float32).reshape(4, 4).T   # column-major -> M[row, col]
    return M[:3, :3].copy(), M[:3, 3].copy()


class Context:
    """mi_ctx handle.  Context(device), Context(device, rank, world, unique_id) for the multi-GPU path over RCCL, or
    Context(device, rank, world, exchange=fn) for the same path over the caller's transport: fn(array, kind) combines the
    numpy array (uint64 for EXCHANGE_MIN_U64, float64 for EXCHANGE_SUM_F64) in place across the ranks."""

    def __init__(self, device=0, rank=None, world=None, unique_id=None, exchange=None):
        self._h = C.c_void_p()
        self._exchange_cb = None
        if world is None:
            _check(lib().mi_ctx_create(device, C.byref(self._h)))
        elif exchange is not None:
            def trampoline(_user, buf, count, kind):
                try:
                    ctype = C.c_uint64 if kind == EXCHANGE_MIN_U64 else C.c_double
                    exchange(np.ctypeslib.as_array(C.cast(buf, C.POINTER(ctype)), shape=(count,)), kind)
                    return 0
                except Exception:       # an exception must not unwind through the C frames
                    import traceback
                    traceback.print_exc()
                    return 1
            self._exchange_cb = EXCHANGE_FN(trampoline)      # kept alive with the context
            _check(lib().mi_ctx_create_exchange(device, rank, world, self._exchange_cb, None, C.byref(self._h)))
        else:
            _check(lib().mi_ctx_create_dist(device, rank, world, unique_id, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().mi_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(lib().mi_ctx_synchronize(self._h))

    def preload(self):
        """Load all device code now instead of lazily inside the first calls (mi_ctx_preload)."""
        _check(lib().mi_ctx_preload(self._h))

    def rank_world(self):
        r, w = C.c_int(0), C.c_int(0)
        _check(lib().mi_ctx_rank(self._h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def dist_info(self):
        """(nranks, rank) as the transport reports them and the bit mask of ranks seen in one all-reduce (collective call)."""
        n, r, seen = C.c_int(0), C.c_int(0), C.c_ulonglong(0)
        _check(lib().mi_dist_info(self._h, C.byref(n), C.byref(r), C.byref(seen)))
        return n.value, r.value, int(seen.value)

    # ---- ICP
    def icp_register(self, before, after, params):
        before, after = _cloud(before), _cloud(after)
        T = (C.c_float * 16)()
        it, err = C.c_int(0), C.c_float(0)
        _check(lib().mi_icp_register(self._h, _fp(before), before.shape[0], _fp(after), after.shape[0], C.byref(params), T,
                                     C.byref(it), C.byref(err)))
        R, t = _T_to_Rt(T)
        return R, t, it.value, err.value

    def icp_register_batch(self, befores, afters, params, before_range=None, after_range=None):
        """B registrations under one set of rules (mi_icp_register_batch).  befores / afters: two lists of (n, 3) arrays -- or two
        (N, 3) arrays plus before_range / after_range, (B, 2) integer arrays of (first point, count).  Returns (R [B,3,3], t [B,3],
        iterations [B], error [B], stop_reason [B], info)."""
        before, br, after, ar = _batch_arrays(befores, afters, before_range, after_range)
        B = len(br)
        T = np.zeros((B, 16), np.float32)
        it, why = np.zeros(B, np.int32), np.zeros(B, np.int32)
        err = np.zeros(B, np.float32)
        info = IcpBatchInfo()
        _check(icp_register_batch_raw(self._h, B, before.ctypes.data, br.ctypes.data, after.ctypes.data, ar.ctypes.data,
                                      C.addressof(params), T.ctypes.data, it.ctypes.data, err.ctypes.data, why.ctypes.data,
                                      C.addressof(info)))
        M = T.reshape(B, 4, 4).transpose(0, 2, 1)        # column-major 4x4 -> [row, col]
        return M[:, :3, :3].copy(), M[:, :3, 3].copy(), it, err, why, info

    def cpd_register_batch(self, befores, afters, params, before_range=None, after_range=None):
        """B CPD registrations under one set of rules (mi_cpd_register_batch).  befores / afters: two lists of (n, 3) arrays -- or two
        (N, 3) arrays plus before_range / after_range, (B, 2) integer arrays of (first point, count).  Returns (sR [B,3,3], t [B,3],
        scale [B], iterations [B], error [B], stop_reason [B], info)."""
        before, br, after, ar = _batch_arrays(befores, afters, before_range, after_range)
        B = len(br)
        T = np.zeros((B, 16), np.float32)
        it, why = np.zeros(B, np.int32), np.zeros(B, np.int32)
        err, scale = np.zeros(B, np.float32), np.zeros(B, np.float32)
        info = CpdBatchInfo()
        _check(cpd_register_batch_raw(self._h, B, before.ctypes.data, br.ctypes.data, after.ctypes.data, ar.ctypes.data,
                                      C.addressof(params), T.ctypes.data, scale.ctypes.data, it.ctypes.data, err.ctypes.data,
                                      why.ctypes.data, C.addressof(info)))
        M = T.reshape(B, 4, 4).transpose(0, 2, 1)        # column-major 4x4 -> [row, col]
        return M[:, :3, :3].copy(), M[:, :3, 3].copy(), scale, it, err, why, info

    def icp_load(self, before, after, params):
        before, after = _cloud(before), _cloud(after)
        _check(lib().mi_icp_load(self._h, _fp(before), before.shape[0], _fp(after), after.shape[0], C.byref(params)))

    def icp_reset(self):
        _check(lib().mi_icp_reset(self._h))

    def icp_run(self, max_new_iterations):
        done = C.c_int(0)
        _check(lib().mi_icp_run(self._h, max_new_iterations, C.byref(done)))
        return done.value

    def icp_result(self):
        T = (C.c_float * 16)()
        it, err, why = C.c_int(0), C.c_float(0), C.c_int(0)
        _check(lib().mi_icp_result(self._h, T, C.byref(it), C.byref(err), C.byref(why)))
        R, t = _T_to_Rt(T)
        return R, t, it.value, err.value, why.value

    # ---- primitives
    def nn_search(self, src, tgt, dist_mode=DIST_CPU_ROUNDING, nn_mode=NN_AUTO):
        src, tgt = _cloud(src), _cloud(tgt)
        n = src.shape[0]
        idx = np.empty(n, np.int32)
        d2 = np.empty(n, np.float32)
        _check(lib().mi_nn_search_ex(self._h, _fp(src), n, _fp(tgt), tgt.shape[0], dist_mode, nn_mode,
                                     idx.ctypes.data_as(_i), _fp(d2)))
        return idx, d2

    def kabsch(self, src, tgt, idx, keep=None):
        src, tgt = _cloud(src), _cloud(tgt)
        idx = np.ascontiguousarray(idx, np.int32)
        kp = None
        if keep is not None:
            keep = np.ascontiguousarray(keep, np.uint8)
            kp = keep.ctypes.data_as(_u8)
        R9 = (C.c_float * 9)()
        t3 = (C.c_float * 3)()
        used = C.c_int(0)
        _check(lib().mi_kabsch(self._h, _fp(src), src.shape[0], _fp(tgt), tgt.shape[0], idx.ctypes.data_as(_i), kp, R9, t3,
                               C.byref(used)))
        return np.array(R9, np.float32).reshape(3, 3).T.copy(), np.array(t3, np.float32), used.value

    def cross_moments(self, src, tgt, idx, keep=None):
        """{pairs, sum src, sum tgt, sum tgt_r src_c} over the kept pairs (src[i], tgt[idx[i]]), fp64."""
        src, tgt = _cloud(src), _cloud(tgt)
        idx = np.ascontiguousarray(idx, np.int32)
        kp = None
        if keep is not None:
            keep = np.ascontiguousarray(keep, np.uint8)
            kp = keep.ctypes.data_as(_u8)
        out = (C.c_double * 16)()
        _check(lib().mi_cross_moments(self._h, _fp(src), src.shape[0], _fp(tgt), tgt.shape[0], idx.ctypes.data_as(_i), kp, out))
        return np.array(out, np.float64)

    def transform_mse(self, src, R, t, tgt=None, idx=None, keep=None, divide_by_pairs=True, want_cloud=True):
        src = _cloud(src)
        n = src.shape[0]
        R9 = np.ascontiguousarray(np.asarray(R, np.float32).T).reshape(9)
        t3 = np.ascontiguousarray(t, np.float32)
        out = np.empty((n, 3), np.float32) if want_cloud else None
        mse = C.c_float(0)
        tp, m, ip, kp = None, 0, None, None
        if tgt is not None:
            tgt = _cloud(tgt)
            tp, m = _fp(tgt), tgt.shape[0]
            idx = np.ascontiguousarray(idx, np.int32)
            ip = idx.ctypes.data_as(_i)
            if keep is not None:
                keep = np.ascontiguousarray(keep, np.uint8)
                kp = keep.ctypes.data_as(_u8)
        _check(lib().mi_transform_mse(self._h, _fp(src), n, _fp(R9), _fp(t3), tp, m, ip, kp, 1 if divide_by_pairs else 0,
                                      _fp(out) if want_cloud else None, C.byref(mse) if tgt is not None else None))
        return out, (mse.value if tgt is not None else None)

    # ---- CPD
    def cpd_register(self, before, after, params):
        before, after = _cloud(before), _cloud(after)
        T = (C.c_float * 16)()
        it, err, sc = C.c_int(0), C.c_float(0), C.c_float(0)
        _check(lib().mi_cpd_register(self._h, _fp(before), before.shape[0], _fp(after), after.shape[0], C.byref(params), T,
                                     C.byref(sc), C.byref(it), C.byref(err)))
        sR, t = _T_to_Rt(T)
        return sR, t, sc.value, it.value, err.value

    def cpd_sigma_squared(self, before, after, mode=SIGMA2_EXACT):
        before, after = _cloud(before), _cloud(after)
        s = C.c_float(0)
        _check(lib().mi_cpd_sigma_squared_mode(self._h, _fp(before), before.shape[0], _fp(after), after.shape[0], mode, C.byref(s)))
        return s.value

    def cpd_estep(self, y, x, constant, sigma2):
        y, x = _cloud(y), _cloud(x)
        m, n = y.shape[0], x.shape[0]
        p1 = np.empty(m, np.float32)
        pt1 = np.empty(n, np.float32)
        px = np.empty((m, 3), np.float32)
        L = C.c_float(0)
        _check(lib().mi_cpd_estep(self._h, _fp(y), m, _fp(x), n, C.c_float(constant), C.c_float(sigma2), _fp(p1), _fp(pt1),
                                  _fp(px), C.byref(L)))
        return p1, pt1, px, L.value

    def cpd_estep_truncated(self, y, x, constant, sigma2, truncate=1e-3):
        y, x = _cloud(y), _cloud(x)
        m, n = y.shape[0], x.shape[0]
        p1, pt1, px, L = np.empty(m, np.float32), np.empty(n, np.float32), np.empty((m, 3), np.float32), C.c_float(0)
        _check(lib().mi_cpd_estep_truncated(self._h, _fp(y), m, _fp(x), n, C.c_float(constant), C.c_float(sigma2),
                                            C.c_float(truncate), _fp(p1), _fp(pt1), _fp(px), C.byref(L)))
        return p1, pt1, px, L.value

    def cpd_estep_fgt(self, y, x, weight, sigma2, sigma2_init, ratio_of_far_field=10.0, order_of_truncation=8):
        y, x = _cloud(y), _cloud(x)
        m, n = y.shape[0], x.shape[0]
        p1, pt1, px, L = np.empty(m, np.float32), np.empty(n, np.float32), np.empty((m, 3), np.float32), C.c_float(0)
        _check(lib().mi_cpd_estep_fgt(self._h, _fp(y), m, _fp(x), n, C.c_float(weight), C.c_float(sigma2), C.c_float(sigma2_init),
                                      C.c_float(ratio_of_far_field), int(order_of_truncation), _fp(p1), _fp(pt1), _fp(px),
                                      C.byref(L)))
        return p1, pt1, px, L.value

    def fgt_kcenter(self, cloud, K):
        cloud = _cloud(cloud)
        centers = np.empty((K, 3), np.float32)
        cluster = np.empty(cloud.shape[0], np.int32)
        _check(lib().mi_fgt_kcenter(self._h, _fp(cloud), cloud.shape[0], int(K), _fp(centers), cluster.ctypes.data_as(_i)))
        return centers, cluster

    def fgt_kcenter_guided(self, cloud, K, guess):
        """-> centers, cluster, picked (the sweep's choices), verified (leading entries of `guess` that were the sweep's own; -1: no replay)"""
        cloud = _cloud(cloud)
        guess = np.ascontiguousarray(guess, np.int32)
        centers = np.empty((K, 3), np.float32)
        cluster = np.empty(cloud.shape[0], np.int32)
        picked = np.empty(K, np.int32)
        verified = C.c_int(-2)
        _check(lib().mi_fgt_kcenter_guided(self._h, _fp(cloud), cloud.shape[0], int(K), guess.ctypes.data_as(_i), int(guess.shape[0]), _fp(centers),
                                           cluster.ctypes.data_as(_i), picked.ctypes.data_as(_i), C.byref(verified)))
        return centers, cluster, picked, verified.value

    def cpd_mstep(self, before, after, p1, pt1, px, const_scale, scale=1.0, sigma2=0.0):
        before, after = _cloud(before), _cloud(after)
        p1 = np.ascontiguousarray(p1, np.float32)
        pt1 = np.ascontiguousarray(pt1, np.float32)
        px = np.ascontiguousarray(px, np.float32)
        R9 = (C.c_float * 9)()
        t3 = (C.c_float * 3)()
        s, s2 = C.c_float(scale), C.c_float(sigma2)
        _check(lib().mi_cpd_mstep(self._h, _fp(before), before.shape[0], _fp(after), after.shape[0], _fp(p1), _fp(pt1), _fp(px),
                                  1 if const_scale else 0, R9, t3, C.byref(s), C.byref(s2)))
        return np.array(R9, np.float32).reshape(3, 3).T.copy(), np.array(t3, np.float32), s.value, s2.value

    # ---- NICP
    def nicp_register(self, before, after, params, order_heads, subcloud_idx=None):
        """order_heads: [repetitions, 3] int32 (first three entries of each repetition's permutation); subcloud_idx None = whole cloud."""
        before, after = _cloud(before), _cloud(after)
        heads = np.ascontiguousarray(order_heads, np.int32)
        reps = 20 if params.max_repetitions == -1 else params.max_repetitions
        if heads.shape != (reps, 3):
            raise ValueError("order_heads must be [%d, 3]" % reps)
        if subcloud_idx is not None:
            subcloud_idx = np.ascontiguousarray(subcloud_idx, np.int32)
        sn = before.shape[0] if subcloud_idx is None else len(subcloud_idx)
        T = (C.c_float * 16)()
        it, err = C.c_int(0), C.c_float(0)
        _check(lib().mi_nicp_register(self._h, _fp(before), before.shape[0], _fp(after), after.shape[0], C.byref(params),
                                      heads.ctypes.data_as(_i), subcloud_idx.ctypes.data_as(_i) if subcloud_idx is not None else None,
                                      sn, T, C.byref(it), C.byref(err)))
        R, t = _T_to_Rt(T)
        return R, t, it.value, err.value

    # ---- input stage
    def prepare_cloud(self, raw, subcloud_idx=None, shuffle_idx=None, noise_rows=None, noise_unit=None, noise_intensity=0.0,
                      outlier_unit=None, spread=None, R=None, t=None):
        """GetCloudsFromConfig's stages for one cloud (mi_prepare_cloud).  R (3x3, row = output component), t: the known
        transformation, or None.  Returns the prepared cloud [(size + outliers), 3]."""
        raw = _cloud(raw)
        opt_i = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
        opt_f = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1)
        sub, shuf, rows, nu, ou = opt_i(subcloud_idx), opt_i(shuffle_idx), opt_i(noise_rows), opt_f(noise_unit), opt_f(outlier_unit)
        n = raw.shape[0] if sub is None else len(sub)
        if shuf is not None and len(shuf) != n:
            raise ValueError("shuffle_idx must have %d entries" % n)
        n_noise = 0 if rows is None else len(rows)
        if n_noise and (nu is None or len(nu) != 3 * n_noise):
            raise ValueError("noise_unit must be [%d, 3]" % n_noise)
        n_out = 0 if ou is None else len(ou) // 3
        p = PrepareParams()
        lib().mi_prepare_params_default(C.byref(p))
        if spread is not None:
            p.has_spread, p.spread = 1, spread
        p.noise_intensity = noise_intensity
        if R is not None:
            p.has_transform = 1
            p.rotation[:] = np.asarray(R, np.float32).T.reshape(9).tolist()        # column-major
            p.translation[:] = np.asarray(t, np.float32).tolist()
        out = np.empty((n + n_out, 3), np.float32)
        got = C.c_int(0)
        ip = lambda a: None if a is None else a.ctypes.data_as(_i)
        fp = lambda a: None if a is None else _fp(a)
        _check(lib().mi_prepare_cloud(self._h, _fp(raw), raw.shape[0], ip(sub), n, ip(shuf), ip(rows), fp(nu), n_noise, fp(ou), n_out,
                                      C.byref(p), _fp(out), C.byref(got)))
        assert got.value == n + n_out
        return out

    # ---- voxel-grid downsampling
    def voxel_downsample(self, xyz, voxel, origin=None, want_counts=False, want_coords=False, want_map=False):
        """Voxel-grid centroids (mi_voxel_downsample): one row per occupied voxel, ascending by (cz, cy, cx).  Returns the centroids
        [rows, 3], followed by whatever was asked for, in this order: counts [rows], voxel coordinates [rows, 3], and the output row
        of every input point [n]."""
        xyz = _cloud(xyz)
        n = xyz.shape[0]
        op = None
        if origin is not None:
            origin = np.ascontiguousarray(origin, np.float32).reshape(3)
            op = origin.ctypes.data
        out = np.empty((n, 3), np.float32)
        counts = np.empty(n, np.int32) if want_counts else None
        coords = np.empty((n, 3), np.int32) if want_coords else None
        vmap = np.empty(n, np.int32) if want_map else None
        rows = C.c_int(0)
        ptr = lambda a: None if a is None else a.ctypes.data
        _check(voxel_downsample_raw(self._h, xyz.ctypes.data, n, float(voxel), op, out.ctypes.data, C.addressof(rows), ptr(counts), ptr(coords),
                                    ptr(vmap)))
        res = [out[:rows.value].copy()]
        if want_counts:
            res.append(counts[:rows.value].copy())
        if want_coords:
            res.append(coords[:rows.value].copy())
        if want_map:
            res.append(vmap)
        return res[0] if len(res) == 1 else tuple(res)

    def voxel_downsample_times(self):
        """ms per stage of the last voxel_downsample: workspace, upload, range, sort, sums, download, total (mi_voxel_downsample_times)."""
        out = (C.c_double * 8)()
        _check(lib().mi_voxel_downsample_times(self._h, out))
        return dict(zip(("workspace", "upload", "range", "sort", "sums", "download", "unused", "total"), list(out)))

    # ---- k nearest neighbours
    def knn_search(self, query, cloud, k, dist_mode=DIST_CPU_ROUNDING, max_d2=np.inf, want_d2=True, want_count=False):
        """Exact k nearest neighbours (mi_knn_search): idx [n, k] int32, ascending by (d2 bits, index), -1 in the slots no candidate
        filled; then d2 [n, k] (+inf there) and count [n] if asked for.  query None: the cloud's own points, neighbour i of row i
        skipped by index."""
        cloud = _cloud(cloud)
        m = cloud.shape[0]
        if query is None:
            n, qp = m, None
        else:
            query = _cloud(query)
            n, qp = query.shape[0], query.ctypes.data
        idx = np.empty((n, int(k)), np.int32)
        d2 = np.empty((n, int(k)), np.float32) if want_d2 else None
        count = np.empty(n, np.int32) if want_count else None
        ptr = lambda a: None if a is None else a.ctypes.data
        _check(knn_search_raw(self._h, qp, n, cloud.ctypes.data, m, int(k), int(dist_mode), float(max_d2), idx.ctypes.data, ptr(d2), ptr(count)))
        res = [idx] + ([d2] if want_d2 else []) + ([count] if want_count else [])
        return res[0] if len(res) == 1 else tuple(res)

    def knn_search_times(self):
        """ms per stage of the last knn_search: workspace, upload, check, grid, order, search, download, total (mi_knn_search_times)."""
        out = (C.c_double * 8)()
        _check(lib().mi_knn_search_times(self._h, out))
        return dict(zip(("workspace", "upload", "check", "grid", "order", "search", "download", "total"), list(out)))

    # ---- surface normals
    def estimate_normals(self, cloud, k, viewpoint=None, dist_mode=DIST_CPU_ROUNDING, max_d2=np.inf, want_curvature=False, want_count=False):
        """Surface normals from every point's k nearest neighbours (mi_estimate_normals): normals [n, 3] float32, unit length, or (0, 0, 0)
        where a point has fewer than two neighbours; then curvature [n] and count [n] if asked for.  viewpoint: normals are turned
        towards it; None leaves the sign to the solve (deterministic)."""
        cloud = _cloud(cloud)
        n = cloud.shape[0]
        view = None if viewpoint is None else np.ascontiguousarray(viewpoint, np.float32).reshape(3)
        normals = np.empty((n, 3), np.float32)
        curvature = np.empty(n, np.float32) if want_curvature else None
        count = np.empty(n, np.int32) if want_count else None
        ptr = lambda a: None if a is None else a.ctypes.data
        _check(estimate_normals_raw(self._h, cloud.ctypes.data, n, int(k), int(dist_mode), float(max_d2), ptr(view), normals.ctypes.data, ptr(curvature), ptr(count)))
        res = [normals] + ([curvature] if want_curvature else []) + ([count] if want_count else [])
        return res[0] if len(res) == 1 else tuple(res)

    def estimate_normals_times(self):
        """ms per stage of the last estimate_normals: workspace, upload, check, grid, order, fused, download, total (mi_estimate_normals_times)."""
        out = (C.c_double * 8)()
        _check(lib().mi_estimate_normals_times(self._h, out))
        return dict(zip(("workspace", "upload", "check", "grid", "order", "fused", "download", "total"), list(out)))

    # ---- outlier removal
    def remove_outliers(self, cloud, params, want_keep=False, want_mean_distance=False, want_neighbours=False, want_stats=False):
        """Statistical or radius outlier removal (mi_remove_outliers; params: outlier_params(...)): the kept points [kept, 3] with the
        input's bits and their indices [kept] int32, ascending; then, as asked for and in this order: keep [n] uint8, mean_distance [n]
        float32 (statistical only), neighbours [n] int32 and the OutlierStats (mean, stddev, threshold, kept)."""
        cloud = _cloud(cloud)
        n = cloud.shape[0]
        if want_mean_distance and params.method != OUTLIER_STATISTICAL:
            raise ValueError("mean_distance exists for the statistical method only")
        out_xyz, out_index, out_n = np.empty((n, 3), np.float32), np.empty(n, np.int32), C.c_int(0)
        keep = np.empty(n, np.uint8) if want_keep else None
        mean_distance = np.empty(n, np.float32) if want_mean_distance else None
        neighbours = np.empty(n, np.int32) if want_neighbours else None
        stats = OutlierStats() if want_stats else None
        ptr = lambda a: None if a is None else a.ctypes.data
        _check(remove_outliers_raw(self._h, cloud.ctypes.data, n, C.addressof(params), out_xyz.ctypes.data, out_index.ctypes.data, C.addressof(out_n),
                                   ptr(keep), ptr(mean_distance), ptr(neighbours), None if stats is None else C.addressof(stats)))
        res = [out_xyz[:out_n.value].copy(), out_index[:out_n.value].copy()]
        res += [a for a in (keep, mean_distance, neighbours, stats) if a is not None]
        return tuple(res)

    def remove_outliers_times(self):
        """ms per stage of the last remove_outliers: workspace, upload, check, grid, order, kernel, finish, total (mi_remove_outliers_times)."""
        out = (C.c_double * 8)()
        _check(lib().mi_remove_outliers_times(self._h, out))
        return dict(zip(("workspace", "upload", "check", "grid", "order", "kernel", "finish", "total"), list(out)))

    # ---- ISS keypoints
    def iss_keypoints(self, cloud, params, want_is_keypoint=False, want_saliency=False, want_eigenvalues=False, want_neighbours=False):
        """ISS keypoint detection (mi_iss_keypoints; params: iss_params(salient_radius=..., non_max_radius=...)): the keypoints [kept, 3]
        with the input's bits and their indices [kept] int32, ascending; then, as asked for and in this order: is_keypoint [n] uint8,
        saliency [n] float32, eigenvalues [n, 3] float32 (ascending) and neighbours [n] int32 (the salient ball's count)."""
        cloud = _cloud(cloud)
        n = cloud.shape[0]
        out_xyz, out_index, out_n = np.empty((n, 3), np.float32), np.empty(n, np.int32), C.c_int(0)
        is_keypoint = np.empty(n, np.uint8) if want_is_keypoint else None
        saliency = np.empty(n, np.float32) if want_saliency else None
        eigenvalues = np.empty((n, 3), np.float32) if want_eigenvalues else None
        neighbours = np.empty(n, np.int32) if want_neighbours else None
        ptr = lambda a: None if a is None else a.ctypes.data
        _check(iss_keypoints_raw(self._h, cloud.ctypes.data, n, C.addressof(params), out_xyz.ctypes.data, out_index.ctypes.data, C.addressof(out_n),
                                 ptr(is_keypoint), ptr(saliency), ptr(eigenvalues), ptr(neighbours)))
        res = [out_xyz[:out_n.value].copy(), out_index[:out_n.value].copy()]
        res += [a for a in (is_keypoint, saliency, eigenvalues, neighbours) if a is not None]
        return tuple(res)

    def iss_keypoints_times(self):
        """ms per stage of the last iss_keypoints: workspace, upload, check, grid, order, saliency, finish, total (mi_iss_keypoints_times)."""
        out = (C.c_double * 8)()
        _check(lib().mi_iss_keypoints_times(self._h, out))
        return dict(zip(("workspace", "upload", "check", "grid", "order", "saliency", "finish", "total"), list(out)))

    # ---- density-based clustering
    def cluster_dbscan(self, cloud, params, want_sizes=False, want_core=False, want_grouped=False):
        """DBSCAN / Euclidean clustering (mi_cluster_dbscan; params: cluster_params(radius=...)): labels [n] int32 (-1: noise or a dissolved
        cluster) and the number of clusters; then, as asked for and in this order: cluster_sizes [n_clusters] int32, is_core [n] uint8 and
        grouped_index [n_grouped] int32 (the labelled points by (label, index); cluster c starts at cluster_sizes[:c].sum())."""
        cloud = _cloud(cloud)
        n = cloud.shape[0]
        labels, n_clusters, n_grouped = np.empty(n, np.int32), C.c_int(0), C.c_int(0)
        sizes = np.empty(n, np.int32) if want_sizes else None
        core = np.empty(n, np.uint8) if want_core else None
        grouped = np.empty(n, np.int32) if want_grouped else None
        ptr = lambda a: None if a is None else a.ctypes.data
        _check(cluster_dbscan_raw(self._h, cloud.ctypes.data, n, C.addressof(params), labels.ctypes.data, C.addressof(n_clusters), ptr(sizes), n, ptr(core),
                                  ptr(grouped), C.addressof(n_grouped) if want_grouped else None))
        res = [labels, n_clusters.value]
        res += ([sizes[:n_clusters.value].copy()] if want_sizes else []) + ([core] if want_core else []) + ([grouped[:n_grouped.value].copy()] if want_grouped else [])
        return tuple(res)

    def cluster_dbscan_times(self):
        """ms per stage of the last cluster_dbscan: workspace, upload (with the check), grid (with the order), count, link, resolve, finish, total (mi_cluster_dbscan_times)."""
        out = (C.c_double * 8)()
        _check(lib().mi_cluster_dbscan_times(self._h, out))
        return dict(zip(("workspace", "upload", "grid", "count", "link", "resolve", "finish", "total"), list(out)))

    # ---- point-to-plane ICP
    def icp_plane_register(self, before, after, after_normals, params, init=None):
        """Point-to-plane ICP of `before` onto `after` with its normals (mi_icp_plane_register; params: plane_params(...); init: a [4, 4]
        transform indexed [row, col], None for the identity) -> (R [3, 3], t [3], iterations, error, stop_reason)."""
        before, after, normals = _cloud(before), _cloud(after), _cloud(after_normals)
        if normals.shape != after.shape:
            raise ValueError("after_normals must have one normal per fixed point")
        T0 = _T16(init)
        T = np.zeros(16, np.float32)
        it, err, why = C.c_int(0), C.c_float(0), C.c_int(0)
        _check(icp_plane_register_raw(self._h, before.ctypes.data, before.shape[0], after.ctypes.data, normals.ctypes.data, after.shape[0],
                                      C.addressof(params), None if T0 is None else T0.ctypes.data, T.ctypes.data, C.addressof(it), C.addressof(err),
                                      C.addressof(why)))
        R, t = _T_to_Rt(T)
        return R, t, it.value, err.value, why.value

    def plane_system(self, before, after, after_normals, T=None, dist_mode=DIST_CPU_ROUNDING, max_d2=np.inf, want_idx=True):
        """One point-to-plane linearisation at transform T (mi_plane_system) -> (sums float64 [32], centre float32 [3], idx int32 [n] if asked
        for: the fixed index of every moving point's pair, -1 where it has none)."""
        before, after, normals = _cloud(before), _cloud(after), _cloud(after_normals)
        if normals.shape != after.shape:
            raise ValueError("after_normals must have one normal per fixed point")
        T0 = _T16(T)
        n = before.shape[0]
        sums, centre = np.zeros(32, np.float64), np.zeros(3, np.float32)
        idx = np.empty(n, np.int32) if want_idx else None
        _check(plane_system_raw(self._h, before.ctypes.data, n, after.ctypes.data, normals.ctypes.data, after.shape[0],
                                None if T0 is None else T0.ctypes.data, int(dist_mode), float(max_d2), sums.ctypes.data, centre.ctypes.data,
                                None if idx is None else idx.ctypes.data))
        return (sums, centre, idx) if want_idx else (sums, centre)

    def icp_plane_times(self):
        """ms per stage of the last icp_plane_register / plane_system: workspace, upload, check, grid, order, iterations, download, total
        (mi_icp_plane_times)."""
        out = (C.c_double * 8)()
        _check(lib().mi_icp_plane_times(self._h, out))
        return dict(zip(("workspace", "upload", "check", "grid", "order", "iterations", "download", "total"), list(out)))

    # ---- generalized ICP
    def estimate_covariances(self, cloud, k, mode=COV_PLANE, epsilon=1e-3, dist_mode=DIST_CPU_ROUNDING, max_d2=np.inf, want_count=False):
        """Per-point covariances from every point's k nearest neighbours (mi_estimate_covariances): [n, 6] float32, the upper triangle row by
        row (xx, xy, xz, yy, yz, zz); COV_RAW: the neighbourhood's covariance, COV_PLANE: its eigenvalues replaced by (epsilon, 1, 1); six zeros
        where a point has fewer than two neighbours; then count [n] if asked for."""
        cloud = _cloud(cloud)
        n = cloud.shape[0]
        cov = np.empty((n, 6), np.float32)
        count = np.empty(n, np.int32) if want_count else None
        _check(estimate_covariances_raw(self._h, cloud.ctypes.data, n, int(k), int(dist_mode), float(max_d2), int(mode), float(epsilon), cov.ctypes.data,
                                        None if count is None else count.ctypes.data))
        return (cov, count) if want_count else cov

    def icp_gicp_register(self, before, before_cov, after, after_cov, params, init=None):
        """Generalized ICP of `before` onto `after` with both clouds' covariances [points, 6] (mi_icp_gicp_register; params:
        plane_params(...); init: a [4, 4] transform indexed [row, col], None for the identity) -> (R [3, 3], t [3], iterations, error,
        stop_reason)."""
        before, after = _cloud(before), _cloud(after)
        cb, ca = _cov6(before_cov, before.shape[0]), _cov6(after_cov, after.shape[0])
        T0 = _T16(init)
        T = np.zeros(16, np.float32)
        it, err, why = C.c_int(0), C.c_float(0), C.c_int(0)
        _check(icp_gicp_register_raw(self._h, before.ctypes.data, cb.ctypes.data, before.shape[0], after.ctypes.data, ca.ctypes.data, after.shape[0],
                                     C.addressof(params), None if T0 is None else T0.ctypes.data, T.ctypes.data, C.addressof(it), C.addressof(err),
                                     C.addressof(why)))
        R, t = _T_to_Rt(T)
        return R, t, it.value, err.value, why.value

    def gicp_system(self, before, before_cov, after, after_cov, T=None, dist_mode=DIST_CPU_ROUNDING, max_d2=np.inf, want_idx=True):
        """One generalized-ICP linearisation at transform T (mi_gicp_system) -> (sums float64 [32], centre float32 [3], idx int32 [n] if asked
        for: the fixed index of every moving point's pair, -1 where it has none)."""
        before, after = _cloud(before), _cloud(after)
        cb, ca = _cov6(before_cov, before.shape[0]), _cov6(after_cov, after.shape[0])
        T0 = _T16(T)
        n = before.shape[0]
        sums, centre = np.zeros(32, np.float64), np.zeros(3, np.float32)
        idx = np.empty(n, np.int32) if want_idx else None
        _check(gicp_system_raw(self._h, before.ctypes.data, cb.ctypes.data, n, after.ctypes.data, ca.ctypes.data, after.shape[0],
                               None if T0 is None else T0.ctypes.data, int(dist_mode), float(max_d2), sums.ctypes.data, centre.ctypes.data,
                               None if idx is None else idx.ctypes.data))
        return (sums, centre, idx) if want_idx else (sums, centre)

    def icp_gicp_times(self):
        """ms per stage of the last icp_gicp_register / gicp_system: workspace, upload, check, grid, order, iterations, download, total
        (mi_icp_gicp_times)."""
        out = (C.c_double * 8)()
        _check(icp_gicp_times_raw(self._h, out))
        return dict(zip(("workspace", "upload", "check", "grid", "order", "iterations", "download", "total"), list(out)))

    # ---- registration against a voxel map
    def ndt_voxels(self, xyz, voxel, origin=None, min_points=6, eig_ratio=0.01, want_cov=False):
        """One Gaussian per occupied voxel (mi_ndt_voxels) -> dict(coord int32 [rows, 3], mean float32 [rows, 3], icov float32 [rows, 6]: the
        inverse covariances (six zeros: no distribution), count int32 [rows], origin float32 [3], voxel; cov float32 [rows, 6] if asked for).
        The dict is what ndt_register and ndt_system take as their map."""
        xyz = _cloud(xyz)
        n = xyz.shape[0]
        o = None if origin is None else np.ascontiguousarray(origin, np.float32).reshape(3)
        coord, mean, icov = np.empty((n, 3), np.int32), np.empty((n, 3), np.float32), np.empty((n, 6), np.float32)
        count, cov, used = np.empty(n, np.int32), (np.empty((n, 6), np.float32) if want_cov else None), np.zeros(3, np.float32)
        rows = C.c_int(0)
        _check(ndt_voxels_raw(self._h, xyz.ctypes.data, n, float(voxel), None if o is None else o.ctypes.data, int(min_points), float(eig_ratio),
                              coord.ctypes.data, mean.ctypes.data, icov.ctypes.data, C.addressof(rows), count.ctypes.data,
                              None if cov is None else cov.ctypes.data, used.ctypes.data))
        r = rows.value
        out = dict(coord=coord[:r].copy(), mean=mean[:r].copy(), icov=icov[:r].copy(), count=count[:r].copy(), origin=used, voxel=float(voxel))
        if want_cov:
            out["cov"] = cov[:r].copy()
        return out

    @staticmethod
    def _ndt_map(vox):
        coord = np.ascontiguousarray(vox["coord"], np.int32)
        mean, icov = np.ascontiguousarray(vox["mean"], np.float32), np.ascontiguousarray(vox["icov"], np.float32)
        origin = np.ascontiguousarray(vox["origin"], np.float32).reshape(3)
        if coord.ndim != 2 or coord.shape[1] != 3 or mean.shape != coord.shape or icov.shape != (coord.shape[0], 6):
            raise ValueError("a voxel map holds coord [nv, 3], mean [nv, 3] and icov [nv, 6]")
        return coord, mean, icov, origin, float(vox["voxel"])

    def ndt_register(self, before, vox, params, init=None):
        """NDT registration of `before` onto the voxel map `vox` (a dict as ndt_voxels returns; mi_ndt_register; params: ndt_params(...);
        init: a [4, 4] transform indexed [row, col], None for the identity) -> (R [3, 3], t [3], iterations, score, stop_reason)."""
        before = _cloud(before)
        coord, mean, icov, origin, voxel = self._ndt_map(vox)
        T0 = _T16(init)
        T = np.zeros(16, np.float32)
        it, score, why = C.c_int(0), C.c_float(0), C.c_int(0)
        _check(ndt_register_raw(self._h, before.ctypes.data, before.shape[0], coord.ctypes.data, mean.ctypes.data, icov.ctypes.data, coord.shape[0], voxel,
                                origin.ctypes.data, C.addressof(params), None if T0 is None else T0.ctypes.data, T.ctypes.data, C.addressof(it),
                                C.addressof(score), C.addressof(why)))
        R, t = _T_to_Rt(T)
        return R, t, it.value, score.value, why.value

    def ndt_system(self, before, vox, T=None, neighbourhood=7, outlier_ratio=0.55):
        """One NDT linearisation at transform T (mi_ndt_system) -> (sums float64 [32], centre float32 [3], idx int32 [n]: the row of every
        point's own voxel or -1, terms uint8 [n]: every point's number of terms)."""
        before = _cloud(before)
        coord, mean, icov, origin, voxel = self._ndt_map(vox)
        T0 = _T16(T)
        n = before.shape[0]
        sums, centre, idx, terms = np.zeros(32, np.float64), np.zeros(3, np.float32), np.empty(n, np.int32), np.empty(n, np.uint8)
        _check(ndt_system_raw(self._h, before.ctypes.data, n, coord.ctypes.data, mean.ctypes.data, icov.ctypes.data, coord.shape[0], voxel, origin.ctypes.data,
                              None if T0 is None else T0.ctypes.data, int(neighbourhood), float(outlier_ratio), sums.ctypes.data, centre.ctypes.data,
                              idx.ctypes.data, terms.ctypes.data))
        return sums, centre, idx, terms

    def ndt_times(self):
        """ms per stage of the last ndt_register / ndt_system: workspace, upload, check, table, order, iterations, download, total (mi_ndt_times)."""
        out = (C.c_double * 8)()
        _check(ndt_times_raw(self._h, out))
        return dict(zip(("workspace", "upload", "check", "table", "order", "iterations", "download", "total"), list(out)))

    # ---- local descriptors
    def fpfh_features(self, cloud, normals, k, dist_mode=DIST_CPU_ROUNDING, max_d2=np.inf, want_counts=False, want_count=False):
        """FPFH descriptors of a cloud with normals from every point's k nearest neighbours (mi_fpfh_features): fpfh [n, 33] float32, the
        blocks of theta, alpha and phi, each summing to 200 (33 zeros where a point has no neighbour); then counts [n, 33] uint8, the SPFH's
        pair counts per bin, and count [n] int32, the neighbours, if asked for."""
        cloud, normals = _cloud(cloud), _cloud(normals)
        if normals.shape != cloud.shape:
            raise ValueError("normals must have one normal per point")
        n = cloud.shape[0]
        fpfh = np.empty((n, FPFH_DIM), np.float32)
        counts = np.empty((n, FPFH_DIM), np.uint8) if want_counts else None
        count = np.empty(n, np.int32) if want_count else None
        ptr = lambda a: None if a is None else a.ctypes.data
        _check(fpfh_features_raw(self._h, cloud.ctypes.data, normals.ctypes.data, n, int(k), int(dist_mode), float(max_d2), fpfh.ctypes.data, ptr(counts), ptr(count)))
        res = [fpfh] + ([counts] if want_counts else []) + ([count] if want_count else [])
        return res[0] if len(res) == 1 else tuple(res)

    def fpfh_features_times(self):
        """ms per stage of the last fpfh_features: workspace, upload, check, grid, order, kernels, download, total (mi_fpfh_features_times)."""
        out = (C.c_double * 8)()
        _check(fpfh_features_times_raw(self._h, out))
        return dict(zip(("workspace", "upload", "check", "grid", "order", "kernels", "download", "total"), list(out)))

    def feature_match(self, query, target, mutual=False, want_d2=False):
        """The nearest row of target [m, dim] for every row of query [n, dim] in descriptor space, every pair looked at (mi_feature_match):
        idx [n] int32 -- with mutual, -1 where the match is not reciprocal -- then d2 [n] float32 (+inf at -1) if asked for."""
        query, target = np.ascontiguousarray(query, np.float32), np.ascontiguousarray(target, np.float32)
        if query.ndim != 2 or target.ndim != 2 or query.shape[1] != target.shape[1]:
            raise ValueError("query and target are [rows, dim] with the same dim")
        n, m, dim = query.shape[0], target.shape[0], query.shape[1]
        idx = np.empty(n, np.int32)
        d2 = np.empty(n, np.float32) if want_d2 else None
        _check(feature_match_raw(self._h, query.ctypes.data, n, target.ctypes.data, m, dim, 1 if mutual else 0, idx.ctypes.data,
                                 None if d2 is None else d2.ctypes.data))
        return (idx, d2) if want_d2 else idx

    def feature_match_times(self):
        """ms per stage of the last feature_match: workspace, upload, check, -, -, kernels, download, total (mi_feature_match_times)."""
        out = (C.c_double * 8)()
        _check(feature_match_times_raw(self._h, out))
        return dict(zip(("workspace", "upload", "check", "unused3", "unused4", "kernels", "download", "total"), list(out)))

    def ransac_register(self, src, tgt, idx, params, want_mask=False):
        """A pose from correspondences src[i] <-> tgt[idx[i]] (idx -1: none) by hypothesise and verify (mi_ransac_register):
        (R [3, 3] float32, t [3], inliers, rmse, best_hypothesis, valid_hypotheses), then the inlier mask [n] uint8 if asked for."""
        src, tgt = _cloud(src), _cloud(tgt)
        idx = np.ascontiguousarray(idx, np.int32)
        if idx.shape != (src.shape[0],):
            raise ValueError("idx has one entry per source point")
        R9, t3 = np.empty(9, np.float32), np.empty(3, np.float32)
        inl, best, nvalid, rmse = C.c_int(0), C.c_int(0), C.c_int(0), C.c_float(0)
        mask = np.empty(src.shape[0], np.uint8) if want_mask else None
        _check(ransac_register_raw(self._h, src.ctypes.data, src.shape[0], tgt.ctypes.data, tgt.shape[0], idx.ctypes.data, C.addressof(params), R9.ctypes.data,
                                   t3.ctypes.data, C.addressof(inl), C.addressof(rmse), C.addressof(best), C.addressof(nvalid), None if mask is None else mask.ctypes.data))
        out = (R9.reshape(3, 3).T.copy(), t3, inl.value, np.float32(rmse.value), best.value, nvalid.value)
        return out + (mask,) if want_mask else out

    def ransac_hypotheses(self, src, tgt, idx, params, first=0, count=None):
        """Hypotheses first .. first + count - 1 of ransac_register (mi_ransac_hypotheses): triples [count, 3] int32 (source indices),
        valid [count] uint8, pose12 [count, 12] float32 (R9 column-major, then t3), inlier_count [count] int32."""
        src, tgt = _cloud(src), _cloud(tgt)
        idx = np.ascontiguousarray(idx, np.int32)
        if idx.shape != (src.shape[0],):
            raise ValueError("idx has one entry per source point")
        count = params.hypotheses - first if count is None else count
        rows = max(count, 1)
        triples, valid = np.empty((rows, 3), np.int32), np.empty(rows, np.uint8)
        pose12, inl = np.empty((rows, 12), np.float32), np.empty(rows, np.int32)
        _check(ransac_hypotheses_raw(self._h, src.ctypes.data, src.shape[0], tgt.ctypes.data, tgt.shape[0], idx.ctypes.data, C.addressof(params), int(first), int(count),
                                     triples.ctypes.data, valid.ctypes.data, pose12.ctypes.data, inl.ctypes.data))
        return triples, valid, pose12, inl

    def ransac_register_times(self):
        """ms per stage of the last ransac_register: workspace, upload, hypotheses, count, argmax, refine, -, total (mi_ransac_register_times)."""
        out = (C.c_double * 8)()
        _check(ransac_register_times_raw(self._h, out))
        return dict(zip(("workspace", "upload", "hypotheses", "count", "argmax", "refine", "unused6", "total"), list(out)))

    # ---- profiling
    def profile_enable(self, on=True):
        _check(lib().mi_profile_enable(self._h, 1 if on else 0))

    def search_stats(self, enable):
        """Counters of the cell-grid search since they were last enabled: (candidates, rows, to_hierarchy, points, nodes, leaves,
        walking waves, longest single walk)."""
        out = (C.c_ulonglong * 8)()
        _check(lib().mi_profile_search_stats(self._h, 1 if enable else 0, out))
        return tuple(int(v) for v in out)

    SEARCH_PHASES = ("waves", "scan_waves", "walk_only_waves", "block_batches", "block_dealt", "block_deal_passes", "block_deal_writes", "block_lockstep_trips",
                     "rest_rounds", "rest_dealt", "rest_deal_passes", "rest_deal_writes", "rest_lockstep_trips", "rest_batches4", "rest_waves",
                     "walk_leaf_hits", "walk_leaf_children", "walk_votes", "walk_pops", "walk_leaf_offers")

    def search_phases(self):
        """Loop trip counts of the counting build since search_stats(True), summed over waves (mi_profile_search_phases) -> dict."""
        out = (C.c_ulonglong * 20)()
        _check(lib().mi_profile_search_phases(self._h, out))
        return {k: int(out[i]) for i, k in enumerate(self.SEARCH_PHASES)}

    def selftest_fail_loads(self, n):
        """Test hook: the next n index builds of this context fail on purpose (mi_selftest_fail_loads)."""
        _check(lib().mi_selftest_fail_loads(self._h, int(n)))

    def selftest_sort_pairs(self, keys, values, bits=30):
        """The library's device radix sort on host arrays: (sorted keys, values carried along), stable."""
        k = np.ascontiguousarray(keys, dtype=np.uint32).copy()
        v = np.ascontiguousarray(values, dtype=np.int32).copy()
        assert k.shape == v.shape and k.ndim == 1
        _check(lib().mi_selftest_sort_pairs(self._h, k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), int(k.size), int(bits)))
        return k, v

    def selftest_cloud_range(self, xyz, check=0):
        """The range pass of csrc/cloud_range.hpp over an (n, 3) host cloud: (lo_hi float32[6], lowest refused index or 0x7fffffff).
        check 0: refuse nothing; 1: non-finite points; 2: those and |coordinate| > 1e18 (mi_selftest_cloud_range)."""
        p = np.ascontiguousarray(xyz, dtype=np.float32)
        assert p.ndim == 2 and p.shape[1] == 3
        lo_hi = np.zeros(6, np.float32)
        bad = C.c_int(-1)
        _check(selftest_cloud_range_raw(self._h, p.ctypes.data, int(p.shape[0]), int(check), lo_hi.ctypes.data, C.byref(bad)))
        return lo_hi, int(bad.value)

    def selftest_icp_schedule(self):
        """What the last ICP step left on the device: dict(order int32[rows], far uint8[rows], cursors int32[4], ticket, sums float64[18]
        = the 16 moments and 2 error sums the last solve read) (mi_selftest_icp_schedule)."""
        f = lib().mi_selftest_icp_schedule
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        f.restype = C.c_int
        rows, ticket = C.c_int(0), C.c_int(-1)
        cursors, sums = np.zeros(4, np.int32), np.zeros(18, np.float64)
        _check(f(self._h, 0, None, None, C.byref(rows), cursors.ctypes.data, C.byref(ticket), sums.ctypes.data))
        order, far = np.zeros(rows.value, np.int32), np.zeros(rows.value, np.uint8)
        _check(f(self._h, rows.value, order.ctypes.data, far.ctypes.data, C.byref(rows), cursors.ctypes.data, C.byref(ticket), sums.ctypes.data))
        return dict(order=order, far=far, cursors=cursors, ticket=int(ticket.value), sums=sums)

    def selftest_cpd_last(self, m, n, arrays=True):
        """What the last cpd_register / cpd_mstep left in the workspace (mi_selftest_cpd_last; it must be the next call on the context): dict(p1 [m],
        pt1 [n], px [m,3], y [m,3] -- with arrays=False these four are left out --, xs float64[5], ks float64[14], R [3,3], t [3], scale, sigma2,
        sigma2_init, constant, route, fused, rows_x, rows_k, reduced, iterations, stop_reason)."""
        f = lib().mi_selftest_cpd_last
        f.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 13
        f.restype = C.c_int
        m, n = int(m), int(n)
        out = {}
        if arrays:
            out.update(p1=np.zeros(m, np.float32), pt1=np.zeros(n, np.float32), px=np.zeros((m, 3), np.float32), y=np.zeros((m, 3), np.float32))
        xs, ks, R9, t3 = np.zeros(5, np.float64), np.zeros(14, np.float64), np.zeros(9, np.float32), np.zeros(3, np.float32)
        sc = [C.c_float(0) for _ in range(4)]
        info = np.zeros(8, np.int32)
        ptr = [out[k].ctypes.data if arrays else None for k in ("p1", "pt1", "px", "y")]
        _check(f(self._h, m, n, *ptr, xs.ctypes.data, ks.ctypes.data, R9.ctypes.data, t3.ctypes.data,
                 *[C.cast(C.byref(v), C.c_void_p) for v in sc], info.ctypes.data))
        out.update(xs=xs, ks=ks, R=R9.reshape(3, 3).T.copy(), t=t3, scale=np.float32(sc[0].value), sigma2=np.float32(sc[1].value),
                   sigma2_init=np.float32(sc[2].value), constant=np.float32(sc[3].value))
        out.update(zip(("route", "fused", "rows_x", "rows_k", "reduced", "iterations", "stop_reason"), (int(v) for v in info[:7])))
        return out

    def selftest_nicp_candidates(self, before, after, order_heads):
        """The moments stage and the candidates of nicp_register without its driver (mi_selftest_nicp_candidates): (raw float64[32] -- the sums of the
        clouds taken about their first points --, R [reps, 3, 3], t [reps, 3], approx [reps]) for order_heads [reps, 3]."""
        f = lib().mi_selftest_nicp_candidates
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        f.restype = C.c_int
        before, after = _cloud(before), _cloud(after)
        heads = np.ascontiguousarray(order_heads, np.int32).reshape(-1, 3)
        raw, out = np.zeros(32, np.float64), np.zeros((len(heads), 13), np.float32)
        _check(f(self._h, before.ctypes.data, before.shape[0], after.ctypes.data, after.shape[0], heads.ctypes.data, len(heads), raw.ctypes.data,
                 out.ctypes.data))
        return raw, out[:, :9].reshape(-1, 3, 3).copy(), out[:, 9:12].copy(), out[:, 12].copy()

    def nn_kernel_name(self, n_moving, m_fixed_local, nn_mode=NN_AUTO):
        lib().mi_nn_kernel_name.restype = C.c_char_p
        return lib().mi_nn_kernel_name(self._h, n_moving, m_fixed_local, nn_mode).decode()

    def profile_select(self, kernels=None):
        """Restrict the event timing to these kernels (KERNEL_* ids); None = all."""
        mask = 0xffffffff if kernels is None else sum(1 << k for k in kernels)
        _check(lib().mi_profile_select(self._h, C.c_uint(mask)))

    def profile_reset(self):
        _check(lib().mi_profile_reset(self._h))

    def icp_load_times(self):
        """ms per stage of the last icp_load: workspace, moving upload, moving order, fixed upload, hierarchy, grid, reset, total."""
        out = (C.c_double * 8)()
        _check(lib().mi_icp_load_times(self._h, out))
        return dict(zip(("workspace", "upload_moving", "order_moving", "upload_fixed", "hierarchy", "grid", "reset", "total"), list(out)))

    def profile_get(self, kernel):
        ms, n = C.c_double(0), C.c_longlong(0)
        _check(lib().mi_profile_get(self._h, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value
