"""ctypes binding of libmislam.so -- the C ABI declared in include/mi_slam.h.

This module is plumbing for the Python-side callers in this repository (tests, bench.py, __graft_entry__): it passes host
numpy buffers straight through to the C entry points and adds nothing of its own.  There is deliberately no fallback: if
the shared library is missing, or no HIP device is usable, the calls raise.  The header is the only statement of the C interface:
lib() parses it and gives every function its argument and return types at load, and nothing else in this module types a call.
"""
import ctypes as C
import os
import re as _re                     # under a private name: the module's public names are its interface

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


# ---- the loader: the header is the only statement of the C interface; every prototype below is read from it
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "mi_slam.h")       # the tree's header, also when MISLAM_LIB names a variant build
_SCALARS = {"int": C.c_int, "float": C.c_float, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "unsigned int": C.c_uint}
_ARGUMENTS = dict(_SCALARS, mi_exchange_fn=EXCHANGE_FN)
_RETURNS = dict(_SCALARS, **{"void": None, "const char*": C.c_char_p})


def _parse_header(text):
    """[(name, return text, [argument texts], restype, [argtypes])] of every mi_* prototype of a header's text.  An argument with a '*' or
    a '[' is a c_void_p; what is left is the vocabulary above.  Anything else raises and names the declaration: no ctypes default is used."""
    text = _re.sub(r"/\*.*?\*/", " ", text, flags=_re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    out = []
    for decl in text.split(";"):
        if not _re.search(r"\bmi_\w+\s*\(", decl):
            continue
        decl = " ".join(decl.split())
        m = _re.fullmatch(r"([\w\s*]+?)\s*\b(mi_\w+)\s*\(([^()]*)\)", decl)
        if not m:
            raise MiSlamError("mi_slam.h: cannot parse the declaration `%s`" % decl)
        ret, name, args = _re.sub(r"\s*\*", "*", m.group(1)), m.group(2), [a.strip() for a in m.group(3).split(",")]
        args = [] if args == ["void"] else args
        if ret not in _RETURNS:
            raise MiSlamError("mi_slam.h: return type `%s` is outside the binding's vocabulary in `%s`" % (ret, decl))
        argtypes = []
        for a in args:
            scalar = _re.fullmatch(r"(.+?)\s*\b\w+", a)          # the type in front of the parameter's name
            if "*" in a or "[" in a:
                argtypes.append(C.c_void_p)
            elif scalar and scalar.group(1) in _ARGUMENTS:
                argtypes.append(_ARGUMENTS[scalar.group(1)])
            else:
                raise MiSlamError("mi_slam.h: argument `%s` is outside the binding's vocabulary in `%s`" % (a, decl))
        out.append((name, ret, args, _RETURNS[ret], argtypes))
    return out


try:
    with open(_HEADER) as _fh:
        _PROTOTYPES = _parse_header(_fh.read())
except OSError:
    _PROTOTYPES = []                                          # lib() raises
EXPORTS = [p[0] for p in _PROTOTYPES]                         # every symbol include/mi_slam.h declares


def lib():
    """Load libmislam.so (raises if it has not been built -- run __graft_entry__.build()) and give every function its header's types."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MiSlamError("libmislam.so not built at %s: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        if not _PROTOTYPES:
            raise MiSlamError("no mi_* prototype read from %s (is the header there?): the binding takes every type from it" % _HEADER)
        loaded = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, _, _, restype, argtypes in _PROTOTYPES:
            if not hasattr(loaded, name):
                raise MiSlamError("%s lacks %s, which mi_slam.h declares" % (LIB_PATH, name))
            f = getattr(loaded, name)
            f.restype, f.argtypes = restype, argtypes
        _lib = loaded
    return _lib


def _check(rc):
    if rc != MI_OK:
        raise MiSlamError("libmislam error %d: %s" % (rc, lib().mi_last_error().decode()))


def _ptr(a):
    return None if a is None else a.ctypes.data


def _raw(name):
    """mi_<name> as the header types it, with pointers as Python ints, ctypes objects or None: returns the error code, raises nothing."""
    return lambda *args: getattr(lib(), name)(*args)


def _params(cls, default, kw):
    """A parameter struct at the library's defaults (the function named `default`) with the fields of kw set."""
    p = cls()
    getattr(lib(), default)(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


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
    return _params(IcpParams, "mi_icp_params_cuda_slam" if cuda_slam else "mi_icp_params_default", kw)


def cpd_params(**kw):
    return _params(CpdParams, "mi_cpd_params_default", kw)


def nicp_params(**kw):
    return _params(NicpParams, "mi_nicp_params_default", kw)


def fgt_tables(order):
    """Host-only: exponents (a, b, c) per monomial in the reference's graded order, C_k and the Horner slot (mi_fgt_tables)."""
    pd = C.c_int(0)
    _check(lib().mi_fgt_tables(int(order), None, None, None, C.byref(pd)))
    mono, ck, slot = np.empty(pd.value, np.uint32), np.empty(pd.value, np.float32), np.empty(pd.value, np.int32)
    _check(lib().mi_fgt_tables(int(order), _ptr(mono), _ptr(ck), _ptr(slot), C.byref(pd)))
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
    return lib().mi_icp_batch_route(int(n_before), int(n_after), C.byref(params))


icp_register_batch_raw = _raw("mi_icp_register_batch")


class CpdBatchInfo(C.Structure):
    _fields_ = [("problems_batched", C.c_int), ("problems_fallback", C.c_int), ("launches", C.c_int), ("reserved", C.c_int * 5)]


def cpd_batch_route(m_before, n_after, params):
    """1 if mi_cpd_register_batch carries a problem of these sizes under these rules on the batched kernel, 0 if it takes the existing path."""
    return lib().mi_cpd_batch_route(int(m_before), int(n_after), C.byref(params))


cpd_register_batch_raw = _raw("mi_cpd_register_batch")


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


def _batch_call(befores, afters, before_range, after_range):
    """What both batched calls start from: the four input arrays, the number of problems B and the per-problem outputs T [B, 16],
    iterations, error and stop_reason [B]."""
    arrays = _batch_arrays(befores, afters, before_range, after_range)
    B = len(arrays[1])
    return arrays, B, np.zeros((B, 16), np.float32), np.zeros(B, np.int32), np.zeros(B, np.float32), np.zeros(B, np.int32)


def _batch_Rt(T):
    M = T.reshape(-1, 4, 4).transpose(0, 2, 1)        # column-major 4x4 -> [row, col]
    return M[:, :3, :3].copy(), M[:, :3, 3].copy()


voxel_index_raw = _raw("mi_voxel_index")


def voxel_index(p, origin, voxel):
    """The voxel a point falls in (mi_voxel_index, host only): int32 [3] = floor((p - origin) / voxel) in fp32."""
    p = np.ascontiguousarray(p, np.float32).reshape(3)
    origin = np.ascontiguousarray(origin, np.float32).reshape(3)
    out = np.zeros(3, np.int32)
    _check(voxel_index_raw(p.ctypes.data, origin.ctypes.data, float(voxel), out.ctypes.data))
    return out


voxel_downsample_raw = _raw("mi_voxel_downsample")


KNN_MAX_K = 32                      # MI_KNN_MAX_K


knn_search_raw = _raw("mi_knn_search")
estimate_normals_raw = _raw("mi_estimate_normals")


OUTLIER_STATISTICAL, OUTLIER_RADIUS = 0, 1     # MI_OUTLIER_*


def outlier_params(**kw):
    """mi_outlier_params at its defaults (statistical, k = 16, std_ratio = 2, CPU rounding) with the given fields set."""
    return _params(OutlierParams, "mi_outlier_params_default", kw)


remove_outliers_raw = _raw("mi_remove_outliers")


def iss_params(**kw):
    """mi_iss_params at its defaults (gamma 0.975 and 0.975, min_neighbours 5, CPU rounding; both radii 0: set them) with the given fields set."""
    return _params(IssParams, "mi_iss_params_default", kw)


iss_keypoints_raw = _raw("mi_iss_keypoints")


class Mls:
    """mi_mls_params, held in a namespace as Fgr's is; the compiler checks this one's layout against the header's in tests/test_mls_abi.py."""
    C_TYPE = "mi_mls_params"
    QUADRATIC, PLANE, UNTOUCHED = 0, 1, 2      # MI_MLS_*: out_status

    class Params(C.Structure):
        _fields_ = [("radius", C.c_float), ("gauss_scale", C.c_float), ("order", C.c_int), ("min_neighbours", C.c_int), ("dist_mode", C.c_int),
                    ("reserved", C.c_int * 11)]


def mls_params(**kw):
    """mi_mls_params at its defaults (order 2, min_neighbours 3, CPU rounding, gauss_scale 0 = the radius; radius 0: set it) with the given fields set."""
    for k in kw:
        if k == "reserved" or k not in [f[0] for f in Mls.Params._fields_]:
            raise TypeError("mi_mls_params has no field %r" % k)
    return _params(Mls.Params, "mi_mls_params_default", kw)


mls_smooth_raw = _raw("mi_mls_smooth")


RADIUS_MAX_TOTAL = 1 << 31          # MI_RADIUS_MAX_TOTAL


def _kernel_constant(name):
    """An integer constant of csrc/kernels.h, read from that file as the prototypes are read from the header: stated in one place."""
    with open(os.path.join(_HERE, "csrc", "kernels.h")) as fh:
        m = _re.search(r"^constexpr int %s = (\d+);" % name, fh.read(), flags=_re.M)
    if not m:
        raise MiSlamError("csrc/kernels.h states no integer constant %s" % name)
    return int(m.group(1))


RADIUS_WAVE_ROW = _kernel_constant("RADIUS_WAVE_ROW")          # the longest row the sort kernel ranks in registers ...
RADIUS_SORT_CHUNK = _kernel_constant("RADIUS_SORT_CHUNK")      # ... and the keys of a longer row it holds in the LDS at a time: where its paths change


radius_search_raw = _raw("mi_radius_search")


def cluster_params(**kw):
    """mi_cluster_params at its defaults (min_points 1, min_cluster_size 1, no upper limit, CPU rounding; radius 0: set it) with the given fields set."""
    return _params(ClusterParams, "mi_cluster_params_default", kw)


cluster_dbscan_raw = _raw("mi_cluster_dbscan")
segment_plane_raw = _raw("mi_segment_plane")
segment_plane_hypotheses_raw = _raw("mi_segment_plane_hypotheses")
SEGMENT_MAX_PLANES = 16


def plane_params(**kw):
    """mi_plane_params at its defaults (eps 1e-6 and 1e-6, 50 iterations, no distance limit, CPU rounding) with the given fields set."""
    return _params(PlaneParams, "mi_plane_params_default", kw)


icp_plane_register_raw = _raw("mi_icp_plane_register")
plane_system_raw = _raw("mi_plane_system")
evaluate_registration_raw = _raw("mi_evaluate_registration")
pose_graph_optimize_raw = _raw("mi_pose_graph_optimize")
pose_graph_system_raw = _raw("mi_pose_graph_system")


class PoseGraph:
    """mi_pose_graph_params, held in a namespace as Fgr holds its own: the compiler checks this one's layout against the header's in
    tests/test_pose_graph_abi.py."""
    C_TYPE = "mi_pose_graph_params"

    class Params(C.Structure):
        _fields_ = [("max_iterations", C.c_int), ("max_pcg_iterations", C.c_int), ("reference_node", C.c_int), ("pcg_tolerance", C.c_double),
                    ("relative_decrease", C.c_double), ("absolute_cost", C.c_double), ("lambda0", C.c_double), ("line_process_mu", C.c_double)]


def pose_graph_params(**kw):
    """mi_pose_graph_params at its defaults (50 linearisations, 200 inner iterations, reference node 0, tolerances 1e-8, 1e-9 and 0,
    lambda0 1e-6, no line process) with the given fields set."""
    return _params(PoseGraph.Params, "mi_pose_graph_default_params", kw)


def _pose_graph_arrays(poses, edge_source, edge_target, edge_T, edge_information, edge_uncertain):
    """The graph as the ABI takes it: [V, 4, 4] and [E, 4, 4] transforms indexed [row, col] become column-major 16s."""
    poses = np.ascontiguousarray(np.swapaxes(np.asarray(poses, np.float64).reshape(-1, 4, 4), 1, 2)).reshape(-1, 16)
    src, tgt = np.ascontiguousarray(edge_source, np.int32).reshape(-1), np.ascontiguousarray(edge_target, np.int32).reshape(-1)
    E = len(src)
    Z = np.ascontiguousarray(np.swapaxes(np.asarray(edge_T, np.float64).reshape(-1, 4, 4), 1, 2)).reshape(-1, 16)
    info = np.ascontiguousarray(edge_information, np.float64).reshape(-1, 36)
    unc = None if edge_uncertain is None else np.ascontiguousarray(edge_uncertain, np.uint8).reshape(-1)
    if len(tgt) != E or len(Z) != E or len(info) != E or (unc is not None and len(unc) != E):
        raise ValueError("edge arrays must hold one entry per edge")
    return poses, src, tgt, Z, info, unc, E


COV_RAW, COV_PLANE = 0, 1     # MI_COV_*


estimate_covariances_raw = _raw("mi_estimate_covariances")
icp_gicp_register_raw = _raw("mi_icp_gicp_register")
gicp_system_raw = _raw("mi_gicp_system")
icp_gicp_times_raw = _raw("mi_icp_gicp_times")


estimate_color_gradients_raw = _raw("mi_estimate_color_gradients")
icp_color_register_raw = _raw("mi_icp_color_register")
color_system_raw = _raw("mi_color_system")
icp_color_times_raw = _raw("mi_icp_color_times")


def intensity_of_rgb(rgb):
    """The intensity the colour calls take, one float32 per point, of colours [n, 3]: (r + g + b) / 3, in float32 and in that order."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    if rgb.ndim != 2 or rgb.shape[1] != 3:
        raise ValueError("colours are [n, 3]: r, g, b per point")
    return ((rgb[:, 0] + rgb[:, 1]) + rgb[:, 2]) / np.float32(3)


def _intensity(a, points):
    a = np.ascontiguousarray(a, np.float32)
    if a.shape != (points,):
        raise ValueError("intensities are [points]: one float per point")
    return a


def ndt_params(**kw):
    """mi_ndt_params with the library's defaults, then the given fields"""
    return _params(NdtParams, "mi_ndt_params_default", kw)


ndt_constants_raw = _raw("mi_ndt_constants")


def ndt_constants(voxel, outlier_ratio=0.55):
    """(d1, d2, h, k) of the NDT score as float64 [4] (mi_ndt_constants, host only)"""
    out = np.zeros(4, np.float64)
    _check(ndt_constants_raw(float(voxel), float(outlier_ratio), out.ctypes.data))
    return out


ndt_voxels_raw = _raw("mi_ndt_voxels")
ndt_register_raw = _raw("mi_ndt_register")
ndt_system_raw = _raw("mi_ndt_system")
ndt_times_raw = _raw("mi_ndt_times")


FPFH_BINS, FPFH_DIM = 11, 33     # MI_FPFH_BINS, MI_FPFH_DIM


fpfh_features_raw = _raw("mi_fpfh_features")
fpfh_features_times_raw = _raw("mi_fpfh_features_times")


FEATURE_MAX_DIM = 64             # MI_FEATURE_MAX_DIM


feature_match_raw = _raw("mi_feature_match")
feature_match_times_raw = _raw("mi_feature_match_times")


class ScanContext:
    """mi_scan_context_params, held in a namespace as PoseGraph holds its own: the compiler checks this one's layout against the header's in
    tests/test_scan_context_abi.py."""
    C_TYPE = "mi_scan_context_params"

    class Params(C.Structure):
        _fields_ = [("rings", C.c_int), ("sectors", C.c_int), ("max_radius", C.c_float), ("z_offset", C.c_float), ("reserved", C.c_int * 12)]


SCAN_CONTEXT_MAX_RINGS, SCAN_CONTEXT_MAX_SECTORS, SCAN_CONTEXT_MAX_ROWS = 32, 64, 1 << 26      # MI_SCAN_CONTEXT_MAX_*
SC_SEARCH_CHUNK = _kernel_constant("SC_SEARCH_CHUNK")          # database rows per workgroup of the search kernel: a multiple of this
SC_SEARCH_WAVES = _kernel_constant("SC_SEARCH_WAVES")
SC_SLICE = _kernel_constant("SC_SLICE")                        # points of a scan per workgroup of the binning kernel


def scan_context_params(**kw):
    """mi_scan_context_params at its defaults (20 rings, 60 sectors, max_radius 80, z_offset 2) with the given fields set."""
    return _params(ScanContext.Params, "mi_scan_context_params_default", kw)


def scan_context_tables(params=None):
    """Host-only: the squared ring edges [rings + 1] and the sectors' boundary directions [sectors, 2] (cos, sin), float64, exactly as
    mi_scan_context bins with them (mi_scan_context_tables)."""
    params = params if params is not None else scan_context_params()
    edge2 = np.empty(max(int(params.rings), 0) + 1, np.float64)
    dirs = np.empty((max(int(params.sectors), 0), 2), np.float64)
    if not (1 <= params.rings <= SCAN_CONTEXT_MAX_RINGS and 1 <= params.sectors <= SCAN_CONTEXT_MAX_SECTORS):
        edge2, dirs = np.empty(SCAN_CONTEXT_MAX_RINGS + 1), np.empty((SCAN_CONTEXT_MAX_SECTORS, 2))     # the call refuses; nothing is written
    _check(lib().mi_scan_context_tables(C.byref(params), edge2.ctypes.data, dirs.ctypes.data))
    return edge2, dirs


scan_context_raw = _raw("mi_scan_context")
scan_context_search_raw = _raw("mi_scan_context_search")


class Tsdf:
    """mi_tsdf_params, held in a namespace as ScanContext holds its own: the compiler checks this one's layout against the header's in
    tests/test_tsdf_abi.py."""
    C_TYPE = "mi_tsdf_params"

    class Params(C.Structure):
        _fields_ = [("voxel_size", C.c_float), ("truncation", C.c_float), ("min_range", C.c_float), ("max_range", C.c_float),
                    ("max_weight", C.c_float), ("reserved", C.c_int * 11)]


TSDF_MAX_HALF_STEPS = 16                                        # MI_TSDF_MAX_HALF_STEPS
TSDF_BLOCK = _kernel_constant("TSDF_BLOCK")                     # rays per workgroup of the sampling kernel


def tsdf_params(**kw):
    """mi_tsdf_params at its defaults (no range gate, no weight cap; voxel_size and truncation 0: set them) with the given fields set."""
    return _params(Tsdf.Params, "mi_tsdf_params_default", kw)


tsdf_integrate_raw = _raw("mi_tsdf_integrate")
tsdf_extract_raw = _raw("mi_tsdf_extract")
tsdf_mesh_raw = _raw("mi_tsdf_mesh")


def _tsdf_map(m):
    """(coord [nv, 3] int32, tsdf [nv] float32, weight [nv] float32) of a map given as such a triple, or of None: the empty map"""
    if m is None:
        return np.zeros((0, 3), np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32)
    coord, tsdf, weight = m
    coord = np.ascontiguousarray(coord, np.int32).reshape(-1, 3)
    tsdf, weight = np.ascontiguousarray(tsdf, np.float32).ravel(), np.ascontiguousarray(weight, np.float32).ravel()
    if not (len(coord) == len(tsdf) == len(weight)):
        raise ValueError("a map is coord [nv, 3], tsdf [nv] and weight [nv]")
    return coord, tsdf, weight


class TsdfRaycast:
    """mi_tsdf_raycast_params, in a namespace as Tsdf: the compiler checks the layout against the header's in tests/test_tsdf_raycast_abi.py."""
    C_TYPE = "mi_tsdf_raycast_params"

    class Params(C.Structure):
        _fields_ = [("voxel_size", C.c_float), ("min_weight", C.c_float), ("min_range", C.c_float), ("max_range", C.c_float),
                    ("visit_every_sample", C.c_int), ("reserved", C.c_int * 11)]


TSDF_RAYCAST_MAX_STEPS = 65536                                  # MI_TSDF_RAYCAST_MAX_STEPS


def tsdf_raycast_params(**kw):
    """mi_tsdf_raycast_params at its defaults (min_weight 1, min_range 0, skipping on; voxel_size and max_range 0: set them) with the given
    fields set."""
    return _params(TsdfRaycast.Params, "mi_tsdf_raycast_params_default", kw)


tsdf_raycast_raw = _raw("mi_tsdf_raycast")


def pinhole_directions(width, height, fx, fy, cx, cy):
    """The rays of a pinhole camera that looks along +z, x to the right and y down: [height * width, 3] float32, row by row, pixel (u, v) at
    row v * width + u with the direction ((u - cx) / fx, (v - cy) / fy, 1).  Not normalised: mi_tsdf_raycast takes any length, and its depth is
    along the ray, not along z."""
    u, v = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], axis=-1)
    return np.ascontiguousarray(d.reshape(-1, 3), np.float32)


def spherical_directions(rows, cols, elevation_lo, elevation_hi):
    """The beams of a spinning LiDAR: [rows * cols, 3] float32, ring by ring; ring r has the elevation elevation_lo + r (elevation_hi -
    elevation_lo) / (rows - 1) (radians above the sensor's xy plane; one ring: elevation_lo), column c the azimuth 2 pi c / cols about +z."""
    elev = np.linspace(elevation_lo, elevation_hi, rows) if rows > 1 else np.array([float(elevation_lo)])
    azim = 2 * np.pi * np.arange(cols) / cols
    e, a = np.meshgrid(elev, azim, indexing="ij")
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=-1)
    return np.ascontiguousarray(d.reshape(-1, 3), np.float32)


class RansacParams(C.Structure):
    _fields_ = [("hypotheses", C.c_int), ("seed", C.c_ulonglong), ("max_distance", C.c_float), ("edge_similarity", C.c_float),
                ("refine_iterations", C.c_int), ("reserved", C.c_int * 8)]


def ransac_params(max_distance, **kw):
    """mi_ransac_params_default with max_distance and any other field set: hypotheses, seed, edge_similarity, refine_iterations."""
    for k in kw:
        if k not in ("hypotheses", "seed", "edge_similarity", "refine_iterations"):
            raise TypeError("mi_ransac_params has no field %r" % k)
    return _params(RansacParams, "mi_ransac_params_default", dict(kw, max_distance=max_distance))


ransac_register_raw = _raw("mi_ransac_register")
ransac_hypotheses_raw = _raw("mi_ransac_hypotheses")
ransac_register_times_raw = _raw("mi_ransac_register_times")


class Fgr:
    """mi_fgr_params, held in a namespace: the module's own Structures are the thirteen that _C_TYPES names and
    tests/test_capi_prototypes.py counts; the compiler checks this one's layout against the header's in tests/test_fgr_abi.py."""
    C_TYPE = "mi_fgr_params"

    class Params(C.Structure):
        _fields_ = [("max_distance", C.c_float), ("division_factor", C.c_float), ("decrease_every", C.c_int), ("max_iterations", C.c_int),
                    ("tuple_scale", C.c_float), ("max_tuples", C.c_int), ("tuple_trials", C.c_int), ("seed", C.c_ulonglong),
                    ("eps_rotation", C.c_float), ("eps_translation", C.c_float), ("sync_every", C.c_int), ("verbose", C.c_int),
                    ("reserved", C.c_int * 8)]


FGR_MAX_TUPLES = 1 << 20         # MI_FGR_MAX_TUPLES
RANSAC_MAX_HYPOTHESES = 1 << 22  # MI_RANSAC_MAX_HYPOTHESES


def fgr_params(max_distance, **kw):
    """mi_fgr_params_default with max_distance and any other field set: division_factor, decrease_every, max_iterations, tuple_scale,
    max_tuples, tuple_trials, seed, eps_rotation, eps_translation, sync_every, verbose."""
    for k in kw:
        if k == "reserved" or k not in [f[0] for f in Fgr.Params._fields_]:
            raise TypeError("mi_fgr_params has no field %r" % k)
    return _params(Fgr.Params, "mi_fgr_params_default", dict(kw, max_distance=max_distance))


def fgr_used_capacity(params, matches):
    """The largest `used` mi_fgr_register can report for these params over `matches` correspondences: what weights and used_src are sized for."""
    if not params.tuple_scale > 0:
        return max(int(matches), 1)
    trials = params.tuple_trials if params.tuple_trials > 0 else min(100 * int(matches), RANSAC_MAX_HYPOTHESES)
    return max(3 * min(trials, params.max_tuples), 1)


fgr_register_raw = _raw("mi_fgr_register")
fgr_tuples_raw = _raw("mi_fgr_tuples")
fgr_system_raw = _raw("mi_fgr_system")
fgr_register_times_raw = _raw("mi_fgr_register_times")


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
    return int(lib().mi_icp_auto_batch(n_moving_total, m_fixed_total, world, 1 if source_sharded else 0, 1 if every_pair_search else 0))


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


selftest_cloud_range_raw = _raw("mi_selftest_cloud_range")


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


# the C type of every Structure above (tests/test_capi_prototypes.py has the compiler check each layout against the header's)
_C_TYPES = {IcpParams: "mi_icp_params", CpdParams: "mi_cpd_params", NicpParams: "mi_nicp_params", PrepareParams: "mi_prepare_params",
            OutlierParams: "mi_outlier_params", OutlierStats: "mi_outlier_stats", IssParams: "mi_iss_params", ClusterParams: "mi_cluster_params",
            PlaneParams: "mi_plane_params", NdtParams: "mi_ndt_params", RansacParams: "mi_ransac_params", IcpBatchInfo: "mi_icp_batch_info",
            CpdBatchInfo: "mi_cpd_batch_info"}


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

    # ---- ms per stage of the last call of each kind: mi_<key>_times fills eight doubles, these are their labels
    _TIMES = {
        "voxel_downsample": ("workspace", "upload", "range", "sort", "sums", "download", "unused", "total"),
        "knn_search": ("workspace", "upload", "check", "grid", "order", "search", "download", "total"),
        "estimate_normals": ("workspace", "upload", "check", "grid", "order", "fused", "download", "total"),
        "remove_outliers": ("workspace", "upload", "check", "grid", "order", "kernel", "finish", "total"),
        "iss_keypoints": ("workspace", "upload", "check", "grid", "order", "saliency", "finish", "total"),
        "mls_smooth": ("workspace", "upload", "check", "grid", "order", "fit", "download", "total"),
        "radius_search": ("workspace", "front", "count", "scan", "fill", "sort", "download", "total"),
        "cluster_dbscan": ("workspace", "upload", "grid", "count", "link", "resolve", "finish", "total"),
        "segment_plane": ("workspace", "upload", "check", "hypotheses", "count", "argmax", "refine", "total"),
        "icp_plane": ("workspace", "upload", "check", "grid", "order", "iterations", "download", "total"),
        "icp_gicp": ("workspace", "upload", "check", "grid", "order", "iterations", "download", "total"),
        "evaluate_registration": ("workspace", "upload", "check", "grid", "order", "step", "download", "total"),
        "pose_graph": ("workspace", "upload", "lists", "linearise", "solve", "candidate", "download", "total"),
        "icp_color": ("workspace", "upload", "check", "grid", "order", "iterations", "download", "total"),
        "ndt": ("workspace", "upload", "check", "table", "order", "iterations", "download", "total"),
        "fpfh_features": ("workspace", "upload", "check", "grid", "order", "kernels", "download", "total"),
        "scan_context": ("workspace", "upload", "check", "unused3", "unused4", "kernels", "download", "total"),
        "tsdf": ("workspace", "upload", "check", "sampling", "sort", "fusion", "download", "total"),
        "feature_match": ("workspace", "upload", "check", "unused3", "unused4", "kernels", "download", "total"),
        "ransac_register": ("workspace", "upload", "hypotheses", "count", "argmax", "refine", "unused6", "total"),
        "fgr_register": ("workspace", "upload", "check", "tuples", "gather", "iterations", "download", "total"),
        "icp_load": ("workspace", "upload_moving", "order_moving", "upload_fixed", "hierarchy", "grid", "reset", "total"),
    }

    def _times(self, name):
        out = (C.c_double * 8)()
        _check(getattr(lib(), "mi_%s_times" % name)(self._h, out))
        return dict(zip(self._TIMES[name], list(out)))

    # ---- ICP
    def icp_register(self, before, after, params):
        before, after = _cloud(before), _cloud(after)
        T = (C.c_float * 16)()
        it, err = C.c_int(0), C.c_float(0)
        _check(lib().mi_icp_register(self._h, _ptr(before), before.shape[0], _ptr(after), after.shape[0], C.byref(params), T,
                                     C.byref(it), C.byref(err)))
        return _T_to_Rt(T) + (it.value, err.value)

    def icp_register_batch(self, befores, afters, params, before_range=None, after_range=None):
        """B registrations under one set of rules (mi_icp_register_batch).  befores / afters: two lists of (n, 3) arrays -- or two
        (N, 3) arrays plus before_range / after_range, (B, 2) integer arrays of (first point, count).  Returns (R [B,3,3], t [B,3],
        iterations [B], error [B], stop_reason [B], info)."""
        clouds, B, T, it, err, why = _batch_call(befores, afters, before_range, after_range)
        info = IcpBatchInfo()
        _check(icp_register_batch_raw(self._h, B, *map(_ptr, clouds), C.addressof(params), T.ctypes.data, it.ctypes.data, err.ctypes.data, why.ctypes.data,
                                      C.addressof(info)))
        return _batch_Rt(T) + (it, err, why, info)

    def cpd_register_batch(self, befores, afters, params, before_range=None, after_range=None):
        """B CPD registrations under one set of rules (mi_cpd_register_batch).  befores / afters: two lists of (n, 3) arrays -- or two
        (N, 3) arrays plus before_range / after_range, (B, 2) integer arrays of (first point, count).  Returns (sR [B,3,3], t [B,3],
        scale [B], iterations [B], error [B], stop_reason [B], info)."""
        clouds, B, T, it, err, why = _batch_call(befores, afters, before_range, after_range)
        scale, info = np.zeros(B, np.float32), CpdBatchInfo()
        _check(cpd_register_batch_raw(self._h, B, *map(_ptr, clouds), C.addressof(params), T.ctypes.data, scale.ctypes.data, it.ctypes.data, err.ctypes.data,
                                      why.ctypes.data, C.addressof(info)))
        return _batch_Rt(T) + (scale, it, err, why, info)

    def icp_load(self, before, after, params):
        before, after = _cloud(before), _cloud(after)
        _check(lib().mi_icp_load(self._h, _ptr(before), before.shape[0], _ptr(after), after.shape[0], C.byref(params)))

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
        return _T_to_Rt(T) + (it.value, err.value, why.value)

    # ---- primitives
    def nn_search(self, src, tgt, dist_mode=DIST_CPU_ROUNDING, nn_mode=NN_AUTO):
        src, tgt = _cloud(src), _cloud(tgt)
        n = src.shape[0]
        idx, d2 = np.empty(n, np.int32), np.empty(n, np.float32)
        _check(lib().mi_nn_search_ex(self._h, _ptr(src), n, _ptr(tgt), tgt.shape[0], dist_mode, nn_mode, _ptr(idx), _ptr(d2)))
        return idx, d2

    def kabsch(self, src, tgt, idx, keep=None):
        src, tgt = _cloud(src), _cloud(tgt)
        idx = np.ascontiguousarray(idx, np.int32)
        keep = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        R9, t3, used = (C.c_float * 9)(), (C.c_float * 3)(), C.c_int(0)
        _check(lib().mi_kabsch(self._h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(idx), _ptr(keep), R9, t3, C.byref(used)))
        return np.array(R9, np.float32).reshape(3, 3).T.copy(), np.array(t3, np.float32), used.value

    def cross_moments(self, src, tgt, idx, keep=None):
        """{pairs, sum src, sum tgt, sum tgt_r src_c} over the kept pairs (src[i], tgt[idx[i]]), fp64."""
        src, tgt = _cloud(src), _cloud(tgt)
        idx = np.ascontiguousarray(idx, np.int32)
        keep = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        out = (C.c_double * 16)()
        _check(lib().mi_cross_moments(self._h, _ptr(src), src.shape[0], _ptr(tgt), tgt.shape[0], _ptr(idx), _ptr(keep), out))
        return np.array(out, np.float64)

    def transform_mse(self, src, R, t, tgt=None, idx=None, keep=None, divide_by_pairs=True, want_cloud=True):
        src = _cloud(src)
        n = src.shape[0]
        R9 = np.ascontiguousarray(np.asarray(R, np.float32).T).reshape(9)
        t3 = np.ascontiguousarray(t, np.float32)
        out, mse = (np.empty((n, 3), np.float32) if want_cloud else None), C.c_float(0)
        if tgt is None:
            idx = keep = None
        else:
            tgt, idx = _cloud(tgt), np.ascontiguousarray(idx, np.int32)
            keep = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        _check(lib().mi_transform_mse(self._h, _ptr(src), n, _ptr(R9), _ptr(t3), _ptr(tgt), 0 if tgt is None else tgt.shape[0], _ptr(idx), _ptr(keep),
                                      1 if divide_by_pairs else 0, _ptr(out), C.byref(mse) if tgt is not None else None))
        return out, (mse.value if tgt is not None else None)

    # ---- CPD
    def cpd_register(self, before, after, params):
        before, after = _cloud(before), _cloud(after)
        T = (C.c_float * 16)()
        it, err, sc = C.c_int(0), C.c_float(0), C.c_float(0)
        _check(lib().mi_cpd_register(self._h, _ptr(before), before.shape[0], _ptr(after), after.shape[0], C.byref(params), T,
                                     C.byref(sc), C.byref(it), C.byref(err)))
        return _T_to_Rt(T) + (sc.value, it.value, err.value)

    def cpd_sigma_squared(self, before, after, mode=SIGMA2_EXACT):
        before, after = _cloud(before), _cloud(after)
        s = C.c_float(0)
        _check(lib().mi_cpd_sigma_squared_mode(self._h, _ptr(before), before.shape[0], _ptr(after), after.shape[0], mode, C.byref(s)))
        return s.value

    def cpd_estep(self, y, x, constant, sigma2):
        y, x = _cloud(y), _cloud(x)
        m, n = y.shape[0], x.shape[0]
        p1, pt1, px, L = np.empty(m, np.float32), np.empty(n, np.float32), np.empty((m, 3), np.float32), C.c_float(0)
        _check(lib().mi_cpd_estep(self._h, _ptr(y), m, _ptr(x), n, constant, sigma2, _ptr(p1), _ptr(pt1), _ptr(px), C.byref(L)))
        return p1, pt1, px, L.value

    def cpd_estep_truncated(self, y, x, constant, sigma2, truncate=1e-3):
        y, x = _cloud(y), _cloud(x)
        m, n = y.shape[0], x.shape[0]
        p1, pt1, px, L = np.empty(m, np.float32), np.empty(n, np.float32), np.empty((m, 3), np.float32), C.c_float(0)
        _check(lib().mi_cpd_estep_truncated(self._h, _ptr(y), m, _ptr(x), n, constant, sigma2, truncate, _ptr(p1), _ptr(pt1), _ptr(px), C.byref(L)))
        return p1, pt1, px, L.value

    def cpd_estep_fgt(self, y, x, weight, sigma2, sigma2_init, ratio_of_far_field=10.0, order_of_truncation=8):
        y, x = _cloud(y), _cloud(x)
        m, n = y.shape[0], x.shape[0]
        p1, pt1, px, L = np.empty(m, np.float32), np.empty(n, np.float32), np.empty((m, 3), np.float32), C.c_float(0)
        _check(lib().mi_cpd_estep_fgt(self._h, _ptr(y), m, _ptr(x), n, weight, sigma2, sigma2_init, ratio_of_far_field,
                                      int(order_of_truncation), _ptr(p1), _ptr(pt1), _ptr(px), C.byref(L)))
        return p1, pt1, px, L.value

    def fgt_kcenter(self, cloud, K):
        cloud = _cloud(cloud)
        centers, cluster = np.empty((K, 3), np.float32), np.empty(cloud.shape[0], np.int32)
        _check(lib().mi_fgt_kcenter(self._h, _ptr(cloud), cloud.shape[0], int(K), _ptr(centers), _ptr(cluster)))
        return centers, cluster

    def fgt_kcenter_guided(self, cloud, K, guess):
        """-> centers, cluster, picked (the sweep's choices), verified (leading entries of `guess` that were the sweep's own; -1: no replay)"""
        cloud = _cloud(cloud)
        guess = np.ascontiguousarray(guess, np.int32)
        centers, cluster = np.empty((K, 3), np.float32), np.empty(cloud.shape[0], np.int32)
        picked, verified = np.empty(K, np.int32), C.c_int(-2)
        _check(lib().mi_fgt_kcenter_guided(self._h, _ptr(cloud), cloud.shape[0], int(K), _ptr(guess), int(guess.shape[0]), _ptr(centers),
                                           _ptr(cluster), _ptr(picked), C.byref(verified)))
        return centers, cluster, picked, verified.value

    def cpd_mstep(self, before, after, p1, pt1, px, const_scale, scale=1.0, sigma2=0.0):
        before, after = _cloud(before), _cloud(after)
        p1, pt1, px = (np.ascontiguousarray(a, np.float32) for a in (p1, pt1, px))
        R9, t3 = (C.c_float * 9)(), (C.c_float * 3)()
        s, s2 = C.c_float(scale), C.c_float(sigma2)
        _check(lib().mi_cpd_mstep(self._h, _ptr(before), before.shape[0], _ptr(after), after.shape[0], _ptr(p1), _ptr(pt1), _ptr(px),
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
        _check(lib().mi_nicp_register(self._h, _ptr(before), before.shape[0], _ptr(after), after.shape[0], C.byref(params),
                                      _ptr(heads), _ptr(subcloud_idx), sn, T, C.byref(it), C.byref(err)))
        return _T_to_Rt(T) + (it.value, err.value)

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
        out, got = np.empty((n + n_out, 3), np.float32), C.c_int(0)
        _check(lib().mi_prepare_cloud(self._h, _ptr(raw), raw.shape[0], _ptr(sub), n, _ptr(shuf), _ptr(rows), _ptr(nu), n_noise, _ptr(ou), n_out,
                                      C.byref(p), _ptr(out), C.byref(got)))
        assert got.value == n + n_out
        return out

    # ---- voxel-grid downsampling
    def voxel_downsample(self, xyz, voxel, origin=None, want_counts=False, want_coords=False, want_map=False):
        """Voxel-grid centroids (mi_voxel_downsample): one row per occupied voxel, ascending by (cz, cy, cx).  Returns the centroids
        [rows, 3], followed by whatever was asked for, in this order: counts [rows], voxel coordinates [rows, 3], and the output row
        of every input point [n]."""
        xyz = _cloud(xyz)
        n = xyz.shape[0]
        origin = None if origin is None else np.ascontiguousarray(origin, np.float32).reshape(3)
        out = np.empty((n, 3), np.float32)
        counts = np.empty(n, np.int32) if want_counts else None
        coords = np.empty((n, 3), np.int32) if want_coords else None
        vmap = np.empty(n, np.int32) if want_map else None
        rows = C.c_int(0)
        _check(voxel_downsample_raw(self._h, xyz.ctypes.data, n, float(voxel), _ptr(origin), out.ctypes.data, C.addressof(rows), _ptr(counts), _ptr(coords),
                                    _ptr(vmap)))
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
        return self._times("voxel_downsample")

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
        _check(knn_search_raw(self._h, qp, n, cloud.ctypes.data, m, int(k), int(dist_mode), float(max_d2), idx.ctypes.data, _ptr(d2), _ptr(count)))
        res = [idx] + ([d2] if want_d2 else []) + ([count] if want_count else [])
        return res[0] if len(res) == 1 else tuple(res)

    def knn_search_times(self):
        """ms per stage of the last knn_search: workspace, upload, check, grid, order, search, download, total (mi_knn_search_times)."""
        return self._times("knn_search")

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
        _check(estimate_normals_raw(self._h, cloud.ctypes.data, n, int(k), int(dist_mode), float(max_d2), _ptr(view), normals.ctypes.data, _ptr(curvature), _ptr(count)))
        res = [normals] + ([curvature] if want_curvature else []) + ([count] if want_count else [])
        return res[0] if len(res) == 1 else tuple(res)

    def estimate_normals_times(self):
        """ms per stage of the last estimate_normals: workspace, upload, check, grid, order, fused, download, total (mi_estimate_normals_times)."""
        return self._times("estimate_normals")

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
        _check(remove_outliers_raw(self._h, cloud.ctypes.data, n, C.addressof(params), out_xyz.ctypes.data, out_index.ctypes.data, C.addressof(out_n),
                                   _ptr(keep), _ptr(mean_distance), _ptr(neighbours), None if stats is None else C.addressof(stats)))
        res = [out_xyz[:out_n.value].copy(), out_index[:out_n.value].copy()]
        res += [a for a in (keep, mean_distance, neighbours, stats) if a is not None]
        return tuple(res)

    def remove_outliers_times(self):
        """ms per stage of the last remove_outliers: workspace, upload, check, grid, order, kernel, finish, total (mi_remove_outliers_times)."""
        return self._times("remove_outliers")

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
        _check(iss_keypoints_raw(self._h, cloud.ctypes.data, n, C.addressof(params), out_xyz.ctypes.data, out_index.ctypes.data, C.addressof(out_n),
                                 _ptr(is_keypoint), _ptr(saliency), _ptr(eigenvalues), _ptr(neighbours)))
        res = [out_xyz[:out_n.value].copy(), out_index[:out_n.value].copy()]
        res += [a for a in (is_keypoint, saliency, eigenvalues, neighbours) if a is not None]
        return tuple(res)

    def iss_keypoints_times(self):
        """ms per stage of the last iss_keypoints: workspace, upload, check, grid, order, saliency, finish, total (mi_iss_keypoints_times)."""
        return self._times("iss_keypoints")

    # ---- moving-least-squares smoothing
    def mls_smooth(self, cloud, params, queries=None, want_normals=False, want_curvature=False, want_neighbours=False, want_status=False):
        """Moving-least-squares smoothing (mi_mls_smooth; params: mls_params(radius=...)): the queries (None: the cloud's own points)
        projected onto the polynomial fitted to the cloud around them, [nq, 3] float32; then, as asked for and in this order: normals
        [nq, 3] float32, curvature [nq] float32, neighbours [nq] int32 (the ball's count, the query's own copy included) and status
        [nq] uint8 (Mls.QUADRATIC, Mls.PLANE, Mls.UNTOUCHED).  Alone, the smoothed queries are returned as an array, not a tuple."""
        cloud = _cloud(cloud)
        queries = None if queries is None else _cloud(queries)
        nq = cloud.shape[0] if queries is None else queries.shape[0]
        out_xyz = np.empty((nq, 3), np.float32)
        normals = np.empty((nq, 3), np.float32) if want_normals else None
        curvature = np.empty(nq, np.float32) if want_curvature else None
        neighbours = np.empty(nq, np.int32) if want_neighbours else None
        status = np.empty(nq, np.uint8) if want_status else None
        _check(mls_smooth_raw(self._h, cloud.ctypes.data, cloud.shape[0], _ptr(queries), nq, C.addressof(params), out_xyz.ctypes.data, _ptr(normals),
                              _ptr(curvature), _ptr(neighbours), _ptr(status)))
        res = [out_xyz] + [a for a in (normals, curvature, neighbours, status) if a is not None]
        return out_xyz if len(res) == 1 else tuple(res)

    def mls_smooth_times(self):
        """ms per stage of the last mls_smooth: workspace, upload, check, grid, order, fit, download, total (mi_mls_smooth_times)."""
        return self._times("mls_smooth")

    # ---- every neighbour within a radius
    def radius_count(self, cloud, radius, query=None, dist_mode=DIST_CPU_ROUNDING):
        """The counts-only form of mi_radius_search: (offsets [n + 1] int64, total).  Row i holds offsets[i + 1] - offsets[i] cloud points
        within `radius` of query i (query None: the cloud's own points, point i itself skipped by index); no list is built and the total
        has no limit."""
        cloud = _cloud(cloud)
        query = None if query is None else _cloud(query)
        n = cloud.shape[0] if query is None else query.shape[0]
        offsets, total = np.empty(n + 1, np.int64), C.c_longlong(0)
        _check(radius_search_raw(self._h, _ptr(query), n, cloud.ctypes.data, cloud.shape[0], float(radius), int(dist_mode), 1, offsets.ctypes.data,
                                 None, None, 0, C.addressof(total)))
        return offsets, total.value

    def radius_search(self, cloud, radius, query=None, dist_mode=DIST_CPU_ROUNDING, sorted=True, want_d2=True, capacity=None):
        """Every cloud point within `radius` of every query, as CSR lists (mi_radius_search): offsets [n + 1] int64, idx [total] int32 and,
        if asked for, d2 [total] float32; row i is idx[offsets[i]:offsets[i + 1]].  query None: the cloud's own points, point i itself
        skipped by index.  sorted: every row ascending by (d2 bits, index), so its head is mi_knn_search's row under the limit radius^2;
        otherwise the order is unspecified but the same on every call.  capacity None: one call for the counts and one to fill arrays of
        exactly that size -- this costs a second count pass; a caller who knows a bound passes it as capacity and pays one call, and gets
        a MiSlamError naming the total if the bound was short."""
        cloud = _cloud(cloud)
        query = None if query is None else _cloud(query)
        n = cloud.shape[0] if query is None else query.shape[0]
        if capacity is None:
            capacity = max(self.radius_count(cloud, radius, query, dist_mode)[1], 1)
        offsets, total = np.empty(n + 1, np.int64), C.c_longlong(0)
        idx = np.empty(int(capacity), np.int32)
        d2 = np.empty(int(capacity), np.float32) if want_d2 else None
        _check(radius_search_raw(self._h, _ptr(query), n, cloud.ctypes.data, cloud.shape[0], float(radius), int(dist_mode), 1 if sorted else 0,
                                 offsets.ctypes.data, idx.ctypes.data, _ptr(d2), int(capacity), C.addressof(total)))
        if total.value > capacity:
            raise MiSlamError("mi_radius_search: %d neighbours in all, capacity %d: nothing was written" % (total.value, capacity))
        res = [offsets, idx[:total.value]] + ([d2[:total.value]] if want_d2 else [])
        return tuple(res)

    def radius_grid(self):
        """(nx, ny, nz) of the cell grid the last radius_search or radius_count walked (mi_selftest_radius_grid)."""
        dims = (C.c_int * 3)()
        _check(lib().mi_selftest_radius_grid(self._h, dims))
        return tuple(dims)

    def radius_search_times(self):
        """ms per stage of the last radius_search or radius_count: workspace, front, count, scan, fill, sort, download, total (mi_radius_search_times)."""
        return self._times("radius_search")

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
        _check(cluster_dbscan_raw(self._h, cloud.ctypes.data, n, C.addressof(params), labels.ctypes.data, C.addressof(n_clusters), _ptr(sizes), n, _ptr(core),
                                  _ptr(grouped), C.addressof(n_grouped) if want_grouped else None))
        res = [labels, n_clusters.value]
        res += ([sizes[:n_clusters.value].copy()] if want_sizes else []) + ([core] if want_core else []) + ([grouped[:n_grouped.value].copy()] if want_grouped else [])
        return tuple(res)

    def cluster_dbscan_times(self):
        """ms per stage of the last cluster_dbscan: workspace, upload (with the check), grid (with the order), count, link, resolve, finish, total (mi_cluster_dbscan_times)."""
        return self._times("cluster_dbscan")

    # ---- the dominant planes of a cloud
    @staticmethod
    def _axis(axis):
        if axis is None:
            return None
        axis = np.ascontiguousarray(axis, np.float32)
        if axis.shape != (3,):
            raise ValueError("axis must have 3 components")
        return axis

    def segment_plane(self, cloud, distance_threshold, hypotheses=1000, seed=0, refine_iterations=2, max_planes=1, min_inliers=3, axis=None,
                      min_axis_cosine=0.0, want_labels=True, want_rmse=False, want_winners=False):
        """The dominant planes of a cloud by hypothesise and verify (mi_segment_plane): planes [n_planes, 4] float32 (a, b, c, d with
        a x + b y + c z + d = 0, in the order found) and plane_inliers [n_planes] int32; then, as asked for and in this order: labels [n]
        int32 (the plane's number or -1), rmse [n_planes] float32 and winners [n_planes] int32 (the winning hypothesis of each round).
        axis: only planes whose normal is within acos(min_axis_cosine) of +-axis."""
        cloud, axis = _cloud(cloud), self._axis(axis)
        n, P = cloud.shape[0], max(int(max_planes), 1)
        planes, inliers, found = np.empty((P, 4), np.float32), np.empty(P, np.int32), C.c_int(0)
        labels = np.empty(n, np.int32) if want_labels else None
        rmse = np.empty(P, np.float32) if want_rmse else None
        winners = np.empty(P, np.int32) if want_winners else None
        _check(segment_plane_raw(self._h, cloud.ctypes.data, n, float(distance_threshold), int(hypotheses), int(seed) & (2 ** 64 - 1), int(refine_iterations),
                                 int(max_planes), int(min_inliers), _ptr(axis), float(min_axis_cosine), planes.ctypes.data, C.addressof(found),
                                 inliers.ctypes.data, _ptr(labels), _ptr(rmse), _ptr(winners)))
        k = found.value
        res = [planes[:k].copy(), inliers[:k].copy()]
        res += ([labels] if want_labels else []) + ([rmse[:k].copy()] if want_rmse else []) + ([winners[:k].copy()] if want_winners else [])
        return tuple(res)

    def segment_plane_hypotheses(self, cloud, distance_threshold, hypotheses=1000, seed=0, axis=None, min_axis_cosine=0.0, first=0, count=None):
        """Hypotheses first .. first + count - 1 of segment_plane's round 0 (mi_segment_plane_hypotheses): triples [count, 3] int32 (the
        caller's indices), valid [count] uint8, plane4 [count, 4] float32 (zeros where invalid), inlier_count [count] int32."""
        cloud, axis = _cloud(cloud), self._axis(axis)
        count = int(hypotheses) - int(first) if count is None else int(count)
        rows = max(count, 1)
        triples, valid = np.empty((rows, 3), np.int32), np.empty(rows, np.uint8)
        plane4, inl = np.empty((rows, 4), np.float32), np.empty(rows, np.int32)
        _check(segment_plane_hypotheses_raw(self._h, cloud.ctypes.data, cloud.shape[0], float(distance_threshold), int(hypotheses), int(seed) & (2 ** 64 - 1),
                                            _ptr(axis), float(min_axis_cosine), int(first), count, triples.ctypes.data, valid.ctypes.data,
                                            plane4.ctypes.data, inl.ctypes.data))
        return triples, valid, plane4, inl

    def segment_plane_times(self):
        """ms per stage of the last segment_plane, summed over its rounds: workspace, upload, check, hypotheses, count, argmax, refine (with
        the flags, the labels, the peel and the downloads), total (mi_segment_plane_times)."""
        return self._times("segment_plane")

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
                                      C.addressof(params), _ptr(T0), T.ctypes.data, C.addressof(it), C.addressof(err),
                                      C.addressof(why)))
        return _T_to_Rt(T) + (it.value, err.value, why.value)

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
                                _ptr(T0), int(dist_mode), float(max_d2), sums.ctypes.data, centre.ctypes.data,
                                _ptr(idx)))
        return (sums, centre, idx) if want_idx else (sums, centre)

    def icp_plane_times(self):
        """ms per stage of the last icp_plane_register / plane_system: workspace, upload, check, grid, order, iterations, download, total
        (mi_icp_plane_times)."""
        return self._times("icp_plane")

    # ---- the quality of a pose
    def evaluate_registration(self, before, after, T=None, pairs=None, dist_mode=DIST_CPU_ROUNDING, max_d2=np.inf, want_sums=False, want_information=True,
                              want_idx=False, want_d2=False):
        """Fitness and inlier RMSE of `before` under the [4, 4] transform T (indexed [row, col]; None: the identity) against `after`
        (mi_evaluate_registration).  pairs None: every moving point's nearest fixed point within max_d2; else int32 [n], -1 or the fixed
        index to pair moving point i with (feature matches under a RANSAC or FGR pose).  Returns (fitness, inlier_rmse) and then, each if
        asked for, sums float64 [32], information float64 [6, 6] (rotation first, about the origin: a pose-graph edge's weight), idx
        int32 [n] (-1: no pair) and d2 float32 [n] (+inf: no pair)."""
        before, after = _cloud(before), _cloud(after)
        n = before.shape[0]
        T0 = _T16(T)
        if pairs is not None:
            pairs = np.ascontiguousarray(pairs, np.int32)
            if pairs.shape != (n,):
                raise ValueError("pairs must hold one fixed index (or -1) per moving point")
        fitness, rmse = C.c_double(0), C.c_double(0)
        sums = np.zeros(32, np.float64) if want_sums else None
        info = np.zeros((6, 6), np.float64) if want_information else None
        idx = np.empty(n, np.int32) if want_idx else None
        d2 = np.empty(n, np.float32) if want_d2 else None
        _check(evaluate_registration_raw(self._h, before.ctypes.data, n, after.ctypes.data, after.shape[0], _ptr(T0), _ptr(pairs), int(dist_mode),
                                         float(max_d2), C.addressof(fitness), C.addressof(rmse), _ptr(sums), _ptr(info), _ptr(idx), _ptr(d2)))
        return (fitness.value, rmse.value) + tuple(x for x in (sums, info, idx, d2) if x is not None)

    def evaluate_registration_times(self):
        """ms per stage of the last evaluate_registration: workspace, upload, check, grid (0 with pairs given), order, step, download, total
        (mi_evaluate_registration_times)."""
        return self._times("evaluate_registration")

    # ---- pose-graph optimisation
    def pose_graph_optimize(self, poses, edge_source, edge_target, edge_T, edge_information, edge_uncertain=None, params=None):
        """Optimises the [V, 4, 4] poses (indexed [row, col], scan frame to world) of a graph whose edge e aligns scan edge_source[e] to scan
        edge_target[e] by edge_T[e] with the [6, 6] weight edge_information[e] (mi_pose_graph_optimize; evaluate_registration's T and
        information).  Returns poses [V, 4, 4], weights [E], chi2 [E] and the report: a dict of initial_cost, final_cost, linearisations,
        accepted, pcg_iterations, lambda, stop_reason and pcg_residual."""
        P, src, tgt, Z, info, unc, E = _pose_graph_arrays(poses, edge_source, edge_target, edge_T, edge_information, edge_uncertain)
        params = params if params is not None else pose_graph_params()
        out, w, chi2, report = np.empty_like(P), np.empty(E, np.float64), np.empty(E, np.float64), np.zeros(8, np.float64)
        _check(pose_graph_optimize_raw(self._h, P.ctypes.data, len(P), _ptr(src), _ptr(tgt), _ptr(Z), _ptr(info), _ptr(unc), E, C.addressof(params),
                                       out.ctypes.data, w.ctypes.data, chi2.ctypes.data, report.ctypes.data))
        names = ("initial_cost", "final_cost", "linearisations", "accepted", "pcg_iterations", "lambda", "stop_reason", "pcg_residual")
        rep = {k: (int(v) if k in ("linearisations", "accepted", "pcg_iterations", "stop_reason") else float(v)) for k, v in zip(names, report)}
        return np.swapaxes(out.reshape(-1, 4, 4), 1, 2).copy(), w, chi2, rep

    def pose_graph_system(self, poses, edge_source, edge_target, edge_T, edge_information, edge_uncertain=None, params=None, p=None, solve=False):
        """One linearisation at the given poses and lambda = params.lambda0 (mi_pose_graph_system).  Returns a dict: r [E, 6], chi2 [E],
        w [E], M [E, 21], h [E, 6], diag [V, 21], g [V, 6], cost, and Hp [V, 6] for a given p [V, 6], and with solve x [V, 6],
        pcg_iterations and pcg_residual."""
        P, src, tgt, Z, info, unc, E = _pose_graph_arrays(poses, edge_source, edge_target, edge_T, edge_information, edge_uncertain)
        params = params if params is not None else pose_graph_params()
        V = len(P)
        o = dict(r=np.zeros((E, 6)), chi2=np.zeros(E), w=np.zeros(E), M=np.zeros((E, 21)), h=np.zeros((E, 6)), diag=np.zeros((V, 21)), g=np.zeros((V, 6)))
        pv = None if p is None else np.ascontiguousarray(p, np.float64).reshape(V, 6)
        hp = np.zeros((V, 6)) if pv is not None else None
        x = np.zeros((V, 6)) if solve else None
        pcg, cost = np.zeros(2), C.c_double(0)
        _check(pose_graph_system_raw(self._h, P.ctypes.data, V, _ptr(src), _ptr(tgt), _ptr(Z), _ptr(info), _ptr(unc), E, C.addressof(params), _ptr(pv),
                                     int(bool(solve)), o["r"].ctypes.data, o["chi2"].ctypes.data, o["w"].ctypes.data, o["M"].ctypes.data, o["h"].ctypes.data,
                                     o["diag"].ctypes.data, o["g"].ctypes.data, _ptr(hp), _ptr(x), pcg.ctypes.data, C.addressof(cost)))
        o["cost"] = cost.value
        if hp is not None:
            o["Hp"] = hp
        if solve:
            o.update(x=x, pcg_iterations=int(pcg[0]), pcg_residual=float(pcg[1]))
        return o

    def pose_graph_times(self):
        """ms per stage of the last pose_graph_optimize or pose_graph_system: workspace, upload, lists, linearise, solve, candidate, download,
        total (mi_pose_graph_times)."""
        return self._times("pose_graph")

    # ---- place recognition
    def scan_context(self, clouds_or_xyz, offsets=None, centres=None, params=None):
        """Scan Context descriptors [n_scans, rings, sectors] float32 of many scans in one call (mi_scan_context).  clouds_or_xyz: a list of
        [n_s, 3] clouds, or with offsets [n_scans + 1] one [n, 3] array that holds them all; centres [n_scans, 3]: the sensors' positions
        (None: the origin); z is up."""
        if offsets is None:
            clouds = [_cloud(c) for c in clouds_or_xyz]
            offsets = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
            xyz = np.concatenate(clouds) if clouds else np.zeros((0, 3), np.float32)
        else:
            xyz, offsets = _cloud(clouds_or_xyz), np.ascontiguousarray(offsets, np.int32).reshape(-1)
            if len(offsets) and offsets[-1] > len(xyz):
                raise ValueError("offsets reach past the points")
        xyz = np.ascontiguousarray(xyz, np.float32)
        n_scans = len(offsets) - 1
        params = params if params is not None else scan_context_params()
        if centres is not None:
            centres = np.ascontiguousarray(centres, np.float32)
            if centres.shape != (n_scans, 3):
                raise ValueError("centres is [n_scans, 3]")
        if xyz.shape[0] == 0:
            xyz = np.zeros((1, 3), np.float32)               # a pointer to pass; no offset reaches it
        desc = np.empty((max(n_scans, 0), max(int(params.rings), 0), max(int(params.sectors), 0)), np.float32)
        _check(scan_context_raw(self._h, xyz.ctypes.data, offsets.ctypes.data, n_scans, _ptr(centres), C.addressof(params), desc.ctypes.data))
        return desc

    def scan_context_search(self, query, db, limit=None, params=None, want_second=False):
        """The best row of db [nd, rings, sectors] for every descriptor of query [nq, rings, sectors], every pair at every shift
        (mi_scan_context_search): idx [nq] int32, dist [nq] float32, shift [nq] int32 -- turning the query scan counter-clockwise about z by
        shift * 2 pi / sectors aligns it with scan idx -- then the runner-up's distance [nq] if asked for.  limit [nq]: query i sees the
        rows below limit[i] (<= 0: idx -1, dist inf, shift 0)."""
        params = params if params is not None else scan_context_params()
        shape = (int(params.rings), int(params.sectors))
        query, db = np.ascontiguousarray(query, np.float32), np.ascontiguousarray(db, np.float32)
        if query.ndim != 3 or db.ndim != 3 or query.shape[1:] != shape or db.shape[1:] != shape:
            raise ValueError("query and db are [rows, rings, sectors] with the params' rings and sectors")
        nq, nd = query.shape[0], db.shape[0]
        if limit is not None:
            limit = np.ascontiguousarray(limit, np.int32)
            if limit.shape != (nq,):
                raise ValueError("limit has one entry per query")
        idx, dist, shift = np.empty(nq, np.int32), np.empty(nq, np.float32), np.empty(nq, np.int32)
        second = np.empty(nq, np.float32) if want_second else None
        _check(scan_context_search_raw(self._h, query.ctypes.data, nq, db.ctypes.data, nd, _ptr(limit), C.addressof(params), idx.ctypes.data,
                                       dist.ctypes.data, shift.ctypes.data, _ptr(second)))
        return (idx, dist, shift, second) if want_second else (idx, dist, shift)

    def scan_context_times(self):
        """ms per stage of the last scan_context or scan_context_search: workspace, upload, check, -, -, kernels, download, total
        (mi_scan_context_times)."""
        return self._times("scan_context")

    # ---- the map
    def tsdf_integrate(self, scans, poses, origin, params, map=None):
        """Posed scans fused into a sparse TSDF map (mi_tsdf_integrate): (coord [nv, 3] int32, tsdf [nv] float32, weight [nv] float32), the
        rows ascending by (cz, cy, cx).  scans: a list of [n_s, 3] clouds in their sensors' frames; poses: [K, 4, 4] sensor to world (the
        mathematical matrices, as icp_plane_register returns R and t), or None: identities; origin [3] and params (tsdf_params(voxel_size=..,
        truncation=..)) fix the lattice and the band; map: such a triple to fuse onto, or None.  Two calls inside: one for the number of
        voxels, one to fill arrays of exactly that size."""
        clouds = [_cloud(s) for s in scans]
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in clouds])]).astype(np.int64)
        xyz = np.ascontiguousarray(np.concatenate(clouds) if clouds else np.zeros((0, 3), np.float32), np.float32)
        if xyz.shape[0] == 0:
            xyz = np.zeros((1, 3), np.float32)               # a pointer to pass; no offset reaches it
        T = None
        if poses is not None:
            poses = np.asarray(poses, np.float64)
            if poses.shape != (len(clouds), 4, 4):
                raise ValueError("poses is [K, 4, 4]")
            T = np.ascontiguousarray(poses.transpose(0, 2, 1), np.float32)      # column-major, as the C interface takes them
        origin = np.ascontiguousarray(origin, np.float32).reshape(3)
        coord, tsdf, weight = _tsdf_map(map)
        nv_in, nv = len(coord), C.c_longlong(0)
        args = (self._h, xyz.ctypes.data, offsets.ctypes.data, len(clouds), _ptr(T), origin.ctypes.data, C.addressof(params),
                coord.ctypes.data if nv_in else None, tsdf.ctypes.data if nv_in else None, weight.ctypes.data if nv_in else None, nv_in)
        _check(tsdf_integrate_raw(*args, None, None, None, 0, C.addressof(nv)))
        n = nv.value
        out_coord, out_tsdf, out_weight = np.empty((n, 3), np.int32), np.empty(n, np.float32), np.empty(n, np.float32)
        if n:
            _check(tsdf_integrate_raw(*args, out_coord.ctypes.data, out_tsdf.ctypes.data, out_weight.ctypes.data, n, C.addressof(nv)))
            if nv.value != n:
                raise MiSlamError("mi_tsdf_integrate: %d voxels counted, then %d" % (n, nv.value))
        return out_coord, out_tsdf, out_weight

    def tsdf_extract(self, map, origin, voxel_size, min_weight=1, want_normals=True):
        """The surface of a TSDF map as points with normals (mi_tsdf_extract): (xyz [n, 3] float32, normals [n, 3] float32 or None), by row,
        then axis; the normals point to the observed side, a zero one where the field has no gradient.  Two calls inside, as above."""
        coord, tsdf, weight = _tsdf_map(map)
        origin = np.ascontiguousarray(origin, np.float32).reshape(3)
        nv, found = len(coord), C.c_longlong(0)
        args = (self._h, coord.ctypes.data if nv else None, tsdf.ctypes.data if nv else None, weight.ctypes.data if nv else None, nv,
                origin.ctypes.data, float(voxel_size), float(min_weight))
        _check(tsdf_extract_raw(*args, None, None, 0, C.addressof(found)))
        n = found.value
        xyz = np.empty((n, 3), np.float32)
        normals = np.empty((n, 3), np.float32) if want_normals else None
        if n:
            _check(tsdf_extract_raw(*args, xyz.ctypes.data, _ptr(normals), n, C.addressof(found)))
            if found.value != n:
                raise MiSlamError("mi_tsdf_extract: %d points counted, then %d" % (n, found.value))
        return xyz, normals

    def tsdf_mesh(self, map, origin, voxel_size, min_weight=1.0, normals=True):
        """The surface of a TSDF map as an indexed triangle mesh (mi_tsdf_mesh): (xyz [nv, 3] float32, normals [nv, 3] float32 or None,
        tri [nt, 3] int32).  The vertices are tsdf_extract's crossings that a triangle uses, in its order and with its bits, each stored
        once; the triangles come by cube in row order, wound so that (v1 - v0) x (v2 - v0) points to the observed side, as the normals do.
        A cube with an unobserved corner gives no triangle.  Two calls inside: one for the two counts, one to fill arrays of exactly that
        size."""
        coord, tsdf, weight = _tsdf_map(map)
        origin = np.ascontiguousarray(origin, np.float32).reshape(3)
        nv, nvert, ntri = len(coord), C.c_longlong(0), C.c_longlong(0)
        args = (self._h, coord.ctypes.data if nv else None, tsdf.ctypes.data if nv else None, weight.ctypes.data if nv else None, nv,
                origin.ctypes.data, float(voxel_size), float(min_weight))
        _check(tsdf_mesh_raw(*args, None, None, 0, C.addressof(nvert), None, 0, C.addressof(ntri)))
        n, t = nvert.value, ntri.value
        xyz, tri = np.empty((n, 3), np.float32), np.empty((t, 3), np.int32)
        nrm = np.empty((n, 3), np.float32) if normals else None
        if n and t:
            _check(tsdf_mesh_raw(*args, xyz.ctypes.data, _ptr(nrm), n, C.addressof(nvert), tri.ctypes.data, t, C.addressof(ntri)))
            if (nvert.value, ntri.value) != (n, t):
                raise MiSlamError("mi_tsdf_mesh: %d vertices and %d triangles counted, then %d and %d" % (n, t, nvert.value, ntri.value))
        return xyz, nrm, tri

    def tsdf_raycast(self, map, origin, params, pose, dirs, compact=False):
        """The map's surface as seen from a pose (mi_tsdf_raycast): (depth [n] float32, xyz [n, 3] float32, normals [n, 3] float32), row i for
        ray i, zeros where a ray misses (depth > 0 marks a hit).  map: a (coord, tsdf, weight) triple or None; origin [3]; params:
        tsdf_raycast_params(voxel_size=.., max_range=..); pose: the 4 x 4 matrix sensor to world, or None: the identity; dirs [n, 3] in the
        sensor's frame, any length (pinhole_directions, spherical_directions).  compact=True: the hit rows only, with their ray indices:
        (depth, xyz, normals, index [hits] int64)."""
        coord, tsdf, weight = _tsdf_map(map)
        origin = np.ascontiguousarray(origin, np.float32).reshape(3)
        dirs = _cloud(dirs)
        T = None
        if pose is not None:
            pose = np.asarray(pose, np.float64)
            if pose.shape != (4, 4):
                raise ValueError("pose is [4, 4]")
            T = np.ascontiguousarray(pose.T, np.float32)     # column-major, as the C interface takes it
        nv, n, hits = len(coord), len(dirs), C.c_longlong(0)
        depth, xyz, normals = np.empty(n, np.float32), np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        _check(tsdf_raycast_raw(self._h, coord.ctypes.data if nv else None, tsdf.ctypes.data if nv else None, weight.ctypes.data if nv else None, nv,
                                origin.ctypes.data, C.addressof(params), _ptr(T), dirs.ctypes.data, n, depth.ctypes.data, xyz.ctypes.data,
                                normals.ctypes.data, C.addressof(hits)))
        if not compact:
            return depth, xyz, normals
        index = np.nonzero(depth > 0)[0]
        if len(index) != hits.value:
            raise MiSlamError("mi_tsdf_raycast: %d hits counted, %d rows with a depth" % (hits.value, len(index)))
        return depth[index], xyz[index], normals[index], index

    def tsdf_times(self):
        """ms per stage of the last tsdf_integrate, tsdf_extract, tsdf_mesh or tsdf_raycast: workspace, upload, check, sampling (extraction,
        mesh and ray cast: table), sort (extraction: count + scan; mesh: cases, used crossings, two scans; ray cast: block table), fusion
        (extraction: fill; mesh: vertex and triangle fill; ray cast: cast), download, total (mi_tsdf_times)."""
        return self._times("tsdf")

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
                                        _ptr(count)))
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
                                     C.addressof(params), _ptr(T0), T.ctypes.data, C.addressof(it), C.addressof(err),
                                     C.addressof(why)))
        return _T_to_Rt(T) + (it.value, err.value, why.value)

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
                               _ptr(T0), int(dist_mode), float(max_d2), sums.ctypes.data, centre.ctypes.data,
                               _ptr(idx)))
        return (sums, centre, idx) if want_idx else (sums, centre)

    def icp_gicp_times(self):
        """ms per stage of the last icp_gicp_register / gicp_system: workspace, upload, check, grid, order, iterations, download, total
        (mi_icp_gicp_times)."""
        return self._times("icp_gicp")

    # ---- colored ICP
    def estimate_color_gradients(self, cloud, normals, intensity, k, dist_mode=DIST_CPU_ROUNDING, max_d2=np.inf, want_count=False):
        """Per-point colour gradients from every point's k nearest neighbours (mi_estimate_color_gradients): [n, 3] float32, the gradient of
        the intensity over the point's tangent plane; (0, 0, 0) where a point has fewer than two neighbours, a zero normal or a singular
        system; then count [n] if asked for."""
        cloud, normals = _cloud(cloud), _cloud(normals)
        n = cloud.shape[0]
        if normals.shape != cloud.shape:
            raise ValueError("normals must have one normal per point")
        intensity = _intensity(intensity, n)
        grad = np.empty((n, 3), np.float32)
        count = np.empty(n, np.int32) if want_count else None
        _check(estimate_color_gradients_raw(self._h, cloud.ctypes.data, normals.ctypes.data, intensity.ctypes.data, n, int(k), int(dist_mode), float(max_d2),
                                            grad.ctypes.data, _ptr(count)))
        return (grad, count) if want_count else grad

    @staticmethod
    def _color_fixed(after, after_normals, after_intensity, after_gradients):
        after, normals, grad = _cloud(after), _cloud(after_normals), _cloud(after_gradients)
        if normals.shape != after.shape or grad.shape != after.shape:
            raise ValueError("after_normals and after_gradients must have one row per fixed point")
        return after, normals, _intensity(after_intensity, after.shape[0]), grad

    def icp_color_register(self, before, before_intensity, after, after_normals, after_intensity, after_gradients, params, lambda_geometric=0.968, init=None):
        """Colored ICP of `before` with its intensities onto `after` with its normals, intensities and colour gradients
        (mi_icp_color_register; params: plane_params(...); init: a [4, 4] transform indexed [row, col], None for the identity) ->
        (R [3, 3], t [3], iterations, error, stop_reason)."""
        before = _cloud(before)
        ib = _intensity(before_intensity, before.shape[0])
        after, normals, ia, grad = self._color_fixed(after, after_normals, after_intensity, after_gradients)
        T0 = _T16(init)
        T = np.zeros(16, np.float32)
        it, err, why = C.c_int(0), C.c_float(0), C.c_int(0)
        _check(icp_color_register_raw(self._h, before.ctypes.data, ib.ctypes.data, before.shape[0], after.ctypes.data, normals.ctypes.data, ia.ctypes.data,
                                      grad.ctypes.data, after.shape[0], C.addressof(params), float(lambda_geometric), _ptr(T0), T.ctypes.data,
                                      C.addressof(it), C.addressof(err), C.addressof(why)))
        return _T_to_Rt(T) + (it.value, err.value, why.value)

    def color_system(self, before, before_intensity, after, after_normals, after_intensity, after_gradients, T=None, dist_mode=DIST_CPU_ROUNDING,
                     max_d2=np.inf, lambda_geometric=0.968, want_idx=True):
        """One colored-ICP linearisation at transform T (mi_color_system) -> (sums float64 [32], centre float32 [3], idx int32 [n] if asked
        for: the fixed index of every moving point's pair, -1 where it has none)."""
        before = _cloud(before)
        n = before.shape[0]
        ib = _intensity(before_intensity, n)
        after, normals, ia, grad = self._color_fixed(after, after_normals, after_intensity, after_gradients)
        T0 = _T16(T)
        sums, centre = np.zeros(32, np.float64), np.zeros(3, np.float32)
        idx = np.empty(n, np.int32) if want_idx else None
        _check(color_system_raw(self._h, before.ctypes.data, ib.ctypes.data, n, after.ctypes.data, normals.ctypes.data, ia.ctypes.data, grad.ctypes.data,
                                after.shape[0], _ptr(T0), int(dist_mode), float(max_d2), float(lambda_geometric), sums.ctypes.data, centre.ctypes.data,
                                _ptr(idx)))
        return (sums, centre, idx) if want_idx else (sums, centre)

    def icp_color_times(self):
        """ms per stage of the last icp_color_register / color_system: workspace, upload, check, grid, order, iterations, download, total
        (mi_icp_color_times)."""
        return self._times("icp_color")

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
        _check(ndt_voxels_raw(self._h, xyz.ctypes.data, n, float(voxel), _ptr(o), int(min_points), float(eig_ratio),
                              coord.ctypes.data, mean.ctypes.data, icov.ctypes.data, C.addressof(rows), count.ctypes.data,
                              _ptr(cov), used.ctypes.data))
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
                                origin.ctypes.data, C.addressof(params), _ptr(T0), T.ctypes.data, C.addressof(it),
                                C.addressof(score), C.addressof(why)))
        return _T_to_Rt(T) + (it.value, score.value, why.value)

    def ndt_system(self, before, vox, T=None, neighbourhood=7, outlier_ratio=0.55):
        """One NDT linearisation at transform T (mi_ndt_system) -> (sums float64 [32], centre float32 [3], idx int32 [n]: the row of every
        point's own voxel or -1, terms uint8 [n]: every point's number of terms)."""
        before = _cloud(before)
        coord, mean, icov, origin, voxel = self._ndt_map(vox)
        T0 = _T16(T)
        n = before.shape[0]
        sums, centre, idx, terms = np.zeros(32, np.float64), np.zeros(3, np.float32), np.empty(n, np.int32), np.empty(n, np.uint8)
        _check(ndt_system_raw(self._h, before.ctypes.data, n, coord.ctypes.data, mean.ctypes.data, icov.ctypes.data, coord.shape[0], voxel, origin.ctypes.data,
                              _ptr(T0), int(neighbourhood), float(outlier_ratio), sums.ctypes.data, centre.ctypes.data,
                              idx.ctypes.data, terms.ctypes.data))
        return sums, centre, idx, terms

    def ndt_times(self):
        """ms per stage of the last ndt_register / ndt_system: workspace, upload, check, table, order, iterations, download, total (mi_ndt_times)."""
        return self._times("ndt")

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
        _check(fpfh_features_raw(self._h, cloud.ctypes.data, normals.ctypes.data, n, int(k), int(dist_mode), float(max_d2), fpfh.ctypes.data, _ptr(counts), _ptr(count)))
        res = [fpfh] + ([counts] if want_counts else []) + ([count] if want_count else [])
        return res[0] if len(res) == 1 else tuple(res)

    def fpfh_features_times(self):
        """ms per stage of the last fpfh_features: workspace, upload, check, grid, order, kernels, download, total (mi_fpfh_features_times)."""
        return self._times("fpfh_features")

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
                                 _ptr(d2)))
        return (idx, d2) if want_d2 else idx

    def feature_match_times(self):
        """ms per stage of the last feature_match: workspace, upload, check, -, -, kernels, download, total (mi_feature_match_times)."""
        return self._times("feature_match")

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
                                   t3.ctypes.data, C.addressof(inl), C.addressof(rmse), C.addressof(best), C.addressof(nvalid), _ptr(mask)))
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
        return self._times("ransac_register")

    # ---- Fast Global Registration
    @staticmethod
    def _matches(src, tgt, idx):
        src, tgt = _cloud(src), _cloud(tgt)
        idx = np.ascontiguousarray(idx, np.int32)
        if idx.shape != (src.shape[0],):
            raise ValueError("idx has one entry per source point")
        return src, tgt, idx

    def fgr_register(self, src, tgt, idx, params, init=None, want_weights=False):
        """A pose from correspondences src[i] <-> tgt[idx[i]] (idx -1: none) by Fast Global Registration (mi_fgr_register; params:
        fgr_params(...); init: a [4, 4] transform indexed [row, col], None for the identity) -> (R [3, 3] float32, t [3], iterations, error,
        stop_reason, used, final_mu), then weights [used] float32 and used_src [used] int32 if asked for."""
        src, tgt, idx = self._matches(src, tgt, idx)
        T0, T = _T16(init), np.zeros(16, np.float32)
        it, why, used, err, mu = C.c_int(0), C.c_int(0), C.c_int(0), C.c_float(0), C.c_float(0)
        cap = fgr_used_capacity(params, int((idx >= 0).sum()))
        weights = np.zeros(cap, np.float32) if want_weights else None
        used_src = np.zeros(cap, np.int32) if want_weights else None
        _check(fgr_register_raw(self._h, src.ctypes.data, src.shape[0], tgt.ctypes.data, tgt.shape[0], idx.ctypes.data, C.addressof(params), _ptr(T0),
                                T.ctypes.data, C.addressof(it), C.addressof(err), C.addressof(why), C.addressof(used), C.addressof(mu), _ptr(weights),
                                _ptr(used_src)))
        out = _T_to_Rt(T) + (it.value, err.value, why.value, used.value, np.float32(mu.value))
        return out + (weights[:used.value].copy(), used_src[:used.value].copy()) if want_weights else out

    def fgr_tuples(self, src, tgt, idx, params):
        """The used list of fgr_register (mi_fgr_tuples): (used, used_src [used] int32, used_tgt [used] int32, accepted_trials)."""
        src, tgt, idx = self._matches(src, tgt, idx)
        cap = fgr_used_capacity(params, int((idx >= 0).sum()))
        used_src, used_tgt = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        used, accepted = C.c_int(0), C.c_int(0)
        _check(fgr_tuples_raw(self._h, src.ctypes.data, src.shape[0], tgt.ctypes.data, tgt.shape[0], idx.ctypes.data, C.addressof(params),
                              C.addressof(used), used_src.ctypes.data, used_tgt.ctypes.data, C.addressof(accepted)))
        return used.value, used_src[:used.value].copy(), used_tgt[:used.value].copy(), accepted.value

    def fgr_system(self, src, tgt, idx, params, T=None, applied_updates=0):
        """One linearisation of fgr_register over its used list at transform T with the mu that follows applied_updates updates
        (mi_fgr_system) -> (sums float64 [32], centre float32 [3], mu float)."""
        src, tgt, idx = self._matches(src, tgt, idx)
        T0 = _T16(T)
        sums, centre, mu = np.zeros(32, np.float64), np.zeros(3, np.float32), C.c_double(0)
        _check(fgr_system_raw(self._h, src.ctypes.data, src.shape[0], tgt.ctypes.data, tgt.shape[0], idx.ctypes.data, C.addressof(params), _ptr(T0),
                              int(applied_updates), sums.ctypes.data, centre.ctypes.data, C.addressof(mu)))
        return sums, centre, mu.value

    def fgr_register_times(self):
        """ms per stage of the last fgr_register / fgr_system: workspace, upload, check, tuples (trials, compaction, read-back), gather,
        iterations, download (with the weights pass), total (mi_fgr_register_times)."""
        return self._times("fgr_register")

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
        _check(lib().mi_selftest_sort_pairs(self._h, _ptr(k), _ptr(v), int(k.size), int(bits)))
        return k, v

    def selftest_cloud_range(self, xyz, check=0):
        """The range pass of csrc/cloud_range.hpp over an (n, 3) host cloud: (lo_hi float32[6], lowest refused index or 0x7fffffff).
        check 0: refuse nothing; 1: non-finite points; 2: those and |coordinate| > 1e18 (mi_selftest_cloud_range)."""
        p = np.ascontiguousarray(xyz, dtype=np.float32)
        assert p.ndim == 2 and p.shape[1] == 3
        lo_hi, bad = np.zeros(6, np.float32), C.c_int(-1)
        _check(selftest_cloud_range_raw(self._h, p.ctypes.data, int(p.shape[0]), int(check), lo_hi.ctypes.data, C.byref(bad)))
        return lo_hi, int(bad.value)

    def selftest_icp_schedule(self):
        """What the last ICP step left on the device: dict(order int32[rows], far uint8[rows], cursors int32[4], ticket, sums float64[18]
        = the 16 moments and 2 error sums the last solve read) (mi_selftest_icp_schedule)."""
        f = lib().mi_selftest_icp_schedule
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
        m, n = int(m), int(n)
        out = {}
        if arrays:
            out.update(p1=np.zeros(m, np.float32), pt1=np.zeros(n, np.float32), px=np.zeros((m, 3), np.float32), y=np.zeros((m, 3), np.float32))
        xs, ks, R9, t3 = np.zeros(5, np.float64), np.zeros(14, np.float64), np.zeros(9, np.float32), np.zeros(3, np.float32)
        sc, info = [C.c_float(0) for _ in range(4)], np.zeros(8, np.int32)
        _check(f(self._h, m, n, *[_ptr(out.get(k)) for k in ("p1", "pt1", "px", "y")], xs.ctypes.data, ks.ctypes.data, R9.ctypes.data, t3.ctypes.data,
                 *map(C.byref, sc), info.ctypes.data))
        out.update(xs=xs, ks=ks, R=R9.reshape(3, 3).T.copy(), t=t3, scale=np.float32(sc[0].value), sigma2=np.float32(sc[1].value),
                   sigma2_init=np.float32(sc[2].value), constant=np.float32(sc[3].value))
        out.update(zip(("route", "fused", "rows_x", "rows_k", "reduced", "iterations", "stop_reason"), (int(v) for v in info[:7])))
        return out

    def selftest_nicp_candidates(self, before, after, order_heads):
        """The moments stage and the candidates of nicp_register without its driver (mi_selftest_nicp_candidates): (raw float64[32] -- the sums of the
        clouds taken about their first points --, R [reps, 3, 3], t [reps, 3], approx [reps]) for order_heads [reps, 3]."""
        before, after = _cloud(before), _cloud(after)
        heads = np.ascontiguousarray(order_heads, np.int32).reshape(-1, 3)
        raw, out = np.zeros(32, np.float64), np.zeros((len(heads), 13), np.float32)
        _check(lib().mi_selftest_nicp_candidates(self._h, _ptr(before), before.shape[0], _ptr(after), after.shape[0], _ptr(heads), len(heads), _ptr(raw), _ptr(out)))
        return raw, out[:, :9].reshape(-1, 3, 3).copy(), out[:, 9:12].copy(), out[:, 12].copy()

    def nn_kernel_name(self, n_moving, m_fixed_local, nn_mode=NN_AUTO):
        return lib().mi_nn_kernel_name(self._h, n_moving, m_fixed_local, nn_mode).decode()

    def profile_select(self, kernels=None):
        """Restrict the event timing to these kernels (KERNEL_* ids); None = all."""
        mask = 0xffffffff if kernels is None else sum(1 << k for k in kernels)
        _check(lib().mi_profile_select(self._h, C.c_uint(mask)))

    def profile_reset(self):
        _check(lib().mi_profile_reset(self._h))

    def icp_load_times(self):
        """ms per stage of the last icp_load: workspace, moving upload, moving order, fixed upload, hierarchy, grid, reset, total."""
        return self._times("icp_load")

    def profile_get(self, kernel):
        ms, n = C.c_double(0), C.c_longlong(0)
        _check(lib().mi_profile_get(self._h, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value
