/* mi_slam.h -- C ABI of the MI355X-native point-set-registration core (libmislam.so).
 *
 * This is the drop-in boundary for the reference's GPU registration path.  A thin C++ adapter with the shape of the
 * reference's Common::SlamFunc (source/common/testrunner.h:7-8) binds these entry points; INTEGRATION.md shows the
 * adapter a maintainer would put where source/cuda-slam/gpumain.cpp:12-38 dispatches today.
 *
 * Conventions (all taken from the reference's own boundary):
 *   - clouds are contiguous AoS float xyz, 12 B per point, no padding: Common::Point<float>
 *     (source/common/point.h:6-64), the layout the reference memcpy's to the device as glm::vec3
 *     (source/cuda-slam/icpcuda.cu:71-72);
 *   - `before` is the moving cloud, `after` the fixed one; the result maps before onto after;
 *   - 4x4 results are COLUMN-MAJOR with the translation in column 3, byte-identical to glm::mat4 as built by
 *     Common::ConvertToTransformationMatrix (source/common/common.cpp:353-358) and to a default Eigen::Matrix4f;
 *   - host pointers in, host pointers out; the library owns every device allocation (context workspace);
 *   - every function returns MI_OK (0) or a negative error code instead of the reference's print-and-exit(1)
 *     (include/helper_cuda.h:567-573); mi_last_error() returns the message; nothing is printed unless verbose != 0.
 *
 * The hot path behind it is hand-written HIP for gfx950; there is no CPU fallback: if no HIP device is usable the
 * calls fail with MI_ERR_NO_DEVICE.
 */
#ifndef MI_SLAM_H
#define MI_SLAM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_SLAM_ABI_VERSION 4   /* 4: mi_profile_search_phases, mi_selftest_fail_loads, mi_runtime_info (additive: no signature of version 3 changed), later and additive again: mi_icp_register_batch, mi_cpd_register_batch, mi_voxel_index, mi_voxel_downsample, mi_voxel_downsample_times, mi_knn_search, mi_knn_search_times, mi_estimate_normals, mi_estimate_normals_times, mi_selftest_cpd_last, mi_selftest_nicp_candidates; 3: mi_icp_load_times, mi_cross_moments, mi_icp_auto_batch; 2: mi_cpd_params gained sigma2_mode; mi_dist_info, mi_source_share, mi_cpd_sigma_squared_mode, mi_profile_search_stats, mi_selftest_sort_pairs */

enum {
    MI_OK = 0,
    MI_ERR_INVALID_ARG = -1,
    MI_ERR_NO_DEVICE = -2,
    MI_ERR_HIP = -3,
    MI_ERR_RCCL = -4,
    MI_ERR_STATE = -5
};

/* Distance arithmetic of the nearest-neighbour search.  Both are IEEE fp32 on (dx,dy,dz) = target - source. */
enum {
    MI_DIST_CPU_ROUNDING = 0,   /* ((dx*dx + dy*dy) + dz*dz), every product and sum rounded: bit-identical to the x86-64
                                   cpu-slam build (source/common/point.h:48-50 via common.cpp:452) */
    MI_DIST_FMA = 1             /* fma(dz,dz, fma(dy,dy, dx*dx)): what nvcc's default contraction makes of
                                   GetDistanceSquared (source/cuda-slam/cudacommon.cu:51-55) */
};

/* Execution strategy of the nearest-neighbour search.  Every mode returns the SAME idx[] and d2[] bit for bit (strict '<',
 * lowest index on ties, same fp32 arithmetic); they differ only in how many candidate pairs are evaluated. */
enum {
    MI_NN_AUTO = 0,         /* cell grid for fixed clouds of >= MI_NN_INDEX_MIN_POINTS points per GPU, every pair below (measured crossover at N = M) */
    MI_NN_BRUTEFORCE = 1,   /* every pair, like FindCorrespondences (cudacommon.cu:57-77): N*M distance evaluations */
    MI_NN_TREE = 2,         /* exact search through a box hierarchy over the Morton-sorted fixed cloud */
    MI_NN_GRID = 3          /* exact search through a uniform cell grid over the fixed cloud; lanes the grid cannot serve cheaply
                               (no starting candidate, far outliers, crowded cells) walk the box hierarchy inside the same launch */
};
#define MI_NN_INDEX_MIN_POINTS 10000

/* What a multi-GPU context (mi_ctx_create_dist) splits across its ranks.  Same registration result either way.
 *   TARGET: rank r owns fixed points [M*r/W, M*(r+1)/W) and ALL moving points; one ncclAllReduce(ncclUint64, ncclMin) of the
 *           N packed (min-dist, argmin) keys per iteration, then owner-accumulated moments/error + one 64 x 18-double sum all-reduce.
 *           The every-pair search scales perfectly this way (its work is N*M/W per rank).
 *   SOURCE: every rank holds a replica of the fixed cloud (12 B/point: trivial at 288 GB) and 1/W of the moving points -- the
 *           64-point chunks of the moving cloud's Hilbert order dealt round-robin (rank r: chunks r, r+W, ...; contiguous
 *           slices [N*r/W, N*(r+1)/W) of the caller's order below 256*W points).  No per-point exchange at all, only one
 *           64 x 18-double sum all-reduce per iteration.  The indexed searches need this split to scale: their cost per moving
 *           point hardly depends on how many fixed points a rank holds.
 *   AUTO:   SOURCE when the search runs through an index (cell grid / box hierarchy), TARGET when it is the every-pair search. */
enum {
    MI_SHARD_AUTO = 0,
    MI_SHARD_TARGET = 1,
    MI_SHARD_SOURCE = 2
};

/* How the two centroids and the error of an ICP iteration are summed.
 *   EXACT:          fp64 two-stage sums (the default; correctly rounded to fp32 at the end).
 *   CPU_SEQUENTIAL: cpu-slam's own arithmetic, bit for bit: ONE sequential fp32 running sum per quantity over the kept
 *                   pairs in the caller's point order (GetCenterOfMass common.cpp:281-284, GetMeanSquaredError :259-268).
 *                   That sum is 1.3e-4 off the exact mean at 2e4 points and worse beyond, and it feeds both the translation
 *                   and the stop rule -- choose this mode to retrace cpu-slam's trajectory at sizes where its own summation
 *                   noise exceeds the 1e-4 parity budget.  Round 6: the mode also takes cpu-slam's own CROSS-COVARIANCE -- the kept pairs centred
 *                   in fp32 with those centroids (GetAlignedCloud, common.cpp:525-530) -- instead of the exact one: the two differ by ~1e-7, which
 *                   is nothing unless the matrix is rank-deficient (a first iteration that matches every moving point to the same two fixed points:
 *                   the exact matrix leaves R undetermined, cpu-slam's R is decided by that centring's rounding).  With it -- and the 3 x 3 SVD in IEEE
 *                   arithmetic, developer switch MISLAM_SVD_IEEE=1 -- the device retraces the CPU restatement of cpu-slam bit for bit on the
 *                   reference's convergence and sizes sets (tests/test_gpu_convergence_set.py).  Single-GPU contexts only; costs ~3.3 ms per million
 *                   points per iteration (a sequential fp32 sum cannot be re-associated). */
enum {
    MI_SUM_EXACT = 0,
    MI_SUM_CPU_SEQUENTIAL = 1
};

/* How the per-iteration solve (Ri, ti) is accumulated into the running transform. */
enum {
    MI_COMPOSE_CPU_ADDITIVE = 0,  /* R <- Ri*R ; t <- ti + t   -- source/cpu-slam/basicicp.cpp:43-44 (the oracle's rule) */
    MI_COMPOSE_EXACT = 1          /* T <- Ti*T (4x4)           -- source/cuda-slam/icpcuda.cu:35 */
};

/* Why a registration loop stopped. */
enum {
    MI_STOP_RUNNING = 0,
    MI_STOP_CONVERGED = 1,        /* error < eps                      basicicp.cpp:52 / icpcuda.cu:40 */
    MI_STOP_MAX_ITERATIONS = 2,   /* iterations reached the cap        basicicp.cpp:32 / icpcuda.cu:31 */
    MI_STOP_NO_PAIRS = 3,         /* no correspondence survived filter basicicp.cpp:36 */
    MI_STOP_ERROR_INCREASED = 4,  /* rollback rule                     icpcuda.cu:43-49 */
    MI_STOP_TOLERANCE = 5,        /* CPD: ntol <= tolerance            coherentpointdrift.cpp:106 */
    MI_STOP_SIGMA = 6             /* CPD: sigma^2 <= eps               coherentpointdrift.cpp:106 */
};

typedef struct mi_ctx mi_ctx;   /* opaque: device, stream, workspace, optional RCCL communicator */

/* ----------------------------------------------------------------------------------------------------------------
 * Context.  Hoists device selection, stream/event creation, workspace allocation and (multi-GPU) the communicator out
 * of the registration calls -- the reference allocates and frees everything per call (icpcuda.cu:21-29,56).
 * -------------------------------------------------------------------------------------------------------------- */
int mi_abi_version(void);
const char* mi_last_error(void);
int mi_device_count(int* count);

int mi_ctx_create(int device, mi_ctx** out);
/* Optional: load all device code now (~170 ms) instead of lazily at the first use of each kernel family, where it would stall
 * that registration call (first CPD call on the bunny clouds: 36 ms lazily, 3 ms after this).  For long-lived processes. */
int mi_ctx_preload(mi_ctx* ctx);

/* Multi-GPU, one process per GPU (no reference counterpart: the reference is single-GPU).  What the ranks split is
 * mi_icp_params.shard_mode (MI_SHARD_* above) for ICP -- with the fixed cloud sharded, the per-point packed (min-dist, argmin)
 * keys are combined with ONE ncclAllReduce(ncclUint64, ncclMin) over xGMI per iteration -- and the fixed cloud for CPD.
 * The library creates the communicator and issues every collective on its own stream.
 * unique_id is the 128-byte ncclUniqueId produced by mi_dist_unique_id() on rank 0 and shipped to the other ranks by
 * the caller's bootstrap (torch.distributed store, MPI, a socket ...). */
#define MI_UNIQUE_ID_BYTES 128
int mi_dist_unique_id(void* out_unique_id);
int mi_ctx_create_dist(int device, int rank, int world, const void* unique_id, mi_ctx** out);
int mi_ctx_rank(const mi_ctx* ctx, int* rank, int* world);
/* What the TRANSPORT says about this context (measurement hook: bench.py prints it as proof that the ranks really met):
 * *nranks / *rank as the RCCL communicator reports them (ncclCommCount / ncclCommUserRank; world / rank of an exchange context,
 * 1 / 0 of a single-GPU one), *ranks_seen the sum over all ranks of 2^rank carried through one all-reduce on the context's
 * stream -- bit r set = rank r took part.  Collective: every rank calls it.  Any output may be NULL. */
int mi_dist_info(mi_ctx* ctx, int* nranks, int* rank, unsigned long long* ranks_seen);

/* Which shared objects this library's HIP and RCCL calls actually bind to in THIS process, and their versions -- no device is touched
 * (dladdr on hipStreamSynchronize / ncclAllReduce, ncclGetVersion, hipRuntimeGetVersion).  A launcher that has imported another copy of the ROCm
 * runtime first (PyTorch bundles libamdhip64 / librccl under torch/lib with the same SONAMEs) decides what these resolve to: bench.py prints
 * them in its N > 1 line and refuses to start when two different RCCL objects of different versions are mapped (round 5).
 * Paths are copied into the caller's buffers (truncated to `cap` bytes, always NUL-terminated); any pointer may be NULL. */
int mi_runtime_info(char* hip_path, char* rccl_path, int cap, int* hip_runtime_version, int* rccl_version);

/* The same multi-GPU path over the CALLER's transport instead of RCCL (MPI between nodes, a test harness ...; no reference
 * counterpart either).  Wherever the RCCL context issues an all-reduce, this one drains its stream, copies the operand to
 * pinned host memory, calls `exchange` and copies the result back: `exchange` must combine host_buf[0 .. count) IN PLACE across
 * all `world` ranks -- element-wise unsigned 64-bit MIN for MI_EXCHANGE_MIN_U64, double SUM for MI_EXCHANGE_SUM_F64 -- and
 * return 0, or non-zero to fail the call with MI_ERR_RCCL.  Every rank makes the same sequence of calls.  Results are those
 * of the RCCL context up to the order in which the transport adds the doubles. */
enum { MI_EXCHANGE_MIN_U64 = 0, MI_EXCHANGE_SUM_F64 = 1 };
typedef int (*mi_exchange_fn)(void* user, void* host_buf, size_t count, int kind);
int mi_ctx_create_exchange(int device, int rank, int world, mi_exchange_fn exchange, void* user, mi_ctx** out);

/* Host-side pieces of the multi-GPU protocol (pure functions, usable without a device; the CPU tests drive them over gloo):
 *   mi_shard_range  the contiguous target range [lo, hi) rank `rank` of `world` owns: lo = M*rank/world, hi = M*(rank+1)/world;
 *   mi_source_share how many moving points rank `rank` of `world` works on under MI_SHARD_SOURCE (the 64-point chunks rank,
 *                   rank + world, ... of the cloud's Hilbert order; n*rank/world .. n*(rank+1)/world below 256*world points);
 *   mi_pack_key     the 64-bit key the search emits per source point: IEEE bits of d2 (d2 >= 0, so they order like the
 *                   value) in the high word, the GLOBAL target index in the low word -- an unsigned min over keys is the
 *                   (min distance, lowest index) rule of cudacommon.cu:68 / common.cpp:454, across chunks and across GPUs. */
int mi_shard_range(int m_total, int rank, int world, int* lo, int* hi);
int mi_source_share(int n_total, int rank, int world, int* count);
unsigned long long mi_pack_key(float d2, int global_index);
void mi_unpack_key(unsigned long long key, float* d2, int* global_index);
void mi_ctx_destroy(mi_ctx* ctx);
int mi_ctx_synchronize(mi_ctx* ctx);

/* ----------------------------------------------------------------------------------------------------------------
 * ICP -- replaces GetCudaIcpTransformationMatrix(before, after, eps, maxIterations, iterations, error)
 *        (source/cuda-slam/icpcuda.cuh:5-11, icpcuda.cu:60-76) and, through its modes, reproduces
 *        BasicICP::GetBasicICPTransformationMatrix (source/cpu-slam/basicicp.cpp:23-61), the parity oracle.
 * -------------------------------------------------------------------------------------------------------------- */
typedef struct {
    float eps;                   /* "convergence-epsilon"                (configparser.cpp:244, default 1e-3) */
    int   max_iterations;        /* "max-iterations", -1 = unbounded     (gpumain.cpp:14) */
    float max_distance_squared;  /* "max-distance-squared" (default 1000, configparser.cpp:207); used when filter_pairs */
    int   dist_mode;             /* MI_DIST_* */
    int   compose_mode;          /* MI_COMPOSE_* */
    int   filter_pairs;          /* 1: drop pairs with d2 >= max_distance_squared and average the error over the survivors
                                       (common.cpp:486-499, :267); 0: keep all and divide the error sum by |after|
                                       (cudacommon.cu:138-148) */
    int   abort_on_increase;     /* 1: stop and roll back when the error rises (icpcuda.cu:43-49); 0: cpu-slam never does */
    int   sync_every;            /* iterations enqueued between host checks of the device-side stop flag; 0 = auto.
                                    The stop rule itself is evaluated on the device after EVERY iteration, so the result
                                    does not depend on this value. */
    int   verbose;               /* 1: print "loop_nr %d, error: %f" lines like basicicp.cpp:50 at every host check */
    int   nn_mode;               /* MI_NN_*: how the correspondence search is carried out; the RESULT is identical in every mode */
    int   shard_mode;            /* MI_SHARD_*: what a multi-GPU context splits across ranks (ignored with one rank) */
    int   sum_mode;              /* MI_SUM_*: how the centroids and the error are summed */
    int   reserved[4];
} mi_icp_params;

/* Defaults = cpu-slam semantics (the parity oracle): CPU rounding, additive translation, filtered pairs, no abort. */
void mi_icp_params_default(mi_icp_params* p);
/* The GPU reference's own driver rules (icpcuda.cu:8-58): FMA distance, exact composition, no filter, abort+rollback. */
void mi_icp_params_cuda_slam(mi_icp_params* p);

/* One-call registration.  out_T: 16 floats column-major; iterations/error as the reference's out-params (non-null). */
int mi_icp_register(mi_ctx* ctx, const float* before_xyz, int n_before, const float* after_xyz, int n_after,
                    const mi_icp_params* params, float out_T[16], int* iterations, float* error);

/* Resident-data form of the same loop (what bench.py times: inputs already in HBM when the clock starts).
 *   mi_icp_load   uploads both clouds (AoS -> SoA on device), sizes the workspace, resets the state to identity;
 *   mi_icp_reset  resets the running transform / counters without re-uploading;
 *   mi_icp_run    enqueues up to `max_new_iterations` more iterations of the loop (fewer if a stop rule fires),
 *                 returns after they finished;
 *   mi_icp_result reads the current (T, iterations, error, stop reason). */
int mi_icp_load(mi_ctx* ctx, const float* before_xyz, int n_before, const float* after_xyz, int n_after,
                const mi_icp_params* params);
int mi_icp_reset(mi_ctx* ctx);
int mi_icp_run(mi_ctx* ctx, int max_new_iterations, int* iterations_done);
/* The iterations mi_icp_run enqueues between two host checks when sync_every = 0 -- a pure function of GLOBAL sizes (moving and
 * fixed points over all ranks, rank count, what is sharded, which search runs): every batch ends in a collective, so every rank
 * of a multi-GPU registration must pick the same number. */
int mi_icp_auto_batch(long long n_moving_total, long long m_fixed_total, int world, int source_sharded, int every_pair_search);
int mi_icp_result(mi_ctx* ctx, float out_T[16], int* iterations, float* error, int* stop_reason);

/* ----------------------------------------------------------------------------------------------------------------
 * Batched ICP: many small registrations under ONE set of rules in one call (single-GPU contexts only).
 * A registration of a few thousand points leaves most of the device idle and is bound by launches and host checks; here every
 * problem gets a workgroup of its own and its iterations run inside one kernel, a few hundred problems side by side.  A caller
 * with ONE pair keeps calling mi_icp_register: a single workgroup is slower than the whole device.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct {
    int problems_batched;    /* problems that ran on the batched kernel */
    int problems_fallback;   /* problems that ran through the existing per-problem path inside this call */
    int launches;            /* launches of the batched kernel */
    int reserved[5];
} mi_icp_batch_info;

/* 1 if a problem of these sizes under these rules is carried by the batched kernel, 0 if the call routes it through the
 * existing path.  Pure host function of its arguments (no context, no device), like mi_icp_auto_batch.  Routed: n_before <= 4096
 * and n_after <= 4096 -- a function of the two sizes only -- under MI_SUM_EXACT with verbose = 0, whatever the other fields say
 * (MI_SUM_CPU_SEQUENTIAL and verbose = 1 belong to the single path: its sequential sums, its per-iteration print). */
int mi_icp_batch_route(int n_before, int n_after, const mi_icp_params* params);

/* B independent registrations.  Problem k moves the points before_xyz[3*before_range[2k] ...] (before_range[2k+1] of them) onto
 * after_xyz[3*after_range[2k] ...] (after_range[2k+1] of them); both arrays must reach as far as the ranges say.  Ranges may
 * overlap or coincide (many scans against one map tile, one scan against many).  out_T: 16*B floats (column-major 4x4 each);
 * iterations, error, stop_reason: B entries each, non-null.  info may be NULL.  Problem k's outputs are, BIT FOR BIT, what
 *   mi_icp_register(ctx, before_k, n_k, after_k, m_k, params, ...) followed by mi_icp_result(...)
 * returns on the same context (its developer switches included) -- whatever else is in the batch and in whatever position;
 * nn_mode and sync_every are accepted and, as in the single call, move no bit.  Every problem mi_icp_register accepts is
 * accepted: the ones mi_icp_batch_route does not route run through the existing path inside the call, one after the other.
 * n_problems == 0 is MI_OK.  A range with a negative offset or a count < 1, or a NULL output: MI_ERR_INVALID_ARG, mi_last_error
 * names the problem, nothing has touched the device.  A distributed context: MI_ERR_STATE.
 * The call REPLACES whatever mi_icp_load had loaded: afterwards no problem is loaded (mi_icp_run / mi_icp_result return
 * MI_ERR_STATE until the next mi_icp_load).  max_iterations = -1 on a problem that never meets a stop rule does not return,
 * exactly like the single call -- but every launch of the kernel ends: it carries a bounded number of iterations. */
int mi_icp_register_batch(mi_ctx* ctx, int n_problems,
                          const float* before_xyz, const int* before_range,
                          const float* after_xyz,  const int* after_range,
                          const mi_icp_params* params,
                          float* out_T, int* iterations, float* error, int* stop_reason,
                          mi_icp_batch_info* info);

/* ----------------------------------------------------------------------------------------------------------------
 * Test-grade primitives (one per reference primitive on the path; host in / host out).
 * -------------------------------------------------------------------------------------------------------------- */

/* CUDACommon::GetCorrespondingPoints + FindCorrespondences (cudacommon.cu:272-289, :57-77) /
 * Common::GetCorrespondingPoints search part (common.cpp:441-478):
 * idx[i] = argmin_j |tgt[j] - src[i]|^2, strict '<', lowest index wins ties; d2[i] = that minimum (may be NULL). */
int mi_nn_search(mi_ctx* ctx, const float* src_xyz, int n, const float* tgt_xyz, int m, int dist_mode,
                 int* idx, float* d2);
/* Same, with an explicit MI_NN_* strategy (mi_nn_search uses MI_NN_AUTO). */
int mi_nn_search_ex(mi_ctx* ctx, const float* src_xyz, int n, const float* tgt_xyz, int m, int dist_mode, int nn_mode,
                    int* idx, float* d2);

/* The sums LeastSquaresSVD is built from (the cross-covariance product of cudacommon.cu:196-201 -- CuBlasMultiply -- and the two
 * centroid sums), over the kept pairs (src[i], tgt[idx[i]]):  out16 = { pairs, sum src (3), sum tgt (3), sum tgt_r * src_c (9, row-major
 * in r) }, fp64.  What the reference's own MultiplicationTest checks on its GEMM (cudacommon.cu:319-343: ones(3x100) * ones(100x3) is
 * 100 everywhere) is checked on these. */
int mi_cross_moments(mi_ctx* ctx, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx,
                     const unsigned char* keep, double out16[16]);

/* CUDACommon::LeastSquaresSVD (cudacommon.cu:168-253) / Common::LeastSquaresSVD (common.cpp:517-552) on the pairs
 * (src[i], tgt[idx[i]]), i = 0..n-1, keeping pair i only if keep == NULL or keep[i] != 0.
 * out_R9 column-major (glm::mat3), out_t3 = centroid_tgt - R * centroid_src.  pairs_used may be NULL. */
int mi_kabsch(mi_ctx* ctx, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx,
              const unsigned char* keep, float out_R9[9], float out_t3[3], int* pairs_used);

/* CUDACommon::TransformCloud + GetMeanSquaredError (cudacommon.cu:132-148) / common.cpp:219-224, :259-268:
 * out[i] = R*src[i] + t (glm operation order, no contraction); *mse = sum_i |tgt[idx[i]] - out[i]|^2 / denom over the
 * kept pairs, denom = number of kept pairs if divide_by_pairs else m.  out_xyz, idx, mse may be NULL. */
int mi_transform_mse(mi_ctx* ctx, const float* src_xyz, int n, const float R9[9], const float t3[3],
                     const float* tgt_xyz, int m, const int* idx, const unsigned char* keep, int divide_by_pairs,
                     float* out_xyz, float* mse);

/* ----------------------------------------------------------------------------------------------------------------
 * Rigid CPD, "approximation-type" none (exact Gaussian P), full or hybrid -- replaces GetCudaCpdTransformationMatrix
 * (source/cuda-slam/cpdcuda.cuh:5-17, cpdcuda.cu:302-386); oracle CoherentPointDrift::GetRigidCPDTransformationMatrix
 * (source/cpu-slam/coherentpointdrift.cpp:69-124).  CPD naming follows the reference: M = |before| (index k),
 * N = |after| (index x).
 * -------------------------------------------------------------------------------------------------------------- */
typedef struct {
    float eps;             /* "convergence-epsilon": loop runs while sigma^2 > eps      (coherentpointdrift.cpp:106) */
    float weight;          /* "cpd-weight" (default .3), clamped to [1e-6, 1-1e-6]      (:93-96) */
    int   const_scale;     /* "cpd-const-scale" (parser default false, configparser.cpp:240) */
    int   max_iterations;  /* loop runs while iterations < max_iterations; NB -1 therefore runs NO iteration (:106) */
    float tolerance;       /* "cpd-tolerance" (default 1e-3) */
    float sigma2_init;     /* > 0: use this initial sigma^2.  <= 0: computed on the device as the exact
                              sum_ij |b_i - a_j|^2 / (3MN) in fp64, or as sigma2_mode says.  cpu-slam's own value is a single
                              sequential fp32 running sum (coherentpointdrift.cpp:126-139) that saturates for M*N >~ 1e7
                              (3.604 instead of 12.943 on the bunny clouds): MI_SIGMA2_CPU_SEQUENTIAL reproduces it. */
    int   sync_every;      /* as in mi_icp_params */
    int   verbose;
    int   approximation;   /* MI_CPD_APPROX_*: "approximation-type" (configparser.cpp:221-230).  0 = the exact Gaussian P. */
    float fgt_ratio_of_far_field;    /* "fgt-ratio-of-far-field" e (default 10): cells farther than sqrt(e)*sigma are skipped */
    int   fgt_order_of_truncation;   /* "fgt-order-of-truncation" p (default 8): monomials of total degree < p, 1..16 */
    int   sigma2_mode;               /* MI_SIGMA2_*: how the initial sigma^2 is computed when sigma2_init <= 0 */
    int   estep_mode;                /* MI_ESTEP_*: the order the exact E-step's sums are added in (round 6; took one of the reserved words: same size) */
    int   reserved[3];
} mi_cpd_params;

/* The exact E-step's summation order.
 *   DEFAULT:        chunked partial sums over the whole chip (K7a / K7b).
 *   CPU_SEQUENTIAL: cpu-slam's own order -- each fixed point's affinities added one by one into one fp32 running sum, each moving point's P1 / PX one
 *                   fixed point at a time, value = p / denominator (coherentpointdrift.cpp:186-213).  A parity mode, ~5 x the default's time: cpu-slam's
 *                   running sums drop small terms whole, a one-sided error of ~2.5e-5 of sigma^2 per EM iteration that the default does not make and that
 *                   `cpd-const-scale: true` amplifies; with this mode the device retraces the CPU restatement through it.  Single-GPU contexts, exact P only. */
enum { MI_ESTEP_DEFAULT = 0, MI_ESTEP_CPU_SEQUENTIAL = 1 };

/* The initial sigma^2 = sum_ij |b_i - a_j|^2 / (3MN) (CalculateSigmaSquared, coherentpointdrift.cpp:126-139 / cpdcuda.cu:65-78).
 *   EXACT:          closed form from the clouds' sums, fp64 (what cuda-slam's thrust reduction approximates).
 *   CPU_SEQUENTIAL: cpu-slam's own arithmetic bit for bit -- ONE sequential fp32 running sum over all M*N squared distances, which
 *                   saturates once it dwarfs its terms (3.604 instead of 12.943 on the bunny clouds).  cpu-slam's whole EM
 *                   trajectory starts from that number, so this is the mode in which mi_cpd_register retraces cpu-slam without
 *                   being handed a constant.  A sequential sum cannot be re-associated, but inside one binade of the running sum
 *                   it IS an integer prefix sum of rne(term / ulp): computed binade by binade over the whole GPU, the blocks
 *                   at binade crossings and exact rounding ties term by term (cpd_kernels.hip) -- 3 ms for the bunny clouds'
 *                   2.2e8 pairs (round 2's one-wave retrace: 750 ms), once per registration; single-GPU contexts only. */
enum { MI_SIGMA2_EXACT = 0, MI_SIGMA2_CPU_SEQUENTIAL = 1 };

/* "approximation-type" of the reference (common/enumerators.h:18-23, coherentpointdrift.cpp:141-167):
 *   FULL    every E-step is the Fast Gauss Transform (common/fgt.cpp) and sigma^2 is clamped to >= 0.05;
 *   HYBRID  the FGT E-step while sigma^2 > 0.015 * sigma^2_init, then the exact P truncated below 1e-3 (the parser's default).
 * The reference runs the FGT on the CPU in both of its builds; here it runs on the device (K9).  With either
 * mode the loop is host-stepped (the cell count and the switch depend on sigma^2), one state read-back per iteration. */
enum { MI_CPD_APPROX_NONE = 0, MI_CPD_APPROX_FULL = 1, MI_CPD_APPROX_HYBRID = 2 };

void mi_cpd_params_default(mi_cpd_params* p);

/* out_sR_t: column-major 4x4 holding scale*R (cpdcuda.cu:360) and t; out_scale may be NULL.
 * On a multi-GPU context (mi_ctx_create_dist) every rank passes both clouds whole and keeps fixed points mi_shard_range(n_after);
 * one all-reduce of 24 doubles per EM iteration merges the M-step moments, every rank returns the same result.  The FGT modes
 * (approximation != MI_CPD_APPROX_NONE; hybrid is the reference parser's default, configparser.cpp:217) keep both clouds whole on every
 * rank -- they cluster whole clouds -- and split the E-step's QUERIES (round 6): the fixed points the first transform is evaluated at, the
 * moving points of the second, the truncated E-step's tiles; the per-point weights travel through an unsigned-minimum all-reduce (bit for
 * bit), the M-step's sums through the 24-double one: the single-GPU run's iteration counts, s R|t within 1e-6 of it.
 * Synchronous: when it returns, the context's stream is drained (round 5; the host checks inside only peek at the state, so up to one
 * iteration's worth of no-op launches or a prelaunched K-centre replay trails the copy that said "done" -- it is waited for here). */
int mi_cpd_register(mi_ctx* ctx, const float* before_xyz, int m_before, const float* after_xyz, int n_after,
                    const mi_cpd_params* params, float out_sR_t[16], float* out_scale, int* iterations, float* error);

/* ----------------------------------------------------------------------------------------------------------------
 * Batched CPD: many small registrations under ONE set of rules in one call (single-GPU contexts only).
 * An exact EM iteration of a cloud of a thousand points is six launches none of which fills more than a fraction of the device; here
 * every problem gets a workgroup of its own and its EM iterations run inside one kernel, a few hundred problems side by side.  A
 * caller with ONE pair keeps calling mi_cpd_register: a single workgroup is slower than the whole device.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct {
    int problems_batched;    /* problems that ran on the batched kernel */
    int problems_fallback;   /* problems that ran through mi_cpd_register's path inside this call */
    int launches;            /* launches of the batched kernel */
    int reserved[5];
} mi_cpd_batch_info;

/* 1 if a problem of these sizes under these rules is carried by the batched kernel, 0 if the call routes it through the existing
 * path.  Pure host function of its arguments (no context, no device).  Routed: 1 <= m_before <= 2048 and 1 <= n_after <= 2048
 * under approximation == MI_CPD_APPROX_NONE, estep_mode == MI_ESTEP_DEFAULT, sigma2_mode == MI_SIGMA2_EXACT (or sigma2_init > 0,
 * which leaves the mode nothing to compute) and verbose == 0 -- a function of the two sizes and those fields only, monotone in the
 * sizes.  The FGT / hybrid E-steps are host-stepped and cluster whole clouds, the two CPU-sequential parity modes and the
 * per-iteration print belong to the single path.  The edge was set by measurement (DESIGN.md section 4, K-batch CPD): at 64
 * problems the batched call beats the loop of single calls 2.2 x at 2048 x 2048 and loses (0.8 x) at 4096 x 4096; sizes in between
 * were not measured and are not routed.  Routed does not mean faster for every batch: one problem alone is slower batched at every
 * size, and near the edge a batch needs several dozen problems to pay off (2048 points: 0.57 x at 16 problems, 2.2 x at 64; 1024
 * points: 1.8 x at 16) -- the table in DESIGN.md has every measured (problems, size).
 * Developer switch: a context created under MISLAM_CPD_MFMA=0 (the single path's contraction on the vector pipe: other roundings
 * than the matrix-pipe chain the batched kernel is built on) sends every problem of a batched call through the existing path,
 * whatever this function says; MISLAM_SVD_IEEE=1 is followed by the batched kernel. */
int mi_cpd_batch_route(int m_before, int n_after, const mi_cpd_params* params);

/* B independent registrations.  Problem k moves the points before_xyz[3*before_range[2k] ...] (before_range[2k+1] of them) onto
 * after_xyz[3*after_range[2k] ...] (after_range[2k+1] of them); both arrays must reach as far as the ranges say.  Ranges may
 * overlap or coincide.  out_sR_t: 16*B floats (column-major 4x4 each: scale*R and t, as mi_cpd_register writes them); out_scale,
 * iterations, error, stop_reason: B entries each; out_scale and info may be NULL, the others not.  Problem k's out_sR_t, out_scale,
 * iterations and error are, BIT FOR BIT, what
 *   mi_cpd_register(ctx, before_k, m_k, after_k, n_k, params, ...)
 * returns on the same context -- whatever else is in the batch and in whatever position; sync_every is accepted and, as in the
 * single call, moves no bit.  stop_reason[k] is the MI_STOP_* of the problem's state block (MI_STOP_MAX_ITERATIONS, MI_STOP_TOLERANCE
 * or MI_STOP_SIGMA, tested in that order after every iteration), which the single call does not return.  Every problem
 * mi_cpd_register accepts is accepted: the ones mi_cpd_batch_route does not route run through the existing path inside the call,
 * one after the other.  n_problems == 0 is MI_OK.  A range with a negative offset or a count < 1, a NULL output, or parameters
 * mi_cpd_register would refuse: MI_ERR_INVALID_ARG, mi_last_error names the problem, nothing has touched the device.  A
 * distributed context: MI_ERR_STATE.  Afterwards no ICP problem is loaded (as after mi_cpd_register).  Every launch of the kernel
 * ends: it carries a bounded number of EM iterations. */
int mi_cpd_register_batch(mi_ctx* ctx, int n_problems,
                          const float* before_xyz, const int* before_range,
                          const float* after_xyz,  const int* after_range,
                          const mi_cpd_params* params,
                          float* out_sR_t, float* out_scale, int* iterations, float* error, int* stop_reason,
                          mi_cpd_batch_info* info);

/* CalculateSigmaSquared (cpdcuda.cu:65-78 / coherentpointdrift.cpp:126-139): the exact value, or with an explicit MI_SIGMA2_* mode. */
int mi_cpd_sigma_squared(mi_ctx* ctx, const float* before_xyz, int m, const float* after_xyz, int n, float* sigma2);
int mi_cpd_sigma_squared_mode(mi_ctx* ctx, const float* before_xyz, int m, const float* after_xyz, int n, int sigma2_mode, float* sigma2);

/* ComputePMatrix, no truncation (cpdcuda.cu:80-116 / coherentpointdrift.cpp:168-221):
 * p_xk = exp(-|x - y_k|^2 / (2 sigma^2)); den_x = sum_k p_xk + c; Pt1[x] = 1 - c/den_x; P1[k] = sum_x p_xk/den_x;
 * PX[k] = sum_x x * p_xk/den_x (row-major M x 3); *L = -sum_x log den_x + 1.5*N*log sigma^2. */
int mi_cpd_estep(mi_ctx* ctx, const float* y_xyz, int m, const float* x_xyz, int n, float constant, float sigma2,
                 float* p1, float* pt1, float* px, float* L);

/* ComputePMatrix with doTruncate (coherentpointdrift.cpp:168-221; the hybrid mode calls it with truncate = 1e-3, :166):
 * affinities with -|x - y_k|^2 / (2 sigma^2) < log(truncate) count as 0. */
int mi_cpd_estep_truncated(mi_ctx* ctx, const float* y_xyz, int m, const float* x_xyz, int n, float constant, float sigma2,
                           float truncate, float* p1, float* pt1, float* px, float* L);

/* ComputePMatrixWithFGT (common/cpdutils.cpp:19-77): the same four products through three Fast Gauss Transforms with
 * K = round(min(N, M, 50 + sigma2_init/sigma2)) cells, bandwidth sqrt(2 sigma2) and the outlier term taken at the CURRENT
 * sigma2.  Needs m, n >= 2 (the clustering starts from point 1, fgt.cpp:162). */
int mi_cpd_estep_fgt(mi_ctx* ctx, const float* y_xyz, int m, const float* x_xyz, int n, float weight, float sigma2,
                     float sigma2_init, float ratio_of_far_field, int order_of_truncation,
                     float* p1, float* pt1, float* px, float* L);

/* KCenter (common/fgt.cpp:152-212): greedy farthest-point clustering from point 1; cluster[i] in [0, K), centers_xyz[K][3] the
 * cell means.  Labels are bit-identical to the reference's (same arithmetic, same tie rules).  n >= 2, 1 <= K <= 65535. */
int mi_fgt_kcenter(mi_ctx* ctx, const float* cloud_xyz, int n, int K, float* centers_xyz, int* cluster);

/* The same clustering with a GUESS of the sweep's choices: guess[0 .. n_guess) = the points expected as centres 0, 1, ... (what an
 * earlier sweep of the same cloud under another similarity transform chose -- how rigid CPD's E-steps cluster the moving cloud: the
 * guess is replayed and checked for all points in parallel, and only what it does not cover, or gets wrong, is swept step by step).
 * The result is mi_fgt_kcenter's, bit for bit, whatever the guess.  picked[K] (may be NULL) receives the sweep's choices, *verified
 * (may be NULL) the number of leading entries of the guess that were the sweep's own (-1: no replay ran, n_guess < 2). */
int mi_fgt_kcenter_guided(mi_ctx* ctx, const float* cloud_xyz, int n, int K, const int* guess, int n_guess, float* centers_xyz,
                          int* cluster, int* picked, int* verified);

/* Host-only (no device needed): the monomial tables of truncation order p the FGT kernels use, pd = C(p+2,3) entries each in
 * the reference's graded monomial order (fgt.cpp:124-137): exponents packed a | b<<8 | c<<16, the constants 2^|alpha|/alpha!
 * of ComputeC_k (fgt.cpp:214-244), and each monomial's slot in the Horner traversal.  Any output may be NULL. */
int mi_fgt_tables(int order_of_truncation, unsigned int* mono, float* ck, int* horner_slot, int* pd);

/* MStep (cpdcuda.cu:172-300 / coherentpointdrift.cpp:223-277).  scale, sigma2 are in/out as in the reference. */
int mi_cpd_mstep(mi_ctx* ctx, const float* before_xyz, int m, const float* after_xyz, int n, const float* p1,
                 const float* pt1, const float* px, int const_scale, float out_R9[9], float out_t3[3], float* scale,
                 float* sigma2);

/* ----------------------------------------------------------------------------------------------------------------
 * Non-iterative registration, "method": "nicp" -- replaces GetCudaNicpTransformationMatrix (source/cuda-slam/nicpcuda.cuh:5-15,
 * nicpcuda.cu:70-184); oracle NonIterative::GetNonIterativeTransformationMatrix with the sequential policy
 * (source/cpu-slam/noniterative.cpp:204-282; the parallel policy races on the shared random generator, :84-101).
 * Each repetition aligns the principal axes of the two clouds, U_after * U_before^T, with the column signs an Eigen::JacobiSVD
 * of the randomly permuted 3 x N matrices would produce (they depend on the first three points only -- nicp_api.hip), and
 * the candidate with the smallest error wins:
 *   MI_CPD_APPROX_NONE    every candidate is scored on the comparison subcloud (exact nearest neighbours), early exit at eps;
 *   MI_CPD_APPROX_FULL    candidates ranked by the index-wise "approximated" error, the best one scored on the subcloud;
 *   MI_CPD_APPROX_HYBRID  the best five are scored on the subcloud (the parser's default).
 * The random choices stay with the caller, who draws them like the reference (std::mt19937 + std::shuffle,
 * GetRandomPermutationVector, common.cpp:554-560): order_heads[3*r .. 3*r+2] are the first three entries of repetition r's
 * permutation of 0..min(m,n)-1 (max_repetitions of them; -1 means 20), subcloud_idx the first subcloud_n entries of the
 * permutation GetSubcloud draws BEFORE them (common.cpp:25-37), or NULL with subcloud_n = m_before for the whole cloud.
 * -------------------------------------------------------------------------------------------------------------- */
typedef struct {
    float eps;              /* "convergence-epsilon" */
    int   max_repetitions;  /* "nicp-iterations" (default 32); -1 = 20 (noniterative.cpp:207-208) */
    int   approximation;    /* MI_CPD_APPROX_* ("approximation-type") */
    int   verbose;
    int   reserved[4];
} mi_nicp_params;

void mi_nicp_params_default(mi_nicp_params* p);

/* out_T: column-major 4x4 (R | t).  *repetitions and *error as the reference leaves them.
 * A candidate's error is the mean over the subcloud points whose nearest squared distance is below 1e6 (maxDistanceForComparison).  When NO point
 * of any scored candidate is that close, every error is 0 / 0 and compares false, and the reference returns an uninitialised pair; here the call
 * returns MI_OK with out_T = the first candidate that was scored (repetition 0 in MI_CPD_APPROX_NONE, the head of the ranked list otherwise: a rigid
 * transform like every candidate), *error = FLT_MAX and *repetitions = max_repetitions. */
int mi_nicp_register(mi_ctx* ctx, const float* before_xyz, int m_before, const float* after_xyz, int n_after,
                     const mi_nicp_params* params, const int* order_heads, const int* subcloud_idx, int subcloud_n,
                     float out_T[16], int* repetitions, float* error);

/* ----------------------------------------------------------------------------------------------------------------
 * Input stage: what Common::GetCloudsFromConfig (source/common/common.cpp:134-210) does to ONE cloud between
 * LoadCloud and the registration call, on the device and with the reference's arithmetic bit for bit:
 *   GetSubcloud (common.cpp:25-37) -> NormalizeCloud to "cloud-spread" (:81-95; the centre of mass is the reference's
 *   sequential fp32 accumulate, :281-284) -> std::shuffle (:166-167) -> AddNoiseToCloud (:97-119) -> AddOutliersToCloud
 *   (:121-132) -> GetTransformedCloud (:219-224, the `after` cloud only).
 * The random outcomes are the caller's, drawn like the reference draws them (mt19937 + std::shuffle for the index vectors,
 * rand() for the unit draws; host/cloud_io.cpp does it):
 *   subcloud_idx   first subcloud_n entries of GetSubcloud's permutation of 0..n_raw-1, or NULL (whole cloud);
 *   shuffle_idx    the shuffle as a gather order -- std::shuffle of an iota of the cloud's size with the same generator:
 *                  prepared row i = normalised row shuffle_idx[i] -- or NULL;
 *   noise_rows     ascending rows of the shuffled cloud that AddNoiseToCloud's flag permutation marks, noise_unit[3q..3q+2]
 *                  the three rand()/RAND_MAX draws of the q-th of them (x, y, z), in the order the reference consumes them;
 *   outlier_unit   three draws per appended outlier.
 * out_xyz holds (cloud size + n_outliers) points; *out_n receives that count.
 * -------------------------------------------------------------------------------------------------------------- */
typedef struct {
    int   has_spread;       /* "cloud-spread" present: normalise to `spread` */
    float spread;
    float noise_intensity;  /* "noise-intensity-before" / "-after" */
    int   has_transform;    /* apply rotation (column-major, like glm::mat3) and translation: p -> R p + t */
    float rotation[9];
    float translation[3];
    int   reserved[4];
} mi_prepare_params;

void mi_prepare_params_default(mi_prepare_params* p);

int mi_prepare_cloud(mi_ctx* ctx, const float* raw_xyz, int n_raw, const int* subcloud_idx, int subcloud_n, const int* shuffle_idx,
                     const int* noise_rows, const float* noise_unit, int n_noise, const float* outlier_unit, int n_outliers,
                     const mi_prepare_params* params, float* out_xyz, int* out_n);

/* ----------------------------------------------------------------------------------------------------------------
 * Voxel-grid downsampling (no reference counterpart: the reference thins a cloud with the random GetSubcloud only): one output
 * point per occupied voxel of a cubic lattice, the mean of the voxel's points -- what a pipeline runs on a raw scan or a map tile
 * before it registers it (downsample, then mi_icp_register_batch).  Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */

/* Pure host function (no context, no device): the voxel a point falls in.
 * out[a] = (int)floorf((p[a] - origin[a]) / voxel_size), a = x,y,z.
 * Arithmetic: one IEEE fp32 subtraction and one IEEE fp32 division, each rounded to nearest.  No reciprocal, no contraction.  The
 * kernels use the same arithmetic, bit for bit.
 * Returns MI_ERR_INVALID_ARG for voxel_size <= 0 or non-finite, a non-finite operand, or a quotient outside [-2^30, 2^30); out is
 * then left as it was. */
int mi_voxel_index(const float p[3], const float origin[3], float voxel_size, int out[3]);

/* Voxel-grid centroids of the n points of xyz, computed on the device.
 *   Voxel of a point: mi_voxel_index with the given origin.  With origin3 == NULL the origin is the exact per-axis minimum of the
 *     cloud, so every coordinate is >= 0; an explicit origin lets a scan and a map share one lattice, and coordinates may then be
 *     negative.  Only the per-axis EXTENT (max - min + 1 over the occupied voxels) is limited, to <= 2^20.
 *   Output order: one row per occupied voxel, ascending by (cz, cy, cx) as signed integers -- deterministic, and independent of the
 *     order of the input points.
 *   Output point: per coordinate, the fp64 sum of the voxel's points, divided in fp64 by their count, rounded once to fp32.  The
 *     order of the sum is fixed by the implementation (a function of the sorted order): the same input gives the same bits on every
 *     call, whatever ran on the context before.  There is no floating-point atomic anywhere on the path.
 *   out_xyz (capacity n points) and *out_n receive the rows and their number.  Optional, each may be NULL: out_count (capacity n)
 *     the points per voxel, summing to n; out_coord (capacity 3n) the voxel coordinate of each row; voxel_of_point (n entries) the
 *     row whose out_coord equals the voxel of point i.
 *   MI_ERR_INVALID_ARG -- mi_last_error names the cause and, for a bad point, its index; NO output array has been written -- for
 *     n < 1; voxel_size non-finite or <= 0; a NULL xyz, out_xyz or out_n; a non-finite origin; a non-finite input coordinate; a
 *     voxel coordinate outside [-2^30, 2^30); an axis extent above 2^20.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call: it works in buffers of its own in the context.
 *   Synchronous, like the other host-in / host-out entry points. */
int mi_voxel_downsample(mi_ctx* ctx, const float* xyz, int n, float voxel_size,
                        const float* origin3,     /* NULL: per-axis minimum of the cloud */
                        float* out_xyz,           /* capacity n points */
                        int* out_n,
                        int* out_count,           /* may be NULL; capacity n: points per voxel */
                        int* out_coord,           /* may be NULL; capacity 3n: voxel coordinate of each output row */
                        int* voxel_of_point);     /* may be NULL; n entries: output row of input point i */

/* Where the last mi_voxel_downsample of this context spent its host wall time, in ms (measurement hook, tools/voxel_bench.py):
 *   out[0] workspace (device allocations)           out[1] upload + AoS -> SoA
 *   out[2] range pass and its read-back             out[3] keys + sort
 *   out[4] head flags, scan, segmented sums         out[5] row count read-back + download of the rows
 *   out[6] unused (0)                               out[7] the whole call
 * As with mi_icp_load_times, the parts are attributable only while profiling is enabled (the stream is then drained after every
 * stage); otherwise the device work of a stage is waited for in the next stage that reads something back. */
#define MI_VOXEL_STAGES 8
int mi_voxel_downsample_times(mi_ctx* ctx, double out_ms[MI_VOXEL_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * Exact k nearest neighbours (no reference counterpart: the reference searches the single nearest neighbour only): what the stages
 * between a downsample and a registration are built on -- normals, statistical and radius outlier removal, local descriptors,
 * point-to-plane weights (neighbourhoods).  Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */

/* The k nearest cloud points of every query, computed on the device.
 *   Order and arithmetic: for query i every cloud point j has the key (bits(d2) << 32) | j, d2 = |cloud[j] - query[i]|^2 evaluated
 *     in the dist_mode arithmetic on the fp32 differences (cloud[j] - query[i]) -- exactly the arithmetic of mi_nn_search:
 *     MI_DIST_CPU_ROUNDING (dx*dx + dy*dy) + dz*dz with every operation rounded, MI_DIST_FMA fma(dz, dz, fma(dy, dy, dx*dx)).  Row i
 *     of the result holds the k SMALLEST keys in ascending order: the smaller distance first, equal distance bits to the lower
 *     index.  For k = 1 and no limit this is mi_nn_search's answer bit for bit.
 *   Self mode, query_xyz == NULL: the queries are the cloud's own points (n must equal m) and candidate j == i is skipped for query
 *     i BY INDEX, not by distance -- a duplicate of point i stored elsewhere in the cloud is returned, at d2 = +0.
 *   max_distance_squared: INFINITY for no limit; otherwise a candidate with d2 > max_distance_squared does not exist for the query.
 *   Missing slots: a query with fewer than k candidates (m < k, m - 1 < k in self mode, or the limit) has its remaining slots set
 *     to idx = -1, d2 = +INFINITY; count[i] is the number of filled slots (<= k).
 *   idx (n*k) receives idx[i*k + r] = the r-th neighbour of query i; d2 (n*k, may be NULL) its distance; count (n, may be NULL).
 *   Exact for every query position, far outside the cloud's bounding box included, and for every cloud shape (all points identical,
 *     collinear, coplanar, a far outlier, m = 1); the speed is only claimed for queries in or near the cloud.  Deterministic: the
 *     same input gives the same bits on every call, whatever ran on the context before.
 *   MI_ERR_INVALID_ARG -- mi_last_error names the cause and, for a bad point, which array and which index; NO output array has been
 *     written -- for a NULL ctx, cloud_xyz or idx; n < 1 or m < 1; k outside [1, MI_KNN_MAX_K]; a dist_mode other than the two
 *     above; max_distance_squared NaN or negative; self mode with n != m; a non-finite coordinate in either array; a coordinate of
 *     magnitude above 1e18 (which keeps every d2 finite: 3 (2e18)^2 < FLT_MAX).
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call: it works in buffers of its own in the context.
 *   Synchronous, host in and host out. */
#define MI_KNN_MAX_K 32
int mi_knn_search(mi_ctx* ctx,
                  const float* query_xyz, int n,   /* NULL: the queries are the cloud's own points (n must equal m); neighbour j == i is skipped */
                  const float* cloud_xyz, int m,
                  int k, int dist_mode,            /* 1 <= k <= MI_KNN_MAX_K; MI_DIST_CPU_ROUNDING or MI_DIST_FMA */
                  float max_distance_squared,      /* INFINITY: no limit; else candidates with d2 > this do not exist for the query */
                  int* idx,                        /* n*k: idx[i*k + r] = r-th neighbour of query i */
                  float* d2,                       /* may be NULL; n*k */
                  int* count);                     /* may be NULL; n: neighbours found for query i (<= k) */

/* Where the last mi_knn_search of this context spent its host wall time, in ms (measurement hook, tools/knn_bench.py):
 *   out[0] workspace (device allocations)           out[1] upload + AoS -> SoA (cloud, queries)
 *   out[2] input check, bounding box, its read-back out[3] cell grid over the cloud
 *   out[4] curve order of the queries + permute     out[5] the search kernel
 *   out[6] download of the results                  out[7] the whole call
 * As with mi_voxel_downsample_times, the parts are attributable only while profiling is enabled (the stream is then drained after
 * every stage, and out[5] is the search launch's own HIP-event time instead of host wall time). */
#define MI_KNN_STAGES 8
int mi_knn_search_times(mi_ctx* ctx, double out_ms[MI_KNN_STAGES]);

/* Every cloud point within a radius of every query, as CSR lists, computed on the device (Open3D's search_radius_vector_3d, PCL's
 * radiusSearch): what mi_knn_search cannot give once a ball holds more than MI_KNN_MAX_K points, and what mi_remove_outliers counts but
 * does not name (neighbourhoods).
 *   Membership: r2 = radius * radius, one IEEE fp32 multiplication (mi_remove_outliers' radius method forms the same number).  Candidate j
 *     belongs to row i if and only if d2(i, j) <= r2, d2 in the dist_mode arithmetic of mi_knn_search on the fp32 differences; a point
 *     exactly AT r2 belongs.  Self mode, query_xyz == NULL: the queries are the cloud's own points (n must equal m) and candidate j == i is
 *     skipped BY INDEX -- a duplicate of point i stored elsewhere belongs, at d2 = +0 -- so a row's length is mi_remove_outliers'
 *     neighbours[i] at the same radius and dist_mode, bit for bit.
 *   Layout: row i is entries [offsets[i], offsets[i + 1]) of idx and d2; offsets[0] = 0, offsets[n] = *total.  An empty row repeats its
 *     offset.  The offsets are 64-bit: a counts-only call has no limit on *total.
 *   Order: sorted = 1: every row ascends by the key (bits(d2) << 32) | j, the smaller distance first, equal distance bits to the lower
 *     index -- for any k <= MI_KNN_MAX_K the first min(k, length) entries of row i are row i of mi_knn_search(ctx, query_xyz, n, cloud_xyz,
 *     m, k, dist_mode, r2, ...), index and distance bits alike.  sorted = 0: the same set in an order that is not specified; the same
 *     input still gives the same bits on every call, whatever ran on the context before.
 *   Two modes, and the capacity protocol (in the manner of snprintf):
 *     idx == NULL  counts only: capacity must be 0, d2 must be NULL; offsets and *total are written and no list is built.
 *     idx != NULL  0 < capacity <= MI_RADIUS_MAX_TOTAL entries of idx (and of d2, unless NULL).  offsets and *total are ALWAYS written.
 *                  idx and d2 are written if and only if *total <= capacity, entries [0, *total) of them and nothing behind; otherwise
 *                  they are left untouched, no device memory is taken for the lists, and the call STILL returns MI_OK: the caller
 *                  compares *total with capacity and, if it was short, calls again with arrays of *total entries.
 *   Cost: two walks of every query's ball (one counts, one writes), each proportional to the points in the ball AND in the cells it
 *     touches; with lists, 16 bytes of device memory per entry; with sorted = 1 a rank per row that is quadratic in the row's length
 *     up to 64 entries and L log^2 L beyond.  A radius that holds much of the cloud makes the whole call quadratic in the cloud: this is
 *     a search of small balls.  Exact for every query position and cloud shape, as mi_knn_search is.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with "mi_radius_search" and names the cause and, for a bad point, which array and which
 *     index; NOTHING has been written -- for a NULL ctx, cloud_xyz, offsets or total; n < 1 or m < 1; self mode with n != m; a dist_mode
 *     other than the two of mi_knn_search; sorted outside {0, 1}; radius NaN, infinite or <= 0, or radius * radius not finite; d2 given
 *     without idx; idx == NULL with capacity != 0; idx != NULL with capacity outside [1, MI_RADIUS_MAX_TOTAL]; a non-finite coordinate
 *     in either array, or one of magnitude above 1e18.
 *   MI_ERR_STATE on a distributed context.  A device allocation that fails (the lists': 16 bytes per entry) is MI_ERR_HIP; the context
 *     stays usable, and the output arrays' contents are then unspecified.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the other searches keep: it works in buffers of its own.
 *   Synchronous, host in and host out. */
#define MI_RADIUS_MAX_TOTAL (1LL << 31)
int mi_radius_search(mi_ctx* ctx,
                     const float* query_xyz, int n,   /* NULL: the queries are the cloud's own points (n must equal m); neighbour j == i is skipped by index */
                     const float* cloud_xyz, int m,
                     float radius, int dist_mode,     /* finite, > 0; MI_DIST_CPU_ROUNDING or MI_DIST_FMA */
                     int sorted,                      /* 1: every row ascending by key; 0: order unspecified but the same on every call */
                     long long* offsets,              /* n + 1: row i is [offsets[i], offsets[i + 1]); offsets[0] = 0, offsets[n] = *total */
                     int* idx, float* d2,             /* capacity entries each; d2 may be NULL; idx NULL: counts only */
                     long long capacity,              /* 0 with idx NULL; else 1 .. MI_RADIUS_MAX_TOTAL */
                     long long* total);               /* the members of all rows, whether the lists were written or not */

/* Where the last mi_radius_search of this context spent its host wall time, in ms (measurement hook, tools/radius_bench.py):
 *   out[0] workspace (device allocations, the lists' included)   out[1] upload, input check, cell grid, curve order (unsorted: + the cells' order)
 *   out[2] the count kernel                                      out[3] the scan and the read-back of the total
 *   out[4] the fill kernel (unsorted: the cells' order in out[1]) out[5] the sort kernel (0 with sorted = 0)
 *   out[6] unpack + download of the results                      out[7] the whole call
 * As with mi_knn_search_times, the parts are attributable only while profiling is enabled (the stream is then drained after every
 * stage, and out[2], out[4] and out[5] are the launches' own HIP-event times instead of host wall time). */
#define MI_RADIUS_STAGES 8
int mi_radius_search_times(mi_ctx* ctx, double out_ms[MI_RADIUS_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * Surface normals and curvature (no reference counterpart: the reference has no normals anywhere): the first consumer of the k-NN
 * lists, which here never leave the device (normals).  Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */

/* Normal, curvature and neighbour count of every point of a cloud, computed on the device.
 *   Neighbourhood of point i: point i itself plus the neighbours that
 *     mi_knn_search(ctx, NULL, n, cloud_xyz, n, k, dist_mode, max_distance_squared, ...) returns for row i -- the same set, bit for
 *     bit: self mode skips by index, and a duplicate of point i stored elsewhere is a neighbour.  count[i] is that call's count[i].
 *     A finite max_distance_squared makes it the "hybrid" k-and-radius neighbourhood; INFINITY is no limit.
 *   Covariance: that of the neighbourhood's count + 1 points about their mean, divided by the number of points, in fp64.  It is formed
 *     in one pass from the differences d = p_j - p_i, taken in fp64 (exact, or rounded at 2^-53): with c = count + 1, m = sum d / c and
 *     C = sum d d^T / c - m m^T; the point itself contributes d = 0.  Every magnitude is bounded by the neighbourhood's radius, not by
 *     the cloud's offset from the origin, so the one pass agrees with the two-pass form to a few 2^-53 of the trace.
 *   Normal: the unit eigenvector of C's smallest eigenvalue from an fp64 cyclic Jacobi iteration, normalised in fp64, rounded once to
 *     fp32.  With viewpoint3 it is flipped so that n . (v - p_i) >= 0, the sign test done in fp64 on the unrounded vector.  Without
 *     viewpoint3 the sign is unspecified but deterministic: the same input gives the same bits on every call, whatever ran on the
 *     context before.
 *   Curvature: lambda0 / (lambda0 + lambda1 + lambda2), lambda0 the smallest eigenvalue clamped below at 0; 0 when the trace is 0.
 *   Too few points: with count[i] < 2 (fewer than three points) the normal is (0, 0, 0) and the curvature 0; count[i] tells the caller.
 *   Degenerate neighbourhoods (collinear, all points identical): the normal is finite and of unit length, or exactly zero under the
 *     rule above; nothing else is promised for them.
 *   normals_xyz (n*3, AoS like the clouds) receives the normals; curvature (n, may be NULL) and count (n, may be NULL; the neighbours
 *     used, the point itself not counted) what their names say.
 *   MI_ERR_INVALID_ARG -- mi_last_error names the cause and, for a bad point, its index; NO output array has been written -- for a
 *     NULL ctx, cloud_xyz or normals_xyz; n < 1; k outside [2, MI_KNN_MAX_K]; a dist_mode other than the two of mi_knn_search;
 *     max_distance_squared NaN or negative; a non-finite viewpoint; a non-finite coordinate or one above 1e18 in magnitude.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything mi_knn_search keeps: it works in buffers of its own.
 *   Synchronous, host in and host out. */
int mi_estimate_normals(mi_ctx* ctx,
                        const float* cloud_xyz, int n,
                        int k, int dist_mode,            /* 2 <= k <= MI_KNN_MAX_K; MI_DIST_CPU_ROUNDING or MI_DIST_FMA */
                        float max_distance_squared,      /* INFINITY: no limit; else neighbours with d2 > this do not exist */
                        const float* viewpoint3,         /* may be NULL; else normals are turned towards this point */
                        float* normals_xyz,              /* n*3 */
                        float* curvature,                /* may be NULL; n */
                        int* count);                     /* may be NULL; n: neighbours used for point i (<= k) */

/* Where the last mi_estimate_normals of this context spent its host wall time, in ms (measurement hook, tools/normals_bench.py).  The
 * stages are those of mi_knn_search_times:
 *   out[0] workspace (device allocations)           out[1] upload + AoS -> SoA
 *   out[2] input check, bounding box, its read-back out[3] cell grid over the cloud
 *   out[4] curve order of the cloud + permute       out[5] the fused search-and-solve kernel
 *   out[6] download of the results                  out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage, and out[5] is the
 * launch's own HIP-event time instead of host wall time). */
#define MI_NORMALS_STAGES 8
int mi_estimate_normals_times(mi_ctx* ctx, double out_ms[MI_NORMALS_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * Statistical and radius outlier removal (no reference counterpart): the second consumer of the k-NN search, whose lists never leave
 * the device here either (outlier removal).  Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */
#define MI_OUTLIER_STATISTICAL 0
#define MI_OUTLIER_RADIUS      1
typedef struct {
    int   method;          /* MI_OUTLIER_* */
    int   dist_mode;       /* MI_DIST_CPU_ROUNDING or MI_DIST_FMA: the d2 arithmetic of mi_knn_search */
    int   k;               /* statistical: neighbours per point, 1 .. MI_KNN_MAX_K */
    float std_ratio;       /* statistical: finite, >= 0 */
    float radius;          /* radius: finite, > 0 */
    int   min_neighbours;  /* radius: >= 1 */
    int   reserved[6];
} mi_outlier_params;
void mi_outlier_params_default(mi_outlier_params* p);   /* statistical, k = 16, std_ratio = 2, CPU rounding (radius = 0, min_neighbours = 1: set both for the radius method) */

typedef struct { double mean, stddev, threshold; long long kept; int reserved[4]; } mi_outlier_stats;

/* The points of a cloud that pass one of the two usual outlier filters, computed on the device.
 *   Statistical (MI_OUTLIER_STATISTICAL): the neighbours of point i are exactly row i of
 *     mi_knn_search(ctx, NULL, n, cloud_xyz, n, k, dist_mode, INFINITY, ...) -- self is skipped by index, a duplicate of point i stored
 *     elsewhere is a neighbour at d2 = +0 -- and neighbours[i] is that call's count[i] (= min(k, n - 1)).  The point's score is
 *     mu_i = (sum over the row of sqrt((double)d2)) / count[i] in fp64, the roots added nearest first; mu_i = 0 when count[i] = 0.
 *     mean_distance[i] is mu_i rounded once to fp32.  The statistics are taken over the UNROUNDED mu_i: mean = sum mu_i / n,
 *     stddev = sqrt(sum (mu_i - mean)^2 / n) -- the population form, two passes, fp64, in a summation order that depends on n alone --
 *     and threshold = mean + (double)std_ratio * stddev.  Point i is kept iff mu_i <= threshold ("<=": a cloud of identical points
 *     keeps every point).
 *   Radius (MI_OUTLIER_RADIUS): r2 = radius * radius, one IEEE fp32 multiplication (it may underflow to +0: only duplicates count
 *     then).  neighbours[i] is the number of j != i (by index) with d2(i, j) <= r2 in the dist_mode arithmetic, and point i is kept iff
 *     that number >= min_neighbours.  min_neighbours may exceed n - 1: nothing is kept, *out_n = 0, MI_OK.  stats->mean, stddev and
 *     threshold are 0, 0 and (double)min_neighbours; mean_distance is not written.  With neighbours == NULL a point's count stops at
 *     min_neighbours; the mask is the same either way.  Cost: a point's work is proportional to the number of points inside its ball
 *     (and its cell's neighbourhood), so a radius that holds a large share of the cloud makes the call quadratic.
 *   Outputs: the kept points in ascending caller index -- out_xyz (capacity n points, may be NULL) their coordinates, the input's bits;
 *     out_index (capacity n, may be NULL) their indices; rows beyond *out_n are not written.  keep (n, may be NULL) is 1 for a kept point
 *     and 0 for a removed one.  *out_n == stats->kept == the number of ones in keep.
 *   Deterministic: the same input gives the same bits on every call, whatever ran on the context before.  No floating-point atomics.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with "mi_remove_outliers" and names the cause and, for a bad point, its index (the
 *     lowest); NO output has been written -- for a NULL ctx, cloud_xyz, params or out_n; n < 1; an unknown method or dist_mode;
 *     statistical: k outside [1, MI_KNN_MAX_K], std_ratio NaN, infinite or negative; radius: radius NaN, infinite or <= 0, radius^2 not
 *     finite, min_neighbours < 1; a non-finite coordinate or one above 1e18 in magnitude.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything mi_knn_search and mi_estimate_normals keep: it works in
 *     buffers of its own.
 *   Synchronous, host in and host out. */
int mi_remove_outliers(mi_ctx* ctx, const float* cloud_xyz, int n, const mi_outlier_params* params,
                       float* out_xyz,          /* may be NULL; capacity n points: the kept points, in the caller's order */
                       int* out_index,          /* may be NULL; capacity n: their indices, ascending */
                       int* out_n,              /* non-NULL */
                       unsigned char* keep,     /* may be NULL; n: 1 kept, 0 removed */
                       float* mean_distance,    /* may be NULL; n; statistical only (radius: not written) */
                       int* neighbours,         /* may be NULL; n */
                       mi_outlier_stats* stats);/* may be NULL */

/* Where the last mi_remove_outliers of this context spent its host wall time, in ms (measurement hook, tools/outlier_bench.py).  The
 * first six stages are those of mi_estimate_normals_times:
 *   out[0] workspace (device allocations)           out[1] upload + AoS -> SoA
 *   out[2] input check, bounding box, its read-back out[3] cell grid over the cloud
 *   out[4] curve order of the cloud + permute       out[5] the score (statistical) or count (radius) kernel
 *   out[6] statistics + flags + compaction + download   out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage, and out[5] is the
 * launch's own HIP-event time instead of host wall time). */
#define MI_OUTLIER_STAGES 8
int mi_remove_outliers_times(mi_ctx* ctx, double out_ms[MI_OUTLIER_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * ISS keypoints (Intrinsic Shape Signatures, Zhong 2009; no reference counterpart): the few per cent of a cloud's points whose
 * neighbourhood is distinctive, to be taken between mi_estimate_normals and mi_fpfh_features so that only their descriptors are
 * matched (keypoints).  Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */
typedef struct {
    float salient_radius;    /* finite, > 0, square finite: the ball the scatter matrix is taken over     default 0: the caller must set it */
    float non_max_radius;    /* finite, > 0, square finite: the ball of the non-maximum suppression       default 0: the caller must set it */
    float gamma_21;          /* finite, > 0                                                                default 0.975f */
    float gamma_32;          /* finite, > 0                                                                default 0.975f */
    int   min_neighbours;    /* >= 1: in BOTH balls                                                         default 5 */
    int   dist_mode;         /* MI_DIST_CPU_ROUNDING / MI_DIST_FMA, as mi_knn_search                        default CPU_ROUNDING */
    int   reserved[10];
} mi_iss_params;             /* 64 bytes */
void mi_iss_params_default(mi_iss_params* p);

/* The ISS keypoints of a cloud, computed on the device.  Every rule below can be retraced in numpy (tests/iss_reference.py does).
 *   Radii: r2s = salient_radius * salient_radius and r2n = non_max_radius * non_max_radius, one IEEE fp32 multiplication each.  The two
 *     radii are independent: either may be the larger.
 *   Salient neighbourhood of point i: { j != i (by index) : d2(i, j) <= r2s } in the dist_mode arithmetic of mi_knn_search.
 *     neighbours[i] is its size: exactly the count mi_remove_outliers gives in radius mode at the same radius with its neighbours
 *     output.  A point AT the radius belongs; a duplicate of point i stored elsewhere is a neighbour.
 *   Scatter: the covariance rule of mi_estimate_covariances, taken over the ball instead of a k-list.  c = neighbours[i] + 1 (the point
 *     itself contributes d = 0); d = p_j - p_i in fp64 (exact, or rounded at 2^-53); nine running fp64 sums S = sum d and Q = sum d d^T
 *     (upper triangle), one product and one addition per entry and neighbour; m = S / c, C_ab = Q_ab / c - m_a m_b.  The summation order
 *     is the walk's over the call's cell grid: a function of the cloud, the radii and the context's tuning alone.
 *   Eigenvalues: lambda0 <= lambda1 <= lambda2 of C by the fp64 cyclic Jacobi of mi_estimate_normals; eigenvalues[3 i .. 3 i + 2] are
 *     those, each rounded once to fp32, written for EVERY point, gated or not; 0, 0, 0 where neighbours[i] = 0.
 *   Gate, in fp64: point i passes when neighbours[i] >= min_neighbours, lambda1 < (double)gamma_21 * lambda2 and
 *     lambda0 < (double)gamma_32 * lambda1.  Products, not quotients: a zero matrix fails and nothing divides by 0.
 *   Saliency: saliency[i] = max((float)lambda0, 0) where the gate holds, +0 elsewhere.  Point i is a candidate iff saliency[i] > 0.  An
 *     exact plane z = const gives lambda0 = 0 exactly (the Jacobi sweep skips zero off-diagonal entries), so none of its points is a
 *     candidate; a cloud of identical points has none either.
 *   Non-maximum suppression, on the fp32 saliency values alone: candidate i is a keypoint iff its non-max ball
 *     { j != i : d2(i, j) <= r2n } holds at least min_neighbours points and, for every j in it, saliency[i] > saliency[j], or
 *     saliency[i] == saliency[j] and i < j.  The index tie-break departs from Open3D, whose strict ">" drops both of two tied points:
 *     two nearby points often share the set ball + self, hence the covariance and, after the rounding, the saliency; here exactly one
 *     point of such a cluster survives.
 *   Outputs: is_keypoint is 0 / 1 per point; out_index holds the indices of the ones, ascending; out_xyz their coordinates, the input's
 *     bits; *out_n their number.  Rows beyond *out_n are not written.  Asking for fewer optional outputs moves no bit of the rest.
 *   Deterministic: the same call gives the same bits whatever ran on the context before.  No floating-point atomics.
 *   Cost: a point's work is proportional to the number of points in its balls (and its cell's neighbourhood), so a radius that holds a
 *     large share of the cloud makes the call quadratic.  The cloud's resolution comes from mi_remove_outliers (statistical, k = 1:
 *     stats->mean); six and four times that resolution are the usual radii.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with "mi_iss_keypoints" and names the cause and, for a bad point, its index (the
 *     lowest); NO output has been written -- for a NULL ctx, cloud_xyz, params or out_n; n < 1; an unknown dist_mode; a radius that is
 *     NaN, infinite or <= 0, or whose square is not finite; a gamma that is NaN, infinite or <= 0; min_neighbours < 1; a non-finite
 *     coordinate or one above 1e18 in magnitude.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the other calls keep: it works in buffers of its own.
 *   Synchronous, host in and host out. */
int mi_iss_keypoints(mi_ctx* ctx, const float* cloud_xyz, int n, const mi_iss_params* params,
                     float* out_xyz,            /* may be NULL; capacity n points: the keypoints, input bits, ascending caller index */
                     int* out_index,            /* may be NULL; capacity n */
                     int* out_n,                /* non-NULL */
                     unsigned char* is_keypoint,/* may be NULL; n */
                     float* saliency,           /* may be NULL; n */
                     float* eigenvalues,        /* may be NULL; 3n: ascending per point */
                     int* neighbours);          /* may be NULL; n: points in the salient ball */

/* Where the last mi_iss_keypoints of this context spent its host wall time, in ms (measurement hook, tools/iss_bench.py):
 *   out[0] workspace (device allocations)           out[1] upload + AoS -> SoA
 *   out[2] input check, bounding box, its read-back out[3] cell grid over the cloud
 *   out[4] curve order of the cloud + permute       out[5] the saliency kernel (K32)
 *   out[6] suppression (K33) + compaction + download    out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage, and out[5] is the
 * launch's own HIP-event time instead of host wall time). */
#define MI_ISS_STAGES 8
int mi_iss_keypoints_times(mi_ctx* ctx, double out_ms[MI_ISS_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * Moving-least-squares surface smoothing (Alexa et al. 2003; PCL's MovingLeastSquares without upsampling; no reference counterpart):
 * moves every query back onto the surface its neighbourhood was sampled from and returns that surface's normal, to be taken between
 * mi_remove_outliers and mi_estimate_normals (smoothing).  Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */
typedef struct mi_mls_params {
    float radius;          /* finite, > 0, square finite: the ball of every fit                           default 0: the caller must set it */
    float gauss_scale;     /* finite, > 0, or 0 = radius (PCL's sqr_gauss_param = radius^2)                default 0 */
    int   order;           /* 1: project onto the local plane; 2: onto the quadratic over it               default 2 */
    int   min_neighbours;  /* >= 3: fewer points in the ball leave the query untouched                     default 3 */
    int   dist_mode;       /* MI_DIST_CPU_ROUNDING / MI_DIST_FMA, as mi_knn_search                         default CPU_ROUNDING */
    int   reserved[11];
} mi_mls_params;           /* 64 bytes */
void mi_mls_params_default(mi_mls_params* p);

#define MI_MLS_QUADRATIC 0   /* out_status: the quadratic fit */
#define MI_MLS_PLANE 1       /*             the plane alone */
#define MI_MLS_UNTOUCHED 2   /*             fewer than min_neighbours points in the ball */

/* The queries (query_xyz == NULL: the cloud's own points, nq == n) projected onto a polynomial fitted to the cloud's points around them,
 * computed on the device.  Every rule below can be retraced in numpy (tests/mls_reference.py does); everything is fp64 unless said
 * otherwise, one operation per written operator, products before sums, sums of three as (a + b) + c.
 *   Ball of query q: N = { j : d2(q, p_j) <= r2 }, r2 = radius * radius in one IEEE fp32 multiplication, d2 in the dist_mode arithmetic
 *     of mi_knn_search.  A point AT the radius belongs.  Nothing is skipped: with query_xyz == NULL point i is in its own ball, and so
 *     are its duplicates.  out_neighbours[q] = c = |N|; in self mode that is the count mi_remove_outliers gives in radius mode at the
 *     same radius with its neighbours output, plus one.
 *   Untouched: c < min_neighbours: out_xyz = the query's input bits, normal (0, 0, 0), curvature 0, status MI_MLS_UNTOUCHED.
 *   Plane (first walk over the ball): d = p_j - q (exact, or rounded at 2^-53); nine running sums S = sum d and Q = sum d d^T (upper
 *     triangle), one product and one addition per entry and point; m = S / c, C_ab = Q_ab / c - m_a m_b: the covariance rule of
 *     mi_estimate_covariances with the query in the place of the point.  lambda0 <= lambda1 <= lambda2 and the eigenvector of lambda0
 *     by the fp64 cyclic Jacobi of mi_estimate_normals, normalised: the unit normal n.  Its sign is deterministic and otherwise
 *     unspecified, as for mi_estimate_normals without a viewpoint.  Curvature = max(lambda0, 0) / ((lambda0 + lambda1) + lambda2), 0
 *     where that sum is not positive.  The query's foot on the plane, relative to q: o = t n, t = (n_x m_x + n_y m_y) + n_z m_z.
 *   Frame: k = the axis with the smallest |n_k|, the lowest k on ties; u = (e_k x n) / |e_k x n|, v = n x u.
 *   Quadratic (second walk over the same ball; order == 2 and c >= 6 only): e = d - o; a = u . e, b = v . e, f = n . e;
 *     w = exp(-((d_x d_x + d_y d_y) + d_z d_z) / (s s)) with s = (double)gauss_scale, or (double)radius where gauss_scale is 0;
 *     phi = (1, a, b, a a, a b, b b); A_ij += (w phi_i) phi_j for i <= j (21 sums) and g_i += (w phi_i) f (6 sums).  A x = g by
 *     the solve of mi_icp_plane_register: A scaled to a unit diagonal, LDL^T without pivoting, a diagonal entry that is not positive
 *     and finite or a pivot below 1e-10 is degenerate.  A degenerate system falls back to the plane.
 *   Outputs, each rounded once to fp32:
 *     MI_MLS_QUADRATIC  out_xyz_k = (float)((q_k + o_k) + x_0 n_k); the normal (n_k - x_1 u_k) - x_2 v_k, divided by its length
 *     MI_MLS_PLANE      (order == 1, c < 6, or a degenerate system)  out_xyz_k = (float)(q_k + o_k); the normal n
 *     The curvature is the plane's in both.  An exact plane z = const gives lambda0 = 0, n = (0, 0, 1), o = 0 and every f = 0
 *     exactly: out_xyz is the query's input bits.  A cloud of identical points gives MI_MLS_PLANE with o = 0.
 *   Summation order: the walk's over the call's cell grid (cells about one radius long): a function of the cloud, the radius and
 *     the context's tuning alone, not of the queries' number or order.
 *   Deterministic: the same call gives the same bits whatever ran on the context before.  No floating-point atomics.  Asking for
 *     fewer optional outputs moves no bit of the rest.
 *   Cost: a query's work is proportional to the number of points in its ball (and its cell's neighbourhood), walked twice at order 2.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with "mi_mls_smooth" and names the cause and, for a bad point, its index (the
 *     lowest); NO output has been written -- for a NULL ctx, cloud_xyz, params or out_xyz; n < 1 or nq < 1; query_xyz == NULL with
 *     nq != n; an unknown dist_mode; a radius that is NaN, infinite or <= 0, or whose square is not finite; a gauss_scale that is
 *     NaN, infinite or < 0; an order outside {1, 2}; min_neighbours < 3; a non-finite coordinate or one above 1e18 in magnitude.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the other calls keep: it works in buffers of its own.
 *   Synchronous, host in and host out. */
int mi_mls_smooth(mi_ctx* ctx, const float* cloud_xyz, int n,
                  const float* query_xyz,       /* NULL: the cloud itself (nq == n) */
                  int nq, const mi_mls_params* params,
                  float* out_xyz,               /* nq * 3, non-NULL */
                  float* out_normals,           /* nq * 3, may be NULL */
                  float* out_curvature,         /* nq, may be NULL */
                  int* out_neighbours,          /* nq, may be NULL */
                  unsigned char* out_status);   /* nq, may be NULL: MI_MLS_QUADRATIC / MI_MLS_PLANE / MI_MLS_UNTOUCHED */

/* Where the last mi_mls_smooth of this context spent its host wall time, in ms (measurement hook, tools/mls_bench.py):
 *   out[0] workspace (device allocations)           out[1] upload + AoS -> SoA
 *   out[2] input check, bounding box, its read-back out[3] cell grid over the cloud
 *   out[4] curve order of the queries + permute     out[5] the fit kernel (K50)
 *   out[6] download                                 out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage, and out[5] is the
 * launch's own HIP-event time instead of host wall time). */
#define MI_MLS_STAGES 8
int mi_mls_smooth_times(mi_ctx* ctx, double out_ms[MI_MLS_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * Density-based clustering (DBSCAN, Ester et al. 1996; with min_points = 1 Euclidean cluster extraction; no reference counterpart):
 * splits a scene into its objects, drops clutter by component size, and yields the per-object clouds that mi_icp_register_batch and
 * mi_cpd_register_batch take (clustering).  Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */
typedef struct mi_cluster_params {
    float radius;            /* eps: finite, > 0, square finite                                            default 0: the caller must set it */
    int   min_points;        /* >= 1: a point is CORE if its ball holds >= min_points points, ITSELF INCLUDED (Open3D, sklearn)   default 1: Euclidean clustering */
    int   min_cluster_size;  /* >= 1                                                                        default 1 */
    int   max_cluster_size;  /* 0: no upper limit; else >= min_cluster_size                                 default 0 */
    int   dist_mode;         /* MI_DIST_CPU_ROUNDING / MI_DIST_FMA, as mi_knn_search                        default CPU_ROUNDING */
    int   reserved[11];
} mi_cluster_params;         /* 64 bytes */
void mi_cluster_params_default(mi_cluster_params* p);

/* The clusters of a cloud, computed on the device.  The result is a pure integer function of the input: every rule below can be retraced
 * in numpy (tests/cluster_reference.py does), and the same input gives the same bits on every run.
 *   Neighbours: j is a neighbour of i when j != i (by index) and d2(i, j) <= r2, with r2 = radius * radius, one IEEE fp32 multiplication
 *     on the host, and d2 the fp32 squared distance of dist_mode, exactly as in mi_remove_outliers' radius method and mi_iss_keypoints.  A
 *     point AT the radius belongs; a duplicate of point i stored elsewhere is a neighbour.  d2 is symmetric bit for bit in both modes: the
 *     three differences of (j, i) are the exact negations of those of (i, j), a square does not see the sign, and the sum is taken in
 *     the same order -- so "i is a neighbour of j" and "j is a neighbour of i" are one statement.
 *   Core: point i is core when 1 + (the number of its neighbours) >= min_points.  is_core[i] is 1 for a core point and 0 otherwise; the
 *     size filter below does not change it.
 *   Clusters: two core points are in one cluster when a chain of core points, each a neighbour of the next, joins them.
 *   Border: a point that is not core and has at least one core neighbour joins the cluster of the core neighbour j with the smallest
 *     packed key (bits(d2(i, j)) << 32) | j: the nearest one, the lower index on an exact tie.  A border point never joins two clusters
 *     and never links two.  This is a stated rule that does not depend on any order; Open3D's and sklearn's DBSCAN give a border point to
 *     whichever cluster's expansion visits it first, so their border labels depend on the order of the input and may differ from these
 *     (the core points, their partition and the noise set are the same).
 *   Noise: every other point; its label is -1.
 *   Size filter: the size of a cluster counts its core and its border points.  A cluster smaller than min_cluster_size, or larger than
 *     max_cluster_size where that is not 0, is dissolved: its points get the label -1.
 *   Numbering: the surviving clusters are numbered 0 .. *n_clusters - 1 by ascending smallest CORE member index, in the caller's order.
 *     The output therefore does not depend on scheduling, on the cell size of the call's grid or on its curve order.
 *   Outputs: labels[i] is the cluster of point i or -1; *n_clusters the number of surviving clusters; cluster_sizes[c], for
 *     c < min(*n_clusters, cluster_cap), the size of cluster c (entries beyond are not written).  grouped_index holds the labelled points
 *     (label >= 0) sorted by (label, index) -- the members of cluster 0 in ascending index, then those of cluster 1, ... -- and *n_grouped
 *     is their number (capacity n).  The members of cluster c start at the running sum of cluster_sizes[0 .. c - 1]: the offsets are that
 *     sum, and there is no output for them.  Asking for fewer optional outputs moves no bit of the rest.
 *   Cost: a point's work is proportional to the number of points in its ball (and its cell's neighbourhood), so a radius that holds a
 *     large share of the cloud makes the call quadratic.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with "mi_cluster_dbscan" and names the cause and, for a bad point, its index (the
 *     lowest); NOTHING the caller passed has been written -- for a NULL ctx, cloud_xyz, params, labels or n_clusters; n < 1; a radius that
 *     is NaN, infinite or <= 0, or whose square is not finite; min_points < 1; min_cluster_size < 1; max_cluster_size < 0, or
 *     0 < max_cluster_size < min_cluster_size; cluster_sizes given with cluster_cap < 1; grouped_index without n_grouped; an unknown
 *     dist_mode; a non-finite coordinate or one above 1e18 in magnitude.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the other calls keep: it works in buffers of its own.
 *   Synchronous, host in and host out. */
int mi_cluster_dbscan(mi_ctx* ctx, const float* cloud_xyz, int n, const mi_cluster_params* params,
                      int* labels,               /* non-NULL; n */
                      int* n_clusters,           /* non-NULL */
                      int* cluster_sizes,        /* may be NULL; the first min(*n_clusters, cluster_cap) sizes */
                      int cluster_cap,           /* >= 1 where cluster_sizes is given; ignored otherwise */
                      unsigned char* is_core,    /* may be NULL; n */
                      int* grouped_index,        /* may be NULL; capacity n: the labelled points by (label, index) */
                      int* n_grouped);           /* non-NULL where grouped_index is given; may be given alone */

/* Where the last mi_cluster_dbscan of this context spent its host wall time, in ms (measurement hook, tools/cluster_bench.py):
 *   out[0] workspace (device allocations)           out[1] upload + AoS -> SoA, input check, bounding box, its read-back
 *   out[2] cell grid over the cloud, curve order    out[3] the core count (K15's count kernel; 0 with min_points = 1)
 *   out[4] the link kernel (K34)                    out[5] the resolve kernel (K35)
 *   out[6] sizes, filter, numbering, labels, the grouping and the downloads     out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage, and out[4] is the
 * launch's own HIP-event time instead of host wall time). */
#define MI_CLUSTER_STAGES 8
int mi_cluster_dbscan_times(mi_ctx* ctx, double out_ms[MI_CLUSTER_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * The dominant planes of a cloud (no reference counterpart): hypothesise and verify, as Open3D's segment_plane and PCL's SACSegmentation
 * with SACMODEL_PLANE -- three draws, the plane through them, a count of the points it explains, every hypothesis evaluated, the best one
 * refined by least squares, its points taken out, and again for the next plane.  The step in front of mi_cluster_dbscan (INTEGRATION.md:
 * planes out, then clusters).  No params struct: every setting is a scalar argument.  Single-GPU contexts only.
 *
 * Every rule below can be retraced in numpy (tests/segment_reference.py does), and the same input gives the same bits on every run.
 *   Rounds: round p = 0 .. max_planes - 1 works on the REMAINING points, those without a plane yet, in ascending caller index: they are
 *     ranks 0 .. C_p - 1, and C_0 = n.  The call ends in front of a round with C_p < 3 or C_p < min_inliers.
 *   Draws, as mi_ransac_register's with the global hypothesis number g = p * H + h, in unsigned 64-bit arithmetic modulo 2^64:
 *       u_r = mix(seed + 0x9E3779B97F4A7C15 * (3 g + r + 1)),  r = 0, 1, 2,   rank_r = ((u_r >> 32) * C_p) >> 32,   mix: the splitmix64 finaliser.
 *     Two equal ranks make the hypothesis invalid.  The triple reported is the three caller indices, in draw order.
 *   Plane of a hypothesis, in fp64 from the fp32 coordinates: e1 = p1 - p0, e2 = p2 - p0, component by component; N = e1 x e2, each
 *     component two products and one subtraction (Nx = e1y e2z - e1z e2y, Ny = e1z e2x - e1x e2z, Nz = e1x e2y - e1y e2x);
 *     len2 = (Nx Nx + Ny Ny) + Nz Nz.  len2 zero or not finite (collinear or coincident points): invalid.  q = 1.0 / sqrt(len2).  The plane
 *     is rounded to fp32 at birth: (a, b, c) = (float)(N q), d = (float)(-(((Nx x0 + Ny y0) + Nz z0) q)).  A non-finite plane is invalid.
 *     An invalid hypothesis reports (0, 0, 0, 0) and counts nothing.
 *   Axis rule, only where axis3 is given, in fp64 from the fp32 values: dot = (a ax + b ay) + c az, aa = (ax ax + ay ay) + az az,
 *     nn = (a a + b b) + c c; the hypothesis stays valid iff dot dot >= (cos cos) (aa nn), cos = min_axis_cosine: the plane's normal is
 *     within acos(cos) of +-axis.  The rule is NOT applied again to refined planes.
 *   Count, over the remaining points, in fp64 from the fp32 plane: s = ((a x + b y) + c z) + d; the point is an inlier iff
 *     s s <= T2 nn, T2 = (double)distance_threshold * (double)distance_threshold.  No root and no division: the count is an integer function
 *     of the reported plane, and a point exactly at the threshold belongs.
 *   Winner: the valid hypothesis with the most inliers, the lowest h among equals.  The call ends when no hypothesis is valid or the
 *     winner has fewer than min_inliers.
 *   Refinement, refine_iterations times: the fp64 centroid of the current inliers (each coordinate's sum divided by their number), then
 *     the six fp64 sums of products of (p - centroid), xx xy xz yy yz zz.  Every sum in one fixed order: rank r among the remaining
 *     points to partial sum r mod 256 in ascending r, the partial sums added pairwise at strides 128, 64 .. 1.  The unit eigenvector of
 *     the smallest eigenvalue (csrc/eig3.hpp in fp64), turned where its fp64 dot with the previous (a, b, c) is negative; d = -(n . centroid)
 *     summed left to right; the plane rounded to fp32; a recount under the count rule.  An iteration that leaves fewer than 3 inliers,
 *     or a non-finite plane, is not taken and ends refinement.
 *   Outputs: plane p is the fp32 plane after refinement, plane_inliers[p] its final count, labels[i] = p at its inliers (-1: no plane),
 *     rmse[p] = (float)sqrt(S / count) with S the sum of s s / nn over the inliers in the fixed order above, winners[p] the winning h of
 *     round p.  The inliers then leave the remaining set.  Entries of the per-plane arrays at and beyond *n_planes are not written.
 *     Asking for fewer optional outputs moves no bit of the rest.  A call that finds nothing returns MI_OK with *n_planes = 0 and,
 *     where asked for, every label -1.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name and names the cause and, for a bad point, its index (the
 *     lowest); NOTHING the caller passed has been written -- for a NULL ctx, cloud_xyz, planes4 or n_planes; n < 3; a distance_threshold
 *     that is NaN, infinite or <= 0, or whose fp32 square is not finite; hypotheses, refine_iterations or max_planes outside the ranges
 *     below; min_inliers < 3; with axis3: a non-finite or zero axis, a min_axis_cosine outside [0, 1); a non-finite coordinate or one above
 *     1e18 in magnitude.  MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the other calls keep: it works in buffers of its own.
 *   Synchronous, host in and host out. */
#define MI_SEGMENT_MAX_PLANES 16
int mi_segment_plane(mi_ctx* ctx, const float* cloud_xyz, int n,
                     float distance_threshold,        /* > 0, finite, square finite */
                     int hypotheses,                  /* H: 1 .. MI_RANSAC_MAX_HYPOTHESES, every one evaluated, per plane */
                     unsigned long long seed,
                     int refine_iterations,           /* 0 .. MI_RANSAC_MAX_REFINE */
                     int max_planes,                  /* P: 1 .. MI_SEGMENT_MAX_PLANES */
                     int min_inliers,                 /* >= 3: a winner with fewer ends the call */
                     const float axis3[3],            /* may be NULL: no constraint */
                     float min_axis_cosine,           /* in [0, 1); read only with axis3 */
                     float* planes4,                  /* non-NULL; 4 * P: a, b, c, d with a x + b y + c z + d = 0 */
                     int* n_planes,                   /* non-NULL */
                     int* plane_inliers,              /* may be NULL; P */
                     int* labels,                     /* may be NULL; n: plane number or -1 */
                     float* rmse,                     /* may be NULL; P */
                     int* winners);                   /* may be NULL; P: the winning h of each round */
/* Test-grade primitive, like mi_ransac_hypotheses: hypotheses first .. first + count - 1 of ROUND 0 (the whole cloud) of the call above
 * (first >= 0, count >= 1, first + count <= hypotheses), each with its triple (3 caller indices), valid flag, plane and inlier count.
 * Every output may be NULL.  The same checks and errors. */
int mi_segment_plane_hypotheses(mi_ctx* ctx, const float* cloud_xyz, int n, float distance_threshold, int hypotheses,
                                unsigned long long seed, const float axis3[3], float min_axis_cosine, int first, int count,
                                int* triples /* 3*count */, unsigned char* valid /* count */, float* plane4 /* 4*count */, int* inlier_count /* count */);
/* Where the last mi_segment_plane of this context spent its host wall time, in ms, summed over the rounds (measurement hook,
 * tools/segment_bench.py):
 *   out[0] workspace (device allocations)           out[1] upload + AoS -> SoA
 *   out[2] input check and its read-back            out[3] the hypothesis kernel (K39)
 *   out[4] the counting kernel (K40)                out[5] arg-max and the winner's read-back
 *   out[6] flags, sums, refinement, labels, the peel and the downloads          out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage). */
#define MI_SEGMENT_STAGES 8
int mi_segment_plane_times(mi_ctx* ctx, double out_ms[MI_SEGMENT_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * Point-to-plane ICP (no reference counterpart: the reference's ICP is point-to-point): the registration the normals are for
 * (plane registration).  It minimises sum (n_j . (R b_i + t - a_j))^2 over the matched pairs, linearised about the
 * current pose, and does not stall on surfaces that slide along themselves.  A sibling of mi_icp_register with buffers, state and
 * kernels of its own; single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */
#define MI_STOP_DEGENERATE 7      /* point-to-plane: the 6 x 6 system does not determine all six motions */

typedef struct mi_plane_params {
    float eps_rotation;           /* converged when |omega| <= this (radians) ...            default 1e-6 */
    float eps_translation;        /* ... and |v| <= this (the clouds' units)                 default 1e-6 */
    int   max_iterations;         /* >= 0; there is no unbounded mode                        default 50   */
    float max_distance_squared;   /* a match with d2 > this is no pair; INFINITY: no limit   default INFINITY */
    int   dist_mode;              /* MI_DIST_CPU_ROUNDING / MI_DIST_FMA, as mi_knn_search     default CPU_ROUNDING */
    int   sync_every;             /* iterations enqueued between host reads of the state; 0 = 4; moves no bit */
    int   verbose;
    int   reserved[9];
} mi_plane_params;
void mi_plane_params_default(mi_plane_params* p);

/* Registers the moving cloud `before` (n points) onto the fixed cloud `after` (m points) with normals, on the device.  Every rule below
 * can be retraced in numpy (tests/plane_reference.py does).
 *   Transform: T, init_T and out_T are column-major 4 x 4 like every transform of this library, T[4 * col + row]; only the rotation
 *     block and the translation column are read.  The rotation block is used as given: neither checked for orthonormality nor
 *     re-orthonormalised.  init_T (NULL: the identity) is promoted to fp64 exactly, and the running pose (R, t) is held in fp64 on the
 *     device.  An iteration applies the pose's rounding to fp32: with every R_ij and t_i rounded once to fp32 and every operation below
 *     rounded to fp32, in this order, q_x = ((R00*b_x + R01*b_y) + R02*b_z) + t_x, and likewise q_y and q_z.
 *   Match: the pair of moving point i is row i of mi_knn_search(ctx, q, n, after_xyz, m, 1, dist_mode, max_distance_squared, ...), key
 *     for key: the same distance arithmetic on the fp32 differences a_j - q_i, equal distance bits going to the lower index.  A query
 *     without a candidate within the limit has no pair.  A query whose matched normal is exactly (0, 0, 0) has no pair either:
 *     mi_estimate_normals writes that normal for a point with fewer than three neighbours.  Normals are otherwise used as given, unit
 *     length or not.
 *   Centre: c0 = 0.5f * (lo + hi) per axis, one fp32 addition and one fp32 multiplication, of the fixed cloud's bounding box.  The
 *     moments are taken about c0, which keeps the system's conditioning independent of the clouds' offset from the origin.
 *   Terms, every operand promoted to fp64 first: r = n . (q - a), J = [(q - c0) x n, n] (six numbers: the three of the rotation
 *     about c0, then the three of the translation).
 *   Sums (mi_plane_system's out_sums): [0, 21) the upper triangle of A = sum J J^T, row-major; [21, 27) g = sum J r; [27] sum r^2;
 *     [28] sum d2 (the matches' fp32 squared distances); [29] the number of pairs; [30, 32) 0.  The sums are added in a fixed order
 *     that depends on n alone, with no floating-point atomics: the same input gives the same bits on every call, whatever ran on the
 *     context before.
 *   Solve: fewer than 6 pairs stop the loop with MI_STOP_NO_PAIRS.  A diagonal entry of A that is <= 0 or not finite stops it with
 *     MI_STOP_DEGENERATE (an exact plane has diagonal entries that are exactly 0).  Otherwise A is scaled to a unit diagonal,
 *     S = D^-1/2 A D^-1/2, and S is factored as L D' L^T without pivoting in fp64; a pivot below 1e-10 stops the loop with
 *     MI_STOP_DEGENERATE (a well-constrained scene has a smallest pivot of about 0.6).  Either stop leaves the pose of the previous
 *     iteration untouched.  Otherwise x = (omega, v) solves A x = -g.
 *   Update: dR = exp([omega]x) by Rodrigues' formula in fp64 (its series below |omega| = 1e-8); R <- dR R;
 *     t <- dR (t - c0) + c0 + v.
 *   Stop rule, tested in this order after every update: MI_STOP_CONVERGED when both |omega|_2 <= eps_rotation and
 *     |v|_2 <= eps_translation; MI_STOP_MAX_ITERATIONS when `iterations` has reached max_iterations.  max_iterations = 0 returns init_T
 *     (or the identity) with 0 iterations, error 0 and MI_STOP_MAX_ITERATIONS.
 *   Outputs: out_T is the fp64 pose rounded once to fp32 (bottom row 0 0 0 1); *iterations counts the updates applied; *error is
 *     sum r^2 / pairs of the last linearisation -- the one the last update, or the stop, was decided from -- rounded to fp32, and 0
 *     when that linearisation had no pair; *stop_reason is one of the four MI_STOP_* above.  Any of the last three may be NULL.
 *   sync_every: the iterations run on the device, sync_every of them enqueued between two host reads of the state block (0: 4); a
 *     launch behind the stop returns at once.  It moves no bit of any output.
 *   The search is exact for any start; the speed is only claimed for a start within a few cells of the fixed cloud, as mi_knn_search
 *     says of itself.  A finite max_distance_squared bounds every walk.  Nothing bounds the pose: a huge init_T or a barely determined
 *     solve can carry q to infinity or NaN; such a point has no pair and its lane walks the whole grid, so a diverged pose shows as
 *     slow iterations that end in MI_STOP_NO_PAIRS, not as an error.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name and names the cause and, for a bad point, which array and
 *     which index (the lowest); NO output has been written -- for a NULL ctx, before_xyz, after_xyz, after_normals_xyz, params or
 *     out_T; n < 1 or m < 1; a dist_mode other than the two of mi_knn_search; max_distance_squared NaN or negative; eps_rotation or
 *     eps_translation NaN or negative; max_iterations < 0; sync_every < 0; a non-finite entry of init_T's rotation block or translation
 *     column; a non-finite coordinate or normal component, or one above 1e18 in magnitude.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything mi_knn_search, mi_estimate_normals and
 *     mi_remove_outliers keep: it works in buffers of its own.
 *   Synchronous, host in and host out. */
int mi_icp_plane_register(mi_ctx* ctx, const float* before_xyz, int n,
                          const float* after_xyz, const float* after_normals_xyz, int m,
                          const mi_plane_params* params, const float init_T[16] /* may be NULL: identity */,
                          float out_T[16], int* iterations, float* error, int* stop_reason);

/* One linearisation at a given transform, for tests and callers who run their own loop: the sums above at the pose T (NULL: the
 * identity, the same bits), the centre c0, and per moving point the fixed index of its pair, or -1 where it has none.  The same
 * arguments are refused, with out_sums in the place of out_T; out_centre and out_idx may be NULL. */
int mi_plane_system(mi_ctx* ctx, const float* before_xyz, int n, const float* after_xyz, const float* after_normals_xyz, int m,
                    const float T[16] /* may be NULL */, int dist_mode, float max_distance_squared,
                    double out_sums[32], float out_centre[3], int* out_idx /* may be NULL; n: matched fixed index or -1 */);

/* Where the last mi_icp_plane_register or mi_plane_system of this context spent its host wall time, in ms (measurement hook,
 * tools/plane_icp_bench.py):
 *   out[0] workspace (device allocations)           out[1] upload + AoS -> SoA (normals, fixed cloud, moving cloud, state)
 *   out[2] input checks, bounding box, read-backs   out[3] cell grid over the fixed cloud
 *   out[4] curve order of the moving cloud + permute out[5] the iterations, host reads of the state included
 *   out[6] download of the results                  out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage). */
#define MI_PLANE_STAGES 8
int mi_icp_plane_times(mi_ctx* ctx, double out_ms[MI_PLANE_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * Generalized ICP (no reference counterpart), also called plane-to-plane or distribution-to-distribution ICP (Segal, Haehnel, Thrun:
 * Generalized-ICP, RSS 2009; INTEGRATION.md: generalized registration).  It minimises sum d^T (C_a + R C_b R^T)^-1 d over the matched
 * pairs, d = R b_i + t - a_j, with a 3 x 3 covariance per point of BOTH clouds: the surface model of both sides, so it tolerates the
 * sampling mismatch between two scans of one surface that biases point-to-plane and stalls point-to-point.  Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */
#define MI_COV_RAW   0            /* the neighbourhood's covariance itself */
#define MI_COV_PLANE 1            /* its eigenvalues replaced by (epsilon, 1, 1): the GICP regularisation */

/* Per-point 3 x 3 covariances of a cloud, computed on the device: six floats per point, the upper triangle row by row
 * (xx, xy, xz, yy, yz, zz).  Every rule can be retraced in numpy (tests/gicp_reference.py does).
 *   Neighbourhood of point i: point i itself plus the neighbours that
 *     mi_knn_search(ctx, NULL, n, cloud_xyz, n, k, dist_mode, max_distance_squared, ...) returns for row i -- the same set, bit for
 *     bit: self mode skips by index, and a duplicate of point i stored elsewhere is a neighbour.  count[i] is that call's count[i].
 *     A finite max_distance_squared makes it the "hybrid" k-and-radius neighbourhood; INFINITY is no limit.
 *   Covariance: that of the neighbourhood's count + 1 points about their mean, divided by the number of points, in fp64.  It is formed
 *     in one pass from the differences d = p_j - p_i, taken in fp64 (exact, or rounded at 2^-53): nine running sums S = sum d,
 *     Q = sum d d^T (one product and one addition per entry and neighbour), added in the order of mi_knn_search's row i, nearest first;
 *     then with c = count + 1, m = S / c and C_ab = Q_ab / c - m_a m_b (one division, one product, one subtraction);
 *     the point itself contributes d = 0.  It is mi_estimate_normals' covariance: the same kernel body in the same order.
 *   MI_COV_RAW: every entry of C rounded once to fp32.  epsilon is ignored.
 *   MI_COV_PLANE: C's eigenvalues replaced by (epsilon, 1, 1), the smallest by epsilon: I - (1 - epsilon) n n^T, with n the unit
 *     eigenvector of C's smallest eigenvalue from mi_estimate_normals' fp64 cyclic Jacobi iteration, normalised in fp64 and NOT rounded
 *     to fp32.  In fp64, in this order: w = 1 - epsilon (epsilon promoted); u = w n (three products); entry ab = delta_ab - u_a n_b (one
 *     product, one subtraction from 1 or 0), a <= b; each rounded once to fp32.  The sign of n cancels.  epsilon must be finite and in
 *     [0, 1].
 *   Too few points: with count[i] < 2 all six entries are 0 in both modes -- a covariance mi_icp_gicp_register treats as "none".
 *   MI_ERR_INVALID_ARG -- mi_last_error names the cause and, for a bad point, its index; NO output array has been written -- for a
 *     NULL ctx, cloud_xyz or cov6; n < 1; k outside [2, MI_KNN_MAX_K]; a dist_mode other than the two of mi_knn_search;
 *     max_distance_squared NaN or negative; a mode other than the two above; with MI_COV_PLANE an epsilon that is not finite or outside
 *     [0, 1]; a non-finite coordinate or one above 1e18 in magnitude.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the other calls of this header keep: it works in buffers
 *     of its own.  Synchronous, host in and host out. */
int mi_estimate_covariances(mi_ctx* ctx,
                            const float* cloud_xyz, int n,
                            int k, int dist_mode,            /* 2 <= k <= MI_KNN_MAX_K; MI_DIST_CPU_ROUNDING or MI_DIST_FMA */
                            float max_distance_squared,      /* INFINITY: no limit; else neighbours with d2 > this do not exist */
                            int mode, float epsilon,         /* MI_COV_RAW / MI_COV_PLANE; epsilon in [0, 1], read by MI_COV_PLANE only */
                            float* cov6,                     /* n*6 */
                            int* count);                     /* may be NULL; n: neighbours used for point i (<= k) */

/* Registers the moving cloud `before` (n points, covariances before_cov6) onto the fixed cloud `after` (m points, covariances
 * after_cov6), on the device.  params is mi_plane_params, and every field means here what it means for mi_icp_plane_register.  Every
 * rule below can be retraced in numpy (tests/gicp_reference.py does).
 *   Transform, the pose's rounding to fp32, q, match, centre c0: exactly those of mi_icp_plane_register -- q = ((R00*b_x + R01*b_y) +
 *     R02*b_z) + t_x in fp32 with the pose rounded once; the pair of moving point i is row i of mi_knn_search(ctx, q, n, after_xyz, m, 1,
 *     dist_mode, max_distance_squared, ...), key for key; c0 = 0.5f * (lo + hi) of the fixed cloud's bounding box.
 *   Covariances: six floats per point, the upper triangle row by row (xx, xy, xz, yy, yz, zz), as mi_estimate_covariances writes them.
 *     They are used as given: not checked for symmetry (there is none to check: the lower triangle is the upper one) or definiteness,
 *     only for finiteness and |x| <= 1e18.
 *   Pair terms, every operand promoted to fp64 first and every operation rounded; Rf is the pose's rotation rounded to fp32 (the
 *     rotation q was formed with) and promoted back; j the match of i; sums of three are formed left to right, (x + y) + z:
 *       d = q - a_j
 *       T = Rf C_b[i]:       T_rc = (Rf_r0 Cb_0c + Rf_r1 Cb_1c) + Rf_r2 Cb_2c
 *       Sigma = C_a[j] + T Rf^T:  S_rc = Ca_rc + ((T_r0 Rf_c0 + T_r1 Rf_c1) + T_r2 Rf_c2) for r <= c; the lower triangle is never formed
 *       cofactors:  c00 = S11 S22 - S12 S12   c01 = S02 S12 - S01 S22   c02 = S01 S12 - S02 S11
 *                   c11 = S00 S22 - S02 S02   c12 = S01 S02 - S00 S12   c22 = S00 S11 - S01 S01   (two products, one subtraction)
 *       det = (S00 c00 + S01 c01) + S02 c02;   M = Sigma^-1:  M_rc = c_rc / det
 *     A pair whose det is <= 0 or not finite is no pair (out_idx -1).  Two zero covariances give det = 0; one zero and one proper
 *     covariance is a valid point-to-distribution pair.
 *   Linearisation: Gauss-Newton with M held fixed within the iteration.  With P = q - c0 the 3 x 6 Jacobian of the update (omega about
 *     c0, then v) is J = [ -[P]x , I ].  Writing (P x y)_0 = P_y y_2 - P_z y_1, (P x y)_1 = P_z y_0 - P_x y_2, (P x y)_2 = P_x y_1 - P_y y_0
 *     (two products, one subtraction each):
 *       W = M J (3 x 6):     W_rb = (P x M_r)_b for b < 3, M_r the row r of M;  W_rb = M_r(b-3) for b >= 3
 *       H = J^T W (6 x 6):   H_ab = (P x W_b)_a for a < 3, W_b the column b of W;  H_ab = W_(a-3)b for a >= 3;  the 21 entries a <= b
 *       Md = M d:            Md_r = (M_r0 d_x + M_r1 d_y) + M_r2 d_z
 *       g = J^T Md:          g_a = (P x Md)_a for a < 3;  g_a = Md_(a-3) for a >= 3
 *       e = d^T Md:          e = (d_x Md_0 + d_y Md_1) + d_z Md_2
 *   Sums (mi_gicp_system's out_sums), the layout of mi_plane_system: [0, 21) the upper triangle of sum H, row-major; [21, 27) sum g;
 *     [27] sum e; [28] sum d2 (the matches' fp32 squared distances); [29] the number of pairs; [30, 32) 0.  The sums are added in a
 *     fixed order that depends on n alone, with no floating-point atomics: the same input gives the same bits on every call, whatever
 *     ran on the context before and whatever sync_every.
 *   Solve, update, stop rule, outputs, sync_every, max_iterations = 0: those of mi_icp_plane_register, by the same code, with
 *     x = (omega, v) solving (sum H) x = -(sum g): MI_STOP_NO_PAIRS below 6 pairs; MI_STOP_DEGENERATE on a diagonal entry that is <= 0
 *     or not finite or a pivot of the scaled LDL^T below 1e-10 (the pose stays as it was); dR by Rodrigues' formula, R <- dR R,
 *     t <- dR (t - c0) + c0 + v; MI_STOP_CONVERGED, then MI_STOP_MAX_ITERATIONS.  *error is sum e / pairs of the last linearisation,
 *     rounded to fp32, 0 when it had no pair.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name and names the cause and, for a bad point or covariance, which
 *     array and which index (the lowest); NO output has been written -- for a NULL ctx, before_xyz, before_cov6, after_xyz, after_cov6,
 *     params or out_T; n < 1 or m < 1; a dist_mode other than the two of mi_knn_search; max_distance_squared NaN or negative;
 *     eps_rotation or eps_translation NaN or negative; max_iterations < 0; sync_every < 0; a non-finite entry of init_T's rotation block
 *     or translation column; a non-finite coordinate or covariance entry, or one above 1e18 in magnitude.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the other calls of this header keep: it works in buffers
 *     of its own.  Synchronous, host in and host out. */
int mi_icp_gicp_register(mi_ctx* ctx, const float* before_xyz, const float* before_cov6, int n,
                         const float* after_xyz, const float* after_cov6, int m,
                         const mi_plane_params* params, const float init_T[16] /* may be NULL: identity */,
                         float out_T[16], int* iterations, float* error, int* stop_reason);

/* One linearisation at a given transform, as mi_plane_system: the sums above at the pose T (NULL: the identity, the same bits), the
 * centre c0, and per moving point the fixed index of its pair, or -1 where it has none.  The same arguments are refused, with out_sums
 * in the place of out_T; out_centre and out_idx may be NULL. */
int mi_gicp_system(mi_ctx* ctx, const float* before_xyz, const float* before_cov6, int n,
                   const float* after_xyz, const float* after_cov6, int m,
                   const float T[16] /* may be NULL */, int dist_mode, float max_distance_squared,
                   double out_sums[32], float out_centre[3], int* out_idx /* may be NULL; n: matched fixed index or -1 */);

/* Where the last mi_icp_gicp_register or mi_gicp_system of this context spent its host wall time, in ms (measurement hook,
 * tools/gicp_bench.py).  The stages are those of mi_icp_plane_times, the covariances in the place of the normals:
 *   out[0] workspace (device allocations)           out[1] upload + repack (covariances, fixed cloud, moving cloud, state)
 *   out[2] input checks, bounding box, read-backs   out[3] cell grid over the fixed cloud
 *   out[4] curve order of the moving cloud + permute (its covariances with it)
 *   out[5] the iterations, host reads of the state included
 *   out[6] download of the results                  out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage). */
#define MI_GICP_STAGES 8
int mi_icp_gicp_times(mi_ctx* ctx, double out_ms[MI_GICP_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * Colored ICP (no reference counterpart): Park, Zhou, Koltun, Colored Point Cloud Registration Revisited, ICCV 2017 (INTEGRATION.md:
 * colour registration).  Beside the point-to-plane residual every pair carries a photometric one: the fixed cloud's intensity, continued
 * over its tangent plane by a per-point gradient, against the moving point's intensity.  On walls, floors and table tops the geometry
 * leaves three motions of six open (mi_icp_plane_register stops with MI_STOP_DEGENERATE there); the texture fixes them.  Intensity is
 * one float per point; a caller with colours converts them first ((r + g + b) / 3 is the usual choice).  Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */

/* Per-point colour gradients of a cloud with normals and intensities, computed on the device: three floats per point, the gradient of the
 * intensity over the point's tangent plane.  Every rule can be retraced in numpy (tests/color_reference.py does).
 *   Neighbourhood of point i: the neighbours that mi_knn_search(ctx, NULL, n, cloud_xyz, n, k, dist_mode, max_distance_squared, ...)
 *     returns for row i -- the same set in the same order, bit for bit: self mode skips by index, and a duplicate of point i stored
 *     elsewhere is a neighbour.  count[i] is that call's count[i].  A finite max_distance_squared makes it the "hybrid" k-and-radius
 *     neighbourhood; INFINITY is no limit.
 *   Sums, every operand promoted to fp64 first and every operation rounded; sums of three are formed left to right, (x + y) + z; the
 *     neighbours j are taken in the order of mi_knn_search's row i, nearest first; n is the normal of point i, used as given:
 *       e = p_j - p_i                                  s = (n_x e_x + n_y e_y) + n_z e_z
 *       u = e - s n      u_a = e_a - s n_a  (the neighbour projected into the tangent plane)
 *       delta = I_j - I_i
 *       M += u u^T       M_ab += u_a u_b for a <= b: xx, xy, xz, yy, yz, zz (one product, one addition per entry and neighbour)
 *       b += u delta     b_a += u_a delta
 *   Constraint: behind the loop, with w = (double)count[i] and ww = w w, M_ab += (ww n_a) n_b for a <= b: the row d . n = 0 of the least
 *     squares, weighted by the neighbour count.
 *   Solve: d = M^-1 b by the adjugate and the determinant, mi_icp_gicp_register's cofactors with M in the place of Sigma:
 *       c00 = M11 M22 - M12 M12   c01 = M02 M12 - M01 M22   c02 = M01 M12 - M02 M11
 *       c11 = M00 M22 - M02 M02   c12 = M01 M02 - M00 M12   c22 = M00 M11 - M01 M01   (two products, one subtraction)
 *       det = (M00 c00 + M01 c01) + M02 c02;   d_r = ((c_r0 b_0 + c_r1 b_1) + c_r2 b_2) / det, c symmetric
 *     Each component is rounded once to fp32.
 *   Zero gradient: d = (0, 0, 0) where count[i] < 2, where the normal of point i is exactly (0, 0, 0) (what mi_estimate_normals writes
 *     for a point with fewer than three points), or where det is <= 0 or not finite.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name and names the cause and, for a bad point, normal or
 *     intensity, its index (the lowest); NO output array has been written -- for a NULL ctx, cloud_xyz, normals_xyz, intensity or
 *     gradients_xyz; n < 1; k outside [2, MI_KNN_MAX_K]; a dist_mode other than the two of mi_knn_search; max_distance_squared NaN or
 *     negative; a non-finite coordinate, normal component or intensity, or one above 1e18 in magnitude.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the other calls of this header keep: it works in buffers
 *     of its own.  Synchronous, host in and host out. */
int mi_estimate_color_gradients(mi_ctx* ctx,
                                const float* cloud_xyz, const float* normals_xyz, const float* intensity, int n,
                                int k, int dist_mode,            /* 2 <= k <= MI_KNN_MAX_K; MI_DIST_CPU_ROUNDING or MI_DIST_FMA */
                                float max_distance_squared,      /* INFINITY: no limit; else neighbours with d2 > this do not exist */
                                float* gradients_xyz,            /* n*3 */
                                int* count);                     /* may be NULL; n: neighbours used for point i (<= k) */

/* Registers the moving cloud `before` (n points with intensities) onto the fixed cloud `after` (m points with normals, intensities and
 * colour gradients), on the device.  params is mi_plane_params, and every field means here what it means for mi_icp_plane_register.
 * lambda_geometric in [0, 1] weighs the geometric residual, 1 - lambda_geometric the photometric one (0.968 is the authors' choice).
 * Every rule below can be retraced in numpy (tests/color_reference.py does).
 *   Transform, the pose's rounding to fp32, q, match, centre c0: exactly those of mi_icp_plane_register -- q = ((R00*b_x + R01*b_y) +
 *     R02*b_z) + t_x in fp32 with the pose rounded once; the pair of moving point i is row i of mi_knn_search(ctx, q, n, after_xyz, m, 1,
 *     dist_mode, max_distance_squared, ...), key for key; c0 = 0.5f * (lo + hi) of the fixed cloud's bounding box.  A query without a
 *     candidate within the limit has no pair, and neither has one whose matched normal is exactly (0, 0, 0).  A matched gradient of
 *     (0, 0, 0) is still a pair: its photometric residual is the plain intensity difference.
 *   Pair terms, every operand promoted to fp64 first and every operation rounded; j the match of i, n, g and Ia the normal, gradient
 *     and intensity of fixed point j, Ib the intensity of moving point i; sums of three are formed left to right; (P x y)_0 = P_y y_2 -
 *     P_z y_1, (P x y)_1 = P_z y_0 - P_x y_2, (P x y)_2 = P_x y_1 - P_y y_0 (two products, one subtraction each):
 *       dv = q - a_j             P = q - c0
 *       rG = (n_x dv_x + n_y dv_y) + n_z dv_z                          JG = [P x n, n]      (mi_icp_plane_register's r and J)
 *       qp = dv - rG n           qp_a = dv_a - rG n_a                  (q projected into the tangent plane of a_j, relative to a_j)
 *       rC = (((g_x qp_x + g_y qp_y) + g_z qp_z) + Ia) - Ib
 *       gn = (g_x n_x + g_y n_y) + g_z n_z       mvec = g - gn n       mvec_a = g_a - gn n_a
 *       JC = [P x mvec, mvec]
 *   Weights: lg = (double)lambda_geometric, lc = 1.0 - lg.  Per pair, with a <= b over the six entries of JG and JC:
 *       H_ab = lg (JG_a JG_b) + lc (JC_a JC_b)       g_a = lg (JG_a rG) + lc (JC_a rC)       e = lg (rG rG) + lc (rC rC)
 *     With lambda_geometric = 1 the colour terms are multiplied by +0: the sums are mi_plane_system's, except where a signed zero differs.
 *   Sums (mi_color_system's out_sums), the layout of mi_plane_system: [0, 21) the upper triangle of sum H, row-major; [21, 27) sum g;
 *     [27] sum e; [28] sum d2 (the matches' fp32 squared distances); [29] the number of pairs; [30, 32) 0.  The sums are added in a
 *     fixed order that depends on n alone, with no floating-point atomics: the same input gives the same bits on every call, whatever
 *     ran on the context before and whatever sync_every.
 *   Solve, update, stop rule, outputs, sync_every, max_iterations = 0: those of mi_icp_plane_register, by the same code, with
 *     x = (omega, v) solving (sum H) x = -(sum g): MI_STOP_NO_PAIRS below 6 pairs; MI_STOP_DEGENERATE on a diagonal entry that is <= 0
 *     or not finite or a pivot of the scaled LDL^T below 1e-10 (the pose stays as it was); dR by Rodrigues' formula, R <- dR R,
 *     t <- dR (t - c0) + c0 + v; MI_STOP_CONVERGED, then MI_STOP_MAX_ITERATIONS.  *error is sum e / pairs of the last linearisation,
 *     rounded to fp32, 0 when it had no pair.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name and names the cause and, for a bad point, normal, intensity
 *     or gradient, which array and which index (the lowest); NO output has been written -- for a NULL ctx, before_xyz, before_intensity,
 *     after_xyz, after_normals_xyz, after_intensity, after_gradients_xyz, params or out_T; n < 1 or m < 1; a dist_mode other than the
 *     two of mi_knn_search; max_distance_squared NaN or negative; lambda_geometric NaN or outside [0, 1]; eps_rotation or
 *     eps_translation NaN or negative; max_iterations < 0; sync_every < 0; a non-finite entry of init_T's rotation block or translation
 *     column; a non-finite coordinate, normal component, intensity or gradient component, or one above 1e18 in magnitude.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the other calls of this header keep: it works in buffers
 *     of its own.  Synchronous, host in and host out. */
int mi_icp_color_register(mi_ctx* ctx, const float* before_xyz, const float* before_intensity, int n,
                          const float* after_xyz, const float* after_normals_xyz, const float* after_intensity,
                          const float* after_gradients_xyz, int m,
                          const mi_plane_params* params, float lambda_geometric, const float init_T[16] /* may be NULL: identity */,
                          float out_T[16], int* iterations, float* error, int* stop_reason);

/* One linearisation at a given transform, as mi_plane_system: the sums above at the pose T (NULL: the identity, the same bits), the
 * centre c0, and per moving point the fixed index of its pair, or -1 where it has none.  The same arguments are refused, with out_sums
 * in the place of out_T; out_centre and out_idx may be NULL. */
int mi_color_system(mi_ctx* ctx, const float* before_xyz, const float* before_intensity, int n,
                    const float* after_xyz, const float* after_normals_xyz, const float* after_intensity,
                    const float* after_gradients_xyz, int m,
                    const float T[16] /* may be NULL */, int dist_mode, float max_distance_squared, float lambda_geometric,
                    double out_sums[32], float out_centre[3], int* out_idx /* may be NULL; n: matched fixed index or -1 */);

/* Where the last mi_icp_color_register or mi_color_system of this context spent its host wall time, in ms (measurement hook,
 * tools/color_icp_bench.py).  The stages are those of mi_icp_plane_times, with the intensities and gradients beside the normals:
 *   out[0] workspace (device allocations)           out[1] upload + repack (intensities, gradients, normals, both clouds, state)
 *   out[2] input checks, bounding box, read-backs   out[3] cell grid over the fixed cloud
 *   out[4] curve order of the moving cloud + permute (its intensities with it)
 *   out[5] the iterations, host reads of the state included
 *   out[6] download of the results                  out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage). */
#define MI_COLOR_STAGES 8
int mi_icp_color_times(mi_ctx* ctx, double out_ms[MI_COLOR_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * Local descriptors (no reference counterpart): Fast Point Feature Histograms (Rusu, Blodow, Beetz, ICRA 2009) of a cloud with normals,
 * the descriptor a global registration matches to find the start that the local registrations above refine (INTEGRATION.md:
 * descriptors).  Matching the descriptors: mi_feature_match below (a start without odometry).  Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */

/* The 33-bin FPFH of every point of a cloud, computed on the device.  Every rule below can be retraced in numpy
 * (tests/fpfh_reference.py does).  In the arithmetic below every operand is promoted to fp64 first and every operation is rounded;
 * sums of three are formed left to right, (x + y) + z; a cross-product component is two products and one subtraction, as in the
 * generalized-ICP section.
 *   Neighbourhood of point i: row i of mi_knn_search(ctx, NULL, n, cloud_xyz, n, k, dist_mode, max_distance_squared, ...), bit for bit:
 *     self is skipped by index, a duplicate of point i stored elsewhere is a neighbour at d2 = +0, and count[i] is that call's count[i].
 *   Pair features of (i, j), p and n the points and normals as given (normals are neither checked for unit length nor normalised):
 *       d = p_j - p_i,  len = sqrt((dx*dx + dy*dy) + dz*dz);  len == 0: the features are (0, 0, 0)
 *       a1 = (n_i . d) / len,  a2 = (n_j . d) / len
 *       |a1| < |a2| (strictly):  u = n_j, t = n_i, d = -d, phi = -a2;   otherwise:  u = n_i, t = n_j, phi = a1
 *       v = d x u,  vl = sqrt((vx*vx + vy*vy) + vz*vz);  vl == 0: the features are (0, 0, 0), phi included
 *       v = v / vl,  w = u x v,  alpha = v . t,  theta = atan2(w . t, u . t)
 *     This is the Darboux-frame feature of PCL and Open3D, their test acos(|a1|) > acos(|a2|) stated without the acos.
 *   Bins, with pi = 3.141592653589793:
 *       b_theta = clamp(floor((11 * (theta + pi)) / (2 * pi)), 0, 10)
 *       b_alpha = clamp(floor((11 * (alpha + 1)) * 0.5), 0, 10) + 11
 *       b_phi   = clamp(floor((11 * (phi + 1)) * 0.5), 0, 10) + 22
 *     A NaN feature (finite input gives none) goes to bin 0 of its block.
 *   SPFH: c_b(i), b = 0 .. 32, is the number of neighbours of i whose pair falls into bin b -- integers, at most MI_KNN_MAX_K; each
 *     block of 11 sums to exactly count[i], the degenerate pairs included (they land in bins 5, 16 and 27).  spfh_counts33 receives
 *     them.  As a value s_b(i) = (100.0 * c_b(i)) / count[i], and 0 where count[i] == 0.
 *   FPFH: with j_1 .. j_c the neighbours of i in key order, nearest first, and d2_r the key's fp32 distance promoted to fp64: for
 *     every r with d2_r > 0, and b = 0 .. 32 ascending:  val = s_b(j_r) / d2_r,  F_b += val,  S_(b / 11) += val.  Then
 *     scale_f = S_f != 0 ? 100.0 / S_f : 0  and  fpfh33[33 i + b] = (float)(F_b * scale_(b / 11) + s_b(i)), rounded once.  A point with
 *     count[i] == 0 gets 33 zeros.  Every block of 11 of a point with a neighbour at d2 > 0 sums to 200 (Open3D's normalisation); a
 *     point whose neighbours are all duplicates of it keeps its own SPFH, blocks of 100.
 *   No floating-point atomics anywhere: the same input gives the same bits on every call, whatever ran on the context before.
 *   fpfh33 (n*33), spfh_counts33 (n*33, may be NULL) and count (n, may be NULL) are row-major, one row per point.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name and names the cause and, for a bad point or normal, which
 *     array and which index (the lowest; the cloud is looked at first); NO output has been written -- for a NULL ctx, cloud_xyz,
 *     normals_xyz or fpfh33; n < 1; k outside [1, MI_KNN_MAX_K]; a dist_mode other than the two of mi_knn_search; max_distance_squared
 *     NaN or negative; a non-finite coordinate or normal component, or one above 1e18 in magnitude.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the other calls of this header keep: it works in buffers
 *     of its own.  Synchronous, host in and host out. */
#define MI_FPFH_BINS 11
#define MI_FPFH_DIM  33
int mi_fpfh_features(mi_ctx* ctx,
                     const float* cloud_xyz, const float* normals_xyz, int n,
                     int k, int dist_mode,             /* 1 <= k <= MI_KNN_MAX_K; MI_DIST_CPU_ROUNDING or MI_DIST_FMA */
                     float max_distance_squared,       /* INFINITY: no limit; else neighbours with d2 > this do not exist */
                     float* fpfh33,                    /* n*33 */
                     unsigned char* spfh_counts33,     /* may be NULL; n*33 */
                     int* count);                      /* may be NULL; n: neighbours of point i (<= k) */

/* Where the last mi_fpfh_features of this context spent its host wall time, in ms (measurement hook, tools/fpfh_bench.py).  The stages
 * are those of mi_estimate_normals_times:
 *   out[0] workspace (device allocations)           out[1] upload + AoS -> SoA (normals, cloud)
 *   out[2] input checks, bounding box, read-backs   out[3] cell grid over the cloud
 *   out[4] curve order of the cloud + permute       out[5] the SPFH search kernel plus the FPFH kernel
 *   out[6] download of the results                  out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage, and out[5] is the two
 * launches' own HIP-event time instead of host wall time; mi_profile_get then has the SPFH kernel under MI_KERNEL_NN and the FPFH
 * kernel under MI_KERNEL_MOMENTS). */
#define MI_FPFH_STAGES 8
int mi_fpfh_features_times(mi_ctx* ctx, double out_ms[MI_FPFH_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * Descriptor matching (no reference counterpart): the exact nearest neighbour of every row of one descriptor array among the rows of
 * another, in up to MI_FEATURE_MAX_DIM dimensions -- the step between mi_fpfh_features and mi_ransac_register, which turns the
 * matches into a start (a start without odometry).  Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */

/* idx[i] = the row of target_feat nearest to row i of query_feat, every pair looked at.  Every rule below can be retraced in numpy
 * (tests/match_reference.py does, with the fp32 fmaf emulated exactly).  All arithmetic is fp32, every operation rounded once, fused
 * where fmaf is written; q_i and t_j are rows i and j, b = 0 .. dim - 1 the components.
 *   Dot product:  dot(i, j) = c_dim  with  c_0 = +0,  c_(b+1) = fmaf(q_i[b], t_j[b], c_b),  b ascending.  The product commutes, so
 *     dot(i, j) is the same number whichever side is called the query: both directions of the mutual filter see the same bits.
 *   Norms:  tt(j) is the same chain of t_j with itself, qq(i) that of q_i with itself.
 *   Forward key:  h(i, j) = fmaf(-2.0f, dot(i, j), tt(j));  idx[i] = argmin_j h(i, j), strict <, j ascending: the lowest index wins a
 *     tie.  h orders the targets as |q_i - t_j|^2 does (it is that minus qq(i)) without the cancellation-prone sum qq + tt - 2 dot.
 *   Reverse key, mutual == 1 only:  g(j, i) = fmaf(-2.0f, dot(i, j), qq(i));  rev[j] = argmin_i g(j, i), the lowest i on ties.
 *     idx[i] is kept iff rev[idx[i]] == i, else it becomes -1.
 *   Distance of a kept match:  d2[i] = (float) sum_b ((double)q_i[b] - (double)t_j[b])^2 -- difference, product and sum each rounded
 *     in fp64, b ascending, the sum rounded to fp32 once.  +INFINITY where idx[i] == -1.
 *   Why the chain: it is bit for bit what the fp32-input matrix instructions of gfx950 compute (v_mfma_f32_32x32x2_f32,
 *     v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain onto the accumulator, one rounding per product, nothing wider inside), and it is
 *     what a loop of fmaf on the vector pipe computes.  So the contract does not say which pipe runs it; the library uses the matrix
 *     pipe (32x32x2).  Padding dim with zero components up to the instruction's K changes no bit: fmaf(0, 0, c) = c for
 *     every c but -0, and a chain that starts at +0 is at -0 only after a product that underflowed to -0, where +0 compares and adds
 *     the same (h is never -0: tt(j) >= +0, and an exact zero sum rounds to +0).
 *   Determinism: the minimum over chunks of targets is merged by an integer atomicMin on (key mapped to an order-preserving unsigned,
 *     index); the same input gives the same bits on every call, whatever ran on the context before.  No floating-point atomics.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name; NO output has been written -- for a NULL ctx, query_feat,
 *     target_feat or idx; n < 1 or m < 1, or either above MI_FEATURE_MAX_ROWS; dim outside [1, MI_FEATURE_MAX_DIM]; mutual neither 0
 *     nor 1; a non-finite component or one above 1e15 in magnitude (64 * (1e15)^2 < FLT_MAX: no chain overflows): the message names
 *     the array and the lowest row, query_feat first.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the other calls of this header keep: it works in buffers
 *     of its own.  Synchronous, host in and host out. */
#define MI_FEATURE_MAX_DIM 64
#define MI_FEATURE_MAX_ROWS (1 << 30)
int mi_feature_match(mi_ctx* ctx,
                     const float* query_feat, int n,   /* n*dim, row-major */
                     const float* target_feat, int m,  /* m*dim */
                     int dim,                          /* 1 .. MI_FEATURE_MAX_DIM; FPFH: 33 */
                     int mutual,                       /* 0: every query keeps its match; 1: only reciprocal matches */
                     int* idx,                         /* n: matched target, or -1 */
                     float* d2);                       /* may be NULL; n */

/* Where the last mi_feature_match of this context spent its host wall time, in ms (measurement hook, tools/global_bench.py):
 *   out[0] workspace (device allocations)           out[1] upload of both arrays
 *   out[2] norms, input check, its read-back        out[3], out[4] unused (0)
 *   out[5] the searches (both directions) + finish  out[6] download of the results
 *   out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage; mi_profile_get then has
 * the search launches' own HIP-event time under MI_KERNEL_NN). */
#define MI_MATCH_STAGES 8
int mi_feature_match_times(mi_ctx* ctx, double out_ms[MI_MATCH_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * A pose from correspondences (no reference counterpart): hypothesise and verify over the matches of mi_feature_match -- three draws, a
 * Kabsch solve, a count of the matches it explains, every hypothesis evaluated, the best one refined.  Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */
#define MI_RANSAC_MAX_HYPOTHESES (1 << 22)
#define MI_RANSAC_MAX_REFINE 8
typedef struct mi_ransac_params {
    int   hypotheses;          /* H: 1 .. MI_RANSAC_MAX_HYPOTHESES; every one of them is evaluated (no early exit) */
    unsigned long long seed;
    float max_distance;        /* inlier: |R s + t - t'| <= max_distance; > 0, finite */
    float edge_similarity;     /* in [0, 1); 0 disables the edge check; Open3D's default is 0.9 */
    int   refine_iterations;   /* 0 .. MI_RANSAC_MAX_REFINE: Kabsch over the inliers, recount, repeat */
    int   reserved[8];
} mi_ransac_params;
void mi_ransac_params_default(mi_ransac_params* params);   /* 100000, 0, max_distance 0 (the caller must set it), 0.9f, 2 */

/* Every rule below can be retraced in numpy (tests/ransac_reference.py does).
 *   Correspondences: the pairs (i, idx[i]) with idx[i] >= 0 in ascending i are ranks 0 .. C - 1.
 *   Draws, counter based (hypothesis h needs no state), in unsigned 64-bit arithmetic modulo 2^64:
 *       u_r = mix(seed + 0x9E3779B97F4A7C15 * (3 h + r + 1)),  r = 0, 1, 2,   rank_r = ((u_r >> 32) * C) >> 32
 *       mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31   (the splitmix64 finaliser)
 *     Two equal ranks make the hypothesis invalid.  The triple reported is the three source indices i, in draw order.
 *   Edge check, in fp64 from the fp32 coordinates, for the pairs of draws (0, 1), (1, 2), (0, 2): with d the difference of the two points,
 *     ls2 = (dx*dx + dy*dy) + dz*dz in the source and lt2 likewise in the target; the hypothesis is valid iff ls2 >= e2 * lt2 and
 *     lt2 >= e2 * ls2 for all three, e2 = (double)edge_similarity * (double)edge_similarity.
 *   Pose of a hypothesis that is still valid: fp64 centroids ((p0 + p1) + p2) * (1.0 / 3.0) of source (cb) and target (ca); the
 *     cross-covariance H[r][c] = (float)(((t0_r s0_c + t1_r s1_c) + t2_r s2_c) - 3.0 * ca_r * cb_c), rounded to fp32 as the ICP solve rounds
 *     its moments; the Kabsch rotation K of H by the library's 3 x 3 SVD in IEEE arithmetic (csrc/svd3.hpp, kabsch_rotation), then one
 *     Newton-Schulz step towards the nearest rotation in fp64 from the fp32 entries of K (the sweeps of the SVD do not re-orthonormalise:
 *     |K^T K - I| reaches 45 eps over thousands of hypotheses; |R^T R - I| stays within an eps):
 *     G_ij = (K_0i K_0j + K_1i K_1j) + K_2i K_2j,  M = 1.5 I - 0.5 G,  R_ij = (float)((K_i0 M_0j + K_i1 M_1j) + K_i2 M_2j);
 *     t_i = (float)ca_i - ((R_i0 (float)cb_0 + R_i1 (float)cb_1) + R_i2 (float)cb_2) in fp32.  R9 is column-major as mi_kabsch's.  Three
 *     collinear points (the second singular value of H is 0) or a non-finite pose make the hypothesis invalid.  An invalid hypothesis
 *     reports the identity and counts nothing.
 *   Count, for every correspondence, in fp64 from the fp32 pose:  px = ((R00 x + R01 y) + R02 z) + tx and so on, d = p - t', and the pair is
 *     an inlier iff (dx*dx + dy*dy) + dz*dz <= (double)max_distance * (double)max_distance.  inlier_count is an integer.
 *   Winner: the valid hypothesis with the most inliers, the lowest h among equals (integers only: deterministic).  Without a valid
 *     hypothesis the call returns MI_OK with *valid_hypotheses = 0, *inliers = 0, *best_hypothesis = -1, the identity, rmse = +INFINITY
 *     and an all-zero mask.
 *   Refinement, refine_iterations times while at least 3 inliers remain: mi_kabsch over the current inliers (its fixed-order fp64 moment
 *     sums and solve), then a recount under the new pose.  An iteration that leaves fewer than 3 inliers is not taken, and refinement
 *     stops there.  Refinement goes through mi_kabsch's buffers: a problem loaded by mi_icp_load does NOT survive a call that refines
 *     (it does with refine_iterations = 0, and it survives mi_ransac_hypotheses).
 *   rmse = (float)sqrt(S / inliers), S the fp64 sum of the final inliers' squared distances in a fixed order (rank r to partial sum
 *     r mod 256 in ascending r, the partial sums added pairwise at strides 128, 64 .. 1).  No floating-point atomics anywhere.
 *     A winner with fewer than 3 inliers is not refined: the call returns that hypothesis's own pose, and with *inliers = 0 an all-zero
 *     mask and rmse = +INFINITY (beside *valid_hypotheses > 0 and a pose that is not the identity).
 *   inlier_mask (n, may be NULL): 1 where pair (i, idx[i]) is an inlier of the returned pose.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name; NO output has been written -- for a NULL ctx, src_xyz, tgt_xyz,
 *     idx, params or required output; n < 1 or m < 1; hypotheses, max_distance, edge_similarity or refine_iterations outside the ranges
 *     above; an idx[i] that is >= m or < -1 (the message names the lowest i); fewer than 3 correspondences.  MI_ERR_STATE on a distributed
 *     context.  Synchronous, host in and host out. */
int mi_ransac_register(mi_ctx* ctx, const float* src_xyz, int n, const float* tgt_xyz, int m,
                       const int* idx,                 /* n: src[i] <-> tgt[idx[i]]; -1: no pair (mi_feature_match's output) */
                       const mi_ransac_params* params,
                       float out_R9[9], float out_t3[3],   /* as mi_kabsch: column-major R, t */
                       int* inliers, float* rmse, int* best_hypothesis, int* valid_hypotheses,
                       unsigned char* inlier_mask);    /* may be NULL; n */
/* Test-grade primitive, like mi_plane_system: hypotheses first .. first + count - 1 of the call above (first >= 0, count >= 1,
 * first + count <= params->hypotheses), each with its triple (3 source indices), valid flag, pose (R9 then t3) and inlier count.  Every
 * output may be NULL.  The same checks and errors. */
int mi_ransac_hypotheses(mi_ctx* ctx, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx,
                         const mi_ransac_params* params, int first, int count,
                         int* triples /* 3*count */, unsigned char* valid /* count */, float* pose12 /* 12*count */, int* inlier_count /* count */);
/* Where the last mi_ransac_register of this context spent its host wall time, in ms (measurement hook, tools/global_bench.py):
 *   out[0] workspace (device allocations)           out[1] upload of the correspondences
 *   out[2] the hypotheses kernel                    out[3] the counting kernel
 *   out[4] arg-max, read-back, the winner's flags   out[5] refinement
 *   out[6] unused (0)                               out[7] the whole device part of the call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage). */
#define MI_RANSAC_STAGES 8
int mi_ransac_register_times(mi_ctx* ctx, double out_ms[MI_RANSAC_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * A pose from correspondences, the second method (no reference counterpart): Fast Global Registration (Zhou, Park, Koltun, ECCV 2016;
 * Open3D's registration_fgr_based_on_feature_matching).  Where mi_ransac_register fits three matches at a time and counts, this
 * minimises a Geman-McClure robust objective over ALL the matches by graduated non-convexity: a few dozen Gauss-Newton iterations of O(C)
 * each, no hypothesis budget and no inlier threshold to choose.  The iterations are the pose loop of mi_icp_plane_register: the same rows,
 * the same reduce, solve, update and stop rule, the same state block.  Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */
#define MI_FGR_MAX_TUPLES (1 << 20)
typedef struct mi_fgr_params {
    float max_distance;        /* delta > 0, finite: the annealing stops dividing once mu <= delta^2          no default: the caller sets it */
    float division_factor;     /* > 1, finite                                                                 default 1.4 */
    int   decrease_every;      /* >= 1: mu is divided once every this many applied updates                    default 4 */
    int   max_iterations;      /* >= 0                                                                        default 64 */
    float tuple_scale;         /* in [0, 1); 0: no tuple filter, every match is used once                     default 0.95 */
    int   max_tuples;          /* 1 .. MI_FGR_MAX_TUPLES                                                      default 1000 */
    int   tuple_trials;        /* 1 .. MI_RANSAC_MAX_HYPOTHESES; 0 = min(100 * C, MI_RANSAC_MAX_HYPOTHESES)   default 0 */
    unsigned long long seed;
    float eps_rotation, eps_translation;   /* as mi_plane_params; default 0, 0: the schedule runs to max_iterations */
    int   sync_every, verbose;             /* as mi_plane_params */
    int   reserved[8];
} mi_fgr_params;
void mi_fgr_params_default(mi_fgr_params* params);   /* the defaults above; max_distance 0 (the caller must set it), seed 0 */

/* All arithmetic is fp64 from the caller's fp32 coordinates, every operation rounded once, nothing contracted.  Every rule below can be
 * retraced in numpy (tests/fgr_reference.py does).
 *   1 Matches: the pairs (i, idx[i]) with idx[i] >= 0 in ascending i are ranks 0 .. C - 1, as in mi_ransac_register.
 *   2 Used list.  tuple_scale == 0: the used list is ranks 0 .. C - 1, once each, used = C.  tuple_scale > 0: trial h = 0 .. trials - 1
 *     (trials = tuple_trials, or min(100 * C, MI_RANSAC_MAX_HYPOTHESES) where that is 0) draws three ranks by mi_ransac_register's
 *     generator unchanged -- u_r = mix(seed + 0x9E3779B97F4A7C15 * (3 h + r + 1)), rank_r = ((u_r >> 32) * C) >> 32, the same mix.  Two
 *     equal ranks reject the trial.  So does mi_ransac_register's edge check with e2 = (double)tuple_scale * (double)tuple_scale over the
 *     pairs of draws (0, 1), (1, 2), (0, 2): ls2 >= e2 * lt2 and lt2 >= e2 * ls2 for all three.  The accepted trials are taken in ascending h
 *     and the first max_tuples of them are kept; each kept trial contributes its three matches in draw order.  Duplicates stay: a match
 *     drawn by several kept trials weighs that many times.  used = 3 * kept.  When no trial is accepted the call returns MI_OK with
 *     *used = 0, init_T (or the identity) in out_T, 0 iterations, error 0, MI_STOP_NO_PAIRS and *final_mu = D2.
 *   3 Scale and schedule.  D2 is the larger of the two clouds' squared bounding-box diagonals over ALL n and ALL m points (the library's
 *     range pass: fp32 minima and maxima): per cloud dx = (double)hi_x - (double)lo_x and so on, ((dx*dx + dy*dy) + dz*dz).  delta2 =
 *     (double)max_distance * (double)max_distance.  The linearisation that follows k applied updates uses mu_k: mu = D2, then
 *     floor(k / decrease_every) times in a row "if mu > delta2: mu = mu / (double)division_factor".  The step kernel forms it from the
 *     device's own iteration count, so sync_every moves no bit.  *final_mu = (float)mu of the last linearisation (D2 if there was none).
 *   4 Step, one term per used match in used order.  The pose (R, t) is the fp64 state block AS IT IS -- NOT rounded to fp32, unlike the
 *     move of mi_icp_plane_register.  c0 is the centre of the TARGET's bounding box, 0.5f * (lo + hi) in fp32, as there.  With p the source
 *     and q the target point promoted to fp64:  x_i = ((R_i0*p_x + R_i1*p_y) + R_i2*p_z) + t_i;  r = x - q;  u = x - c0;
 *     d2 = (r_x*r_x + r_y*r_y) + r_z*r_z;  w = mu / (mu + d2);  l = w * w.  The Jacobian's rows over (omega, v):
 *       J_x = (0, u_z, -u_y, 1, 0, 0),  J_y = (-u_z, 0, u_x, 0, 1, 0),  J_z = (u_y, -u_x, 0, 0, 0, 1)
 *     with -u_y and so on exact negations, and the term's entries, every product formed (the zeros and ones included):
 *       H(i, j) = l * ((J_x[i]*J_x[j] + J_y[i]*J_y[j]) + J_z[i]*J_z[j])  for i <= j,   g(i) = l * ((J_x[i]*r_x + J_y[i]*r_y) + J_z[i]*r_z),
 *       e = l * d2 + mu * ((w - 1) * (w - 1))   (the paper's objective with the line process eliminated: sqrt(l) = w),
 *     aux = d2, count = 1.  A term whose x has a non-finite component contributes zeros and count 0.  No finite init_T can cause that
 *     (|x| stays below 1e58); a pose that diverged inside the loop can.
 *   Sums (mi_fgr_system's out_sums), the layout of mi_plane_system: [0, 21) the upper triangle of sum H, row-major; [21, 27) sum g; [27]
 *     sum e; [28] sum d2; [29] the number of terms; [30, 32) 0.  Fixed order, a function of `used` alone: used match s is lane s % 64 of
 *     row s / 64; a row is the tree v += shift-down(v, 32), 16, .. 1 over its 64 lanes (absent lanes hold +0); the rows are added as
 *     mi_plane_system's are (one workgroup up to 1024 rows, 64 slabs first beyond).
 *   5 Solve, update, stop: mi_icp_plane_register's, unchanged -- MI_STOP_NO_PAIRS below 6 terms, the scaled LDL^T with its pivot floor
 *     (MI_STOP_DEGENERATE, the pose of the previous iteration staying), x = (omega, v) solving (sum H) x = -(sum g), R <- dR R,
 *     t <- dR (t - c0) + c0 + v, then MI_STOP_CONVERGED under both eps, then MI_STOP_MAX_ITERATIONS.  A positive eps may stop the loop
 *     BEFORE the schedule has brought mu down to delta2 (a step can be small while mu is still large): both default to 0, which runs the
 *     schedule to max_iterations.  max_iterations = 0 returns init_T with MI_STOP_MAX_ITERATIONS.
 *   6 Outputs.  out_T: the fp64 pose rounded once to fp32, column-major, as mi_icp_plane_register writes it -- it goes straight into the
 *     init_T of that call and its siblings.  *error = (float)(sum e / terms) of the last linearisation, 0 without one.  weights[r] =
 *     (float)l of used match r under the RETURNED fp64 pose and the mu of the last linearisation (one more pass of the step's arithmetic, no
 *     update; 0 for a non-finite x); used_src[r] its source index i.  Both may be NULL; the caller sizes them for the largest `used` the
 *     params allow: C without a filter, else 3 * min(trials, max_tuples).  iterations, error, stop_reason and final_mu may be NULL.
 *   7 Determinism: no floating-point atomics, counter-based draws, an integer compaction: the same input and seed give the same bits on
 *     every call, whatever ran on the context before.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name; NO output has been written -- for a NULL ctx, src_xyz, tgt_xyz,
 *     idx, params, out_T or used; n < 1 or m < 1; a field of params outside the ranges above (eps NaN or negative, sync_every < 0); a
 *     non-finite entry of init_T's rotation block or translation column; an idx[i] that is >= m or < -1 (the message names the lowest i);
 *     fewer than 3 matches; a coordinate that is not finite or above 1e18 in magnitude (the message names the array and the lowest index).
 *     MI_ERR_STATE on a distributed context.  A problem loaded by mi_icp_load survives the call: it works in buffers of its own.
 *     Synchronous, host in and host out. */
int mi_fgr_register(mi_ctx* ctx, const float* src_xyz, int n, const float* tgt_xyz, int m,
                    const int* idx,                    /* n: src[i] <-> tgt[idx[i]]; -1: no pair (mi_feature_match's output) */
                    const mi_fgr_params* params, const float init_T[16] /* may be NULL: identity */,
                    float out_T[16], int* iterations, float* error, int* stop_reason, int* used, float* final_mu,
                    float* weights /* may be NULL; used */, int* used_src /* may be NULL; used */);
/* Test-grade primitive: the used list of the call above (rule 2) -- *used, the source and target indices of every used match in used
 * order (either may be NULL; sized as weights above) and the number of accepted trials before max_tuples cuts (0 without a filter; may
 * be NULL).  The same checks and errors, with used in the place of out_T. */
int mi_fgr_tuples(mi_ctx* ctx, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx, const mi_fgr_params* params,
                  int* used, int* used_src, int* used_tgt, int* accepted_trials);
/* Test-grade primitive, like mi_plane_system: one linearisation (rules 3 and 4) over the used list at the pose T (NULL: the identity, the
 * same bits) with the mu that follows applied_updates (>= 0) updates: the sums, the centre c0 and that mu, unrounded (the last two may be
 * NULL).  Without a used match the sums are 0.  The same checks and errors, with out_sums in the place of out_T. */
int mi_fgr_system(mi_ctx* ctx, const float* src_xyz, int n, const float* tgt_xyz, int m, const int* idx, const mi_fgr_params* params,
                  const float T[16] /* may be NULL */, int applied_updates, double out_sums[32], float out_centre[3], double* mu);
/* Where the last mi_fgr_register or mi_fgr_system of this context spent its host wall time, in ms (measurement hook, tools/fgr_bench.py):
 *   out[0] workspace (device allocations)           out[1] upload (both clouds, the matches, the state)
 *   out[2] range pass, input check, its read-back   out[3] tuple trials, their compaction, its read-back
 *   out[4] gather of the used list                  out[5] the iterations, host reads of the state included
 *   out[6] weights pass and downloads               out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage). */
#define MI_FGR_STAGES 8
int mi_fgr_register_times(mi_ctx* ctx, double out_ms[MI_FGR_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * Registration against a voxel map (no reference counterpart): the Normal Distributions Transform (Biber & Strasser, IROS 2003; Magnusson,
 * 2009), as in PCL's NormalDistributionsTransform (registration against a voxel map).  The fixed side is summarised ONCE as
 * one Gaussian per occupied voxel (mi_ndt_voxels); a scan is then registered against those Gaussians by a direct voxel lookup per point,
 * with no neighbour search: an iteration is O(n) whatever the size of the map, and the basin of convergence is set by the voxel size, so
 * the same call runs coarse to fine.  The optimiser is the Gauss-Newton / reweighted form below -- NOT PCL's full Newton Hessian with the
 * More-Thuente line search.  Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */

/* The constants of the NDT score for a voxel size r and an outlier ratio o, in fp64 on the host (no context), with r and o promoted
 * and every operation rounded:  c1 = 10 (1 - o);  c2 = o / ((r r) r);  d3 = -log(c2);  d1 = -log(c1 + c2) - d3;
 * d2 = -2 log((-log(c1 exp(-0.5) + c2) - d3) / d1).   out = d1, d2, h = -0.5 d2, k = -(d1 d2).
 * MI_ERR_INVALID_ARG (out untouched) for a NULL out, a voxel_size that is not positive and finite, an outlier_ratio outside (0, 1), or
 * values that leave fp64. */
int mi_ndt_constants(float voxel_size, float outlier_ratio, double out[4]);

/* One Gaussian per occupied voxel of a cloud, computed on the device.  Every rule can be retraced in numpy (tests/ndt_reference.py does).
 *   Voxel of a point, output order, count, mean: exactly mi_voxel_downsample's, by the same kernels -- mi_voxel_index's arithmetic with
 *     origin3 (NULL: the per-axis minimum), rows ascending by (cz, cy, cx), a per-axis extent of at most 2^20, the mean the fp64 sum over
 *     the count rounded once to fp32.  out_coord, out_count and out_mean equal that call's out_coord, out_count and out_xyz bit for bit on
 *     the same input; out_origin is the origin used.
 *   Scatter about the fp32 mean promoted back to fp64 (so it can be retraced from the outputs): d = p - mu (one fp64 subtraction per
 *     coordinate), Q_ab = sum d_a d_b (one product and one addition per entry and point), a <= b.  The order of the sum is a function of
 *     the sorted order alone, and there is no floating-point atomic: the same input gives the same bits.  C = Q / (count - 1).
 *   Regularisation (PCL's): lambda_0 <= lambda_1 <= lambda_2 and the unit eigenvectors V (columns) of C by mi_estimate_normals' cyclic
 *     Jacobi iteration in fp64;  lambda_i' = max(lambda_i, eig_ratio lambda_2), eig_ratio promoted;  with x_i = 1 / lambda_i',
 *     M_ab = ((V_a0 x_0) V_b0 + (V_a1 x_1) V_b1) + (V_a2 x_2) V_b2, and C'_ab the same with lambda_i' in the place of x_i -- except that,
 *     as in PCL, C' is C itself where no eigenvalue was raised.  Six entries each (xx, xy, xz, yy, yz, zz), each rounded once to fp32:
 *     out_icov6 = M, out_cov6 = C'.
 *   No distribution: a voxel with count < min_points, or with a lambda_2 that is <= 0 or not finite (identical points), still has its
 *     row; its out_icov6 (and out_cov6) is six zeros, which mi_ndt_register treats as "no Gaussian here".
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name and, for a bad point, names its index (the lowest); NO output
 *     has been written -- for a NULL ctx, xyz, out_coord, out_mean, out_icov6 or out_n; n < 1; a voxel_size that is not positive and
 *     finite; a non-finite origin; min_points < 3; an eig_ratio outside (0, 1]; a non-finite coordinate; a voxel coordinate outside
 *     [-2^30, 2^30); occupied voxels that span more than 2^20 along an axis.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the other calls of this header keep: it works in buffers
 *     of its own.  Synchronous, host in and host out. */
int mi_ndt_voxels(mi_ctx* ctx, const float* xyz, int n, float voxel_size,
                  const float* origin3,            /* may be NULL: the per-axis minimum of the cloud */
                  int min_points,                  /* >= 3; PCL: 6 */
                  float eig_ratio,                 /* in (0, 1]; PCL: 0.01 */
                  int* out_coord,                  /* capacity n*3: (cx, cy, cz) of every row */
                  float* out_mean,                 /* capacity n*3 */
                  float* out_icov6,                /* capacity n*6 */
                  int* out_n,                      /* rows written */
                  int* out_count,                  /* may be NULL; capacity n */
                  float* out_cov6,                 /* may be NULL; capacity n*6 */
                  float out_origin[3]);            /* may be NULL */

typedef struct mi_ndt_params {
    float eps_rotation;           /* converged when |omega| <= this (radians) ...            default 1e-6 */
    float eps_translation;        /* ... and |v| <= this (the clouds' units)                 default 1e-6 */
    int   max_iterations;         /* >= 0; there is no unbounded mode                        default 50   */
    int   neighbourhood;          /* voxels looked up per point: 1, 7 or 27                  default 7    */
    float outlier_ratio;          /* in (0, 1)                                               default 0.55 */
    int   sync_every;             /* iterations enqueued between host reads of the state; 0 = 4; moves no bit */
    int   verbose;
    int   reserved[9];
} mi_ndt_params;
void mi_ndt_params_default(mi_ndt_params* p);

/* Registers the moving cloud `before` (n points) onto nv voxel Gaussians (vox_coord, vox_mean, vox_icov6 as mi_ndt_voxels writes them,
 * with the voxel_size and the origin of that call), on the device.  Every rule below can be retraced in numpy (tests/ndt_reference.py does).
 *   Transform, the pose's rounding to fp32, q, the update, the solve, the stop rules and their order, sync_every, max_iterations = 0:
 *     exactly those of mi_icp_plane_register, by the same code -- q = ((R00*b_x + R01*b_y) + R02*b_z) + t_x in fp32 with the pose rounded
 *     once; x = (omega, v) solving (sum H) x = -(sum g) by the scaled LDL^T with a pivot floor of 1e-10 (MI_STOP_DEGENERATE below it or on
 *     a bad diagonal, the pose staying as it was); R <- dR R, t <- dR (t - c0) + c0 + v; MI_STOP_CONVERGED, then MI_STOP_MAX_ITERATIONS.
 *     MI_STOP_NO_PAIRS fires below 6 terms.
 *   Centre: c0 = 0.5f * (lo + hi) per axis of the bounding box of vox_mean over the rows that have a distribution (0 where none has).
 *   Constants: h and k of mi_ndt_constants(voxel_size, outlier_ratio).
 *   Lookup: the voxel of q is mi_voxel_index(q, origin3, voxel_size), bit for bit; a q that function refuses has no term.  The
 *     neighbourhood is that voxel plus offsets in this fixed order -- 1: none; 7: -x, +x, -y, +y, -z, +z behind the voxel itself; 27: all
 *     (dz, dy, dx) in {-1, 0, 1}^3 ascending, the voxel itself in its place (the 14th).  A voxel that is not listed, or whose six
 *     vox_icov6 entries are all zero, gives no term.
 *   Term of (q, voxel v), every operand promoted to fp64 first and every operation rounded, sums of three formed left to right:
 *       d = q - mu_v;   Md_r = (M_r0 d_x + M_r1 d_y) + M_r2 d_z;   m = (d_x Md_0 + d_y Md_1) + d_z Md_2
 *     an m that is negative or not finite (an indefinite matrix given by the caller) is no term;  e = exp(h m);  w = k e.
 *   Per point, from +0 and in the offsets' order: A += w M_v (six entries, one product and one addition each), b += w Md (three),
 *     E += e.  With P = q - c0 the 21 entries of H are formed from A exactly as mi_icp_gicp_register forms them from M, and the six of g
 *     from b as it forms them from Md: Gauss-Newton on sum -d1 exp(-d2 m / 2) with the weights held fixed within the iteration.
 *   Sums (mi_ndt_system's out_sums), the layout of mi_plane_system: [0, 21) the upper triangle of sum H, row-major; [21, 27) sum g;
 *     [27] sum E; [28] the number of points with at least one term; [29] the number of terms; [30, 32) 0.  The sums are added in a fixed
 *     order that depends on n alone, with no floating-point atomics: the same input gives the same bits on every call, whatever ran on
 *     the context before and whatever sync_every.
 *   Outputs: out_T as mi_icp_plane_register's; *iterations counts the updates applied; *score is sums[27] / sums[29] of the last
 *     linearisation rounded to fp32 -- the mean likelihood per term, in (0, 1], higher is better; 0 without terms; *stop_reason is one
 *     of MI_STOP_CONVERGED, MI_STOP_MAX_ITERATIONS, MI_STOP_NO_PAIRS, MI_STOP_DEGENERATE.  Any of the last three may be NULL.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name and names the cause and, for a bad point or row, which array
 *     and which index (the lowest); NO output has been written -- for a NULL ctx, before_xyz, vox_coord, vox_mean, vox_icov6, origin3,
 *     params or out_T; n < 1 or nv < 1; a voxel_size that is not positive and finite; a non-finite origin; an outlier_ratio outside
 *     (0, 1); a neighbourhood other than 1, 7 or 27; eps_rotation or eps_translation NaN or negative; max_iterations < 0; sync_every < 0;
 *     a non-finite entry of init_T's rotation block or translation column; a non-finite point, mean or vox_icov6 entry, or one above 1e18
 *     in magnitude; a vox_coord coordinate outside [-2^30, 2^30); vox_coord rows that are not strictly ascending by (cz, cy, cx) (the
 *     message names the first row that does not come behind its predecessor; duplicates are such rows); listed voxels that span more
 *     than 2^20 along an axis.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the other calls of this header keep: it works in buffers
 *     of its own; the voxel list is uploaded by every call and not kept.  Synchronous, host in and host out. */
int mi_ndt_register(mi_ctx* ctx, const float* before_xyz, int n,
                    const int* vox_coord, const float* vox_mean, const float* vox_icov6, int nv, float voxel_size, const float origin3[3],
                    const mi_ndt_params* params, const float init_T[16] /* may be NULL: identity */,
                    float out_T[16], int* iterations, float* score, int* stop_reason);

/* One linearisation at a given transform, as mi_plane_system: the sums above at the pose T (NULL: the identity, the same bits), the
 * centre c0, per moving point out_idx[i] -- the row of q_i's own voxel if it is listed with a distribution, else -1 -- and out_terms[i],
 * the point's number of terms.  The same arguments are refused, with out_sums in the place of out_T; out_centre, out_idx and out_terms
 * may be NULL. */
int mi_ndt_system(mi_ctx* ctx, const float* before_xyz, int n,
                  const int* vox_coord, const float* vox_mean, const float* vox_icov6, int nv, float voxel_size, const float origin3[3],
                  const float T[16] /* may be NULL */, int neighbourhood, float outlier_ratio,
                  double out_sums[32], float out_centre[3], int* out_idx /* may be NULL; n */, unsigned char* out_terms /* may be NULL; n */);

/* Where the last mi_ndt_register or mi_ndt_system of this context spent its host wall time, in ms (measurement hook, tools/ndt_bench.py):
 *   out[0] workspace (device allocations)           out[1] upload + AoS -> SoA (voxel list, moving cloud, state)
 *   out[2] input checks, bounding box, read-backs   out[3] the voxels' hash table
 *   out[4] curve order of the moving cloud + permute out[5] the iterations, host reads of the state included
 *   out[6] download of the results                  out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage). */
#define MI_NDT_STAGES 8
int mi_ndt_times(mi_ctx* ctx, double out_ms[MI_NDT_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * The quality of a pose (no reference counterpart): what Open3D's evaluate_registration and get_information_matrix_from_point_clouds
 * and PCL's getFitnessScore give -- the fitness, the inlier RMSE, the correspondence set and the 6 x 6 information matrix a pose-graph
 * edge carries -- behind any of the registrations above, whose `error` means something else in each.  One search launch and the rows
 * reduce of mi_plane_system; single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */
/* Evaluates the pose T of the moving cloud `before` (n points) against the fixed cloud `after` (m points), on the device.  Every rule
 * below can be retraced in numpy (tests/eval_reference.py does).
 *   Transform: T is column-major 4 x 4 like every transform of this library, T[4 * col + row]; only the rotation block and the
 *     translation column are read, as given.  Move: the move of mi_icp_plane_register, by the same code -- every read entry of T is
 *     promoted to fp64 and rounded once to fp32 (the same bits), and with every operation rounded to fp32, in this order,
 *     q_x = ((R00*b_x + R01*b_y) + R02*b_z) + t_x, and likewise q_y and q_z.  A NULL T gives the identity's bits.
 *   Pair, search mode (pair_idx NULL): the pair of moving point i is row i of mi_knn_search(ctx, q, n, after_xyz, m, 1, dist_mode,
 *     max_distance_squared, ...), key for key: the same distance arithmetic on the fp32 differences a_j - q_i, equal distance bits going
 *     to the lower index.  A query without a candidate within the limit has no pair.
 *   Pair, given mode (pair_idx non-NULL, n entries): j = pair_idx[i]; -1 means no pair.  Otherwise d2 is the fp32 squared distance of
 *     q_i and a_j in dist_mode's arithmetic, on the differences a_j - q_i: (dx*dx + dy*dy) + dz*dz for MI_DIST_CPU_ROUNDING,
 *     fma(dz, dz, fma(dy, dy, dx*dx)) for MI_DIST_FMA -- what mi_knn_search computes for that pair.  The pair counts when
 *     d2 <= max_distance_squared and d2 is finite.  No cell grid is built in this mode: it evaluates feature matches (mi_feature_match's
 *     idx) under the pose of mi_ransac_register or mi_fgr_register.
 *   Terms, every operand promoted to fp64 first: a = a_j, d = q - a, and the three rows of G = [ -[a]x | I ],
 *       G0 = (0, a_z, -a_y, 1, 0, 0)      G1 = (-a_z, 0, a_x, 0, 1, 0)      G2 = (a_y, -a_x, 0, 0, 0, 1)
 *     -- Open3D's convention: the fixed point, about the origin, the rotation's entries first.
 *   Sums (out_sums, the layout of mi_plane_system): [0, 21) the upper triangle of Lambda = sum G^T G, row-major, a pair's entry (i, j)
 *     being (G0i*G0j + G1i*G1j) + G2i*G2j; [21, 27) g = sum G^T d, a pair's entry i being (G0i*d_x + G1i*d_y) + G2i*d_z; [27] the sum
 *     of (d_x^2 + d_y^2) + d_z^2; [28] the sum of (double)d2, the pairs' fp32 squared distances; [29] the number of pairs; [30, 32) 0.
 *     So Lambda x = -g is one point-to-point Gauss-Newton step about the origin, x = (omega, v).  The device forms only the products
 *     that are not 0 or 1 whatever the point, with the bits of the expressions above.  The sums are added in a fixed order that depends
 *     on n alone, with no floating-point atomics, and a moving point's place in that order is the same in both modes: the same input
 *     gives the same bits on every call, whatever ran on the context before, and given mode handed search mode's own out_idx repeats
 *     every output of search mode bit for bit.
 *   Outputs: *out_fitness = pairs / n, one fp64 division.  *out_inlier_rmse = sqrt(sums[27] / pairs), one fp64 division and one root,
 *     or 0 with no pair.  out_information (row-major 6 x 6) is the symmetric expansion of sums[0, 21), the same bits, and all zeros with
 *     no pair.  out_idx[i] is the fixed index of moving point i's pair or -1; out_d2[i] the pair's fp32 d2, or +INFINITY where there is
 *     no pair.  out_sums, out_information, out_idx and out_d2 may be NULL.  No pair at all is a valid answer: MI_OK, fitness 0, RMSE 0,
 *     every sum +0.
 *   The search is exact for any pose; the speed is only claimed for a pose that brings the moving cloud within a few cells of the fixed
 *     one, as mi_knn_search says of itself.  A finite max_distance_squared bounds every walk.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name and names the cause and, for a bad point or pair, which
 *     array and which index (the lowest); NO output has been written -- for a NULL ctx, before_xyz, after_xyz, out_fitness or
 *     out_inlier_rmse; n < 1 or m < 1; a dist_mode other than the two of mi_knn_search; max_distance_squared NaN or negative; a
 *     non-finite entry of T's rotation block or translation column; a non-finite coordinate, or one above 1e18 in magnitude; a pair_idx
 *     entry that is neither -1 nor in [0, m) (found on the device, read back with the coordinates' check).
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the searches and the registrations keep: it works in
 *     buffers of its own.
 *   Synchronous, host in and host out. */
int mi_evaluate_registration(mi_ctx* ctx, const float* before_xyz, int n, const float* after_xyz, int m,
                             const float T[16] /* may be NULL: identity */,
                             const int* pair_idx /* may be NULL: search; else n entries, -1 or a fixed index in [0, m) */,
                             int dist_mode, float max_distance_squared, double* out_fitness, double* out_inlier_rmse,
                             double out_sums[32] /* may be NULL */, double out_information[36] /* may be NULL; row-major, symmetric */,
                             int* out_idx /* may be NULL; n */, float* out_d2 /* may be NULL; n */);

/* Where the last mi_evaluate_registration of this context spent its host wall time, in ms (measurement hook, tools/eval_bench.py), laid
 * out as mi_icp_plane_times:
 *   out[0] workspace (device allocations)           out[1] upload + AoS -> SoA (pair_idx, fixed cloud, moving cloud, state)
 *   out[2] input checks, bounding box, read-backs   out[3] cell grid over the fixed cloud (0 with the pairs given)
 *   out[4] curve order of the moving cloud + permute out[5] the step, the rows reduce and the host read of the state
 *   out[6] download of the results                  out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage). */
#define MI_EVAL_STAGES 8
int mi_evaluate_registration_times(mi_ctx* ctx, double out_ms[MI_EVAL_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * Pose-graph optimisation (no reference counterpart): what Open3D's global_optimization does for multiway registration and g2o or
 * GTSAM do for a SLAM back end -- many pairwise poses, each weighted by the information matrix mi_evaluate_registration returns, turned
 * into one consistent set of scan poses.  Levenberg-Marquardt outside, preconditioned conjugate gradients on the block-sparse system
 * inside, everything fp64 and on the device; single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */
typedef struct mi_pose_graph_params {
    int max_iterations;        /* linearisations at most */
    int max_pcg_iterations;    /* conjugate-gradient iterations per solve at most */
    int reference_node;        /* the node that never moves */
    double pcg_tolerance;      /* a solve stops at |r_k|_2 <= pcg_tolerance |g|_2 */
    double relative_decrease;  /* MI_STOP_CONVERGED when an accepted step lowers the cost by this fraction or less */
    double absolute_cost;      /* MI_STOP_CONVERGED when the cost is this or less */
    double lambda0;            /* the damping the outer loop starts with; mi_pose_graph_system's lambda */
    double line_process_mu;    /* > 0: the edges flagged uncertain are weighted by the line process; 0: every weight is 1 */
} mi_pose_graph_params;
/* 50, 200, 0, 1e-8, 1e-9, 0, 1e-6, 0 */
void mi_pose_graph_default_params(mi_pose_graph_params* p);

/* Optimises the poses of a graph of V nodes and E edges.  Every rule below can be retraced in numpy (tests/pose_graph_reference.py does).
 *   Graph: node k has a pose T_k = (R_k, t_k), scan frame to world, column-major 4 x 4 like every transform of this library,
 *     T[4 * col + row]; only the rotation block and the translation column are read.  Edge e = (s, t) = (edge_source[e], edge_target[e])
 *     has a measurement Z_e (edge_T, the same layout) that aligns the source scan to the target scan -- exactly the T of
 *     mi_evaluate_registration(before = source, after = target, T) -- and an information matrix Lambda_e, row-major 6 x 6 with the
 *     rotation first: that call's out_information.  Only its upper triangle is read.
 *   Error of an edge: E_e = T_t^-1 T_s Z_e^-1.  Z_e is inverted in the edge kernel, from the measurement as given.
 *   Residual: r_e = (omega, v), omega = log_SO3(R_E) -- half the antisymmetric part s of R_E, scaled by theta / |s| with
 *     theta = atan2(|s|, (trace - 1) / 2); below |s| = 1e-8, s itself -- and v = t_E (not the SE(3) logarithm's translation).  The left
 *     error in the target's frame: the perturbation mi_evaluate_registration's Lambda weights.
 *   Update of a node: T_k <- exp(delta_k) T_k, delta = (omega, v): R <- dR R, t <- dR t + v with Rodrigues' dR of
 *     mi_icp_plane_register (centre 0).  A node whose step is all zeros keeps its pose's bits.
 *   Jacobians (the Gauss-Newton approximation, stated and not refined): d r_e / d delta_s = A_e = Ad(T_t^-1) =
 *     [[R_t^T, 0], [[t']x R_t^T, R_t^T]], t' = -R_t^T t_t, and d r_e / d delta_t = -A_e.
 *   Terms: chi2_e = r_e^T Lambda_e r_e; M_e = w_e A_e^T Lambda_e A_e (symmetric, its upper triangle's 21 numbers row-major);
 *     h_e = w_e A_e^T Lambda_e r_e.  H_ss += M_e, H_tt += M_e, H_st = H_ts^T -= M_e, g_s += h_e, g_t -= h_e: a graph Laplacian with
 *     6 x 6 block weights, (H p)_s += M_e (p_s - p_t), (H p)_t -= M_e (p_s - p_t).
 *   Line process (switchable loop closures as Geman-McClure): an edge with edge_uncertain[e] != 0, under mu = line_process_mu > 0,
 *     has w_e = (mu / (mu + chi2_e))^2 and the share mu chi2_e / (mu + chi2_e) of the cost F; every other edge w_e = 1 and the share
 *     chi2_e.  Weights are recomputed at every linearisation; the final ones are an output, and the caller prunes the edges whose
 *     weight is below its own threshold (0.25 in Open3D).
 *   Gauge: reference_node never moves; its rows and columns are left out (p_ref = 0).  A node without edges keeps its pose.  A
 *     component without the reference node is determined only up to a common motion; the damping keeps the system solvable.
 *   Sums: a node's diagonal block, gradient and row of H p are sums over its incidence list, ascending in the edge index, an edge's
 *     source side before its target side: 64 partial sums over the entries l, l + 64, ... each, added from l = 0 on (for a list of at
 *     most 64 entries: the list's own order).  Lists above 64 entries are summed by one wave, shorter ones by one lane, to the same bits.
 *     Every dot product, norm and cost is summed in a fixed order that depends on V or E alone.  No floating-point atomics: the same
 *     input gives the same bits on every call, whatever ran on the context before.
 *   Inner solve: (H + lambda diag(H)) x = -g by preconditioned conjugate gradients from x = 0.  The preconditioner is, per node, the
 *     inverse of the damped 6 x 6 diagonal block, applied by mi_icp_plane_register's scaled LDL^T afresh at every use (no inverse is
 *     stored); a block that solve calls degenerate is preconditioned by the identity.  It stops at |r_k|_2 <= pcg_tolerance |g|_2 or at
 *     max_pcg_iterations; the step reached at the cap is still tried.  alpha, beta, the norms and the done flag live on the device;
 *     the host reads them every 16 iterations and once per solve, never per iteration.
 *   Outer loop (Levenberg-Marquardt, Marquardt's scaling): linearise, F = the cost; F <= absolute_cost returns the input poses with
 *     MI_STOP_CONVERGED.  lambda = lambda0.  Solve, form the candidate poses and their cost F_new on the device.  F_new < F: accept,
 *     lambda <- max(lambda / 10, 1e-12); then MI_STOP_CONVERGED when (F - F_new) / F <= relative_decrease or F_new <= absolute_cost,
 *     MI_STOP_MAX_ITERATIONS when max_iterations linearisations have been made, else linearise again.  Otherwise lambda <- 10 lambda
 *     and the solve is repeated on the same linearisation; eight rejections in a row stop with MI_STOP_ERROR_INCREASED.
 *   Outputs: out_poses in the layout of poses, every entry outside the rotation block and the translation column copied from poses;
 *     out_weights[e] and out_chi2[e] at the returned poses; out_report = initial cost, final cost, linearisations, accepted steps,
 *     conjugate-gradient iterations in total, final lambda, stop reason, the last solve's |r|_2 / |g|_2.  E = 0 returns the poses as given.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name and names the array and the lowest offending index; NO output
 *     has been written -- for a NULL ctx, poses, params, out_poses or out_report, or NULL edge arrays with E > 0; V < 1 or E < 0;
 *     reference_node outside [0, V); an edge endpoint outside [0, V) or source == target; a non-finite entry of a pose, a measurement
 *     or an information matrix (upper triangle); a rotation block with max |R^T R - I| > 1e-3; a negative diagonal entry of an
 *     information matrix; pcg_tolerance, relative_decrease, absolute_cost or line_process_mu NaN or negative; lambda0 <= 0 or NaN.
 *     E >= 2^30 is refused too (V < 2^31 by its type).
 *   MI_ERR_STATE on a distributed context.  A problem loaded by mi_icp_load survives the call: it works in buffers of its own.
 *   Synchronous, host in and host out. */
int mi_pose_graph_optimize(mi_ctx* ctx, const double* poses /* V x 16 */, int V,
                           const int* edge_source, const int* edge_target, const double* edge_T /* E x 16 */,
                           const double* edge_information /* E x 36 */, const unsigned char* edge_uncertain /* may be NULL; E */, int E,
                           const mi_pose_graph_params* params, double* out_poses /* V x 16 */,
                           double* out_weights /* may be NULL; E */, double* out_chi2 /* may be NULL; E */, double out_report[8]);

/* One linearisation at the given poses with lambda = params->lambda0, stage by stage (the counterpart of mi_plane_system): per edge
 * out_r (E x 6), out_chi2 (E), out_w (E), out_M (E x 21) and out_h (E x 6); per node out_diag (V x 21, the upper triangle of the
 * diagonal block) and out_g (V x 6); for the caller's p (V x 6, may be NULL; the reference node's row is taken as 0) out_Hp (V x 6) =
 * (H + lambda diag H) p with the reference node's row 0; with solve != 0 the inner solve's step out_x (V x 6) and its
 * out_pcg[2] = iterations, |r|_2 / |g|_2.  Every output may be NULL; *out_cost (may be NULL) is F.  Same checks, same refusals. */
int mi_pose_graph_system(mi_ctx* ctx, const double* poses, int V, const int* edge_source, const int* edge_target, const double* edge_T,
                         const double* edge_information, const unsigned char* edge_uncertain, int E, const mi_pose_graph_params* params,
                         const double* p, int solve, double* out_r, double* out_chi2, double* out_w, double* out_M, double* out_h,
                         double* out_diag, double* out_g, double* out_Hp, double* out_x, double* out_pcg, double* out_cost);

/* Where the last mi_pose_graph_optimize or mi_pose_graph_system of this context spent its host wall time, in ms (measurement hook,
 * tools/pose_graph_bench.py):
 *   out[0] workspace (device allocations)           out[1] input checks on the host, AoS -> SoA, upload
 *   out[2] incidence lists (sort, offsets)          out[3] linearisations (edge terms, node gather, the cost's read-back)
 *   out[4] inner solves, host reads included        out[5] candidate poses and their cost
 *   out[6] download of the results                  out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage). */
#define MI_POSE_GRAPH_STAGES 8
int mi_pose_graph_times(mi_ctx* ctx, double out_ms[MI_POSE_GRAPH_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * Place recognition (no reference counterpart): which earlier scan a new scan should be tried against -- the loop-closure candidates the
 * pose graph weighs.  Scan Context (Kim and Kim, IROS 2018): a small polar height map per scan and a comparison that is invariant to
 * a rotation about the up axis, whose best column shift is also a yaw estimate: the init_T of the local registrations (INTEGRATION.md:
 * which tile to try).  The search is exact: every query is compared with every stored descriptor at every shift; no ring key, no pruning.
 * Single-GPU contexts only.
 * -------------------------------------------------------------------------------------------------------------- */
#define MI_SCAN_CONTEXT_MAX_RINGS 32
#define MI_SCAN_CONTEXT_MAX_SECTORS 64
#define MI_SCAN_CONTEXT_MAX_ROWS (1 << 26)
typedef struct mi_scan_context_params {
    int rings;           /* 1 .. MI_SCAN_CONTEXT_MAX_RINGS: equal steps of the planar distance from the centre */
    int sectors;         /* 1 .. MI_SCAN_CONTEXT_MAX_SECTORS: equal steps of the angle about z, counter-clockwise from +x */
    float max_radius;    /* > 0: points at or beyond it in the xy-plane belong to no bin */
    float z_offset;      /* added to every height, so that the ground is positive (the sensor's height above it) */
    int reserved[12];
} mi_scan_context_params;
/* 20, 60, 80, 2 */
void mi_scan_context_params_default(mi_scan_context_params* p);

/* The two tables of the binning, written by the host alone: ring_edge2[rings + 1], the squared ring edges (max_radius r / rings)^2 in
 * fp64, r = 0 .. rings, the last one max_radius^2 itself; sector_dir[2 * sectors], the unit directions (cos, sin)(2 pi j / sectors) of the
 * boundary at which sector j begins, the four axes exact and, for an even number of sectors, direction j + sectors / 2 the exact negative
 * of direction j.  mi_scan_context bins with exactly these doubles, and so does the restatement (tests/scan_context_reference.py), which
 * reads them through this call.  MI_ERR_INVALID_ARG for a NULL argument or params out of range (as below).  Needs no context. */
int mi_scan_context_tables(const mi_scan_context_params* params, double* ring_edge2, double* sector_dir);

/* The descriptors of n_scans scans in one call: desc[n_scans][rings][sectors], fp32.  Scan s is the points [offsets[s], offsets[s + 1]) of
 * xyz (offsets has n_scans + 1 ascending entries from 0; an empty scan is allowed and gives an all-zero descriptor) seen from
 * centres[3 s ..] (the sensor's position; centres NULL: the origin).  z is the up axis: the caller supplies gravity-aligned scans.
 * Every rule below can be retraced in numpy (tests/scan_context_reference.py does, bit for bit).
 *   A bin holds the largest z + z_offset -- one fp32 addition -- over the scan's points that fall into it; a bin without points holds +0,
 *     and so does a bin whose largest value is <= 0.
 *   The bin of a point: no transcendental function and no square root stands between a point and its bin.  dx = (double)x - (double)cx,
 *     dy = (double)y - (double)cy, d2 = dx dx + dy dy: two fp64 products and one sum, every operation rounded once, none fused.
 *     Ring: d2 >= ring_edge2[rings] belongs to no bin (a point exactly at max_radius is out); otherwise the ring is the number of inner
 *       edges ring_edge2[1 .. rings - 1] that are <= d2: a point exactly on an edge belongs to the ring outside it.
 *     Sector: the half-plane first -- upper for dy > 0, or dy == 0 and dx > 0; lower for dy < 0, or dy == 0 and dx < 0; the point exactly
 *       at the centre goes to sector 0 (of ring 0).  The upper half-plane holds the boundaries j with 2 j < sectors, the lower one the
 *       others.  The point has passed boundary j = (c_j, s_j) when c_j dy - s_j dx >= 0 (two fp64 products, one difference): a point
 *       exactly on a boundary belongs to the sector that begins there.  With j0 the first boundary of the point's half-plane and p the
 *       number of that half-plane's boundaries it has passed, the sector is j0 - 1 + p (in the upper half-plane boundary 0 is always
 *       passed; in the lower one p = 0 leaves the point in the last sector that began above, which happens for odd `sectors`).
 *   Determinism: the maximum is merged by integer atomics on the fp32 bits (a positive fp32 orders as its bits do); the same input gives
 *     the same bits on every call, and a scan's descriptor does not depend on what else is in the batch.  No floating-point atomics.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name and names the cause and the lowest offending index; NO output
 *     has been written -- for a NULL ctx, xyz, offsets, params or desc; n_scans < 1; offsets[0] != 0 or offsets that descend; rings or
 *     sectors out of range; max_radius or z_offset not finite, or max_radius <= 0; a coordinate of a centre or of a point that is not
 *     finite or above 1e18 in magnitude (checked in this order: offsets, centres, points).
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call, and so does everything the other calls of this header keep: it works in buffers
 *     of its own.  Synchronous, host in and host out. */
int mi_scan_context(mi_ctx* ctx,
                    const float* xyz,          /* offsets[n_scans] * 3 */
                    const int* offsets,        /* n_scans + 1 */
                    int n_scans,
                    const float* centres,      /* may be NULL; n_scans * 3 */
                    const mi_scan_context_params* params,
                    float* desc);              /* n_scans * rings * sectors */

/* The best stored descriptor for every query, every pair looked at, at every shift: idx[i] = the winning row of db_desc, dist[i] its
 * distance, shift[i] in [0, sectors) the column shift at which it was reached.  Both arrays have mi_scan_context's layout,
 * [rows][rings][sectors]; params gives the shape (max_radius and z_offset are checked and otherwise unused).  Query i sees the rows
 * [0, limit[i]) (limit NULL: all nd) -- an online caller passes i - 50 to skip the scans just behind it; limit[i] <= 0 gives idx = -1,
 * dist = +INFINITY, shift = 0.  second_dist (may be NULL) receives the lowest distance among the rows query i sees other than idx[i]
 * (+INFINITY if there is none): the runner-up of a ratio test.  Every rule below can be retraced in numpy (tests/scan_context_reference.py
 * does, with the fp32 fmaf emulated exactly).
 *   Normalised columns: column j of a descriptor is its `rings` values in sector j.  A column whose values are all zero is empty.
 *     Otherwise u_j = column / |column|: the norm is the fp64 square root of the fp64 sum of squares, rings ascending, every product
 *     exact and every sum rounded once; each component is divided in fp64 and rounded to fp32 once.
 *   Cosine: G(j, k) = c_rings with c_0 = +0, c_(r+1) = fmaf(uq_j[r], uc_k[r], c_r), r ascending: all fp32, the bits the fp32-input
 *     matrix instructions produce (see mi_feature_match).  Zero-padding rings to the instruction's K and sectors to its tile changes no
 *     bit of any output: a zero step leaves the chain alone, and no padded column is ever on a diagonal.
 *   Distance at shift s: with P_s the sectors j for which neither column j of the query nor column (j + s) mod sectors of the row is
 *     empty, d_s = (float)(sum_(j in P_s) (1.0 - (double)G(j, (j + s) mod sectors)) / |P_s|): every term, the sum (j ascending, from +0)
 *     and the quotient in fp64, rounded to fp32 once.  P_s empty: d_s = 1.
 *   Winner: the minimum over s, the lowest s on ties; then the minimum over the rows, the lowest row on ties.  Chunks of rows are merged
 *     by an integer atomicMin on (distance mapped to an order-preserving unsigned, row, shift); the same input gives the same bits on
 *     every call.  No floating-point atomics.
 *   Which way the shift turns: sector j is the angle [2 pi j / sectors, 2 pi (j + 1) / sectors) counter-clockwise from +x, so rotating
 *     the QUERY scan about +z through its centre by shift[i] 2 pi / sectors aligns it with scan idx[i] (about that one's centre): the
 *     init_T of a local registration of the query onto the stored scan is that rotation, moved from the query's centre to the stored
 *     one's.  A query that is the stored scan turned counter-clockwise by k sectors comes back with shift = (sectors - k) mod sectors.
 *     The estimate is good to within a sector's width.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with the entry point's name; NO output has been written -- for a NULL ctx, query_desc,
 *     db_desc, params, idx, dist or shift; nq < 1 or nd < 1, or nd above MI_SCAN_CONTEXT_MAX_ROWS; params out of range as for
 *     mi_scan_context; a limit[i] > nd (the lowest i); a negative or non-finite descriptor value: the message names the array and the
 *     lowest row, query_desc first.
 *   MI_ERR_STATE on a distributed context.
 *   A problem loaded by mi_icp_load survives the call: it works in buffers of its own.  Synchronous, host in and host out. */
int mi_scan_context_search(mi_ctx* ctx,
                           const float* query_desc, int nq,   /* nq * rings * sectors */
                           const float* db_desc, int nd,      /* nd * rings * sectors */
                           const int* limit,                  /* may be NULL; nq */
                           const mi_scan_context_params* params,
                           int* idx, float* dist, int* shift, /* nq each */
                           float* second_dist);               /* may be NULL; nq */

/* Where the last mi_scan_context or mi_scan_context_search of this context spent its host wall time, in ms (measurement hook,
 * tools/scan_context_bench.py):
 *   out[0] workspace (device allocations)           out[1] upload (points, offsets, tables; or the two descriptor arrays)
 *   out[2] the search's normalisation, the input check and its read-back (mi_scan_context: 0, its check runs inside the binning kernel)
 *   out[3], out[4] unused (0)                       out[5] the kernels (binning and its check's read-back; or searches + finish)
 *   out[6] download of the results                  out[7] the whole call
 * The parts are attributable only while profiling is enabled (the stream is then drained after every stage; mi_profile_get then has
 * the search launches' own HIP-event time under MI_KERNEL_NN and the binning kernel's under MI_KERNEL_MOMENTS). */
#define MI_SCAN_CONTEXT_STAGES 8
int mi_scan_context_times(mi_ctx* ctx, double out_ms[MI_SCAN_CONTEXT_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * The map: posed scans fused into a sparse truncated signed distance field (TSDF; Curless and Levoy), and its surface read back as points
 * with normals -- the tile and tile_normals of the next mi_icp_plane_register.  Single-GPU contexts, synchronous, host in and host out, in
 * buffers of their own: a problem loaded by mi_icp_load and everything the searches and registrations keep survive both calls.  A map is
 * three arrays of nv rows: coord (cx, cy, cz per row, the voxel of mi_voxel_index with the caller's origin and voxel_size), tsdf in [-1, 1]
 * (the signed distance to the surface in truncations, positive on the sensor's side) and weight > 0 (the samples fused so far), the rows
 * strictly ascending by (cz, cy, cx) as signed integers: the order mi_tsdf_integrate writes, and mi_voxel_downsample's.
 *
 * mi_tsdf_integrate -- every rule, so that it can be retraced in numpy (tests/tsdf_reference.py does):
 *   Ray.  Point p of scan s (scan s holds the points scan_offsets[s] .. scan_offsets[s + 1] - 1) moves by the scan's pose T_s (16 floats,
 *     column-major, sensor to world, as mi_icp_plane_register's out_T; scan_T NULL: identities, through the same arithmetic) in fp32, in
 *     the order of mi_icp_plane_register's move: w = ((R0 p_x + R1 p_y) + R2 p_z) + t per row of R, every operation rounded.  The sensor
 *     position o is the translation column.  Everything behind this is fp64 on promoted operands, every operation rounded once, none
 *     fused: e = w - o; rho = sqrt((e_x^2 + e_y^2) + e_z^2); d = e / rho.  A ray with rho == 0, rho not finite, rho < min_range or
 *     rho > max_range contributes nothing.
 *   Samples.  h = voxel_size / 2; S = floor(truncation / h), refused above MI_TSDF_MAX_HALF_STEPS.  For k = -S .. S ascending the depth is
 *     s_k = rho + k h (one product, one sum); a sample with s_k <= 0 does not exist.  Its position is x_k = o + s_k d, one product and one
 *     sum per coordinate, rounded once to fp32; its voxel is mi_voxel_index(x_k, origin3, voxel_size).  A sample whose voxel is that of
 *     sample k - 1 of the same ray (where that one exists) is dropped: a line meets a convex voxel in one interval, so every voxel is
 *     sampled at most once per ray.  This is fixed-step sampling, not an exact traversal: a voxel the ray only clips at a corner, between
 *     two samples, can be missed.
 *   Value.  The voxel's centre is c = origin + (index + 0.5) voxel_size per axis; sdf = (d_x (w_x - c_x) + d_y (w_y - c_y)) + d_z (w_z - c_z).
 *     A sample with sdf < -truncation is dropped; otherwise its value is f = min(1, sdf / truncation) and its weight 1.
 *   Fusion, per voxel and per call.  F = the fp64 sum of the voxel's f in ascending (scan, point within the scan, k), C = their number.  With
 *     the voxel's stored (D, W) of the input map, or (0, 0): D' = (W D + F) / (W + C) and W' = min(W + C, max_weight), each rounded once to
 *     fp32.  An input voxel that no sample touches passes through with its bits.  No floating-point atomic occurs anywhere: the same input
 *     gives the same bits on every call, whatever ran on the context before.  The cap binds per call, so K scans in one call and K calls
 *     of one scan differ once it binds -- and by the fp32 rounding of (D, W) between calls.
 *   Output.  The union of the input voxels and the touched ones, ascending by (cz, cy, cx).  The capacity protocol is mi_radius_search's, in
 *     the manner of snprintf: *out_nv is always written; the three arrays are written if and only if 0 < *out_nv <= capacity; a short
 *     capacity still returns MI_OK; capacity == 0 (the arrays may be NULL) is a counts-only call.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with "mi_tsdf_integrate" and names the cause and, for a bad element, the array and the
 *     lowest index; NOTHING has been written, *out_nv included -- for: a NULL required argument; K < 1; scan_offsets not starting at 0,
 *     descending, or ending at 0; a coordinate that is not finite or above 1e18 in magnitude; a non-finite pose entry or origin; params
 *     outside what the struct states; S above MI_TSDF_MAX_HALF_STEPS; a voxel coordinate (of a sample or of the input map) outside
 *     [-2^30, 2^30); an occupied extent (input map and samples together) above 2^20 voxels along an axis; an input map that is not strictly
 *     ascending, or holds a weight that is not finite and positive or a value that is not finite and in [-1, 1]; nv_in < 0 or capacity < 0;
 *     capacity > 0 with a NULL output array; rays (2 S + 1) + nv_in >= 2^31.  nv_in == 0 with NULL in_* arrays is the empty map.
 *   MI_ERR_STATE on a distributed context.  A device allocation that fails is MI_ERR_HIP; the context stays usable.
 * -------------------------------------------------------------------------------------------------------------- */
#define MI_TSDF_MAX_HALF_STEPS 16
typedef struct mi_tsdf_params {
    float voxel_size;     /* > 0, finite */
    float truncation;     /* tau; >= voxel_size / 2, finite */
    float min_range;      /* >= 0; default 0 */
    float max_range;      /* > min_range; default INFINITY */
    float max_weight;     /* > 0; default INFINITY (no cap) */
    int   reserved[11];
} mi_tsdf_params;
void mi_tsdf_params_default(mi_tsdf_params* p);   /* voxel_size and truncation 0: the caller must set them */
int mi_tsdf_integrate(mi_ctx* ctx,
                      const float* scans_xyz, const long long* scan_offsets /* K + 1 */, int K,
                      const float* scan_T /* K x 16, sensor to world; NULL: identities */,
                      const float origin3[3], const mi_tsdf_params* params,
                      const int* in_coord, const float* in_tsdf, const float* in_weight, int nv_in /* may be 0 */,
                      int* out_coord, float* out_tsdf, float* out_weight, long long capacity, long long* out_nv);
/* mi_tsdf_extract -- the surface of a map as points with normals.  The map is held to the checks of mi_tsdf_integrate's input map (nv == 0
 * is the empty map: *out_n = 0).  A voxel is OBSERVED when weight >= min_weight (> 0); lookups by coordinate go through a table of packed
 * coordinates, so the map's occupied extent is at most 2^20 voxels along an axis.
 *   Crossing.  For every observed voxel i in row order and for the axis a = x, y, z in that order, with the neighbour j = i + e_a where it is
 *     observed: f0 = tsdf[i] and f1 = tsdf[j] promoted to fp64; there is a crossing when (f0 > 0) != (f1 > 0) and not both |f| >= 1.  Then
 *     r = f0 / (f0 - f1), and the point is the centre of i (origin + (index + 0.5) voxel_size per axis, fp64) with r voxel_size added along
 *     a (one product, one sum), every coordinate rounded once to fp32.
 *   Normal.  The gradient g at a voxel, per axis and in voxels: the central difference (f+ - f-) / 2 where both neighbours are observed, the
 *     one-sided difference (f+ - f, or f - f-) where one is, 0 where none is.  The normal is v = (1 - r) g(i) + r g(j) (two products and a sum
 *     per axis) divided by sqrt((v_x^2 + v_y^2) + v_z^2), rounded once to fp32: it points to the observed side, towards the sensor.  A zero
 *     vector stays (0, 0, 0), which mi_icp_plane_register reads as "no pair here".
 *   Output.  By row, then axis; 3 floats per crossing in out_xyz and, unless NULL, out_normals.  The capacity protocol is the one above:
 *     *out_n is always written, the arrays if and only if 0 < *out_n <= capacity, capacity == 0 is a counts-only call.
 *   Refusals as above, the message starting with "mi_tsdf_extract"; the map's arrays are called coord, tsdf and weight. */
int mi_tsdf_extract(mi_ctx* ctx, const int* coord, const float* tsdf, const float* weight, int nv,
                    const float origin3[3], float voxel_size, float min_weight /* > 0 */,
                    float* out_xyz, float* out_normals /* may be NULL */, long long capacity, long long* out_n);
/* mi_tsdf_mesh -- the surface of a map as an indexed triangle mesh, by marching cubes over the observed voxels: what a viewer, a mesh file or
 * a collision check takes.  The map is held to every check of mi_tsdf_extract (nv == 0 is the empty map: both counts 0), a voxel is OBSERVED as
 * there, and the vertices are mi_tsdf_extract's crossings with its bits.  Every rule, so that it can be retraced in numpy
 * (tests/tsdf_mesh_reference.py does):
 *   Cube.  The cube at an observed voxel i has the corners c = 0 .. 7 at i + (c & 1, (c >> 1) & 1, (c >> 2) & 1).  Its case is the OR of
 *     1 << c over the corners whose value is > 0: mi_tsdf_extract's sign test.  Edge e = 4 axis + 2 hi + lo runs along `axis` from its owner
 *     corner, whose offset has lo on the lower and hi on the higher of the two other axes: along x (e = 0 .. 3) the owners are (0,0,0),
 *     (0,1,0), (0,0,1), (0,1,1); along y (e = 4 .. 7) (0,0,0), (1,0,0), (0,0,1), (1,0,1); along z (e = 8 .. 11) (0,0,0), (1,0,0), (0,1,0),
 *     (1,1,0).  The vertex on edge e of the cube at i is mi_tsdf_extract's crossing of the voxel i + owner offset along `axis`.
 *   Meshed.  The cube is MESHED when all eight corners are observed and every edge whose ends differ in sign is a crossing by
 *     mi_tsdf_extract's rule (not both |f| >= 1).  Every other cube gives no triangle: the mesh has a hole where the map has one, and at a
 *     saturated step (+1 beside -1), which is the back of the band and no surface.
 *   Table.  256 rows of at most 5 triangles, each three edge numbers (csrc/tsdf_mesh_table.hpp), generated by tools/gen_mc_table.py from
 *     these rules.  Segments: on each of the six faces the edges whose ends differ in sign are two or four; two are joined by one segment,
 *     four by two, each cutting off one positive corner and joining the two face edges that meet at it -- a rule of the face's four signs
 *     alone, so the two cubes on a face agree.  Direction: with n the face's outward normal, m_a and m_b the edge midpoints and p a positive
 *     corner of the face (the one cut off, on a face of four), the segment runs a -> b when n . ((m_b - m_a) x (p - m_a)) > 0: seen from
 *     outside, the positive corner lies to the left.  Every crossed edge then has one successor.  Loops: follow the successors from the
 *     lowest unvisited edge; loops come by their lowest edge.  Fan: rotate the loop to the first start, counted from its lowest edge, for
 *     which no diagonal (r0, rk), 2 <= k <= len - 2, joins two edges of one cube face (the neighbour cube could make the same diagonal
 *     again); the triangles are (r0, rk, rk+1) for k = 1 .. len - 2.  Row 0x01 is (0,8,4); row 0x03 is (4,5,9), (4,9,8).  The geometric
 *     normal (v1 - v0) x (v2 - v0) points to the positive side, towards the sensor, as the vertex normals do.
 *   Output.  Triangles by cube in row order, then in table order, three vertex indices each.  The vertices are the crossings (row, axis) of
 *     mi_tsdf_extract that at least one triangle uses, in its order (by row, then axis), with its bits for coordinates and normals: the
 *     vertex arrays are a subsequence of mi_tsdf_extract's output, each vertex stored once and shared by every triangle round its edge.
 *   Capacity.  *out_nvert and *out_ntri are always written; the three arrays are written if and only if 0 < *out_nvert <= vertex_capacity
 *     and 0 < *out_ntri <= tri_capacity; a short capacity still returns MI_OK; both capacities 0 (the arrays may be NULL) is a counts-only
 *     call.  No floating-point atomic occurs: the same input gives the same bits on every call, whatever ran on the context before.
 *   Refusals.  Every refusal of mi_tsdf_extract, the message starting with "mi_tsdf_mesh"; also a negative capacity, a positive capacity
 *     with a NULL out_xyz (vertex_capacity) or out_tri (tri_capacity), a NULL out_nvert or out_ntri, and 2^31 or more vertices or triangle
 *     indices (3 per triangle).  NOTHING has been written then, the counts included.  MI_ERR_STATE on a distributed context. */
int mi_tsdf_mesh(mi_ctx* ctx, const int* coord, const float* tsdf, const float* weight, int nv,
                 const float origin3[3], float voxel_size, float min_weight /* > 0 */,
                 float* out_xyz, float* out_normals /* may be NULL */, long long vertex_capacity, long long* out_nvert,
                 int* out_tri /* 3 per triangle */, long long tri_capacity, long long* out_ntri);
/* mi_tsdf_raycast -- the map's surface as seen from a pose: one depth, one point and one normal per sensor ray, interpolated inside the
 * voxels; the frame-to-model read-out of a TSDF tracker, a depth image, a synthetic LiDAR sweep or an occlusion test, according to the
 * directions the caller gives.  The map is held to the checks of mi_tsdf_integrate's input map and to mi_tsdf_extract's extent (at most
 * 2^20 voxels along an axis); nv == 0 is the empty map: every ray misses.  Every rule, so that it can be retraced in numpy
 * (tests/tsdf_raycast_reference.py does).  Everything behind the fp32 rotation is fp64 on promoted operands, every operation rounded once,
 * none fused; only +, -, *, /, sqrt, floor and comparisons occur.
 *   1 Ray.  The sensor position o is T's translation column (T: 16 floats, column-major, sensor to world; NULL: the identity, through the
 *     same arithmetic).  Ray i's direction in the world is u = (R0 d_x + R1 d_y) + R2 d_z per row of R in fp32, every operation rounded:
 *     mi_tsdf_integrate's move without the translation.  len = sqrt((u_x^2 + u_y^2) + u_z^2), d = u / len.  A ray with len == 0 or len not
 *     finite is a miss.  The directions may have any length; all depths are along the unit direction d.
 *   2 Samples.  h = voxel_size / 2; K = floor((max_range - min_range) / h) + 1, refused above MI_TSDF_RAYCAST_MAX_STEPS.  For k = 0 .. K - 1
 *     the depth is s_k = min_range + k h (one product, one sum), the position x_k = o + s_k d per coordinate (one product, one sum), rounded
 *     once to fp32, and its voxel mi_voxel_index(x_k, origin3, voxel_size), exactly as mi_tsdf_integrate places a sample.  Sample k is
 *     OBSERVED when that voxel is in the map with weight >= min_weight; g_k is then the voxel's value.  A voxel coordinate outside
 *     [-2^30, 2^30), or outside the map's box, is unobserved, not an error.
 *   3 March, over k ascending.  An unobserved sample, or an observed one with g_k > 0, goes on.  At the first observed sample with g_k <= 0
 *     the march ends: as a HIT when k >= 1, sample k - 1 is observed and g_(k-1) > 0; otherwise as a MISS (the surface was met from behind
 *     or out of unobserved space).  A march that runs out of samples is a miss.
 *   4 Refinement, between a = s_(k-1) and b = s_k, by the trilinear field F(s): p = o + s d in fp64 (not rounded to fp32);
 *     q = (p - origin) / voxel_size - 0.5 per axis (three operations); i = floor(q), w = q - i; the eight corner voxels i + {0, 1}^3 have the
 *     values f_xyz.  F is AVAILABLE when every q is in [-2^30, 2^30) and all eight corners are observed; then
 *     c_yz = f_0yz + w_x (f_1yz - f_0yz), c_z = c_0z + w_y (c_1z - c_0z), F = c_0 + w_z (c_1 - c_0).  If F(a) and F(b) are both available and
 *     F(a) > 0 >= F(b), r = F(a) / (F(a) - F(b)); otherwise r = g_(k-1) / (g_(k-1) - g_k), which is always defined and in (0, 1].  The depth
 *     is t = a + r h and the point o + t d per coordinate (one product, one sum), each rounded once to fp32.  (A depth that rounds to 0 in
 *     fp32 makes the ray a miss: the depth is the hit flag.)
 *   5 Normal.  With i the voxel of sample k - 1 and j the voxel of sample k (they differ: their values differ in sign) and the gradient g of
 *     mi_tsdf_extract at each, over the observed neighbours, the normal is mi_tsdf_extract's: v = (1 - r) g(i) + r g(j) with the r of rule
 *     4, divided by its norm, rounded once to fp32.  It points to the observed side, towards the sensor; a zero vector stays (0, 0, 0).
 *   Output.  Row i of out_depth, out_xyz (world) and out_normals (world) belongs to ray i; out_xyz, out_normals and out_hits may each be
 *     NULL.  A miss gets depth 0, point (0, 0, 0) and normal (0, 0, 0); a hit has depth > 0; *out_hits is the number of hits.  No
 *     floating-point atomic occurs: the same input gives the same bits on every call, whatever ran on the context before.
 *   Empty-space skipping.  Rule 3 says an unobserved sample does nothing, so the march leaves out samples it can prove unobserved: where a
 *     sample's voxel lies in a block of 8^3 voxels that holds no observed voxel and has no neighbour block that does, the 14 samples behind
 *     it are stepped over.  The proof needs (3 max|o| + 2 max|origin3| + 3 max_range) / voxel_size <= 2^21; where that fails the
 *     call marches plainly.  visit_every_sample = 1 marches plainly always.  Neither moves a bit of the result.
 *   MI_ERR_INVALID_ARG -- mi_last_error starts with "mi_tsdf_raycast" and names the cause and, for a bad element, the array and the lowest
 *     index; NOTHING has been written -- for: a NULL required argument (ctx, origin3, params, dirs_xyz, out_depth; the map's arrays with
 *     nv > 0); n < 1 or nv < 0; params outside what the struct states; K above MI_TSDF_RAYCAST_MAX_STEPS; a non-finite entry of T or
 *     origin3; a component of dirs_xyz that is not finite or above 1e18 in magnitude; every map refusal of mi_tsdf_extract (the arrays are
 *     called coord, tsdf and weight).  MI_ERR_STATE on a distributed context.  A device allocation that fails is MI_ERR_HIP; the context
 *     stays usable.  A problem loaded by mi_icp_load and everything the searches keep survive the call. */
#define MI_TSDF_RAYCAST_MAX_STEPS 65536
typedef struct mi_tsdf_raycast_params {
    float voxel_size;   /* > 0, finite: the map's */
    float min_weight;   /* > 0: a voxel is OBSERVED when weight >= min_weight; default 1 */
    float min_range;    /* >= 0, finite; default 0 */
    float max_range;    /* > min_range, finite; no default: the caller must set it */
    int   visit_every_sample;  /* 0: default; 1: no empty-space skipping (measurement, tests); moves no bit */
    int   reserved[11];
} mi_tsdf_raycast_params;      /* 64 bytes */
void mi_tsdf_raycast_params_default(mi_tsdf_raycast_params* p);
int mi_tsdf_raycast(mi_ctx* ctx, const int* coord, const float* tsdf, const float* weight, int nv,
                    const float origin3[3], const mi_tsdf_raycast_params* params,
                    const float T[16] /* sensor to world; NULL: identity, same arithmetic */,
                    const float* dirs_xyz /* n x 3, sensor frame, any length */, int n,
                    float* out_depth /* n */, float* out_xyz /* n x 3, world; may be NULL */,
                    float* out_normals /* n x 3, world; may be NULL */, long long* out_hits /* may be NULL */);
/* Where the last mi_tsdf_integrate, mi_tsdf_extract, mi_tsdf_mesh or mi_tsdf_raycast of this context spent its host wall time, in ms:
 *   out[0] workspace (device allocations)   out[1] upload   out[2] checks and read-backs
 *   out[3] sampling (extraction, mesh and ray cast: the table)
 *   out[4] sort and runs (extraction: count + scan; mesh: the cubes' cases, the used crossings and the two scans; ray cast: the block table)
 *   out[5] fusion (extraction: fill; mesh: the vertex fill and the triangle fill; ray cast: the cast)
 *   out[6] download   out[7] the whole call
 * While profiling is enabled the stream is drained after every stage, so the parts are attributable (mi_profile_get then also holds the
 * sampling, crossing and cast launches' own HIP-event time under MI_KERNEL_NN and the fusion kernel's under MI_KERNEL_MOMENTS; of a mesh,
 * the vertex fill under MI_KERNEL_NN and the three launches of its own -- cases, used crossings, triangles -- under MI_KERNEL_MOMENTS). */
#define MI_TSDF_STAGES 8
int mi_tsdf_times(mi_ctx* ctx, double out_ms[MI_TSDF_STAGES]);

/* ----------------------------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py): per-kernel HIP-event timing on the context's own stream.
 * -------------------------------------------------------------------------------------------------------------- */
enum {
    MI_KERNEL_NN = 0,          /* K1 brute-force nearest-neighbour search */
    MI_KERNEL_MOMENTS = 1,     /* K2 fused gather + centroid/cross-covariance partial sums */
    MI_KERNEL_SOLVE = 2,       /* K3 reduce + 3x3 SVD + compose */
    MI_KERNEL_TRANSFORM = 3,   /* K4/K5 transform + error partial sums + key reset */
    MI_KERNEL_FINALIZE = 4,    /* K6 error reduce + stop rule */
    MI_KERNEL_ALLREDUCE = 5,   /* C1 RCCL packed-min all-reduce (multi-GPU) */
    MI_KERNEL_CPD_DENOM = 6,   /* K7a column sums (den, Pt1, L) */
    MI_KERNEL_CPD_CONTRACT = 7,/* K7b P~.[X|1] contraction (MFMA) */
    MI_KERNEL_CPD_MSTEP = 8,   /* K8 weighted moments + solve */
    MI_KERNEL_CPD_FGT = 9,     /* K9 Fast-Gauss-Transform E-step (clustering, model, predict) */
    MI_KERNEL_COUNT = 10
};
int mi_profile_enable(mi_ctx* ctx, int enable);
/* Which kernels get events while profiling is enabled: bit k = MI_KERNEL_k (default: all).  Two event records around every
 * launch of a 5-kernel iteration cost a few per cent of a millisecond-sized step; bench.py times only the search in its timed
 * region and the rest in a separate short run. */
int mi_profile_select(mi_ctx* ctx, unsigned int kernel_mask);
int mi_profile_reset(mi_ctx* ctx);
/* total_ms = sum of event-timed durations of that kernel since the last reset; launches = how many. */
int mi_profile_get(mi_ctx* ctx, int kernel, double* total_ms, long long* launches);
/* Where the last mi_icp_load (or the load inside mi_icp_register) spent its host wall time, in ms -- what the reference's own
 * timing of a whole SlamFunc call includes besides the iterations (testrunner.cpp:54-56, doc/documentation.tex:397):
 *   out[0] workspace (device allocations)          out[1] moving cloud: upload + AoS -> SoA
 *   out[2] moving cloud: Hilbert order + permute    out[3] fixed cloud: upload + AoS -> SoA
 *   out[4] box hierarchy over the fixed cloud       out[5] cell grid over the fixed cloud
 *   out[6] state reset                              out[7] the whole load
 * While profiling is enabled (mi_profile_enable) the stream is drained after every stage, so the parts are attributable (and no
 * longer overlap); otherwise only out[7] is meaningful. */
#define MI_LOAD_STAGES 8
int mi_icp_load_times(mi_ctx* ctx, double out_ms[MI_LOAD_STAGES]);
/* Work counters of the cell-grid search (MI_NN_GRID), summed over its launches while enabled: out[0] candidates tested in the
 * grid, out[1] cell rows scanned, out[2] moving points that went on to the box hierarchy, out[3] moving points searched, out[4]
 * hierarchy nodes and out[5] leaves visited by out[6] walking waves, out[7] nodes + leaves of the longest single walk (a
 * maximum, not a sum).
 * enable != 0 starts counting (and zeroes the counters), 0 stops; out may be NULL.  Costs four atomics per moving point while on. */
int mi_profile_search_stats(mi_ctx* ctx, int enable, unsigned long long out[8]);
/* The same counting build's LOOP TRIP COUNTS since counting was switched on (call it BEFORE mi_profile_search_stats(ctx, 0, ..) switches it off), summed over
 * waves -- what tools/isa_budget.py multiplies the kernel's static per-phase instruction counts by (the measured instruction budget of DESIGN section 4):
 * out[0] waves, [1] waves that ran the grid scan, [2] walk-only waves; of the scanning waves: [3] nearest-block batches, [4] of them with their trips dealt
 * over the wave, [5] deal passes, [6] iterations of the deal's write loop, [7] lockstep trips; [8] rounds of leftover rows dealt out, [9] of them with their
 * trips dealt, [10] deal passes, [11] write-loop iterations, [12] lockstep trips, [13] leftover batches of the four-rows-per-lane form, [14] waves that had
 * leftover rows; of the walking waves: [15] leaves that held a candidate at or below some lane's best, [16] leaf children looked at, [17] votes for the nearest
 * child, [18] pops of a pending child, [19] leaves whose sequential (index-settling) offers ran.  Measurement hook: no reference counterpart. */
int mi_profile_search_phases(mi_ctx* ctx, unsigned long long out[20]);
/* Self-test of the library's own device radix sort (the Hilbert ordering of the index build): sorts the n (key, value) pairs in
 * place, stable, ascending by the low `bits` (10, 20 or 30) of the keys.  Host arrays; test use only. */
int mi_selftest_sort_pairs(mi_ctx* ctx, unsigned int* keys, int* values, int n, int bits);
/* Self-test of the range pass every cloud-taking call opens with (csrc/cloud_range.hpp): per-axis minimum and maximum over the usable points of
 * the n points of xyz (host, AoS) into out_lo_hi (lo xyz, hi xyz; +inf / -inf where no point is usable) and the lowest index of a refused point, or
 * 0x7fffffff, into out_first_bad.  check = 0 refuses nothing (NaN coordinates are ignored), 1 refuses points with a non-finite coordinate (the voxel
 * call's rule), 2 those and coordinates above 1e18 in magnitude (the k-NN call's).  Test use only. */
int mi_selftest_cloud_range(mi_ctx* ctx, const float* xyz, int n, int check, float out_lo_hi[6], int* out_first_bad);
/* Fault injection for the library's own tests: the next n index builds of this context fail with MI_ERR_INVALID_ARG behind the fixed cloud's upload (the
 * early-return path of mi_icp_load).  Only ever by this explicit call -- round 5 read it from the environment, where a stray variable could have failed
 * loads in production.  n = 0 disarms. */
int mi_selftest_fail_loads(mi_ctx* ctx, int n);
/* Device buffers of the library now alive in this process, over all contexts: successful allocations minus frees.  A buffer that was outgrown counts
 * until it is really freed (behind the next drain of its context's stream).  Creating a context, using it and destroying it leaves the count where
 * it was: what the library's own tests check.  Needs no context. */
int mi_selftest_live_buffers(long long* count);
/* The cells per axis of the grid that the last mi_radius_search of this context walked (0, 0, 0 before the first): how a test tells that
 * MISLAM_OUTLIER_RADIUS_CELL or MISLAM_KNN_POINTS_PER_CELL was taken and gave the regime it was meant to give. */
int mi_selftest_radius_grid(mi_ctx* ctx, int dims[3]);
/* What the last ICP step of the loaded problem left on the device besides its result: rows = the moving cloud's 64-point chunks; the first
 * min(cap_rows, rows) entries of the work order dealt for the next search (a permutation of the chunks, walking ones first) and of the chunks' flags
 * (non-zero: its wave walked the box hierarchy); the four range cursors of the dealing (two pairs: a step deals on the pair of its parity and leaves the
 * other pair zero); the arrival ticket of the rows reduction whose last workgroup solves (zero between launches); and the 16 moments and 2 error sums the
 * last solve read.  order / far may be NULL when cap_rows is 0.  Test use only. */
int mi_selftest_icp_schedule(mi_ctx* ctx, int cap_rows, int* order, unsigned char* far, int* rows, int cursors[4], int* ticket, double sums[18]);
/* What the last mi_cpd_register / mi_cpd_mstep on this context left in the CPD workspace, copied out: the arrays of its last E-step (p1[m], pt1[n],
 * px[3m] row-major -- for mi_cpd_mstep the caller's own), the moving cloud as the last transform left it (y_xyz[3m]; mi_cpd_mstep transforms nothing:
 * the cloud as loaded), and from the state block the call's last host read brought back: the M-step's moments xs[5] = { sum log den, sum pt1 a (3),
 * sum pt1 |a|^2 } and ks[14] = { Np, sum p1 b (3), sum b_r px_c (9, row-major in r), sum p1 |b|^2 } as the last solve read them, R9 (column-major), t3, scale,
 * sigma2, sigma2_init, constant.  info[8] = { MI_CPD_ROUTE_* of the last E-step (-1: none ran, mi_cpd_mstep), 1 if the M-step summed the rows the
 * E-step's own kernels left (0: the stand-alone sums kernels ran), rows of x-sums, rows of k-sums it summed, 1 if the moments went through the state
 * block (a distributed context's reduce + all-reduce), iterations, stop reason, 0 }.  Every output pointer may be NULL.  m, n: the sizes of that call
 * (n: this rank's share of the fixed cloud).  MI_ERR_STATE when the last entry point called on the context was not one of the two (any call in between
 * may have reused the buffers; the read-back itself may be repeated) or when m / n are not the loaded sizes.  Launches no kernel and changes nothing
 * a later call reads.  Test use only. */
enum {
    MI_CPD_ROUTE_EXACT_MFMA = 0,        /* exact P, matrix-pipe contraction */
    MI_CPD_ROUTE_EXACT_VALU = 1,        /* exact P, vector-pipe contraction (MISLAM_CPD_MFMA=0) */
    MI_CPD_ROUTE_SEQUENTIAL = 2,        /* MI_ESTEP_CPU_SEQUENTIAL */
    MI_CPD_ROUTE_TRUNC_CULLED = 3,      /* hybrid mode's truncated E-step, culled by tile boxes */
    MI_CPD_ROUTE_TRUNC_EVERY_PAIR = 4,  /* ... every pair (MISLAM_CPD_TRUNC_CULL=0) */
    MI_CPD_ROUTE_FGT = 5                /* Fast Gauss Transform */
};
int mi_selftest_cpd_last(mi_ctx* ctx, int m, int n, float* p1, float* pt1, float* px, float* y_xyz, double xs[5], double ks[14], float R9[9],
                         float t3[3], float* scale, float* sigma2, float* sigma2_init, float* constant, int info[8]);
/* The moments stage and the candidates of mi_nicp_register without its driver loop: the same uploads, the same moments and reduce launches and the
 * same host solve per repetition, no search and no pick.  raw_sums receives the 32 fp64 sums as the device left them, every point taken about the
 * FIRST point of its cloud (b_i - b_0, a_i - a_0, exact in fp64): 0-2 sum b, 3-8 sum b b^T (xx xy xz yy yz zz), 9-11 sum a, 12-17 sum a a^T, and over
 * the pairs i < min(m, n) 18-20 sum a_i, 21 sum |a_i|^2, 22-30 sum a_i b_i^T (row-major in a); 31 is spare and 0.  R9_t3_approx receives 13 floats
 * per repetition: the candidate's R (ROW-major), t and approximated error, for order_heads[3 r .. 3 r + 2] as in mi_nicp_register.  Sizes and heads
 * are checked as there (m > n is allowed, as in MI_CPD_APPROX_NONE, the one mode that reads no approximated error: for m > n that output is
 * not defined); a refused call leaves its outputs untouched.  Like the registration it reuses
 * the context's cloud buffers, so no ICP problem stays loaded behind it; it keeps no state of its own.  Test use only. */
int mi_selftest_nicp_candidates(mi_ctx* ctx, const float* before_xyz, int m_before, const float* after_xyz, int n_after, const int* order_heads,
                                int reps, double raw_sums[32], float* R9_t3_approx);
/* Name of the correspondence-search kernel (MI_KERNEL_NN) a search of n_moving points against m_fixed_local fixed points runs
 * with this nn_mode and the current settings -- the name a rocprofv3 kernel trace shows (static string). */
const char* mi_nn_kernel_name(const mi_ctx* ctx, int n_moving, int m_fixed_local, int nn_mode);

#ifdef __cplusplus
}
#endif
#endif /* MI_SLAM_H */
