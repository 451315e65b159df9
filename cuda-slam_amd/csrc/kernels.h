// Internal launch interfaces between the C-ABI/driver layer (mislam_api.hip, nn_api.hip, icp_api.hip) and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pose_block.hpp"
#include "voxel_table.hpp"

namespace mislam {

// ---------------------------------------------------------------------------------------------------------------
// K1 nearest-neighbour search (nn_kernel.hip)
// ---------------------------------------------------------------------------------------------------------------
constexpr int NN_TARGET_BLOCK = 16;       // T: targets per min-only block of K1 (chunk_len and target padding granule)
constexpr int NN_MAX_R = 8;               // sources per lane
constexpr int NN_SRC_PAD = 256 * NN_MAX_R;  // source arrays are padded to a multiple of this
constexpr unsigned long long KEY_INIT = 0xFFFFFFFFFFFFFFFFull;

struct NnLaunch {
    const float *sx, *sy, *sz;            // sources, SoA, n_pad floats each (n_pad % (256*R) == 0)
    int n, n_pad;
    const float *tx, *ty, *tz;            // targets, SoA, >= n_chunks*chunk_len floats each
    int chunk_len, n_chunks;              // chunk_len % NN_TARGET_BLOCK == 0
    int index_base;                       // global index of target 0 of this device's shard
    unsigned long long* keys;             // n packed (d2 bits << 32 | index) keys: KEY_INIT or a REAL candidate's key
    const int* done_flag;                 // device-side stop flag (may be null)
    int R;                                // 1, 2, 4 or 8
    int fma;
};
hipError_t nn_launch(const NnLaunch& a, hipStream_t stream);

// ---------------------------------------------------------------------------------------------------------------
// ICP iteration kernels (icp_kernels.hip)
// ---------------------------------------------------------------------------------------------------------------
constexpr int ICP_MOMENTS = 16;              // count, sum b (3), sum a (3), sum a b^T (9)
constexpr int ICP_ERRSUMS = 2;               // sum |a - b'|^2, kept pairs
constexpr int ICP_REDUCED_ROWS = 64;          // rows icp_rows_reduce leaves at most (= ICP_MAX_REDUCED_ROWS of icp_rows.hpp): one per lane of the solve kernel
constexpr int ICP_MAX_PARTIAL_BLOCKS = 512;   // 2 blocks per CU: enough loads in flight for the O(N) passes, few rows to reduce

// mirror of the public MI_STOP_* values (mi_slam.h) for device code
enum { MI_STOP_RUNNING_ = 0, MI_STOP_CONVERGED_ = 1, MI_STOP_MAX_ITERATIONS_ = 2, MI_STOP_NO_PAIRS_ = 3,
       MI_STOP_ERROR_INCREASED_ = 4, MI_STOP_TOLERANCE_ = 5, MI_STOP_SIGMA_ = 6 };

// Device-resident loop state.  The host only ever copies it back; every decision is taken on the device.
struct IcpState {
    float R[9];              // running rotation, column-major (glm::mat3)
    float t[3];              // running translation
    float prevR[9];
    float prevT[3];
    float Ri[9];             // last per-iteration solve
    float ti[3];
    float error;             // *error of the reference drivers
    float prev_error;
    int iterations;          // *iterations of the reference drivers
    int passes;              // loop bodies executed
    int done;
    int stop_reason;
    int pairs;               // correspondences kept in the last solve (this rank's share in the multi-GPU path)
    int err_pending;         // multi-GPU: err[] holds the last iteration's sums and its stop rule has not been evaluated yet
    double mom[ICP_MOMENTS];
    double err[ICP_ERRSUMS];
    // MI_SUM_CPU_SEQUENTIAL only: cpu-slam's own sequential fp32 running sums over the kept pairs in the caller's order
    float seq_sum_b[3];      // sum of the moving points        (GetCenterOfMass, common.cpp:281-284)
    float seq_sum_a[3];      // sum of their matched fixed points
    float seq_sum_err;       // sum of squared residuals         (GetMeanSquaredError, common.cpp:259-268)
    float seq_H[9];          // cpu-slam's cross-covariance of the kept pairs: sum fl32(a - ca) fl32(b - cb)^T with ITS centroids (round 6, icp_seq_cross_kernel)
};

struct IcpView {
    IcpState* state;
    const float *bx, *by, *bz;       // original `before`, SoA, n_pad
    float *cx, *cy, *cz;             // current (transformed) cloud, SoA, n_pad
    const float4* tgt4;              // this rank's target shard as float4 (gather-friendly), local index
    unsigned long long* keys;        // n packed keys
    int n, n_pad;
    int shard_lo, shard_hi;          // global target index range owned by this rank
    int filter_pairs;
    float max_distance_squared;
    int fma;                         // distance arithmetic used when re-arming keys with the previous match
    const int* inv_order;            // caller's index -> sorted slot (MI_SUM_CPU_SEQUENTIAL), else null
    float* resid;                    // per sorted slot: squared residual of the kept pair, +0 otherwise (same mode), else null
};

struct IcpRules {
    float eps;
    int max_iterations;
    int filter_pairs;
    int abort_on_increase;
    int m_total;                     // |after| over all ranks
    int seq_sums;                    // MI_SUM_CPU_SEQUENTIAL: the error comes from state->seq_sum_err
    int svd_ieee;                    // developer switch MISLAM_SVD_IEEE=1: K3 in IEEE divisions and roots instead of the refined hardware forms
};

constexpr int ICP_CHUNK_POINTS = 64;          // moving points per wave / per row of partial sums (icp_rows.hpp ICP_ROW_POINTS)
// stable LSD radix sort of (key, value) pairs on the low `bits` of the keys (radix_sort.hip); the *_in arrays are scratch afterwards
size_t radix_sort_temp_bytes(int n);
hipError_t radix_sort_pairs_u32(void* temp, unsigned int* keys_in, unsigned int* keys_out, int* vals_in, int* vals_out, int n, int bits,
                                hipStream_t s);
hipError_t fill_keys(unsigned long long* keys, int n, hipStream_t s);
// dst[i] (i < n_local) = the i-th point of the 64-point chunks rank, rank + world, rank + 2*world ... of src (n_all points); entries
// [n_local, n_pad) replicate the last one
hipError_t deal_chunks_soa(const float* sx, const float* sy, const float* sz, int n_all, int rank, int world, int n_local, int n_pad,
                           float* dx, float* dy, float* dz, hipStream_t s);
hipError_t aos_to_soa(const float* aos, int n, int n_pad, float* x, float* y, float* z, float4* packed, hipStream_t s);
hipError_t soa_to_aos(const float* x, const float* y, const float* z, int n, float* aos, hipStream_t s);
hipError_t unpack_keys(const unsigned long long* keys, const int* order, int n, int* idx, float* d2, hipStream_t s);
hipError_t pack_keys(const int* idx, const unsigned char* keep, int n, unsigned long long* keys, hipStream_t s);

int icp_reduce_blocks(int n);
// An iteration's sums are "rows" (icp_rows.hpp): one row of 18 partial sums -- 16 moments, 2 error sums -- per 64 moving points,
// whichever kernel produced them (the fused search of nn_grid.hip, or the two stand-alone kernels below).
int icp_row_count(int n);                  // rows of a cloud of n points
int icp_reduced_count(int nrows);          // rows left after icp_rows_reduce (<= 64)
hipError_t icp_moments_rows(const IcpView& v, double* rows, hipStream_t s);                    // K2: columns [0,16) of rows [0, row_count(n))
// K4+K5: cur = R*before + t for all n_pad entries, columns [16,18) of rows [0, row_count(n_pad)), keys re-armed:
// rearm 0 = leave keys, 1 = KEY_INIT, 2 = the previous match's key under the NEW transform (a real candidate: the next search
// starts from a tight bound)
hipError_t icp_transform_error_rows(const IcpView& v, double* rows, int rearm, hipStream_t s);
// Work order of the fused search (nn_grid.hip): order[position] = chunk; the rows-reduce kernel rewrites it every iteration from
// the flags the search left (far[chunk] != 0: its wave walked the box hierarchy), walking chunks first.  Scheduling only.
struct IcpSchedule {
    int* order;                            // nrows entries, always a permutation of the chunks
    unsigned char* far;                    // nrows flags
    unsigned long long* lanes;             // nrows lane masks (GridSearchArgs::far_lanes)
    int* counters;                         // ICP_SCHED_CURSORS cursors: two pairs, a step deals on the pair of its parity; zeroed by the solve
    int* ticket;                           // arrivals of icp_rows_reduce_solve's summing workgroups; 0 between launches
};
constexpr int ICP_SCHED_CURSORS = 4;
hipError_t icp_schedule_reset(const IcpSchedule& sched, int nrows, hipStream_t s);             // identity order, no flags
hipError_t icp_rows_reduce(const double* rows, int nrows, double* part, hipStream_t s, const IcpSchedule* sched = nullptr, bool all_rows = false,
                           int parity = 0);   // -> part[icp_reduced_count(nrows)][18]
// the same launch with icp_solve_deferred behind it: the summing workgroup that arrives last (by `ticket`) solves.  One rank, part != null.
hipError_t icp_rows_reduce_solve(IcpState* state, const double* rows, int nrows, double* part, const IcpSchedule* sched, int parity, int* ticket,
                                 int compose_mode, const IcpRules& rules, int mark_pending, hipStream_t s);
constexpr int ICP_FUSED_SOLVE_MAX_ROWS = 2048;      // up to this many rows (131 072 moving points) rows reduce + solve are one launch of one workgroup
hipError_t icp_reduce_solve(IcpState* state, const double* rows, int nrows, int compose_mode, const IcpRules& rules, int mark_pending, hipStream_t s);
// reduced rows -> state->mom / state->err (which: 1 moments, 2 error sums, 3 both); the multi-GPU paths all-reduce them there
hipError_t icp_rows_to_state(IcpState* state, const double* part, int count, int which, hipStream_t s);
// K3 + K6, deferred: settles the PREVIOUS iteration's stop rule from the error sums (if state->err_pending), then -- unless it
// fired -- solves from the moments and composes.  part != null: sums = the reduced rows; null: already in state->mom / err.
// mark_pending: this iteration's own error will arrive with the next call (or with icp_finalize_pending).
hipError_t icp_solve_deferred(IcpState* state, const double* part, int count, int compose_mode, const IcpRules& rules, int mark_pending,
                              hipStream_t s, int* sched_counters = nullptr);
hipError_t icp_finalize_pending(IcpState* state, const double* part, int count, const IcpRules& rules, hipStream_t s);
hipError_t icp_mark_pending(IcpState* state, hipStream_t s);
// MI_SUM_CPU_SEQUENTIAL: cpu-slam's sequential fp32 running sums, reproduced bit for bit (one wave per sum)
hipError_t invert_order(const int* order, int n, int* inv, hipStream_t s);
hipError_t icp_seq_centroids(const IcpView& v, hipStream_t s);
hipError_t icp_seq_error(const IcpView& v, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K-batch: many small registrations, one workgroup per problem, the iterations inside the kernel (icp_batch.hip)
// ---------------------------------------------------------------------------------------------------------------
constexpr int ICP_BATCH_MAX_MOVING = 4096;    // moving points a workgroup carries in registers: 8 waves x 8 rows of 64 (mi_icp_batch_route)
constexpr int ICP_BATCH_MAX_FIXED = 4096;     // fixed points: streamed through LDS in tiles, so a routing choice rather than a limit of the kernel
struct IcpBatchProblem {
    int b_off, n;                    // moving cloud: first point in `before`, count
    int a_off, m;                    // fixed cloud: first point in `after`, count
    int s_off;                       // first slot of the problem's sorted moving cloud in sx / sy / sz
    int pad;
};
struct IcpBatchArgs {
    const float* before;             // AoS xyz, as uploaded
    const float* after;
    const IcpBatchProblem* problems;
    float *sx, *sy, *sz;             // every problem's moving cloud in its curve order, SoA
    IcpState* states;                // one block per problem
    int* running;                    // += 1 per problem still running when a launch ends (zeroed by the host before it)
    int n_problems;
    int iters;                       // loop bodies per problem and launch, at most
    int compose_mode;
    float max_distance_squared;
    IcpRules rules;                  // m_total is the problem's own (set in the kernel)
};
hipError_t icp_batch_prepare(const IcpBatchArgs& a, hipStream_t s);            // sorted clouds + states at identity
hipError_t icp_batch_iterate(const IcpBatchArgs& a, int fma, hipStream_t s);   // up to a.iters iterations of every running problem

// ---------------------------------------------------------------------------------------------------------------
// Voxel-grid centroids of a cloud (voxel_kernels.hip; driver: voxel_api.hip)
// ---------------------------------------------------------------------------------------------------------------
// The voxel of a coordinate: floorf((p - o) / v) with one IEEE subtraction and one IEEE division, the same instructions' worth of
// arithmetic on the host (mi_voxel_index) and in the kernels.  false: the quotient is not finite or outside [-2^30, 2^30).
__host__ __device__ __forceinline__ bool voxel_axis(float p, float o, float v, int* out)
{
    const float q = floorf((p - o) / v);
    if (!(q >= -1073741824.f && q < 1073741824.f)) return false;
    *out = (int)q;
    return true;
}

constexpr int VOX_RANGE_BLOCKS = 1024;       // blocks of the range pass at most (one partial row each)
constexpr int VOX_SCAN_TILE = 1024;          // sorted positions per workgroup of the head-flag scan
constexpr int VOX_SUM_TILE = 256;            // sorted positions per workgroup of the segmented sum: one per lane
constexpr int VOX_NO_POINT = 0x7fffffff;     // VoxState::bad_index when every coordinate is finite

// Device-resident facts of one call; the host reads it back once, behind the range pass, and `rows` behind the scan.
struct VoxState {
    float lo[3], hi[3];      // per-axis minimum and maximum over the finite coordinates
    float origin[3];         // the caller's, or lo
    int imin[3], imax[3];    // voxel coordinate of lo / hi: the occupied range (the voxel of a coordinate is monotone in it)
    int bad_index;           // lowest index of a point with a non-finite coordinate, or VOX_NO_POINT
    int range_bad;           // bit a / bit 3 + a: the voxel coordinate of lo[a] / hi[a] is outside [-2^30, 2^30)
    int rows;                // occupied voxels
};

struct VoxArgs {
    int n;
    float voxel;
    VoxState* state;
    const float *x, *y, *z;          // the cloud, SoA, n entries
    const float4* pts;               // the same points packed (gathers)
    float* range_lo_hi;              // VOX_RANGE_BLOCKS x 6 partial minima / maxima
    int* range_bad;                  // VOX_RANGE_BLOCKS partial lowest bad indices
    unsigned int* keys;              // n sort keys (packed path: cx | cy << 10 | cz << 20, each minus the axis minimum; else cx)
    unsigned int* axis_keys;         // 3 n: cx, cy, cz minus the axis minimum, by point (null on the packed path)
    int* vals;                       // n: the identity, the sort's values
    const unsigned int* sorted_keys; // packed path: the keys in sorted order
    const int* sorted_idx;           // n: point of every sorted position
    int* block_heads;                // per scan tile: heads in it, then (scanned) heads before it
    int* row_of;                     // n: output row of every sorted position
    int* run_start;                  // rows + 1: first sorted position of every row, then n
    double *front, *back;            // per sum tile, 3 doubles: sum of the tile's points that belong to the run entering it / leaving it
    int* fix;                        // per sum tile: the row whose run enters the tile and ends in it, or -1
    float* out_xyz;                  // rows x 3
    int *out_count, *out_coord, *voxel_of_point;
};
hipError_t vox_range(const VoxArgs& a, const float* origin3, hipStream_t s);         // -> state (origin3: 3 HOST floats, or null: the minimum)
hipError_t vox_keys(const VoxArgs& a, hipStream_t s);                                 // -> keys (+ axis_keys), vals
hipError_t vox_gather_keys(const unsigned int* axis_keys, const int* idx, int n, unsigned int* keys, hipStream_t s);   // keys[j] = axis_keys[idx[j]]
hipError_t vox_rows(const VoxArgs& a, hipStream_t s);                                 // head flags + scan -> row_of, run_start, state->rows
hipError_t vox_sums(const VoxArgs& a, hipStream_t s);                                 // segmented fp64 sums -> out_xyz, out_count, out_coord, voxel_of_point

// ---------------------------------------------------------------------------------------------------------------
// K13 exact k nearest neighbours (knn_kernels.hip; driver: knn_api.hip)
// ---------------------------------------------------------------------------------------------------------------
constexpr int KNN_MAX_K = 32;                // = MI_KNN_MAX_K (knn_api.hip asserts it)
constexpr int KNN_RANGE_BLOCKS = 512;        // blocks of the input check per array at most (one partial row each)
constexpr int KNN_NO_POINT = 0x7fffffff;     // KnnState::bad_cloud / bad_query when every coordinate is usable
constexpr float KNN_MAX_COORD = 1e18f;       // |coordinate| above this is refused: 3 (2e18)^2 < FLT_MAX keeps every d2 finite
constexpr int KNN_BLOCK = 64;                // queries per workgroup of the search: one wave, no LDS
// a slot no candidate filled: (+inf bits << 32) | 0xffffffff unpacks to d2 = +INFINITY, idx = -1, and every real key is below it
constexpr unsigned long long KNN_KEY_EMPTY = 0x7f800000ffffffffull;

// Device-resident facts of one call; the host reads it back once, behind the input check, before anything is written.
struct KnnState {
    float lo[3], hi[3];      // bounding box of the cloud's usable points
    int bad_cloud;           // lowest index of a cloud point with a non-finite or too large coordinate, or KNN_NO_POINT
    int bad_query;           // the same for the queries
};

struct NnGridView;           // nn_grid.h
// What every kernel that walks a cloud's cell grid is handed beside the grid (search_front_queries, search_front_cloud: search_front.hip).
// In self mode the queries are the cloud's own points, and order[s] is also the one candidate slot s skips, by index.
struct SearchQueries {
    const float *x, *y, *z;          // the queries along their curve order, SoA, n entries
    const int* order;                // sorted slot -> the caller's query index (the row the slot's answer goes to)
    int n;
    float hi[3];                     // upper corner of the cloud's bounding box (the lower one is the grid's origin)
};
struct SearchCloud {
    const float *x, *y, *z;          // the cloud in the caller's order, SoA: what a neighbour's or a match's index points into
};

struct KnnSearchArgs {
    const float *qx, *qy, *qz;       // SearchQueries' fields, laid out as before the view: with it inside, the search stage of
    const int* order;                // mi_knn_search measured 1.5 to 3 % slower (behind K33)
    int n, k;
    int self;                        // queries are the cloud's own points: candidate order[s] is skipped, by index
    float max_d2;                    // candidates with d2 > this do not exist (+inf: no limit)
    float hi[3];
    int* idx;                        // n * k
    float* d2;                       // n * k
    int* count;                      // n
};
// partial minima / maxima and lowest bad index of one array (lo_hi: KNN_RANGE_BLOCKS x 6, bad: KNN_RANGE_BLOCKS), then both arrays
// into the state (query partials may be null: self mode)
hipError_t knn_check_inputs(const float* cx, const float* cy, const float* cz, int m, const float* qx, const float* qy, const float* qz, int n,
                            float* lo_hi, int* bad, KnnState* st, hipStream_t s);
hipError_t knn_search(const NnGridView& g, const KnnSearchArgs& a, int fma, hipStream_t s);
int knn_list_size(int k);            // registers' worth of list the search of this k is instantiated with: 8, 16 or 32
float knn_default_points_per_cell(int k);    // cell size of the k-NN grid unless MISLAM_KNN_POINTS_PER_CELL says otherwise (search_front.hip)
// points per cell of a fixed-radius search's grid: a cell's edge is cell_in_radii radii long (search_front.hip; mi_remove_outliers' radius method, mi_iss_keypoints)
float radius_points_per_cell(const float bbox[6], int n, float radius, float cell_in_radii);

// ---------------------------------------------------------------------------------------------------------------
// K14 surface normals and curvature (normals_kernels.hip; driver: normals_api.hip): K13's search in self mode and, with the keys
// still in registers, the neighbourhood's fp64 covariance and its smallest eigenvector (eig3.hpp)
// ---------------------------------------------------------------------------------------------------------------
struct KnnNormalsArgs {
    SearchQueries q;                 // the cloud itself (self mode)
    SearchCloud c;
    int k;
    float max_d2;                    // candidates with d2 > this do not exist (+inf: no limit)
    int oriented;                    // view holds a viewpoint: normals are turned towards it
    double view[3];
    float* normals;                  // n * 3, AoS, the caller's order
    float* curvature;                // n, may be null
    int* count;                      // n, may be null
};
hipError_t knn_normals(const NnGridView& g, const KnnNormalsArgs& a, int fma, hipStream_t s);
// the same search and moments with the covariance as the output (mi_estimate_covariances; K17's inputs)
struct KnnCovariancesArgs {
    const float *qx, *qy, *qz;       // SearchQueries' and SearchCloud's fields, laid out as before the two views: through them
    const int* order;                // knn_covariances_kernel<32> takes one more VGPR
    const float *cx, *cy, *cz;
    int n, k;
    float max_d2;
    float hi[3];
    int plane;                       // 0: C itself (MI_COV_RAW); 1: I - (1 - epsilon) n n^T (MI_COV_PLANE)
    double epsilon;                  // the caller's fp32 value, promoted
    float* cov6;                     // n * 6, AoS, the caller's order: xx, xy, xz, yy, yz, zz
    int* count;                      // n, may be null
};
hipError_t knn_covariances(const NnGridView& g, const KnnCovariancesArgs& a, int fma, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K15 statistical and radius outlier removal (outlier_kernels.hip; driver: outlier_api.hip): K13's search in self mode with the
// keys' fp64 mean root as the point's score, or a fixed-radius count over the same shells (knn_scan.hpp); fp64 mean / deviation
// of the scores in a fixed order (reduce.hpp); flags in the caller's order and their stable compaction
// ---------------------------------------------------------------------------------------------------------------
constexpr int OUTLIER_STAT_BLOCK = 256;      // scores per workgroup and trip of the two statistics passes (reduce.hpp's block)
constexpr int OUTLIER_STAT_BLOCKS = 512;     // workgroups of a statistics pass at most (one partial sum each)
constexpr int OUTLIER_SCAN_TILE = 1024;      // flags per workgroup of the compaction: 256 lanes x 4 consecutive flags

// Device-resident facts of one call; the host reads it back once, with the results.
struct OutlierState {
    double mean, stddev, threshold;  // statistical: of the unrounded scores; the flags pass reads threshold from here
    long long kept;                  // the last element of the flags' scan
};

struct KnnOutlierArgs {
    SearchQueries q;                 // the cloud itself (self mode)
    int k;
    double* score;                   // n: (sum of sqrt((double)d2) over the filled slots, nearest first) / count, 0 where count is 0
    int* count;                      // n, may be null
};
hipError_t knn_outlier_score(const NnGridView& g, const KnnOutlierArgs& a, int fma, hipStream_t s);

struct RadiusCountArgs {
    SearchQueries q;                 // as above
    float r2;                        // a point j != row (by index) with d2 <= r2 counts
    int min_neighbours;              // early: a lane leaves its loops once it has counted this many
    int* count;                      // n: the number of neighbours, or (early) min(that, some value >= min_neighbours)
};
hipError_t radius_count(const NnGridView& g, const RadiusCountArgs& a, int fma, int early, hipStream_t s);

int outlier_stat_blocks(int n);      // partial sums of a statistics pass over n scores (<= OUTLIER_STAT_BLOCKS)
int outlier_scan_tiles(int n);       // tiles of the compaction of n flags
// mean, stddev (population, two passes) and threshold = mean + (double)std_ratio * stddev of n scores -> state; partials: outlier_stat_blocks(n) doubles
hipError_t outlier_statistics(const double* score, int n, float std_ratio, double* partials, OutlierState* state, hipStream_t s);
// keep[i] = score[i] <= state->threshold; mean_distance[i] = (float)score[i] where asked
hipError_t outlier_flags_statistical(const double* score, int n, const OutlierState* state, unsigned char* keep, float* mean_distance, hipStream_t s);
// keep[i] = count[i] >= min_neighbours
hipError_t outlier_flags_radius(const int* count, int n, int min_neighbours, unsigned char* keep, hipStream_t s);
struct OutlierCompactArgs {
    const unsigned char* keep;       // n flags, the caller's order
    const float* xyz;                // n * 3, AoS, as uploaded
    int n;
    int* tile_counts;                // outlier_scan_tiles(n): ones per tile, then (scanned) ones before the tile
    int* out_index;                  // n: indices of the ones, ascending (may be null)
    float* out_xyz;                  // n * 3: their points (may be null)
    OutlierState* state;             // kept
};
hipError_t outlier_compact(const OutlierCompactArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K16 point-to-plane ICP (plane_kernels.hip; driver: plane_api.hip up to the step's arguments, then pose_loop.hip, the one loop of K16, K17
// and K31; the solve: plane_solve.hpp): K13's search with one key per lane
// (NearestSink, knn_scan.hpp), the pair's 29 fp64 terms summed over the wave into one row per 64 moving points, the rows summed in a
// fixed order, and one lane's 6 x 6 solve, pose update and stop rule in the device state block
// ---------------------------------------------------------------------------------------------------------------
// PLANE_ROW (32 doubles per row and per system) and PlaneState, the device-resident loop state: pose_block.hpp, which needs no HIP
constexpr int PLANE_ONE_STAGE_ROWS = 1024;   // up to this many rows (65 536 moving points) one workgroup sums the rows and solves in one launch
constexpr int PLANE_PARTS = 64;              // beyond: this many workgroups sum a slab of rows each first (a function of the row count alone)
constexpr int MI_STOP_DEGENERATE_ = 7;       // mirror of MI_STOP_DEGENERATE (mi_slam.h; pose_loop.hip asserts it)

struct PlaneStepArgs {
    const PlaneState* state;         // the pose to linearise at (rounded to fp32 by every lane), the centre, done
    SearchQueries q;                 // the moving cloud
    SearchCloud c;                   // the fixed cloud
    const float4* normals;           // the fixed cloud's normals in the caller's order (w unused)
    float max_d2;                    // a match with d2 > this is no pair (+inf: no limit)
    double* rows;                    // plane_row_count(n) x PLANE_ROW
    int* idx;                        // may be null; n, the caller's order: the matched fixed index of a pair, -1 otherwise
};
struct PlaneRules {
    double eps_rotation, eps_translation;
    int max_iterations;
    int solve;                       // 0: the sums go into the state and nothing else happens (mi_plane_system)
};
int plane_row_count(int n);          // rows of a moving cloud of n points: one per 64
int plane_part_count(int nrows);     // 0: one launch sums the rows and solves; else the slabs of the first of two
hipError_t plane_step(const NnGridView& g, const PlaneStepArgs& a, int fma, hipStream_t s);
// rows -> state->sums -> (rules.solve) the solve, the update and the stop rule; parts: plane_part_count(nrows) x PLANE_ROW doubles, null where that is 0
hipError_t plane_reduce_solve(PlaneState* state, const double* rows, int nrows, double* parts, const PlaneRules& rules, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K17 generalized ICP (gicp_kernels.hip; driver: gicp_api.hip, then pose_loop.hip): K16's iteration with a 3 x 3 information matrix per pair where K16 has a
// normal.  The step kernel writes K16's rows (PLANE_ROW doubles per 64 moving points, the same layout), so the rows reduce, the solve,
// the state block and the rules are K16's own: plane_reduce_solve, PlaneState, PlaneRules.
// ---------------------------------------------------------------------------------------------------------------
struct GicpStepArgs {
    const PlaneState* state;         // the pose to linearise at (rounded to fp32 by every lane), the centre, done
    SearchQueries q;                 // the moving cloud
    SearchCloud c;                   // the fixed cloud
    const float4* cov_a;             // the fixed cloud's covariances in the caller's order, two float4 each: (xx, xy, xz, 0), (yy, yz, zz, 0)
    const float4* cov_b;             // the moving cloud's along its curve order, the same layout: read at the lane's own slot
    float max_d2;                    // a match with d2 > this is no pair (+inf: no limit)
    double* rows;                    // plane_row_count(n) x PLANE_ROW
    int* idx;                        // may be null; n, the caller's order: the matched fixed index of a pair, -1 otherwise
};
hipError_t gicp_step(const NnGridView& g, const GicpStepArgs& a, int fma, hipStream_t s);
// count covariances of six floats as uploaded -> two float4 each; *bad = min(*bad, the lowest index with a non-finite entry or one above
// 1e18 in magnitude) -- the caller sets *bad to KNN_NO_POINT first
hipError_t gicp_pack_covariances(const float* cov6, int count, float4* packed, int* bad, hipStream_t s);
// out[2 s], out[2 s + 1] = in[2 order[s]], in[2 order[s] + 1]: the moving cloud's covariances along its curve
hipError_t gicp_permute_covariances(const float4* in, const int* order, int n, float4* out, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K18 / K19 FPFH descriptors (fpfh_kernels.hip; driver: fpfh_api.hip; the pair features and bins: fpfh_pair.hpp): K13's search in self
// mode with the pairs' bins counted while the keys are in registers, then the distance-weighted sums over every point's neighbours
// ---------------------------------------------------------------------------------------------------------------
constexpr int FPFH_WORDS = 9;                // 32-bit words of a point's packed counts: per feature 11 bins as bytes of three words,
                                             // bin b in byte b & 3 of word b >> 2; byte 3 of the third word: the point's neighbour count
constexpr int FPFH_SUM_POINTS = 64;          // points per workgroup of K19 ...
constexpr int FPFH_SUM_BLOCK = 3 * FPFH_SUM_POINTS;   // ... at three lanes a point, one per feature
struct FpfhSpfhArgs {
    SearchQueries q;                 // the cloud itself (self mode)
    SearchCloud c;
    const float *nx, *ny, *nz;       // the normals, as the cloud: SoA, the caller's order
    int k;
    float max_d2;                    // candidates with d2 > this do not exist (+inf: no limit)
    unsigned long long* keys;        // n * k, the caller's order: row i of mi_knn_search as keys, KNN_KEY_EMPTY behind the filled slots
    unsigned int* packed;            // n * FPFH_WORDS, the caller's order
    int* count;                      // n, may be null
};
hipError_t fpfh_spfh(const NnGridView& g, const FpfhSpfhArgs& a, int fma, hipStream_t s);
struct FpfhSumArgs {
    const int* order;                // K18's: lanes next to each other work on points next to each other
    const unsigned long long* keys;  // K18's
    const unsigned int* packed;      // K18's
    int n, k;
    float* fpfh;                     // n * 33, the caller's order
    unsigned char* counts;           // n * 33, may be null: the counts, unpacked
};
hipError_t fpfh_sum(const FpfhSumArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K20 - K22 descriptor matching (match_kernels.hip; driver: match_api.hip): every pair's dot product on the matrix pipe, the running minimum
// of fmaf(-2, dot, |t|^2) per query, chunks of targets merged by a packed atomicMin
// ---------------------------------------------------------------------------------------------------------------
constexpr int MATCH_MAX_DIM = 64;            // MI_FEATURE_MAX_DIM
constexpr float MATCH_MAX_ABS = 1e15f;       // 64 * (1e15)^2 < FLT_MAX: no chain overflows
constexpr int MATCH_TILE = 128;              // queries of a workgroup (32 per wave), and targets of an LDS tile
constexpr int MATCH_BLOCK = 256;
constexpr int MATCH_NO_ROW = 0x7fffffff;     // K20's *bad while no row has been refused
// norm[i] = the fmaf chain of row i with itself; *bad = min(*bad, the lowest row with a non-finite component or one above MATCH_MAX_ABS)
hipError_t match_norms(const float* feat, int rows, int dim, float* norm, int* bad, hipStream_t s);
struct MatchArgs {
    const float* query;              // n * dim, row-major: the side that searches
    const float* target;             // m * dim: the side that is searched
    const float* target_norm;        // m (K20)
    int n, m, dim;
    int chunk_len;                   // targets per workgroup column, a multiple of MATCH_TILE (match_chunk_len)
    unsigned long long* keys;        // n, all ones before the launch: (ordered key << 32 | target) of the minimum
};
int match_chunk_len(int n, int m, int cu_count);
hipError_t match_search(const MatchArgs& a, hipStream_t s);
struct MatchFinishArgs {
    const float *query, *target;
    int n, m, dim;
    const unsigned long long* keys;      // n: the forward search's
    const unsigned long long* rev_keys;  // m: the reverse search's (the mutual filter), or null
    int* idx;                        // n
    float* d2;                       // n, may be null
};
hipError_t match_finish(const MatchFinishArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K23 - K26 hypothesise and verify over correspondences (ransac_kernels.hip; driver: ransac_api.hip)
// ---------------------------------------------------------------------------------------------------------------
constexpr int RANSAC_BLOCK = 256;
struct RansacHypArgs {
    const float* pairs6;             // C x (sx, sy, sz, tx, ty, tz): the correspondences by rank
    const int* src_index;            // C: rank -> the source index i of the pair
    int C;
    unsigned long long seed;
    double e2;                       // (double)edge_similarity squared
    int first, count;                // hypotheses first .. first + count - 1; the outputs are indexed from 0
    int* triples;                    // 3 * count: the source indices of the three draws
    unsigned char* valid;            // count
    float* pose12;                   // 12 * count: R9 column-major, then t3; the identity where invalid
};
hipError_t ransac_hypotheses(const RansacHypArgs& a, hipStream_t s);
struct RansacCountArgs {
    const float* pairs6; int C;
    const float* pose12; const unsigned char* valid; int count;
    double max_d2;                   // (double)max_distance squared
    int chunk_len;                   // pairs per workgroup row, a multiple of RANSAC_BLOCK (ransac_chunk_len)
    int* inlier_count;               // count, zero before the launch
};
int ransac_chunk_len(int count, int C, int cu_count);
hipError_t ransac_count(const RansacCountArgs& a, hipStream_t s);
// *best = max(*best, inliers << 32 | 0xFFFFFFFF - h) over the valid hypotheses, *nvalid += their number; both zero before the launch
hipError_t ransac_argmax(const unsigned char* valid, const int* inlier_count, int count, unsigned long long* best, int* nvalid, hipStream_t s);
struct RansacMaskArgs {
    const float* pairs6; int C;
    const float* pose;               // 12 floats on the device
    double max_d2;
    unsigned char* mask;             // C, by rank
    double* d2;                      // C: the squared distance of an inlier, 0 otherwise
};
hipError_t ransac_mask_and_sum(const RansacMaskArgs& a, int* out_count, double* out_sum, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K39 - K43 the dominant planes of a cloud (segment_kernels.hip; driver: segment_api.hip; the contract: mi_segment_plane in mi_slam.h).
// K23 - K26's pattern over points instead of pairs: a round works on the REMAINING points by rank (rem_xyz, AoS, and rem_index, rank ->
// the caller's index), K25's ransac_argmax picks the winner as it is, and K15's outlier_compact peels a plane's inliers off.
// ---------------------------------------------------------------------------------------------------------------
constexpr int SEGMENT_BLOCK = 256;   // = RANSAC_BLOCK: ransac_chunk_len plans K40's chunks, ransac_argmax reads its counts
static_assert(SEGMENT_BLOCK == RANSAC_BLOCK, "K40 is planned by ransac_chunk_len");
constexpr int SEGMENT_SUMS = 12;     // what K42 leaves: count, S, sum x y z, then xx xy xz yy yz zz about the centroid
struct SegmentHypArgs {
    const float* rem_xyz;            // C x 3: the remaining points by rank
    const int* rem_index;            // C: rank -> the caller's index
    int C;
    unsigned long long seed;
    unsigned long long g0;           // the global number of the first hypothesis of the launch: round * H + first
    int count;                       // hypotheses g0 .. g0 + count - 1; the outputs are indexed from 0
    int has_axis;
    double axis[3], cos2;            // the caller's fp32 values, promoted; (double)cos * (double)cos
    int* triples;                    // 3 * count: the caller's indices of the three draws
    unsigned char* valid;            // count
    float* plane4;                   // 4 * count: a, b, c, d; zeros where invalid
};
hipError_t segment_hypotheses(const SegmentHypArgs& a, hipStream_t s);
struct SegmentCountArgs {
    const float* rem_xyz; int C;
    const float* plane4; const unsigned char* valid; int count;
    double T2;                       // (double)distance_threshold squared
    int chunk_len;                   // points per workgroup row, a multiple of SEGMENT_BLOCK (ransac_chunk_len)
    int* inlier_count;               // count, zero before the launch
};
hipError_t segment_count(const SegmentCountArgs& a, hipStream_t s);
// mask[r], s2[r] = s s / nn of an inlier (0 otherwise) of every remaining point under ONE plane on the device, then sums[SEGMENT_SUMS] by
// one workgroup each in ransac_sum's fixed order: count, S and the coordinate sums; with want_scatter the six sums about the centroid too
struct SegmentMaskArgs {
    const float* rem_xyz; int C;
    const float* plane;              // 4 floats on the device
    double T2;
    unsigned char* mask;             // C, by rank
    double* s2;                      // C
    double* sums;                    // SEGMENT_SUMS
};
hipError_t segment_mask_and_sums(const SegmentMaskArgs& a, int want_scatter, hipStream_t s);
// labels[i] = -1, keep[i] = 1 for the n points of a call
hipError_t segment_begin(int* labels, unsigned char* keep, int n, hipStream_t s);
// labels[rem_index[r]] = plane, keep[rem_index[r]] = 0 where mask[r]
hipError_t segment_label(const unsigned char* mask, const int* rem_index, int C, int plane, int* labels, unsigned char* keep, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K44 - K47 Fast Global Registration over correspondences (fgr_kernels.hip; driver: fgr_api.hip, then pose_loop.hip for the iterations;
// the contract: mi_fgr_register in mi_slam.h).  K23's draws and edge rule (ransac_draw.hpp) as a filter over trials, K15's
// outlier_compact over the trials' flags, the kept triples gathered into the USED list (pairs of points by used rank), and a step kernel
// that writes K16's rows from the used list alone -- no search -- so the reduce and the solve are K16's own.
// ---------------------------------------------------------------------------------------------------------------
constexpr int FGR_BLOCK = 256;
struct FgrTrialArgs {
    const float4 *src4, *tgt4;       // both clouds as uploaded, packed (w unused)
    const int *match_src, *match_tgt;   // C: rank -> the source index i and the target index idx[i] of the match
    int C;
    unsigned long long seed;
    double e2;                       // (double)tuple_scale squared
    int trials;
    int* triples;                    // 3 * trials: the RANKS of the three draws
    unsigned char* accept;           // trials: three distinct ranks whose edges pass
};
hipError_t fgr_trials(const FgrTrialArgs& a, hipStream_t s);            // K44
struct FgrGatherArgs {
    const float4 *src4, *tgt4;
    const int *match_src, *match_tgt;
    const int* kept_trials;          // outlier_compact's out_index over accept: used match u is draw u % 3 of trial kept_trials[u / 3];
    const int* triples;              // ... both null: used match u is rank u (no tuple filter)
    int used;                        // 3 * the kept trials, or C
    int *used_src, *used_tgt;        // used: the match's indices into the caller's clouds
    float4 *used_p, *used_q;         // used: its source and its target point
};
hipError_t fgr_gather(const FgrGatherArgs& a, hipStream_t s);           // K45
struct FgrStepArgs {
    const PlaneState* state;         // the fp64 pose to linearise at (NOT rounded to fp32), the centre, iterations, done
    const float4 *p, *q;             // the used list: source and target points
    int used;
    double D2, delta2, division_factor;   // the schedule's operands (fgr_schedule.hpp)
    int decrease_every;
    int k;                           // the applied updates mu is formed from; < 0: state->iterations
    double* rows;                    // plane_row_count(used) x PLANE_ROW
    double* mu_out;                  // [0]: the mu of this linearisation
    float* weights;                  // fgr_weights alone; used: (float)l
};
hipError_t fgr_step(const FgrStepArgs& a, hipStream_t s);               // K46; returns at once where the state says done
hipError_t fgr_weights(const FgrStepArgs& a, hipStream_t s);            // K47: the step's arithmetic up to l, no rows, whatever done says

// ---------------------------------------------------------------------------------------------------------------
// K27 - K31 NDT registration (ndt_kernels.hip; driver: ndt_api.hip, then pose_loop.hip for the iterations; the term of a pair: ndt_term.hpp).  mi_ndt_voxels: the voxel filter's
// own front end (VoxArgs above: coordinates, counts and means are mi_voxel_downsample's by construction), then a second segmented pass
// over the sorted order for the scatter about the fp32 mean and one lane per voxel for the eigenvalue floor and the inverse.
// mi_ndt_register: the listed voxels in the hash table of voxel_table.hpp, the step kernel writing K16's rows from a direct lookup per point,
// and K16's own reduce and solve behind the rows.
// ---------------------------------------------------------------------------------------------------------------
struct NdtScatterArgs {
    VoxArgs v;                       // the front end's arrays, as vox_sums left them (out_xyz: the fp32 means)
    double *front, *back;            // per sum tile, 6 doubles: as VoxArgs::front / back, of the six products
    int* fix;                        // per sum tile: as VoxArgs::fix
    double* q6;                      // rows x 6: sum (p_a - mu_a)(p_b - mu_b), xx xy xz yy yz zz
};
hipError_t ndt_scatter(const NdtScatterArgs& a, hipStream_t s);
// one lane per voxel, rows_at_most lanes (>= st->rows, which the device knows): C = Q / (count - 1), the eigenvalue floor, C' (cov6, may be
// null) and M = C'^-1, six floats each (zeros: no distribution)
hipError_t ndt_voxel_finish(const double* q6, const int* count, const VoxState* st, int rows_at_most, int min_points, float eig_ratio, float* icov6,
                            float* cov6, hipStream_t s);

constexpr int NDT_NO_ROW = 0x7fffffff;       // NdtMapState's bad_* while no row has been refused
// Device-resident facts of the listed voxels; the host sets the starts, the check kernel folds every row in with integer atomics (minima
// and maxima: the same answer in any order), and the host reads it back once, before anything is written.
struct NdtMapState {
    int bad_mean, bad_icov, bad_coord, bad_order;    // lowest refused row of each kind, or NDT_NO_ROW
    int cmin[3], cmax[3];            // per-axis range of the listed coordinates
    unsigned int lo[3], hi[3];       // bounding box of the means of the rows with a distribution, as ordered keys (ndt_float_key)
    int with_distribution;           // such rows
};
// an fp32 value as an unsigned key of the same order, and back (-0 below +0; the check has refused NaN before a key is formed)
__host__ __device__ __forceinline__ unsigned int ndt_float_key(float v)
{
    union { float f; unsigned int u; } x;
    x.f = v;
    return (x.u & 0x80000000u) ? ~x.u : (x.u | 0x80000000u);
}
__host__ __device__ __forceinline__ float ndt_key_float(unsigned int k)
{
    union { float f; unsigned int u; } x;
    x.u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return x.f;
}

struct NdtMapView {
    VoxelTableView table;            // voxel_table.hpp: the listed voxels' rows, 2 slots per voxel
    const float4* mean;              // nv: (x, y, z, 0)
    const float4* icov;              // 2 nv: (xx, xy, xz, 0), (yy, yz, zz, 0)
};
// the listed voxels as uploaded -> packed means and matrices, and the facts of NdtMapState
hipError_t ndt_check_voxels(const int* coord, const float* mean, const float* icov6, int nv, float4* mean4, float4* icov4, NdtMapState* st, hipStream_t s);
// the rows with a distribution into the table (every slot free before the launch)
hipError_t ndt_hash_build(const int* coord, const float4* icov4, int nv, const NdtMapView& map, unsigned long long* keys, int* vals, hipStream_t s);

struct NdtStepArgs {
    const PlaneState* state;         // the pose to linearise at (rounded to fp32 by every lane), the centre, done
    const float *bx, *by, *bz;       // the moving cloud along its curve order, SoA, n entries
    const int* order;                // sorted slot -> the caller's moving index
    int n;
    NdtMapView map;
    float origin[3], voxel;          // mi_voxel_index's operands
    double h, k;                     // mi_ndt_constants' out[2], out[3]
    double* rows;                    // plane_row_count(n) x PLANE_ROW
    int* idx;                        // may be null; n, the caller's order: the row of the point's own voxel, or -1
    unsigned char* terms;            // may be null; n, the caller's order: the point's number of terms
};
hipError_t ndt_step(const NdtStepArgs& a, int neighbourhood, hipStream_t s);      // neighbourhood 1, 7 or 27

// ---------------------------------------------------------------------------------------------------------------
// K32 / K33 ISS keypoints (iss_kernels.hip; driver: iss_api.hip): the fixed-radius walk of K15 over one cell grid, twice.  K32 takes the
// fp64 scatter of the salient ball as it walks, and behind the walk the eigenvalues (eig3.hpp), the gate and the fp32 saliency; K33 walks
// the non-max ball of every candidate, gathers the neighbours' saliencies and leaves at the first one that dominates.  The flags are
// compacted by K15's outlier_compact.
// ---------------------------------------------------------------------------------------------------------------
struct IssSaliencyArgs {
    SearchQueries q;                 // the cloud itself (self mode)
    SearchCloud c;
    float r2;                        // a point j != row (by index) with d2 <= r2 is in the salient ball
    int min_neighbours;
    double gamma_21, gamma_32;       // the caller's fp32 values, promoted
    float* saliency;                 // n, the caller's order: max((float)lambda0, 0) where the gate holds, +0 elsewhere
    float* eigenvalues;              // n * 3, ascending, may be null
    int* neighbours;                 // n, may be null
};
hipError_t iss_saliency(const NnGridView& g, const IssSaliencyArgs& a, int fma, hipStream_t s);

struct IssSuppressArgs {
    SearchQueries q;                 // as above
    float r2;                        // the non-max ball
    int min_neighbours;
    const float* saliency;           // n, the caller's order (K32's)
    unsigned char* is_keypoint;      // n, the caller's order: every row is written
};
hipError_t iss_suppress(const NnGridView& g, const IssSuppressArgs& a, int fma, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K50 moving-least-squares smoothing (mls_kernels.hip; driver: mls_api.hip; the arithmetic behind the walks: mls_fit.hpp): the fixed-radius
// walk of K15 over one cell grid, twice per query and with nothing skipped.  The first walk takes K32's nine fp64 sums about the query, and
// behind it come the plane (eig3.hpp), the query's foot on it and the frame; the second walk takes the 27 weighted sums of a full quadratic over
// that plane, and behind it come plane_solve6 (plane_solve.hpp), the fall-back decision and the projection.  order == 1 is an instance without the
// second walk.
// ---------------------------------------------------------------------------------------------------------------
struct MlsArgs {
    SearchQueries q;                 // the queries: the cloud itself in self mode, or a cloud of their own along their own curve
    SearchCloud c;
    float r2;                        // a point with d2 <= r2 is in the ball, the query's own copy included
    int min_neighbours;              // >= 3
    double s2;                       // the square of the Gaussian's scale
    float* xyz;                      // nq * 3, AoS, the caller's order: every row is written
    float* normals;                  // nq * 3, may be null
    float* curvature;                // nq, may be null
    int* neighbours;                 // nq, may be null
    unsigned char* status;           // nq, may be null
};
hipError_t mls_smooth(const NnGridView& g, const MlsArgs& a, int order, int fma, hipStream_t s);      // order 1 or 2

// ---------------------------------------------------------------------------------------------------------------
// K51 - K54 every neighbour within a radius, as CSR lists (radius_kernels.hip; driver: radius_api.hip).  The lengths are K15's full radius
// count; K51 scans them into 64-bit offsets in the caller's row order (three small launches, a fixed order, no atomics); K52 walks the ball
// a second time with a sink that stores the packed keys (bits(d2) << 32) | j at keys[offsets[row] + found++] (RadiusFillSink, knn_scan.hpp);
// K53 orders every row in place by key, one wave per row: a rank by counted smaller keys over the wave's lanes up to RADIUS_WAVE_ROW keys,
// a bitonic network through LDS chunks of RADIUS_SORT_CHUNK keys beyond; K54 unpacks the keys into idx and d2.
// ---------------------------------------------------------------------------------------------------------------
constexpr int RADIUS_SCAN_TILE = 1024;       // counts per workgroup of the scan: 256 lanes x 4 consecutive counts
constexpr int RADIUS_WAVE_ROW = 64;          // the longest row K53 ranks in registers: one key per lane of a wave
constexpr int RADIUS_SORT_CHUNK = 512;       // keys of a longer row that K53 holds in the LDS at a time (a power of two, >= 2 * RADIUS_WAVE_ROW)

int radius_scan_tiles(int n);        // tiles of the scan of n counts
// offsets[i] = count[0] + ... + count[i - 1] for i = 0 .. n (offsets[n]: the total), all sums in 64 bits; tile_sums: radius_scan_tiles(n) words
hipError_t radius_scan_offsets(const int* count, int n, long long* tile_sums, long long* offsets, hipStream_t s);

struct RadiusFillArgs {
    SearchQueries q;                 // the queries: the cloud itself in self mode, or a cloud of their own along their own curve
    int self;                        // self mode: candidate order[s] is skipped, by index
    float r2;                        // a point with d2 <= r2 belongs to the row
    const long long* offsets;        // n + 1, the caller's row order
    unsigned long long* keys;        // offsets[n] keys: row i is [offsets[i], offsets[i + 1]), in the order the walk met its members
    int* mismatch;                   // one word the caller zeroed: set to 1 by a lane whose walk met another number of members than its row holds
};
// the count of a separate query set: radius_count (K15) skips index order[s] whatever the mode, so it serves self mode alone
hipError_t radius_query_count(const NnGridView& g, const SearchQueries& q, float r2, int* count, int fma, hipStream_t s);
hipError_t radius_fill(const NnGridView& g, const RadiusFillArgs& a, int fma, hipStream_t s);
// every row [offsets[i], offsets[i + 1]) of keys ascending, in place
hipError_t radius_sort_rows(const long long* offsets, long long rows, unsigned long long* keys, hipStream_t s);
// the points of every cell of a grid ascending by index, in place: the build leaves them in the order its atomics made, and a walk that
// writes what it meets (K52 without K53 behind it) must meet the same order on every call.  Leaves NnGridView::slot_of stale.
hipError_t radius_order_cells(const unsigned int* cell_start, long long n_cells, float4* pts, hipStream_t s);
hipError_t radius_unpack(const unsigned long long* keys, long long total, int* idx, float* d2, hipStream_t s);     // d2 may be null

// ---------------------------------------------------------------------------------------------------------------
// K34 - K38 density-based clustering (cluster_kernels.hip; driver: cluster_api.hip): the core flags are K15's early radius count; K34 links
// the core points of every ball in a lock-free union-find over the caller's indices (the argument: the head of cluster_kernels.hip); K35
// resolves every point to the root of its cluster (a core point's own, a border point's nearest core neighbour's); K36 counts the clusters'
// sizes and flags the roots that pass the size filter, K15's outlier_compact numbers them, K37 scatters ranks and sizes, K38 writes the labels.
// ---------------------------------------------------------------------------------------------------------------
struct ClusterLinkArgs {
    SearchQueries q;                 // the cloud itself (self mode)
    float r2;                        // a point j != row (by index) with d2 <= r2 is a neighbour
    const int* count;                // n, the caller's order: K15's early count; null: every point is core
    int need;                        // point j is core iff count[j] >= need (= min_points - 1)
    int* parent;                     // n, the caller's order, the identity before the launch; parent[x] <= x always
};
hipError_t cluster_identity(int* parent, int n, hipStream_t s);
hipError_t cluster_link(const NnGridView& g, const ClusterLinkArgs& a, int fma, hipStream_t s);
struct ClusterResolveArgs {
    SearchQueries q;                 // as above
    float r2;
    const int* count;                // as above
    int need;
    const int* parent;               // K34's, read only
    int* root_of;                    // n, the caller's order: the root (= smallest core index) of the point's cluster, or -1 (noise)
    unsigned char* is_core;          // n, the caller's order: every row is written
};
hipError_t cluster_resolve(const NnGridView& g, const ClusterResolveArgs& a, int fma, hipStream_t s);
struct ClusterNumberArgs {
    int n;
    const int* root_of;              // K35's
    int* size;                       // n, zero before cluster_count_sizes: size[r] = the points whose root is r
    int min_size, max_size;          // max_size 0: no upper limit
    unsigned char* keep;             // n: root_of[i] == i and size[i] within the limits -- the surviving roots (what outlier_compact numbers)
    const int* roots;                // outlier_compact's out_index over keep: the surviving roots, ascending
    const OutlierState* state;       // ... and its kept: their number
    int* rank;                       // n: rank[roots[c]] = c; other entries are not written (cluster_labels reads it where keep is 1 only)
    int* sizes_out;                  // may be null; cap entries: size[roots[c]] for c < min(kept, cap)
    int cap;
    int* labels;                     // n
    unsigned char* labelled;         // may be null; n: labels[i] >= 0
};
hipError_t cluster_count_sizes(const ClusterNumberArgs& a, hipStream_t s);      // K36: size, then keep
hipError_t cluster_ranks(const ClusterNumberArgs& a, hipStream_t s);      // K37: rank, sizes_out
hipError_t cluster_labels(const ClusterNumberArgs& a, hipStream_t s);     // K38: labels, labelled
// keys[k] = (unsigned)labels[index[k]] >> shift for k < count: the sort keys of the grouping
hipError_t cluster_group_keys(const int* labels, const int* index, int count, int shift, unsigned int* keys, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K48 / K49 colored ICP (color_kernels.hip; driver: color_api.hip, then pose_loop.hip for the iterations; the arithmetic of a gradient and
// of a pair: color_terms.hpp).  K48 is K14's shape -- K13's search in self mode and, with the keys still in registers, the sums of a
// tangent-plane least squares and its 3 x 3 solve.  K49 is K16's step with a photometric residual beside the geometric one; it writes K16's
// rows, so the reduce, the solve, the state block and the rules are K16's own: plane_reduce_solve, PlaneState, PlaneRules.
// ---------------------------------------------------------------------------------------------------------------
struct ColorGradientArgs {
    SearchQueries q;                 // the cloud itself (self mode)
    SearchCloud c;
    const float *nx, *ny, *nz;       // the normals, as the cloud: SoA, the caller's order
    const float* intensity;          // n, the caller's order
    int k;
    float max_d2;                    // candidates with d2 > this do not exist (+inf: no limit)
    float* gradients;                // n * 3, AoS, the caller's order
    int* count;                      // n, may be null
};
hipError_t color_gradients(const NnGridView& g, const ColorGradientArgs& a, int fma, hipStream_t s);
struct ColorStepArgs {
    const PlaneState* state;         // the pose to linearise at (rounded to fp32 by every lane), the centre, done
    SearchQueries q;                 // the moving cloud
    SearchCloud c;                   // the fixed cloud
    const float4* normals;           // the fixed cloud's normals in the caller's order (w unused)
    const float4* grad_i;            // the fixed cloud's colour gradients and intensities in the caller's order: (g_x, g_y, g_z, I)
    const float* ib;                 // the moving cloud's intensities along its curve order: read at the lane's own slot
    double lambda;                   // the caller's fp32 lambda_geometric, promoted
    float max_d2;                    // a match with d2 > this is no pair (+inf: no limit)
    double* rows;                    // plane_row_count(n) x PLANE_ROW
    int* idx;                        // may be null; n, the caller's order: the matched fixed index of a pair, -1 otherwise
};
hipError_t color_step(const NnGridView& g, const ColorStepArgs& a, int fma, hipStream_t s);
// *bad = min(*bad, the lowest index of v with a value that is not finite or above 1e18 in magnitude) -- the caller sets *bad to KNN_NO_POINT first
hipError_t color_check_values(const float* v, int count, int* bad, hipStream_t s);
// m gradients of three floats and m intensities as uploaded -> one float4 each; both arrays checked as above, each into its own word
hipError_t color_pack_fixed(const float* grad3, const float* intensity, int m, float4* packed, int* bad_intensity, int* bad_gradient, hipStream_t s);
// out[s] = in[order[s]]: the moving cloud's intensities along its curve
hipError_t color_permute_intensity(const float* in, const int* order, int n, float* out, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K55 the quality of a pose (eval_kernels.hip; driver: eval_api.hip; the host arithmetic behind the sums: eval_block.hpp): K16's move and
// match, or the caller's pairs, and the point-to-point terms about the origin in K16's row -- so the rows reduce, the state block and the
// read-back are K16's own: plane_reduce_solve with solve = 0, PlaneState.
// ---------------------------------------------------------------------------------------------------------------
struct EvalStepArgs {
    const PlaneState* state;         // the pose to evaluate at (rounded to fp32 by every lane)
    SearchQueries q;                 // the moving cloud along its curve order, in both modes
    SearchCloud c;                   // the fixed cloud
    const int* pair_idx;             // null: the pair is the nearest fixed point (the grid is walked); else n entries in the caller's
                                     // order, -1 or a fixed index in [0, m) (eval_check_pairs), and the grid is not touched
    int m;                           // fixed points (what a given index is held against once more)
    float max_d2;                    // a pair with d2 > this, or with a d2 that is not finite, is no pair (+inf: no limit)
    double* rows;                    // plane_row_count(n) x PLANE_ROW
    int* idx;                        // may be null; n, the caller's order: the fixed index of a pair, -1 otherwise
    float* d2;                       // may be null; n, the caller's order: the pair's fp32 squared distance, +inf otherwise
};
hipError_t eval_step(const NnGridView& g, const EvalStepArgs& a, int fma, hipStream_t s);
// *bad = min(*bad, the lowest i with pair_idx[i] outside {-1} and [0, m)) -- the caller sets *bad to KNN_NO_POINT first
hipError_t eval_check_pairs(const int* pair_idx, int n, int m, int* bad, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K56-K63 pose-graph optimisation (pose_graph_kernels.hip; driver: pose_graph_api.hip; the edge's arithmetic: pose_graph_terms.hpp).
// Everything fp64.  Per edge and per node arrays are structure-of-arrays: component c of item i at [c * count + i].  Every sum over a node's
// incidence list follows one rule, whichever kernel forms it: lane l of 64 adds the list's entries l, l + 64, ... in ascending order, and
// the 64 partial sums are added one by one from lane 0 on -- for a list of at most 64 entries that is the list's own order, which one lane
// retraces alone; longer lists (PG_LONG_LIST) take one wave per node.  Every sum over the nodes or the edges goes through reduce.hpp.
// ---------------------------------------------------------------------------------------------------------------
struct PgGraph {
    int V, E, reference;
    const int *src, *tgt;            // E each
    const unsigned char* uncertain;  // E, or null: no edge is
    const double* Z;                 // [12][E]: the measurements as given, R row-major then t
    const double* L;                 // [21][E]: the upper triangles of the information matrices
    const int* list;                 // 2 E entries 2 * edge + side, by node, ascending within a node
    const int* offsets;              // V + 1
    const int* long_nodes;           // the nodes whose list is longer than PG_LONG_LIST, ascending
    int n_long;
    double mu;                       // line_process_mu
};
struct PgTerms {
    double *r, *chi2, *w, *M, *h;    // [6][E], E, E, [21][E], [6][E]
};
struct PgState {                     // the device-resident scalars of the inner solve and the costs
    double rz, pq, alpha, beta, gg, rr;
    double cost[2];                  // [0] at the linearisation, [1] of the candidate
    double tolerance;
    int done, iterations, max_iterations, breakdown;
};
static_assert(sizeof(PgState) <= 64 * sizeof(float), "a PgState must fit the context's pinned scratch");
struct PgVectors {
    double *x, *r, *z, *p, *q;       // [6][V] each
    double* pq_node;                 // V: a long node's p . q, from the wave that formed it
    double* parts;                   // pg_node_blocks(V) x 2: the partial rows of the dots
};
static inline int pg_blocks(int count) { return (count + 255) / 256; }
// K56: keys[i] = (the node of list entry vals_in[i]) >> shift; with vals_in null the entries are 0 .. n2 - 1 themselves and vals_out receives them
hipError_t pg_incidence_keys(const int* src, const int* tgt, const int* vals_in, int n2, int shift, unsigned int* keys, int* vals_out, hipStream_t s);
hipError_t pg_build_offsets(const PgGraph& g, int* offsets, hipStream_t s);                       // K56 (g.list filled, g.offsets not read)
// K57: one lane per edge; with system = 0 only chi2 and w are written (the candidate pass).  cost_parts: pg_blocks(E) partial sums.
hipError_t pg_edge_terms_launch(const PgGraph& g, const double* poses, const PgTerms& t, int system, double* cost_parts, hipStream_t s);
hipError_t pg_cost_finish(const double* cost_parts, int nparts, PgState* st, int slot, hipStream_t s);   // K58
hipError_t pg_node_gather(const PgGraph& g, const PgTerms& t, double* diag /*[21][V]*/, double* grad /*[6][V]*/, hipStream_t s);   // K59
// K60: q = (H + lambda diag H) p and the partial sums of p . q; honours st->done unless st is null
hipError_t pg_product(const PgGraph& g, const PgTerms& t, const double* diag, double lambda, const double* p, double* q, double* pq_node, double* parts,
                      const PgState* st, hipStream_t s);
// K61, K62: the inner solve.  pg_pcg_begin resets the state and forms r = -g, z, p; pg_pcg_iterations enqueues `count` iterations, each of
// which returns at once where the state says done.
hipError_t pg_pcg_begin(const PgGraph& g, const double* diag, const double* grad, double lambda, double tolerance, int max_iterations, const PgVectors& v,
                        PgState* st, hipStream_t s);
hipError_t pg_pcg_iterations(const PgGraph& g, const PgTerms& t, const double* diag, double lambda, const PgVectors& v, PgState* st, int count, hipStream_t s);
hipError_t pg_apply_step(const PgGraph& g, const double* poses, const double* x, double* out_poses, hipStream_t s);   // K63

// ---------------------------------------------------------------------------------------------------------------
// K64-K67 Scan Context: place recognition for loop closures (scan_context_kernels.hip; driver: scan_context_api.hip; the binning's
// arithmetic: scan_context_bin.hpp; the contract: mi_scan_context and mi_scan_context_search in mi_slam.h).
//   K64 sc_bins:      one workgroup per slice of SC_SLICE points of one scan: the descriptor of the slice in the LDS as the bits of the bins'
//                     positive fp32 maxima (which order as unsigned integers), merged into the scan's descriptor by atomicMax; the input
//                     check (lowest refused point by atomicMin) in the same pass.
//   K65 sc_normalise: one wave per descriptor, one lane per sector: the column's fp64 norm in ring order, the fp32 unit column, the
//                     64-bit mask of the non-empty columns, the input check.
//   K66 sc_search:    one workgroup of SC_SEARCH_WAVES waves per (query, chunk of SC_SEARCH_CHUNK-row multiples); a wave forms one
//                     candidate's sectors x sectors cosines on the matrix pipe (v_mfma_f32_32x32x2_f32, the query's unit columns resident
//                     in registers as the A operand), parks them in its own LDS tile, and lane s sums the wrapped diagonal of shift s in
//                     fp64; every lane keeps the running minimum of its shift, merged at the end by atomicMin on
//                     (ordered(distance) << 32 | row << 6 | shift).
//   K67 sc_finish:    one lane per query: the key unpacked into idx, dist, shift (and the runner-up's distance).
// ---------------------------------------------------------------------------------------------------------------
constexpr int SC_SLICE = 4096;               // points of a scan per workgroup of K64, at least (a longer scan than 65 535 slices: longer slices)
constexpr int SC_SEARCH_WAVES = 2;           // waves of a K66 workgroup; each takes every SC_SEARCH_WAVES-th row of the chunk
constexpr int SC_SEARCH_CHUNK = 64;          // database rows of a K66 workgroup: a multiple of this (sc_chunk_len)
constexpr int SC_ROW_BITS = 26;              // of the packed key: rows below 2^26 (MI_SCAN_CONTEXT_MAX_ROWS), 6 bits of shift
constexpr int SC_NO_INDEX = 0x7fffffff;      // *bad while nothing has been refused
struct ScBinArgs {
    const float* xyz;                // all points, AoS
    const int* offsets;              // n_scans + 1
    const float* centres;            // 3 per scan, or null: the origin
    int n_scans, rings, sectors, slice;
    float z_offset;
    const double* ring_edge2;        // rings + 1 (mi_scan_context_tables)
    const double* sector_dir;        // 2 * sectors
    unsigned int* desc;              // n_scans * rings * sectors, zero before the launch: the bits of the fp32 descriptor
    int* bad;                        // SC_NO_INDEX before the launch: the lowest point with a coordinate that is not finite or above SC_MAX_ABS
};
hipError_t sc_bins(const ScBinArgs& a, int longest_scan, hipStream_t s);
// unit[row] = the descriptor with every column scaled to length 1 (an empty column stays +0), mask[row] bit j = column j is not empty;
// *bad = min(*bad, the lowest row with a negative or non-finite value)
hipError_t sc_normalise(const float* desc, int rows, int rings, int sectors, float* unit, unsigned long long* mask, int* bad, hipStream_t s);
struct ScSearchArgs {
    const float* q_unit; const unsigned long long* q_mask; int nq;
    const float* d_unit; const unsigned long long* d_mask; int nd;
    const int* limit;                // nq, or null: every query sees all nd rows
    const int* exclude;              // nq, or null: a row that query i does not see (the runner-up pass: the winner)
    int rings, sectors, chunk_len;
    unsigned long long* keys;        // nq, all ones before the launch
};
int sc_chunk_len(int nq, int nd, int cu_count);
hipError_t sc_search(const ScSearchArgs& a, hipStream_t s);
// idx / dist / shift from keys (all ones: -1, +inf, 0); second (may be null) from keys2 alone
hipError_t sc_finish(const unsigned long long* keys, const unsigned long long* keys2, int nq, int* idx, float* dist, int* shift, float* second, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K68-K72 TSDF map: posed scans fused into a sparse truncated signed distance field, and its surface read back as points with normals
// (tsdf_kernels.hip; driver: tsdf_api.hip; the arithmetic: tsdf_ray.hpp; the contract: mi_tsdf_integrate and mi_tsdf_extract in mi_slam.h).
//   K68 tsdf_samples:  one lane per ray, twice: the count of its surviving samples (with the input check and the occupied range, folded over
//                      the wave and merged by integer atomics), and behind K51's scan of the counts the fill: per sample the three axis keys
//                      and the fp64 value, at the position (ray, k) gives it.  No LDS, no scratch.
//   K69 tsdf_map_keys: one lane per row of the input map: its axis keys, in front of every sample.
//       The voxel filter's stable radix sort (one per axis) and head-flag scan (vox_rows) order the entries and find the voxels' runs: a
//       voxel's input row, then its samples in ascending (scan, point, k).
//   K70 tsdf_fuse:     one lane per voxel: the fp64 sum of its run in that order, the count, the fused row.
//   K71 tsdf_table:    one lane per row of a map: the observed voxels into the table of voxel_table.hpp.
//   K72 tsdf_crossings: one lane per row, twice: the count of its crossings, and behind K51's scan the fill of points and normals.
// ---------------------------------------------------------------------------------------------------------------
constexpr int TSDF_BLOCK = 256;              // rays, rows or voxels per workgroup of K68-K72: one per lane
constexpr int TSDF_NO_INDEX = 0x7fffffff;    // TsdfState's bad_* while nothing has been refused
// Device-resident facts of one mi_tsdf_integrate; the host sets the starts and reads it back once, behind the count pass.
struct TsdfState {
    int bad_point;                   // the lowest point with a coordinate that is not finite or above 1e18 in magnitude
    int bad_range;                   // the lowest point with a sample whose voxel coordinate is outside [-2^30, 2^30)
    int cmin[3], cmax[3];            // the occupied range of the surviving samples (INT_MAX / INT_MIN: none)
};
struct TsdfSampleArgs {
    const float* xyz;                // all points, AoS
    const long long* offsets;        // n_scans + 1
    const float* poses;              // 16 per scan, column-major, or null: identities
    int n_scans, rays;
    float origin[3], voxel, truncation, min_range, max_range;
    int half_steps;                  // S
    TsdfState* state;
    int* count;                      // rays: the count pass writes, the fill reads nothing of it
    // the fill alone:
    const long long* sample_off;     // rays + 1: K51's scan of count
    int base;                        // entries in front of the samples (the input map's rows)
    size_t entries;                  // base + all samples: the stride of axis_keys
    int cmin[3];                     // what the axis keys are taken from
    unsigned int *keys, *axis_keys;  // entries; 3 x entries
    int* vals;                       // entries: the identity
    double* value;                   // all samples: f
};
hipError_t tsdf_samples(const TsdfSampleArgs& a, bool fill, hipStream_t s);
hipError_t tsdf_map_keys(const int* coord, int nv, const int cmin[3], size_t entries, unsigned int* keys, unsigned int* axis_keys, int* vals, hipStream_t s);
struct TsdfFuseArgs {
    const int* sorted_idx;           // entries: the entry at every sorted position
    const int* run_start;            // rows + 1
    int rows, base;
    size_t entries;
    const unsigned int* axis_keys;
    int cmin[3];
    const double* value;
    const float *in_tsdf, *in_weight;   // base
    float max_weight;
    int* out_coord;                  // rows x 3
    float *out_tsdf, *out_weight;    // rows
};
hipError_t tsdf_fuse(const TsdfFuseArgs& a, hipStream_t s);
// the rows with weight >= min_weight into the table (2 slots per row, every slot free before the launch)
hipError_t tsdf_table(const int* coord, const float* weight, int nv, float min_weight, const VoxelTableView& t, unsigned long long* keys, int* vals, hipStream_t s);
struct TsdfCrossArgs {
    const int* coord; const float* tsdf; const float* weight; int nv;
    float origin[3], voxel, min_weight;
    VoxelTableView table;
    int* count;                      // nv: the count pass writes
    const long long* offsets;        // nv + 1 (the fill)
    float *out_xyz, *out_normals;    // 3 per crossing; out_normals may be null
    const unsigned char* use;        // null: every crossing.  K77's masks (the fill of mi_tsdf_mesh): bit a of use[i] keeps the crossing (i, a)
};
hipError_t tsdf_crossings(const TsdfCrossArgs& a, bool fill, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K73-K75 TSDF ray casting: the map's surface as seen from a pose, one depth, point and normal per ray (tsdf_kernels.hip; driver:
// tsdf_api.hip; the arithmetic: tsdf_cast.hpp; the contract: mi_tsdf_raycast in mi_slam.h).  The observed voxels are in K71's table.
//   K73 tsdf_blocks:        one lane per row of the map: the 8^3-voxel block of every observed voxel into a table of K71's packing and hash
//                           (keys alone), the new ones counted by an integer atomic.
//   K74 tsdf_blocks_dilate: one lane per slot of K73's table: a held block marks itself and its 26 neighbours in a second table, sized from
//                           K73's count.  A block that is NOT in it has no observed voxel within 8 voxels of any of its own.
//   K75 tsdf_cast_rays:     one lane per ray: the direction turned by the pose, the march over the samples with one look-up each -- and,
//                           with skipping on, a look-up in K74's table where a sample is unobserved, 14 samples stepped over where the block
//                           is unmarked -- then, for a hit, the trilinear refinement (16 look-ups) and the normal (12).  Hits are counted over
//                           the wave and added once per wave.  No LDS, no scratch, no floating-point atomic.
// ---------------------------------------------------------------------------------------------------------------
// the blocks of the observed rows into the table t (keys all ones and *count 0 before the launch); t.cmin / t.ext are in blocks
hipError_t tsdf_blocks(const int* coord, const float* weight, int nv, float min_weight, const VoxelTableView& t, unsigned long long* keys, int* count, hipStream_t s);
// held: K73's table of `slots` slots with `blocks` keys; keys: mask + 1 >= 54 blocks slots, all ones before the launch, in the same frame
hipError_t tsdf_blocks_dilate(const unsigned long long* held, unsigned long long slots, int blocks, unsigned long long* keys, unsigned long long mask, hipStream_t s);
struct TsdfCastArgs {
    const float* dirs; int n;        // n x 3, the sensor's frame
    float pose[16]; int has_pose;    // column-major, sensor to world; has_pose 0: the identity
    float origin[3], voxel, min_range;
    int steps;                       // K
    const float* tsdf;               // the map's values by row
    VoxelTableView table;             // K71's
    VoxelTableView blocks;            // K74's (vals null; cmin / ext in blocks); read while skip != 0
    int skip;
    float* out_depth;                // n
    float *out_xyz, *out_normals;    // n x 3 each; either may be null
    int* hits;                       // 0 before the launch
};
hipError_t tsdf_cast_rays(const TsdfCastArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------
// K76-K78 TSDF mesh: the map's surface as an indexed triangle mesh by marching cubes (tsdf_kernels.hip; driver: tsdf_api.hip; the table:
// tsdf_mesh_table.hpp, generated by tools/gen_mc_table.py; the contract: mi_tsdf_mesh in mi_slam.h).  The observed voxels are in K71's table;
// the vertices are K72's crossings, filled by K72's own fill behind K77's masks.
//   K76 tsdf_mesh_classify:  one lane per row: the seven other corners of its cube looked up, the case byte, and -- where all eight corners
//                            are observed and no crossed edge is saturated at both ends -- the row's number of triangles, from the table.
//   K77 tsdf_mesh_edges:     one lane per row: for each of its up to three crossings, whether one of the four cubes round that edge has a
//                            triangle: a gather over K76's counts (no atomic, no racing store).  A 3-bit mask and its population per row.
//       K51's scan, twice: the rows' vertices and the rows' triangles into 64-bit offsets.
//   K78 tsdf_mesh_triangles: one lane per row with triangles: every table edge becomes offset[owner row] + the rank of the edge's axis in
//                            the owner's mask.
// K76 and K78 stage the table (256 packed 64-bit rows, 2 KB) in LDS: every lane indexes it by its own case, which a scalar or constant read
// would serialise.  K78 also keeps each lane's eight corner rows in LDS ([corner][lane]: a lane's column is its own bank), because the table
// picks the corner at run time and a register array indexed so would go to scratch.  No scratch, no floating-point atomic, no atomic at all.
// ---------------------------------------------------------------------------------------------------------------
struct TsdfMeshArgs {
    const int* coord; const float* tsdf; const float* weight; int nv;
    float min_weight;
    VoxelTableView table;            // K71's
    unsigned char* cube_case;        // nv: K76 writes
    int* tri_count;                  // nv: K76 writes; > 0 exactly where the row's cube is meshed and has a triangle
    unsigned char* use;              // nv: K77 writes
    int* vert_count;                 // nv: K77 writes
    const long long* vert_off;       // nv + 1: K51's scan of vert_count (K78)
    const long long* tri_off;        // nv + 1: K51's scan of tri_count (K78)
    int* out_tri;                    // 3 per triangle (K78)
};
hipError_t tsdf_mesh_classify(const TsdfMeshArgs& a, hipStream_t s);
hipError_t tsdf_mesh_edges(const TsdfMeshArgs& a, hipStream_t s);
hipError_t tsdf_mesh_triangles(const TsdfMeshArgs& a, hipStream_t s);

// One per translation unit with kernels: loads that unit's code object (see the definitions).
hipError_t preload_nn_kernel();
hipError_t preload_nn_tree();
hipError_t preload_nn_grid();
hipError_t preload_icp_kernels();
hipError_t preload_icp_batch();
hipError_t preload_cpd_kernels();
hipError_t preload_cpd_batch();
hipError_t preload_cpd_fgt();
hipError_t preload_nicp_api();
hipError_t preload_prepare_api();
hipError_t preload_voxel_kernels();
hipError_t preload_knn_kernels();
hipError_t preload_normals_kernels();
hipError_t preload_outlier_kernels();
hipError_t preload_plane_kernels();
hipError_t preload_gicp_kernels();
hipError_t preload_fpfh_kernels();
hipError_t preload_match_kernels();
hipError_t preload_ransac_kernels();
hipError_t preload_ndt_kernels();
hipError_t preload_iss_kernels();
hipError_t preload_cluster_kernels();
hipError_t preload_segment_kernels();
hipError_t preload_fgr_kernels();
hipError_t preload_color_kernels();
hipError_t preload_mls_kernels();
hipError_t preload_radius_kernels();
hipError_t preload_eval_kernels();
hipError_t preload_pose_graph_kernels();
hipError_t preload_scan_context_kernels();
hipError_t preload_tsdf_kernels();

}  // namespace mislam
