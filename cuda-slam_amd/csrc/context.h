// Context object behind the opaque mi_ctx handle: device, stream, grow-only workspace, optional RCCL communicator,
// HIP-event profiling.  Shared by the ICP and CPD drivers.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <sys/resource.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mi_slam.h"
#include "cpd_kernels.h"
#include "call_buffers.hpp"
#include "devbuf.h"
#include "kernels.h"
#include "nn_grid.h"
#include "nn_tree.h"

namespace mislam {

void retire_buffers(struct ::mi_ctx* ctx);         // call right behind a synchronisation of ctx->stream, ctx->device current (devbuf.h: retire_later)

#define MI_NCCL(call)                                                                                      \
    do {                                                                                                   \
        ncclResult_t r_ = (call);                                                                          \
        if (r_ != ncclSuccess) {                                                                           \
            mislam::set_error("%s failed: %s (%s:%d)", #call, ncclGetErrorString(r_), __FILE__, __LINE__); \
            return MI_ERR_RCCL;                                                                            \
        }                                                                                                  \
    } while (0)

#define MI_TRY(call)             \
    do {                         \
        int rc_ = (call);        \
        if (rc_ != MI_OK) return rc_; \
    } while (0)

// The buffers of one cell grid (nn_grid.h): the fixed cloud's of a context, the cloud's of a k-NN call.  grid_reserve plans the grid over a cloud of
// m points with bounding box bbox (host), sizes the buffers and fills the view; grid_build_into enqueues the build of that view on `s`.  Two steps, so
// that a caller can look at the plan, and book the reserves' time, before anything is enqueued (nn_api.hip).
struct GridBuffers {
    DevBuf<float4> pts;                              // points sorted by cell
    DevBuf<unsigned int> start, fill, scan;          // cell offsets, build cursors, scan scratch
    DevBuf<unsigned int> slot_of;                    // point -> its slot in pts
    DevBuf<unsigned int> row_occ;                    // per cell: which of the 5 x 5 cell rows around it hold a point within reach (NnGridView::row_occ)
    DevBuf<unsigned char> near_tmp;                  // build scratch
};
int grid_reserve(GridBuffers& b, const float bbox[6], int m, int index_base, float points_per_cell, NnGridView* view);
int grid_build_into(GridBuffers& b, const NnGridView& view, const float* x, const float* y, const float* z, int m, hipStream_t s);

// Scratch of one Morton sort (morton_order, nn_tree.h); morton_args sizes it for m points and fills the sort's arguments (nn_api.hip).
struct MortonScratch {
    DevBuf<unsigned int> codes_in, codes_out;
    DevBuf<int> order_in;
    DevBuf<float> bbox;
    DevBuf<unsigned char> sort_temp;
};
int morton_args(MortonScratch& sc, const float* x, const float* y, const float* z, int m, int* order_out, MortonArgs* out);

// What every search over a cloud's cell grid needs before its own kernel runs (search_front.hip): the uploads, the input check, the cell grid
// over the cloud and the queries along their curve.  One instance per call that searches (mi_ctx::knn, normals, outlier).
struct SearchFrontBuffers {
    DevBuf<float> staging;                           // the cloud as uploaded (AoS); separate queries pass through it behind the cloud
    DevBuf<float> cx, cy, cz;                        // the cloud, SoA, the caller's order
    DevBuf<float> ux, uy, uz;                        // separate queries, SoA as uploaded (mi_knn_search alone)
    DevBuf<float> qx, qy, qz;                        // the queries along their curve (self mode: the cloud)
    DevBuf<float> range_lo_hi;                       // the input check's partials ...
    DevBuf<int> range_bad;
    DevBuf<KnnState> state;                          // ... and what the host reads back from it
    DevBuf<int> order;                               // sorted slot -> the caller's query index
    MortonScratch morton;                            // the queries' curve order
    GridBuffers cells;                               // the cell grid over the cloud
    hipEvent_t ev[2] = {nullptr, nullptr};           // around the call's search launch while profiling; destroyed by mi_ctx_destroy (search_front_destroy_events)
};

// What the pose loop of plane ICP, generalized ICP and NDT iterates on (pose_loop.hip).  One instance per registration (mi_ctx::plane, gicp, ndt):
// nothing is shared between calls.
struct PoseLoopBuffers {
    DevBuf<double> rows, parts;                      // one row of PLANE_ROW sums per 64 moving points; the slabs' sums
    DevBuf<PlaneState> state;
    DevBuf<int> out_idx;                             // the *_system call's out_idx
};

struct ProfileSpan {
    int kernel;
    hipEvent_t e0, e1;
};

struct CpdWorkspace;   // cpd_workspace.h
struct PrepState;      // prepare_api.hip

}  // namespace mislam

struct mi_ctx {
    int device = 0;
    std::vector<void*> retired;                          // outgrown device buffers waiting for the next drain of `stream` (retire_buffers)
    unsigned long long entered = 0;                      // entry points opened on this context so far (CtxScope): lets mi_selftest_cpd_last tell that nothing ran in between
    hipStream_t stream = nullptr;
    int rank = 0, world = 1;
    ncclComm_t comm = nullptr;
    mi_exchange_fn exchange = nullptr;                   // the caller's transport instead of RCCL (mi_ctx_create_exchange)
    void* exchange_user = nullptr;
    void* exchange_host = nullptr;                       // pinned staging for it
    size_t exchange_cap = 0;
    bool distributed() const { return comm != nullptr || exchange != nullptr; }
    int cu_count = 256;
    // developer switches, read ONCE at context creation (none changes a result)
    struct Tuning {
        int nn_force_mode = 0;                           // MISLAM_NN_MODE: force MI_NN_* whatever the call asks
        int nn_R = 2, nn_wgs = 0, nn_chunks = 0;         // MISLAM_NN_R / _WGS / _CHUNKS: K1 sources per lane, workgroup budget, target chunks
        float grid_points_per_cell = mislam::GRID_POINTS_PER_CELL;   // MISLAM_GRID_PPC
        int cpd_mfma = 1;                                // MISLAM_CPD_MFMA=0: VALU contraction instead of MFMA
        int cpd_trunc_cull = 1;                          // MISLAM_CPD_TRUNC_CULL=0: the hybrid mode's truncated E-step over every pair (round 4's kernels) instead of K7t
        int fgt_resume = 1;                              // MISLAM_FGT_RESUME=0: re-cluster the fixed cloud from scratch every E-step
        int grid_split_walks = -1;                       // MISLAM_GRID_SPLIT_WALKS=0 / 1 / 2: the fused search's helper waves: none / for every walk / only beside a scan (default: by size)
        int grid_deal_rows = -1;                         // MISLAM_GRID_DEAL_ROWS=0 / 1: K1g's leftover rows never / always dealt out one per lane (default: by size)
        int svd_ieee = 0;                                // MISLAM_SVD_IEEE=1: the 3 x 3 SVD of every solve in IEEE divisions and roots (svd3.hpp)
        int icp_fused_solve = 1;                         // MISLAM_ICP_FUSED_SOLVE=0: rows reduce and solve as two launches at every size
        int icp_ticket_solve = 1;                        // MISLAM_ICP_TICKET_SOLVE=0: above the one-workgroup size, rows reduce and solve as two launches
        int icp_pipeline = 1;                            // MISLAM_ICP_PIPELINE=0: every host check of mi_icp_run settles the pending iteration and drains the stream
        int fgt_two_streams = 1;                         // MISLAM_FGT_TWO_STREAMS=0: the fixed cloud's clustering of an FGT E-step on the main stream, behind the moving side's
        int fgt_lists_in_model = 1;                      // MISLAM_FGT_LISTS_IN_MODEL=0: the member lists of an FGT E-step by the three-launch counting sort (round 4) instead of inside the model kernel
        int fgt_coop_sweep = 1;                          // MISLAM_FGT_COOP_SWEEP=0: K-centre sweeps of clouds beyond 16 384 points as in rounds 1-4 (one workgroup / two launches per centre); 2: the cooperative kernel for every sweep
        int fgt_shard_queries = 1;                       // MISLAM_FGT_SHARD_QUERIES=0: the FGT / hybrid CPD modes run replicated on a multi-rank context, no collective (rounds 4-5)
        int fgt_model_splits = 1;                        // MISLAM_FGT_MODEL_SPLITS=0: one workgroup per cell in the FGT model build whatever the cells' sizes (rounds 1-4)
        float knn_points_per_cell = 0.f;                 // MISLAM_KNN_POINTS_PER_CELL: cell size of mi_knn_search's grid (0: the default for the call's k, knn_default_points_per_cell of search_front.hip)
        float outlier_radius_cell = 1.f;                 // MISLAM_OUTLIER_RADIUS_CELL: cell edge of mi_remove_outliers' radius grid and of mi_iss_keypoints' grid in radii (radius_points_per_cell, search_front.hip)
        int fgt_replay = 1;                              // MISLAM_FGT_REPLAY=0: sweep the moving cloud step by step every E-step (no guess replayed)
    } tune;

    // ---- a second lane for the loads (round 4): mi_icp_load uploads and indexes the FIXED cloud on `aux` (hierarchy) and `aux2` (cell grid)
    // while the moving cloud is uploaded and ordered on `stream`; the helpers enqueue on work_stream() and take their scratch from
    // scratch[lane], so two lanes never share a scratch buffer.  Everything else runs on `stream`.
    hipStream_t aux = nullptr, aux2 = nullptr;
    hipEvent_t aux_event[3] = {nullptr, nullptr, nullptr};
    hipStream_t lane_stream = nullptr;                   // null: `stream`
    int lane = 0;
    hipStream_t work_stream() const { return lane_stream ? lane_stream : stream; }
    struct LaneScratch {
        mislam::DevBuf<float> staging;                   // AoS upload/download staging
        mislam::MortonScratch morton;                    // (the fixed cloud's hierarchy and the moving cloud's ordering)
    } scratch[2];

    // ---- workspace shared by the drivers
    // pinned host staging of the cloud uploads (host_to_device): the runtime's own pageable-copy path stalls for 20-50 ms every
    // few dozen calls on this machine (tools/alloc_probe.cpp: median 0.36 ms, max 27 ms for 12 MB).  A ring of SLOTS pieces of
    // 1 MB, pinned once per context: a piece is copied in while the pieces before it are on their way -- 0.30 ms for 12 MB, every time
    struct PinnedRing {
        static constexpr int SLOTS = 16;
        static constexpr size_t PIECE = 1u << 20;
        char* buf = nullptr;
        hipEvent_t event[SLOTS] = {nullptr};             // recorded behind the last transfer out of slot k
        unsigned int busy = 0;                           // bit k: event[k] has been recorded and not waited for since
        unsigned int next = 0;
    } pin;
    float* h_scratch = nullptr;                          // 64 pinned floats for small read-backs
    mislam::DevBuf<float> bx, by, bz;                    // original moving cloud, SoA
    mislam::DevBuf<float> cx, cy, cz;                    // current (transformed) moving cloud, SoA
    mislam::DevBuf<float> ax, ay, az;                    // multi-GPU load scratch: the whole moving cloud in Hilbert order
    mislam::DevBuf<float> tx, ty, tz;                    // this rank's fixed-cloud shard, SoA (K1 scalar streams)
    mislam::DevBuf<float4> tgt4;                         // same shard as float4 (gathers)
    mislam::DevBuf<unsigned long long> keys;
    mislam::DevBuf<double> part_mom, part_err;           // per-workgroup partial sums of the NICP / CPD drivers
    struct WorkOrder {                                   // work order of the fused search (IcpSchedule)
        mislam::DevBuf<int> order, counters;
        mislam::DevBuf<int> ticket;                      // icp_rows_reduce_solve: summing workgroups that have arrived (a line of its own; 0 between launches)
        mislam::DevBuf<unsigned char> far;
        mislam::DevBuf<unsigned long long> lanes;        // per chunk: the lanes that walked (IcpSchedule::lanes)
    } sched;
    mislam::DevBuf<double> rows, rows_reduced;           // ICP: one row of 18 sums per 64 moving points (icp_rows.hpp), and <= 64 reduced rows
    mislam::DevBuf<int> idx_tmp;
    mislam::DevBuf<unsigned char> keep_tmp;
    mislam::IcpState* d_state = nullptr;
    mislam::IcpState* h_state = nullptr;                 // pinned
    hipEvent_t peek_event = nullptr;                     // behind the state copy of an intermediate host check (mi_icp_run)

    // ---- exact-NN indexes over the fixed-cloud shard (built lazily, valid until the shard is replaced)
    struct TreeIndex {                                   // box hierarchy (nn_tree.h)
        mislam::DevBuf<int> order_out;                   // the hierarchy's own Morton order (a lane's scratch holds only what a sort consumes)
        mislam::DevBuf<float4> pts, boxes;               // sorted points and node boxes (build scratch)
        mislam::DevBuf<float4> leaf;                     // what the walk reads (NnTreeView): leaf coordinates, ...
        mislam::DevBuf<int> idx;                         // ... global indices ...
        mislam::DevBuf<float> boxes6;                    // ... and node boxes, six floats each
        mislam::NnTreeView view{};
        bool valid = false;
    } tree;
    struct GridIndex {                                   // cell grid (nn_grid.h)
        mislam::GridBuffers cells;
        mislam::DevBuf<float> bbox;                      // (its own: a Morton sort's bounding box may be in flight on another lane)
        mislam::DevBuf<unsigned int> match_slot;         // fused ICP: per moving point, the slot of its current match
        mislam::NnGridView view{};
        bool valid = false;
    } grid;
    mislam::DevBuf<int> sorder;                          // Morton order of the moving cloud (sorted slot -> caller's index)
    mislam::DevBuf<int> sinv;                            // its inverse (caller's index -> sorted slot), MI_SUM_CPU_SEQUENTIAL only
    mislam::DevBuf<float> resid;                         // per-slot squared residuals, same mode

    // ---- mi_icp_register_batch / mi_cpd_register_batch: both concatenated arrays as uploaded (AoS) and the "still running" word (shared);
    // every ICP problem's sorted moving cloud; per method the problem table and one state block per problem (icp_batch.hip, cpd_batch.hip)
    struct BatchBuffers {
        mislam::DevBuf<float> before, after, sx, sy, sz;
        mislam::DevBuf<mislam::IcpBatchProblem> problems;
        mislam::DevBuf<mislam::IcpState> states;
        mislam::DevBuf<mislam::CpdBatchProblem> cpd_problems;
        mislam::DevBuf<mislam::CpdState> cpd_states;
        mislam::DevBuf<int> running;
    } bat;

    // ---- mi_voxel_downsample: buffers of its own (a loaded ICP problem survives the call); what each one holds: VoxArgs, kernels.h
    struct VoxelBuffers {
        mislam::DevBuf<float> staging, x, y, z, range_lo_hi, out_xyz;
        mislam::DevBuf<float4> pts;
        mislam::DevBuf<unsigned int> keys_a, keys_b, axis_keys;
        mislam::DevBuf<int> vals_a, vals_b, range_bad, block_heads, row_of, run_start, fix, out_count, out_coord, voxel_of_point;
        mislam::DevBuf<double> front, back;
        mislam::DevBuf<unsigned char> sort_temp;
        mislam::DevBuf<mislam::VoxState> state;
        double ms[MI_VOXEL_STAGES] = {0};                // mi_voxel_downsample_times
    } vox;

    // ---- mi_knn_search, mi_estimate_normals, mi_remove_outliers: each call has a search front end (SearchFrontBuffers) and results of its own,
    // so that none leaves anything in another's buffers, and a loaded ICP problem survives all three
    struct KnnBuffers {
        mislam::SearchFrontBuffers front;
        mislam::DevBuf<float> out_d2;
        mislam::DevBuf<int> out_idx, out_count;
        double ms[MI_KNN_STAGES] = {0};                  // mi_knn_search_times
    } knn;
    struct NormalsBuffers {
        mislam::SearchFrontBuffers front;
        mislam::DevBuf<float> out_normals, out_curvature;
        mislam::DevBuf<int> out_count;
        double ms[MI_NORMALS_STAGES] = {0};              // mi_estimate_normals_times
    } normals;
    struct OutlierBuffers {
        mislam::SearchFrontBuffers front;                // (front.staging, the cloud as uploaded, is what the compaction gathers from)
        mislam::DevBuf<float> out_xyz, out_mean;
        mislam::DevBuf<int> count, tile_counts, out_index;
        mislam::DevBuf<double> score, partials;          // the unrounded scores; one partial sum per workgroup of a statistics pass
        mislam::DevBuf<unsigned char> keep;              // the flags, the caller's order
        mislam::DevBuf<mislam::OutlierState> ostate;
        double ms[MI_OUTLIER_STAGES] = {0};              // mi_remove_outliers_times
    } outlier;

    // ---- mi_iss_keypoints: OutlierBuffers' sibling -- a search front end in self mode, K32's per-point results, K33's flags and their compaction
    struct IssBuffers {
        mislam::SearchFrontBuffers front;                // (front.staging, the cloud as uploaded, is what the compaction gathers from)
        mislam::DevBuf<float> saliency, eigenvalues, out_xyz;
        mislam::DevBuf<int> neighbours, tile_counts, out_index;
        mislam::DevBuf<unsigned char> flag;              // is_keypoint, the caller's order
        mislam::DevBuf<mislam::OutlierState> ostate;     // (kept: the number of keypoints)
        double ms[MI_ISS_STAGES] = {0};                  // mi_iss_keypoints_times
    } iss;

    // ---- mi_mls_smooth: a search front end over the cloud with the queries beside it (the cloud itself, or a cloud of their own) and K50's
    // per-query results
    struct MlsBuffers {
        mislam::SearchFrontBuffers front;
        mislam::DevBuf<float> out_xyz, out_normals, out_curvature;
        mislam::DevBuf<int> out_neighbours;
        mislam::DevBuf<unsigned char> out_status;
        double ms[MI_MLS_STAGES] = {0};                  // mi_mls_smooth_times
    } mls;

    // ---- mi_radius_search: MlsBuffers' sibling -- a search front end over the cloud with the queries beside it, the rows' lengths, the scan's
    // tile sums, the 64-bit offsets and, once their length is known, the lists: packed keys, and what K54 unpacks them into
    struct RadiusBuffers {
        mislam::SearchFrontBuffers front;
        mislam::DevBuf<int> count;                       // n, the caller's row order
        mislam::DevBuf<long long> tile_sums, offsets;    // radius_scan_tiles(n); n + 1
        mislam::DevBuf<unsigned long long> keys;         // offsets[n]
        mislam::DevBuf<int> out_idx;
        mislam::DevBuf<float> out_d2;
        mislam::DevBuf<int> mismatch;                    // [0]: a fill walk disagreed with its count (RadiusFillArgs::mismatch)
        int grid_dims[3] = {0, 0, 0};                    // the last call's cell grid (mi_selftest_radius_grid)
        double ms[MI_RADIUS_STAGES] = {0};               // mi_radius_search_times
    } radius;

    // ---- mi_cluster_dbscan: a search front end in self mode, the core count, the union-find's parents, every point's root, the clusters' sizes,
    // the flags and scan tiles of the two compactions (the surviving roots; the labelled points) and the grouping's sort
    struct ClusterBuffers {
        mislam::SearchFrontBuffers front;
        mislam::DevBuf<int> count, parent, root_of, size, rank, roots, labels, tile_counts, sizes_out;
        mislam::DevBuf<unsigned char> keep, labelled, core;
        mislam::DevBuf<mislam::OutlierState> ostate;     // [0] kept: the surviving clusters; [1] kept: the labelled points
        mislam::DevBuf<unsigned int> keys_a, keys_b;     // the grouping: labels of the labelled points, ping and pong
        mislam::DevBuf<int> group_a, group_b;            // ... and their indices
        mislam::DevBuf<unsigned char> sort_temp;
        double ms[MI_CLUSTER_STAGES] = {0};              // mi_cluster_dbscan_times
    } cluster;

    // ---- mi_segment_plane, mi_segment_plane_hypotheses: a search front end for its upload and input check (front.staging is the cloud as
    // uploaded, what the peel gathers from), the labels and "still without a plane" flags in the caller's order, the remaining points by
    // rank, one row per hypothesis, and two sets of flags and terms by rank: the plane that stands and the one on trial
    struct SegmentBuffers {
        mislam::SearchFrontBuffers front;
        mislam::DevBuf<int> labels, rem_index, tile_counts, triples, inlier_count, nvalid;
        mislam::DevBuf<unsigned char> keep, valid, mask[2];
        mislam::DevBuf<float> rem_xyz, plane4, plane;    // plane: the 4 floats K41 reads
        mislam::DevBuf<double> s2[2], sums;              // sums: SEGMENT_SUMS
        mislam::DevBuf<unsigned long long> best;
        mislam::DevBuf<mislam::OutlierState> ostate;     // (kept: the remaining points)
        double ms[MI_SEGMENT_STAGES] = {0};              // mi_segment_plane_times
    } segment;

    // ---- mi_icp_plane_register, mi_plane_system: a search front end over the FIXED cloud with the moving cloud as its queries, the fixed
    // cloud's normals, the rows of an iteration's sums and the loop's state block -- a sibling of the three above, nothing shared with mi_icp_*
    struct PlaneBuffers {
        mislam::SearchFrontBuffers front;
        mislam::DevBuf<float> nx, ny, nz;                // the normals, SoA, the caller's order (what their input check reads)
        mislam::DevBuf<float4> normals;                  // the same, packed (what the step kernel gathers)
        mislam::DevBuf<mislam::KnnState> nstate;         // the normals' input check
        mislam::PoseLoopBuffers loop;
        double ms[MI_PLANE_STAGES] = {0};                // mi_icp_plane_times
    } plane;

    // ---- mi_evaluate_registration: PlaneBuffers' sibling without normals -- a search front end over the FIXED cloud with the moving cloud as
    // its queries, the rows of the one linearisation and the state block, the pairs' distances, and with the pairs given the caller's
    // pair_idx and the lowest refused entry
    struct EvalBuffers {
        mislam::SearchFrontBuffers front;
        mislam::PoseLoopBuffers loop;
        mislam::DevBuf<float> out_d2;
        mislam::DevBuf<int> pair_idx;                    // as uploaded, the caller's order
        mislam::DevBuf<int> pair_bad;                    // [0] the lowest index of an entry outside {-1} and [0, m), or KNN_NO_POINT
        double ms[MI_EVAL_STAGES] = {0};                 // mi_evaluate_registration_times
    } eval;

    // ---- mi_pose_graph_optimize, mi_pose_graph_system: the graph as uploaded (poses of 12 numbers, the edges' endpoints, flags, measurements
    // and information triangles), the incidence lists and their sort, the edge terms of the linearisation and the weights of the candidate,
    // the nodes' diagonal blocks and gradients, the inner solve's vectors and partial sums, and the state block
    struct PoseGraphBuffers {
        mislam::DevBuf<double> poses, candidate;         // 12 V each
        mislam::DevBuf<int> src, tgt, list, list_tmp, offsets, long_nodes;
        mislam::DevBuf<unsigned char> uncertain;
        mislam::DevBuf<double> Z, L;                     // [12][E], [21][E]
        mislam::DevBuf<unsigned int> keys_a, keys_b;
        mislam::DevBuf<unsigned char> sort_temp;
        mislam::DevBuf<double> r, chi2, w, M, h;         // the edge terms (PgTerms)
        mislam::DevBuf<double> chi2_c, w_c;              // ... of the candidate pass
        mislam::DevBuf<double> cost_parts;
        mislam::DevBuf<double> diag, grad;               // [21][V], [6][V]
        mislam::DevBuf<double> x, pr, pz, pp, pq, pq_node, parts, user_p, hp;
        mislam::DevBuf<mislam::PgState> state;
        double ms[MI_POSE_GRAPH_STAGES] = {0};           // mi_pose_graph_times
    } pose_graph;

    // ---- mi_scan_context, mi_scan_context_search: the points, offsets and centres of the scans with the two tables and the descriptors; the
    // two descriptor arrays of a search, their unit columns and masks, the limits, the packed winners (and runners-up) and the outputs
    struct ScanContextBuffers {
        mislam::DevBuf<float> xyz, centres, out_desc;
        mislam::DevBuf<int> offsets;
        mislam::DevBuf<double> tables;                   // rings + 1 squared ring edges, then 2 * sectors boundary directions
        mislam::DevBuf<float> query, db, q_unit, d_unit;
        mislam::DevBuf<unsigned long long> q_mask, d_mask, keys, keys2;
        mislam::DevBuf<int> limit;
        mislam::DevBuf<int> bad;                         // [0] the points' or the queries', [1] the database's lowest refused index, or SC_NO_INDEX
        mislam::DevBuf<int> out_idx, out_shift;
        mislam::DevBuf<float> out_dist, out_second;
        double ms[MI_SCAN_CONTEXT_STAGES] = {0};         // mi_scan_context_times
    } scan_context;

    // ---- mi_tsdf_integrate: the scans, offsets and poses as uploaded, the input map, the rays' counts and K51's scan of them, the entries'
    // keys, values and the sort's ping and pong, the voxel filter's head-flag scan, and the fused rows; mi_tsdf_extract: the map as uploaded,
    // the table of its observed voxels, the rows' counts and their scan, the points and normals; mi_tsdf_raycast: the map and that table again,
    // the directions in xyz, the two block tables of the skip, the counts, and a depth, a point and a normal per ray; mi_tsdf_mesh: the
    // extraction's, with the cubes' cases and triangle counts, the rows' masks, a second scan and the triangles
    struct TsdfBuffers {
        mislam::DevBuf<float> xyz, poses, in_tsdf, in_weight;
        mislam::DevBuf<long long> offsets, tile_sums, sample_off;
        mislam::DevBuf<int> in_coord, count;
        mislam::DevBuf<mislam::TsdfState> state;
        mislam::DevBuf<unsigned int> keys_a, keys_b, axis_keys;
        mislam::DevBuf<int> vals_a, vals_b, block_heads, row_of, run_start;
        mislam::DevBuf<unsigned char> sort_temp;
        mislam::DevBuf<mislam::VoxState> vstate;         // (rows: the voxels of the output)
        mislam::DevBuf<double> value;
        mislam::DevBuf<int> out_coord;
        mislam::DevBuf<float> out_tsdf, out_weight;
        mislam::DevBuf<unsigned long long> hkeys;
        mislam::DevBuf<int> hvals;
        mislam::DevBuf<float> out_xyz, out_normals;
        mislam::DevBuf<unsigned long long> block_held, block_keys;       // mi_tsdf_raycast: K73's and K74's tables
        mislam::DevBuf<int> cast_counts;                 // [0] the blocks K73 found, [1] the hits
        mislam::DevBuf<float> out_depth;
        mislam::DevBuf<unsigned char> mesh_case, mesh_use;               // mi_tsdf_mesh: K76's case bytes, K77's used-crossing masks
        mislam::DevBuf<int> mesh_tris, out_tri;          // the rows' triangle counts; the triangles
        mislam::DevBuf<long long> tri_off;               // K51's scan of mesh_tris (the vertices' scan is sample_off)
        double ms[MI_TSDF_STAGES] = {0};                 // mi_tsdf_times
    } tsdf;

    // ---- mi_estimate_covariances: mi_estimate_normals' sibling with six floats per point as its result, in buffers of its own
    struct CovarianceBuffers {
        mislam::SearchFrontBuffers front;
        mislam::DevBuf<float> out_cov;
        mislam::DevBuf<int> out_count;
        double ms[MI_NORMALS_STAGES] = {0};              // (the stages of mi_estimate_normals_times; no entry point reads them yet)
    } cov;

    // ---- mi_icp_gicp_register, mi_gicp_system: PlaneBuffers' sibling -- a search front end over the FIXED cloud with the moving cloud as its
    // queries, both clouds' covariances, the rows of an iteration's sums and the loop's state block (K16's layout: its reduce and solve run on them)
    struct GicpBuffers {
        mislam::SearchFrontBuffers front;
        mislam::DevBuf<float> cov_staging;               // a cloud's covariances as uploaded, six floats each
        mislam::DevBuf<float4> cov_a;                    // the fixed cloud's, two float4 each, the caller's order (what the step kernel gathers)
        mislam::DevBuf<float4> cov_b_in, cov_b;          // the moving cloud's: the caller's order, and along the curve (what the step kernel streams)
        mislam::DevBuf<int> cov_bad;                     // [0] the moving, [1] the fixed cloud's lowest refused covariance, or KNN_NO_POINT
        mislam::PoseLoopBuffers loop;
        double ms[MI_GICP_STAGES] = {0};                 // mi_icp_gicp_times
    } gicp;

    // ---- mi_estimate_color_gradients: mi_fpfh_features' front end -- self mode, the normals beside the cloud -- with the intensities beside
    // them and three floats per point as its result
    struct ColorGradientBuffers {
        mislam::SearchFrontBuffers front;
        mislam::DevBuf<float> nx, ny, nz;                // the normals, SoA, the caller's order
        mislam::DevBuf<mislam::KnnState> nstate;         // the normals' input check
        mislam::DevBuf<float> intensity;                 // as uploaded, the caller's order
        mislam::DevBuf<int> bad;                         // [0] the lowest refused intensity, or KNN_NO_POINT
        mislam::DevBuf<float> out_gradients;
        mislam::DevBuf<int> out_count;
        double ms[MI_NORMALS_STAGES] = {0};              // (the stages of mi_estimate_normals_times; no entry point reads them yet)
    } colorgrad;

    // ---- mi_icp_color_register, mi_color_system: PlaneBuffers' sibling -- a search front end over the FIXED cloud with the moving cloud as its
    // queries, the fixed cloud's normals, gradients and intensities, the moving cloud's intensities, the rows of an iteration's sums and the
    // loop's state block (K16's layout: its reduce and solve run on them)
    struct ColorBuffers {
        mislam::SearchFrontBuffers front;
        mislam::DevBuf<float> nx, ny, nz;                // the normals, SoA, the caller's order (what their input check reads)
        mislam::DevBuf<float4> normals;                  // the same, packed (what the step kernel gathers)
        mislam::DevBuf<mislam::KnnState> nstate;         // the normals' input check
        mislam::DevBuf<float> ia_in, grad_in;            // the fixed cloud's intensities and gradients as uploaded
        mislam::DevBuf<float4> grad_i;                   // ... packed, (g_x, g_y, g_z, I), the caller's order (what the step kernel gathers)
        mislam::DevBuf<float> ib_in, ib;                 // the moving cloud's intensities: the caller's order, and along the curve (what the step kernel streams)
        mislam::DevBuf<int> bad;                         // [0] before_intensity, [1] after_intensity, [2] after_gradients_xyz: the lowest refused index, or KNN_NO_POINT
        mislam::PoseLoopBuffers loop;
        double ms[MI_COLOR_STAGES] = {0};                // mi_icp_color_times
    } color;

    // ---- mi_fpfh_features: a search front end in self mode, the normals beside the cloud, what K18 leaves for K19 and the results
    struct FpfhBuffers {
        mislam::SearchFrontBuffers front;
        mislam::DevBuf<float> nx, ny, nz;                // the normals, SoA, the caller's order
        mislam::DevBuf<mislam::KnnState> nstate;         // the normals' input check
        mislam::DevBuf<unsigned long long> keys;         // every point's sorted k-list (FpfhSpfhArgs::keys)
        mislam::DevBuf<unsigned int> packed;             // every point's packed counts (FPFH_WORDS each)
        mislam::DevBuf<float> out_fpfh;
        mislam::DevBuf<unsigned char> out_counts;
        mislam::DevBuf<int> out_count;
        double ms[MI_FPFH_STAGES] = {0};                 // mi_fpfh_features_times
    } fpfh;

    // ---- mi_feature_match: both descriptor arrays as uploaded, their norms, the packed minima of both directions and the results
    struct MatchBuffers {
        mislam::DevBuf<float> query, target, qq, tt;
        mislam::DevBuf<int> bad;                         // [0] the queries', [1] the targets' lowest refused row, or MATCH_NO_ROW
        mislam::DevBuf<unsigned long long> keys, rev_keys;
        mislam::DevBuf<int> out_idx;
        mislam::DevBuf<float> out_d2;
        double ms[MI_MATCH_STAGES] = {0};                // mi_feature_match_times
    } match;

    // ---- mi_ransac_register, mi_ransac_hypotheses: the correspondences by rank, one row per hypothesis, and the final pose's flags and distances
    struct RansacBuffers {
        mislam::DevBuf<float> pairs6, pose12, pose;
        mislam::DevBuf<int> src_index, triples, inlier_count, small;   // small: [0] valid hypotheses, [1] the final pose's inliers
        mislam::DevBuf<unsigned char> valid, mask;
        mislam::DevBuf<unsigned long long> best;
        mislam::DevBuf<double> d2, sum;
        double ms[MI_RANSAC_STAGES] = {0};               // mi_ransac_register_times
    } ransac;

    // ---- mi_fgr_register, mi_fgr_tuples, mi_fgr_system: both clouds packed as uploaded (x, y, z and the range partials are scratch of their
    // upload and check, one cloud after the other), the matches by rank, one row per tuple trial with the flags' compaction, the used
    // list (indices and points by used rank), the weights, the step's mu, and K16's rows and state block
    struct FgrBuffers {
        mislam::DevBuf<float> staging, x, y, z, range_lo_hi, weights;
        mislam::DevBuf<float4> src4, tgt4, used_p, used_q;
        mislam::DevBuf<int> range_bad, match_src, match_tgt, triples, kept_trials, tile_counts, used_src, used_tgt;
        mislam::DevBuf<unsigned char> accept;
        mislam::DevBuf<mislam::KnnState> kstate;         // [0] the source's, [1] the target's bounding box and lowest refused point
        mislam::DevBuf<mislam::OutlierState> ostate;     // (kept: the accepted trials)
        mislam::DevBuf<double> mu;                       // [0]: the mu of the last linearisation that ran
        mislam::PoseLoopBuffers loop;
        double ms[MI_FGR_STAGES] = {0};                  // mi_fgr_register_times
    } fgr;

    // ---- mi_ndt_voxels: the voxel filter's buffers once more (its front end runs on them: voxel_front_run), the scatter's partials and the results;
    // mi_ndt_register, mi_ndt_system: the moving cloud and its curve order, the listed voxels, their table, K16's rows and state block
    struct NdtBuffers {
        VoxelBuffers vox;
        mislam::DevBuf<double> q6, front, back;
        mislam::DevBuf<int> fix;
        mislam::DevBuf<float> icov, cov;
        double voxel_ms[8] = {0};                        // (the stages of mi_voxel_downsample_times; no entry point reads them yet)
        mislam::DevBuf<float> staging, ux, uy, uz, qx, qy, qz, range_lo_hi;
        mislam::DevBuf<int> range_bad, order;
        mislam::DevBuf<mislam::KnnState> kstate;         // the moving cloud's input check
        mislam::MortonScratch morton;
        mislam::DevBuf<int> vcoord, hvals;
        mislam::DevBuf<float> vmean, vicov;              // the listed voxels as uploaded
        mislam::DevBuf<float4> mean4, icov4;             // ... and packed (what the step kernel gathers)
        mislam::DevBuf<mislam::NdtMapState> mstate;
        mislam::DevBuf<unsigned long long> hkeys;
        mislam::PoseLoopBuffers loop;
        mislam::DevBuf<unsigned char> out_terms;         // mi_ndt_system's out_terms
        double ms[MI_NDT_STAGES] = {0};                  // mi_ndt_times
    } ndt;

    // ---- mi_prepare_cloud: buffers of its own, like the voxel call's: the raw cloud, the prepared one, the caller's index vectors and draws
    struct PrepareBuffers {
        mislam::DevBuf<float> raw, out, partials, noise_unit, outlier_unit;
        mislam::DevBuf<int> sub, shuffle, rows;
        mislam::DevBuf<mislam::PrepState> state;
    } prep;

    // ---- ICP problem currently loaded
    struct IcpProblem {
        bool icp_loaded = false;
        int n = 0, n_pad = 0;
        int n_global = 0;                                // moving points over ALL ranks (what rank-independent decisions are taken from)
        int m_total = 0, shard_lo = 0, shard_hi = 0;
        bool source_sharded = false;                     // MI_SHARD_SOURCE in effect: n = this rank's slice, fixed cloud replicated
        bool fused = false;                              // the grid search carries the O(N) part of the iteration (nn_grid.hip)
        int enqueued_passes = 0;                         // fused iterations enqueued since the load / reset (GridSearchArgs::extend_reach)
        mi_icp_params icp{};
        double load_ms[MI_LOAD_STAGES] = {0};            // mi_icp_load_times
    } prob;

    // ---- CPD workspace (allocated on first use)
    mislam::CpdWorkspace* cpd = nullptr;

    // ---- profiling
    mislam::DevBuf<unsigned long long> nn_stats;         // mi_profile_search_stats counters
    bool nn_stats_on = false;
    int selftest_fail_loads = 0;                         // mi_selftest_fail_loads: the next N index builds fail on purpose (an explicit call of a test, never the environment: ADVICE r05)
    struct Profiler {                                    // HIP events on the context's stream `s` around each kernel launch
        bool on = false;
        unsigned int mask = 0xffffffffu;                 // kernels that get events while profiling (mi_profile_select)
        std::vector<mislam::ProfileSpan> spans;
        std::vector<hipEvent_t> event_pool;
        double ms[MI_KERNEL_COUNT] = {0};
        long long n[MI_KERNEL_COUNT] = {0};
        bool times(int kernel) const { return on && ((mask >> kernel) & 1u); }
        int begin(int kernel, hipStream_t s);
        int end(hipStream_t s);
        int span(int kernel, hipEvent_t* e0, hipEvent_t* e1);   // a span whose events the LAUNCH records (hipExtLaunchKernelGGL); null events if `kernel` is not being timed
        int collect(hipStream_t s);
    } prof;
};

namespace mislam {

// Every entry point that works on a context opens one: the context's device becomes current and buffers outgrown during the call
// are retired into the context's own list.  On the way out, whatever is on that list is released if the stream happens to be
// drained (the entry points that return host results end in a synchronisation), else it waits for the next one.
struct CtxScope {
    mi_ctx* ctx;
    std::vector<void*>* outer;
    explicit CtxScope(mi_ctx* c);
    ~CtxScope();
    CtxScope(const CtxScope&) = delete;
    CtxScope& operator=(const CtxScope&) = delete;
};
#define MI_ENTER(c)                          \
    MI_HIP(hipSetDevice((c)->device));       \
    mislam::CtxScope mi_ctx_scope_(c)

// the helpers called inside enqueue on `s` and use scratch set `lane` (mi_ctx::work_stream)
struct LaneScope {
    mi_ctx* c;
    LaneScope(mi_ctx* ctx, hipStream_t s, int lane) : c(ctx) { c->lane_stream = s; c->lane = lane; }
    ~LaneScope() { c->lane_stream = nullptr; c->lane = 0; }
};

struct ProfScope {
    mi_ctx* c;
    bool on;
    ProfScope(mi_ctx* ctx, int kernel) : c(ctx), on(ctx->prof.times(kernel)) { if (on) (void)c->prof.begin(kernel, c->stream); }
    ~ProfScope() { if (on) (void)c->prof.end(c->stream); }
};

// Host wall time per stage of a call, into the eight slots of ms (mi_icp_load_times, mi_voxel_downsample_times, mi_knn_search_times, mi_estimate_normals_times, mi_remove_outliers_times): mark(stage) books
// the time since the last mark to `stage` and the device allocations in it to slot 0; with profiling on, the stream is drained at every mark.
struct StageClock {
    mi_ctx* c;
    double* ms;
    double t_begin, t_mark, a_mark;
    StageClock(mi_ctx* ctx, double* stage_ms) : c(ctx), ms(stage_ms), t_begin(wall_ms()), t_mark(t_begin), a_mark(alloc_ms_counter())
    {
        for (int i = 0; i < 8; i++) ms[i] = 0.0;
    }
    int mark(int stage)
    {
        if (c->prof.on) MI_HIP(hipStreamSynchronize(c->stream));
        const double now = wall_ms(), a_now = alloc_ms_counter();
        ms[0] += a_now - a_mark;
        ms[stage] += (now - t_mark) - (a_now - a_mark);
        t_mark = now; a_mark = a_now;
        return MI_OK;
    }
    void finish() { ms[7] = wall_ms() - t_begin; }
};
static_assert(MI_LOAD_STAGES == 8 && MI_VOXEL_STAGES == 8 && MI_KNN_STAGES == 8 && MI_NORMALS_STAGES == 8 && MI_OUTLIER_STAGES == 8 && MI_PLANE_STAGES == 8 && MI_GICP_STAGES == 8 && MI_FPFH_STAGES == 8 && MI_MATCH_STAGES == 8 && MI_RANSAC_STAGES == 8 && MI_NDT_STAGES == 8 && MI_ISS_STAGES == 8 && MI_CLUSTER_STAGES == 8 && MI_SEGMENT_STAGES == 8 && MI_FGR_STAGES == 8 && MI_COLOR_STAGES == 8 && MI_MLS_STAGES == 8 && MI_RADIUS_STAGES == 8 && MI_EVAL_STAGES == 8 && MI_POSE_GRAPH_STAGES == 8 && MI_SCAN_CONTEXT_STAGES == 8 && MI_TSDF_STAGES == 8, "StageClock: eight slots, the last one the whole call");
// The body of every *_times entry point: the eight slots a StageClock left in the context.  ms: null for a null context.
static inline int stage_times(const char* who, const double* ms, double* out_ms)
{
    if (!ms || !out_ms) { set_error("%s: null argument", who); return MI_ERR_INVALID_ARG; }
    for (int i = 0; i < 8; i++) out_ms[i] = ms[i];
    return MI_OK;
}

// ---- the voxel filter's front end (voxel_api.hip), for mi_voxel_downsample and mi_ndt_voxels: the reserves, the upload, the range pass and its
// read-back with everything that can refuse the cloud (nothing has been written to a caller's array then), the keys, the sort, the rows and the
// segmented sums (stages 0 - 4 of mi_voxel_downsample_times).  Behind it *a names the arrays of b the kernels filled and *st (the context's
// pinned scratch) holds the range pass's facts; rows is not read back yet.
int voxel_front_run(mi_ctx* c, const char* who, mi_ctx::VoxelBuffers& b, StageClock& clock, const float* xyz, int n, float voxel_size, const float* origin3,
                    VoxArgs* a, VoxState** st);

// ---- the front end of a search over a cloud's cell grid (search_front.hip).  A driver calls, in this order: search_front_reserve and its own
// reserves (every reserve comes before the first upload), clock.mark(0), search_front_upload_and_check (stages 1 and 2: nothing has been written
// to a caller's array when it refuses), search_front_index_and_order with the points per cell it chose (stages 3 and 4; the plan's reserves to
// slot 0), search_front_fits beside the check of its own buffers, search_front_timed_launch (stage 5).  who: the entry point's name, for messages.
struct SearchFront {
    int n = 0, m = 0;                                // queries, cloud points
    const float *ux = nullptr, *uy = nullptr, *uz = nullptr;   // the queries as uploaded, SoA: the cloud's arrays in self mode
    float bbox[6] = {0};                             // of the cloud: lower corner, upper corner
    NnGridView g{};
    size_t n_cells = 0;
};
int search_front_reserve(SearchFrontBuffers& b, size_t n, size_t m, bool self);
// query_xyz null: self mode, the cloud is its own query set (n == m); cloud_name, query_name: what a refusal calls the two arrays
int search_front_upload_and_check(mi_ctx* c, SearchFrontBuffers& b, StageClock& clock, const char* who, const float* cloud_xyz, int m,
                                  const float* query_xyz, int n, SearchFront* f, const char* cloud_name = "cloud_xyz",
                                  const char* query_name = "query_xyz");
int search_front_index_and_order(mi_ctx* c, SearchFrontBuffers& b, StageClock& clock, const char* who, float points_per_cell, SearchFront* f);
// its second half alone, stage 4: the queries along their curve and no grid (mi_evaluate_registration with the pairs given: f->g stays empty,
// search_front_fits does not hold, and the driver checks q*, order and c* itself)
int search_front_order(mi_ctx* c, SearchFrontBuffers& b, StageClock& clock, SearchFront* f);
// What a search kernel is handed beside the grid f.g.  No driver reads these buffers for a launch itself, so search_front_fits, the host-side
// shape check of what every search kernel indexes (q*, order, c*, the grid's offsets and points), checks what was handed out.
SearchQueries search_front_queries(const SearchFrontBuffers& b, const SearchFront& f);
SearchCloud search_front_cloud(const SearchFrontBuffers& b);
bool search_front_fits(const SearchFrontBuffers& b, const SearchFront& f);
// A call with normals beside its cloud (m of them; mi_icp_plane_register, mi_fpfh_features) puts search_front_upload_and_check between these
// two.  enqueue: the normals go first through the staging buffer and the check's partials, which the front end then takes over (one stream:
// in order), into nx, ny, nz (and packed, unless null), checked into *nstate.  refuse: the one read-back of *nstate behind the front end's,
// stage 2, and the refusal of a normal with an unusable component; name: what it calls the array.
int search_front_enqueue_normals(mi_ctx* c, SearchFrontBuffers& b, const float* normals_xyz, int m, float* nx, float* ny, float* nz, float4* packed,
                                 KnnState* nstate);
int search_front_refuse_normals(mi_ctx* c, StageClock& clock, const char* who, const char* name, const KnnState* nstate);
void search_front_destroy_events(mi_ctx* c);         // of every call's front end (mi_ctx_destroy)
// Stage 5: `launch` enqueues the call's search kernel.  With profiling on, the slot holds the launch's own HIP-event time instead of the host's.
template <class Launch>
static inline int search_front_timed_launch(mi_ctx* c, SearchFrontBuffers& b, StageClock& clock, Launch&& launch)
{
    const bool timed = c->prof.on;
    if (timed) {
        for (hipEvent_t& e : b.ev)
            if (!e) MI_HIP(hipEventCreate(&e));
        MI_HIP(hipEventRecord(b.ev[0], c->stream));
    }
    MI_HIP(launch());
    if (timed) MI_HIP(hipEventRecord(b.ev[1], c->stream));
    MI_TRY(clock.mark(5));
    if (timed) {
        float ms = 0.f;
        MI_HIP(hipEventElapsedTime(&ms, b.ev[0], b.ev[1]));
        clock.ms[5] = (double)ms;
    }
    return MI_OK;
}

// ---- the tail of a call that compacts flags over its cloud (outlier_compact, kernels.h: mi_remove_outliers, mi_iss_keypoints; the two counts
// of mi_cluster_dbscan are read the same way).  compact_enqueue gathers the flagged rows of the cloud as uploaded (front.staging) and their
// indices, where asked for, and counts them into *state.  compact_read_state puts `blocks` state blocks on their way into the context's pinned
// scratch: a driver calls it once, with its per-point results, in front of their synchronisation; behind it compact_host_state is what came,
// compact_kept block i's count (false unless within [0, n]: the driver refuses in its own words) and compact_download the kept rows.
static_assert(2 * sizeof(OutlierState) <= 64 * sizeof(float), "two OutlierStates must fit the context's pinned scratch");
static inline int compact_enqueue(mi_ctx* c, const SearchFrontBuffers& front, const unsigned char* keep, int n, int* tile_counts, int* out_index,
                                  float* out_xyz, OutlierState* state)
{
    OutlierCompactArgs a{};
    a.keep = keep; a.xyz = front.staging.p; a.n = n; a.tile_counts = tile_counts;
    a.out_index = out_index; a.out_xyz = out_xyz; a.state = state;
    MI_HIP(outlier_compact(a, c->stream));
    return MI_OK;
}
static inline int compact_read_state(mi_ctx* c, const OutlierState* state, int blocks)
{
    MI_HIP(hipMemcpyAsync(c->h_scratch, state, (size_t)blocks * sizeof(OutlierState), hipMemcpyDeviceToHost, c->stream));
    return MI_OK;
}
static inline const OutlierState* compact_host_state(const mi_ctx* c) { return reinterpret_cast<const OutlierState*>(c->h_scratch); }
static inline bool compact_kept(const mi_ctx* c, int i, int n, long long* kept)
{
    *kept = compact_host_state(c)[i].kept;
    return *kept >= 0 && *kept <= (long long)n;
}
static inline int compact_download(mi_ctx* c, long long kept, float* out_xyz, const float* d_xyz, int* out_index, const int* d_index)
{
    if (kept <= 0) return MI_OK;
    if (out_xyz) MI_HIP(hipMemcpyAsync(out_xyz, d_xyz, sizeof(float) * 3 * (size_t)kept, hipMemcpyDeviceToHost, c->stream));
    if (out_index) MI_HIP(hipMemcpyAsync(out_index, d_index, sizeof(int) * (size_t)kept, hipMemcpyDeviceToHost, c->stream));
    if (out_xyz || out_index) MI_HIP(hipStreamSynchronize(c->stream));
    return MI_OK;
}

// ---- the pose loop of mi_icp_plane_register, mi_icp_gicp_register, mi_ndt_register and their *_system probes (pose_loop.hip; the host arithmetic:
// pose_block.hpp): everything behind "the step kernel's arguments are complete".  A driver calls pose_check_transform among its argument checks
// (and pose_check_fields behind them), pose_loop_reserve among its reserves (every reserve comes before the first upload), pose_loop_upload_state
// behind its last stage (it books stage 1), pose_loop_fits beside the check of its own buffers, and then either pose_loop_run and
// pose_loop_results, or pose_loop_system_run and pose_loop_system_finish.  `step` enqueues the driver's step kernel.
struct PoseLoopFields {
    float eps_rotation, eps_translation;
    int max_iterations, sync_every, verbose;
    const char* noun;                                // what the verbose line counts: "pairs" or "terms"
};
int pose_check_transform(const char* who, const float* T);                     // T null: nothing to refuse
int pose_check_fields(const char* who, const PoseLoopFields& p);
int pose_loop_reserve(PoseLoopBuffers& b, int n, bool want_idx);
bool pose_loop_fits(const PoseLoopBuffers& b, int n, bool want_idx);           // the host-side shape check of what the step and the reduce index
// *h = the block at pose T (null: the identity) about the fp32 centre, and its upload
int pose_loop_upload_state(mi_ctx* c, PoseLoopBuffers& b, StageClock& clock, const float* T, const float centre[3], PlaneState* h);
int pose_loop_read_state(mi_ctx* c, PoseLoopBuffers& b, PlaneState* h);        // the copy back and the wait for it
// stage 6 of a registration: out_T, iterations, error and stop_reason from the state
int pose_loop_results(StageClock& clock, const PlaneState& h, float out_T[16], int* iterations, float* error, int* stop_reason);
// stage 6 of a *_system call: the wait for the copies in flight, then out_sums and out_centre from the state
int pose_loop_system_finish(mi_ctx* c, StageClock& clock, const PlaneState& h, double out_sums[PLANE_ROW], float out_centre[3]);

// one iteration's launches: the step, then rows -> sums -> (rules.solve) solve, update, stop rule.  With profiling on, the step's time
// is booked to MI_KERNEL_NN and the other launches' to MI_KERNEL_SOLVE (mi_profile_get).
template <class Step>
static inline int pose_loop_iteration(mi_ctx* c, PoseLoopBuffers& b, int n, const PlaneRules& rules, Step&& step)
{
    const int nrows = plane_row_count(n);
    {
        ProfScope p(c, MI_KERNEL_NN);
        MI_HIP(step());
    }
    {
        ProfScope p(c, MI_KERNEL_SOLVE);
        MI_HIP(plane_reduce_solve(b.state.p, b.rows.p, nrows, plane_part_count(nrows) > 0 ? b.parts.p : nullptr, rules, c->stream));
    }
    return MI_OK;
}
// Stage 5 of a registration: batches of sync_every (0: 4) iterations between host reads of the state, until it says done.  The device enforces
// the iteration cap; the host never enqueues beyond it.
template <class Step>
static inline int pose_loop_run(mi_ctx* c, PoseLoopBuffers& b, StageClock& clock, const char* who, int n, const PoseLoopFields& p, PlaneState* h, Step&& step)
{
    PlaneRules rules{};
    rules.eps_rotation = (double)p.eps_rotation; rules.eps_translation = (double)p.eps_translation;
    rules.max_iterations = p.max_iterations; rules.solve = 1;
    const int batch = pose_batch(p.sync_every);
    int enqueued = 0;
    if (p.max_iterations == 0) { h->done = 1; h->stop_reason = MI_STOP_MAX_ITERATIONS; }
    while (!h->done) {
        if (enqueued >= p.max_iterations) { set_error("internal: %s ran %d iterations without a stop", who, enqueued); return MI_ERR_STATE; }
        const int todo = pose_batch_todo(batch, p.max_iterations, enqueued);
        for (int i = 0; i < todo; i++) MI_TRY(pose_loop_iteration(c, b, n, rules, step));
        enqueued += todo;
        MI_TRY(pose_loop_read_state(c, b, h));
        if (p.verbose)
            fprintf(stderr, "%s: %d enqueued, %d applied, |omega| %.3e |v| %.3e, %s %.0f, stop %d\n", who, enqueued, h->iterations, h->omega, h->v, p.noun,
                    h->sums[PLANE_ROW_COUNT], h->stop_reason);
    }
    return clock.mark(5);
}
// Stage 5 of a *_system call: one iteration with solve = 0 (the sums and nothing else), the state's read-back, and out_idx on its way
template <class Step>
static inline int pose_loop_system_run(mi_ctx* c, PoseLoopBuffers& b, StageClock& clock, int n, PlaneState* h, int* out_idx, Step&& step)
{
    MI_TRY(pose_loop_iteration(c, b, n, PlaneRules{}, step));
    MI_TRY(pose_loop_read_state(c, b, h));
    MI_TRY(clock.mark(5));
    if (out_idx) MI_HIP(hipMemcpyAsync(out_idx, b.out_idx.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    return MI_OK;
}

// developer switch MISLAM_DEV_STALL_MS=<ms>: report any host-side section that takes longer, with the calling thread's context switches
// over it -- an INVOLUNTARY one with no voluntary ones means the thread was taken off its core (a CPU quota of the container
// running out: numpy's BLAS pool spinning on every host core did exactly that to the round-2 sweeps), not that the GPU or the
// runtime made it wait.
extern double g_stall_ms;
struct StallProbe {
    const char* label; double t0; struct rusage ru0;
    explicit StallProbe(const char* l) : label(l), t0(0.0) { if (g_stall_ms > 0) { t0 = wall_ms(); getrusage(RUSAGE_THREAD, &ru0); } }
    ~StallProbe()
    {
        if (g_stall_ms <= 0) return;
        const double d = wall_ms() - t0;
        if (d <= g_stall_ms) return;
        struct rusage ru1; getrusage(RUSAGE_THREAD, &ru1);
        fprintf(stderr, "mislam stall: %s %.2f ms (context switches: %ld voluntary, %ld involuntary)\n", label, d, ru1.ru_nvcsw - ru0.ru_nvcsw, ru1.ru_nivcsw - ru0.ru_nivcsw);
    }
};

static inline int round_up(int v, int g) { return (v + g - 1) / g * g; }
struct NnPlan { int R, n_chunks, chunk_len; };
NnPlan plan_nn(const mi_ctx* ctx, int n, int m_local);
size_t target_alloc_len(int m_local);

// Host -> device on the context's stream, through the context's pinned staging buffer for anything sizeable (returns at once;
// the caller's buffer may be reused as soon as this returns).
int host_to_device(mi_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
// Upload an AoS host cloud into SoA device arrays of n_pad entries (tail = copies of the last point).
int upload_soa(mi_ctx* ctx, const float* host_aos, int n, int n_pad, float* x, float* y, float* z, float4* packed);
// Uploads this rank's shard of the fixed cloud (SoA streams for K1 + float4 for gathers); invalidates the box hierarchy.
int upload_target_shard(mi_ctx* ctx, const float* after_xyz, int m_total, bool replicate = false);
int reserve_moving(mi_ctx* ctx, size_t n_pad, size_t c_pad);   // bx..bz and keys of n_pad entries, cx..cz of c_pad (>= n_pad where they double as load scratch)
// Morton-sorts the moving cloud; the two index builds over the resident fixed-cloud shard, no-ops while it is valid (nn_api.hip)
int sort_sources(mi_ctx* ctx, const float* sx, const float* sy, const float* sz, int n, int n_pad, float* dx, float* dy, float* dz);
int ensure_tree(mi_ctx* ctx, int m_local, int index_base);
int ensure_grid(mi_ctx* ctx, int m_local, int index_base);
// Correspondence search of n moving points (SoA, padded) against the loaded fixed-cloud shard into ctx->keys (K1, K1t or K1g).
int resolve_nn_mode(const mi_ctx* ctx, int nn_mode, int m_local);
GridSearchArgs grid_search_args(const mi_ctx* ctx, int n);   // the fields of a grid search that depend on the context and n alone: n, keys, stats, deal_rows
int launch_nn(mi_ctx* ctx, const float* sx, const float* sy, const float* sz, int n, int m_local, int index_base, int fma,
              const int* done_flag, int nn_mode);
int allreduce_keys(mi_ctx* ctx, int n);                      // min over the ranks of ctx->keys[0, n), under MI_KERNEL_ALLREDUCE
// In-place all-reduce of a device array over the ranks, on the context's stream: RCCL, or the caller's transport through pinned
// host memory.  No-ops on a single-GPU context.
int allreduce_min_u64(mi_ctx* ctx, unsigned long long* dev_ptr, size_t count);
int allreduce_sum_f64(mi_ctx* ctx, double* dev_ptr, size_t count);

// ---- host plumbing the batched calls share (mi_icp_register_batch, mi_cpd_register_batch)
// The points any batched problem of a call uses: [b_lo, b_hi) of the caller's moving array, [a_lo, a_hi) of the fixed one.
struct BatchSpan {
    long long b_lo = -1, b_hi = 0, a_lo = -1, a_hi = 0;
    void add(long long bo, long long bn, long long ao, long long an)
    {
        b_lo = b_lo < 0 || bo < b_lo ? bo : b_lo; b_hi = bo + bn > b_hi ? bo + bn : b_hi;
        a_lo = a_lo < 0 || ao < a_lo ? ao : a_lo; a_hi = ao + an > a_hi ? ao + an : a_hi;
    }
};
// One upload of each array (AoS, as it is, through the pinned ring) into ctx->bat.before / after; overlapping ranges travel once.
static inline int batch_upload_clouds(mi_ctx* c, const float* before_xyz, const float* after_xyz, const BatchSpan& sp)
{
    const size_t nbefore = (size_t)(sp.b_hi - sp.b_lo), nafter = (size_t)(sp.a_hi - sp.a_lo);
    MI_TRY(c->bat.before.reserve(3 * nbefore)); MI_TRY(c->bat.after.reserve(3 * nafter)); MI_TRY(c->bat.running.reserve(1));
    MI_TRY(host_to_device(c, c->bat.before.p, before_xyz + 3 * (size_t)sp.b_lo, sizeof(float) * 3 * nbefore));
    MI_TRY(host_to_device(c, c->bat.after.p, after_xyz + 3 * (size_t)sp.a_lo, sizeof(float) * 3 * nafter));
    return MI_OK;
}
// Bounded launches until no problem is running: `launch` enqueues one launch of the iterate kernel, whose workgroups count the problems
// they leave unfinished in ctx->bat.running; the host reads the word behind every launch.
template <class Launch>
static inline int batch_run_until_quiet(mi_ctx* c, bool anything_to_run, Launch&& launch, int* launches)
{
    int* h_running = reinterpret_cast<int*>(c->h_scratch);
    *h_running = anything_to_run ? 1 : 0;
    while (*h_running != 0) {
        MI_HIP(hipMemsetAsync(c->bat.running.p, 0, sizeof(int), c->stream));
        MI_HIP(launch());
        (*launches)++;
        MI_HIP(hipMemcpyAsync(h_running, c->bat.running.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
    }
    return MI_OK;
}

}  // namespace mislam
