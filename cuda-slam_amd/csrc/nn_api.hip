// Correspondence search behind the C ABI: the search plan, the uploads, the two exact indexes over the fixed cloud (box hierarchy,
// cell grid) and the launch of K1 / K1t / K1g; mi_nn_search is the test-grade entry point.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "context.h"

using namespace mislam;

namespace mislam {

constexpr int NN_MAX_CHUNKS = 1024;

size_t target_alloc_len(int m_local)
{
    // any chunking with <= NN_MAX_CHUNKS chunks of T-aligned length stays inside this allocation
    return (size_t)round_up(std::max(m_local, 1), NN_TARGET_BLOCK) + (size_t)NN_TARGET_BLOCK * NN_MAX_CHUNKS;
}

// 2-D decomposition of the (source, target) pair space for K1.  Few chunks = few re-scan restarts and few atomics;
// enough workgroups = every CU busy with a short tail.  Measured on MI355X (profiles/r01_nn_microbench.log): R = 2 with
// the smallest chunk count that still yields >= ~8 workgroups per CU is the fastest configuration at every size.
NnPlan plan_nn(const mi_ctx* ctx, int n, int m_local)
{
    NnPlan p;
    p.R = ctx->tune.nn_R;
    if (p.R != 1 && p.R != 2 && p.R != 4 && p.R != 8) p.R = 2;
    const int n_src_blocks = round_up(std::max(n, 1), 256 * p.R) / (256 * p.R);
    const int target_wgs = ctx->tune.nn_wgs > 0 ? ctx->tune.nn_wgs : ctx->cu_count * 8;
    int chunks = (target_wgs + n_src_blocks - 1) / n_src_blocks;
    // a chunk should fit an XCD's L2 next to everything else it holds: <= 2 MB of target xyz (12 B/point)
    const int l2_chunks = (int)(((long long)std::max(m_local, 1) * 12 + (2 << 20) - 1) / (2 << 20));
    chunks = std::max(chunks, l2_chunks);
    const int max_chunks = std::max(1, std::min(NN_MAX_CHUNKS, m_local / (NN_TARGET_BLOCK * 4)));
    chunks = std::max(1, std::min(chunks, max_chunks));
    // multiples of 8 get the XCD-pinned block mapping of K1
    if (chunks > 1 && max_chunks >= 8) chunks = std::min(round_up(chunks, 8), max_chunks / 8 * 8);
    const int forced = ctx->tune.nn_chunks;
    if (forced > 0) chunks = std::min(forced, NN_MAX_CHUNKS);
    p.chunk_len = round_up((std::max(m_local, 1) + chunks - 1) / chunks, NN_TARGET_BLOCK);
    p.n_chunks = (std::max(m_local, 1) + p.chunk_len - 1) / p.chunk_len;
    return p;
}

int host_to_device(mi_ctx* c, void* dst_dev, const void* src_host, size_t bytes)
{
    const hipStream_t ws = c->work_stream();
    constexpr size_t PIECE = mi_ctx::PinnedRing::PIECE;
    if (bytes < PIECE / 4 || c->pin.buf == nullptr) {     // small: the runtime's path is fine (and synchronous for pageable memory)
        MI_HIP(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ws));
        return MI_OK;
    }
    for (size_t o = 0; o < bytes; o += PIECE) {       // the copy of piece k overlaps the transfers of the pieces before it
        const size_t nb = std::min(PIECE, bytes - o);
        const unsigned int k = c->pin.next++ % mi_ctx::PinnedRing::SLOTS;
        if (c->pin.busy & (1u << k)) { MI_HIP(hipEventSynchronize(c->pin.event[k])); c->pin.busy &= ~(1u << k); }   // (sixteen pieces ago: long done)
        char* slot = c->pin.buf + (size_t)k * PIECE;
        memcpy(slot, (const char*)src_host + o, nb);
        MI_HIP(hipMemcpyAsync((char*)dst_dev + o, slot, nb, hipMemcpyHostToDevice, ws));
        MI_HIP(hipEventRecord(c->pin.event[k], ws));
        c->pin.busy |= 1u << k;
    }
    return MI_OK;
}

int upload_soa(mi_ctx* c, const float* host_aos, int n, int n_pad, float* x, float* y, float* z, float4* packed)
{
    DevBuf<float>& staging = c->scratch[c->lane].staging;
    MI_TRY(staging.reserve((size_t)3 * n));
    MI_TRY(host_to_device(c, staging.p, host_aos, sizeof(float) * 3 * (size_t)n));
    MI_HIP(aos_to_soa(staging.p, n, n_pad, x, y, z, packed, c->work_stream()));
    // the staging buffer is reused by the next upload of the same lane: stream order keeps them apart, and a pageable-memory copy is
    // already synchronous with respect to the host buffer
    return MI_OK;
}

// Scratch for one Morton sort of m points.  (sort_temp_bytes is a bound nothing reads: the radix sort's scratch has one size whatever m is.)
int morton_args(MortonScratch& sc, const float* x, const float* y, const float* z, int m, int* order_out, MortonArgs* out)
{
    const size_t sort_bytes = tree_sort_temp_bytes(m);
    MI_TRY(sc.codes_in.reserve((size_t)m)); MI_TRY(sc.codes_out.reserve((size_t)m));
    MI_TRY(sc.order_in.reserve((size_t)m));
    MI_TRY(sc.bbox.reserve(256 * 6 + 8));
    MI_TRY(sc.sort_temp.reserve(sort_bytes + 16));
    MortonArgs a{};
    a.x = x; a.y = y; a.z = z; a.m = m;
    a.bbox_partials = sc.bbox.p; a.bbox = sc.bbox.p + 256 * 6;
    a.codes_in = sc.codes_in.p; a.codes_out = sc.codes_out.p; a.order_in = sc.order_in.p; a.order_out = order_out;
    a.sort_temp = sc.sort_temp.p; a.sort_temp_bytes = sort_bytes;
    *out = a;
    return MI_OK;
}

int grid_reserve(GridBuffers& b, const float bbox[6], int m, int index_base, float points_per_cell, NnGridView* view)
{
    NnGridView g{};
    grid_plan(bbox, m, points_per_cell, &g);
    const size_t n_cells = (size_t)g.nx * g.ny * g.nz;
    MI_TRY(b.pts.reserve((size_t)m + GRID_PTS_PAD));
    MI_TRY(b.row_occ.reserve(n_cells)); MI_TRY(b.near_tmp.reserve(n_cells));
    MI_TRY(b.start.reserve(n_cells + 1 + 3));           // (+3: a row's offsets are fetched four words at a time)
    MI_TRY(b.fill.reserve(n_cells + 1));
    MI_TRY(b.scan.reserve((n_cells + 1) / 1024 + 2));
    MI_TRY(b.slot_of.reserve((size_t)m));
    g.pts = b.pts.p;
    g.cell_start = b.start.p;
    g.slot_of = b.slot_of.p;
    g.row_occ = b.row_occ.p;
    g.index_base = index_base;
    *view = g;
    return MI_OK;
}

int grid_build_into(GridBuffers& b, const NnGridView& view, const float* x, const float* y, const float* z, int m, hipStream_t s)
{
    GridBuildArgs a{};
    a.x = x; a.y = y; a.z = z; a.m = m; a.index_base = view.index_base;
    a.view = view; a.cell_fill = b.fill.p; a.scan_tmp = b.scan.p; a.pts_out = b.pts.p; a.cell_start_out = b.start.p; a.slot_of_out = b.slot_of.p;
    a.row_occ_out = b.row_occ.p; a.near_tmp = b.near_tmp.p;
    MI_HIP(grid_build(a, s));
    return MI_OK;
}

// Builds the box hierarchy over the resident fixed-cloud shard if it is not there yet (once per mi_icp_load / search).
int ensure_tree(mi_ctx* c, int m_local, int index_base)
{
    if (c->tree.valid) return MI_OK;
    const int n_leaves = (m_local + TREE_LEAF - 1) / TREE_LEAF;
    int n_pad = 1, height = 0;
    while (n_pad < n_leaves) { n_pad <<= 1; height++; }
    if (height > TREE_MAX_HEIGHT) { set_error("fixed cloud too large for the box hierarchy"); return MI_ERR_INVALID_ARG; }
    if (c->selftest_fail_loads > 0) {      // mi_selftest_fail_loads (tests): the next N index builds of the context fail HERE -- behind the fixed cloud's
        c->selftest_fail_loads -= 1;       // upload, which is already on the auxiliary stream: the early return mi_icp_load's lane guard exists for
        set_error("index build failed on request (mi_selftest_fail_loads)");
        return MI_ERR_INVALID_ARG;
    }
    MI_TRY(c->tree.order_out.reserve((size_t)m_local));
    MI_TRY(c->tree.pts.reserve((size_t)n_leaves * TREE_LEAF));
    MI_TRY(c->tree.boxes.reserve((size_t)4 * n_pad));
    MI_TRY(c->tree.leaf.reserve((size_t)n_leaves * (3 * TREE_LEAF / 4)));
    MI_TRY(c->tree.idx.reserve((size_t)n_leaves * TREE_LEAF));
    MI_TRY(c->tree.boxes6.reserve((size_t)12 * ((size_t)n_pad + 6)));        // pairs of nodes (nn_tree.h), incl. the padding a step may read
    TreeBuildArgs a{};
    MI_TRY(morton_args(c->scratch[c->lane].morton, c->tx.p, c->ty.p, c->tz.p, m_local, c->tree.order_out.p, &a.morton));   // (the lane's own scratch: two sorts may be in flight, one per lane)
    a.index_base = index_base; a.n_leaves = n_leaves; a.n_pad = n_pad;
    a.pts = c->tree.pts.p; a.boxes = c->tree.boxes.p;
    a.leaf_soa = c->tree.leaf.p; a.leaf_idx = c->tree.idx.p; a.boxes6 = c->tree.boxes6.p;
    MI_HIP(tree_build(a, c->work_stream()));
    c->tree.view.boxes6 = c->tree.boxes6.p;
    c->tree.view.leaf_soa = c->tree.leaf.p; c->tree.view.leaf_idx = c->tree.idx.p;
    c->tree.view.n_pad = n_pad; c->tree.view.height = height; c->tree.view.n_leaves = n_leaves;
    c->tree.valid = true;
    return MI_OK;
}

// Builds the cell grid over the resident fixed-cloud shard if it is not there yet.  The cell size comes from the cloud's bounding
// box, which the host reads back: one stream synchronisation per fixed cloud, at load time.
int ensure_grid(mi_ctx* c, int m_local, int index_base)
{
    if (c->grid.valid) return MI_OK;
    const hipStream_t ws = c->work_stream();
    MI_TRY(c->grid.bbox.reserve(256 * 6 + 8));              // (its own: a Morton sort's bounding box may be in flight on another lane)
    float* d_bbox = c->grid.bbox.p + 256 * 6;
    MI_HIP(cloud_bbox(c->tx.p, c->ty.p, c->tz.p, m_local, c->grid.bbox.p, d_bbox, ws));
    float* bbox = c->h_scratch;                        // (pinned: a read-back into pageable memory goes through the runtime's staging)
    MI_HIP(hipMemcpyAsync(bbox, d_bbox, 6 * sizeof(float), hipMemcpyDeviceToHost, ws));
    { StallProbe sp("grid: bounding-box synchronize"); MI_HIP(hipStreamSynchronize(ws)); }
    StallProbe sp_rest("grid: reserve + enqueue build");
    NnGridView g{};
    MI_TRY(grid_reserve(c->grid.cells, bbox, m_local, index_base, c->tune.grid_points_per_cell, &g));
    MI_TRY(grid_build_into(c->grid.cells, g, c->tx.p, c->ty.p, c->tz.p, m_local, ws));
    c->grid.view = g;
    c->grid.valid = true;
    return MI_OK;
}

int reserve_moving(mi_ctx* c, size_t n_pad, size_t c_pad)
{
    MI_TRY(c->bx.reserve(n_pad)); MI_TRY(c->by.reserve(n_pad)); MI_TRY(c->bz.reserve(n_pad));
    MI_TRY(c->cx.reserve(c_pad)); MI_TRY(c->cy.reserve(c_pad)); MI_TRY(c->cz.reserve(c_pad));
    return c->keys.reserve(n_pad);
}

// Morton-sorts the moving cloud once: src (SoA, n real points) -> dst (SoA, n_pad entries, tail = copies of the last sorted
// point); c->sorder[s] = the caller's index of sorted slot s.  Spatially adjacent sources then share a wave, which is what
// makes the wave-cooperative hierarchy walk tight; K2-K6 are order-agnostic sums, so nothing else changes.
int sort_sources(mi_ctx* c, const float* sx, const float* sy, const float* sz, int n, int n_pad, float* dx, float* dy, float* dz)
{
    MI_TRY(c->sorder.reserve((size_t)n));
    MortonArgs ma{};
    MI_TRY(morton_args(c->scratch[c->lane].morton, sx, sy, sz, n, c->sorder.p, &ma));
    MI_HIP(morton_order(ma, c->work_stream()));
    MI_HIP(permute_soa(sx, sy, sz, c->sorder.p, n, n_pad, dx, dy, dz, c->work_stream()));
    return MI_OK;
}

int resolve_nn_mode(const mi_ctx* c, int nn_mode, int m_local)
{
    const int forced = c->tune.nn_force_mode;
    if (forced == MI_NN_BRUTEFORCE || forced == MI_NN_TREE || forced == MI_NN_GRID) nn_mode = forced;
    if (nn_mode == MI_NN_BRUTEFORCE || nn_mode == MI_NN_TREE || nn_mode == MI_NN_GRID) return nn_mode;
    // measured crossover on MI355X, every-pair against the cell grid, ms per ICP step at N = M (profiles/r03_crossover.log):
    // 6 000: 0.042 / 0.042, 8 000: 0.048 / 0.046, 10 000: 0.056 / 0.048, 12 000: 0.063 / 0.047, 16 000: 0.085 / 0.051 -- the grid's
    // index builds (0.3 ms per registration) are what keeps the switch at 10 000 rather than 7 000
    return m_local >= MI_NN_INDEX_MIN_POINTS ? MI_NN_GRID : MI_NN_BRUTEFORCE;
}

extern "C" const char* mi_nn_kernel_name(const mi_ctx* c, int n_moving, int m_fixed_local, int nn_mode)
{
    (void)n_moving;
    if (!c) return "";
    const int mode = resolve_nn_mode(c, nn_mode, m_fixed_local);
    return mode == MI_NN_GRID ? nn_grid_kernel_name(false) : (mode == MI_NN_TREE ? "nn_tree_kernel" : "nn_bruteforce_kernel");
}

GridSearchArgs grid_search_args(const mi_ctx* c, int n)
{
    GridSearchArgs a{};
    a.n = n; a.keys = c->keys.p;
    a.stats = c->nn_stats_on ? c->nn_stats.p : nullptr;
    a.deal_rows = c->tune.grid_deal_rows < 0 ? (n >= GRID_DEAL_ROWS_MIN_POINTS ? 1 : 0) : c->tune.grid_deal_rows;
    return a;
}

int launch_nn(mi_ctx* c, const float* sx, const float* sy, const float* sz, int n, int m_local, int index_base, int fma,
                      const int* done_flag, int nn_mode)
{
    const int mode = resolve_nn_mode(c, nn_mode, m_local);
    if (mode == MI_NN_TREE || mode == MI_NN_GRID) {
        MI_TRY(ensure_tree(c, m_local, index_base));
        if (mode == MI_NN_GRID) MI_TRY(ensure_grid(c, m_local, index_base));
        ProfScope ps(c, MI_KERNEL_NN);
        if (mode == MI_NN_GRID) {
            GridSearchArgs a = grid_search_args(c, n);
            a.sx = sx; a.sy = sy; a.sz = sz; a.done_flag = done_flag;
            MI_HIP(nn_grid_query(c->grid.view, c->tree.view, a, fma, c->stream));
        } else {
            MI_HIP(nn_tree_query(c->tree.view, sx, sy, sz, n, c->keys.p, done_flag, fma, c->stream));
        }
        return MI_OK;
    }
    const NnPlan p = plan_nn(c, n, m_local);
    NnLaunch a{};
    a.sx = sx; a.sy = sy; a.sz = sz;
    a.n = n; a.n_pad = round_up(n, 256 * p.R);
    a.tx = c->tx.p; a.ty = c->ty.p; a.tz = c->tz.p;
    a.chunk_len = p.chunk_len; a.n_chunks = p.n_chunks;
    a.index_base = index_base;
    a.keys = c->keys.p;
    a.done_flag = done_flag;
    a.R = p.R;
    a.fma = fma;
    // host-side shape checks before a hand-written kernel runs (a fault can reset the whole node)
    if ((size_t)a.n_pad > c->cx.cap && sx == c->cx.p) { set_error("internal: source padding exceeds allocation"); return MI_ERR_STATE; }
    if ((size_t)a.n_chunks * a.chunk_len > c->tx.cap) { set_error("internal: target chunking exceeds allocation"); return MI_ERR_STATE; }
    if (a.chunk_len % NN_TARGET_BLOCK != 0) { set_error("internal: chunk_len not a multiple of the target block"); return MI_ERR_STATE; }
    ProfScope ps(c, MI_KERNEL_NN);
    MI_HIP(nn_launch(a, c->stream));
    return MI_OK;
}

int allreduce_keys(mi_ctx* c, int n)
{
    if (!c->distributed()) return MI_OK;
    ProfScope ps(c, MI_KERNEL_ALLREDUCE);
    return allreduce_min_u64(c, c->keys.p, (size_t)n);
}

// Uploads this rank's shard of the fixed cloud (SoA streams for K1 + float4 for gathers).
int upload_target_shard(mi_ctx* c, const float* after_xyz, int m_total, bool replicate)
{
    c->prob.m_total = m_total;
    c->tree.valid = false;   // the indexes cover the previous shard
    c->grid.valid = false;
    if (replicate) { c->prob.shard_lo = 0; c->prob.shard_hi = m_total; }      // source-sharded: every rank holds the whole fixed cloud
    else (void)mi_shard_range(m_total, c->rank, c->world, &c->prob.shard_lo, &c->prob.shard_hi);
    const int m_local = c->prob.shard_hi - c->prob.shard_lo;
    const size_t len = target_alloc_len(m_local);
    MI_TRY(c->tx.reserve(len)); MI_TRY(c->ty.reserve(len)); MI_TRY(c->tz.reserve(len));
    MI_TRY(c->tgt4.reserve(len));
    if (m_local > 0)
        MI_TRY(upload_soa(c, after_xyz + 3 * (size_t)c->prob.shard_lo, m_local, (int)len, c->tx.p, c->ty.p, c->tz.p, c->tgt4.p));
    return MI_OK;
}

}  // namespace mislam

extern "C" int mi_nn_search(mi_ctx* c, const float* src_xyz, int n, const float* tgt_xyz, int m, int dist_mode, int* idx, float* d2)
{
    return mi_nn_search_ex(c, src_xyz, n, tgt_xyz, m, dist_mode, MI_NN_AUTO, idx, d2);
}

extern "C" int mi_nn_search_ex(mi_ctx* c, const float* src_xyz, int n, const float* tgt_xyz, int m, int dist_mode, int nn_mode,
                               int* idx, float* d2)
{
    if (!c) { set_error("mi_nn_search: null context"); return MI_ERR_INVALID_ARG; }
    if (nn_mode != MI_NN_AUTO && nn_mode != MI_NN_BRUTEFORCE && nn_mode != MI_NN_TREE && nn_mode != MI_NN_GRID) { set_error("mi_nn_search: bad nn_mode"); return MI_ERR_INVALID_ARG; }
    if (n < 0 || m < 0 || (n > 0 && (!src_xyz || !idx)) || (m > 0 && !tgt_xyz)) { set_error("mi_nn_search: bad arguments"); return MI_ERR_INVALID_ARG; }
    if (dist_mode != MI_DIST_CPU_ROUNDING && dist_mode != MI_DIST_FMA) { set_error("mi_nn_search: bad dist_mode"); return MI_ERR_INVALID_ARG; }
    if (n == 0) return MI_OK;
    if (m == 0) { set_error("mi_nn_search: empty target cloud"); return MI_ERR_INVALID_ARG; }
    if (m < c->world) { set_error("mi_nn_search: fewer targets than ranks"); return MI_ERR_INVALID_ARG; }
    MI_ENTER(c);
    c->prob.icp_loaded = false;   // the workspace is being reused
    const int n_pad = round_up(n, NN_SRC_PAD);
    MI_TRY(reserve_moving(c, (size_t)n_pad, (size_t)n_pad));
    MI_TRY(upload_soa(c, src_xyz, n, n_pad, c->bx.p, c->by.p, c->bz.p, nullptr));
    MI_TRY(sort_sources(c, c->bx.p, c->by.p, c->bz.p, n, n_pad, c->cx.p, c->cy.p, c->cz.p));
    MI_TRY(upload_target_shard(c, tgt_xyz, m));
    MI_HIP(fill_keys(c->keys.p, n, c->stream));
    MI_TRY(launch_nn(c, c->cx.p, c->cy.p, c->cz.p, n, c->prob.shard_hi - c->prob.shard_lo, c->prob.shard_lo, dist_mode == MI_DIST_FMA, nullptr, nn_mode));
    MI_TRY(allreduce_keys(c, n));
    MI_TRY(c->idx_tmp.reserve((size_t)n));
    MI_TRY(c->scratch[0].staging.reserve((size_t)n));
    // keys are in sorted-slot order: scatter back to the caller's order
    MI_HIP(unpack_keys(c->keys.p, c->sorder.p, n, c->idx_tmp.p, d2 ? c->scratch[0].staging.p : nullptr, c->stream));
    MI_HIP(hipMemcpyAsync(idx, c->idx_tmp.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (d2) MI_HIP(hipMemcpyAsync(d2, c->scratch[0].staging.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    return MI_OK;
}
