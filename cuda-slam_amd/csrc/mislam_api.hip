// C ABI (include/mi_slam.h): error text, device memory, the context, the distributed transports and their all-reduces, profiling.
// The search lives in nn_api.hip, the ICP driver in icp_api.hip.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "cloud_range.hpp"
#include "context.h"

using namespace mislam;

// ---------------------------------------------------------------------------------------------------------------
// error reporting
// ---------------------------------------------------------------------------------------------------------------
namespace mislam {
static thread_local char g_error[512] = "";
void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

static thread_local std::vector<void*>* t_retire_sink = nullptr;      // the running call's context list (CtxScope)
double& alloc_ms_counter()
{
    static thread_local double ms = 0.0;
    return ms;
}
double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
void device_free(void* p);
void retire_later(void* p)
{
    if (t_retire_sink != nullptr) { t_retire_sink->push_back(p); return; }
    (void)hipDeviceSynchronize();               // outside any context call (not a path the library takes): nothing may still read it after this
    device_free(p);
}
CtxScope::CtxScope(mi_ctx* c) : ctx(c), outer(t_retire_sink) { t_retire_sink = &c->retired; c->entered += 1; }
CtxScope::~CtxScope()
{
    t_retire_sink = outer;
    if (!ctx->retired.empty() && ctx->stream != nullptr && hipStreamQuery(ctx->stream) == hipSuccess) retire_buffers(ctx);
    else (void)hipGetLastError();               // (hipErrorNotReady is not an error here)
}
// One allocation stream and one PRIVATE memory pool per device (hipMemPoolCreate; release threshold: never -- the library's buffers
// are meant to be handed out again, not returned to the driver between calls).  The device's default pool is left alone: its
// attributes belong to the host application.  The stream carries no work, so the pool's stream-ordered calls complete at once
// there.  A buffer is only ever freed behind a synchronisation of the stream that used it (retire_buffers, context destruction),
// so handing its memory out again -- to this context or another -- is safe whatever stream the new owner works on.  When the last
// context on a device is destroyed the pool is trimmed to nothing (pool_context_gone).  MISLAM_POOL=0: plain hipMalloc / hipFree.
static constexpr int MAX_DEVICES = 64;
static hipStream_t g_alloc_stream[MAX_DEVICES] = {nullptr};
static hipMemPool_t g_pool[MAX_DEVICES] = {nullptr};
static int g_pool_contexts[MAX_DEVICES] = {0};
static int g_use_pool = -1;                     // -1: not decided yet
static std::mutex g_pool_mutex;
static hipStream_t alloc_stream(hipMemPool_t* pool_out = nullptr)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return nullptr;
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    if (g_use_pool == -1) {
        const char* e = getenv("MISLAM_POOL");
        g_use_pool = (e && e[0] == '0') ? 0 : 1;
    }
    if (!g_use_pool) return nullptr;
    if (g_alloc_stream[dev] == nullptr) {
        hipMemPool_t pool = nullptr;
        hipStream_t s = nullptr;
        unsigned long long keep = ~0ull;
        hipMemPoolProps props;
        memset(&props, 0, sizeof props);
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = dev;
        if (hipMemPoolCreate(&pool, &props) != hipSuccess || hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep) != hipSuccess ||
            hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            if (pool != nullptr) (void)hipMemPoolDestroy(pool);
            g_use_pool = 0;
            return nullptr;
        }
        g_pool[dev] = pool;
        g_alloc_stream[dev] = s;
    }
    if (pool_out) *pool_out = g_pool[dev];
    return g_alloc_stream[dev];
}
static bool g_pool_proven = false;               // a pool allocation has succeeded: the mode never changes after that
static std::atomic<long long> g_live_buffers{0}; // successful device_alloc calls minus device_free calls (mi_selftest_live_buffers)
hipError_t device_alloc(void** p, size_t bytes)
{
    hipMemPool_t pool = nullptr;
    if (hipStream_t s = alloc_stream(&pool)) {
        hipError_t e = hipMallocFromPoolAsync(p, bytes, pool, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);          // (nothing else is ever on this stream: the memory is usable on any stream from here)
        std::lock_guard<std::mutex> lock(g_pool_mutex);
        if (e == hipSuccess) { g_pool_proven = true; g_live_buffers += 1; return e; }
        (void)hipGetLastError();
        if (g_pool_proven || e == hipErrorOutOfMemory) return e;
        g_use_pool = 0;                          // this runtime has no working pool: plain allocations throughout
    }
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) g_live_buffers += 1;
    return e;
}
void device_free(void* p)
{
    if (p == nullptr) return;
    g_live_buffers -= 1;
    if (hipStream_t s = alloc_stream()) { (void)hipFreeAsync(p, s); return; }
    (void)hipFree(p);
}
// context bookkeeping per device: the last one to go returns the pool's memory to the driver
static void pool_context_created(int dev)
{
    if (dev < 0 || dev >= MAX_DEVICES) return;
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    g_pool_contexts[dev] += 1;
}
static void pool_context_gone(int dev)
{
    if (dev < 0 || dev >= MAX_DEVICES) return;
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    if (g_pool_contexts[dev] > 0) g_pool_contexts[dev] -= 1;
    if (g_pool_contexts[dev] == 0 && g_pool[dev] != nullptr && g_alloc_stream[dev] != nullptr) {
        (void)hipStreamSynchronize(g_alloc_stream[dev]);           // the frees enqueued by the destructor have landed
        (void)hipMemPoolTrimTo(g_pool[dev], 0);
    }
}
// (called right behind a synchronisation of the context's stream, its device current: nothing still uses these)
void retire_buffers(mi_ctx* ctx)
{
    std::vector<void*> v;
    v.swap(ctx->retired);
    for (void* p : v) device_free(p);
}
}  // namespace mislam

double mislam::g_stall_ms = -1.0;       // MISLAM_DEV_STALL_MS (StallProbe, context.h)

extern "C" const char* mi_last_error(void) { return g_error; }
extern "C" int mi_abi_version(void) { return MI_SLAM_ABI_VERSION; }

extern "C" int mi_device_count(int* count)
{
    if (!count) { set_error("mi_device_count: null argument"); return MI_ERR_INVALID_ARG; }
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess || c <= 0) {
        *count = 0;
        set_error("no usable HIP device (%s); this library has no CPU fallback", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
        return MI_ERR_NO_DEVICE;
    }
    *count = c;
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------------------------
// Loads every code object of the library now.  With the runtime's deferred loading the first launch out of each translation
// unit otherwise stalls whatever call it happens in (measured: first ICP call at 1e6 points 22 -> 17 ms, first CPD call
// 36 -> 3 ms) -- at the price of ~170 ms here, so it is the caller's choice: a long-lived process wants it, a one-shot run not.
extern "C" int mi_ctx_preload(mi_ctx* c)
{
    if (!c) { set_error("mi_ctx_preload: null context"); return MI_ERR_INVALID_ARG; }
    MI_ENTER(c);
    MI_HIP(preload_nn_kernel()); MI_HIP(preload_nn_tree()); MI_HIP(preload_nn_grid()); MI_HIP(preload_icp_kernels()); MI_HIP(preload_icp_batch()); MI_HIP(preload_cpd_kernels()); MI_HIP(preload_cpd_batch());
    MI_HIP(preload_cpd_fgt()); MI_HIP(preload_nicp_api()); MI_HIP(preload_prepare_api()); MI_HIP(preload_voxel_kernels()); MI_HIP(preload_knn_kernels()); MI_HIP(preload_normals_kernels()); MI_HIP(preload_outlier_kernels()); MI_HIP(preload_plane_kernels()); MI_HIP(preload_gicp_kernels()); MI_HIP(preload_fpfh_kernels()); MI_HIP(preload_match_kernels()); MI_HIP(preload_ransac_kernels()); MI_HIP(preload_ndt_kernels()); MI_HIP(preload_iss_kernels()); MI_HIP(preload_cluster_kernels()); MI_HIP(preload_segment_kernels()); MI_HIP(preload_fgr_kernels()); MI_HIP(preload_color_kernels()); MI_HIP(preload_mls_kernels()); MI_HIP(preload_radius_kernels()); MI_HIP(preload_eval_kernels()); MI_HIP(preload_pose_graph_kernels()); MI_HIP(preload_scan_context_kernels()); MI_HIP(preload_tsdf_kernels());
    return MI_OK;
}

static int ctx_create_common(int device, mi_ctx** out)
{
    if (!out) { set_error("mi_ctx_create: null out pointer"); return MI_ERR_INVALID_ARG; }
    *out = nullptr;
    int count = 0;
    MI_TRY(mi_device_count(&count));
    if (device < 0 || device >= count) { set_error("mi_ctx_create: device %d out of range [0,%d)", device, count); return MI_ERR_INVALID_ARG; }
    MI_HIP(hipSetDevice(device));
    mi_ctx* c = new mi_ctx();
    c->device = device;
    pool_context_created(device);
    // a failure half way releases what was created so far (mi_ctx_destroy copes with null members)
    const int rc = [&]() -> int {
        hipDeviceProp_t prop;
        MI_HIP(hipGetDeviceProperties(&prop, device));
        c->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        MI_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        MI_HIP(hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
        MI_HIP(hipStreamCreateWithFlags(&c->aux2, hipStreamNonBlocking));
        for (hipEvent_t& e : c->aux_event) MI_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        MI_HIP(hipMalloc((void**)&c->d_state, sizeof(IcpState)));
        MI_HIP(hipHostMalloc((void**)&c->h_state, sizeof(IcpState), hipHostMallocDefault));
        MI_HIP(hipEventCreateWithFlags(&c->peek_event, hipEventDisableTiming));
        memset(c->h_state, 0, sizeof(IcpState));
        // developer switches: read here, once -- nothing on the per-iteration path looks at the environment
        auto env_i = [](const char* name, int dflt) { const char* v = getenv(name); return (v && *v) ? atoi(v) : dflt; };
        if (const char* sm = getenv("MISLAM_DEV_STALL_MS")) g_stall_ms = atof(sm);
        c->tune.nn_force_mode = env_i("MISLAM_NN_MODE", 0);
        c->tune.nn_R = env_i("MISLAM_NN_R", 2);
        c->tune.nn_wgs = env_i("MISLAM_NN_WGS", 0);
        c->tune.nn_chunks = env_i("MISLAM_NN_CHUNKS", 0);
        c->tune.cpd_mfma = env_i("MISLAM_CPD_MFMA", 1);
        c->tune.cpd_trunc_cull = env_i("MISLAM_CPD_TRUNC_CULL", 1);
        c->tune.fgt_resume = env_i("MISLAM_FGT_RESUME", 1);
        c->tune.fgt_replay = env_i("MISLAM_FGT_REPLAY", 1);
        c->tune.fgt_two_streams = env_i("MISLAM_FGT_TWO_STREAMS", 1);
        c->tune.fgt_lists_in_model = env_i("MISLAM_FGT_LISTS_IN_MODEL", 1);
        c->tune.fgt_coop_sweep = env_i("MISLAM_FGT_COOP_SWEEP", 1);
        c->tune.fgt_model_splits = env_i("MISLAM_FGT_MODEL_SPLITS", 1);
        c->tune.fgt_shard_queries = env_i("MISLAM_FGT_SHARD_QUERIES", 1);
        c->tune.grid_deal_rows = env_i("MISLAM_GRID_DEAL_ROWS", -1);
        c->tune.grid_split_walks = env_i("MISLAM_GRID_SPLIT_WALKS", -1);
        c->tune.icp_pipeline = env_i("MISLAM_ICP_PIPELINE", 1);
        c->tune.icp_fused_solve = env_i("MISLAM_ICP_FUSED_SOLVE", 1);
        c->tune.icp_ticket_solve = env_i("MISLAM_ICP_TICKET_SOLVE", 1);
        c->tune.svd_ieee = env_i("MISLAM_SVD_IEEE", 0);
        if (const char* ppc = getenv("MISLAM_GRID_PPC")) { const float f = (float)atof(ppc); if (f >= 0.25f && f <= 64.f) c->tune.grid_points_per_cell = f; }
        if (const char* ppc = getenv("MISLAM_KNN_POINTS_PER_CELL")) { const float f = (float)atof(ppc); if (f >= 0.125f && f <= 1e30f) c->tune.knn_points_per_cell = f; }
        if (const char* rc = getenv("MISLAM_OUTLIER_RADIUS_CELL")) { const float f = (float)atof(rc); if (f >= 0.125f && f <= 1024.f) c->tune.outlier_radius_cell = f; }
        if (env_i("MISLAM_PRELOAD", 0) == 1) MI_TRY(mi_ctx_preload(c));       // =1: mi_ctx_preload as part of every context creation
        // Host clouds go up through the runtime's own pageable-copy path (round 6).  Rounds 3-5 staged them through an own pinned ring of 16 x 1 MB, built
        // against 20-50 ms stalls that round 3 pinned on the runtime's path -- and that were the process's CPU quota being throttled by idle BLAS pools
        // (profiles/r03_stall_hunt.log: gone with the pools quiet, for either path).  Measured side by side, 20 calls each (profiles/r06_upload_paths.log):
        // a load of two 12 MB clouds 1.35 -> 1.01 ms (the ring's one host thread copies every byte itself, 37 us per MB; the runtime pipelines larger pieces
        // over its own staging buffers), 120 MB clouds 13.3 -> 7.8 ms, the whole 50-iteration registration at 1e6 points 6.43 -> 6.04 ms; outliers as
        // rare on one as on the other.  MISLAM_PIN=1 brings the ring back (4 ms of pinning per context).
        if (env_i("MISLAM_PIN", 0) != 0) {
            MI_HIP(hipHostMalloc((void**)&c->pin.buf, mi_ctx::PinnedRing::PIECE * mi_ctx::PinnedRing::SLOTS, hipHostMallocDefault));
            for (hipEvent_t& e : c->pin.event) MI_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        MI_HIP(hipHostMalloc((void**)&c->h_scratch, 64 * sizeof(float), hipHostMallocDefault));
        return MI_OK;
    }();
    if (rc != MI_OK) { mi_ctx_destroy(c); return rc; }
    *out = c;
    return MI_OK;
}

extern "C" int mi_ctx_create(int device, mi_ctx** out) { return ctx_create_common(device, out); }

extern "C" int mi_dist_unique_id(void* out_unique_id)
{
    if (!out_unique_id) { set_error("mi_dist_unique_id: null argument"); return MI_ERR_INVALID_ARG; }
    static_assert(sizeof(ncclUniqueId) == MI_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    MI_NCCL(ncclGetUniqueId(&id));
    memcpy(out_unique_id, &id, sizeof id);
    return MI_OK;
}

extern "C" int mi_ctx_create_dist(int device, int rank, int world, const void* unique_id, mi_ctx** out)
{
    if (world < 1 || rank < 0 || rank >= world || !unique_id) { set_error("mi_ctx_create_dist: bad rank/world/id"); return MI_ERR_INVALID_ARG; }
    MI_TRY(ctx_create_common(device, out));
    mi_ctx* c = *out;
    c->rank = rank;
    c->world = world;
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof id);
    ncclResult_t r = ncclCommInitRank(&c->comm, world, id, rank);
    if (r != ncclSuccess) {
        set_error("ncclCommInitRank(rank %d of %d) failed: %s", rank, world, ncclGetErrorString(r));
        mi_ctx_destroy(c);
        *out = nullptr;
        return MI_ERR_RCCL;
    }
    return MI_OK;
}

extern "C" int mi_ctx_create_exchange(int device, int rank, int world, mi_exchange_fn exchange, void* user, mi_ctx** out)
{
    if (world < 1 || rank < 0 || rank >= world || !exchange) { set_error("mi_ctx_create_exchange: bad rank/world/callback"); return MI_ERR_INVALID_ARG; }
    MI_TRY(ctx_create_common(device, out));
    mi_ctx* c = *out;
    c->rank = rank;
    c->world = world;
    c->exchange = exchange;
    c->exchange_user = user;
    return MI_OK;
}

// The caller's transport: drain the stream, stage through pinned host memory, combine there, copy back.
static int exchange_on_host(mi_ctx* c, void* dev_ptr, size_t count, int kind)
{
    const size_t bytes = count * 8;
    if (bytes > c->exchange_cap) {
        if (c->exchange_host) (void)hipHostFree(c->exchange_host);
        c->exchange_host = nullptr;
        c->exchange_cap = 0;
        MI_HIP(hipHostMalloc(&c->exchange_host, bytes, hipHostMallocDefault));
        c->exchange_cap = bytes;
    }
    MI_HIP(hipMemcpyAsync(c->exchange_host, dev_ptr, bytes, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    const int r = c->exchange(c->exchange_user, c->exchange_host, count, kind);
    if (r != 0) { set_error("the exchange callback failed with %d (rank %d of %d, %zu elements, kind %d)", r, c->rank, c->world, count, kind); return MI_ERR_RCCL; }
    MI_HIP(hipMemcpyAsync(dev_ptr, c->exchange_host, bytes, hipMemcpyHostToDevice, c->stream));
    return MI_OK;
}

int mislam::allreduce_min_u64(mi_ctx* c, unsigned long long* dev_ptr, size_t count)
{
    if (c->exchange) return exchange_on_host(c, dev_ptr, count, MI_EXCHANGE_MIN_U64);
    if (!c->comm) return MI_OK;
    MI_NCCL(ncclAllReduce(dev_ptr, dev_ptr, count, ncclUint64, ncclMin, c->comm, c->stream));
    return MI_OK;
}

int mislam::allreduce_sum_f64(mi_ctx* c, double* dev_ptr, size_t count)
{
    if (c->exchange) return exchange_on_host(c, dev_ptr, count, MI_EXCHANGE_SUM_F64);
    if (!c->comm) return MI_OK;
    MI_NCCL(ncclAllReduce(dev_ptr, dev_ptr, count, ncclDouble, ncclSum, c->comm, c->stream));
    return MI_OK;
}

extern "C" int mi_ctx_rank(const mi_ctx* ctx, int* rank, int* world)
{
    if (!ctx) { set_error("mi_ctx_rank: null context"); return MI_ERR_INVALID_ARG; }
    if (rank) *rank = ctx->rank;
    if (world) *world = ctx->world;
    return MI_OK;
}

extern "C" int mi_dist_info(mi_ctx* c, int* nranks, int* rank, unsigned long long* ranks_seen)
{
    if (!c) { set_error("mi_dist_info: null context"); return MI_ERR_INVALID_ARG; }
    MI_ENTER(c);
    int n = c->world, r = c->rank;
    if (c->comm) {
        MI_NCCL(ncclCommCount(c->comm, &n));
        MI_NCCL(ncclCommUserRank(c->comm, &r));
    }
    if (nranks) *nranks = n;
    if (rank) *rank = r;
    if (ranks_seen) {
        if (c->world > 52) { set_error("mi_dist_info: ranks_seen holds at most 52 ranks"); return MI_ERR_INVALID_ARG; }
        // 2^rank is exact in a double, and so is any sum of distinct powers of two below 2^53: the SUM all-reduce of the moments
        // path carries the mask
        MI_TRY(c->rows_reduced.reserve(64 * 18));
        const double mine = (double)(1ull << c->rank);
        MI_HIP(hipMemcpyAsync(c->rows_reduced.p, &mine, sizeof mine, hipMemcpyHostToDevice, c->stream));
        MI_TRY(allreduce_sum_f64(c, c->rows_reduced.p, 1));
        double all = 0.0;
        MI_HIP(hipMemcpyAsync(&all, c->rows_reduced.p, sizeof all, hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
        *ranks_seen = (unsigned long long)all;
    }
    return MI_OK;
}

extern "C" int mi_runtime_info(char* hip_path, char* rccl_path, int cap, int* hip_runtime_version, int* rccl_version)
{
    const auto object_of = [cap](const void* symbol, char* out) {
        if (!out || cap <= 0) return;
        Dl_info info;
        const char* name = (dladdr(symbol, &info) != 0 && info.dli_fname) ? info.dli_fname : "";
        snprintf(out, (size_t)cap, "%s", name);
    };
    object_of(reinterpret_cast<const void*>(&hipStreamSynchronize), hip_path);
    object_of(reinterpret_cast<const void*>(&ncclAllReduce), rccl_path);
    if (hip_runtime_version) {
        int v = 0;
        if (hipRuntimeGetVersion(&v) != hipSuccess) v = -1;      // (no device needed: the runtime's own build number)
        *hip_runtime_version = v;
    }
    if (rccl_version) {
        int v = 0;
        if (ncclGetVersion(&v) != ncclSuccess) v = -1;
        *rccl_version = v;
    }
    return MI_OK;
}

extern "C" int mi_shard_range(int m_total, int rank, int world, int* lo, int* hi)
{
    if (m_total < 0 || world < 1 || rank < 0 || rank >= world || !lo || !hi) { set_error("mi_shard_range: bad arguments"); return MI_ERR_INVALID_ARG; }
    *lo = (int)((long long)m_total * rank / world);
    *hi = (int)((long long)m_total * (rank + 1) / world);
    return MI_OK;
}

extern "C" int mi_source_share(int n_total, int rank, int world, int* count)
{
    if (n_total < 0 || world < 1 || rank < 0 || rank >= world || !count) { set_error("mi_source_share: bad arguments"); return MI_ERR_INVALID_ARG; }
    if (n_total < 4 * ICP_CHUNK_POINTS * world) {                                   // too few chunks to deal: contiguous slices
        *count = (int)((long long)n_total * (rank + 1) / world) - (int)((long long)n_total * rank / world);
        return MI_OK;
    }
    const int chunks = (n_total + ICP_CHUNK_POINTS - 1) / ICP_CHUNK_POINTS;
    const int mine = (chunks - rank + world - 1) / world;                           // chunks rank, rank + W, ...
    const bool has_last = (chunks - 1) % world == rank;                             // the (possibly partial) last chunk of the cloud
    *count = mine * ICP_CHUNK_POINTS - (has_last ? chunks * ICP_CHUNK_POINTS - n_total : 0);
    return MI_OK;
}

extern "C" unsigned long long mi_pack_key(float d2, int global_index)
{
    unsigned int bits;
    memcpy(&bits, &d2, sizeof bits);
    return ((unsigned long long)bits << 32) | (unsigned int)global_index;
}

extern "C" void mi_unpack_key(unsigned long long key, float* d2, int* global_index)
{
    const unsigned int bits = (unsigned int)(key >> 32);
    if (d2) memcpy(d2, &bits, sizeof bits);
    if (global_index) *global_index = (int)(unsigned int)(key & 0xffffffffull);
}

namespace mislam { void cpd_workspace_destroy(mi_ctx* ctx); }

extern "C" void mi_ctx_destroy(mi_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->aux) (void)hipStreamSynchronize(c->aux);
    if (c->aux2) (void)hipStreamSynchronize(c->aux2);
    retire_buffers(c);
    if (c->comm) (void)ncclCommDestroy(c->comm);
    if (c->exchange_host) (void)hipHostFree(c->exchange_host);
    for (hipEvent_t e : c->pin.event) if (e) (void)hipEventDestroy(e);
    if (c->pin.buf) (void)hipHostFree(c->pin.buf);
    if (c->h_scratch) (void)hipHostFree(c->h_scratch);
    cpd_workspace_destroy(c);
    search_front_destroy_events(c);
    for (auto& s : c->prof.spans) { (void)hipEventDestroy(s.e0); (void)hipEventDestroy(s.e1); }
    for (auto e : c->prof.event_pool) (void)hipEventDestroy(e);
    if (c->d_state) (void)hipFree(c->d_state);
    if (c->h_state) (void)hipHostFree(c->h_state);
    if (c->peek_event) (void)hipEventDestroy(c->peek_event);
    for (hipEvent_t e : c->aux_event) if (e) (void)hipEventDestroy(e);
    if (c->aux) (void)hipStreamDestroy(c->aux);
    if (c->aux2) (void)hipStreamDestroy(c->aux2);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    const int device = c->device;
    delete c;                                   // every DevBuf of the context frees itself here (device_free: on the allocation stream) ...
    pool_context_gone(device);                  // ... and the last context of a device trims the pool behind those frees
}

extern "C" int mi_ctx_synchronize(mi_ctx* c)
{
    if (!c) { set_error("mi_ctx_synchronize: null context"); return MI_ERR_INVALID_ARG; }
    MI_ENTER(c);
    MI_HIP(hipStreamSynchronize(c->stream));
    retire_buffers(c);
    return MI_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// profiling: HIP events on the context's own stream around each kernel launch
// ---------------------------------------------------------------------------------------------------------------
// Timing events WITHOUT the system-scope release a default event performs when it is recorded (hipEventDisableSystemFence): behind the search
// kernel that release writes back ~20 MB of dirty L2 lines, twice per step.  MISLAM_PROF_EVENT_FLAGS overrides (developer switch).
static unsigned int c_prof_event_flags()
{
    static const unsigned int flags = [] { const char* e = getenv("MISLAM_PROF_EVENT_FLAGS"); return e ? (unsigned int)strtoul(e, nullptr, 0) : (unsigned int)hipEventDisableSystemFence; }();
    return flags;
}

int mi_ctx::Profiler::begin(int kernel, hipStream_t stream)
{
    ProfileSpan s{};
    s.kernel = kernel;
    for (hipEvent_t* e : {&s.e0, &s.e1}) {
        if (!event_pool.empty()) { *e = event_pool.back(); event_pool.pop_back(); }
        else MI_HIP(hipEventCreateWithFlags(e, c_prof_event_flags()));
    }
    MI_HIP(hipEventRecord(s.e0, stream));
    spans.push_back(s);
    return MI_OK;
}

int mi_ctx::Profiler::span(int kernel, hipEvent_t* e0, hipEvent_t* e1)
{
    *e0 = *e1 = nullptr;
    if (!times(kernel)) return MI_OK;
    ProfileSpan s{};
    s.kernel = kernel;
    for (hipEvent_t* e : {&s.e0, &s.e1}) {
        if (!event_pool.empty()) { *e = event_pool.back(); event_pool.pop_back(); }
        else MI_HIP(hipEventCreateWithFlags(e, c_prof_event_flags()));
    }
    spans.push_back(s);
    *e0 = s.e0; *e1 = s.e1;
    return MI_OK;
}

int mi_ctx::Profiler::end(hipStream_t stream)
{
    MI_HIP(hipEventRecord(spans.back().e1, stream));
    return MI_OK;
}

int mi_ctx::Profiler::collect(hipStream_t stream)
{
    if (spans.empty()) return MI_OK;
    MI_HIP(hipStreamSynchronize(stream));
    for (auto& s : spans) {
        float t = 0.f;
        MI_HIP(hipEventElapsedTime(&t, s.e0, s.e1));
        ms[s.kernel] += t;
        n[s.kernel] += 1;
        event_pool.push_back(s.e0);
        event_pool.push_back(s.e1);
    }
    spans.clear();
    return MI_OK;
}

extern "C" int mi_profile_enable(mi_ctx* c, int enable)
{
    if (!c) { set_error("mi_profile_enable: null context"); return MI_ERR_INVALID_ARG; }
    MI_ENTER(c);
    MI_TRY(c->prof.collect(c->stream));
    c->prof.on = enable != 0;
    return MI_OK;
}

extern "C" int mi_profile_select(mi_ctx* c, unsigned int kernel_mask)
{
    if (!c) { set_error("mi_profile_select: null context"); return MI_ERR_INVALID_ARG; }
    c->prof.mask = kernel_mask;
    return MI_OK;
}

extern "C" int mi_profile_reset(mi_ctx* c)
{
    if (!c) { set_error("mi_profile_reset: null context"); return MI_ERR_INVALID_ARG; }
    MI_ENTER(c);
    MI_TRY(c->prof.collect(c->stream));
    for (int k = 0; k < MI_KERNEL_COUNT; k++) { c->prof.ms[k] = 0; c->prof.n[k] = 0; }
    return MI_OK;
}

// The counting build's counters (GRID_STATS_ROWS copies of GRID_STATS_COLS words), summed over the copies ([7] is a maximum)
static int search_counters(mi_ctx* c, unsigned long long (&sum)[GRID_STATS_COLS])
{
    const size_t words = (size_t)GRID_STATS_ROWS * GRID_STATS_COLS;
    for (int i = 0; i < GRID_STATS_COLS; i++) sum[i] = 0;
    if (!c->nn_stats_on) return MI_OK;
    std::vector<unsigned long long> h(words);
    MI_HIP(hipMemcpyAsync(h.data(), c->nn_stats.p, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    for (size_t r = 0; r < (size_t)GRID_STATS_ROWS; r++)
        for (int i = 0; i < GRID_STATS_COLS; i++) sum[i] = i == 7 ? std::max(sum[i], h[r * GRID_STATS_COLS + i]) : sum[i] + h[r * GRID_STATS_COLS + i];
    return MI_OK;
}

extern "C" int mi_profile_search_stats(mi_ctx* c, int enable, unsigned long long out[8])
{
    if (!c) { set_error("mi_profile_search_stats: null context"); return MI_ERR_INVALID_ARG; }
    MI_ENTER(c);
    const size_t words = (size_t)GRID_STATS_ROWS * GRID_STATS_COLS;
#ifdef MISLAM_DEV_WAVE_TIMELINE        // developer build: 4 words per wave of the last search behind the counters, dumped to $MISLAM_DEV_TIMELINE_FILE
    const size_t tl_words = (size_t)16 * (1u << 18);
    MI_TRY(c->nn_stats.reserve(words + tl_words));
    if (out && c->nn_stats_on && getenv("MISLAM_DEV_TIMELINE_FILE")) {
        std::vector<unsigned long long> tl(tl_words);
        MI_HIP(hipMemcpyAsync(tl.data(), c->nn_stats.p + words, sizeof(unsigned long long) * tl_words, hipMemcpyDeviceToHost, c->stream));
        MI_HIP(hipStreamSynchronize(c->stream));
        if (FILE* f = fopen(getenv("MISLAM_DEV_TIMELINE_FILE"), "wb")) { fwrite(tl.data(), sizeof(unsigned long long), tl_words, f); fclose(f); }
    }
#endif
    MI_TRY(c->nn_stats.reserve(words));
    if (out) {
        unsigned long long sum[GRID_STATS_COLS];
        MI_TRY(search_counters(c, sum));
        for (int i = 0; i < 8; i++) out[i] = sum[i];
    }
    c->nn_stats_on = enable != 0;
    if (enable) MI_HIP(hipMemsetAsync(c->nn_stats.p, 0, sizeof(unsigned long long) * words, c->stream));
    return MI_OK;
}

extern "C" int mi_profile_search_phases(mi_ctx* c, unsigned long long out[20])
{
    if (!c || !out) { set_error("mi_profile_search_phases: null argument"); return MI_ERR_INVALID_ARG; }
    MI_ENTER(c);
    if (!c->nn_stats_on) { set_error("mi_profile_search_phases: counting is off (mi_profile_search_stats(ctx, 1, NULL) first)"); return MI_ERR_STATE; }
    unsigned long long sum[GRID_STATS_COLS];
    MI_TRY(search_counters(c, sum));
    static_assert(GRID_STATS_COLS >= 8 + 20, "phases: 20 counters behind the 8 of mi_profile_search_stats");
    for (int i = 0; i < 20; i++) out[i] = sum[8 + i];
    return MI_OK;
}

extern "C" int mi_selftest_fail_loads(mi_ctx* c, int n)
{
    if (!c || n < 0) { set_error("mi_selftest_fail_loads: bad argument"); return MI_ERR_INVALID_ARG; }
    c->selftest_fail_loads = n;
    return MI_OK;
}

extern "C" int mi_selftest_live_buffers(long long* count)
{
    if (!count) { set_error("mi_selftest_live_buffers: null argument"); return MI_ERR_INVALID_ARG; }
    *count = g_live_buffers.load();
    return MI_OK;
}

extern "C" int mi_selftest_sort_pairs(mi_ctx* c, unsigned int* keys, int* values, int n, int bits)
{
    if (!c || n < 0 || (n > 0 && (!keys || !values)) || (bits != 10 && bits != 20 && bits != 30)) {
        set_error("mi_selftest_sort_pairs: bad argument");
        return MI_ERR_INVALID_ARG;
    }
    if (n == 0) return MI_OK;
    MI_ENTER(c);
    DevBuf<unsigned int> k0, k1;
    DevBuf<int> v0, v1;
    DevBuf<unsigned char> temp;
    MI_TRY(k0.reserve((size_t)n)); MI_TRY(k1.reserve((size_t)n)); MI_TRY(v0.reserve((size_t)n)); MI_TRY(v1.reserve((size_t)n));
    MI_TRY(temp.reserve(radix_sort_temp_bytes(n)));
    MI_HIP(hipMemcpyAsync(k0.p, keys, sizeof(unsigned int) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    MI_HIP(hipMemcpyAsync(v0.p, values, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    MI_HIP(radix_sort_pairs_u32(temp.p, k0.p, k1.p, v0.p, v1.p, n, bits, c->stream));
    MI_HIP(hipMemcpyAsync(keys, k1.p, sizeof(unsigned int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipMemcpyAsync(values, v1.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    return MI_OK;
}

// the range pass of cloud_range.hpp and nothing else: SoA loader, block cap 256, the result as six floats and one index
template <class Pred>
__global__ __launch_bounds__(256) void selftest_range_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                             int n, float* __restrict__ lo_hi, int* __restrict__ bad)
{
    range_block(SoaPoints{x, y, z}, Pred{}, n, lo_hi, bad);
}
template <int NBAD>
__global__ __launch_bounds__(256) void selftest_range_finish_kernel(const float* __restrict__ lo_hi, const int* __restrict__ bad, int nblocks,
                                                                    float* __restrict__ out)
{
    RangeAcc a;
    if (!range_finish<NBAD>(a, lo_hi, nblocks, bad)) return;
#pragma unroll
    for (int k = 0; k < 6; k++) out[k] = a.v[k];
    out[6] = __int_as_float(a.bad[0]);       // (RANGE_NO_POINT where nothing can be refused)
}

extern "C" int mi_selftest_cloud_range(mi_ctx* c, const float* xyz, int n, int check, float out_lo_hi[6], int* out_first_bad)
{
    if (!c || !xyz || !out_lo_hi || !out_first_bad || n < 1 || check < 0 || check > 2) {
        set_error("mi_selftest_cloud_range: bad argument");
        return MI_ERR_INVALID_ARG;
    }
    MI_ENTER(c);
    std::vector<float> soa((size_t)3 * n);
    for (int i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) soa[(size_t)k * n + i] = xyz[3 * (size_t)i + k];
    const int nb = range_blocks(n, 256);
    DevBuf<float> pts, lo_hi, out;
    DevBuf<int> bad;
    MI_TRY(pts.reserve((size_t)3 * n)); MI_TRY(lo_hi.reserve((size_t)6 * 256)); MI_TRY(bad.reserve(256)); MI_TRY(out.reserve(7));
    MI_HIP(hipMemcpyAsync(pts.p, soa.data(), sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    const float *x = pts.p, *y = pts.p + n, *z = pts.p + 2 * (size_t)n;
    if (check == 0) {
        hipLaunchKernelGGL(selftest_range_kernel<AnyPoint>, dim3(nb), dim3(256), 0, c->stream, x, y, z, n, lo_hi.p, bad.p);
        hipLaunchKernelGGL(selftest_range_finish_kernel<0>, dim3(1), dim3(256), 0, c->stream, lo_hi.p, bad.p, nb, out.p);
    } else {
        if (check == 1) hipLaunchKernelGGL(selftest_range_kernel<FinitePoint>, dim3(nb), dim3(256), 0, c->stream, x, y, z, n, lo_hi.p, bad.p);
        else hipLaunchKernelGGL(selftest_range_kernel<UsablePoint>, dim3(nb), dim3(256), 0, c->stream, x, y, z, n, lo_hi.p, bad.p);
        hipLaunchKernelGGL(selftest_range_finish_kernel<1>, dim3(1), dim3(256), 0, c->stream, lo_hi.p, bad.p, nb, out.p);
    }
    MI_HIP(hipGetLastError());
    float h[7];
    MI_HIP(hipMemcpyAsync(h, out.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    MI_HIP(hipStreamSynchronize(c->stream));
    memcpy(out_lo_hi, h, 6 * sizeof(float));
    memcpy(out_first_bad, &h[6], sizeof(int));
    return MI_OK;
}

extern "C" int mi_profile_get(mi_ctx* c, int kernel, double* total_ms, long long* launches)
{
    if (!c || kernel < 0 || kernel >= MI_KERNEL_COUNT) { set_error("mi_profile_get: bad argument"); return MI_ERR_INVALID_ARG; }
    MI_ENTER(c);
    MI_TRY(c->prof.collect(c->stream));
    if (total_ms) *total_ms = c->prof.ms[kernel];
    if (launches) *launches = c->prof.n[kernel];
    return MI_OK;
}
