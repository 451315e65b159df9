// K34 - K38 -- density-based clustering (mi_cluster_dbscan; driver: cluster_api.hip).  K34 and K35 are the fixed-radius walk of K15's radius
// method (shell_walk, knn_scan.hpp) over ONE cell grid, one lane per point in curve order, with a sink of their own; the core flags they
// read are K15's early count (count[j] >= need), taken in a launch before them.
//
//   K34 link      a core lane walks its ball and unites itself with every core candidate j < i within r2 (d2 is symmetric bit for bit, so
//                 the pair (i, j) is met from both ends and taken from the higher one: every edge once) in parent[], a union-find over the
//                 caller's indices.  Lanes cooperate through global memory and through nothing else: no LDS, no scratch, no barrier.
//   K35 resolve   a second launch.  A core lane writes the root of its tree; a lane that is not core walks its ball for the core candidate
//                 with the smallest key (bits(d2) << 32) | j (NearestSink's rule with the core filter) and writes that one's root, or -1.
//   K36 sizes     size[root] += 1 over the points with a root (integer adds: any order gives the same sum; one add per wave and root),
//                 then keep[i] = "i is a root and its size passes the filter".  K15's compaction turns keep into the ascending list of
//                 surviving roots; K37 scatters rank[root] = c and the sizes, K38 writes labels[i] = rank[root_of[i]] or -1.
//
// The union-find of K34, and why it is right whatever the memory system shows a lane.
//   State: parent[x] for every caller index x, the identity before the launch.  Three operations ever write it:
//     hook      atomicCAS(&parent[hi], hi, lo) with lo < hi: succeeds only if parent[hi] == hi AT THAT MOMENT, i.e. hi is a root then;
//     shorten   atomicMin(&parent[x], m) with m < x a member of x's set (below);
//     nothing else -- no plain store, so no store can race the CAS.
//   Invariant 1: parent[x] <= x, always, and every value parent[x] ever held is x itself or a member of x's set at the time it was
//     stored.  Sets only grow (no operation splits one), so a STALE value of parent[x] -- L1 is per CU and L2 per XCD; a read may return
//     any value the word held earlier in the launch -- is still x or a smaller member of x's set.  Reads are relaxed agent-scope atomic
//     loads so that they bypass L1 and are not hoisted, but nothing below rests on their freshness.
//   Invariant 2: the edges x -> parent[x] < x form a forest, and the one root of a set is its smallest index.  A hook puts the root hi
//     under lo < hi: lo need not be a root any more, the merged set's root is lo's set's root, which is <= lo < hi = the smallest index
//     of hi's set.  A shortening moves a non-root x (a set that holds m < x has a root below x, and a node that has been hooked never
//     becomes a root again) under a smaller member of its own set: sets and roots are unchanged, edges still point downwards.
//   find(x) follows parents while they are below x; by invariant 1 it returns a member of x's set (possibly not the root, if what it
//     read was stale).  unite(a, b) finds both, returns if they are equal (then a and b are in one set), and tries the hook of the larger
//     under the smaller.  If the CAS succeeds the sets of a and b are one.  If it fails it returns the value it found, a member of hi's
//     set below hi, and the lane goes on from that value and lo: still one member of each set.  So unite ends only with the two sets
//     joined, and only a CAS on a word that is a root at that moment ever hooks.
//   Progress: no lane ever waits for another lane: every loop below strictly decreases an index (find: x; unite: the larger of its two
//     ends, since a failed CAS hands back a value below hi), so a lane leaves find after at most x steps and unite after at most n rounds
//     whatever the other lanes do, and the lockstep of a wave cannot deadlock it.  A round of unite beyond the first follows another
//     lane's successful hook of that very word, and a launch has at most n - 1 successful hooks.
//   Result: when the launch ends, two core points are in one set iff a chain of core neighbours joins them (every edge was united by
//     its higher end; nothing else was), and the kernel boundary makes parent[] visible to K35's plain loads.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "knn_scan.hpp"
#include "nn_grid.h"

namespace mislam {

namespace {

__device__ __forceinline__ int uf_parent(const int* parent, int x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a member of x's set at or below x: the root, if every read was fresh.  x decreases strictly: at most x steps (the unsigned
// comparison ends the loop on anything that is not a smaller index, whatever the word holds)
__device__ __forceinline__ int uf_find(const int* parent, int x)
{
    for (;;) {
        const int p = uf_parent(parent, x);
        if ((unsigned int)p >= (unsigned int)x) return x;
        x = p;
    }
}

// joins the sets of a and b; returns a member of the joined set at or below both ends.  The larger end decreases strictly from round to
// round: at most n rounds, and every round but the first follows another lane's hook of parent[hi] (at most n - 1 in a launch)
__device__ __forceinline__ int uf_unite(int* parent, int a, int b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicCAS(parent + hi, hi, lo);
        if ((unsigned int)old >= (unsigned int)hi) return lo;                       // old == hi: hooked
        a = old; b = lo;                                                            // hi was hooked under old < hi meanwhile: go on from there
    }
}

// K34's sink: the reach is r2, a point AT r2 belongs (RadiusCountSink's rule), the stop is strict.  `mine`: a member of the lane's own
// set at or below the lane's index, the lowest the lane has seen
struct ClusterLinkSink {
    static constexpr bool LEAVES = false;
    unsigned int self;
    float r2;
    const int* count;
    int need;
    int* parent;
    int mine;
    __device__ __forceinline__ bool take(float d2, unsigned int pj)
    {
        if (pj < self && d2 <= r2 && (!count || count[pj] >= need)) {               // (pj < n: the index the grid build stored)
            const int pp = uf_parent(parent, (int)pj);                              // a member of j's set
            if (pp != mine) mine = uf_unite(parent, mine, pp);                      // (equal: j hangs under the lane's own ancestor already)
        }
        return false;
    }
    __device__ __forceinline__ bool stop(float bound) const { return bound > r2; }
};

// K35's sink for a lane that is not core: NearestSink with the core filter (the lane itself is not core, so it never takes itself)
struct ClusterBorderSink {
    static constexpr bool LEAVES = false;
    unsigned long long best;
    float r2;
    const int* count;
    int need;
    __device__ __forceinline__ bool take(float d2, unsigned int pj)
    {
        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | pj;
        if (key < best && d2 <= r2 && count[pj] >= need) best = key;
        return false;
    }
    __device__ __forceinline__ bool stop(float bound) const
    {
        const float nearest = __uint_as_float((unsigned int)(best >> 32));             // (+inf while nothing was taken)
        return bound > nearest || bound > r2;
    }
};

__global__ __launch_bounds__(256) void cluster_identity_kernel(int* __restrict__ parent, int n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)n) parent[i] = (int)i;
}

template <bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) void cluster_link_kernel(NnGridView g, ClusterLinkArgs a)
{
    float q[3];
    int row_out;
    if (!knn_lane(a.q, q, row_out)) return;
    if (a.count && a.count[row_out] < a.need) return;                               // not core: no edge of its own
    ClusterLinkSink sink{(unsigned int)row_out, a.r2, a.count, a.need, a.parent, row_out};
    shell_walk<FMA>(g, q, a.q.hi, sink);
    // shorten: sink.mine < row_out is a smaller member of the lane's set, so row_out is no root and never will be one (invariant 2)
    if (sink.mine < row_out) atomicMin(a.parent + row_out, sink.mine);
}

template <bool FMA>
__global__ __launch_bounds__(KNN_BLOCK) void cluster_resolve_kernel(NnGridView g, ClusterResolveArgs a)
{
    float q[3];
    int row_out;
    if (!knn_lane(a.q, q, row_out)) return;
    const bool core = !a.count || a.count[row_out] >= a.need;
    int at = row_out;
    if (!core) {
        ClusterBorderSink sink{KNN_KEY_EMPTY, a.r2, a.count, a.need};
        shell_walk<FMA>(g, q, a.q.hi, sink);
        at = sink.best == KNN_KEY_EMPTY ? -1 : (int)(unsigned int)(sink.best & 0xffffffffull);
    }
    if (at >= 0) {                                                                  // the root of `at`: plain loads behind the kernel boundary; `at` decreases strictly
        for (;;) {
            const int p = a.parent[at];
            if ((unsigned int)p >= (unsigned int)at) break;
            at = p;
        }
    }
    a.root_of[row_out] = at;
    a.is_core[row_out] = core ? 1 : 0;
}

// size[r] += the points of this wave whose root is r: one add per wave and distinct root (a large cluster's points would otherwise meet
// in one word one by one)
__global__ __launch_bounds__(256) void cluster_size_kernel(ClusterNumberArgs a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int r = i < (size_t)a.n ? a.root_of[i] : -1;
    const bool has = r >= 0;                                                        // (r < n: a caller index K35 wrote)
    unsigned long long todo = __builtin_amdgcn_ballot_w64(has);
    while (todo) {                                                                  // (uniform over the wave; one round per distinct root, at most 64)
        const int leader = (int)__builtin_ctzll(todo);
        const int lr = __shfl(r, leader, 64);
        const unsigned long long same = __builtin_amdgcn_ballot_w64(has && r == lr);
        if (lane == leader) atomicAdd(a.size + lr, (int)__builtin_popcountll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(256) void cluster_keep_kernel(ClusterNumberArgs a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.n) return;
    const int sz = a.size[i];
    a.keep[i] = a.root_of[i] == (int)i && sz >= a.min_size && (a.max_size == 0 || sz <= a.max_size) ? 1 : 0;
}

__global__ __launch_bounds__(256) void cluster_rank_kernel(ClusterNumberArgs a)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= (size_t)a.n || (long long)c >= a.state->kept) return;
    const int r = a.roots[c];                                                       // (< n: an index of a one in keep)
    a.rank[r] = (int)c;
    if (a.sizes_out && c < (size_t)a.cap) a.sizes_out[c] = a.size[r];
}

__global__ __launch_bounds__(256) void cluster_label_kernel(ClusterNumberArgs a)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)a.n) return;
    const int r = a.root_of[i];
    const int label = r >= 0 && a.keep[r] ? a.rank[r] : -1;
    a.labels[i] = label;
    if (a.labelled) a.labelled[i] = label >= 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void cluster_group_keys_kernel(const int* __restrict__ labels, const int* __restrict__ index, int count, int shift,
                                                                 unsigned int* __restrict__ keys)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < (size_t)count) keys[k] = (unsigned int)labels[index[k]] >> shift;
}

unsigned int blocks256(int n) { return (unsigned int)(((long long)n + 255) / 256); }

}  // namespace

hipError_t cluster_identity(int* parent, int n, hipStream_t s)
{
    if (n < 1 || !parent) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cluster_identity_kernel, dim3(blocks256(n)), dim3(256), 0, s, parent, n);
    return hipGetLastError();
}

hipError_t cluster_link(const NnGridView& g, const ClusterLinkArgs& a, int fma, hipStream_t s)
{
    if (a.q.n < 1 || !(a.r2 >= 0.f) || !a.parent || (a.count && a.need < 1)) return hipErrorInvalidValue;
    const dim3 grid((a.q.n + KNN_BLOCK - 1) / KNN_BLOCK), block(KNN_BLOCK);
    if (fma) hipLaunchKernelGGL((cluster_link_kernel<true>), grid, block, 0, s, g, a);
    else hipLaunchKernelGGL((cluster_link_kernel<false>), grid, block, 0, s, g, a);
    return hipGetLastError();
}

hipError_t cluster_resolve(const NnGridView& g, const ClusterResolveArgs& a, int fma, hipStream_t s)
{
    if (a.q.n < 1 || !(a.r2 >= 0.f) || !a.parent || !a.root_of || !a.is_core || (a.count && a.need < 1)) return hipErrorInvalidValue;
    const dim3 grid((a.q.n + KNN_BLOCK - 1) / KNN_BLOCK), block(KNN_BLOCK);
    if (fma) hipLaunchKernelGGL((cluster_resolve_kernel<true>), grid, block, 0, s, g, a);
    else hipLaunchKernelGGL((cluster_resolve_kernel<false>), grid, block, 0, s, g, a);
    return hipGetLastError();
}

hipError_t cluster_count_sizes(const ClusterNumberArgs& a, hipStream_t s)
{
    if (a.n < 1 || !a.root_of || !a.size || !a.keep || a.min_size < 1 || a.max_size < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cluster_size_kernel, dim3(blocks256(a.n)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(cluster_keep_kernel, dim3(blocks256(a.n)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t cluster_ranks(const ClusterNumberArgs& a, hipStream_t s)
{
    if (a.n < 1 || !a.roots || !a.state || !a.rank || !a.size || (a.sizes_out && a.cap < 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cluster_rank_kernel, dim3(blocks256(a.n)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t cluster_labels(const ClusterNumberArgs& a, hipStream_t s)
{
    if (a.n < 1 || !a.root_of || !a.keep || !a.rank || !a.labels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cluster_label_kernel, dim3(blocks256(a.n)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t cluster_group_keys(const int* labels, const int* index, int count, int shift, unsigned int* keys, hipStream_t s)
{
    if (count < 1 || shift < 0 || shift > 31 || !labels || !index || !keys) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cluster_group_keys_kernel, dim3(blocks256(count)), dim3(256), 0, s, labels, index, count, shift, keys);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_cluster_kernels_kernel() {}
hipError_t preload_cluster_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_cluster_kernels_kernel));
}

}  // namespace mislam
