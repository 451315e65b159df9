// K64 - K67 Scan Context descriptors and their exact search (driver: scan_context_api.hip; the contracts: mi_scan_context and
// mi_scan_context_search in mi_slam.h; the binning's arithmetic: scan_context_bin.hpp).
//   K64 sc_bins:      a workgroup owns one slice of one scan.  The slice's descriptor lives in the LDS as unsigned integers: a bin holds the
//                     bits of the largest positive z + z_offset met so far, and positive fp32 values order as their bits do, so the maximum
//                     is an integer atomicMax, in the LDS and then once per non-empty bin in the scan's descriptor.  A bin nobody touched
//                     stays 0 = +0.  The maximum does not depend on the order of arrival, nor on what else is in the batch.
//   K65 sc_normalise: one wave per descriptor, lane j its sector j: the column's sum of squares in fp64, rings ascending, its root, every
//                     component divided in fp64 and rounded to fp32 once; the wave's ballot of the non-empty columns is the row's mask.
//   K66 sc_search:    a workgroup of SC_SEARCH_WAVES waves owns one query and one chunk of database rows; wave w takes the rows w,
//                     w + SC_SEARCH_WAVES, ... of the chunk.  The query's unit columns are the A operand of v_mfma_f32_32x32x2_f32 and stay
//                     in registers for the whole chunk; a row's unit columns are the B operand, read from global memory straight into
//                     registers (the next row's while this row's diagonals are summed).  sectors x rings x sectors, padded to 64 x 2 KS x 64
//                     (32 x 2 KS x 32 up to 32 sectors) with zeros, is two by two accumulators of 32 x 32: G(j, k) with k on the lane and j
//                     in the registers.  They go to the wave's own LDS tile, and lane s walks the wrapped diagonal k = (j + s) mod sectors,
//                     j ascending, adding 1 - G in fp64 where both columns are non-empty -- the pair mask of shift s is the query's mask
//                     and the row's mask rotated by s, its popcount the divisor.  Padding never reaches a diagonal: the walk stays below
//                     `sectors` in both indices, and a zero k-step leaves the chain's bits alone.  Lane s keeps the minimum of its shift over
//                     the wave's rows (rows ascend, strict <: the lowest row on ties); the lanes' minima are merged by atomicMin on
//                     (ordered(distance) << 32 | row << 6 | shift), which is the contract's order: distance, then row, then shift.
//   K67 sc_finish:    the keys unpacked.
// No scratch, no floating-point atomics.  Registers and LDS: DESIGN.md, K64-K67.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "scan_context_bin.hpp"

namespace mislam {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void sc_bins_kernel(const ScBinArgs a)
{
    __shared__ unsigned int bins[SC_MAX_RINGS * SC_MAX_SECTORS];
    __shared__ double edge2[SC_MAX_RINGS + 1];
    __shared__ double dir[2 * SC_MAX_SECTORS];

    const int scan = blockIdx.x;
    const int lo = a.offsets[scan], hi = a.offsets[scan + 1];
    const long long begin = (long long)lo + (long long)blockIdx.y * (long long)a.slice;
    if (begin >= (long long)hi) return;                              // uniform over the workgroup, in front of every barrier
    const long long end = begin + a.slice < (long long)hi ? begin + a.slice : (long long)hi;
    const int rings = a.rings, sectors = a.sectors, nb = rings * sectors;

    for (int e = threadIdx.x; e < nb; e += 256) bins[e] = 0u;
    if ((int)threadIdx.x <= rings) edge2[threadIdx.x] = a.ring_edge2[threadIdx.x];
    if ((int)threadIdx.x < 2 * sectors) dir[threadIdx.x] = a.sector_dir[threadIdx.x];
    __syncthreads();

    const double cx = a.centres ? (double)a.centres[3 * (size_t)scan] : 0.0;
    const double cy = a.centres ? (double)a.centres[3 * (size_t)scan + 1] : 0.0;
    for (long long i = begin + threadIdx.x; i < end; i += 256) {
        const float x = a.xyz[3 * (size_t)i], y = a.xyz[3 * (size_t)i + 1], z = a.xyz[3 * (size_t)i + 2];
        if (!(__builtin_fabsf(x) <= SC_MAX_ABS && __builtin_fabsf(y) <= SC_MAX_ABS && __builtin_fabsf(z) <= SC_MAX_ABS)) {     // false for a NaN
            atomicMin(a.bad, (int)i);
            continue;
        }
        const double dx = (double)x - cx, dy = (double)y - cy;
        const double xx = dx * dx, yy = dy * dy;
        const int r = sc_ring(xx + yy, edge2, rings);
        if (r < 0) continue;
        const float v = z + a.z_offset;
        if (!(v > 0.f)) continue;
        atomicMax(&bins[r * sectors + sc_sector(dx, dy, dir, sectors)], __float_as_uint(v));
    }
    __syncthreads();
    unsigned int* out = a.desc + (size_t)scan * (size_t)nb;
    for (int e = threadIdx.x; e < nb; e += 256)
        if (bins[e] != 0u) atomicMax(&out[e], bins[e]);
}

__global__ __launch_bounds__(256) void sc_normalise_kernel(const float* __restrict__ desc, int rows, int rings, int sectors, float* __restrict__ unit,
                                                           unsigned long long* __restrict__ mask, int* bad)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                         // wave-uniform; the kernel has no barrier
    const bool in = lane < sectors;
    const size_t base = (size_t)row * (size_t)rings * (size_t)sectors + (size_t)lane;
    double ss = 0.0;
    bool ok = true;
    for (int r = 0; r < rings; r++) {
        const float v = in ? desc[base + (size_t)r * sectors] : 0.f;
        ok = ok && (v >= 0.f && v <= 3.402823466e38f);               // false for a NaN, an infinity and a negative value
        const double w = (double)v;
        ss = ss + w * w;                                             // the product is exact, the sum rounds once
    }
    const double norm = __builtin_sqrt(ss);
    if (in)
        for (int r = 0; r < rings; r++) {
            const float v = desc[base + (size_t)r * sectors];
            unit[base + (size_t)r * sectors] = ss > 0.0 ? (float)((double)v / norm) : 0.f;
        }
    const unsigned long long m = __ballot(in && ss > 0.0);
    if (lane == 0) mask[row] = m;
    if (!ok) atomicMin(bad, (int)row);
}

// a float as an unsigned that orders the same way, and back
__device__ __forceinline__ unsigned int sc_ordered(float h)
{
    const unsigned int u = __float_as_uint(h);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sc_unordered(unsigned int o) { return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o); }

// component 2 s + half of sector col + 32 t of one descriptor's unit columns, zero beyond rings and sectors
template <int KS>
__device__ __forceinline__ void sc_load_operand(const float* __restrict__ u, int R, int S, int col, int half, float (&v)[2][KS])
{
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int s = 0; s < KS; s++) {
            const int r = 2 * s + half, k = col + 32 * t;
            v[t][s] = (r < R && k < S) ? u[r * S + k] : 0.f;
        }
}

constexpr int SC_G_STRIDE = 72;              // floats between rows of a wave's G tile: the two halves of a wave (rows 4 apart) write disjoint banks

template <int KS>
__global__ __launch_bounds__(64 * SC_SEARCH_WAVES) void sc_search_kernel(const ScSearchArgs a)
{
    __shared__ float g_all[SC_SEARCH_WAVES * 64 * SC_G_STRIDE];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int qi = blockIdx.x;
    const int R = a.rings, S = a.sectors;
    const size_t RS = (size_t)R * (size_t)S;
    float* g = g_all + wave * 64 * SC_G_STRIDE;

    int lim = a.limit ? a.limit[qi] : a.nd;
    if (lim > a.nd) lim = a.nd;
    const int ex = a.exclude ? a.exclude[qi] : -1;
    const long long begin = (long long)blockIdx.y * (long long)a.chunk_len;
    if (begin >= (long long)lim) return;                             // the kernel has no workgroup barrier
    const int end = begin + a.chunk_len < (long long)lim ? (int)(begin + a.chunk_len) : lim;
    const bool two = S > 32;                                         // two tiles of 32 sectors a side

    float qv[2][KS], cv[2][KS];
    sc_load_operand<KS>(a.q_unit + (size_t)qi * RS, R, S, col, half, qv);
    const unsigned long long qmask = a.q_mask[qi];
    const unsigned long long all = S == 64 ? ~0ull : ((1ull << S) - 1ull);

    float best = __builtin_inff();
    int best_row = SC_NO_INDEX;
    int row = (int)begin + wave;
    if (row < end) sc_load_operand<KS>(a.d_unit + (size_t)row * RS, R, S, col, half, cv);
    for (; row < end; row += SC_SEARCH_WAVES) {
        f32x16 acc[2][2];
#pragma unroll
        for (int jt = 0; jt < 2; jt++)
#pragma unroll
            for (int kt = 0; kt < 2; kt++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[jt][kt][r] = 0.f;
#pragma unroll
        for (int s = 0; s < KS; s++) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(qv[0][s], cv[0][s], acc[0][0], 0, 0, 0);
            if (two) {
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(qv[0][s], cv[1][s], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(qv[1][s], cv[0][s], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(qv[1][s], cv[1][s], acc[1][1], 0, 0, 0);
            }
        }
        const unsigned long long cmask = a.d_mask[row];
        const int next = row + SC_SEARCH_WAVES;
        if (next < end) sc_load_operand<KS>(a.d_unit + (size_t)next * RS, R, S, col, half, cv);     // in flight while the diagonals are summed

        // acc[jt][kt][r] = G(j, k), j = 32 jt + (r & 3) + 8 (r >> 2) + 4 half (a sector of the query), k = 32 kt + col (a sector of the row)
#pragma unroll
        for (int jt = 0; jt < 2; jt++)
#pragma unroll
            for (int kt = 0; kt < 2; kt++)
                if (two || (jt == 0 && kt == 0)) {
#pragma unroll
                    for (int r = 0; r < 16; r++) g[(32 * jt + (r & 3) + 8 * (r >> 2) + 4 * half) * SC_G_STRIDE + 32 * kt + col] = acc[jt][kt][r];
                }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");       // the tile is the wave's own: its lanes wait for each other's stores only
        __builtin_amdgcn_wave_barrier();

        if (lane < S && row != ex) {
            const int s = lane;
            const unsigned long long rot = s == 0 ? cmask : (((cmask >> s) | (cmask << (S - s))) & all);     // bit j: the row's column (j + s) mod S
            const unsigned long long pair = qmask & rot;
            double sum = 0.0;
            int k = s;
            for (int j = 0; j < S; j++) {
                const double term = 1.0 - (double)g[j * SC_G_STRIDE + k];
                sum = sum + (((pair >> j) & 1ull) ? term : 0.0);
                k = k + 1 == S ? 0 : k + 1;
            }
            const int cnt = __popcll(pair);
            const float d = cnt ? (float)(sum / (double)cnt) : 1.0f;
            if (d < best) { best = d; best_row = row; }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");       // every lane has read the tile before the next row's stores
        __builtin_amdgcn_wave_barrier();
    }
    if (lane < S && best_row != SC_NO_INDEX)
        atomicMin(&a.keys[qi], ((unsigned long long)sc_ordered(best) << 32) | ((unsigned long long)(unsigned int)best_row << 6) | (unsigned long long)lane);
}

__global__ __launch_bounds__(256) void sc_finish_kernel(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ keys2, int nq,
                                                        int* __restrict__ idx, float* __restrict__ dist, int* __restrict__ shift, float* __restrict__ second)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const unsigned long long k = keys[i];
    const bool none = k == ~0ull;
    idx[i] = none ? -1 : (int)((unsigned int)(k & 0xffffffffull) >> 6);
    dist[i] = none ? __builtin_inff() : sc_unordered((unsigned int)(k >> 32));
    shift[i] = none ? 0 : (int)(k & 63ull);
    if (second) {
        const unsigned long long k2 = keys2[i];
        second[i] = k2 == ~0ull ? __builtin_inff() : sc_unordered((unsigned int)(k2 >> 32));
    }
}

bool sc_shape_ok(int rings, int sectors) { return rings >= 1 && rings <= SC_MAX_RINGS && sectors >= 1 && sectors <= SC_MAX_SECTORS; }

}  // namespace

hipError_t sc_bins(const ScBinArgs& a, int longest_scan, hipStream_t s)
{
    if (a.n_scans < 1 || !sc_shape_ok(a.rings, a.sectors) || a.slice < 1 || longest_scan < 0) return hipErrorInvalidValue;
    const long long slices = longest_scan == 0 ? 1 : ((long long)longest_scan + a.slice - 1) / a.slice;
    if (slices > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sc_bins_kernel, dim3((unsigned int)a.n_scans, (unsigned int)slices), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t sc_normalise(const float* desc, int rows, int rings, int sectors, float* unit, unsigned long long* mask, int* bad, hipStream_t s)
{
    if (rows < 1 || !sc_shape_ok(rings, sectors)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sc_normalise_kernel, dim3((unsigned int)(((long long)rows + 3) / 4)), dim3(256), 0, s, desc, rows, rings, sectors, unit, mask, bad);
    return hipGetLastError();
}

int sc_chunk_len(int nq, int nd, int cu_count)
{
    const long long units = ((long long)nd + SC_SEARCH_CHUNK - 1) / SC_SEARCH_CHUNK;
    long long chunks = (8LL * cu_count + nq - 1) / nq;               // eight workgroups per CU where the queries alone do not give them
    if (chunks < 1) chunks = 1;
    if (chunks > units) chunks = units;
    if (chunks > 65535) chunks = 65535;                              // grid.y
    return (int)((units + chunks - 1) / chunks) * SC_SEARCH_CHUNK;
}

hipError_t sc_search(const ScSearchArgs& a, hipStream_t s)
{
    if (a.nq < 1 || a.nd < 1 || a.nd > (1 << SC_ROW_BITS) || !sc_shape_ok(a.rings, a.sectors) || a.chunk_len < SC_SEARCH_CHUNK ||
        a.chunk_len % SC_SEARCH_CHUNK != 0)
        return hipErrorInvalidValue;
    const long long chunks = ((long long)a.nd + a.chunk_len - 1) / a.chunk_len;
    if (chunks > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned int)a.nq, (unsigned int)chunks), block(64 * SC_SEARCH_WAVES);
    if (a.rings <= 8) hipLaunchKernelGGL(sc_search_kernel<4>, grid, block, 0, s, a);
    else if (a.rings <= 20) hipLaunchKernelGGL(sc_search_kernel<10>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(sc_search_kernel<16>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t sc_finish(const unsigned long long* keys, const unsigned long long* keys2, int nq, int* idx, float* dist, int* shift, float* second, hipStream_t s)
{
    if (nq < 1 || (second && !keys2)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sc_finish_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, keys, keys2, nq, idx, dist, shift, second);
    return hipGetLastError();
}

// loads this translation unit's code object at mi_ctx_preload (kernels.h)
__global__ void preload_scan_context_kernels_kernel() {}
hipError_t preload_scan_context_kernels()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(preload_scan_context_kernels_kernel));
}

}  // namespace mislam
