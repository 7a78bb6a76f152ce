// PQ training for 16-bit sub-quantizers: the sorted centroid update.
//
// The contract fixes the order of every float sum: per (sub-quantizer m, centroid k, component d) ONE running sum over the members
// of k in ascending vector index (kmeans_fast_iterations_thread, databases.cpp:67-88, on the columns of m).  With 65536 centroids a
// chain cannot walk the whole learning set as pq_train_update_kernel's does, so the vectors are first put in (code, index) order:
//   pq_train16_hist_kernel     digit histogram of every tile of kPqTrain16Tile entries of one radix pass;
//   pq_train16_scan_kernel     the histograms turned into write positions, digit-major then tile order (one workgroup);
//   pq_train16_scatter_kernel  the stable scatter of the pass: rank among the equal digits of the wave by ballots, of the waves
//                              before through LDS counts (the (assign, i) sort of db_add, on strided 16-bit keys and with no
//                              row to move, so it is written here);
//   pq_train16_start_kernel    start[k] = the first sorted position whose code is >= k, by binary search (start[65536] = n);
//   pq_train16_walk_kernel     one lane per chain: cluster k's run perm[start[k] .. start[k + 1]) added in list order.
// Two passes (low byte, then high byte) over the identity permutation give the order; only integers are counted, and no float
// meets an atomic or a sum whose order depends on which workgroup finishes first.  Geometry: host/pq_train16_plan.hpp.  Built
// with -ffp-contract=off like every kernel whose sums are pinned.
#include "qadc_pq_train16.h"

namespace qadc {

namespace {
constexpr int kWG = kPqTrain16WG;
constexpr int kTile = kPqTrain16Tile;

// entry `pos` of a pass: the vector it stands for (pass 0 reads the vectors in input order)
__device__ __forceinline__ uint32_t entry_of(const uint32_t* __restrict__ perm, uint32_t pos) { return perm ? perm[pos] : pos; }
// code m of vector i: codes points at column m of [n][stride]
__device__ __forceinline__ uint32_t code_of(const uint16_t* __restrict__ codes, int stride, uint32_t i) {
    return codes[(size_t)i * (size_t)stride];
}
}  // namespace

__global__ __launch_bounds__(kPqTrain16WG) void pq_train16_hist_kernel(const uint16_t* __restrict__ codes, int stride,
                                                                       const uint32_t* __restrict__ perm, uint32_t n, int shift,
                                                                       uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    const uint32_t tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    for (int r = 0; r < kTile / kWG; ++r) {
        const uint64_t pos = (uint64_t)blockIdx.x * kTile + (uint32_t)r * kWG + tid;
        if (pos < n) atomicAdd(&h[(code_of(codes, stride, entry_of(perm, (uint32_t)pos)) >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)blockIdx.x * 256 + tid] = h[tid];
}

// hist [tiles][256] counts -> the first write position of (tile, digit): the entries of smaller digits, then those of the same
// digit in earlier tiles.  Thread d owns digit d.
__global__ __launch_bounds__(kPqTrain16WG) void pq_train16_scan_kernel(uint32_t* __restrict__ hist, uint32_t tiles) {
    __shared__ uint32_t total[256];
    const uint32_t d = threadIdx.x;
    uint32_t sum = 0;
    for (uint32_t t = 0; t < tiles; ++t) {
        const uint32_t c = hist[(size_t)t * 256 + d];
        hist[(size_t)t * 256 + d] = sum;
        sum += c;
    }
    total[d] = sum;
    __syncthreads();
    uint32_t below = 0;
    for (uint32_t j = 0; j < d; ++j) below += total[j];
    if (below)
        for (uint32_t t = 0; t < tiles; ++t) hist[(size_t)t * 256 + d] += below;
}

__global__ __launch_bounds__(kPqTrain16WG) void pq_train16_scatter_kernel(const uint16_t* __restrict__ codes, int stride,
                                                                          const uint32_t* __restrict__ perm, uint32_t n, int shift,
                                                                          const uint32_t* __restrict__ hist,
                                                                          uint32_t* __restrict__ perm_out) {
    __shared__ uint32_t run[256];                                // write position of the next entry of each digit
    __shared__ uint32_t wcount[4 * 256];                         // entries of the digit in each wave of the round
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    run[tid] = hist[(size_t)blockIdx.x * 256 + tid];
    for (int w = 0; w < 4; ++w) wcount[w * 256 + tid] = 0;
    __syncthreads();
    for (int r = 0; r < kTile / kWG; ++r) {
        const uint64_t p0 = (uint64_t)blockIdx.x * kTile + (uint32_t)r * kWG;
        if (p0 >= n) break;                                      // (the same for every thread of the workgroup)
        const bool valid = p0 + tid < n;
        const uint32_t i = valid ? entry_of(perm, (uint32_t)(p0 + tid)) : 0u;
        const uint32_t d = valid ? (code_of(codes, stride, i) >> shift) & 255u : 0u;
        unsigned long long same = __ballot(valid);               // lanes of this wave with the same digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(same & below);
        if (valid && rank == 0) wcount[wave * 256 + d] = (uint32_t)__popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t pos = run[d] + rank;
            for (uint32_t w = 0; w < wave; ++w) pos += wcount[w * 256 + d];
            perm_out[pos] = i;                                   // (pos < n: the positions of a pass are a permutation of [0, n))
        }
        __syncthreads();
        {                                                        // thread d owns digit d: advance its position, clear the counts
            uint32_t c = 0;
            for (int w = 0; w < 4; ++w) {
                c += wcount[w * 256 + tid];
                wcount[w * 256 + tid] = 0;
            }
            run[tid] += c;
        }
        __syncthreads();
    }
}

// start[k], k = 0 .. 65536: the first position j of the sorted order with code(perm[j]) >= k; n where there is none.
__global__ __launch_bounds__(kPqTrain16WG) void pq_train16_start_kernel(const uint16_t* __restrict__ codes, int stride,
                                                                        const uint32_t* __restrict__ perm, uint32_t n,
                                                                        uint32_t* __restrict__ start) {
    const uint32_t k = blockIdx.x * kWG + threadIdx.x;
    if (k > (uint32_t)kPqTrain16K) return;
    uint32_t lo = 0, hi = n;                                     // the answer is in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;                 // (mid < hi <= n)
        if (code_of(codes, stride, perm[mid]) < k) lo = mid + 1;
        else hi = mid;
    }
    start[k] = lo;
}

// x: the learning set [n][dim] advanced to the first column of the sub-quantizer; cb [65536][dsub] and counts [65536] (nullable)
// are the sub-quantizer's.  The lanes of a group read the same perm[j] (a broadcast) and one contiguous 4 * width byte segment
// of the vector; the loads of kPqTrain16Unroll steps are issued before the first add, the adds stay in list order.
__global__ __launch_bounds__(kPqTrain16WG) void pq_train16_walk_kernel(const float* __restrict__ x, int dim,
                                                                       const uint32_t* __restrict__ perm,
                                                                       const uint32_t* __restrict__ start, float* __restrict__ cb,
                                                                       uint32_t* __restrict__ counts, int dsub, int width, int dblocks,
                                                                       int wave_groups, int div_mode) {
    const PqTrain16Owner o = pq_train16_owner(dsub, width, dblocks, wave_groups, blockIdx.x, (int)threadIdx.x);
    uint32_t j = 0, e = 0;
    if (o.owns) {
        j = start[o.k];
        e = start[o.k + 1];                                      // (k + 1 <= 65536: start has 65537 entries)
    }
    const uint32_t count = e - j;
    const float* __restrict__ xp = x + (o.owns ? o.d : 0);
    float acc = 0.0f;
    static_assert(kPqTrain16Unroll == 4, "the steady state below issues four steps' loads");
    while (e - j >= 4u) {                                        // (a lane without a chain has e == j == 0)
        const uint32_t i0 = perm[j], i1 = perm[j + 1], i2 = perm[j + 2], i3 = perm[j + 3];
        const float v0 = xp[(size_t)i0 * (size_t)dim], v1 = xp[(size_t)i1 * (size_t)dim];
        const float v2 = xp[(size_t)i2 * (size_t)dim], v3 = xp[(size_t)i3 * (size_t)dim];
        acc += v0;
        acc += v1;
        acc += v2;
        acc += v3;
        j += 4;
    }
    for (; j < e; ++j) acc += xp[(size_t)perm[j] * (size_t)dim];
    if (o.owns) {
        const float cf = (float)(int)count;
        cb[(size_t)o.k * dsub + o.d] = div_mode ? acc * (1.0f / cf) : acc / cf;
        if (counts && o.d == 0) counts[o.k] = count;
    }
}

hipError_t launch_pq_train16_update(const float* d_x, uint32_t n, int dim, int sq_count, const uint16_t* d_codes, float* d_codebooks,
                                    uint32_t* d_counts, int div_mode, uint32_t* d_perm_a, uint32_t* d_perm_b, uint32_t* d_hist,
                                    uint32_t* d_start, hipStream_t stream) {
    PqTrain16Plan p;
    if (!pq_train16_plan(sq_count, dim, &p) || n == 0 || !d_x || !d_codes || !d_codebooks || !d_perm_a || !d_perm_b || !d_hist || !d_start)
        return hipErrorInvalidValue;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + kTile - 1) / kTile);
    for (int m = 0; m < sq_count; ++m) {
        const uint16_t* codes = d_codes + m;
        const uint32_t* in = nullptr;                            // pass 0 sorts the identity permutation
        uint32_t* out = d_perm_a;
        for (int shift = 0; shift < 16; shift += 8) {
            hipLaunchKernelGGL(pq_train16_hist_kernel, dim3(tiles), dim3(kWG), 0, stream, codes, sq_count, in, n, shift, d_hist);
            hipLaunchKernelGGL(pq_train16_scan_kernel, dim3(1), dim3(kWG), 0, stream, d_hist, tiles);
            hipLaunchKernelGGL(pq_train16_scatter_kernel, dim3(tiles), dim3(kWG), 0, stream, codes, sq_count, in, n, shift, d_hist, out);
            in = out;
            out = d_perm_b;
        }
        hipLaunchKernelGGL(pq_train16_start_kernel, dim3(kPqTrain16K / kWG + 1), dim3(kWG), 0, stream, codes, sq_count, d_perm_b, n, d_start);
        hipLaunchKernelGGL(pq_train16_walk_kernel, dim3(p.walk_grid), dim3(kWG), 0, stream, d_x + (size_t)m * p.dsub, dim, d_perm_b, d_start,
                           d_codebooks + (size_t)m * kPqTrain16K * p.dsub, d_counts ? d_counts + (size_t)m * kPqTrain16K : nullptr, p.dsub,
                           p.width, p.dblocks, p.wave_groups, div_mode);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

}  // namespace qadc
