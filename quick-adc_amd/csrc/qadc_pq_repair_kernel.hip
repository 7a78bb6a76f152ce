// Empty-cluster repair of PQ training in every sub-space at once (include/qadc.h "Empty-cluster repair").
//
//   repair_count_kernel    count[m][k] and first[m][k] by integer atomics (add and min: the result does not depend on the order);
//                          a workgroup reads a tile of code units of all sub-spaces, coalesced, and keeps the tables in LDS where
//                          they fit;
//   repair_empties_kernel  the empties of a sub-space in ascending k, by an ordered compaction (ballot ranks, wave counts); E[m];
//   repair_keys_kernel     one vector per lane: the distance chain to the assigned centroid, the key (0 where not eligible);
//   repair_hist_kernel /   the E-th largest key by radix select: eight 8-bit digits, most significant first; per digit a histogram
//   repair_pick_kernel     of the keys under the prefix found so far, then the digit that holds the wanted rank;
//   repair_mark_kernel /   the ordered compaction of the chosen vectors in ascending index: chosen per workgroup, an exclusive scan
//   repair_scan_kernel /   over the workgroups, then the rank j by ballots in the wave, wave counts and the workgroup's offset; the
//   repair_rank_kernel     vector's key word is overwritten by its new code (bit 63 set) or 0;
//   repair_apply_kernel    the rewrite, one thread per code unit: at 4 bits the thread owns the byte and reads the decisions of both
//                          sub-spaces that share it, so one byte is never two read-modify-writes.
// Only integers are counted; the one float chain is per vector.  E[m] lives in device memory: every kernel after the list returns
// at once for a sub-space without an empty cluster.  Geometry: host/pq_repair_plan.hpp.  Built with -ffp-contract=off; the fused
// operation is explicit.
#include "qadc_pq_repair.h"

namespace qadc {

namespace {
constexpr int kWG = kPqRepairWG;
constexpr int kRowsPerThread = kPqRepairRowTile / kPqRepairWG;
constexpr int kUnitsPerThread = kPqRepairUnitTile / kPqRepairWG;
constexpr unsigned long long kChosenBit = 1ull << 63;

__device__ __forceinline__ uint32_t repair_code(const void* __restrict__ codes, int bits, int S, uint64_t i, int m) {
    if (bits == 4) return (static_cast<const uint8_t*>(codes)[i * (uint64_t)(S / 2) + (uint64_t)(m / 2)] >> (4 * (m & 1))) & 15u;
    if (bits == 8) return static_cast<const uint8_t*>(codes)[i * (uint64_t)S + (uint64_t)m];
    return static_cast<const uint16_t*>(codes)[i * (uint64_t)S + (uint64_t)m];
}

// the exclusive prefix of `flag` over the workgroup in thread order, and the workgroup's total; wc: 4 words of LDS.  Two barriers.
__device__ __forceinline__ uint32_t repair_block_rank(bool flag, uint32_t* wc, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) wc[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t off = (uint32_t)__popcll(bal & ((1ull << lane) - 1)), all = 0;
    for (uint32_t w = 0; w < kWG / 64; ++w) {
        if (w < wave) off += wc[w];
        all += wc[w];
    }
    __syncthreads();
    *total = all;
    return off;
}
}  // namespace

__global__ __launch_bounds__(kPqRepairWG) void repair_count_kernel(const void* __restrict__ codes, int bits, int S, uint32_t K,
                                                                   uint32_t units_per_row, uint64_t units, int in_lds,
                                                                   uint32_t* __restrict__ count, uint32_t* __restrict__ first) {
    extern __shared__ uint32_t repair_lds[];                     // in_lds: [S * K] counts, then [S * K] firsts
    const uint32_t tid = threadIdx.x, SK = (uint32_t)S * K;
    uint32_t* const cnt = in_lds ? repair_lds : count;
    uint32_t* const fst = in_lds ? repair_lds + SK : first;
    if (in_lds) {
        for (uint32_t t = tid; t < SK; t += kWG) {
            cnt[t] = 0u;
            fst[t] = 0xFFFFFFFFu;
        }
        __syncthreads();
    }
    for (int r = 0; r < kUnitsPerThread; ++r) {
        const uint64_t e = (uint64_t)blockIdx.x * kPqRepairUnitTile + (uint64_t)(r * kWG) + tid;
        if (e >= units) break;
        const uint32_t i = (uint32_t)(e / units_per_row), u = (uint32_t)(e % units_per_row);
        if (bits == 4) {
            const uint32_t b = static_cast<const uint8_t*>(codes)[e];
            const uint32_t lo = (2u * u) * K + (b & 15u), hi = (2u * u + 1u) * K + (b >> 4);
            atomicAdd(&cnt[lo], 1u);
            atomicMin(&fst[lo], i);
            atomicAdd(&cnt[hi], 1u);
            atomicMin(&fst[hi], i);
        } else {
            const uint32_t k = bits == 8 ? (uint32_t) static_cast<const uint8_t*>(codes)[e] : (uint32_t) static_cast<const uint16_t*>(codes)[e];
            atomicAdd(&cnt[u * K + k], 1u);
            atomicMin(&fst[u * K + k], i);
        }
    }
    if (in_lds) {
        __syncthreads();
        for (uint32_t t = tid; t < SK; t += kWG) {
            const uint32_t c = cnt[t];
            if (c) {
                atomicAdd(&count[t], c);
                atomicMin(&first[t], fst[t]);
            }
        }
    }
}

// grid: sq_count
__global__ __launch_bounds__(kPqRepairWG) void repair_empties_kernel(const uint32_t* __restrict__ count, uint32_t K,
                                                                     uint32_t* __restrict__ empties, PqRepairCtl* __restrict__ ctl) {
    __shared__ uint32_t wc[kWG / 64];
    const uint32_t m = blockIdx.x, tid = threadIdx.x;
    uint32_t running = 0;
    for (uint32_t base = 0; base < K; base += kWG) {             // (the same trips in every thread: the barriers are uniform)
        const uint32_t k = base + tid;
        const bool empty = k < K && count[(uint64_t)m * K + k] == 0u;
        uint32_t total;
        const uint32_t off = repair_block_rank(empty, wc, &total);
        if (empty) empties[(uint64_t)m * K + running + off] = k;  // (running + off < K: at most K empties)
        running += total;
    }
    if (tid == 0) ctl[m].E = running;
}

// grid: (row_blocks, sq_count)
__global__ __launch_bounds__(kPqRepairWG) void repair_keys_kernel(const float* __restrict__ x, const float* __restrict__ cb,
                                                                  const void* __restrict__ codes, int bits, int S, uint32_t K, int dim,
                                                                  int dsub, uint64_t n, const uint32_t* __restrict__ first,
                                                                  PqRepairCtl* __restrict__ ctl, unsigned long long* __restrict__ keys) {
    __shared__ uint32_t s_eligible;
    const uint32_t m = blockIdx.y, tid = threadIdx.x;
    if (ctl[m].E == 0u) return;                                  // (uniform in the workgroup)
    if (tid == 0) s_eligible = 0u;
    __syncthreads();
    uint32_t eligible = 0;
    for (int r = 0; r < kRowsPerThread; ++r) {
        const uint64_t i = (uint64_t)blockIdx.x * kPqRepairRowTile + (uint64_t)(r * kWG) + tid;
        if (i >= n) break;
        const uint32_t c = repair_code(codes, bits, S, i, (int)m);
        const float* xr = x + i * (uint64_t)dim + (uint64_t)m * (uint64_t)dsub;
        const float* cr = cb + ((uint64_t)m * K + c) * (uint64_t)dsub;
        float acc = 0.0f;
        for (int d = 0; d < dsub; ++d) {                         // ascending column: the pinned order
            const float t = xr[d] - cr[d];
            acc = __fmaf_rn(t, t, acc);
        }
        unsigned long long key = 0ull;
        if (acc > 0.0f && acc < __builtin_inff() && first[(uint64_t)m * K + c] != (uint32_t)i)
            key = ((unsigned long long)__float_as_uint(acc) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
        keys[(uint64_t)m * n + i] = key;
        eligible += key != 0ull;
    }
    if (eligible) atomicAdd(&s_eligible, eligible);
    __syncthreads();
    if (tid == 0 && s_eligible) atomicAdd(&ctl[m].eligible, s_eligible);
}

// grid: (row_blocks, sq_count).  The digit at `shift` of the keys whose higher digits equal the prefix.
__global__ __launch_bounds__(kPqRepairWG) void repair_hist_kernel(const unsigned long long* __restrict__ keys, uint64_t n, int shift,
                                                                  const PqRepairCtl* __restrict__ ctl, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    const uint32_t m = blockIdx.y, tid = threadIdx.x;
    if (ctl[m].E == 0u) return;
    const bool top = shift == 8 * (kPqRepairDigits - 1);
    if (!top && ctl[m].want == 0u) return;                       // nothing is chosen in this sub-space
    const unsigned long long prefix = top ? 0ull : ctl[m].prefix >> (shift + 8);
    h[tid] = 0u;
    __syncthreads();
    for (int r = 0; r < kRowsPerThread; ++r) {
        const uint64_t i = (uint64_t)blockIdx.x * kPqRepairRowTile + (uint64_t)(r * kWG) + tid;
        if (i >= n) break;
        const unsigned long long key = keys[(uint64_t)m * n + i];
        if (top || (key >> (shift + 8)) == prefix) atomicAdd(&h[(uint32_t)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&hist[m * 256u + tid], h[tid]);
}

// grid: sq_count.  The digit that holds the wanted rank, counted from the largest; the histogram is cleared for the next pass.
__global__ __launch_bounds__(kPqRepairWG) void repair_pick_kernel(int shift, PqRepairCtl* __restrict__ ctl, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    const uint32_t m = blockIdx.x, tid = threadIdx.x;
    if (ctl[m].E == 0u) return;
    h[tid] = hist[m * 256u + tid];
    hist[m * 256u + tid] = 0u;
    __syncthreads();
    if (tid != 0) return;
    uint32_t want = ctl[m].want;
    if (shift == 8 * (kPqRepairDigits - 1)) {
        want = min(ctl[m].E, ctl[m].eligible);
        ctl[m].prefix = 0ull;
        ctl[m].threshold = ~0ull;
        ctl[m].want = want;
    }
    if (want == 0u) return;
    uint32_t above = 0;
    int digit = 0;
    for (int d = 255; d >= 0; --d) {
        if (above + h[d] >= want) {
            digit = d;
            break;
        }
        above += h[d];
    }
    const unsigned long long prefix = ctl[m].prefix | ((unsigned long long)digit << shift);
    ctl[m].prefix = prefix;
    ctl[m].want = want - above;
    if (shift == 0) ctl[m].threshold = prefix;
}

// grid: (row_blocks, sq_count)
__global__ __launch_bounds__(kPqRepairWG) void repair_mark_kernel(const unsigned long long* __restrict__ keys, uint64_t n,
                                                                  const PqRepairCtl* __restrict__ ctl, uint32_t* __restrict__ blockcnt) {
    __shared__ uint32_t s_chosen;
    const uint32_t m = blockIdx.y, tid = threadIdx.x;
    if (ctl[m].E == 0u) return;
    const unsigned long long threshold = ctl[m].threshold;
    if (tid == 0) s_chosen = 0u;
    __syncthreads();
    uint32_t chosen = 0;
    for (int r = 0; r < kRowsPerThread; ++r) {
        const uint64_t i = (uint64_t)blockIdx.x * kPqRepairRowTile + (uint64_t)(r * kWG) + tid;
        if (i >= n) break;
        const unsigned long long key = keys[(uint64_t)m * n + i];
        chosen += key != 0ull && key >= threshold;
    }
    if (chosen) atomicAdd(&s_chosen, chosen);
    __syncthreads();
    if (tid == 0) blockcnt[(uint64_t)m * gridDim.x + blockIdx.x] = s_chosen;
}

// grid: sq_count.  blockcnt[m][] becomes its exclusive prefix; moved.
__global__ __launch_bounds__(kPqRepairWG) void repair_scan_kernel(uint32_t* __restrict__ blockcnt, uint32_t row_blocks,
                                                                  PqRepairCtl* __restrict__ ctl, uint32_t* __restrict__ any_moved,
                                                                  unsigned long long* __restrict__ moved_total) {
    __shared__ uint32_t ws[kWG / 64];
    const uint32_t m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (ctl[m].E == 0u) return;
    uint32_t* const bc = blockcnt + (uint64_t)m * row_blocks;
    uint32_t running = 0;
    for (uint32_t base = 0; base < row_blocks; base += kWG) {    // (the same trips in every thread: the barriers are uniform)
        const uint32_t b = base + tid;
        const uint32_t v = b < row_blocks ? bc[b] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o);
            if ((int)lane >= o) inc += t;
        }
        if (lane == 63) ws[wave] = inc;
        __syncthreads();
        uint32_t off = 0, all = 0;
        for (uint32_t w = 0; w < kWG / 64; ++w) {
            if (w < wave) off += ws[w];
            all += ws[w];
        }
        __syncthreads();
        if (b < row_blocks) bc[b] = running + off + inc - v;
        running += all;
    }
    if (tid == 0) {
        ctl[m].moved = running;
        if (running) {
            *any_moved = 1u;                                     // (every writer writes the same word)
            moved_total[m] += (unsigned long long)running;
        }
    }
}

// grid: (row_blocks, sq_count).  keys[m][i] becomes kChosenBit | new code for a chosen vector, 0 for every other.
__global__ __launch_bounds__(kPqRepairWG) void repair_rank_kernel(unsigned long long* __restrict__ keys, uint64_t n, uint32_t K,
                                                                  const PqRepairCtl* __restrict__ ctl, const uint32_t* __restrict__ blockcnt,
                                                                  const uint32_t* __restrict__ empties) {
    __shared__ uint32_t wc[kWG / 64];
    const uint32_t m = blockIdx.y, tid = threadIdx.x;
    if (ctl[m].E == 0u || ctl[m].moved == 0u) return;
    const unsigned long long threshold = ctl[m].threshold;
    uint32_t base = blockcnt[(uint64_t)m * gridDim.x + blockIdx.x];
    for (int r = 0; r < kRowsPerThread; ++r) {                   // (every thread takes every trip: the barriers are uniform)
        const uint64_t i = (uint64_t)blockIdx.x * kPqRepairRowTile + (uint64_t)(r * kWG) + tid;
        const unsigned long long key = i < n ? keys[(uint64_t)m * n + i] : 0ull;
        const bool chosen = key != 0ull && key >= threshold;
        uint32_t total;
        const uint32_t j = base + repair_block_rank(chosen, wc, &total);
        if (i < n) keys[(uint64_t)m * n + i] = chosen ? kChosenBit | (unsigned long long)empties[(uint64_t)m * K + j] : 0ull;   // j < moved <= E
        base += total;
    }
}

// grid: unit_blocks.  One thread per code unit.
__global__ __launch_bounds__(kPqRepairWG) void repair_apply_kernel(void* __restrict__ codes, int bits, uint32_t units_per_row, uint64_t units,
                                                                   uint64_t n, const PqRepairCtl* __restrict__ ctl,
                                                                   const uint32_t* __restrict__ any_moved,
                                                                   const unsigned long long* __restrict__ keys) {
    if (*any_moved == 0u) return;
    for (int r = 0; r < kUnitsPerThread; ++r) {
        const uint64_t e = (uint64_t)blockIdx.x * kPqRepairUnitTile + (uint64_t)(r * kWG) + threadIdx.x;
        if (e >= units) break;
        const uint64_t i = e / units_per_row;
        const uint32_t u = (uint32_t)(e % units_per_row);
        if (bits == 4) {                                         // the byte of sub-quantizers 2u (low nibble) and 2u + 1: owned here
            const bool lo = ctl[2u * u].moved != 0u, hi = ctl[2u * u + 1u].moved != 0u;
            if (!lo && !hi) continue;
            const unsigned long long klo = lo ? keys[(uint64_t)(2u * u) * n + i] : 0ull, khi = hi ? keys[(uint64_t)(2u * u + 1u) * n + i] : 0ull;
            if (!((klo | khi) & kChosenBit)) continue;
            uint8_t* p = static_cast<uint8_t*>(codes) + e;
            uint32_t b = *p;
            if (klo & kChosenBit) b = (b & 0xF0u) | ((uint32_t)klo & 15u);
            if (khi & kChosenBit) b = (b & 0x0Fu) | (((uint32_t)khi & 15u) << 4);
            *p = (uint8_t)b;
        } else {
            if (ctl[u].moved == 0u) continue;
            const unsigned long long k = keys[(uint64_t)u * n + i];
            if (!(k & kChosenBit)) continue;
            if (bits == 8) static_cast<uint8_t*>(codes)[e] = (uint8_t)k;
            else static_cast<uint16_t*>(codes)[e] = (uint16_t)k;
        }
    }
}

hipError_t launch_pq_repair(const PqRepairState& st, const PqRepairPlan& p, hipStream_t stream) {
    if (!st.x || !st.cb || !st.codes || !st.zeroed || !st.first || !st.empties || !st.blockcnt || !st.keys || !st.moved_total)
        return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(st.zeroed, 0, st.zeroed_bytes, stream)) return e;
    if (hipError_t e = hipMemsetAsync(st.first, 0xFF, p.first_bytes, stream)) return e;
    const dim3 wg(kPqRepairWG), rows(p.row_blocks, (uint32_t)p.sq_count), subs((uint32_t)p.sq_count);
    hipLaunchKernelGGL(repair_count_kernel, dim3(p.unit_blocks), wg, p.count_lds_bytes, stream, st.codes, p.sq_bits, p.sq_count, p.K,
                       p.units_per_row, p.units, p.count_in_lds, st.count, st.first);
    hipLaunchKernelGGL(repair_empties_kernel, subs, wg, 0, stream, st.count, p.K, st.empties, st.ctl);
    hipLaunchKernelGGL(repair_keys_kernel, rows, wg, 0, stream, st.x, st.cb, st.codes, p.sq_bits, p.sq_count, p.K, p.dim, p.dsub, p.n, st.first,
                       st.ctl, st.keys);
    for (int digit = kPqRepairDigits - 1; digit >= 0; --digit) {
        hipLaunchKernelGGL(repair_hist_kernel, rows, wg, 0, stream, st.keys, p.n, 8 * digit, st.ctl, st.hist);
        hipLaunchKernelGGL(repair_pick_kernel, subs, wg, 0, stream, 8 * digit, st.ctl, st.hist);
    }
    hipLaunchKernelGGL(repair_mark_kernel, rows, wg, 0, stream, st.keys, p.n, st.ctl, st.blockcnt);
    hipLaunchKernelGGL(repair_scan_kernel, subs, wg, 0, stream, st.blockcnt, p.row_blocks, st.ctl, st.any_moved, st.moved_total);
    hipLaunchKernelGGL(repair_rank_kernel, rows, wg, 0, stream, st.keys, p.n, p.K, st.ctl, st.blockcnt, st.empties);
    hipLaunchKernelGGL(repair_apply_kernel, dim3(p.unit_blocks), wg, 0, stream, st.codes, p.sq_bits, p.units_per_row, p.units, p.n, st.ctl,
                       st.any_moved, st.keys);
    return hipGetLastError();
}

}  // namespace qadc
