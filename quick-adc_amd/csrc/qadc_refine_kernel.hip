// Kernels of exact re-ranking (qadc_refine_*), gfx950, built with -ffp-contract=off: every result is held
// bit for bit to host/refine.hpp.
//   refine_dist_kernel<M, Row>  one candidate per wave: the 64-bit word (image of the distance or score << 32 | key) of every candidate
//   refine_select_kernel<M, N, T>  one workgroup per query: bitonic sort of the words in LDS, equal words kept once, the first R out
//   refine_convert_kernel<Row>  the append: float -> the store's element type
//   refine_get_kernel<Row>      the read-back: one key per wave, its row decoded to floats
//   refine_sq_range_kernel      the range of an SQ8 store: per-dimension min and max of the finite components of a learning set
// SQ8 rows: a component is vmin[i] + (float)byte * step[i], the product and the sum rounded one by one;
// the distance kernel stages vmin and step beside the query in LDS, loads a row as one dword per lane and hands the bytes to the
// lanes that own the components 64 j + l with ds_bpermute, so that the definition's summation order holds.
// The keyed store: refine_dist_kernel finds a candidate's row through a lookup policy, DenseLookup (the
// range test) or KeyedLookup (a probe of the table); keyed_*_kernel are the put, the remove and the rebuild.
// The metric is the policy M of csrc/qadc_refine_dev.h, MetricL2 or MetricIP: the term of a component, the
// image of the folded value and, in the select, the image's inverse and the filler of out_dist.
#include "qadc_refine_dev.h"

#include <cfloat>
#include <type_traits>

namespace qadc {
namespace refine {

namespace {

// Lane l of a wave owns the partial sum p[l] of the definition: the components 64 j + l, in ascending j, then the tree at the
// strides 32 .. 1 (lane l < s adds lane l + s; what the lanes at and above s compute is never read by a lane below).  A component
// that does not exist is left out: its lane's p keeps its value.  Under MetricIP a lane's p starts at +0 and IEEE addition gives -0
// only from two -0 operands, so no partial sum and no score is ever -0.
template <typename M, typename Row, typename Lookup>
__global__ __launch_bounds__(kRefineWaves * 64) void refine_dist_kernel(const Row* __restrict__ rows, Lookup look, int dim,
                                                                        const float* __restrict__ sq_vmin, const float* __restrict__ sq_step,
                                                                        const float* __restrict__ queries, int r_in,
                                                                        const uint32_t* __restrict__ keys, const int32_t* __restrict__ counts,
                                                                        const float* __restrict__ values, int cands_per_wg, int chunks,
                                                                        uint64_t* __restrict__ words, unsigned long long* __restrict__ missing) {
    extern __shared__ float s_query[];   // [dim]; SQ8 rows: then vmin [dim] and step [dim]
    __shared__ unsigned s_missing;
    constexpr bool kSq = std::is_same<Row, sq8_t>::value;
    const int q = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* qv = queries + (size_t)q * dim;
    for (int i = tid; i < dim; i += kRefineWaves * 64) {
        s_query[i] = qv[i];
        if (kSq) {
            s_query[dim + i] = sq_vmin[i];
            s_query[2 * dim + i] = sq_step[i];
        }
    }
    if (tid == 0) s_missing = 0;
    __syncthreads();

    const int count = counts ? min(max(counts[q], 0), r_in) : r_in;
    const int c0 = chunk * cands_per_wg, c1 = min(r_in, c0 + cands_per_wg);
    const size_t list = (size_t)q * r_in;
    unsigned lost = 0;
    for (int base = c0 + wave * kRefineInFlight; base < c1; base += kRefineWaves * kRefineInFlight) {
        const Row* x[kRefineInFlight];
        uint32_t key[kRefineInFlight];
        float p[kRefineInFlight];
#pragma unroll
        for (int c = 0; c < kRefineInFlight; ++c) {   // (everything here is uniform over the wave)
            const int i = base + c;
            x[c] = nullptr;
            key[c] = 0;
            p[c] = 0.0f;
            if (i < c1 && i < count && !(values && values[list + i] == FLT_MAX)) {
                key[c] = keys[list + i];
                uint64_t row;
                if (look.row_of(key[c], &row))
                    x[c] = rows + row * (uint64_t)dim;
                else
                    ++lost;
            }
        }
        if constexpr (kSq) {
            for (int b0 = 0; b0 < dim; b0 += 256) {   // 256 components of every row in flight: one dword per lane
                uint32_t w[kRefineInFlight];
#pragma unroll
                for (int c = 0; c < kRefineInFlight; ++c) w[c] = x[c] ? sq_load4(x[c], b0 + 4 * lane, dim) : 0u;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if (b0 + 64 * s >= dim) break;    // (uniform)
                    const int j = b0 + 64 * s + lane;
                    const bool mine = j < dim;
                    const float qj = mine ? s_query[j] : 0.0f, vj = mine ? s_query[dim + j] : 0.0f, sj = mine ? s_query[2 * dim + j] : 0.0f;
#pragma unroll
                    for (int c = 0; c < kRefineInFlight; ++c)
                        if (x[c]) {                   // (uniform: the exchange runs with every lane)
                            const float tt = M::term(qj, sq_lane_value(w[c], s, lane, vj, sj));
                            if (mine) p[c] = p[c] + tt;
                        }
                }
            }
        } else {
            for (int j = lane; j < dim; j += 64) {
                const float qj = s_query[j];
#pragma unroll
                for (int c = 0; c < kRefineInFlight; ++c)
                    if (x[c]) {
                        const float tt = M::term(qj, row_value(x[c], j, 0.0f, 0.0f));
                        p[c] = p[c] + tt;
                    }
            }
        }
#pragma unroll
        for (int c = 0; c < kRefineInFlight; ++c) {
            float v = p[c];
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s, 64);
            const int i = base + c;
            if (lane == 0 && i < c1) words[list + i] = x[c] ? ((uint64_t)M::image(v) << 32) | key[c] : kNoWord;
        }
    }
    if (lane == 0 && lost) atomicAdd(&s_missing, lost);
    __syncthreads();
    if (tid == 0 && s_missing) atomicAdd(missing, (unsigned long long)s_missing);
}

// N words (the list, padded with ~0) sorted ascending by T threads; a word survives where it differs from the one before it and
// is not ~0; the survivors' ranks come from a prefix sum over the threads' segments of N / T consecutive words.
template <typename M, int N, int T>
__global__ __launch_bounds__(T) void refine_select_kernel(const uint64_t* __restrict__ words, int r_in, int R, uint32_t* __restrict__ out_keys,
                                                          float* __restrict__ out_dist, int32_t* __restrict__ out_sizes) {
    extern __shared__ uint64_t s_words[];             // [N], then uint32 [T]
    uint32_t* s_scan = reinterpret_cast<uint32_t*>(s_words + N);
    const int q = blockIdx.x, tid = threadIdx.x;
    const uint64_t* list = words + (size_t)q * r_in;
    for (int i = tid; i < N; i += T) s_words[i] = i < r_in ? list[i] : kNoWord;
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = tid; t < N / 2; t += T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint64_t a = s_words[i], b = s_words[l];
                if ((a > b) == ((i & k) == 0)) {
                    s_words[i] = b;
                    s_words[l] = a;
                }
            }
        }
    __syncthreads();
    constexpr int S = N / T;
    const int first = tid * S;
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const uint64_t w = s_words[first + i];
        mine += (w != kNoWord && (first + i == 0 || w != s_words[first + i - 1])) ? 1u : 0u;
    }
    s_scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < T; d <<= 1) {                 // inclusive scan over the threads' counts
        const uint32_t add = tid >= d ? s_scan[tid - d] : 0u;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    const uint32_t total = s_scan[T - 1];
    uint32_t rank = s_scan[tid] - mine;
    uint32_t* ok = out_keys + (size_t)q * R;
    float* od = out_dist + (size_t)q * R;
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const uint64_t w = s_words[first + i];
        if (w != kNoWord && (first + i == 0 || w != s_words[first + i - 1])) {
            if (rank < (uint32_t)R) {
                ok[rank] = (uint32_t)w;
                od[rank] = M::value((uint32_t)(w >> 32));
            }
            ++rank;
        }
    }
    const uint32_t size = min(total, (uint32_t)R);
    for (uint32_t k = size + tid; k < (uint32_t)R; k += T) {
        ok[k] = 0xFFFFFFFFu;
        od[k] = __uint_as_float(M::kFillerBits);
    }
    if (tid == 0) out_sizes[q] = (int32_t)size;
}

__device__ inline void store_as(float* dst, size_t i, float v) { dst[i] = v; }
__device__ inline void store_as(__half* dst, size_t i, float v) { dst[i] = __float2half_rn(v); }

// How a float becomes an element of a row.  PlainEncode: store_as.  SqEncode: sq_encode of host/refine.hpp under the parameters of
// component `comp`; a component outside the range counts as clamped.
struct PlainEncode {
    static constexpr bool kCounts = false;
    template <typename Row>
    __device__ inline unsigned put(Row* dst, size_t at, uint32_t, float v) const {
        store_as(dst, at, v);
        return 0u;
    }
    __device__ inline unsigned long long* counter() const { return nullptr; }
};

struct SqEncode {
    static constexpr bool kCounts = true;
    const float* __restrict__ vmin;
    const float* __restrict__ step;
    const float* __restrict__ inv;
    unsigned long long* clamped;
    __device__ inline unsigned put(sq8_t* dst, size_t at, uint32_t comp, float x) const {
        const float lo = vmin[comp], st = step[comp];
        const float d = x - lo;
        const float u = d * inv[comp];
        uint8_t c = 0;
        if (u > 0.0f) c = u >= 255.0f ? (uint8_t)255 : (uint8_t)rintf(u);   // (rintf: to nearest, ties to even)
        dst[at].b = c;
        return (st > 0.0f ? (!(d >= 0.0f) || !(u <= 255.0f)) : !(x == lo)) ? 1u : 0u;
    }
    __device__ inline unsigned long long* counter() const { return clamped; }
};

// every thread of the workgroup arrives: the waves' sums of `mine`, then one add to the 64-bit counter
__device__ inline void block_count(unsigned mine, unsigned long long* counter) {
    __shared__ unsigned s_sum;
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) mine += __shfl_down(mine, s, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum) atomicAdd(counter, (unsigned long long)s_sum);
}

// n floats, whole rows of dim: element i is component i % dim of its row
template <typename Row, typename Enc>
__global__ __launch_bounds__(256) void refine_convert_kernel(const float* __restrict__ src, Row* __restrict__ dst, uint64_t n, uint32_t dim, Enc enc) {
    const uint64_t first = (uint64_t)blockIdx.x * 256 + threadIdx.x, stride = (uint64_t)gridDim.x * 256;
    uint32_t comp = Enc::kCounts ? (uint32_t)(first % dim) : 0u;
    const uint32_t hop = Enc::kCounts ? (uint32_t)(stride % dim) : 0u;
    unsigned clamped = 0;
    for (uint64_t i = first; i < n; i += stride) {
        clamped += enc.put(dst, i, comp, src[i]);
        comp += hop;
        if (comp >= dim) comp -= dim;
    }
    if (Enc::kCounts) block_count(clamped, enc.counter());
}

// One key per wave: the row found as refine_dist_kernel finds it, decoded to floats with coalesced stores
template <typename Row, typename Lookup>
__global__ __launch_bounds__(256) void refine_get_kernel(const Row* __restrict__ rows, Lookup look, int dim, const float* __restrict__ sq_vmin,
                                                         const float* __restrict__ sq_step, const uint32_t* __restrict__ keys, uint64_t count,
                                                         float* __restrict__ out, uint8_t* __restrict__ found) {
    constexpr bool kSq = std::is_same<Row, sq8_t>::value;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint64_t k = (uint64_t)blockIdx.x * 4 + wave; k < count; k += (uint64_t)gridDim.x * 4) {
        const uint32_t key = __builtin_amdgcn_readfirstlane(keys[k]);
        uint64_t row = 0;
        const bool held = look.row_of(key, &row);
        const Row* x = rows + row * (uint64_t)dim;
        float* o = out + k * (uint64_t)dim;
        for (int j = lane; j < dim; j += 64)
            o[j] = held ? row_value(x, j, kSq ? sq_vmin[j] : 0.0f, kSq ? sq_step[j] : 0.0f) : __uint_as_float(kNanImage);
        if (found && lane == 0) found[k] = held ? 1 : 0;
    }
}

// A workgroup walks tiles of kSqRangeRows rows with coalesced loads and keeps the columns' extremes in LDS, as ordered images
// (-0 below +0; a non-finite component takes no part); the workgroups' extremes meet in lo and hi by integer atomics.
__global__ __launch_bounds__(256) void refine_sq_range_kernel(const float* __restrict__ vectors, uint64_t n, uint32_t dim, uint32_t* __restrict__ lo,
                                                              uint32_t* __restrict__ hi) {
    extern __shared__ uint32_t s_ext[];   // lo [dim], hi [dim]
    uint32_t *s_lo = s_ext, *s_hi = s_ext + dim;
    for (uint32_t c = threadIdx.x; c < dim; c += 256) {
        s_lo[c] = 0xFFFFFFFFu;
        s_hi[c] = 0u;
    }
    __syncthreads();
    const uint64_t tiles = (n + kSqRangeRows - 1) / kSqRangeRows;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t r0 = tile * kSqRangeRows, r1 = min(n, r0 + (uint64_t)kSqRangeRows);
        const float* v = vectors + r0 * dim;
        const uint32_t cnt = (uint32_t)(r1 - r0) * dim;
        for (uint32_t e = threadIdx.x; e < cnt; e += 256) {
            const uint32_t u = __float_as_uint(v[e]);
            if ((u & 0x7F800000u) == 0x7F800000u) continue;
            const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u), c = e % dim;
            if (o < s_lo[c]) atomicMin(s_lo + c, o);   // (the extremes only move outwards: a stale read costs one atomic at most)
            if (o > s_hi[c]) atomicMax(s_hi + c, o);
        }
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < dim; c += 256)
        if (s_lo[c] <= s_hi[c]) {
            atomicMin(lo + c, s_lo[c]);
            atomicMax(hi + c, s_hi[c]);
        }
}

// ---- the keyed store: put (precheck, claim, count, assign, store), remove, rebuild.  One input, row or slot per thread, strided
// over the grid; every counter is added to once per wave. ----

__device__ inline void keyed_add(unsigned long long* cnt, bool flag) {
    const unsigned long long m = __ballot(flag);
    if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(cnt, (unsigned long long)__popcll(m));
}

// the slot that holds `key`, live or dead, or kKeyedNoRow at the chain's end.  No slot of the table changes its key meanwhile.
__device__ inline uint32_t keyed_find(const uint32_t* __restrict__ tkey, int bits, uint32_t key) {
    const uint32_t mask = (1u << bits) - 1u;
    for (uint32_t s = keyed_slot(key, bits);; s = (s + 1u) & mask) {
        const uint32_t k = tkey[s];
        if (k == key) return s;
        if (k == kKeyedEmpty) return kKeyedNoRow;
    }
}

__global__ __launch_bounds__(kKeyedThreads) void keyed_precheck_kernel(const uint32_t* __restrict__ labels, uint64_t n, const uint32_t* __restrict__ tkey,
                                                                       int bits, unsigned long long* __restrict__ cnt) {
    const uint64_t span = ((n + kKeyedThreads - 1) / kKeyedThreads) * kKeyedThreads;   // (whole waves reach the ballots)
    for (uint64_t i = (uint64_t)blockIdx.x * kKeyedThreads + threadIdx.x; i < span; i += (uint64_t)gridDim.x * kKeyedThreads) {
        const uint32_t key = i < n ? labels[i] : 0u;
        const bool bad = i < n && key == kKeyedEmpty;
        keyed_add(cnt + kKeyedCntBad, bad);
        keyed_add(cnt + kKeyedCntAbsent, i < n && !bad && keyed_find(tkey, bits, key) == kKeyedNoRow);
    }
}

__global__ __launch_bounds__(kKeyedThreads) void keyed_claim_kernel(const uint32_t* __restrict__ labels, uint32_t n, uint32_t* tkey, uint32_t* win, int bits,
                                                                    uint32_t* __restrict__ slot_of, unsigned long long* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * kKeyedThreads + threadIdx.x;
    bool claimed = false;
    if (i < n) {
        const uint32_t key = labels[i], mask = (1u << bits) - 1u;
        uint32_t s = keyed_slot(key, bits);
        for (;; s = (s + 1u) & mask) {                // (slots only go from empty to a key here, so a stale read costs one CAS at most)
            uint32_t k = *reinterpret_cast<volatile const uint32_t*>(tkey + s);
            if (k == kKeyedEmpty) {
                k = atomicCAS(tkey + s, kKeyedEmpty, key);
                claimed = k == kKeyedEmpty;
                if (claimed) break;
            }
            if (k == key) break;
        }
        slot_of[i] = s;
        atomicMax(win + s, i + 1u);
    }
    keyed_add(cnt + kKeyedCntClaimed, claimed);
}

__global__ __launch_bounds__(kKeyedThreads) void keyed_count_kernel(uint32_t n, const uint32_t* __restrict__ trow, const uint32_t* __restrict__ win,
                                                                    const uint32_t* __restrict__ slot_of, uint32_t* __restrict__ dst,
                                                                    unsigned long long* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * kKeyedThreads + threadIdx.x;
    bool need = false;
    if (i < n) {
        const uint32_t s = slot_of[i];
        uint32_t d = kKeyedLoser;
        if (win[s] == i + 1u) {
            d = trow[s];
            need = d == kKeyedNoRow;
            if (need) d = kKeyedNeedsRow;
        }
        dst[i] = d;
    }
    keyed_add(cnt + kKeyedCntNeed, need);
}

__global__ __launch_bounds__(kKeyedThreads) void keyed_assign_kernel(const uint32_t* __restrict__ labels, uint32_t n, uint32_t* __restrict__ trow,
                                                                     uint32_t* __restrict__ win, const uint32_t* __restrict__ slot_of,
                                                                     uint32_t* __restrict__ dst, uint32_t* __restrict__ row_key,
                                                                     const uint32_t* __restrict__ free_list, uint32_t free_rows, uint32_t alloc_rows,
                                                                     unsigned long long* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * kKeyedThreads + threadIdx.x;
    if (i >= n || dst[i] == kKeyedLoser) return;      // (one winner per slot: nobody else touches what is written below)
    const uint32_t s = slot_of[i];
    if (dst[i] == kKeyedNeedsRow) {
        const uint32_t t = (uint32_t)atomicAdd(cnt + kKeyedCntTaken, 1ull);
        const uint32_t r = t < free_rows ? free_list[free_rows - 1u - t] : alloc_rows + (t - free_rows);
        row_key[r] = labels[i];
        trow[s] = r;
        dst[i] = r;
    }
    win[s] = 0u;
}

__global__ __launch_bounds__(kKeyedThreads) void keyed_reset_kernel(uint32_t n, uint32_t* __restrict__ win, const uint32_t* __restrict__ slot_of) {
    const uint32_t i = blockIdx.x * kKeyedThreads + threadIdx.x;
    if (i < n) win[slot_of[i]] = 0u;
}

// refine_convert_kernel's work with a destination row per input: consecutive threads take consecutive components.  An input that
// lost its key to a later one writes nothing and counts nothing.
template <typename Row, typename Enc>
__global__ __launch_bounds__(kKeyedThreads) void keyed_store_kernel(const float* __restrict__ src, const uint32_t* __restrict__ dst, uint64_t total,
                                                                    uint32_t dim, Row* __restrict__ rows, Enc enc) {
    unsigned clamped = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * kKeyedThreads + threadIdx.x; e < total; e += (uint64_t)gridDim.x * kKeyedThreads) {
        const uint64_t i = e / dim;
        const uint32_t r = dst[i], comp = (uint32_t)(e - i * dim);
        if (r != kKeyedLoser) clamped += enc.put(rows + (uint64_t)r * dim, (size_t)comp, comp, src[e]);
    }
    if (Enc::kCounts) block_count(clamped, enc.counter());
}

__global__ __launch_bounds__(kKeyedThreads) void keyed_remove_kernel(const uint32_t* __restrict__ labels, uint32_t n, const uint32_t* __restrict__ tkey,
                                                                     uint32_t* trow, int bits, uint32_t* __restrict__ row_key,
                                                                     uint32_t* __restrict__ free_list, uint32_t free_rows,
                                                                     unsigned long long* __restrict__ cnt) {
    const uint32_t i = blockIdx.x * kKeyedThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = labels[i];
    if (key == kKeyedEmpty) return;
    const uint32_t s = keyed_find(tkey, bits, key);
    if (s == kKeyedNoRow) return;
    const uint32_t r = atomicExch(trow + s, kKeyedNoRow);    // whoever gets the row back frees it: a key listed twice counts once
    if (r == kKeyedNoRow) return;
    row_key[r] = kKeyedEmpty;
    free_list[free_rows + (uint32_t)atomicAdd(cnt + kKeyedCntRemoved, 1ull)] = r;
}

__global__ __launch_bounds__(kKeyedThreads) void keyed_rebuild_kernel(const uint32_t* __restrict__ row_key, uint32_t alloc_rows, uint32_t* tkey,
                                                                      uint32_t* __restrict__ trow, int bits) {
    const uint32_t mask = (1u << bits) - 1u;
    for (uint64_t r = (uint64_t)blockIdx.x * kKeyedThreads + threadIdx.x; r < alloc_rows; r += (uint64_t)gridDim.x * kKeyedThreads) {
        const uint32_t key = row_key[r];
        if (key == kKeyedEmpty) continue;
        uint32_t s = keyed_slot(key, bits);
        while (atomicCAS(tkey + s, kKeyedEmpty, key) != kKeyedEmpty) s = (s + 1u) & mask;   // (the live keys differ: no slot matches)
        trow[s] = (uint32_t)r;
    }
}

template <typename M, int N, int T>
hipError_t launch_select(const RefinePass& p, const RefinePlan& plan, hipStream_t stream) {
    if (plan.select_lds_bytes > kRefineLdsDefault) {   // the largest instantiation: above the default limit of dynamic LDS
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&refine_select_kernel<M, N, T>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.select_lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((refine_select_kernel<M, N, T>), dim3((unsigned)p.nq), dim3(T), plan.select_lds_bytes, stream, p.words, p.r_in, p.R,
                       p.out_keys, p.out_dist, p.out_sizes);
    return hipGetLastError();
}

template <typename M>
hipError_t launch_dist(const RefinePass& p, const RefinePlan& plan, hipStream_t stream) {
    const dim3 grid((unsigned)((uint64_t)p.nq * plan.chunks)), block(kRefineWaves * 64);
    const DenseLookup dense{p.lo, p.nrows};
    const KeyedLookup keyed{p.tkey, p.trow, p.tbits};
#define QADC_RD(ROW, LOOKUP, look)                                                                                                       \
    hipLaunchKernelGGL((refine_dist_kernel<M, ROW, LOOKUP>), grid, block, lds, stream, static_cast<const ROW*>(p.rows), look, p.dim, p.sq.vmin, \
                       p.sq.step, p.queries, p.r_in, p.keys, p.counts, p.values, plan.cands_per_wg, plan.chunks, p.words, p.missing)
    // (SQ8 rows: vmin and step behind the query, 3 * dim floats <= 48 KiB)
    const size_t lds = p.elem == Elem::kSQ8 ? 3 * plan.dist_lds_bytes : plan.dist_lds_bytes;
    if (p.tkey) {
        if (p.elem == Elem::kSQ8) QADC_RD(sq8_t, KeyedLookup, keyed);
        else if (p.elem == Elem::kF16) QADC_RD(__half, KeyedLookup, keyed);
        else QADC_RD(float, KeyedLookup, keyed);
    } else {
        if (p.elem == Elem::kSQ8) QADC_RD(sq8_t, DenseLookup, dense);
        else if (p.elem == Elem::kF16) QADC_RD(__half, DenseLookup, dense);
        else QADC_RD(float, DenseLookup, dense);
    }
#undef QADC_RD
    return hipGetLastError();
}

template <typename M>
hipError_t dispatch_select(const RefinePass& p, const RefinePlan& plan, hipStream_t stream) {
    switch (plan.sort_n) {
        case 512: return launch_select<M, 512, 256>(p, plan, stream);
        case 2048: return launch_select<M, 2048, 1024>(p, plan, stream);
        case 8192: return launch_select<M, 8192, 1024>(p, plan, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_refine_dist(const RefinePass& p, const RefinePlan& plan, hipStream_t stream) {
    return p.metric == kMetricIP ? launch_dist<MetricIP>(p, plan, stream) : launch_dist<MetricL2>(p, plan, stream);
}

hipError_t launch_refine_get(const RefinePass& p, const uint32_t* keys, uint64_t count, float* out, uint8_t* found, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<uint64_t>((count + 3) / 4, 65536)), block(256);
    const DenseLookup dense{p.lo, p.nrows};
    const KeyedLookup keyed{p.tkey, p.trow, p.tbits};
#define QADC_RG(ROW, LOOKUP, look)                                                                                                         \
    hipLaunchKernelGGL((refine_get_kernel<ROW, LOOKUP>), grid, block, 0, stream, static_cast<const ROW*>(p.rows), look, p.dim, p.sq.vmin, \
                       p.sq.step, keys, count, out, found)
    if (p.tkey) {
        if (p.elem == Elem::kSQ8) QADC_RG(sq8_t, KeyedLookup, keyed);
        else if (p.elem == Elem::kF16) QADC_RG(__half, KeyedLookup, keyed);
        else QADC_RG(float, KeyedLookup, keyed);
    } else {
        if (p.elem == Elem::kSQ8) QADC_RG(sq8_t, DenseLookup, dense);
        else if (p.elem == Elem::kF16) QADC_RG(__half, DenseLookup, dense);
        else QADC_RG(float, DenseLookup, dense);
    }
#undef QADC_RG
    return hipGetLastError();
}

hipError_t launch_refine_sq_range(const float* vectors, uint64_t n, int dim, uint32_t* lo, uint32_t* hi, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t tiles = (n + kSqRangeRows - 1) / kSqRangeRows;
    hipLaunchKernelGGL(refine_sq_range_kernel, dim3((unsigned)std::min<uint64_t>(tiles, 2048)), dim3(256), 2 * (size_t)dim * sizeof(uint32_t), stream,
                       vectors, n, (uint32_t)dim, lo, hi);
    return hipGetLastError();
}

hipError_t launch_refine_select(const RefinePass& p, const RefinePlan& plan, hipStream_t stream) {
    return p.metric == kMetricIP ? dispatch_select<MetricIP>(p, plan, stream) : dispatch_select<MetricL2>(p, plan, stream);
}

hipError_t launch_refine_convert(const float* src, void* dst, Elem elem, const SqParams& sq, int dim, uint64_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<uint64_t>((n + 255) / 256, 65536)), block(256);
    if (elem == Elem::kSQ8)
        hipLaunchKernelGGL((refine_convert_kernel<sq8_t, SqEncode>), grid, block, 0, stream, src, static_cast<sq8_t*>(dst), n, (uint32_t)dim,
                           SqEncode{sq.vmin, sq.step, sq.inv, sq.clamped});
    else if (elem == Elem::kF16)
        hipLaunchKernelGGL((refine_convert_kernel<__half, PlainEncode>), grid, block, 0, stream, src, static_cast<__half*>(dst), n, (uint32_t)dim,
                           PlainEncode{});
    else
        hipLaunchKernelGGL((refine_convert_kernel<float, PlainEncode>), grid, block, 0, stream, src, static_cast<float*>(dst), n, (uint32_t)dim,
                           PlainEncode{});
    return hipGetLastError();
}

hipError_t launch_keyed_precheck(const uint32_t* labels, uint64_t n, KeyedTable t, unsigned long long* cnt, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(keyed_precheck_kernel, dim3(keyed_grid(n)), dim3(kKeyedThreads), 0, stream, labels, n, t.key, t.bits, cnt);
    return hipGetLastError();
}

hipError_t launch_keyed_claim(const uint32_t* labels, uint32_t n, KeyedTable t, uint32_t* slot_of, unsigned long long* cnt, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > kKeyedPass) return hipErrorInvalidValue;   // (one input per thread, no stride)
    hipLaunchKernelGGL(keyed_claim_kernel, dim3(keyed_grid(n)), dim3(kKeyedThreads), 0, stream, labels, n, t.key, t.win, t.bits, slot_of, cnt);
    return hipGetLastError();
}

hipError_t launch_keyed_count(uint32_t n, KeyedTable t, const uint32_t* slot_of, uint32_t* dst, unsigned long long* cnt, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > kKeyedPass) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyed_count_kernel, dim3(keyed_grid(n)), dim3(kKeyedThreads), 0, stream, n, t.row, t.win, slot_of, dst, cnt);
    return hipGetLastError();
}

hipError_t launch_keyed_assign(const uint32_t* labels, uint32_t n, KeyedTable t, const uint32_t* slot_of, uint32_t* dst, uint32_t* row_key,
                               const uint32_t* free_list, uint32_t free_rows, uint32_t alloc_rows, unsigned long long* cnt, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > kKeyedPass) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyed_assign_kernel, dim3(keyed_grid(n)), dim3(kKeyedThreads), 0, stream, labels, n, t.row, t.win, slot_of, dst, row_key,
                       free_list, free_rows, alloc_rows, cnt);
    return hipGetLastError();
}

hipError_t launch_keyed_reset(uint32_t n, KeyedTable t, const uint32_t* slot_of, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > kKeyedPass) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyed_reset_kernel, dim3(keyed_grid(n)), dim3(kKeyedThreads), 0, stream, n, t.win, slot_of);
    return hipGetLastError();
}

hipError_t launch_keyed_store(const float* src, const uint32_t* dst, uint32_t n, int dim, void* rows, Elem elem, const SqParams& sq,
                              hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t total = (uint64_t)n * (uint64_t)dim;
    if (elem == Elem::kSQ8)
        hipLaunchKernelGGL((keyed_store_kernel<sq8_t, SqEncode>), dim3(keyed_grid(total)), dim3(kKeyedThreads), 0, stream, src, dst, total,
                           (uint32_t)dim, static_cast<sq8_t*>(rows), SqEncode{sq.vmin, sq.step, sq.inv, sq.clamped});
    else if (elem == Elem::kF16)
        hipLaunchKernelGGL((keyed_store_kernel<__half, PlainEncode>), dim3(keyed_grid(total)), dim3(kKeyedThreads), 0, stream, src, dst, total,
                           (uint32_t)dim, static_cast<__half*>(rows), PlainEncode{});
    else
        hipLaunchKernelGGL((keyed_store_kernel<float, PlainEncode>), dim3(keyed_grid(total)), dim3(kKeyedThreads), 0, stream, src, dst, total,
                           (uint32_t)dim, static_cast<float*>(rows), PlainEncode{});
    return hipGetLastError();
}

hipError_t launch_keyed_remove(const uint32_t* labels, uint32_t n, KeyedTable t, uint32_t* row_key, uint32_t* free_list, uint32_t free_rows,
                               unsigned long long* cnt, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n > kKeyedPass) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyed_remove_kernel, dim3(keyed_grid(n)), dim3(kKeyedThreads), 0, stream, labels, n, t.key, t.row, t.bits, row_key, free_list,
                       free_rows, cnt);
    return hipGetLastError();
}

hipError_t launch_keyed_rebuild(const uint32_t* row_key, uint32_t alloc_rows, KeyedTable t, hipStream_t stream) {
    if (alloc_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(keyed_rebuild_kernel, dim3(keyed_grid(alloc_rows)), dim3(kKeyedThreads), 0, stream, row_key, alloc_rows, t.key, t.row, t.bits);
    return hipGetLastError();
}

}  // namespace refine
}  // namespace qadc
