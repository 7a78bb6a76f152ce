// Kernels of the exact range search over a refine store (qadc_refine_range, qadc_refine_rerank_range),
// gfx950, built with -ffp-contract=off: every result is held bit for bit to refine::range and refine::rerank_range of
// host/refine.hpp.  The geometry is host/refine_range_plan.hpp.
//   refine_range_dist_kernel<Row, QT, J>   refine_knn_dist_kernel's tile and fold; the words below the query's limit are appended to
//                                          the query's region through a counter, those beyond its capacity counted and not written
//   refine_range_cand_kernel<Row, Lookup>  refine_dist_kernel's gather over the flattened candidate lists: one candidate per wave,
//                                          a workgroup per chunk of one query's segment; the word, or ~0 for a candidate that is
//                                          missing or not below the limit
//   refine_range_sort_kernel               one workgroup per region: a bitonic sort in LDS up to kRangeSortLds words, LSD radix passes
//                                          between the region and a scratch above; counts the survivors
//   refine_range_compact_kernel            one workgroup per region: the survivors written densely at the query's offset
// The distance body is restated here, not shared with the k-NN and rerank kernels: their code and results stay as they are.
#include "qadc_refine.h"

#include <hip/hip_fp16.h>

#include <type_traits>

namespace qadc {
namespace refine {

namespace {

constexpr uint32_t kNanImage = 0x7FC00000u;
constexpr uint64_t kNoWord = ~0ull;

struct sq8_t {                                        // a component of an SQ8 row
    uint8_t b;
};

__device__ inline float row_value(const float* x, int i, float, float) { return x[i]; }
__device__ inline float row_value(const __half* x, int i, float, float) { return __half2float(x[i]); }
__device__ inline float row_value(const sq8_t* x, int i, float vmin, float step) {
    const float m = (float)x[i].b * step;
    return vmin + m;
}

// ScanFilter's rule (csrc/qadc_adc_kernels.h), as refine_knn_dist_kernel applies it
__device__ inline bool range_passes(const adc::ScanFilter& f, uint32_t key) {
    const uint32_t d = key - f.lo;
    const bool marked = d <= f.last && ((f.bitmap[d >> 5] >> (d & 31u)) & 1u);
    return marked == (f.mode == adc::kFilterAllow);
}

constexpr int range_log2(int n) { return n <= 1 ? 0 : 1 + range_log2(n / 2); }

// The tile, the partial sums and the transposed fold are refine_knn_dist_kernel's, operation for operation (its comment explains
// them): lane l keeps the components 64 j + l of the tile's queries, p[q] is the definition's p[l] for query q, and after the fold
// the lanes whose low 6 - log2(QT) bits are zero hold D of query lane >> (6 - log2(QT)) of the tile.  The emit differs: there is no
// bound to lower, only the query's limit word, and the region belongs to the query, whatever group the row lies in.
template <typename Row, int QT, int J>
__global__ __launch_bounds__(kKnnWaves * 64) void refine_range_dist_kernel(const Row* __restrict__ rows, uint32_t lo, uint64_t nrows,
                                                                           const uint32_t* __restrict__ row_key, adc::ScanFilter filter, int dim,
                                                                           const float* __restrict__ sq_vmin, const float* __restrict__ sq_step,
                                                                           const float* __restrict__ queries, int nq, uint64_t chunk_rows,
                                                                           int groups, int slice_rows, int slices, uint64_t launch,
                                                                           const uint64_t* __restrict__ limit, const uint64_t* __restrict__ base,
                                                                           const uint64_t* __restrict__ cap, unsigned long long* __restrict__ cnt,
                                                                           uint64_t* __restrict__ buf) {
    extern __shared__ float s_tile[];   // LDS tile (J == 0): [QT][dim]
    constexpr int kLog = range_log2(QT), kShift = 6 - kLog, JR = J > 0 ? J : 1;
    constexpr bool kSq = std::is_same<Row, sq8_t>::value;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int q0 = blockIdx.x * QT, group = blockIdx.y / slices, slice = blockIdx.y % slices;

    float qr[QT][JR], vr[JR], sr[JR];
#pragma unroll
    for (int j = 0; j < JR; ++j) {
        const int i = 64 * j + lane;
        vr[j] = (kSq && J > 0 && i < dim) ? sq_vmin[i] : 0.0f;
        sr[j] = (kSq && J > 0 && i < dim) ? sq_step[i] : 0.0f;
    }
    if (J > 0) {
#pragma unroll
        for (int q = 0; q < QT; ++q)
#pragma unroll
            for (int j = 0; j < JR; ++j) {
                const int i = 64 * j + lane;
                qr[q][j] = (q0 + q < nq && i < dim) ? queries[(size_t)(q0 + q) * dim + i] : 0.0f;
            }
    } else {
        for (int e = tid; e < QT * dim; e += kKnnWaves * 64) {
            const int q = e / dim;
            s_tile[e] = q0 + q < nq ? queries[(size_t)q0 * dim + e] : 0.0f;
        }
        __syncthreads();
    }

    const int myq = q0 + (lane >> kShift);
    const bool emitter = (lane & ((1 << kShift) - 1)) == 0 && myq < nq;
    const uint64_t my_limit = emitter ? limit[myq] : 0ull;
    const uint64_t my_base = emitter ? base[myq] : 0ull, my_cap = emitter ? cap[myq] : 0ull;

    uint64_t first, last;
    knn_slice(nrows, chunk_rows, groups, slice_rows, launch, group, slice, &first, &last);
    for (uint64_t r = first + wave; r < last; r += kKnnWaves) {
        // (the row, its key and the filter's verdict are the same in every lane of the wave)
        const uint32_t key = __builtin_amdgcn_readfirstlane(row_key ? row_key[r] : lo + (uint32_t)r);
        if (row_key && key == kKeyedEmpty) continue;
        if (filter.bitmap && !range_passes(filter, key)) continue;
        const Row* x = rows + r * (uint64_t)dim;
        float p[QT];
#pragma unroll
        for (int q = 0; q < QT; ++q) p[q] = 0.0f;
        if (J > 0) {
#pragma unroll
            for (int j = 0; j < JR; ++j) {
                const int i = 64 * j + lane;
                const float xv = i < dim ? row_value(x, i, vr[j], sr[j]) : 0.0f;
#pragma unroll
                for (int q = 0; q < QT; ++q) {
                    const float t = qr[q][j] - xv;
                    const float tt = t * t;
                    p[q] = p[q] + tt;
                }
            }
        } else {
            for (int i = lane; i < dim; i += 64) {
                const float xv = row_value(x, i, kSq ? sq_vmin[i] : 0.0f, kSq ? sq_step[i] : 0.0f);
#pragma unroll
                for (int q = 0; q < QT; ++q) {
                    const float t = s_tile[q * dim + i] - xv;
                    const float tt = t * t;
                    p[q] = p[q] + tt;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kLog; ++k) {
            const int h = QT >> (k + 1), s = 32 >> k;
            const bool up = (lane & s) != 0;
#pragma unroll
            for (int i = 0; i < QT / 2; ++i)
                if (i < h) {
                    const float a = p[i], b = p[i + h];
                    const float send = up ? a : b;
                    const float keep = up ? b : a;
                    p[i] = keep + __shfl_xor(send, s, 64);
                }
        }
        float v = p[0];
#pragma unroll
        for (int s = (1 << kShift) >> 1; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
        if (emitter) {
            uint32_t img = __float_as_uint(v);
            if (v != v) img = kNanImage;
            const uint64_t word = ((uint64_t)img << 32) | key;
            if (word < my_limit) {                    // (a NaN's image is above every limit)
                const unsigned long long pos = atomicAdd(cnt + myq, 1ull);
                if (pos < my_cap) buf[my_base + pos] = word;
            }
        }
    }
}

// ---- the candidate form: refine_dist_kernel's lookups, loads and tree ----

__device__ inline uint32_t sq_load4(const sq8_t* x, int b, int dim) {
    uint32_t w = 0;
    if (b + 4 <= dim) {
        __builtin_memcpy(&w, x + b, 4);               // (no alignment is promised: dim may be odd)
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (b + k < dim) w |= (uint32_t)x[b + k].b << (8 * k);
    }
    return w;
}

__device__ inline float sq_lane_value(uint32_t w, int s, int lane, float vmin, float step) {
    const uint32_t v = (uint32_t)__builtin_amdgcn_ds_bpermute((16 * s + (lane >> 2)) << 2, (int)w);
    const float m = (float)((v >> (8 * (lane & 3))) & 0xFFu) * step;
    return vmin + m;
}

struct DenseLookup {                                  // the keys [lo, lo + nrows), row = key - lo
    uint32_t lo;
    uint64_t nrows;
    __device__ inline bool row_of(uint32_t key, uint64_t* row) const {
        *row = (uint64_t)key - lo;
        return key >= lo && *row < nrows;
    }
};

struct KeyedLookup {                                  // linear probing from the key's home slot; the table is at most half used
    const uint32_t* __restrict__ tkey;
    const uint32_t* __restrict__ trow;
    int bits;
    __device__ inline bool row_of(uint32_t key, uint64_t* row) const {
        if (key == kKeyedEmpty) return false;         // (0xFFFFFFFF is never held)
        const uint32_t mask = (1u << bits) - 1u;
        for (uint32_t s = keyed_slot(key, bits);; s = (s + 1u) & mask) {
            const uint32_t k = tkey[s];
            if (k == key) {                           // live, or dead: a removed key is missing
                const uint32_t r = trow[s];
                *row = r;
                return r != kKeyedNoRow;
            }
            if (k == kKeyedEmpty) return false;
        }
    }
};

// grid: the pass's chunks.  Workgroup b owns the candidates [first, first + count) of the pass, all of query q.
template <typename Row, typename Lookup>
__global__ __launch_bounds__(kRefineWaves * 64) void refine_range_cand_kernel(const Row* __restrict__ rows, Lookup look, int dim,
                                                                              const float* __restrict__ sq_vmin, const float* __restrict__ sq_step,
                                                                              const float* __restrict__ queries, const uint32_t* __restrict__ keys,
                                                                              const RangeChunk* __restrict__ chunks,
                                                                              const uint64_t* __restrict__ limit, uint64_t* __restrict__ words,
                                                                              unsigned long long* __restrict__ missing) {
    extern __shared__ float s_query[];   // [dim]; SQ8 rows: then vmin [dim] and step [dim]
    __shared__ unsigned s_missing;
    constexpr bool kSq = std::is_same<Row, sq8_t>::value;
    const RangeChunk chunk = chunks[blockIdx.x];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* qv = queries + (size_t)chunk.q * dim;
    for (int i = tid; i < dim; i += kRefineWaves * 64) {
        s_query[i] = qv[i];
        if (kSq) {
            s_query[dim + i] = sq_vmin[i];
            s_query[2 * dim + i] = sq_step[i];
        }
    }
    if (tid == 0) s_missing = 0;
    __syncthreads();

    const uint64_t my_limit = limit[chunk.q];
    const uint32_t c1 = chunk.count;
    const uint32_t* list = keys + chunk.first;
    uint64_t* out = words + chunk.first;
    unsigned lost = 0;
    for (uint32_t base = wave * kRefineInFlight; base < c1; base += kRefineWaves * kRefineInFlight) {
        const Row* x[kRefineInFlight];
        uint32_t key[kRefineInFlight];
        float p[kRefineInFlight];
#pragma unroll
        for (int c = 0; c < kRefineInFlight; ++c) {   // (everything here is uniform over the wave)
            const uint32_t i = base + c;
            x[c] = nullptr;
            key[c] = 0;
            p[c] = 0.0f;
            if (i < c1) {
                key[c] = list[i];
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
                            const float t = qj - sq_lane_value(w[c], s, lane, vj, sj);
                            const float tt = t * t;
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
                        const float t = qj - row_value(x[c], j, 0.0f, 0.0f);
                        const float tt = t * t;
                        p[c] = p[c] + tt;
                    }
            }
        }
#pragma unroll
        for (int c = 0; c < kRefineInFlight; ++c) {
            float v = p[c];
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s, 64);
            const uint32_t i = base + c;
            if (lane == 0 && i < c1) {
                uint32_t img = __float_as_uint(v);
                if (v != v) img = kNanImage;
                const uint64_t word = ((uint64_t)img << 32) | key[c];
                out[i] = (x[c] && word < my_limit) ? word : kNoWord;
            }
        }
    }
    if (lane == 0 && lost) atomicAdd(&s_missing, lost);
    __syncthreads();
    if (tid == 0 && s_missing) atomicAdd(missing, (unsigned long long)s_missing);
}

// ---- sort and compact ----

// grid nq.  The region's words sorted ascending where they lie — adc_range_sort_kernel's two forms, on words that are already
// words: up to kRangeSortLds a bitonic network in LDS; above, LSD radix passes of 8 bits that alternate between the region and
// tmp[base[q] ..), skipping every digit in which all words agree, and a copy back where the last pass ended in tmp.  Equal words
// are the same (distance, key) pair, so the sorted region is a function of the multiset of its words, whatever order the atomics
// gave them.  Then kept[q] = the words that are not ~0 and differ from the word before them.
__global__ __launch_bounds__(kRangeSortThreads) void refine_range_sort_kernel(const uint64_t* __restrict__ base, const uint64_t* __restrict__ cap,
                                                                              const unsigned long long* __restrict__ cnt, uint64_t* buf,
                                                                              uint64_t* tmp_all, uint32_t* __restrict__ kept) {
    constexpr int T = kRangeSortThreads;
    __shared__ unsigned long long lkey[kRangeSortLds];
    __shared__ unsigned long long s_or, s_and;
    __shared__ uint32_t s_kept;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t n = (uint32_t)min((unsigned long long)cnt[q], (unsigned long long)cap[q]);   // (a run holds at most 2^31 words)
    if (n == 0) {
        if (tid == 0) kept[q] = 0;
        return;
    }
    uint64_t* words = buf + base[q];
    if (tid == 0) {
        s_or = 0;
        s_and = ~0ull;
        s_kept = 0;
    }
    __syncthreads();

    if (n <= (uint32_t)kRangeSortLds) {
        uint32_t n2 = 1;
        while (n2 < n) n2 <<= 1;
        for (uint32_t i = tid; i < n2; i += T) lkey[i] = i < n ? words[i] : kNoWord;
        __syncthreads();
        for (uint32_t k = 2; k <= n2; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t t = tid; t < n2 / 2; t += T) {
                    const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                    const unsigned long long a = lkey[i], b = lkey[p];
                    if ((a > b) == ((i & k) == 0)) { lkey[i] = b; lkey[p] = a; }
                }
                __syncthreads();
            }
        uint32_t mine = 0;
        for (uint32_t i = tid; i < n; i += T) {
            const unsigned long long e = lkey[i];
            words[i] = e;
            mine += (e != kNoWord && (i == 0 || e != lkey[i - 1])) ? 1u : 0u;
        }
        if (mine) atomicAdd(&s_kept, mine);
        __syncthreads();
        if (tid == 0) kept[q] = s_kept;
        return;
    }

    {                                                            // which digits differ anywhere
        unsigned long long o = 0, a = ~0ull;
        for (uint32_t i = tid; i < n; i += T) {
            const unsigned long long e = words[i];
            o |= e;
            a &= e;
        }
        atomicOr(&s_or, o);
        atomicAnd(&s_and, a);
    }
    __syncthreads();
    const unsigned long long differ = s_or ^ s_and;
    uint32_t active = 0;                                         // bit d: digit d (bits [8d, 8d + 8) of the word) gets a pass
    for (int d = 0; d < 8; ++d)
        if ((differ >> (8 * d)) & 255ull) active |= 1u << d;

    uint32_t* hist = reinterpret_cast<uint32_t*>(lkey);          // [256] entries of the digit, then its running write position
    uint32_t* wcount = hist + 256;                               // [4][256] entries of the digit in each wave of the tile
    uint64_t* tmp = tmp_all + base[q];
    const uint32_t lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    int pass = 0;
    for (int digit = 0; digit < 8; ++digit) {
        if (!((active >> digit) & 1u)) continue;                 // (the same in every lane)
        const uint64_t* src = (pass & 1) ? tmp : words;
        uint64_t* dst = (pass & 1) ? words : tmp;
        const int shift = 8 * digit;
        ++pass;
        hist[tid] = 0;
        for (int w = 0; w < 4; ++w) wcount[w * 256 + tid] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += T) atomicAdd(&hist[(uint32_t)(src[i] >> shift) & 255u], 1u);
        __syncthreads();
        if (tid < 64) {                                          // wave 0: exclusive prefix sums, lane l holds digits 4l .. 4l+3
            const uint32_t h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
            uint32_t incl = h0 + h1 + h2 + h3;
            for (int step = 1; step < 64; step <<= 1) {
                const uint32_t o = __shfl_up(incl, step);
                if (tid >= (uint32_t)step) incl += o;
            }
            const uint32_t excl = incl - (h0 + h1 + h2 + h3);
            hist[4 * tid] = excl;
            hist[4 * tid + 1] = excl + h0;
            hist[4 * tid + 2] = excl + h0 + h1;
            hist[4 * tid + 3] = excl + h0 + h1 + h2;
        }
        __syncthreads();
        for (uint32_t t0 = 0; t0 < n; t0 += T) {                 // (n <= 2^31: t0 + tid does not wrap)
            const bool valid = t0 + tid < n;
            const uint32_t i = t0 + tid;
            const unsigned long long e = valid ? src[i] : 0ull;
            const uint32_t d = (uint32_t)(e >> shift) & 255u;
            unsigned long long same = __ballot(valid);           // lanes of this wave with the same digit
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
                uint32_t pos = hist[d] + rank;
                for (uint32_t w = 0; w < wave; ++w) pos += wcount[w * 256 + d];
                dst[pos] = e;                                    // (pos < n: the digits' counts sum to n)
            }
            __syncthreads();
            {                                                    // thread d owns digit d: advance its position, clear the counts
                uint32_t c = 0;
                for (int w = 0; w < 4; ++w) {
                    c += wcount[w * 256 + tid];
                    wcount[w * 256 + tid] = 0;
                }
                hist[tid] += c;
            }
            __syncthreads();
        }
    }
    if (pass & 1) {                                              // the last pass wrote tmp
        for (uint32_t i = tid; i < n; i += T) words[i] = tmp[i];
        __syncthreads();
    }
    uint32_t mine = 0;
    for (uint32_t i = tid; i < n; i += T) {
        const unsigned long long e = words[i];
        mine += (e != kNoWord && (i == 0 || e != words[i - 1])) ? 1u : 0u;
    }
    if (mine) atomicAdd(&s_kept, mine);
    __syncthreads();
    if (tid == 0) kept[q] = s_kept;
}

// grid nq.  The sorted region's survivors, in order, to out_keys / out_dist [out_off[q] ..): a tile of T words at a time, a
// survivor's place = the survivors before the tile + those of the earlier waves + those of the lower lanes of its wave.
__global__ __launch_bounds__(kRangeSortThreads) void refine_range_compact_kernel(const uint64_t* __restrict__ base, const uint64_t* __restrict__ cap,
                                                                                 const unsigned long long* __restrict__ cnt,
                                                                                 const uint64_t* __restrict__ buf, const uint64_t* __restrict__ out_off,
                                                                                 uint32_t* __restrict__ out_keys, float* __restrict__ out_dist) {
    constexpr int T = kRangeSortThreads, W = T / 64;
    __shared__ uint32_t s_wave[W];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n = (uint32_t)min((unsigned long long)cnt[q], (unsigned long long)cap[q]);
    const uint64_t* words = buf + base[q];
    uint32_t* ok = out_keys + out_off[q];
    float* od = out_dist + out_off[q];
    uint32_t done = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += T) {
        const uint32_t i = t0 + tid;
        const uint64_t e = i < n ? words[i] : kNoWord;
        const bool keep = e != kNoWord && (i == 0 || e != words[i - 1]);
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t pos = done + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if ((uint32_t)w < wave) pos += s_wave[w];
            total += s_wave[w];
        }
        if (keep) {
            ok[pos] = (uint32_t)e;
            od[pos] = __uint_as_float((uint32_t)(e >> 32));
        }
        done += total;
        __syncthreads();
    }
}

template <typename Row, int QT, int J>
hipError_t launch_dist(const RangeStore& s, const adc::ScanFilter& filter, const float* queries, const RangeRegions& g, const RangePlan& plan,
                       uint64_t launch, int live, hipStream_t stream) {
    const dim3 grid((unsigned)((g.nq + QT - 1) / QT), (unsigned)(live * plan.slices)), block(kKnnWaves * 64);
    hipLaunchKernelGGL((refine_range_dist_kernel<Row, QT, J>), grid, block, plan.dist_lds_bytes, stream, static_cast<const Row*>(s.rows), s.lo,
                       s.nrows, s.row_key, filter, s.dim, s.sq.vmin, s.sq.step, queries, g.nq, plan.chunk_rows, plan.groups, plan.slice_rows,
                       plan.slices, launch, g.limit, g.base, g.cap, g.cnt, g.buf);
    return hipGetLastError();
}

template <typename Row>
hipError_t dispatch_dist(const RangeStore& s, const adc::ScanFilter& filter, const float* queries, const RangeRegions& g, const RangePlan& plan,
                         uint64_t launch, int live, hipStream_t stream) {
#define QADC_RANGE(QT, J) \
    if (plan.qt == QT && plan.jregs == J) return launch_dist<Row, QT, J>(s, filter, queries, g, plan, launch, live, stream)
    QADC_RANGE(32, 1); QADC_RANGE(32, 2); QADC_RANGE(16, 3); QADC_RANGE(16, 4);
    QADC_RANGE(4, 1); QADC_RANGE(4, 2); QADC_RANGE(4, 3); QADC_RANGE(4, 4);
    QADC_RANGE(32, 0); QADC_RANGE(16, 0); QADC_RANGE(8, 0); QADC_RANGE(4, 0);
#undef QADC_RANGE
    return hipErrorInvalidValue;   // (a tile the plan does not make)
}

}  // namespace

hipError_t launch_range_dist(const RangeStore& s, const adc::ScanFilter& filter, const float* queries, const RangeRegions& g,
                             const RangePlan& plan, uint64_t launch, hipStream_t stream) {
    const int live = knn_launch_groups(s.nrows, plan.chunk_rows, plan.groups, launch);
    if (live == 0 || g.nq == 0) return hipSuccess;
    if (s.elem == Elem::kSQ8) return dispatch_dist<sq8_t>(s, filter, queries, g, plan, launch, live, stream);
    return s.elem == Elem::kF16 ? dispatch_dist<__half>(s, filter, queries, g, plan, launch, live, stream)
                                : dispatch_dist<float>(s, filter, queries, g, plan, launch, live, stream);
}

hipError_t launch_range_cand(const RangeStore& s, const float* queries, const uint32_t* keys, const RangeChunk* chunks, uint32_t nchunks,
                             const RangeRegions& g, unsigned long long* missing, hipStream_t stream) {
    if (nchunks == 0) return hipSuccess;
    const dim3 grid(nchunks), block(kRefineWaves * 64);
    const DenseLookup dense{s.lo, s.nrows};
    const KeyedLookup keyed{s.tkey, s.trow, s.tbits};
    // (SQ8 rows: vmin and step behind the query, 3 * dim floats <= 48 KiB)
    const size_t lds = (size_t)s.dim * sizeof(float) * (s.elem == Elem::kSQ8 ? 3 : 1);
#define QADC_RC(ROW, LOOKUP, look)                                                                                                         \
    hipLaunchKernelGGL((refine_range_cand_kernel<ROW, LOOKUP>), grid, block, lds, stream, static_cast<const ROW*>(s.rows), look, s.dim, s.sq.vmin, \
                       s.sq.step, queries, keys, chunks, g.limit, g.buf, missing)
    if (s.tkey) {
        if (s.elem == Elem::kSQ8) QADC_RC(sq8_t, KeyedLookup, keyed);
        else if (s.elem == Elem::kF16) QADC_RC(__half, KeyedLookup, keyed);
        else QADC_RC(float, KeyedLookup, keyed);
    } else {
        if (s.elem == Elem::kSQ8) QADC_RC(sq8_t, DenseLookup, dense);
        else if (s.elem == Elem::kF16) QADC_RC(__half, DenseLookup, dense);
        else QADC_RC(float, DenseLookup, dense);
    }
#undef QADC_RC
    return hipGetLastError();
}

hipError_t launch_range_sort(const RangeRegions& g, uint32_t* kept, hipStream_t stream) {
    if (g.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(refine_range_sort_kernel, dim3((unsigned)g.nq), dim3(kRangeSortThreads), 0, stream, g.base, g.cap, g.cnt, g.buf, g.tmp, kept);
    return hipGetLastError();
}

hipError_t launch_range_compact(const RangeRegions& g, const uint64_t* out_off, uint32_t* out_keys, float* out_dist, hipStream_t stream) {
    if (g.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(refine_range_compact_kernel, dim3((unsigned)g.nq), dim3(kRangeSortThreads), 0, stream, g.base, g.cap, g.cnt, g.buf, out_off,
                       out_keys, out_dist);
    return hipGetLastError();
}

}  // namespace refine
}  // namespace qadc
