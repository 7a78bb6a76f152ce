// Float ADC over whole-byte PQ codes on gfx950: the GPU form of the reference's scan_standard<uint8_t | uint16_t, NSQ>
// (query_common.hpp:92-118) as scanner_simple::query_scan drives it (db_query.cpp:26-45).  Host side: csrc/qadc_adc.cpp.
//
//   adc_scan_kernel    one workgroup per run of codes of one probed partition: the (query, slot) float table goes to LDS, each lane
//                      sums the looked-up entries of its codes in the reference's grouping and emits (candidate, key, scan index)
//                      when candidate < bound[query].  One body over ByteCodes<NSQ> (tables [NSQ][256], the owned database by
//                      value), NibbleCodes<M> (the view: a 4-bit index read in place, scan_4<M>, tables [M][16]) and
//                      WordCodes<NSQ> (16-bit codes, tables [NSQ][65536]: too large for LDS, gathered from global memory);
//   adc_scan_filtered_kernel  the same body with a key filter in front of the emit (qadc_adc_index_set_filter, section 11.10);
//   adc_scan_qfiltered_kernel the same body with the index's filter and the filter of the workgroup's own query (the *_filtered
//                             calls, section 11.12);
//   adc_select_kernel one workgroup per query: bound = the R-th smallest value the query emitted so far (radix select on
//                      the order-preserving integer image of the floats), the bound of the next level's runs;
//   adc_pack_kernel    the per-query regions packed densely for one device-to-host copy;
//   adc_order_kernel   the device finish: each query's stored candidates put in scan order (LDS sort, or radix passes through
//                      global scratch for streams of any length);
//   adc_replay_kernel  the device finish: the ordered stream pushed through kv_binheap<unsigned, float>(R) in LDS, one wave per query;
//   adc_tables_kernel  the float tables of every (query, probe) from query vectors (residual, OPQ rotation, both table forms);
//   adc_encode_kernel  vectors -> one code byte per sub-quantizer;
//   adc_encode16_kernel  vectors -> one 16-bit code per sub-quantizer of 65536 centroids (and adc_encode16_merge_kernel);
//   adc_add_* / index_* / remove_*  the database that grows and shrinks in device memory (sections 11.5 to 11.7), further down.
// The bound rule and why it is exact: DESIGN.md section 11.  Built with -ffp-contract=off and without fast-math (Makefile):
// every sum rounds like the reference's.
#include <algorithm>
#include <cfloat>
#include <type_traits>

#include "../host/adc_tables_plan.hpp"     // adc_tables_plan, adc_encode_plan: the feeders' launch geometry
#include "../host/index_append_plan.hpp"   // index_padded_end: the span kept zero behind a partition's last row
#include "qadc_adc_kernels.h"
#include "qadc_float_sum.h"

namespace qadc {
namespace adc {
namespace {

template <int BYTES>
struct alignas(BYTES) CodeWords {   // one code, 4, 8 or 16 bytes = one dword, dwordx2 or dwordx4 load
    uint32_t w[BYTES / 4];
};

// What a code is and how its looked-up entries are summed: the only things the scan kernel leaves to a policy.  kBytes =
// bytes per code (one dword, dwordx2 or dwordx4 load), kTable = floats of one (query, slot) table, kTableInLds = the kernel
// copies that table to LDS before it scans, sum<SUM>(table, words) = the candidate of one code in the reference's float
// grouping (SUM 0 source order, 1 as compiled).
template <int NSQ>
struct ByteCodes {   // scan_standard<uint8_t, NSQ>: one byte per sub-quantizer, tables [NSQ][256]
    static constexpr int kBytes = NSQ, kTable = NSQ * 256;
    static constexpr bool kTableInLds = true;
    template <int SUM>
    static __device__ __forceinline__ float sum(const float* lds, const CodeWords<kBytes>& c) {
        float t[NSQ];
#pragma unroll
        for (int m = 0; m < NSQ; ++m) t[m] = lds[m * 256 + ((c.w[m / 4] >> (8 * (m % 4))) & 0xffu)];
        if constexpr (SUM == 0) {                                 // source order, from 0 like the reference's loop
            float s = 0.0f;
#pragma unroll
            for (int m = 0; m < NSQ; ++m) s += t[m];
            return s;
        } else if constexpr (NSQ == 4) {
            return adc_sum4_standard_compiled(t);
        } else if constexpr (NSQ == 8) {
            return adc_sum8_standard_compiled(t);
        } else {
            return adc_sum8_compiled_first(t);
        }
    }
};

// The nibble form: scan_4<M> (query_common.hpp:59-90) over the partitions of a 4-bit index, read in place.  A code is
// M/2 bytes = one dwordx2 (M 16) or dwordx4 (M 32) load; sub-quantizer m's entry is table[m][nibble m], nibble m = bits
// 4(m % 8) .. of word m / 8 (the even sub-quantizer in the low nibble of its byte).  The (query, slot) table [M][16] is 1 or
// 2 KiB of LDS.  Every lane of a wave reads sub-quantizer m in the same instruction: its 16 entries lie in 16 distinct
// banks and equal addresses broadcast, so the lookups cannot conflict.
template <int M>
struct NibbleCodes {
    static constexpr int kBytes = M / 2, kTable = M * 16;
    static constexpr bool kTableInLds = true;
    template <int SUM>
    static __device__ __forceinline__ float sum(const float* lds, const CodeWords<kBytes>& c) {
        float v[M];
#pragma unroll
        for (int m = 0; m < M; ++m) v[m] = lds[m * 16 + ((c.w[m / 8] >> (4 * (m % 8))) & 15u)];
        return adc_sum_code<M>(v, SUM, 0.0f);
    }
};

// scan_standard<uint16_t, NSQ>: one little-endian 16-bit word per sub-quantizer, tables [NSQ][65536] — 512 KiB, 1 MiB or 2 MiB per
// (query, slot), which no LDS holds: the table stays in global memory and every entry is a cached 4-byte gather, served by
// the L2 of the workgroup's XCD while the tables live in a launch fit it.  The kernel reads the
// codes with non-temporal loads so that the code stream does not push table lines out.  gather() issues the NSQ loads of one
// code and add<SUM>() sums them, so that the kernel can have the loads of all its codes in flight before the first add.
// Grouping (pinned by tests/golden/ref_scan_standard_u16_cases.npz): NSQ 2 t0 + t1 (no leading 0 +), NSQ 4 and 8 as the
// uint8_t instances.
template <int NSQ>
struct WordCodes {
    static constexpr int kBytes = 2 * NSQ, kTable = NSQ * 65536;
    static constexpr bool kTableInLds = false;
    static __device__ __forceinline__ void gather(const float* __restrict__ tab, const CodeWords<kBytes>& c, float* t) {
#pragma unroll
        for (int m = 0; m < NSQ; ++m) t[m] = tab[m * 65536 + ((c.w[m / 2] >> (16 * (m % 2))) & 0xffffu)];
    }
    template <int SUM>
    static __device__ __forceinline__ float add(const float* t) {
        if constexpr (SUM == 0) {                                 // source order, from 0 like the reference's loop
            float s = 0.0f;
#pragma unroll
            for (int m = 0; m < NSQ; ++m) s += t[m];
            return s;
        } else if constexpr (NSQ == 4) {
            return adc_sum4_standard_compiled(t);
        } else if constexpr (NSQ == 8) {
            return adc_sum8_standard_compiled(t);
        } else {
            return t[0] + t[1];
        }
    }
    template <int SUM>
    static __device__ __forceinline__ float sum(const float* tab, const CodeWords<kBytes>& c) {
        float t[NSQ];
        gather(tab, c, t);
        return add<SUM>(t);
    }
};

// One code by a non-temporal load (the word policy: a code is read once and must not displace table lines in L2).
template <int BYTES>
__device__ __forceinline__ CodeWords<BYTES> load_code_streaming(const CodeWords<BYTES>* p) {
    typedef uint32_t words_t __attribute__((ext_vector_type(BYTES / 4)));
    CodeWords<BYTES> c;
    if constexpr (BYTES == 4) {
        c.w[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
    } else {
        const words_t v = __builtin_nontemporal_load(reinterpret_cast<const words_t*>(p));
#pragma unroll
        for (int i = 0; i < BYTES / 4; ++i) c.w[i] = v[i];
    }
    return c;
}

// Where a partition lies, from what the kernel was given (its Source): the owned database by value, or a view's partition table.
struct PartRef { const uint8_t* codes; const uint32_t* labels; uint32_t key_base; };   // labels null: key = key_base + position
__device__ __forceinline__ PartRef locate(const Db& db, int part) {
    return PartRef{db.codes + db.off[part], db.labels ? db.labels + db.lab_off[part] : nullptr, 0u};
}
__device__ __forceinline__ PartRef locate(const Part4* parts, int part) {
    const Part4 p = parts[part];
    return PartRef{p.codes, p.labels, p.key_base};
}

constexpr int kUnroll = 4;   // codes per lane in flight

// The key bitmap of remove-by-label and of the filtered scan, without a branch so that the loads of several rows go out
// together: the bitmap word of a key inside [lo, lo + last] (word 0 for one outside: the bitmap has one word at least), then the test.
__device__ __forceinline__ uint32_t remove_word(const uint32_t* __restrict__ bitmap, uint32_t lo, uint32_t last, uint32_t label) {
    const uint32_t d = label - lo;
    return bitmap[d <= last ? d >> 5 : 0u];
}
__device__ __forceinline__ bool remove_marked(uint32_t word, uint32_t lo, uint32_t last, uint32_t label) {
    const uint32_t d = label - lo;
    return d <= last && ((word >> (d & 31u)) & 1u);
}

// Which rows the scan may emit (qadc_adc_index_set_filter): the compile-time policy of adc_scan_body.
// NoFilter: every row, and the kernel's code is the unfiltered kernel's.  KeyFilter: the rows whose key passes the ScanFilter —
// a key marked in the bitmap is dropped under QADC_ADC_FILTER_EXCLUDE and is the only kind kept under QADC_ADC_FILTER_ALLOW; a key
// outside [lo, lo + last] is not marked.  QueryFilter: the rows that pass both the index's ScanFilter and the one of the workgroup's
// query (the *_filtered calls; section 11.12); either may be absent (bitmap null), which is a branch on a value the whole
// workgroup shares, so remove_word never sees a null bitmap.
struct NoFilter {
    static constexpr bool kOn = false;
    __device__ __forceinline__ bool passes(uint32_t) const { return true; }
};
struct KeyFilter {
    static constexpr bool kOn = true;
    ScanFilter f;
    __device__ __forceinline__ bool passes(uint32_t key) const {
        return remove_marked(remove_word(f.bitmap, f.lo, f.last, key), f.lo, f.last, key) == (f.mode == kFilterAllow);
    }
};
struct QueryFilter {
    static constexpr bool kOn = true;
    ScanFilter index, query;   // the same in every lane of the workgroup: kernel argument and table entry [it.query]
    __device__ __forceinline__ bool passes(uint32_t key) const {
        bool ok = true;
        if (index.bitmap) ok = KeyFilter{index}.passes(key);
        if (query.bitmap) ok = ok & KeyFilter{query}.passes(key);
        return ok;
    }
};

template <class Code, int SUM, class Source, class Filter>
__device__ __forceinline__ void adc_scan_body(const Item* __restrict__ items, uint32_t first, Source src,
                                              const int32_t* __restrict__ assign, int ma, const float* __restrict__ tables,
                                              const float* __restrict__ bound, Emit emit, Filter filter,
                                              [[maybe_unused]] const ScanFilter* __restrict__ qfilters = nullptr) {
    constexpr int CS = Code::kBytes;
    constexpr bool kLds = Code::kTableInLds;
    __shared__ float lds[kLds ? Code::kTable : 1];                // (the word policy's table stays where it is)
    const Item it = items[first + blockIdx.x];
    const PartRef part = locate(src, assign[(size_t)it.query * ma + it.slot]);
    const float* __restrict__ gtab = tables + ((size_t)it.query * ma + it.slot) * Code::kTable;
    if constexpr (kLds) {
        const float4* tab = reinterpret_cast<const float4*>(gtab);
        for (int i = threadIdx.x; i < Code::kTable / 4; i += kWG) reinterpret_cast<float4*>(lds)[i] = tab[i];
    }
    if constexpr (std::is_same<Filter, QueryFilter>::value) filter.query = qfilters[it.query];   // once per workgroup
    const float b = bound[it.query];
    const uint64_t region = emit.base[it.query];
    const uint32_t cap = emit.cap[it.query];
    if constexpr (kLds) __syncthreads();

    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    for (uint32_t base = 0; base < it.count; base += kWG * kUnroll) {
        CodeWords<CS> c[kUnroll];
        bool valid[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const uint32_t r = base + u * kWG + threadIdx.x;
            valid[u] = r < it.count;
            if constexpr (kLds) {
                if (valid[u]) c[u] = reinterpret_cast<const CodeWords<CS>*>(part.codes)[it.start + r];
            } else {   // no branch around the loads: a lane past the run's end reads the run's last code and its sum is dropped
                c[u] = load_code_streaming(reinterpret_cast<const CodeWords<CS>*>(part.codes) + it.start + min(r, it.count - 1));
            }
        }
        [[maybe_unused]] float t[kLds ? 1 : kUnroll][kLds ? 1 : Code::kBytes / 2];
        if constexpr (!kLds) {                                    // every gather of the lane is issued before the first add
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) Code::gather(gtab, c[u], t[u]);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            float v = 0.0f;
            if constexpr (kLds) {
                if (valid[u]) v = Code::template sum<SUM>(lds, c[u]);
            } else {
                v = Code::template add<SUM>(t[u]);
            }
            bool keep = valid[u] && v < b;                        // a NaN v or b and v = +inf never pass.  Top-R: b <= FLT_MAX, so FLT_MAX
                                                                  // does not either; range: b is the radius, any float, and under
                                                                  // +inf FLT_MAX passes, under NaN and -inf nothing, -inf under the rest
            [[maybe_unused]] uint32_t key = 0;
            if constexpr (Filter::kOn) {                          // ahead of the ballot and the count: a dropped row is in no level's
                if (keep) {                                       // stored values, so no bound ever comes from it; a lane that fails the
                    const uint32_t r = base + u * kWG + threadIdx.x;   // bound reads neither label nor bitmap
                    key = part.labels ? part.labels[it.start + r] : part.key_base + it.start + r;
                    keep = filter.passes(key);
                }
            }
            const unsigned long long m = __ballot(keep);
            if (m == 0) continue;
            const int leader = __builtin_ctzll(m);
            uint32_t o = 0;
            if (lane == leader) o = atomicAdd(emit.count + it.query, (uint32_t)__popcll(m));
            o = __shfl(o, leader) + (uint32_t)__popcll(m & below);
            if (keep && o < cap) {
                const uint32_t r = base + u * kWG + threadIdx.x;
                const size_t at = region + o;
                emit.vals[at] = v;
                if constexpr (Filter::kOn) emit.keys[at] = key;
                else emit.keys[at] = part.labels ? part.labels[it.start + r] : part.key_base + it.start + r;
                emit.sidx[at] = it.sbase + r;
            }
        }
    }
}

// The three kernels over the body: the unfiltered one, whose arguments and code are what they were before there was a filter, the
// filtered one, which takes the filter by value behind them, and the per-query one, which takes the table of the call's queries too.
template <class Code, int SUM, class Source>
__global__ __launch_bounds__(kWG) void adc_scan_kernel(const Item* __restrict__ items, uint32_t first, Source src,
                                                       const int32_t* __restrict__ assign, int ma,
                                                       const float* __restrict__ tables, const float* __restrict__ bound,
                                                       Emit emit) {
    adc_scan_body<Code, SUM>(items, first, src, assign, ma, tables, bound, emit, NoFilter{});
}

template <class Code, int SUM, class Source>
__global__ __launch_bounds__(kWG) void adc_scan_filtered_kernel(const Item* __restrict__ items, uint32_t first, Source src,
                                                                const int32_t* __restrict__ assign, int ma,
                                                                const float* __restrict__ tables, const float* __restrict__ bound,
                                                                Emit emit, ScanFilter filter) {
    adc_scan_body<Code, SUM>(items, first, src, assign, ma, tables, bound, emit, KeyFilter{filter});
}

template <class Code, int SUM, class Source>
__global__ __launch_bounds__(kWG) void adc_scan_qfiltered_kernel(const Item* __restrict__ items, uint32_t first, Source src,
                                                                 const int32_t* __restrict__ assign, int ma,
                                                                 const float* __restrict__ tables, const float* __restrict__ bound,
                                                                 Emit emit, ScanFilter filter, const ScanFilter* __restrict__ qfilters) {
    adc_scan_body<Code, SUM>(items, first, src, assign, ma, tables, bound, emit, QueryFilter{filter, ScanFilter{}}, qfilters);
}

// order-preserving image of a float (never NaN here): -x < -y < -0 < +0 < y < x
__device__ __forceinline__ uint32_t order_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_val(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(kWG) void adc_select_kernel(int R, Emit emit, float* __restrict__ bound) {
    const uint32_t q = blockIdx.x;
    const uint32_t n = min(emit.count[q], emit.cap[q]);
    if (n < (uint32_t)R) return;                                 // fewer than R: the FLT_MAX padding is the R-th smallest
    const float* v = emit.vals + emit.base[q];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_k;
    uint32_t prefix = 0, k = (uint32_t)R;                        // k = rank (1-based) still to find under the prefix
    for (int shift = 24; shift >= 0; shift -= 8) {
        const uint32_t mask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += kWG) {
            const uint32_t u = order_key(v[i]);
            if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 64) {                                  // wave 0: lane l holds bins 4l .. 4l+3; prefix sums by shuffles
            const uint32_t l = threadIdx.x;
            const uint32_t h0 = hist[4 * l], h1 = hist[4 * l + 1], h2 = hist[4 * l + 2], h3 = hist[4 * l + 3];
            uint32_t incl = h0 + h1 + h2 + h3;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d);
                if (l >= (uint32_t)d) incl += o;
            }
            const uint32_t excl = incl - (h0 + h1 + h2 + h3);
            if (excl < k && k <= incl) {                         // exactly one lane: the k-th value is in its bins
                uint32_t cum = excl, bin = 4 * l;
                if (cum + h0 < k) { cum += h0; ++bin;
                    if (cum + h1 < k) { cum += h1; ++bin;
                        if (cum + h2 < k) { cum += h2; ++bin; } } }
                s_prefix = prefix | (bin << shift);
                s_k = k - cum;
            }
        }
        __syncthreads();
        prefix = s_prefix;
        k = s_k;
    }
    if (threadIdx.x == 0) bound[q] = fminf(bound[q], order_val(prefix));
}

__global__ __launch_bounds__(kWG) void adc_pack_kernel(Emit emit, uint32_t* __restrict__ out) {
    const uint32_t q = blockIdx.x;
    __shared__ unsigned long long s_off;
    if (threadIdx.x == 0) s_off = 0;
    __syncthreads();
    unsigned long long part = 0;
    for (uint32_t j = threadIdx.x; j < q; j += kWG) part += min(emit.count[j], emit.cap[j]);
    if (part) atomicAdd(&s_off, part);
    __syncthreads();
    const size_t off = s_off;
    const uint32_t n = min(emit.count[q], emit.cap[q]);
    const size_t src = emit.base[q];
    for (uint32_t i = threadIdx.x; i < n; i += kWG) {
        uint32_t* r = out + 3 * (off + i);
        r[0] = __float_as_uint(emit.vals[src + i]);
        r[1] = emit.keys[src + i];
        r[2] = emit.sidx[src + i];
    }
}

// ---------------------------------------------------------------------------------------------
// The device finish: what the host otherwise does with the packed stream.
//
// adc_order_kernel: one workgroup per query puts the query's stored candidates in scan order (scan indices are distinct
// within a query) and writes (value, key) of the i-th candidate of the scan to ovals / okeys [base[q] + i].
//   n <= kOrderLds   a bitonic sort of (scan index << 32 | position in the region) in LDS;
//   longer streams   LSD radix passes of 8 bits over the `bits` low bits of the scan index (the host knows the longest scan
//                    order of the batch), one workgroup per query, through the global scratch tmp_a / tmp_b [base[q] + i]:
//                    a histogram of the digit, then a stable scatter tile by tile (256 entries, one per thread: rank among
//                    the equal digits of the wave by ballots, of the waves before through LDS counts).  The last pass
//                    writes (value, key) instead of the pair.  The passes of a query meet only inside its workgroup, so a
//                    workgroup barrier orders them.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void wave_lds_sync() {
    // LDS operations of one wave execute in order; this only stops the compiler from moving them
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(kWG) void adc_order_kernel(Emit emit, int bits, float* __restrict__ ovals,
                                                        uint32_t* __restrict__ okeys, unsigned long long* tmp_a,
                                                        unsigned long long* tmp_b) {
    __shared__ unsigned long long lkey[kOrderLds];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t n = min(emit.count[q], emit.cap[q]);
    if (n == 0) return;
    const size_t region = emit.base[q];
    const float* __restrict__ vals = emit.vals + region;
    const uint32_t* __restrict__ keys = emit.keys + region;
    const uint32_t* __restrict__ sidx = emit.sidx + region;
    float* __restrict__ ov = ovals + region;
    uint32_t* __restrict__ ok = okeys + region;

    if (n <= (uint32_t)kOrderLds) {
        uint32_t n2 = 1;
        while (n2 < n) n2 <<= 1;
        for (uint32_t i = tid; i < n2; i += kWG) lkey[i] = i < n ? ((unsigned long long)sidx[i] << 32) | i : ~0ull;
        __syncthreads();
        for (uint32_t k = 2; k <= n2; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t t = tid; t < n2 / 2; t += kWG) {   // the t-th pair of this step: i has bit j clear
                    const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                    const unsigned long long a = lkey[i], b = lkey[p];
                    if ((a > b) == ((i & k) == 0)) { lkey[i] = b; lkey[p] = a; }
                }
                __syncthreads();
            }
        for (uint32_t i = tid; i < n; i += kWG) {
            const uint32_t j = (uint32_t)lkey[i];
            ov[i] = vals[j];
            ok[i] = keys[j];
        }
        return;
    }

    uint32_t* hist = reinterpret_cast<uint32_t*>(lkey);          // [256] entries of the digit, then its running write position
    uint32_t* wcount = hist + 256;                               // [4][256] entries of the digit in each wave of the tile
    unsigned long long* ta = tmp_a + region;
    unsigned long long* tb = tmp_b + region;
    const uint32_t lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    const int passes = (bits + 7) / 8;
    for (int pass = 0; pass < passes; ++pass) {
        const unsigned long long* src = (pass & 1) ? ta : tb;    // pass 0 reads the region itself
        unsigned long long* dst = (pass & 1) ? tb : ta;
        const int shift = 32 + 8 * pass;
        const bool last = pass + 1 == passes;
        auto entry = [&](uint32_t i) { return pass == 0 ? ((unsigned long long)sidx[i] << 32) | i : src[i]; };
        hist[tid] = 0;
        for (int w = 0; w < 4; ++w) wcount[w * 256 + tid] = 0;
        __syncthreads();
        for (unsigned long long i = tid; i < n; i += kWG) atomicAdd(&hist[(uint32_t)(entry((uint32_t)i) >> shift) & 255u], 1u);
        __syncthreads();
        if (tid < 64) {                                          // wave 0: exclusive prefix sums, lane l holds digits 4l .. 4l+3
            const uint32_t h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
            uint32_t incl = h0 + h1 + h2 + h3;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d);
                if (tid >= (uint32_t)d) incl += o;
            }
            const uint32_t excl = incl - (h0 + h1 + h2 + h3);
            hist[4 * tid] = excl;
            hist[4 * tid + 1] = excl + h0;
            hist[4 * tid + 2] = excl + h0 + h1;
            hist[4 * tid + 3] = excl + h0 + h1 + h2;
        }
        __syncthreads();
        for (unsigned long long t0 = 0; t0 < n; t0 += kWG) {     // (64-bit: n may be within 256 of 2^32)
            const bool valid = t0 + tid < n;
            const uint32_t i = (uint32_t)(t0 + tid);
            const unsigned long long e = valid ? entry(i) : 0ull;
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
                if (last) {
                    const uint32_t j = (uint32_t)e;
                    ov[pos] = vals[j];
                    ok[pos] = keys[j];
                } else {
                    dst[pos] = e;
                }
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
}

// adc_replay_kernel: kv_binheap<unsigned, float>::push (binheap.hpp:75-116) on the device, the float twin of
// replay_heap_kernel (csrc/qadc_kernels.hip).  One wave per query, `waves` queries per workgroup, each with its heap
// [R] (key | value bits << 32) and a 64-entry stage in LDS.  The R sentinels come first (db_query.cpp:31-33) and
// FLT_MAX - t is FLT_MAX for every t the engine takes, and equal values appended never move: the heap starts as R times
// (0, FLT_MAX), full, and only the full branch of push remains — accepted iff strictly below the root, sinking with the
// left child preferred unless the right one is strictly greater, stopping at a child <= the value.  All compares are float
// compares (-0 == +0), as the reference's.  The lanes stage 64 entries of the ordered stream at a time and drop those not
// below the root as it stands (the root only falls); lane 0 pushes the rest in order.  Output: the heap's arrays.
__global__ __launch_bounds__(kWG) void adc_replay_kernel(int nq, int R, const uint32_t* __restrict__ count,
                                                         const uint32_t* __restrict__ cap, const uint64_t* __restrict__ base,
                                                         const float* __restrict__ ovals, const uint32_t* __restrict__ okeys,
                                                         uint32_t* __restrict__ keys, float* __restrict__ values,
                                                         int32_t* __restrict__ sizes) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long dyn64[];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = (int)(blockIdx.x * (blockDim.x >> 6) + wave);
    if (q >= nq) return;                                         // (no workgroup barrier below: waves run on their own)
    unsigned long long* hv = dyn64 + (size_t)wave * (R + 64);
    unsigned long long* buf = hv + R;
    const uint32_t n = min(count[q], cap[q]);
    const float* __restrict__ sv = ovals + base[q];
    const uint32_t* __restrict__ sk = okeys + base[q];
    const uint32_t uR = (uint32_t)R;
    for (uint32_t i = lane; i < uR; i += 64) hv[i] = (unsigned long long)__float_as_uint(FLT_MAX) << 32;
    wave_lds_sync();
    auto val_of = [](unsigned long long e) { return __uint_as_float((uint32_t)(e >> 32)); };
    auto push = [&](unsigned long long e) {
        const float value = val_of(e);
        if (!(value < val_of(hv[0]))) return;
        uint32_t i = 0;
        for (;;) {
            const uint32_t l = 2 * i + 1;
            if (l >= uR) break;
            unsigned long long ce = hv[l];
            uint32_t c = l;
            if (l + 1 < uR) {
                const unsigned long long re = hv[l + 1];
                if (val_of(re) > val_of(ce)) { ce = re; c = l + 1; }
            }
            if (val_of(ce) <= value) break;
            hv[i] = ce;
            i = c;
        }
        hv[i] = e;
    };
    float v = 0.0f;
    uint32_t k = 0;
    if (lane < n) { v = sv[lane]; k = sk[lane]; }
    for (uint32_t at = 0; at < n; at += 64) {
        const uint32_t m = min(64u, n - at);
        const float cv = v;
        const uint32_t ck = k;
        if (at + 64 < n && lane < n - (at + 64)) {               // the next 64 are on their way while lane 0 pushes these
            v = sv[at + 64 + lane];
            k = sk[at + 64 + lane];
        }
        const unsigned long long live = __ballot(lane < m && cv < val_of(hv[0]));
        if (live == 0) continue;
        buf[lane] = (unsigned long long)ck | ((unsigned long long)__float_as_uint(cv) << 32);
        wave_lds_sync();
        if (lane == 0)
            for (unsigned long long rest = live; rest; rest &= rest - 1) push(buf[__builtin_ctzll(rest)]);
        wave_lds_sync();
    }
    for (uint32_t i = lane; i < uR; i += 64) {
        const unsigned long long e = hv[i];
        keys[(size_t)q * R + i] = (uint32_t)e;
        values[(size_t)q * R + i] = val_of(e);
    }
    if (lane == 0) sizes[q] = R;
}

// Words from one device buffer to another by a kernel: a buffer of the caller's need not be known to this library's copy of
// the HIP runtime (a tensor of a framework that carries its own), and a memcpy on a pointer the runtime does not know treats it as host memory.
__global__ __launch_bounds__(kWG) void adc_copy_words_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * kWG + threadIdx.x; i < n; i += (size_t)gridDim.x * kWG) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------------
// Range search: the scan kernels above under bound[q] = radius[q] leave every kept row of query q in its
// region, in no order.  adc_range_sort_kernel: one workgroup per query sorts the region's (value, key) pairs ascending by the word
// order_key(value) << 32 | key and writes them densely behind the queries before it: entry out_base + sum_{j<q} stored_j + i of
// out_vals / out_keys (the offset is summed here, as adc_pack_kernel sums it: the host has the counts but uploads nothing).
//   n <= kRangeSortLds  a bitonic sort of the words in LDS;
//   longer segments     LSD radix passes of 8 bits over the 64 bits of the word through the global scratch tmp_a / tmp_b
//                       [base[q] + i], scattered tile by tile like adc_order_kernel's.  One sweep first ORs and ANDs all words: a
//                       digit in which OR and AND agree is the same in every entry — its histogram has one bin — and its pass, which
//                       would move nothing, is skipped; the last pass that runs writes (value, key) instead of the word.  Equal words
//                       are the same pair, so the result is a function of the multiset alone.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWG) void adc_range_sort_kernel(Emit emit, unsigned long long out_base, uint32_t* __restrict__ out_keys,
                                                             float* __restrict__ out_vals, unsigned long long* tmp_a,
                                                             unsigned long long* tmp_b) {
    __shared__ unsigned long long lkey[kRangeSortLds];
    __shared__ unsigned long long s_off, s_or, s_and;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        s_off = 0;
        s_or = 0;
        s_and = ~0ull;
    }
    __syncthreads();
    unsigned long long part = 0;
    for (uint32_t j = tid; j < q; j += kWG) part += min(emit.count[j], emit.cap[j]);
    if (part) atomicAdd(&s_off, part);
    __syncthreads();
    const uint32_t n = min(emit.count[q], emit.cap[q]);
    if (n == 0) return;
    const size_t region = emit.base[q];
    const float* __restrict__ vals = emit.vals + region;
    const uint32_t* __restrict__ keys = emit.keys + region;
    float* __restrict__ ov = out_vals + out_base + s_off;
    uint32_t* __restrict__ ok = out_keys + out_base + s_off;
    auto word = [&](uint32_t i) { return ((unsigned long long)order_key(vals[i]) << 32) | keys[i]; };

    if (n <= (uint32_t)kRangeSortLds) {
        uint32_t n2 = 1;
        while (n2 < n) n2 <<= 1;
        for (uint32_t i = tid; i < n2; i += kWG) lkey[i] = i < n ? word(i) : ~0ull;   // (~0 is the image of a NaN: no kept row has it)
        __syncthreads();
        for (uint32_t k = 2; k <= n2; k <<= 1)
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                for (uint32_t t = tid; t < n2 / 2; t += kWG) {
                    const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                    const unsigned long long a = lkey[i], b = lkey[p];
                    if ((a > b) == ((i & k) == 0)) { lkey[i] = b; lkey[p] = a; }
                }
                __syncthreads();
            }
        for (uint32_t i = tid; i < n; i += kWG) {
            const unsigned long long e = lkey[i];
            ov[i] = order_val((uint32_t)(e >> 32));
            ok[i] = (uint32_t)e;
        }
        return;
    }

    {                                                            // which digits differ anywhere
        unsigned long long o = 0, a = ~0ull;
        for (unsigned long long i = tid; i < n; i += kWG) {
            const unsigned long long e = word((uint32_t)i);
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
    if (active == 0) {                                           // every entry is the same pair
        for (unsigned long long i = tid; i < n; i += kWG) {
            ov[i] = vals[i];
            ok[i] = keys[i];
        }
        return;
    }

    uint32_t* hist = reinterpret_cast<uint32_t*>(lkey);          // [256] entries of the digit, then its running write position
    uint32_t* wcount = hist + 256;                               // [4][256] entries of the digit in each wave of the tile
    unsigned long long* ta = tmp_a + region;
    unsigned long long* tb = tmp_b + region;
    const uint32_t lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    int pass = 0;
    for (int digit = 0; digit < 8; ++digit) {
        if (!((active >> digit) & 1u)) continue;                 // (the same in every lane)
        const unsigned long long* src = (pass & 1) ? ta : tb;    // the first pass reads the region itself
        unsigned long long* dst = (pass & 1) ? tb : ta;
        const int shift = 8 * digit;
        const bool first = pass == 0, last = (active >> (digit + 1)) == 0;
        ++pass;
        auto entry = [&](uint32_t i) { return first ? word(i) : src[i]; };
        hist[tid] = 0;
        for (int w = 0; w < 4; ++w) wcount[w * 256 + tid] = 0;
        __syncthreads();
        for (unsigned long long i = tid; i < n; i += kWG) atomicAdd(&hist[(uint32_t)(entry((uint32_t)i) >> shift) & 255u], 1u);
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
        for (unsigned long long t0 = 0; t0 < n; t0 += kWG) {     // (64-bit: n may be within 256 of 2^32)
            const bool valid = t0 + tid < n;
            const uint32_t i = (uint32_t)(t0 + tid);
            const unsigned long long e = valid ? entry(i) : 0ull;
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
                if (last) {
                    ov[pos] = order_val((uint32_t)(e >> 32));
                    ok[pos] = (uint32_t)e;
                } else {
                    dst[pos] = e;
                }
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
}

// ---------------------------------------------------------------------------------------------
// Feeders: what nns_engine(_batch)::process_query does before query_scan (query_common.hpp:194-213, 283-297), for 256 or 65536
// centroids per sub-quantizer, and base_pq::encode_multiple_vectors (quantizers.hpp:222-245) for 256.
// Arithmetic entry for entry that of build_tables_kernel (csrc/qadc_kernels.hip) and of the host twin pq_bytes::tables /
// tables_blas (host/scanner_simple.hpp): residual q - coarse[assign]; OPQ rotation rotated[r] = sum_c x[c] rotation[r][c],
// one sequential sum in ascending c; direct form = direct_sqdist, expansion form = (||v||^2 + ||c||^2) + (-2 v.c) with the
// norms of expansion_sqnorm and one sequential dot (qadc_float_sum.h).  ||c||^2 comes from the caller, once per codebook set.
// ---------------------------------------------------------------------------------------------
template <int DS>
struct CentroidRow {   // DS = 8, 16, 32: the row in registers;  0: any sq_dim, read where it is used
    float v[DS];
    __device__ __forceinline__ void load(const float* __restrict__ row, int) {
#pragma unroll
        for (int i = 0; i < DS / 4; ++i) {
            const float4 t = reinterpret_cast<const float4*>(row)[i];
            v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
        }
    }
    __device__ __forceinline__ float operator[](int d) const { return v[d]; }
};
template <>
struct CentroidRow<0> {
    const float* __restrict__ p;
    __device__ __forceinline__ void load(const float* __restrict__ row, int) { p = row; }
    __device__ __forceinline__ float operator[](int d) const { return p[d]; }
};

// Grid (query, probe group, sub-quantizer slice x centroid slice).  A workgroup holds the residuals of `probes` probes of one
// query in LDS (only the components of its sub-quantizers m0 .. m0 + mper) and builds `cper` blocks of 256 centroids of each
// of them (one block is all there is of an 8-bit sub-quantizer; a 16-bit one has 256): lane c owns centroid block * 256 + c
// of the current sub-quantizer, keeps its row and walks the probes: every store instruction of the workgroup writes one
// contiguous 1 KiB of a table row.
// Dynamic LDS: res [probes][mper * ds] | vnorm [probes][mper] | (OPQ) whole un-rotated residuals [probes][dim].
template <int DS>
__global__ __launch_bounds__(kWG) void adc_tables_kernel(const float* __restrict__ queries, const float* __restrict__ coarse,
                                                         const int32_t* __restrict__ assign, const float* __restrict__ codebooks,
                                                         const float* __restrict__ cbnorm, const float* __restrict__ rotation,
                                                         int ma, int nsq, int centroids, int dim, int probes, int mper, int cper,
                                                         int expansion, int sum_mode, float* __restrict__ tables) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    const int ds = DS ? DS : dim / nsq;
    const int cslices = centroids / (256 * cper);
    const int qi = blockIdx.x, a0 = blockIdx.y * probes, m0 = (blockIdx.z / cslices) * mper, tid = threadIdx.x;
    const int c0 = (blockIdx.z % cslices) * cper * 256;
    const int na = min(probes, ma - a0);
    const int lo = m0 * ds, width = mper * ds;
    float* res = dyn;
    float* vnorm = res + probes * width;
    float* whole = vnorm + probes * mper;
    const float* __restrict__ q = queries + (size_t)qi * dim;
    if (!rotation) {
        for (int i = tid; i < na * width; i += kWG) {
            const int a = i / width, j = i - a * width;
            const float x = q[lo + j];
            res[i] = coarse ? x - coarse[(size_t)assign[(size_t)qi * ma + a0 + a] * dim + lo + j] : x;
        }
    } else {
        for (int i = tid; i < na * dim; i += kWG) {
            const int a = i / dim, d = i - a * dim;
            const float x = q[d];
            whole[i] = coarse ? x - coarse[(size_t)assign[(size_t)qi * ma + a0 + a] * dim + d] : x;
        }
        __syncthreads();
        // opq::rotate_multiple_vectors (quantizers.hpp:289-301): the rows this workgroup's sub-quantizers read
        for (int i = tid; i < na * width; i += kWG) {
            const int a = i / width, j = i - a * width;
            const float* __restrict__ row = rotation + (size_t)(lo + j) * dim;
            const float* x = whole + a * dim;
            float acc = 0.0f;
            for (int c = 0; c < dim; ++c) acc += x[c] * row[c];
            res[i] = acc;
        }
    }
    __syncthreads();
    if (expansion) {
        for (int i = tid; i < na * mper; i += kWG) vnorm[i] = expansion_sqnorm(res + (size_t)i * ds, ds, sum_mode);
        __syncthreads();
    }
    for (int mm = 0; mm < mper; ++mm) {
        const int m = m0 + mm;
        for (int cb = 0; cb < cper; ++cb) {
            const size_t c = (size_t)m * centroids + c0 + cb * 256 + tid;
            CentroidRow<DS> ce;
            ce.load(codebooks + c * ds, ds);
            const float cn = expansion ? cbnorm[c] : 0.0f;
            float* __restrict__ out = tables + ((size_t)qi * ma + a0) * nsq * centroids + c;
            for (int a = 0; a < na; ++a) {
                const float* r = res + a * width + mm * ds;
                float s;
                if (expansion) s = expansion_dist(r, ce, ds, vnorm[a * mper + mm], cn);
                else s = direct_sqdist(r, ce, ds, sum_mode);
                out[(size_t)a * nsq * centroids] = s;
            }
        }
    }
}

// encode_multiple_vectors for 8-bit sub-quantizers: per (vector, sub-quantizer) the 256 expansion distances pushed in centroid
// order into a kv_binheap of capacity 1 (find_k_neighbors with k = 1, neighbors.cpp:18-76), whose replace test AS COMPILED is
// !(s >= kept): the pick is 255 when distance 255 is NaN, else the first smallest distance among the centroids after the last
// NaN.  Lane c holds distance c, so every wave settles its 64 centroids by that rule — (value, index) keys, lanes up to its last
// NaN left out — and one thread per vector then walks the four waves in order: a wave with a NaN restarts the history, a wave
// whose lane 63 is NaN leaves a NaN kept, which the next wave's first centroid replaces whatever its distance.
// Dynamic LDS: wave keys [vper][4] u64 | wave flags [vper][4] | x [vper][dim] | ||x_m||^2 [vper][nsq] | codes [vper][nsq].
template <int DS>
__global__ __launch_bounds__(kWG) void adc_encode_kernel(const float* __restrict__ x, uint64_t n, int nsq, int dim,
                                                         const float* __restrict__ codebooks, const float* __restrict__ cbnorm,
                                                         int vper, int sum_mode, uint8_t* __restrict__ codes) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    const int ds = DS ? DS : dim / nsq;
    unsigned long long* wkey = reinterpret_cast<unsigned long long*>(dyn);
    uint32_t* wflag = reinterpret_cast<uint32_t*>(wkey + vper * 4);
    float* xs = reinterpret_cast<float*>(wflag + vper * 4);
    float* vnorm = xs + (size_t)vper * dim;
    uint8_t* picked = reinterpret_cast<uint8_t*>(vnorm + vper * nsq);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint64_t v0 = (uint64_t)blockIdx.x * vper; v0 < n; v0 += (uint64_t)gridDim.x * vper) {
        const int nv = (int)min((uint64_t)vper, n - v0);
        __syncthreads();                                          // (the last chunk's picks have been written out)
        for (int i = tid; i < nv * dim; i += kWG) xs[i] = x[v0 * dim + i];
        __syncthreads();
        for (int i = tid; i < nv * nsq; i += kWG) vnorm[i] = expansion_sqnorm(xs + (size_t)(i / nsq) * dim + (i % nsq) * ds, ds, sum_mode);
        __syncthreads();
        for (int m = 0; m < nsq; ++m) {
            CentroidRow<DS> ce;
            ce.load(codebooks + ((size_t)m * 256 + tid) * ds, ds);
            const float cn = cbnorm[m * 256 + tid];
            for (int v = 0; v < nv; ++v) {
                const float s = expansion_dist(xs + (size_t)v * dim + m * ds, ce, ds, vnorm[v * nsq + m], cn) + 0.0f;   // (-0 -> +0)
                const unsigned long long nans = __ballot(s != s);
                const int last_nan = nans ? 63 - __builtin_clzll(nans) : -1;
                unsigned long long key = lane > last_nan ? ((unsigned long long)order_key(s) << 32) | (uint32_t)tid : ~0ull;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const unsigned long long o = __shfl_xor(key, d);
                    key = o < key ? o : key;
                }
                if (lane == 0) {
                    wkey[v * 4 + wave] = key;
                    wflag[v * 4 + wave] = nans ? (last_nan == 63 ? 2u : 1u) : 0u;
                }
            }
            __syncthreads();
            if (tid < nv) {
                unsigned long long best = ~0ull;
                bool kept_nan = false;
                uint32_t nan_at = 0;
                for (int w = 0; w < 4; ++w) {
                    const unsigned long long k = wkey[tid * 4 + w];
                    const uint32_t f = wflag[tid * 4 + w];
                    if (f == 2u) { kept_nan = true; nan_at = 64u * w + 63u; }
                    else if (f == 1u || kept_nan) { best = k; kept_nan = false; }
                    else best = k < best ? k : best;
                }
                picked[tid * nsq + m] = (uint8_t)(kept_nan ? nan_at : (uint32_t)best);
            }
            __syncthreads();
        }
        for (int i = tid; i < nv * nsq; i += kWG) codes[v0 * nsq + i] = picked[i];
    }
}

// encode_multiple_vectors for 16-bit sub-quantizers: the same capacity-1 heap fed 65536 expansion distances in centroid order
// (256 blocks of BLOCK_NEIGHS; the heap is not reset between blocks).  The roles of adc_encode_kernel are swapped: a LANE owns
// vectors, not centroids.  Lane t keeps the sub-vectors of VL vectors of the current sub-quantizer in registers (DS 8 / 16: 4,
// DS 32 / 64: 2; DS 0 reads its one vector where it lies) and the workgroup sweeps the centroid rows, staged kEnc16Tile at a time in
// LDS, in ascending index: every lane reads the same row (a broadcast read: ds / 4 ds_read_b128 feed 2 * ds * VL VALU
// operations per lane), so a loaded row meets V = 256 VL vectors and a sub-quantizer's codebook is read once per V vectors.
// Because one lane sees all the distances of its vector in heap order, the pick IS the heap: kept starts as NaN (an empty heap
// takes its first push), and `if (!(s >= kept))` is the replace test as compiled — NaN distances, ties and -0 need no second
// look.  Pairs of vectors go through float2 arithmetic (v_pk_mul_f32 / v_pk_add_f32: every component rounds as the scalar
// instruction, unfused under -ffp-contract=off), entry for entry expansion_dist.
// Grid (x): vector tile fastest, then centroid slice, then sub-quantizer, so that workgroups resident together sweep the
// same rows.  A small call cuts the 65536 centroids into `slices` runs (launch_adc_encode16) to fill the chip; every
// (slice, sub-quantizer, vector) leaves its heap's state as distance bits << 32 | saw a NaN << 31 | centroid in `part`
// [slices][nsq][n], and adc_encode16_merge_kernel continues the heap over the slices.
// Dynamic LDS: rows [tile][ds] | ||c||^2 [tile].
typedef float float2v __attribute__((ext_vector_type(2)));

template <int DS>
__global__ __launch_bounds__(kWG) void adc_encode16_kernel(const float* __restrict__ x, uint32_t n, int nsq, int dim,
                                                           const float* __restrict__ codebooks, const float* __restrict__ cbnorm,
                                                           int slices, int tile, int sum_mode, unsigned long long* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    constexpr int VL = encode16_lane_vectors(DS);
    const int ds = DS ? DS : dim / nsq;
    const int tid = threadIdx.x;
    const uint32_t vtiles = (n + kWG * VL - 1) / (kWG * VL);
    const uint32_t vt = blockIdx.x % vtiles, rest = blockIdx.x / vtiles;
    const int slice = (int)(rest % (uint32_t)slices), m = (int)(rest / (uint32_t)slices);
    const int per = 65536 / slices, c_lo = slice * per;
    float* rows = dyn;
    float* norms = dyn + (size_t)tile * ds;
    const float* __restrict__ cb = codebooks + (size_t)m * 65536 * ds;

    // the lane's vectors: vt * 256 VL + j * 256 + tid.  A lane past the end computes on vector n - 1 and writes nothing.
    uint32_t vi[VL];
    const float* __restrict__ xp[VL];
    float vn[VL], kept[VL];
    uint32_t pick[VL];
    unsigned long long saw_nan[VL];                           // per wave: the lanes whose vector j met a NaN distance (a scalar OR per centroid)
    [[maybe_unused]] float xr[VL][DS ? DS : 1];
#pragma unroll
    for (int j = 0; j < VL; ++j) {
        vi[j] = vt * (uint32_t)(kWG * VL) + (uint32_t)(j * kWG + tid);
        xp[j] = x + (size_t)min(vi[j], n - 1) * dim + (size_t)m * ds;
        if constexpr (DS != 0) {
#pragma unroll
            for (int i = 0; i < DS / 4; ++i) {
                const float4 t = reinterpret_cast<const float4*>(xp[j])[i];
                xr[j][4 * i] = t.x; xr[j][4 * i + 1] = t.y; xr[j][4 * i + 2] = t.z; xr[j][4 * i + 3] = t.w;
            }
            vn[j] = expansion_sqnorm(xr[j], ds, sum_mode);
        } else {
            vn[j] = expansion_sqnorm(xp[j], ds, sum_mode);
        }
        kept[j] = __uint_as_float(0x7fc00000u);                   // the empty heap: its first push always enters
        pick[j] = 0;
        saw_nan[j] = 0;
    }

    for (int c0 = c_lo; c0 < c_lo + per; c0 += tile) {
        __syncthreads();                                          // (the last tile has been read)
        if constexpr (DS != 0) {
            const float4* src = reinterpret_cast<const float4*>(cb + (size_t)c0 * ds);
            for (int i = tid; i < tile * (DS / 4); i += kWG) reinterpret_cast<float4*>(rows)[i] = src[i];
        } else {
            for (int i = tid; i < tile * ds; i += kWG) rows[i] = cb[(size_t)c0 * ds + i];
        }
        for (int i = tid; i < tile; i += kWG) norms[i] = cbnorm[(size_t)m * 65536 + c0 + i];
        __syncthreads();
        for (int c = 0; c < tile; ++c) {
            const float cn = norms[c];
            const uint32_t at = (uint32_t)(c0 + c);
            if constexpr (DS != 0) {
                CentroidRow<DS> ce;
                ce.load(rows + c * DS, DS);
#pragma unroll
                for (int p = 0; p < VL / 2; ++p) {                // vectors 2p and 2p + 1, one component each
                    float2v dot = {0.0f, 0.0f};
#pragma unroll
                    for (int d = 0; d < DS; ++d) {
                        const float2v xv = {xr[2 * p][d], xr[2 * p + 1][d]};
                        dot = dot + xv * ce[d];
                    }
                    const float2v base = {vn[2 * p] + cn, vn[2 * p + 1] + cn};
                    const float2v s = base + (-2.0f * dot);
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const bool enter = !(s[h] >= kept[2 * p + h]);
                        saw_nan[2 * p + h] |= __ballot(s[h] != s[h]);
                        pick[2 * p + h] = enter ? at : pick[2 * p + h];
                        kept[2 * p + h] = enter ? s[h] : kept[2 * p + h];
                    }
                }
            } else {
                const float s = expansion_dist(xp[0], rows + c * ds, ds, vn[0], cn);
                saw_nan[0] |= __ballot(s != s);
                if (!(s >= kept[0])) {
                    pick[0] = at;
                    kept[0] = s;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < VL; ++j)
        if (vi[j] < n)
            part[((size_t)slice * nsq + m) * n + vi[j]] = ((unsigned long long)__float_as_uint(kept[j]) << 32) | (((saw_nan[j] >> (tid & 63)) & 1) ? 0x80000000u : 0u) | pick[j];
}

// The heap carried over the slices of one (vector, sub-quantizer): a slice that saw a NaN has forgotten everything before it,
// a kept NaN is replaced by whatever comes next, and otherwise a later slice's first smallest distance enters only when it is
// strictly smaller.  One thread per (vector, sub-quantizer); codes [n][nsq] uint16.
__global__ __launch_bounds__(kWG) void adc_encode16_merge_kernel(const unsigned long long* __restrict__ part, uint32_t n, int nsq,
                                                                 int slices, uint16_t* __restrict__ codes) {
    const size_t i = (size_t)blockIdx.x * kWG + threadIdx.x;
    if (i >= (size_t)n * nsq) return;
    const uint32_t v = (uint32_t)(i / nsq);
    const int m = (int)(i % nsq);
    float kept = __uint_as_float(0x7fc00000u);
    uint32_t pick = 0;
    for (int sl = 0; sl < slices; ++sl) {
        const unsigned long long e = part[((size_t)sl * nsq + m) * n + v];
        const float s = __uint_as_float((uint32_t)(e >> 32));
        if (((uint32_t)e & 0x80000000u) || !(s >= kept)) {
            kept = s;
            pick = (uint32_t)e & 0xffffu;
        }
    }
    codes[i] = (uint16_t)pick;
}

// ---------------------------------------------------------------------------------------------
// db_add: index_db::add_vectors' dispatch of the encoded rows to their partitions
// (databases.hpp:291-297), and the move of the database into a larger layout.
//   adc_add_count_kernel    vectors per partition (atomics only count: no position depends on their order);
//   adc_add_hist_kernel     digit histogram of every tile of kAddTile entries of one radix pass;
//   adc_add_scan_kernel     the histograms turned into write positions, digit-major then tile order (one workgroup);
//   adc_add_scatter_kernel  the stable scatter of the pass, tile by tile as adc_order_kernel's: rank among the equal digits
//                           of the wave by ballots, of the waves before through LDS counts.  The last pass writes the code row
//                           (one dword, dwordx2 or dwordx4 store) and the label instead of the permutation: the caller's
//                           row_labels[i] where given, else first_label + i;
//   adc_move_kernel         the relocation, one thread per (partition, 16-byte word) and per (partition, label).
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kAddCountLds = 8192;   // partitions + 1 the count kernel privatises in LDS; more go to global atomics

__global__ __launch_bounds__(kWG) void adc_add_count_kernel(const int32_t* __restrict__ assign, uint32_t n, uint32_t K,
                                                            uint32_t* __restrict__ count, uint32_t lds_bins) {
    extern __shared__ uint32_t add_bins[];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < lds_bins; i += kWG) add_bins[i] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + tid; i < n; i += (uint64_t)gridDim.x * kWG) {
        const uint32_t a = (uint32_t)assign[i];                  // (a negative assignment is a large one)
        const uint32_t b = a < K ? a : K;
        if (lds_bins) atomicAdd(&add_bins[b], 1u);
        else atomicAdd(&count[b], 1u);
    }
    __syncthreads();
    for (uint32_t i = tid; i < lds_bins; i += kWG)
        if (add_bins[i]) atomicAdd(&count[i], add_bins[i]);
}

// entry `pos` of a pass: the vector it stands for (pass 0 reads the vectors in input order)
__device__ __forceinline__ uint32_t add_entry(const uint32_t* __restrict__ perm, uint32_t pos) { return perm ? perm[pos] : pos; }

__global__ __launch_bounds__(kWG) void adc_add_hist_kernel(const int32_t* __restrict__ assign, const uint32_t* __restrict__ perm,
                                                           uint32_t n, int shift, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    const uint32_t tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    for (int r = 0; r < kAddTile / kWG; ++r) {
        const uint64_t pos = (uint64_t)blockIdx.x * kAddTile + (uint32_t)r * kWG + tid;
        if (pos < n) atomicAdd(&h[((uint32_t)assign[add_entry(perm, (uint32_t)pos)] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)blockIdx.x * 256 + tid] = h[tid];
}

// hist [tiles][256] counts -> the first write position of (tile, digit): the entries of smaller digits, then those of the same
// digit in earlier tiles.  Thread d owns digit d.
__global__ __launch_bounds__(kWG) void adc_add_scan_kernel(uint32_t* __restrict__ hist, uint32_t tiles) {
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

template <int BYTES>
__global__ __launch_bounds__(kWG) void adc_add_scatter_kernel(const int32_t* __restrict__ assign, const uint32_t* __restrict__ perm,
                                                              uint32_t n, uint32_t K, int shift, const uint32_t* __restrict__ hist,
                                                              uint32_t* __restrict__ perm_out, bool last,
                                                              const CodeWords<BYTES>* __restrict__ rows, uint32_t first_label,
                                                              const uint32_t* __restrict__ row_labels, AddDst dst) {
    __shared__ uint32_t run[256];                                // write position of the next entry of each digit
    __shared__ uint32_t wcount[4 * 256];                         // entries of the digit in each wave of the round
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    run[tid] = hist[(size_t)blockIdx.x * 256 + tid];
    for (int w = 0; w < 4; ++w) wcount[w * 256 + tid] = 0;
    __syncthreads();
    for (int r = 0; r < kAddTile / kWG; ++r) {
        const uint64_t p0 = (uint64_t)blockIdx.x * kAddTile + (uint32_t)r * kWG;
        if (p0 >= n) break;                                      // (the same for every thread of the workgroup)
        const bool valid = p0 + tid < n;
        const uint32_t i = valid ? add_entry(perm, (uint32_t)(p0 + tid)) : 0u;
        const uint32_t a = valid ? (uint32_t)assign[i] : 0u;
        const uint32_t d = (a >> shift) & 255u;
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
            if (!last) {
                perm_out[pos] = i;
            } else if (a < K) {
                const uint32_t row = dst.base[a] + pos;          // (modulo 2^32: base = size - entries of the partitions below)
                *reinterpret_cast<CodeWords<BYTES>*>(dst.codes + dst.off[a] + (uint64_t)row * BYTES) = rows[i];
                if (dst.labels) dst.labels[dst.lab_off[a] + row] = row_labels ? row_labels[i] : first_label + i;
            }
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

__global__ __launch_bounds__(kWG) void adc_move_kernel(int parts, int code_bytes, const uint32_t* __restrict__ sizes,
                                                       const uint8_t* __restrict__ src_codes, const uint64_t* __restrict__ src_off,
                                                       const uint32_t* __restrict__ src_labels, const uint64_t* __restrict__ src_lab_off,
                                                       uint8_t* __restrict__ dst_codes, const uint64_t* __restrict__ dst_off,
                                                       uint32_t* __restrict__ dst_labels, const uint64_t* __restrict__ dst_lab_off) {
    const uint64_t t0 = (uint64_t)blockIdx.x * kWG + threadIdx.x, step = (uint64_t)gridDim.x * kWG;
    for (int p = (int)blockIdx.y; p < parts; p += (int)gridDim.y) {
        const uint64_t rows = sizes[p];
        if (rows == 0) continue;
        const uint64_t words = (rows * (uint64_t)code_bytes + 15) / 16;   // (both regions hold whole 16-byte words)
        const uint4* __restrict__ s = reinterpret_cast<const uint4*>(src_codes + src_off[p]);
        uint4* __restrict__ d = reinterpret_cast<uint4*>(dst_codes + dst_off[p]);
        for (uint64_t w = t0; w < words; w += step) d[w] = s[w];
        if (src_labels && dst_labels) {
            const uint32_t* __restrict__ sl = src_labels + src_lab_off[p];
            uint32_t* __restrict__ dl = dst_labels + dst_lab_off[p];
            for (uint64_t j = t0; j < rows; j += step) dl[j] = sl[j];
        }
    }
}

// ---- the growing storage of the 4-bit index ----
// The gather-move of a relocation: partition p = blockIdx.y, y-strided, goes from wherever it lies (an allocation of its own on the
// consolidating call, the old arena later; never the destination buffer) to its region of the new arena — whole 16-byte words, the
// odd half of the last word of an 8-byte-row partition as one dwordx2, labels as dwords — and bytes [n * cs, align16(n * cs) + 64)
// behind the last row are zeroed, for empty partitions too (host/index_append_plan.hpp has why).
__global__ __launch_bounds__(kWG) void index_move_kernel(const IndexMove* __restrict__ moves, int parts, int code_bytes) {
    const uint64_t t0 = (uint64_t)blockIdx.x * kWG + threadIdx.x, step = (uint64_t)gridDim.x * kWG;
    for (int p = (int)blockIdx.y; p < parts; p += (int)gridDim.y) {
        const IndexMove m = moves[p];
        const uint64_t bytes = (uint64_t)m.n * (uint64_t)code_bytes;      // (a multiple of 8: rows are 8 or 16 bytes)
        const uint64_t words = bytes / 16;
        const uint4* __restrict__ s = reinterpret_cast<const uint4*>(m.src_codes);
        uint4* __restrict__ d = reinterpret_cast<uint4*>(m.dst_codes);
        for (uint64_t w = t0; w < words; w += step) d[w] = s[w];
        if (t0 < 10) {                                           // the tail: the odd half word, then up to 9 dwordx2 of zeroes
            const uint64_t u = words * 2 + t0, last = index_padded_end(bytes) / 8;
            if (u < last) {
                uint2 v = make_uint2(0u, 0u);
                if (u * 8 < bytes) v = reinterpret_cast<const uint2*>(m.src_codes)[u];
                reinterpret_cast<uint2*>(m.dst_codes)[u] = v;
            }
        }
        if (m.src_labels && m.dst_labels)
            for (uint64_t j = t0; j < m.n; j += step) m.dst_labels[j] = m.src_labels[j];
    }
}

// Bytes [n * cs, align16(n * cs) + 64) behind the last row of every partition zeroed where the partitions lie now: 16 threads a
// partition, 9 of them storing one dwordx2 each.  sizes [parts] rows held; off [parts] as AddDst's.
__global__ __launch_bounds__(kWG) void index_zero_tails_kernel(uint8_t* __restrict__ codes, const uint64_t* __restrict__ off,
                                                               const uint32_t* __restrict__ sizes, uint32_t parts, int code_bytes) {
    const uint64_t t = (uint64_t)blockIdx.x * kWG + threadIdx.x;
    const uint64_t p = t / 16, j = t % 16;
    if (p >= parts) return;
    const uint64_t bytes = (uint64_t)sizes[p] * (uint64_t)code_bytes;
    const uint64_t u = bytes / 8 + j, last = index_padded_end(bytes) / 8;
    if (u < last) reinterpret_cast<uint2*>(codes + off[p])[u] = make_uint2(0u, 0u);
}

__global__ __launch_bounds__(kWG) void adc_fill_words_kernel(uint32_t* __restrict__ dst, size_t n, uint32_t value) {
    for (size_t i = (size_t)blockIdx.x * kWG + threadIdx.x; i < n; i += (size_t)gridDim.x * kWG) dst[i] = value;
}

// ---------------------------------------------------------------------------------------------
// Remove by label: the rows whose label is in the caller's list leave their partitions, the others
// keep their order.
//   remove_minmax_kernel   the smallest and largest label of a list that lies in device memory (reduced in the wave, then across
//                          the waves through LDS: one atomicMin and one atomicMax per workgroup);
//   remove_mark_kernel     bit (label - lo) of the bitmap set for every label of the list (atomicOr: duplicates set it twice);
//   remove_count_kernel    per partition the rows whose label is marked and the first tile that holds one — labels only, one
//                          atomicAdd and one atomicMin per (partition, tile) that was hit (atomics only count: no position
//                          depends on their order);
//   remove_compact_kernel  one workgroup per touched partition walks it front to back and moves the kept rows to the front.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWG) void remove_minmax_kernel(const uint32_t* __restrict__ list, uint64_t count, uint32_t* __restrict__ lohi) {
    __shared__ uint32_t wlo[kWG / 64], whi[kWG / 64];
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x; i < count; i += (uint64_t)gridDim.x * kWG) {
        const uint32_t l = list[i];
        lo = min(lo, l);
        hi = max(hi, l);
    }
    for (int d = 32; d >= 1; d >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, d));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, d));
    }
    if ((threadIdx.x & 63) == 0) {
        wlo[threadIdx.x >> 6] = lo;
        whi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWG / 64; ++w) {
            lo = min(lo, wlo[w]);
            hi = max(hi, whi[w]);
        }
        atomicMin(&lohi[0], lo);
        atomicMax(&lohi[1], hi);
    }
}

__global__ __launch_bounds__(kWG) void remove_mark_kernel(const uint32_t* __restrict__ list, uint64_t count, uint32_t lo,
                                                          uint32_t* __restrict__ bitmap) {
    for (uint64_t i = (uint64_t)blockIdx.x * kWG + threadIdx.x; i < count; i += (uint64_t)gridDim.x * kWG) {
        const uint32_t d = list[i] - lo;
        atomicOr(&bitmap[d >> 5], 1u << (d & 31u));
    }
}

// (remove_word / remove_marked, the label's bit: beside the scan kernel, which tests keys with them too)

// Partition p = blockIdx.y, y-strided; its tiles of kRemoveTile rows x-strided over grid.x; a thread tests one bit a round.
__global__ __launch_bounds__(kWG) void remove_count_kernel(const RemoveSrc* __restrict__ src, int parts, const uint32_t* __restrict__ bitmap,
                                                           uint32_t lo, uint32_t last, uint32_t* __restrict__ hits, uint32_t* __restrict__ first) {
    __shared__ uint32_t wsum[kWG / 64];
    const uint32_t tid = threadIdx.x;
    for (int p = (int)blockIdx.y; p < parts; p += (int)gridDim.y) {
        const RemoveSrc m = src[p];
        const uint64_t tiles = ((uint64_t)m.n + kRemoveTile - 1) / kRemoveTile;
        for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {          // (the same trip count for every thread of the workgroup)
            uint32_t c = 0;                                                  // rows of the tile that go, seen by this wave
#pragma unroll 4
            for (int r = 0; r < kRemoveTile / kWG; ++r) {
                const uint64_t row = t * kRemoveTile + (uint32_t)r * kWG + tid;
                const uint32_t label = row < m.n ? m.labels[row] : 0u;
                const bool hit = row < m.n && remove_marked(remove_word(bitmap, lo, last, label), lo, last, label);
                c += (uint32_t)__popcll(__ballot(hit));
            }
            if ((tid & 63) == 0) wsum[tid >> 6] = c;
            __syncthreads();
            if (tid == 0) {
                uint32_t sum = 0;
                for (int w = 0; w < kWG / 64; ++w) sum += wsum[w];
                if (sum) {
                    atomicAdd(&hits[p], sum);
                    atomicMin(&first[p], (uint32_t)t);
                }
            }
            __syncthreads();
        }
    }
}

template <int BYTES> struct RowWord;                            // a code row as one dword, dwordx2 or dwordx4 register value
template <> struct RowWord<4> { using type = uint32_t; };
template <> struct RowWord<8> { typedef uint32_t type __attribute__((ext_vector_type(2))); };
template <> struct RowWord<16> { typedef uint32_t type __attribute__((ext_vector_type(4))); };

// One workgroup of kRemoveWG threads per touched partition.  An iteration takes one tile: every thread loads the labels and code
// words of its kRemoveRows rows (row = tile + j * kRemoveWG + thread, so a wave's loads are contiguous) into registers and tests
// their bits; the rank of a kept row among the kept rows of the tile is its rank in the wave's ballot (mbcnt) plus the kept rows
// of the (j, wave) pairs before it — kRemoveRows * 16 = 64 counts in LDS, one per lane, summed by every wave for itself — plus the
// write position w the tiles before left.  Only behind the __syncthreads() that follows the loads are rows stored, to [w, w + kept).
//
// Why in place is safe: w <= the tile's first row, so the stores of an iteration fall inside rows this
// workgroup has loaded — earlier tiles, and this tile, whose loads the barrier has completed; the next tile's loads touch rows no
// store of this iteration reaches; no workgroup reads or writes another partition's region.  The counts are double-buffered: a wave
// that runs ahead into the next iteration writes the other half.
template <int BYTES>
__global__ __launch_bounds__(kRemoveWG) void remove_compact_kernel(const RemovePart* __restrict__ parts, const uint32_t* __restrict__ bitmap,
                                                                   uint32_t lo, uint32_t last) {
    static_assert(kRemoveRows * (kRemoveWG / 64) == 64, "one lane per (row slot, wave) count");
    __shared__ uint32_t wcount[2][64];
    const RemovePart m = parts[blockIdx.x];
    using Row = typename RowWord<BYTES>::type;
    Row* rows = reinterpret_cast<Row*>(m.codes);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    uint32_t w = m.first_tile * (uint32_t)kRemoveTile;                      // the rows before the first tile stay where they are
    int buf = 0;
    for (uint64_t t0 = (uint64_t)m.first_tile * kRemoveTile; t0 < m.n; t0 += kRemoveTile, buf ^= 1) {
        Row c[kRemoveRows];
        uint32_t l[kRemoveRows], word[kRemoveRows], rank[kRemoveRows];
        bool keep[kRemoveRows];
#pragma unroll
        for (int j = 0; j < kRemoveRows; ++j) {
            const uint64_t r = t0 + (uint32_t)j * kRemoveWG + tid;
            const uint64_t in = r < m.n ? r : m.n - 1;                       // (past the end: the last row again, never kept)
            l[j] = m.labels[in];
            c[j] = rows[in];
        }
#pragma unroll
        for (int j = 0; j < kRemoveRows; ++j) word[j] = remove_word(bitmap, lo, last, l[j]);
#pragma unroll
        for (int j = 0; j < kRemoveRows; ++j) {
            const uint64_t r = t0 + (uint32_t)j * kRemoveWG + tid;
            keep[j] = r < m.n && !remove_marked(word[j], lo, last, l[j]);
            const unsigned long long kept = __ballot(keep[j]);
            rank[j] = (uint32_t)__popcll(kept & below);
            if (lane == 0) wcount[buf][j * (kRemoveWG / 64) + wave] = (uint32_t)__popcll(kept);
        }
        __syncthreads();
        uint32_t incl = wcount[buf][lane];                                   // inclusive sum of the 64 counts, in every wave
        const uint32_t own = incl;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= (uint32_t)d) incl += up;
        }
        const uint32_t excl = incl - own;
        const uint32_t total = (uint32_t)__shfl((int)incl, 63);
#pragma unroll
        for (int j = 0; j < kRemoveRows; ++j) {
            const uint32_t before = (uint32_t)__shfl((int)excl, j * (kRemoveWG / 64) + (int)wave);
            const uint64_t r = t0 + (uint32_t)j * kRemoveWG + tid;
            const uint32_t dst = w + before + rank[j];
            if (keep[j] && dst != r) {                                       // (a row in front of the first removed one stays)
                rows[dst] = c[j];
                m.labels[dst] = l[j];
            }
        }
        w += total;
    }
    if (tid * 8u < m.zero_bytes)                                             // the zero tail behind the new last row: dwordx2 each
        *reinterpret_cast<uint2*>(m.codes + (uint64_t)w * BYTES + tid * 8u) = make_uint2(0u, 0u);
}

}  // namespace

hipError_t launch_adc_scan(const ScanDb& db, int sum_mode, const Item* items, uint32_t first, uint32_t n_items, const int32_t* assign,
                           int ma, const float* tables, const float* bound, Emit emit, hipStream_t s) {
    if (n_items == 0) return hipSuccess;
    const auto scan = [&](auto code, auto src) {
        if (db.qfilters) {        // the call carries a filter of a query (the *_filtered calls): the per-query instantiation
            const auto kernel = sum_mode == 0 ? adc_scan_qfiltered_kernel<decltype(code), 0, decltype(src)>
                                              : adc_scan_qfiltered_kernel<decltype(code), 1, decltype(src)>;
            hipLaunchKernelGGL(kernel, dim3(n_items), dim3(kWG), 0, s, items, first, src, assign, ma, tables, bound, emit, db.filter, db.qfilters);
            return hipGetLastError();
        }
        if (db.filter.bitmap) {   // the index has a filter (qadc_adc_index_set_filter): the filtered instantiation
            const auto kernel = sum_mode == 0 ? adc_scan_filtered_kernel<decltype(code), 0, decltype(src)>
                                              : adc_scan_filtered_kernel<decltype(code), 1, decltype(src)>;
            hipLaunchKernelGGL(kernel, dim3(n_items), dim3(kWG), 0, s, items, first, src, assign, ma, tables, bound, emit, db.filter);
            return hipGetLastError();
        }
        const auto kernel = sum_mode == 0 ? adc_scan_kernel<decltype(code), 0, decltype(src)> : adc_scan_kernel<decltype(code), 1, decltype(src)>;
        hipLaunchKernelGGL(kernel, dim3(n_items), dim3(kWG), 0, s, items, first, src, assign, ma, tables, bound, emit);
        return hipGetLastError();
    };
    if (db.centroids == 256 && db.nsq == 4) return scan(ByteCodes<4>{}, db.bytes);
    if (db.centroids == 256 && db.nsq == 8) return scan(ByteCodes<8>{}, db.bytes);
    if (db.centroids == 256 && db.nsq == 16) return scan(ByteCodes<16>{}, db.bytes);
    if (db.centroids == 16 && db.nsq == 16) return scan(NibbleCodes<16>{}, db.parts);
    if (db.centroids == 16 && db.nsq == 32) return scan(NibbleCodes<32>{}, db.parts);
    if (db.centroids == 65536 && db.nsq == 2) return scan(WordCodes<2>{}, db.bytes);
    if (db.centroids == 65536 && db.nsq == 4) return scan(WordCodes<4>{}, db.bytes);
    if (db.centroids == 65536 && db.nsq == 8) return scan(WordCodes<8>{}, db.bytes);
    return hipErrorInvalidValue;
}

hipError_t launch_adc_select(int nq, int R, Emit emit, float* bound, hipStream_t s) {
    hipLaunchKernelGGL(adc_select_kernel, dim3(nq), dim3(kWG), 0, s, R, emit, bound);
    return hipGetLastError();
}

hipError_t launch_adc_pack(int nq, Emit emit, uint32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(adc_pack_kernel, dim3(nq), dim3(kWG), 0, s, emit, out);
    return hipGetLastError();
}

hipError_t launch_adc_order(int nq, Emit emit, int bits, float* ovals, uint32_t* okeys, uint64_t* tmp_a, uint64_t* tmp_b, hipStream_t s) {
    hipLaunchKernelGGL(adc_order_kernel, dim3(nq), dim3(kWG), 0, s, emit, bits, ovals, okeys,
                       reinterpret_cast<unsigned long long*>(tmp_a), reinterpret_cast<unsigned long long*>(tmp_b));
    return hipGetLastError();
}

hipError_t launch_adc_replay(int nq, int R, Emit emit, const float* ovals, const uint32_t* okeys, uint32_t* keys, float* values,
                             int32_t* sizes, hipStream_t s) {
    if (R < 1 || R > kAdcReplayMaxR) return hipErrorInvalidValue;
    const size_t per_wave = (size_t)(R + 64) * 8;                // heap + stage of one query
    const int waves = (int)std::max<size_t>(1, std::min<size_t>(kWG / 64, (60 * 1024) / per_wave));
    hipLaunchKernelGGL(adc_replay_kernel, dim3((nq + waves - 1) / waves), dim3(64 * waves), waves * per_wave, s, nq, R, emit.count,
                       emit.cap, emit.base, ovals, okeys, keys, values, sizes);
    return hipGetLastError();
}

hipError_t launch_adc_range_sort(int nq, Emit emit, uint64_t out_base, uint32_t* out_keys, float* out_vals, uint64_t* tmp_a, uint64_t* tmp_b,
                                 hipStream_t s) {
    hipLaunchKernelGGL(adc_range_sort_kernel, dim3(nq), dim3(kWG), 0, s, emit, (unsigned long long)out_base, out_keys, out_vals,
                       reinterpret_cast<unsigned long long*>(tmp_a), reinterpret_cast<unsigned long long*>(tmp_b));
    return hipGetLastError();
}

hipError_t launch_adc_copy_words(const void* src, void* dst, size_t words, hipStream_t s) {
    if (words == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((words + kWG - 1) / kWG, 4096);
    hipLaunchKernelGGL(adc_copy_words_kernel, dim3(grid), dim3(kWG), 0, s, static_cast<const uint32_t*>(src), static_cast<uint32_t*>(dst), words);
    return hipGetLastError();
}

static_assert(kAdcPlanMaxDim == kAdcMaxDim, "host/adc_tables_plan.hpp plans for the dimensions the feeders take");

hipError_t launch_adc_tables(const float* d_queries, const float* d_coarse, const int32_t* d_assign, const float* d_codebooks,
                             const float* d_cbnorm, const float* d_rotation, int nq, int ma, int nsq, int centroids, int dim,
                             int expansion, int sum_mode, float* d_tables, hipStream_t s) {
    if (nq <= 0 || ma <= 0) return hipSuccess;
    AdcTablesPlan p;                                             // host/adc_tables_plan.hpp: the whole geometry
    if (!adc_tables_plan(nq, ma, nsq, centroids, dim, d_rotation != nullptr, &p)) return hipErrorInvalidValue;
    const dim3 grid(p.grid_x, p.grid_y, p.grid_z);
#define QADC_AT(DS) hipLaunchKernelGGL((adc_tables_kernel<DS>), grid, dim3(kWG), p.lds_bytes, s, d_queries, d_coarse, d_assign, d_codebooks, \
                                       d_cbnorm, d_rotation, ma, nsq, centroids, dim, p.probes, p.mper, p.cper, expansion, sum_mode, d_tables)
    if (p.DS == 8) QADC_AT(8);
    else if (p.DS == 16) QADC_AT(16);
    else if (p.DS == 32) QADC_AT(32);
    else QADC_AT(0);
#undef QADC_AT
    return hipGetLastError();
}

hipError_t launch_adc_encode(const float* d_x, uint64_t n, int nsq, int dim, const float* d_codebooks, const float* d_cbnorm,
                             int sum_mode, uint8_t* d_codes, hipStream_t s) {
    if (n == 0) return hipSuccess;
    AdcEncodePlan p;
    if (!adc_encode_plan(n, nsq, dim, &p)) return hipErrorInvalidValue;
#define QADC_AE(DS) hipLaunchKernelGGL((adc_encode_kernel<DS>), dim3(p.grid), dim3(kWG), p.lds_bytes, s, d_x, n, nsq, dim, d_codebooks, d_cbnorm, \
                                       p.vper, sum_mode, d_codes)
    if (p.DS == 8) QADC_AE(8);
    else if (p.DS == 16) QADC_AE(16);
    else if (p.DS == 32) QADC_AE(32);
    else QADC_AE(0);
#undef QADC_AE
    return hipGetLastError();
}

int encode16_slices(uint32_t n, int nsq, int ds) {
    const int lane_vectors = encode16_lane_vectors(encode16_register_row(ds));
    const uint64_t vtiles = ((uint64_t)n + kWG * lane_vectors - 1) / (kWG * lane_vectors);
    int slices = 1;
    while (slices < 65536 / kEnc16MinSlice && vtiles * nsq * slices < 512) slices *= 2;
    return slices;
}

hipError_t launch_adc_encode16(const float* d_x, uint32_t n, int nsq, int dim, const float* d_codebooks, const float* d_cbnorm,
                               int sum_mode, unsigned long long* d_part, uint16_t* d_codes, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (dim <= 0 || dim > kAdcMaxDim || dim % nsq != 0) return hipErrorInvalidValue;
    const int ds = dim / nsq;
    const int DS = encode16_register_row(ds);
    const int lane_vectors = encode16_lane_vectors(DS);
    const int slices = encode16_slices(n, nsq, ds);
    // centroid rows per LDS tile: kEnc16Tile, fewer (a power of two) where the rows are long: at most 32 KiB of rows
    int tile = kEnc16Tile;
    while (tile > 1 && (size_t)tile * ds * 4 > 32 * 1024) tile /= 2;
    const size_t lds = (size_t)tile * (ds + 1) * 4;
    const uint64_t vtiles = ((uint64_t)n + kWG * lane_vectors - 1) / (kWG * lane_vectors);
    const dim3 grid((unsigned)(vtiles * slices * nsq));
#define QADC_AE16(D) hipLaunchKernelGGL((adc_encode16_kernel<D>), grid, dim3(kWG), lds, s, d_x, n, nsq, dim, d_codebooks, d_cbnorm, \
                                        slices, tile, sum_mode, d_part)
    if (DS == 8) QADC_AE16(8);
    else if (DS == 16) QADC_AE16(16);
    else if (DS == 32) QADC_AE16(32);
    else if (DS == 64) QADC_AE16(64);   // 2x16 at 128 dimensions
    else QADC_AE16(0);
#undef QADC_AE16
    if (hipError_t e = hipGetLastError()) return e;
    const size_t total = (size_t)n * nsq;
    hipLaunchKernelGGL(adc_encode16_merge_kernel, dim3((unsigned)((total + kWG - 1) / kWG)), dim3(kWG), 0, s, d_part, n, nsq, slices, d_codes);
    return hipGetLastError();
}

hipError_t launch_adc_add_count(const int32_t* d_assign, uint32_t n, uint32_t K, uint32_t* d_count, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t lds_bins = K + 1 <= kAddCountLds ? K + 1 : 0;
    const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)n + 4 * kWG - 1) / (4 * kWG), 1024);
    hipLaunchKernelGGL(adc_add_count_kernel, dim3(grid), dim3(kWG), lds_bins * sizeof(uint32_t), s, d_assign, n, K, d_count, lds_bins);
    return hipGetLastError();
}

hipError_t launch_adc_add_scatter(const int32_t* d_assign, uint32_t n, uint32_t K, int code_bytes, const uint8_t* d_rows,
                                  uint32_t first_label, const uint32_t* d_row_labels, AddDst dst, uint32_t* d_hist, uint32_t* d_perm_a,
                                  uint32_t* d_perm_b, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (K == 0 || (code_bytes != 4 && code_bytes != 8 && code_bytes != 16)) return hipErrorInvalidValue;
    int bits = 0;
    while (bits < 32 && ((K - 1) >> bits)) ++bits;
    const int passes = std::max(1, (bits + 7) / 8);
    const uint32_t tiles = (uint32_t)(((uint64_t)n + kAddTile - 1) / kAddTile);
    for (int pass = 0; pass < passes; ++pass) {
        const uint32_t* in = pass == 0 ? nullptr : (pass & 1) ? d_perm_a : d_perm_b;
        uint32_t* out = (pass & 1) ? d_perm_b : d_perm_a;
        const bool last = pass + 1 == passes;
        const int shift = 8 * pass;
        hipLaunchKernelGGL(adc_add_hist_kernel, dim3(tiles), dim3(kWG), 0, s, d_assign, in, n, shift, d_hist);
        hipLaunchKernelGGL(adc_add_scan_kernel, dim3(1), dim3(kWG), 0, s, d_hist, tiles);
#define QADC_AS(B) hipLaunchKernelGGL((adc_add_scatter_kernel<B>), dim3(tiles), dim3(kWG), 0, s, d_assign, in, n, K, shift, d_hist, out, last, \
                                      reinterpret_cast<const CodeWords<B>*>(d_rows), first_label, d_row_labels, dst)
        if (code_bytes == 4) QADC_AS(4);
        else if (code_bytes == 8) QADC_AS(8);
        else QADC_AS(16);
#undef QADC_AS
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

hipError_t launch_adc_move_partitions(int parts, int code_bytes, const uint32_t* d_sizes, uint32_t max_size, const uint8_t* src_codes,
                                      const uint64_t* src_off, const uint32_t* src_labels, const uint64_t* src_lab_off, uint8_t* dst_codes,
                                      const uint64_t* dst_off, uint32_t* dst_labels, const uint64_t* dst_lab_off, hipStream_t s) {
    if (parts <= 0 || max_size == 0) return hipSuccess;
    // grid.y walks the partitions, grid.x the words of the largest one (4 a thread), about 65536 workgroups at most
    const unsigned gy = (unsigned)std::min(parts, 65535);
    const uint64_t threads = std::max<uint64_t>(((uint64_t)max_size * code_bytes + 15) / 16, max_size);
    const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((threads + 4 * kWG - 1) / (4 * kWG), std::max(1u, 65536u / gy)));
    hipLaunchKernelGGL(adc_move_kernel, dim3(gx, gy), dim3(kWG), 0, s, parts, code_bytes, d_sizes, src_codes, src_off, src_labels, src_lab_off,
                       dst_codes, dst_off, dst_labels, dst_lab_off);
    return hipGetLastError();
}

hipError_t launch_adc_fill_words(void* dst, size_t words, uint32_t value, hipStream_t s) {
    if (words == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((words + kWG - 1) / kWG, 4096);
    hipLaunchKernelGGL(adc_fill_words_kernel, dim3(grid), dim3(kWG), 0, s, static_cast<uint32_t*>(dst), words, value);
    return hipGetLastError();
}

hipError_t launch_index_move(const IndexMove* d_moves, int parts, int code_bytes, uint32_t max_size, hipStream_t s) {
    if (parts <= 0) return hipSuccess;
    if (code_bytes != 8 && code_bytes != 16) return hipErrorInvalidValue;
    // grid.y walks the partitions, grid.x the 16-byte words of the largest one (4 a thread), about 65536 workgroups at most
    const unsigned gy = (unsigned)std::min(parts, 65535);
    const uint64_t threads = std::max<uint64_t>((uint64_t)max_size * code_bytes / 16, max_size);
    const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((threads + 4 * kWG - 1) / (4 * kWG), std::max(1u, 65536u / gy)));
    hipLaunchKernelGGL(index_move_kernel, dim3(gx, gy), dim3(kWG), 0, s, d_moves, parts, code_bytes);
    return hipGetLastError();
}

hipError_t launch_index_zero_tails(uint8_t* d_codes, const uint64_t* d_off, const uint32_t* d_sizes, uint32_t parts, int code_bytes,
                                   hipStream_t s) {
    if (parts == 0) return hipSuccess;
    if (code_bytes != 8 && code_bytes != 16) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)(((uint64_t)parts * 16 + kWG - 1) / kWG);
    hipLaunchKernelGGL(index_zero_tails_kernel, dim3(grid), dim3(kWG), 0, s, d_codes, d_off, d_sizes, parts, code_bytes);
    return hipGetLastError();
}

hipError_t launch_remove_minmax(const uint32_t* d_list, uint64_t count, uint32_t* d_lohi, hipStream_t s) {
    if (count == 0) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<uint64_t>((count + 4 * kWG - 1) / (4 * kWG), 1024);
    hipLaunchKernelGGL(remove_minmax_kernel, dim3(grid), dim3(kWG), 0, s, d_list, count, d_lohi);
    return hipGetLastError();
}

hipError_t launch_remove_mark(const uint32_t* d_list, uint64_t count, uint32_t lo, uint32_t* d_bitmap, hipStream_t s) {
    if (count == 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<uint64_t>((count + 4 * kWG - 1) / (4 * kWG), 4096);
    hipLaunchKernelGGL(remove_mark_kernel, dim3(grid), dim3(kWG), 0, s, d_list, count, lo, d_bitmap);
    return hipGetLastError();
}

hipError_t launch_remove_count(const RemoveSrc* d_src, int parts, uint32_t max_size, const uint32_t* d_bitmap, uint32_t lo, uint32_t last,
                               uint32_t* d_hits, uint32_t* d_first, hipStream_t s) {
    if (parts <= 0 || max_size == 0) return hipSuccess;
    // grid.y walks the partitions, grid.x the tiles of the largest one, about 65536 workgroups at most (adc_move_kernel's shape)
    const unsigned gy = (unsigned)std::min(parts, 65535);
    const uint64_t tiles = ((uint64_t)max_size + kRemoveTile - 1) / kRemoveTile;
    const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(tiles, std::max(1u, 65536u / gy)));
    hipLaunchKernelGGL(remove_count_kernel, dim3(gx, gy), dim3(kWG), 0, s, d_src, parts, d_bitmap, lo, last, d_hits, d_first);
    return hipGetLastError();
}

hipError_t launch_remove_compact(const RemovePart* d_parts, uint32_t touched, int code_bytes, const uint32_t* d_bitmap, uint32_t lo,
                                 uint32_t last, hipStream_t s) {
    if (touched == 0) return hipSuccess;
    if ((code_bytes != 4 && code_bytes != 8 && code_bytes != 16) || touched > 0x7fffffffu) return hipErrorInvalidValue;
#define QADC_RC(B) hipLaunchKernelGGL((remove_compact_kernel<B>), dim3(touched), dim3(kRemoveWG), 0, s, d_parts, d_bitmap, lo, last)
    if (code_bytes == 4) QADC_RC(4);
    else if (code_bytes == 8) QADC_RC(8);
    else QADC_RC(16);
#undef QADC_RC
    return hipGetLastError();
}

}  // namespace adc
}  // namespace qadc
