// Exact re-ranking (qadc_refine_* in include/qadc.h): what the host unit (qadc_refine.cpp) and the kernels
// (qadc_refine_kernel.hip) share.  The launch geometry is host/refine_plan.hpp, that of the keyed store host/refine_keyed_plan.hpp;
// the definition the kernels are held to, bit for bit, is host/refine.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../host/refine_keyed_plan.hpp"
#include "../host/refine_knn_plan.hpp"
#include "../host/refine_plan.hpp"
#include "../host/refine_probe_plan.hpp"
#include "../host/refine_range_plan.hpp"
#include "qadc_adc_kernels.h"   // ScanFilter

namespace qadc {
namespace refine {

// The element type of a store's rows (= QADC_REFINE_F32 / _F16 / _SQ8, asserted in qadc_refine.cpp)
enum class Elem : int { kF32 = 0, kF16 = 1, kSQ8 = 2 };
inline size_t elem_bytes(Elem e) { return e == Elem::kF32 ? 4 : e == Elem::kF16 ? 2 : 1; }

// The metric of a pass (= QADC_REFINE_L2 / _IP, asserted in qadc_refine.cpp): which instantiation of the
// distance, select and final kernels a launch picks (csrc/qadc_refine_dev.h: MetricL2, MetricIP)
constexpr int kMetricL2 = 0, kMetricIP = 1;

// The parameters of an SQ8 store in device memory: vmin, step and inv = 1 / step (0 where step is 0),
// [dim] each, and the counter of clamped components.  All null for the other element types.
struct SqParams {
    const float* vmin;
    const float* step;
    const float* inv;
    unsigned long long* clamped;
};

// One re-ranking pass over nq queries (a pass of the plan).  Every pointer is device memory and is touched by kernels only, so
// memory of another HIP runtime is legal.  rows: the store, `elem` says which element type; counts and values may be null.
struct RefinePass {
    const void* rows;
    Elem elem;
    int metric;                    // kMetricL2 / kMetricIP
    SqParams sq;
    uint32_t lo;
    uint64_t nrows;
    const uint32_t* tkey;          // a keyed store: its table's keys and rows [2^tbits] in place of [lo, lo + nrows); else null
    const uint32_t* trow;
    int tbits;
    int dim, nq, r_in, R;
    const float* queries;          // [nq][dim]
    const uint32_t* keys;          // [nq][r_in]
    const int32_t* counts;         // [nq], clamped to [0, r_in] by the kernel
    const float* values;           // [nq][r_in]
    uint64_t* words;               // scratch [nq][r_in]
    unsigned long long* missing;   // += the missing entries of the pass
    uint32_t* out_keys;            // [nq][R]
    float* out_dist;               // [nq][R]
    int32_t* out_sizes;            // [nq]
};

// refine_dist_kernel<M, Row, Lookup>: the word of every candidate of the pass into p.words (M: p.metric)
hipError_t launch_refine_dist(const RefinePass& p, const RefinePlan& plan, hipStream_t stream);
// refine_select_kernel<M, N, T>: sort, dedupe, the first R survivors and the tail of every query of the pass
hipError_t launch_refine_select(const RefinePass& p, const RefinePlan& plan, hipStream_t stream);
// refine_convert_kernel<Row>: dst[i] = Row(src[i]) for n floats, whole rows of dim (Row float: a copy; __half: round to nearest
// even; SQ8: sq_encode under component i % dim's parameters, clamped components added to sq.clamped)
hipError_t launch_refine_convert(const float* src, void* dst, Elem elem, const SqParams& sq, int dim, uint64_t n, hipStream_t stream);
// refine_get_kernel<Row, Lookup>: out[k] = the row of keys[k] as floats, or dim times 0x7FC00000 where the store does not hold it;
// found[k] (may be null) = 1 / 0.  p: rows, elem, sq, lo, nrows, the table and dim are read, nothing else.
hipError_t launch_refine_get(const RefinePass& p, const uint32_t* keys, uint64_t count, float* out, uint8_t* found, hipStream_t stream);
// refine_sq_range_kernel: lo[i] = min, hi[i] = max over the finite components of column i of vectors [n][dim], as ordered images
// (host/refine.hpp: sq_ordered); the caller has set lo to 0xFFFFFFFF and hi to 0
hipError_t launch_refine_sq_range(const float* vectors, uint64_t n, int dim, uint32_t* lo, uint32_t* hi, hipStream_t stream);
constexpr int kSqRangeRows = 64;                   // rows of a workgroup's tile of refine_sq_range_kernel

// ---- the keyed store.  Every launch takes at most kKeyedPass inputs; labels are device memory read by
// kernels only. ----

// The table, 2^bits slots: key (kKeyedEmpty = empty), row (kKeyedNoRow = empty or dead), win (the put's scratch word per slot, zero
// between calls).
struct KeyedTable {
    uint32_t* key;
    uint32_t* row;
    uint32_t* win;
    int bits;
};
// The counters of a call, device memory, zeroed by the host before the launches that add to them.
enum { kKeyedCntBad = 0, kKeyedCntAbsent, kKeyedCntClaimed, kKeyedCntNeed, kKeyedCntTaken, kKeyedCntRemoved, kKeyedCounters = 8 };
// What keyed_count leaves in dst[i] for an input that writes no row / that wins a slot without a row
constexpr uint32_t kKeyedLoser = 0xFFFFFFFFu, kKeyedNeedsRow = 0xFFFFFFFEu;

// cnt[Bad] += the labels equal to 0xFFFFFFFF, cnt[Absent] += the others the table does not know, live or dead.  Writes nothing else.
hipError_t launch_keyed_precheck(const uint32_t* labels, uint64_t n, KeyedTable t, unsigned long long* cnt, hipStream_t stream);
// Claim: slot_of[i] = the slot of labels[i], found or claimed by a CAS on the key word; win[slot] = max over its inputs of i + 1;
// cnt[Claimed] += the empty slots claimed.  The caller has made sure that the claims fit (plan_put).
hipError_t launch_keyed_claim(const uint32_t* labels, uint32_t n, KeyedTable t, uint32_t* slot_of, unsigned long long* cnt, hipStream_t stream);
// dst[i] = kKeyedLoser where a later input holds the same key, else the slot's row, or kKeyedNeedsRow (cnt[Need] += 1) where it has none
hipError_t launch_keyed_count(uint32_t n, KeyedTable t, const uint32_t* slot_of, uint32_t* dst, unsigned long long* cnt, hipStream_t stream);
// Winners without a row take one — the free list's last `free_rows` entries first, then alloc_rows, alloc_rows + 1, ... — and write
// row_key and the slot's row; every winner clears its slot's win word.  The caller has made room for the rows.
hipError_t launch_keyed_assign(const uint32_t* labels, uint32_t n, KeyedTable t, const uint32_t* slot_of, uint32_t* dst, uint32_t* row_key,
                               const uint32_t* free_list, uint32_t free_rows, uint32_t alloc_rows, unsigned long long* cnt, hipStream_t stream);
// win[slot_of[i]] = 0 for every input: what a put that fails between claim and assign leaves behind it
hipError_t launch_keyed_reset(uint32_t n, KeyedTable t, const uint32_t* slot_of, hipStream_t stream);
// rows[dst[i]] = the store's element type of src[i] for every input whose dst[i] is a row
hipError_t launch_keyed_store(const float* src, const uint32_t* dst, uint32_t n, int dim, void* rows, Elem elem, const SqParams& sq,
                              hipStream_t stream);
// Every listed key that is live: its slot's row becomes none (the slot dead), its row free (row_key, the free list from entry
// free_rows on); cnt[Removed] += 1 each.  A key listed twice frees its row once.
hipError_t launch_keyed_remove(const uint32_t* labels, uint32_t n, KeyedTable t, uint32_t* row_key, uint32_t* free_list, uint32_t free_rows,
                               unsigned long long* cnt, hipStream_t stream);
// (row_key[r], r) of every live row r < alloc_rows into the cleared table t
hipError_t launch_keyed_rebuild(const uint32_t* row_key, uint32_t alloc_rows, KeyedTable t, hipStream_t stream);

// ---- exhaustive search (qadc_refine_knn; kernels: csrc/qadc_refine_knn_kernel.hip; geometry:
// host/refine_knn_plan.hpp).  One pass of the plan over nq queries; every pointer is device memory touched by kernels only. ----
struct KnnPass {
    const void* rows;              // the store's rows [nrows][dim], `elem` says which element type
    Elem elem;
    int metric;                    // kMetricL2 / kMetricIP
    SqParams sq;
    int dim;
    uint32_t lo;                   // a dense store: the key of row r is lo + r
    uint64_t nrows;                // rows to walk (a keyed store: the rows allocated so far)
    const uint32_t* row_key;       // a keyed store: a row's key, 0xFFFFFFFF for a free row (skipped); else null
    adc::ScanFilter filter;        // bitmap null: none
    int nq, R;
    const float* queries;          // [nq][dim]
    uint64_t* buf;                 // scratch [nq][groups][buf_cap] words
    uint32_t* cnt;                 // scratch [nq][groups]: words in the buffer (zero before the first launch)
    uint64_t* bound;               // scratch [nq][groups]: the largest word that may still enter (~0 before the first launch)
    uint32_t* out_keys;            // [nq][R]
    float* out_dist;               // [nq][R]
    int32_t* out_sizes;            // [nq]
};
// refine_knn_dist_kernel<M, Row, QT, J>: the words of launch `launch`'s rows that are <= their (query, group)'s bound, appended
hipError_t launch_knn_dist(const KnnPass& p, const KnnPlan& plan, uint64_t launch, hipStream_t stream);
// refine_knn_select_kernel: every buffer of the launch's groups that holds at least R words keeps its first R, sorted; bound = the R-th
hipError_t launch_knn_select(const KnnPass& p, const KnnPlan& plan, uint64_t launch, hipStream_t stream);
// refine_knn_final_kernel<M>: the groups' lists merged: the first R words, the fillers behind them and the size of every query
hipError_t launch_knn_final(const KnnPass& p, const KnnPlan& plan, hipStream_t stream);

// ---- probed exact search (qadc_refine_knn_probed; kernels: csrc/qadc_refine_probe_kernel.hip; geometry:
// host/refine_probe_plan.hpp).  One pass of the plan over nq queries; every pointer is device memory touched by kernels only. ----

// A partition of the index as the kernel reads it: row i has the key labels[i], or key_base + i where labels is null
struct ProbePart {
    const uint32_t* labels;
    uint32_t key_base;
    uint32_t rows;
};

struct ProbePass {
    const void* rows;              // the store's rows, `elem` says which element type
    Elem elem;
    int metric;                    // kMetricL2 / kMetricIP
    SqParams sq;
    int dim;
    uint32_t lo;                   // a dense store: the keys [lo, lo + nrows)
    uint64_t nrows;
    const uint32_t* tkey;          // a keyed store: its table [2^tbits]; else null
    const uint32_t* trow;
    int tbits;
    const ProbePart* parts;        // [partitions of the index]
    adc::ScanFilter index_filter;  // the index's set filter and the call's (bitmap null: none); a key passes both
    adc::ScanFilter filter;
    int nq, R;
    const float* queries;          // [nq][dim]
    const ProbeItem* items;        // the pass's work (ProbeWork)
    const uint32_t* slots;
    uint64_t* buf;                 // scratch [nq][groups][buf_cap] words
    uint32_t* cnt;                 // scratch [nq][groups] (zero before the first launch)
    uint64_t* bound;               // scratch [nq][groups] (~0 before the first launch)
    unsigned long long* missing;   // += the entries of the pass whose key the store does not hold
    uint32_t* out_keys;            // [nq][R]
    float* out_dist;               // [nq][R]
    int32_t* out_sizes;            // [nq]
};
// One distance launch of a pass: ProbeWork's launch_items[launch], launch_slices[launch] and slice_rows
struct ProbeLaunch {
    uint32_t items, slices;
    int slice_rows;
    uint64_t launch;
};
// refine_probe_dist_kernel<M, Row, Lookup, QT, J>: the words of the launch's rows that are <= their (query, group)'s bound, appended
hipError_t launch_probe_dist(const ProbePass& p, const ProbePlan& plan, const ProbeLaunch& l, hipStream_t stream);
// refine_probe_select_kernel: every buffer that holds at least R words keeps its first R distinct ones, sorted; bound = the R-th
hipError_t launch_probe_select(const ProbePass& p, const ProbePlan& plan, hipStream_t stream);
// refine_probe_final_kernel<M>: the groups' lists merged, equal words once: the first R, the fillers behind them and the size of every query
hipError_t launch_probe_final(const ProbePass& p, const ProbePlan& plan, hipStream_t stream);

// ---- exact range search (qadc_refine_range, qadc_refine_rerank_range; kernels:
// csrc/qadc_refine_range_kernel.hip; geometry: host/refine_range_plan.hpp).  Every pointer is device memory touched by kernels only. ----

// The regions of a pass of nq queries: query q's words are buf[base[q] .. base[q] + min(cnt[q], cap[q])).
struct RangeRegions {
    int nq;
    const uint64_t* limit;         // [nq] a word is kept where it is below limit[q] (range_limit_word; 0: nothing)
    const uint64_t* base;          // [nq]
    const uint64_t* cap;           // [nq]
    unsigned long long* cnt;       // [nq] words appended, counted also beyond cap[q] (exhaustive form: zero before the first launch;
                                   //      candidate form: the segment sizes)
    uint64_t* buf;                 // the words
    uint64_t* tmp;                 // scratch of the radix passes, as large as buf (may be null where no region exceeds kRangeSortLds)
};

// The store a range kernel reads
struct RangeStore {
    const void* rows;
    Elem elem;
    SqParams sq;
    int dim;
    uint32_t lo;
    uint64_t nrows;
    const uint32_t* row_key;       // a keyed store, exhaustive form: a row's key (0xFFFFFFFF: free); else null
    const uint32_t* tkey;          // a keyed store, candidate form: the table
    const uint32_t* trow;
    int tbits;
};

// refine_range_dist_kernel<Row, QT, J>: the words of launch `launch`'s rows that are below their query's limit, appended to its region
hipError_t launch_range_dist(const RangeStore& s, const adc::ScanFilter& filter, const float* queries, const RangeRegions& g,
                             const RangePlan& plan, uint64_t launch, hipStream_t stream);
// refine_range_cand_kernel<Row, Lookup>: word i of the pass = the word of candidate keys[i] where its key is held and the word is
// below its query's limit, else ~0; *missing += the candidates whose key is not held.  chunks: the pass's chunk table [nchunks].
hipError_t launch_range_cand(const RangeStore& s, const float* queries, const uint32_t* keys, const RangeChunk* chunks, uint32_t nchunks,
                             const RangeRegions& g, unsigned long long* missing, hipStream_t stream);
// refine_range_sort_kernel: every region sorted ascending where it lies; kept[q] = its words that are not ~0 and differ from the
// word before them
hipError_t launch_range_sort(const RangeRegions& g, uint32_t* kept, hipStream_t stream);
// refine_range_compact_kernel: the kept[q] survivors of query q to out_keys / out_dist [out_off[q] ..)
hipError_t launch_range_compact(const RangeRegions& g, const uint64_t* out_off, uint32_t* out_keys, float* out_dist, hipStream_t stream);

}  // namespace refine
}  // namespace qadc
