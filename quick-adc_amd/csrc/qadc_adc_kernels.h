// Device side of the float-ADC engine for whole-byte PQ codes (the reference's scanner_simple / scan_standard<uint8_t, NSQ>,
// db_query.cpp:17-46, query_common.hpp:92-146).  Internal header shared by csrc/qadc_adc_kernel.hip and csrc/qadc_adc.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../host/adc_plan.hpp"   // Item, the level constants, plan_levels

namespace qadc {
namespace adc {

constexpr int kWG = 256;              // threads per workgroup of every kernel here

// One region per query, of its own size: query q's emitted candidates (value, key, scan-order index) go to entries
// [base[q], base[q] + cap[q]) of vals / keys / sidx.
struct Emit {
    uint32_t* count;        // [nq] candidates emitted (counted also beyond cap[q]: the host regrows that region and re-runs)
    float* vals;
    uint32_t* keys;
    uint32_t* sidx;
    const uint64_t* base;   // [nq] first entry of each region
    const uint32_t* cap;    // [nq] entries of each region
};

struct Db {
    const uint8_t* codes;     // every partition, row-major [n][code bytes], each starting on a 16-byte boundary, 16 bytes of tail padding
    const uint64_t* off;      // [part] byte offset of the partition in codes
    const uint32_t* labels;   // all partitions' labels, or nullptr (flat keys = position inside the partition)
    const uint64_t* lab_off;  // [part] first label of the partition
};

// A 4-bit database read where a qadc_index keeps it (the view of qadc_adc_index_create_view): every partition is an
// allocation of its own, row-major [n][M/2], 16-byte aligned; key = labels[position], else key_base + position.
struct Part4 {
    const uint8_t* codes;
    const uint32_t* labels;   // nullptr: unlabelled
    uint32_t key_base;
    uint32_t pad;
};

// The database launch_adc_scan reads.  centroids 256: nsq 4, 8 or 16 whole-byte codes in `bytes`, tables [nq][ma][nsq][256] (scan_standard<uint8_t,
// NSQ>).  centroids 65536: nsq 2, 4 or 8 little-endian 16-bit codes in `bytes` (rows of 2 nsq bytes), tables [nq][ma][nsq][65536], read
// from global memory (scan_standard<uint16_t, NSQ>).  centroids 16: nsq 16 or 32 nibble codes in `parts`, tables [nq][ma][nsq][16]
// summed as adc_sum_code<M> (scan_4<M>, query_common.hpp:59-90).
// The key filter of a scan (qadc_adc_filter, include/qadc.h): a bitmap over the keys [lo, lo + last], bit
// key - lo set for every key of the caller's set — the bitmap launch_remove_mark fills.  mode kFilterExclude: a row whose key is
// marked is dropped; kFilterAllow: a row whose key is not marked, or lies outside the span, is dropped.  bitmap null: no filter.
constexpr int kFilterExclude = 0, kFilterAllow = 1;   // QADC_ADC_FILTER_EXCLUDE, QADC_ADC_FILTER_ALLOW
struct ScanFilter {
    const uint32_t* bitmap = nullptr;   // last / 32 + 1 words
    uint32_t lo = 0, last = 0;
    int mode = kFilterExclude;
};

struct ScanDb {
    int nsq, centroids;
    Db bytes;             // a kernel argument by value: the owned index's code loads are global loads
    const Part4* parts;   // device memory, one entry per partition
    ScanFilter filter;    // a kernel argument by value of the filtered kernel; bitmap null: the unfiltered kernel is launched
    const ScanFilter* qfilters = nullptr;   // device memory, one entry per query of the launch (bitmap null: none for that query), or
                                            // null: no query of the call has a filter of its own and the kernels above are launched
};

// Scans items [first, first + n_items): emits (candidate, key, scan index) for every code with candidate < bound[query] whose key
// passes db.filter and db.qfilters[query].
hipError_t launch_adc_scan(const ScanDb& db, int sum_mode, const Item* items, uint32_t first, uint32_t n_items, const int32_t* assign,
                           int ma, const float* tables, const float* bound, Emit emit, hipStream_t s);
// bound[q] = min(bound[q], the R-th smallest of the values query q has stored so far) where it stored at least R.
hipError_t launch_adc_select(int nq, int R, Emit emit, float* bound, hipStream_t s);
// Packs the stored records of every query densely in query order: record sum_{j<q} stored_j + i of `out` = three words
// (value bits, key, scan index).
hipError_t launch_adc_pack(int nq, Emit emit, uint32_t* out, hipStream_t s);

// The device finish.
constexpr int kOrderLds = 4096;       // entries adc_order_kernel sorts in LDS (8 bytes each); longer streams take radix passes
constexpr int kAdcReplayMaxR = 4096;  // largest heap adc_replay_kernel keeps in LDS (8 bytes per entry and 512 of stage)

// Puts the stored candidates of every query in scan order: (value, key) of the i-th of query q to ovals / okeys [base[q] + i].
// bits = bits of the largest scan index of the batch.  tmp_a, tmp_b: scratch of as many entries as the regions, read only by
// queries that stored more than kOrderLds entries (tmp_a when bits > 8, tmp_b when bits > 16; else may be null).
hipError_t launch_adc_order(int nq, Emit emit, int bits, float* ovals, uint32_t* okeys, uint64_t* tmp_a, uint64_t* tmp_b, hipStream_t s);
// Replays every query's ordered stream through kv_binheap<unsigned, float>(R) after its R sentinels: keys / values [nq][R] and
// sizes [nq] (device memory) = the heap's arrays.  R <= kAdcReplayMaxR.
hipError_t launch_adc_replay(int nq, int R, Emit emit, const float* ovals, const uint32_t* okeys, uint32_t* keys, float* values,
                             int32_t* sizes, hipStream_t s);
// Range search.
constexpr int kRangeSortLds = 4096;   // entries adc_range_sort_kernel sorts in LDS (QADC_ADC_RANGE_SORT_LDS; 8 bytes each: 32 KiB of the CU's
                                      // 160 leave four workgroups resident); longer segments take radix passes through global scratch
// Sorts the stored (value, key) pairs of every query ascending by order_key(value) << 32 | key and writes query q's densely to
// out_vals / out_keys [out_base + sum_{j<q} stored_j + i].  tmp_a, tmp_b: scratch of as many entries as the regions, touched only by
// queries that stored more than kRangeSortLds entries (else may be null).
hipError_t launch_adc_range_sort(int nq, Emit emit, uint64_t out_base, uint32_t* out_keys, float* out_vals, uint64_t* tmp_a, uint64_t* tmp_b,
                                 hipStream_t s);
// dst[i] = src[i] for `words` 32-bit words, by a kernel (either side may be memory this library's HIP runtime did not allocate).
hipError_t launch_adc_copy_words(const void* src, void* dst, size_t words, hipStream_t s);

constexpr int kAdcMaxDim = 4096;      // largest vector dimension the feeders take (their residuals live in LDS)

// The float tables of nq queries from their vectors: d_tables [nq][ma][nsq][centroids], the layout launch_adc_scan reads;
// centroids is 256 or 65536.  d_assign [nq][ma] probed partitions (read only with d_coarse); d_coarse [K][dim] or nullptr (flat:
// residual = query); d_rotation [dim][dim] or nullptr; d_codebooks [nsq][centroids][dim/nsq]; d_cbnorm [nsq*centroids] =
// launch_row_sqnorm of the codebook rows under the same sum_mode (read by the expansion form only).  expansion 0 = the direct
// form (compute_dists_single_simd_cg), 1 = the BLAS-expansion form (compute_dists_multiple_blas_cg).  dim <= kAdcMaxDim,
// dim % nsq == 0.
hipError_t launch_adc_tables(const float* d_queries, const float* d_coarse, const int32_t* d_assign, const float* d_codebooks,
                             const float* d_cbnorm, const float* d_rotation, int nq, int ma, int nsq, int centroids, int dim,
                             int expansion, int sum_mode, float* d_tables, hipStream_t s);
// encode_multiple_vectors (quantizers.hpp:222-245) with 256 centroids per sub-quantizer on vectors already made residuals and
// rotated: d_codes [n][nsq], the capacity-1 heap's pick as compiled on the expansion distances.
hipError_t launch_adc_encode(const float* d_x, uint64_t n, int nsq, int dim, const float* d_codebooks, const float* d_cbnorm,
                             int sum_mode, uint8_t* d_codes, hipStream_t s);


// encode_multiple_vectors with 65536 centroids per sub-quantizer (nsq 2, 4 or 8), on vectors already made residuals and rotated.
// A lane owns `encode16_lane_vectors` vectors and the workgroup sweeps the centroids in ascending order, kEnc16Tile rows at a
// time through LDS (fewer where the rows are long), so a workgroup encodes 256 * encode16_lane_vectors vectors of one sub-quantizer.  A call too small to fill
// the chip with whole sweeps cuts the centroids into encode16_slices runs of at least kEnc16MinSlice (a power of two of them):
// tests/test_gpu_adc16_encode.py places NaN rows on both sides of every multiple of kEnc16MinSlice.
constexpr int kEnc16Tile = 256;
constexpr int kEnc16MinSlice = 1024;
constexpr int encode16_register_row(int ds) { return ds == 8 || ds == 16 || ds == 32 || ds == 64 ? ds : 0; }   // DS of a sq_dim: 0 = any other
constexpr int encode16_lane_vectors(int DS) { return DS >= 32 ? 2 : DS ? 4 : 1; }
int encode16_slices(uint32_t n, int nsq, int ds);
// d_codes [n][nsq] uint16 = the capacity-1 heap's pick as compiled on the expansion distances; d_part: scratch of
// encode16_slices(n, nsq, dim / nsq) * nsq * n entries.  n < 2^31 / nsq.
hipError_t launch_adc_encode16(const float* d_x, uint32_t n, int nsq, int dim, const float* d_codebooks, const float* d_cbnorm,
                               int sum_mode, unsigned long long* d_part, uint16_t* d_codes, hipStream_t s);

// ---- db_add: the dispatch of index_db::add_vectors (databases.hpp:291-297) and the growth of the owned database (DESIGN.md
// section 11.5).  The code of vector i of a pass goes to row size[p] + rank of partition p = assign[i], rank = the earlier
// vectors of the pass with the same assignment: a stable LSD radix sort of (assign, i) over the bits of K - 1, 8 bits a pass,
// whose last pass writes the rows. ----
constexpr int kAddTile = 1024;        // vectors one workgroup of the sort passes ranks (kAddTile / kWG rounds of one per thread)

// d_count[p] += vectors of the pass assigned to p, d_count[K] += those outside [0, K).  d_count [K + 1], zeroed by the caller.
hipError_t launch_adc_add_count(const int32_t* d_assign, uint32_t n, uint32_t K, uint32_t* d_count, hipStream_t s);
// Where the rows go: the owned database and, per partition, base[p] = size[p] - (vectors of the pass assigned to partitions
// below p), modulo 2^32: the i-th of the pass in (assign, i) order lands in row base[p] + i.
struct AddDst {
    uint8_t* codes;
    const uint64_t* off;
    uint32_t* labels;         // null: an unlabelled database
    const uint64_t* lab_off;
    const uint32_t* base;
};
// Scatters the pass: d_rows [n][code_bytes] (4, 8 or 16) and the label of vector i: d_row_labels[i] where d_row_labels [n] is given
// (device memory, read only by the last pass' kernel), first_label + i where it is null.  Every assign[i] is in [0, K)
// (launch_adc_add_count found none outside) and every destination row within its partition's capacity.  d_hist: (n / kAddTile + 1)
// * 256 words, d_perm_a / d_perm_b: n words each (read only where K > 256 / K > 65536).
hipError_t launch_adc_add_scatter(const int32_t* d_assign, uint32_t n, uint32_t K, int code_bytes, const uint8_t* d_rows,
                                  uint32_t first_label, const uint32_t* d_row_labels, AddDst dst, uint32_t* d_hist, uint32_t* d_perm_a,
                                  uint32_t* d_perm_b, hipStream_t s);
// Moves every partition into a new layout, one thread per (partition, 16-byte word) and per (partition, label): sizes [parts] rows
// held, offsets as Db's.  Labels are moved where both label buffers are given.
hipError_t launch_adc_move_partitions(int parts, int code_bytes, const uint32_t* d_sizes, uint32_t max_size, const uint8_t* src_codes,
                                      const uint64_t* src_off, const uint32_t* src_labels, const uint64_t* src_lab_off, uint8_t* dst_codes,
                                      const uint64_t* dst_off, uint32_t* dst_labels, const uint64_t* dst_lab_off, hipStream_t s);
// dst[i] = value for `words` 32-bit words.
hipError_t launch_adc_fill_words(void* dst, size_t words, uint32_t value, hipStream_t s);

// ---- the growing storage of the 4-bit index (csrc/qadc_index_add.cpp) ----
// One partition of a relocation: n rows from src_codes (null where n is 0) to dst_codes, its region of the new arena, and n labels
// where both label pointers are given.  Source and destination never overlap: a relocation fills a new arena.
struct IndexMove {
    const uint8_t* src_codes;
    uint8_t* dst_codes;
    const uint32_t* src_labels;
    uint32_t* dst_labels;
    uint32_t n;
    uint32_t pad;
};
// Moves every partition in one launch (grid.y over the partitions) and zeroes bytes [n * cs, align16(n * cs) + 64) behind the last
// row of each, empty ones included.  code_bytes 8 or 16; max_size: the largest n.
hipError_t launch_index_move(const IndexMove* d_moves, int parts, int code_bytes, uint32_t max_size, hipStream_t s);
// The same zeroes behind the last row of partitions that stay where they are (after an append in place, after a restore):
// partition p holds d_sizes[p] rows at d_codes + d_off[p].
hipError_t launch_index_zero_tails(uint8_t* d_codes, const uint64_t* d_off, const uint32_t* d_sizes, uint32_t parts, int code_bytes,
                                   hipStream_t s);

// ---- remove by label: the partitions of both engines compacted in place (csrc/qadc_remove.h).  The labels
// of the list are marked in a bitmap over [lo, lo + last]; a row goes when its label's bit is set. ----
constexpr int kRemoveWG = 1024;       // threads of the one workgroup that compacts a partition
constexpr int kRemoveRows = 4;        // rows a thread of it holds in registers per iteration (the loads in flight: 4 code words, 4 labels)
constexpr int kRemoveTile = 4096;     // rows of one iteration of remove_compact_kernel, and of one count of remove_count_kernel
static_assert(kRemoveTile == kRemoveWG * kRemoveRows, "a tile is what one workgroup holds in registers");

// lohi[0] = min(lohi[0], every label), lohi[1] = max(lohi[1], every label): lohi preset to {2^32 - 1, 0} by the caller.  count > 0.
hipError_t launch_remove_minmax(const uint32_t* d_list, uint64_t count, uint32_t* d_lohi, hipStream_t s);
// bit (label - lo) of d_bitmap set for every label of the list; every label lies in [lo, lo + 2^32) of a bitmap zeroed by the caller.
hipError_t launch_remove_mark(const uint32_t* d_list, uint64_t count, uint32_t lo, uint32_t* d_bitmap, hipStream_t s);
// One partition as the count reads it: its labels and rows held.
struct RemoveSrc {
    const uint32_t* labels;
    uint32_t n;
    uint32_t pad;
};
// d_hits[p] += rows of partition p whose label is marked; d_first[p] = min(d_first[p], the first tile of kRemoveTile rows that
// holds one).  d_hits zeroed, d_first preset to 2^32 - 1 by the caller.  max_size: the largest n.
hipError_t launch_remove_count(const RemoveSrc* d_src, int parts, uint32_t max_size, const uint32_t* d_bitmap, uint32_t lo, uint32_t last,
                               uint32_t* d_hits, uint32_t* d_first, hipStream_t s);
// One touched partition of the compaction: its n rows and labels where they lie, the tile to start at (the rows before it hold no
// marked label), and the bytes to zero behind the new last row (a multiple of 8; 0: none — the float-ADC index keeps none).
struct RemovePart {
    uint8_t* codes;
    uint32_t* labels;
    uint32_t n;
    uint32_t first_tile;
    uint32_t zero_bytes;
    uint32_t pad;
};
// Compacts every partition of the table in place, one workgroup each: the rows whose label is not marked move to the front in their
// old order, labels with them.  code_bytes 4, 8 or 16; touched <= 2^31 - 1.
hipError_t launch_remove_compact(const RemovePart* d_parts, uint32_t touched, int code_bytes, const uint32_t* d_bitmap, uint32_t lo,
                                 uint32_t last, hipStream_t s);

}  // namespace adc
}  // namespace qadc
