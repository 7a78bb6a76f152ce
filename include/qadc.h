/*
 * qadc.h — C-ABI of the MI355X-native Quick-ADC scan engine (libqadc_hip.so).
 *
 * Drop-in boundary for ONE path of technicolor-research/quick-adc: the 4-bit PQ scan + top-R
 * that lives behind the reference's duck-typed ScannerType.  Every entry point
 * names the reference interface it replaces (paths relative to the reference tree).  Plain
 * pointers and sizes only; no C++ types, no exceptions cross this boundary.  All functions
 * return QADC_OK (0) or a negative QADC_E_* code; qadc_last_error() gives the message of the
 * last failure on the calling thread.
 *
 * Threading: one host thread drives one index (as the reference's query loop,
 * query_common.hpp:351-365).  One index = one GPU (one process per GPU for multi-GPU).
 */
#ifndef QADC_H_
#define QADC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QADC_OK 0
#define QADC_E_ARG (-1)       /* bad argument (unsupported M, mixed labels, not finalized, ...) */
#define QADC_E_HIP (-2)       /* HIP runtime failure */
#define QADC_E_CAPACITY (-3)  /* candidate buffer too small even after regrowth / caller buffer too small */
#define QADC_E_STATE (-4)     /* call out of order */

typedef struct qadc_index qadc_index;

const char* qadc_last_error(void);
const char* qadc_version(void);

/* ---------------------------------------------------------------------------------------------
 * Device pointers of the caller (every parameter named d_*): memory behaviour.
 * A call reads the documented extent of its inputs and nothing else of the caller's, writes every element the comment of the
 * entry point lists as an output and no other byte, and a refused call (QADC_E_ARG, QADC_E_STATE, or QADC_E_CAPACITY from a
 * *_collect* / *_candidates call whose buffer is too small) writes no caller buffer but the `offsets` / `lims` arrays documented
 * for that case.  Such buffers are only ever touched by kernels, never by a memcpy of this library's HIP runtime, so they may
 * belong to another copy of the runtime (a framework's allocator).
 * Alignment: a kernel dereferences each pointer as a type of the size below, so the ADDRESS must be a multiple of it.  A pointer
 * that is not is refused with QADC_E_ARG ("<name> must be <n>-byte aligned") before any HIP call; nothing is written and the index
 * or store answers as before.  A slice of a larger allocation is a legal argument as long as its first byte obeys the table.
 *   16 bytes  d_tables    qadc_adc_query_scan_device(_filtered), qadc_adc_range_scan_device: the scan stages a table with 16-byte loads
 *             d_vectors   qadc_adc_index_add_vectors_device, _labelled_device, qadc_pq_train16_device, qadc_pq_train16_repair_device: the 16-bit encoder loads a
 *                         sub-vector 16 bytes at a time (stated for every float-ADC index, whatever its code width)
 *             d_codes     qadc_index_add_partition_device: a borrowed partition (readable up to size * M/2 rounded up to 16 bytes)
 *    4 bytes  every other float, uint32 and int32 array: d_queries, d_keys, d_values, d_sizes, d_labels, d_counts, d_out_keys,
 *             d_out_dist, d_out_sizes, and d_vectors of qadc_index_add_vectors_device, _labelled_device, qadc_refine_add_device,
 *             qadc_refine_put_device, qadc_pq_encode(_mode), qadc_pq_train_device, qadc_opq_cross_device, qadc_opq_train_device,
 *             qadc_kmeans_seed_device, qadc_pq_train_repair_device, qadc_opq_train_repair_device; d_assign, d_vectors, d_out and
 *             d_err_out of qadc_pq_decode_device, d_keys, d_out and d_where_out of qadc_adc_index_reconstruct(_rows)_device
 *             (a where entry is written as its two 32-bit words)
 *    1 byte   d_codes of qadc_pq_encode(_mode): [n][M/2] bytes, each written by itself; d_codes of qadc_pq_decode_device, read
 *             byte by byte at every code width
 * Host arrays carry no such requirement beyond their element type's.
 * ------------------------------------------------------------------------------------------- */

/* ---------------------------------------------------------------------------------------------
 * Database side — replaces scanner_4::prepare_database (db_query_4.cpp:210-228) and the layout
 * step interleave_partition_4 (simd_layout.hpp:55-65).  The device layout is plain row-major
 * [n][M/2] (one coalesced 16-byte load per lane); the 16-code block transpose is an AVX2 need.
 * ------------------------------------------------------------------------------------------- */

/* Optional, idempotent: creates the library's per-device set of HIP streams NOW (the first qadc_index_create on the device does
 * it otherwise).  The set — scan, copy, ordering, front, collectives, merge — is created once per process and device, back to
 * back, because which hardware queue and compute pipe a stream lands on depends on the streams that exist already (DESIGN.md
 * section 5).  Four of the seven are highest-priority streams and the runtime keeps at most four queues per priority: a process that
 * creates a communicator (RCCL / torch.distributed "nccl": one more highest-priority stream) BEFORE the set measured a 14-30 %
 * slower multi-GPU IVF batch (40-60 % with the priorities of rounds 1-4: profiles/r05_queue_map_rccl.txt, r05_stream_priorities.txt);
 * created AFTER the set it costs nothing.  So: call this (or create the
 * first index) right after the process selected its GPU and before it initialises any communicator.  No reference counterpart
 * (the reference is single-process CPU code).  After hipDeviceReset() the set is rebuilt by the next call / index. */
int qadc_device_prepare(int device_id);

/* Diagnostic of the stream layout (no reference counterpart): launches a kernel whose workgroups wait for CUs for several rounds on
 * stream `a` of the device's set and a one-wave marker on stream `b` right behind it (streams: 0 scan, 1 copy, 2 ordering, 3 front,
 * 4 alternative scan, 5 collectives, 6 merge).  *wait_us = when the marker started, counted from the first workgroup of the long
 * launch; *spin_us (optional) = how long that launch lasted.  A marker that starts within a few microseconds sits on another
 * compute pipe; one that waits most of spin_us shares the long launch's pipe (or its hardware queue): what a scan does to the
 * collectives or to the next batch's front when the process created other queues before the set. */
int qadc_stream_probe(int device_id, int a, int b, double* wait_us, double* spin_us);
/* The check a deployment runs once: "<creation order of the set> | ok" or "... | <pairs still obstructed, with the marker's
 * wait>", from ten probes of the pairs that matter (nothing may hold up the scan stream but its idle alternative; copy, ordering
 * and collectives must not hold up the front stream; ordering and front not the collectives').  ~3 ms, on demand only.  Not "ok"
 * means the process created queues before the set: call qadc_device_prepare earlier (a search over pad streams that would repair
 * the layout from inside was built and does not converge: DESIGN.md section 5). */
const char* qadc_stream_layout(int device_id);

/* M = 16 or 32 sub-quantizers of 4 bits (get_simd_scan_func_epi8, db_query_4.cpp:22-35). */
int qadc_index_create(qadc_index** out, int M, int device_id);
/* QADC_E_ARG, the index left intact, while a float-ADC view of it is alive (qadc_adc_index_create_view): destroy the views first. */
int qadc_index_destroy(qadc_index* idx);

/* Append partitions given as base_db::get_partition() yields them (databases.hpp:50-55):
 * row-major codes [sizes[p]][M/2], labels[p] = u32[sizes[p]] or labels == NULL for a flat DB
 * (key = position).  Host buffers are copied to the GPU; the caller may free them afterwards
 * (the reference does, db_query_4.cpp:190).  All-or-none labels (db_query_4.cpp:118-124). */
int qadc_index_add_partitions(qadc_index* idx, int part_count, const uint8_t* const* codes,
                              const uint32_t* const* labels, const uint32_t* sizes);

/* Append one partition already laid out in the reference's block layout [ceil(n/16)][M/2][16]
 * (what scanner_4::parts holds, db_query_4.cpp:171-177); converted on the GPU. */
int qadc_index_add_partition_interleaved(qadc_index* idx, const uint8_t* interleaved,
                                         const uint32_t* labels, uint32_t size);

/* Append one partition whose row-major codes (and labels) already live in device memory of this
 * GPU (borrowed, not freed; must stay valid; 16-byte aligned, readable up to size*M/2 rounded up
 * to 16 bytes).  They are read in place at query time and may change between queries: such a
 * partition gets no byte-plane copy for the split scan (qadc_index_set_split). */
int qadc_index_add_partition_device(qadc_index* idx, const void* d_codes, const void* d_labels, uint32_t size);

/* Append one synthetic flat partition generated on the GPU: 8-byte word w of the code stream =
 * splitmix64(seed ^ splitmix64(first_word + w)) (reproducible on the CPU). */
int qadc_index_add_partition_synthetic(qadc_index* idx, uint32_t size, uint64_t seed, uint64_t first_word);

/* Multi-GPU: append the local range [first_pos, first_pos + local_n) of a partition of global_n
 * codes (one process per GPU, contiguous ranges in rank order; every range but the last a multiple
 * of 16 codes).  Keys of an unlabeled shard are first_pos + local position.  `starts` = the first
 * starts_count codes of the WHOLE partition (>= max(1, unsigned(global_n * keep))), needed by every
 * rank whose range does not begin the partition: the pre-scan and therefore qmax / the int8 tables
 * are then identical on all ranks without any exchange (the reference keeps the starts in a
 * separate buffer too, db_query_4.cpp:137-145).  The padding-lane replay of the partition's last
 * code happens only on the rank that holds it. */
int qadc_index_add_partition_shard(qadc_index* idx, const uint8_t* codes, const uint32_t* labels, uint32_t local_n,
                                   uint32_t global_n, uint32_t first_pos, const uint8_t* starts, uint32_t starts_count);
/* (synthetic form: the partition's generator stream is `seed`; local_n == 0 keeps only the starts replica) */
int qadc_index_add_partition_synthetic_shard(qadc_index* idx, uint32_t global_n, uint32_t first_pos, uint32_t local_n,
                                             uint64_t seed, uint32_t starts_count);

/* Keys reported for an unlabeled partition are key_base + position (shard offset for multi-GPU). */
int qadc_index_set_key_base(qadc_index* idx, int part, uint32_t key_base);

/* Fix the "starts" sizes: max(1, unsigned(size * keep)) with the product in float
 * (db_query_4.cpp:125-126).  keep is a fraction (the CLI's -k percent * 0.01). */
int qadc_index_finalize(qadc_index* idx, float keep);

int qadc_index_partition_count(const qadc_index* idx);
uint32_t qadc_index_partition_size(const qadc_index* idx, int part);
uint32_t qadc_index_start_size(const qadc_index* idx, int part);

/* Options (30; qadc_option_names() returns the list, comma separated).  None changes WHAT is computed except the three parity
 * switches of the float half; the rest choose paths and sizes, and tests/test_gpu_fuzz.py draws them at random against the oracle.
 *  parity      "quant_mode"  1 = QuantizerMAX as the reference is compiled (one reciprocal, multiply), 0 = its source's division
 *              "sum_mode"    grouping of the float sums of the pre-scan (scan_4, query_common.hpp:72-80), of the direct table form
 *                            (fmanorm, distances.hpp:60-76) and of the expansion form's norms: 1 = as the reference binary adds them —
 *                            it is built with -ffast-math, CMakeLists.txt:7 —, 0 = source order
 *              "table_form"  float tables of qadc_search: 0 direct, 1 BLAS expansion, 2 (default) nns_engine's rule: expansion iff ma > 1
 *  diagnostics "profile"     0/1: HIP-event timing of the scan launches (qadc_profile_read)
 *  path        "wgq"         the one-workgroup-per-query path: 0 never, 1 auto (default), 2 whenever structurally possible
 *              "wgq_group"   large IVF batches take a partition-major second phase: 0 never, 1 auto, 2 whenever possible
 *              "wgq_group_head"  probes per query the head walks before it (default 2; 4 under the multi-GPU merge)
 *              "head_level"  level path: bound levels 0 .. head_level-1 are scanned by ONE head launch (default 5; 0 = off)
 *              "head_wg"     512 = the IVF head in 512-thread workgroups (8 waves per query; default at 16x4), 0 = 1024
 *  level path  "mq"          queries that share a run are scanned 8 per pass (default 1)
 *              "share_variant"  kernel form of such shared launches (bit 6 = sibling-major, bit 3 = chunked; 0 = never share)
 *              "variant"     kernel form of the other launches: bit 2 non-temporal loads, bit 3 chunked tiles, bit 4 the PROBE
 *                            diagnostic (lookups replaced by an XOR: bench.py's measured streaming ceiling; results meaningless)
 *              "front_run_max"  leading levels whose runs are at most this long join the front stream (0 = none)
 *              "wgs_per_item"   workgroups per (query, level) run (0 = auto)
 *              "cand_capacity", "level_base", "level_growth", "small_run", "prescan_sample"   sizes of the candidate regions, the
 *                            bound levels, the small-run kernel's limit, the unfiltered part of the pre-scan
 *  replay      "device_replay_nq" / "device_replay_alone_nq"  batches of at least this many queries replay their streams on the
 *                            device (0 = never) / the same for a batch with nothing else in flight (a synchronous call)
 *  query path  "wgq_split" / "wgq_split_codes"  workgroups a call of one or two queries spreads each over (default 32) / codes each
 *                            keeps at least (2048); small batches of three or more queries: at most 12, four times the codes
 *              "wgq_capacity" / "wgq_cand_cap"  stream entries per query to start with / candidates per query before a batch falls
 *                            back to the level path
 *  multi-GPU   "dist_cap_entries", "dist_device_nq", "dist_shard_replay" (an enqueued merge replays only this rank's share of the
 *              queries and a second, small all-gather shares the heaps; default 1), "dist_shard_front" (feeders + pre-scan +
 *              quantizer of a qadc_search batch are split over the ranks; default 1), "dist_inject_failure" (tests: this rank's
 *              next collect fails before the gather) — after qadc_dist_init only.
 * Streams: the library keeps ONE set of HIP streams per process and device, created by the first index on the device and shared
 * by every later one. */
const char* qadc_option_names(void);
int qadc_set_option(qadc_index* idx, const char* name, double value);

/* Copy codes back (tests / checksums): partition `part`, codes [first, first+count). */
int qadc_index_read_codes(qadc_index* idx, int part, uint32_t first, uint32_t count, uint8_t* out);

/* ---------------------------------------------------------------------------------------------
 * Query side.
 * ------------------------------------------------------------------------------------------- */

/* scanner_4::query_scan (db_query_4.cpp:245-309) for nq queries at once.
 *   assign  [nq][ma]          probed partitions in scan order (index_db::assign_compute_residuals)
 *   tables  [nq][ma][M*16]    float distance tables; MUTATED like the reference (negatives -> 0)
 *   R                         heap capacity (-r)
 * Outputs, per query q (any may be NULL):
 *   keys[q][R], values[q][R], sizes[q]   the heap ARRAYS the reference's kv_binheap would hold
 *                                        after the query (incl. the (0,127) sentinel if it survived)
 *   status[q]   0 ok; 1 = qmax > 1e30: the reference prints "Max quantization bound too high" and
 *               exit(1)s (db_query_4.cpp:271-274); here the query is skipped (sizes[q] = 0)
 *   qmin[q], qmax[q], qtables[q][ma][M][16]   the quantizer inputs/outputs (diagnostics, parity)
 * Non-finite tables follow the reference BUILD (compiled with -ffast-math):
 *   - a pre-scan sum that is not below FLT_MAX (NaN of either sign, +inf, FLT_MAX) is never among the R smallest and
 *     does not count towards them: with fewer than R sums below FLT_MAX, qmax = FLT_MAX and status[q] = 1;
 *   - qmin is the build's min reduction: a NaN in the last table entry makes it NaN (nothing is clamped then, the
 *     caller's tables stay as they are), a NaN elsewhere can leave it above the smallest entry;
 *   - a NaN entry's int8 value is 127 (the worst score).  An entry below qmax whose scaled value is NaN or outside int32
 *     is 0, otherwise the low byte of the truncation: entries below a qmin that overshoots come out NEGATIVE.  The
 *     streaming int8 scans are exact for entries in [0, 127] only; the heap of such a query (found from the caller's
 *     tables at collect time) is made from the exact saturating sums of every probed code instead, synchronously.
 *     This covers the calls that return heaps from caller-supplied tables on unsharded partitions; the candidate-
 *     stream forms, qadc_dist_collect and qadc_search do not detect it. */
int qadc_query_scan(qadc_index* idx, int nq, int ma, const int32_t* assign, float* tables, int R,
                    uint32_t* keys, int8_t* values, int32_t* sizes, int32_t* status,
                    float* qmin, float* qmax, int8_t* qtables);

/* Same work, but returns the ordered candidate stream instead of replaying it: pushing
 * (cand_keys[i], cand_vals[i]) for i in [offsets[q], offsets[q+1]) in order into the reference's
 * own kv_binheap<unsigned,int8_t>(R), after bh.push(0,127), leaves it in exactly the state the
 * reference scan would (a superset of its successful pushes, in scan order, padding-lane
 * duplicates included).  This is what a ScannerType::query_scan wrapper calls.
 * cand_capacity = entries available in cand_keys/cand_vals; QADC_E_CAPACITY if too small
 * (offsets[nq] then holds the required count). */
int qadc_query_scan_candidates(qadc_index* idx, int nq, int ma, const int32_t* assign, float* tables, int R,
                               uint64_t cand_capacity, uint32_t* cand_keys, int8_t* cand_vals,
                               uint64_t* offsets, int32_t* status, float* qmin, float* qmax);

/* Integer half only — replaces the scan_avx_4<M> calls (simd_scan.hpp:125-187; call sites
 * db_query_4.cpp:287-308): the caller supplies int8 tables qtables[nq][ma][M][16] with entries
 * in [0,127] (what QuantizerMAX<int8_t> produces) and gets the heap arrays. */
int qadc_scan_i8(qadc_index* idx, int nq, int ma, const int32_t* assign, const int8_t* qtables, int R,
                 uint32_t* keys, int8_t* values, int32_t* sizes);

int qadc_scan_i8_candidates(qadc_index* idx, int nq, int ma, const int32_t* assign, const int8_t* qtables, int R,
                            uint64_t cand_capacity, uint32_t* cand_keys, int8_t* cand_vals, uint64_t* offsets);

/* Float pre-scan only — replaces scanner_4::query_scan_start + tmp_bh.max()
 * (db_query_4.cpp:230-242, 259): qmax[q] = R-th smallest float ADC distance over the starts of
 * the probed partitions (FLT_MAX when fewer than R starts). */
int qadc_scan_start(qadc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R, float* qmax);

/* Asynchronous form of qadc_query_scan for throughput: submit enqueues all GPU work of a batch on the
 * index's streams and returns; collect waits for that batch, replays and fills the outputs.  slot is
 * 0..7 (up to eight batches in flight: one being collected, one scanning, the others queued with their
 * pre-scan fronts running ahead); a slot must be collected before it is submitted again.  `tables` must stay valid until
 * collect (it is mutated then). */
int qadc_query_scan_submit(qadc_index* idx, int slot, int nq, int ma, const int32_t* assign, float* tables, int R);
int qadc_query_scan_collect(qadc_index* idx, int slot, uint32_t* keys, int8_t* values, int32_t* sizes,
                            int32_t* status, float* qmin, float* qmax, int8_t* qtables);

/* Sharded pre-scan for multi-GPU (no counterpart in the reference, whose scan is one process).  With every rank
 * holding a replica of the starts, the float pre-scan (query_scan_start, db_query_4.cpp:230-242) would be repeated
 * on every rank; instead rank r of w pre-scans slice r of w of every probed partition's starts:
 *   qadc_prescan_submit   enqueues that pass (own buffers and stream: it may overlap an uncollected batch);
 *   qadc_prescan_collect  returns vals[nq][R] = the R smallest distances of the slice per query, FLT_MAX-padded;
 *   the caller gathers vals over the ranks (one small all-gather) into gathered[nq][w*R] and submits the batch with
 *   qadc_query_scan_submit_prescanned, which selects qmax from the gathered values instead of pre-scanning.
 * The R-th smallest of the union of the slices' R smallest values is the R-th smallest of all starts, so qmax, the
 * int8 tables and the heaps are bit-identical to qadc_query_scan_submit.  Collect with the usual collect calls. */
int qadc_prescan_submit(qadc_index* idx, int slot, int nq, int ma, const int32_t* assign, float* tables, int R,
                        int slice, int nslices);
int qadc_prescan_collect(qadc_index* idx, int slot, float* vals);
int qadc_query_scan_submit_prescanned(qadc_index* idx, int slot, int nq, int ma, const int32_t* assign, float* tables,
                                      int R, const float* prescan_vals, int nvals);

/* collect variant returning the ordered candidate stream (see qadc_query_scan_candidates): what a
 * rank hands to the cross-GPU gather.  cand_slots[i] (nullable) = position in assign[] of the probed
 * partition entry i comes from: with every partition range-sharded over the ranks, the global scan order is
 * (assign slot, rank, position), so the merge needs the slot boundaries of each rank's stream.
 * On QADC_E_CAPACITY the result is kept: call again with buffers of offsets[nq] entries. */
int qadc_query_scan_collect_candidates(qadc_index* idx, int slot, uint64_t cand_capacity, uint32_t* cand_keys,
                                       int8_t* cand_vals, uint16_t* cand_slots, uint64_t* offsets, int32_t* status,
                                       float* qmin, float* qmax);

/* ---------------------------------------------------------------------------------------------
 * "Next" row N1 of SURVEY.md §8(f): the host feeders of the path, on the device.  Queries in, heaps out;
 * assignment, residuals and float tables never cross PCIe.  Replaces:
 *   index_db::assign_compute_residuals  (databases.hpp:201-211; find_k_neighbors, neighbors.cpp:30-76)
 *   flat_db::assign_compute_residuals   (databases.hpp:93-101)
 *   opq::rotate_multiple_vectors        (quantizers.hpp:289-301)
 *   compute_dists_single_simd_cg        (distances.hpp:294-311)
 * followed by the same chain as qadc_query_scan.  Pinned to the reference's own code: the direct
 * table form (fmanorm as compiled), the residuals, the SELECTION of the ma nearest — find_k_neighbors' heaps, exact
 * distance ties included (what the heap's history and kv_binheap::sort leave, neighbors.cpp:18-28, 47-71) — and the NORM half
 * of the BLAS-expansion form (||v||^2 + ||c||^2 as compute_cross_dists_blas hands it to sgemm, distances.hpp:151-215): the
 * coarse distances under the selection and the ma > 1 tables are in that form.  Restated, unpinned: the products of cblas_sgemm
 * (OpenBLAS is not in the image: one sequential dot each); bit-exact against quick-adc_amd/host/query_driver.hpp and the
 * oracle, which evaluate the same sums on the host.
 * ------------------------------------------------------------------------------------------- */
/* codebooks [M][16][dim/M] (base_pq::centroids_flat order). */
int qadc_index_set_pq(qadc_index* idx, int dim, const float* codebooks);
/* OPQ rotation [dim][dim] (opq::rotation): residuals are rotated before the tables are built,
 * rotated[r] = sum_c x[c] * rotation[r][c] (opq::rotate_multiple_vectors, quantizers.hpp:289-301).  NULL = plain PQ. */
int qadc_index_set_rotation(qadc_index* idx, const float* rotation);
/* coarse centroids [K][dim], K == partition count (partition p belongs to centroid p).  Not called = flat. */
int qadc_index_set_coarse(qadc_index* idx, int K, const float* centroids);
/* queries [nq][dim]; outputs as qadc_query_scan; assign_out [nq][ma] (nullable) = probed partitions. */
int qadc_search(qadc_index* idx, int nq, const float* queries, int ma, int R, uint32_t* keys, int8_t* values,
                int32_t* sizes, int32_t* status, int32_t* assign_out);
int qadc_search_submit(qadc_index* idx, int slot, int nq, const float* queries, int ma, int R);
int qadc_search_collect(qadc_index* idx, int slot, uint32_t* keys, int8_t* values, int32_t* sizes, int32_t* status,
                        int32_t* assign_out);

/* "Next" row N4 (database build): PQ encode on the device — base_pq::encode_multiple_vectors for plain PQ
 * (quantizers.hpp:222-245): per sub-quantizer find_k_neighbors(count, 16, sq_dim, k = 1, ...) (neighbors.cpp:30-76) — the
 * BLAS-expansion distances (||v||^2 + ||c||^2) - 2 v.c of compute_cross_dists_blas (distances.hpp:151-215) pushed in
 * centroid order into a capacity-1 kv_binheap: the first strict minimum — packed by multiple_set_bits_4
 * (quantizers.hpp:49-68).  The norms add as the reference is compiled (pinned to its own text), the
 * product is one sequential dot (the reference's is OpenBLAS's sgemm: restated).  d_vectors [n][dim] float and d_codes
 * [n][M/2] are device pointers of `device_id` (the _host form stages host buffers).
 * _mode: encode_form 1 = that (what the plain entry points do), 0 = the direct form sum (x - c)^2, first minimum (this
 * library's encoder before round 6: vectors nearly equidistant from two centroids can get another code than the
 * reference writes); sum_mode 1 = norms as compiled, 0 = sequential. */
int qadc_pq_encode(int M, int dim, const float* codebooks, const void* d_vectors, uint64_t n, void* d_codes, int device_id);
int qadc_pq_encode_host(int M, int dim, const float* codebooks, const float* vectors, uint64_t n, uint8_t* codes,
                        int device_id);
int qadc_pq_encode_mode(int M, int dim, const float* codebooks, const void* d_vectors, uint64_t n, void* d_codes,
                        int encode_form, int sum_mode, int device_id);
int qadc_pq_encode_host_mode(int M, int dim, const float* codebooks, const float* vectors, uint64_t n, uint8_t* codes,
                             int encode_form, int sum_mode, int device_id);

/* N4, the rest of the build path (host buffers in and out, any device).
 * qadc_ivf_encode_host = the compute of index_db::add_vectors (databases.hpp:270-298) / flat_db::add_vectors (136-156):
 *   nearest coarse centroid per vector (K > 0; find_k_neighbors with k = 1 on the expansion distances: its compiled replace
 *   test !(d >= kept), the first strict minimum after the last NaN), residual, optional OPQ rotation rotated[r] = sum_c x[c] * rotation[r][c] (quantizers.hpp:289-301; rotation
 *   [dim][dim] or NULL), PQ encode (quantizers.hpp:222-245; qadc_pq_encode above, _mode likewise).  assign_out [n]
 *   (nullable; untouched when K == 0), codes [n][M/2].  The caller dispatches (assign, code, label = index + offset) to its partitions in vector order
 *   like databases.hpp:291-297 (host/db_build.hpp does).
 * qadc_kmeans_iterations_host = kmeans_fast_iterations_thread (databases.cpp:50-90): `iters` rounds of assign-to-nearest
 *   + centroid = (sum of the members in ascending vector order) * (1.0f / count) — AS THE REFERENCE IS COMPILED: under its
 *   -ffast-math g++ replaces the source's division (databases.cpp:83-88) by a reciprocal and a multiplication, pinned to those
 *   loops compiled here with the reference's flags (tests/test_oracle_float_ref.py); an empty cluster becomes NaN either way;
 *   centroids [K][dim] in and out.  qadc_kmeans_iterations_host_mode: div_mode 1 = that, 0 = the source's division.  The reference seeds these iterations with two OpenCV
 *   k-means++ iterations (databases.cpp:96-113) — third-party, not restated: the caller provides the seed, or takes
 *   qadc_kmeans_seed_host's (k-means++ seeding, below). */
int qadc_ivf_encode_host(int M, int dim, const float* codebooks, const float* rotation, int K, const float* coarse,
                         const float* vectors, uint64_t n, int32_t* assign_out, uint8_t* codes, int device_id);
int qadc_ivf_encode_host_mode(int M, int dim, const float* codebooks, const float* rotation, int K, const float* coarse,
                              const float* vectors, uint64_t n, int32_t* assign_out, uint8_t* codes, int encode_form,
                              int sum_mode, int device_id);
int qadc_kmeans_iterations_host(const float* vectors, uint64_t n, int dim, int K, float* centroids, int iters,
                                int32_t* assign_out, int device_id);
/* qadc_coarse_assign_host = find_k_neighbors (neighbors.cpp:30-76) with k = ma on the coarse centroids, as qadc_search's front
 *   computes it (the expansion distances, then the reference's heap selection AS COMPILED, NaN and exact ties included):
 *   queries [nq][dim], coarse [K][dim] -> assign_out [nq][ma], nearest first; 0 < ma <= K.  Every entry is in [0, K).
 *   A query with a NaN distance and ma > 256 is refused (QADC_E_ARG): the exact replay keeps at most 256 entries. */
int qadc_coarse_assign_host(const float* queries, int nq, const float* coarse, int K, int dim, int ma, int32_t* assign_out,
                            int device_id);
int qadc_kmeans_iterations_host_mode(const float* vectors, uint64_t n, int dim, int K, float* centroids, int iters,
                                     int32_t* assign_out, int div_mode, int device_id);

/* Learning the product quantizer: `iters` rounds of k-means in every sub-space at once, on a learning set held once in device
 * memory.  Sub-quantizer m of sq_count (dsub = dim / sq_count) ends as kmeans_fast_iterations_thread (databases.cpp:50-90)
 * applied to the n x dsub matrix of columns [m dsub, (m + 1) dsub), started from codebooks[m]: the bits that
 * qadc_kmeans_iterations_host_mode returns for that slice.  A round assigns with the encoder of the index the codebooks are for
 * (sq_bits 4 with sq_count 16 or 32: qadc_pq_encode's reference form; sq_bits 8 with sq_count 4, 8 or 16: qadc_adc_encode_host's),
 * then centroid = (its members' sub-vectors summed in ascending vector index into one running float from 0.0f) * (1.0f / count)
 * (div_mode 1, as the reference is compiled; 0: divided by the count, as its source reads).  An empty cluster becomes NaN and
 * stays NaN, as in the reference; qadc_pq_train_repair_host below repairs it on request ("Empty-cluster repair").  sum_mode: the norms' grouping, as for the encoders.
 * K_coarse > 0: the learning set is first made residuals to the nearest of coarse [K_coarse][dim] (find_k_neighbors, k = 1);
 * rotation [dim][dim] or NULL: ... and rotated (rotated[r] = sum_c x[c] * rotation[r][c]) — what index_db::add_vectors hands to
 * the quantizer.  The caller seeds (the reference leaves learning to an outside project; qadc_kmeans_seed_host below is one seed): codebooks [sq_count][2^sq_bits][dsub] in
 * and out; iters == 0 returns them untouched and writes no code.  codes_out (nullable, host memory): the last round's
 * assignment in the encoder's layout ([n][sq_count / 2] packed nibbles, or [n][sq_count] bytes) — the codes under the codebooks
 * of BEFORE the last update.  empty_out (nullable): centroids with a NaN component at return.
 * Limits: the learning set is resident for the call; 0 < n < 2^32; dim <= 2048 at 4 bits, <= 4096 at 8 bits (the encoders').
 * sq_bits 16 is refused (QADC_E_ARG): qadc_pq_train16_host below learns those.  qadc_pq_train_device: the same with the vectors already in device memory
 * (read only, by kernels); every other pointer is host memory. */
int qadc_pq_train_host(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                       const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode,
                       int sum_mode, int device_id);
int qadc_pq_train_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                         const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode,
                         int sum_mode, int device_id);

/* The same for 16-bit sub-quantizers: sq_count 2, 4 or 8, codebooks [sq_count][65536][dsub] in and out.
 * No float semantics are new: sub-quantizer m ends as kmeans_fast_iterations_thread on columns [m dsub, (m + 1) dsub) started
 * from codebooks[m].  A round assigns with the 16-bit encoder (qadc_adc_encode16_host's kernels, over the resident learning set in
 * passes of QADC_ADC_ENCODE16_CHUNK vectors), then updates: per sub-quantizer the vectors are sorted by (code, index) on the GPU
 * and centroid (m, k) = (its members' sub-vectors summed in ascending vector index into one running float from 0.0f)
 * * (1.0f / (float)count) (div_mode 1) or / (float)count (div_mode 0).  An empty cluster becomes NaN and stays NaN; empty_out
 * counts them, and qadc_pq_train16_repair_host below repairs them on request ("Empty-cluster repair").  K_coarse, coarse, rotation, sum_mode: as for qadc_pq_train_host.  codes_out (nullable,
 * host memory): little-endian uint16 [n][sq_count], qadc_adc_encode16_host's layout — the last round's assignment, under the
 * codebooks of BEFORE the last update.  iters == 0 returns the seed untouched, writes no code and touches no device.
 * Refused with QADC_E_ARG before the first HIP call: sq_count outside {2, 4, 8}; dim not a multiple of it or > 4096; dsub > 2048;
 * NULL vectors or codebooks; n == 0 or n >= 2^32; iters < 0; K_coarse < 0, or > 0 without coarse; div_mode or sum_mode not 0 or 1.
 * Limits: the learning set, its residual copy (with coarse or rotation), the codes and two index permutations of n words are
 * resident for the call.  The update's critical path is the largest cluster: one cluster holding every vector is n dependent
 * additions on one lane group — correct, and slow.  The OPQ rotation is not learned, the seed is the caller's, and an empty
 * cluster is re-seeded only by qadc_pq_train16_repair_host.
 * qadc_pq_train16_device: the vectors already in device memory (read only, by kernels); every other pointer is host memory. */
int qadc_pq_train16_host(const float* vectors, uint64_t n, int dim, int sq_count, int K_coarse, const float* coarse,
                         const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode,
                         int sum_mode, int device_id);
int qadc_pq_train16_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int K_coarse, const float* coarse,
                           const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode,
                           int sum_mode, int device_id);
/* The update of qadc_pq_train16_host alone, from codes the caller gives (a caller who assigns by other means): vectors [n][dim]
 * as the quantizer sees them, codes [n][sq_count] -> codebooks_out [sq_count][65536][dsub], every centroid written (NaN where
 * empty), and counts_out [sq_count][65536] (nullable) the cluster sizes.  Refusals as above, and NULL codes. */
int qadc_pq_update16_host(const float* vectors, uint64_t n, int dim, int sq_count, const uint16_t* codes, float* codebooks_out,
                          uint32_t* counts_out, int div_mode, int device_id);

/* ---- Learning the OPQ rotation: non-parametric OPQ, Procrustes rounds around qadc_pq_train_*. ----
 *
 * X0 = the learning set as the quantizer sees it BEFORE rotation: with K_coarse > 0 the residual to the nearest of
 * coarse [K_coarse][dim] (what qadc_pq_train_* computes in front of a NULL rotation), else the vectors themselves.
 *
 * qadc_opq_cross_host: the cross matrix M = X0^T Y between X0 and its reconstruction in the rotated space,
 *   Y[i][b] = codebooks[m][code(i, m)][b - m dsub], m = b / dsub, code(i, m) read from `codes` in the encoder's layout (sq_bits 4:
 *   packed nibbles [n][sq_count / 2], the even sub-quantizer in the low nibble; 8: bytes [n][sq_count]).  Every float is pinned:
 *   for block j = vectors [QADC_OPQ_BLOCK j, min(n, QADC_OPQ_BLOCK (j + 1))), partial_j[a][b] is the float chain
 *   acc = fmaf(X0[i][a], Y[i][b], acc) over ascending i from 0.0f; M_out[a][b] (double [dim][dim], row a = component of X0, column
 *   b = component of Y) = the sum of (double)partial_j[a][b] over ascending j from 0.0.  Host twin: host/db_build.hpp opq_cross.
 *   Limits: the learning set, its residual (with a coarse quantizer), the codes, the codebooks and
 *   ceil(n / QADC_OPQ_BLOCK) * dim^2 * 4 bytes of partials are resident for the call; one device; synchronous.
 *   Refused with QADC_E_ARG before the first HIP call: everything qadc_pq_train_host refuses (sq_bits 16 included: a follow-up
 *   on the sorted update), dim > 1024, NULL codes or M_out.  qadc_opq_cross_device: the vectors already in device memory (read
 *   only, by kernels); every other pointer is host memory. */
#define QADC_OPQ_BLOCK 2048   /* vectors per float partial sum of the cross matrix */
int qadc_opq_cross_host(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                        const void* codes, const float* codebooks, double* M_out, int sum_mode, int device_id);
int qadc_opq_cross_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                          const void* codes, const float* codebooks, double* M_out, int sum_mode, int device_id);
/* Host only (no GPU involved; host/procrustes.hpp): the orthogonal rotation_out [dim][dim] that maximises tr(R M) for M [dim][dim]
 *   doubles — with M = U S V^T, R = V U^T, rounded to float.  In the project's convention rotated[r] = sum_c x[c] R[r][c], so for
 *   M = X0^T Y it is the rotation with X0 R^T closest to Y.  A deterministic one-sided (Hestenes) Jacobi SVD in double, cyclic
 *   order; sweeps_out (nullable): the sweeps it took.  A rank-deficient M (the zero matrix included) still gives an orthogonal R:
 *   the missing left vectors are completed by Gram-Schmidt against the unit vectors in index order; a positive diagonal M gives
 *   the identity exactly.  QADC_E_ARG: a non-finite entry of M, NULL pointers, dim outside [1, 1024] (O(dim^3) per sweep).
 *   QADC_E_STATE: the sweep cap (64) was reached — no matrix is returned, never a non-orthogonal one.  rotation_out is
 *   untouched on every error. */
int qadc_procrustes_host(const double* M, int dim, float* rotation_out, int* sweeps_out);
/* qadc_opq_train_host: rotation [dim][dim] in and out (the identity for "none": it is applied like any rotation), codebooks
 *   [sq_count][2^sq_bits][dsub] in and out, seeded by the caller as for qadc_pq_train_host; outer >= 0, inner >= 1.
 *     for t in 0 .. outer - 1:
 *         (codebooks, codes) = qadc_pq_train_host(..., rotation, codebooks, iters = inner)
 *         M = qadc_opq_cross_host(..., codes, codebooks)        -- the codes of the last round, the codebooks after its update
 *         if M has a non-finite entry: leave the loop            -- rotation untouched, rounds_done = t
 *         rotation = qadc_procrustes_host(M)
 *     (codebooks, codes) = qadc_pq_train_host(..., rotation, codebooks, iters = inner)    -- the closing rounds, always run
 *   and every returned float and code equals, bit for bit, that loop written with the three public calls (host twin:
 *   host/db_build.hpp opq_train_iterations).  outer == 0 is qadc_pq_train_host with iters = inner.  The learning set goes up
 *   once; X0, its rotated copy (refreshed per outer round by the training call's own kernel), the codes and the codebooks stay
 *   in device memory; the coarse assignment is computed once; per outer round only M comes down and the rotation goes up.
 *   codes_out, empty_out: as for qadc_pq_train_host, after the closing rounds.  rounds_done_out (nullable): rotation updates
 *   completed.  div_mode, sum_mode: as for qadc_pq_train_host.
 *   Refused with QADC_E_ARG before the first HIP call: everything qadc_pq_train_host refuses; sq_bits 16; dim > 1024; NULL
 *   rotation; outer < 0; inner < 1.  QADC_E_STATE: a Procrustes solve hit its sweep cap (rotation and codebooks are then not
 *   a fitted pair).  Limits: 4 and 8 bits; dim <= 1024; the learning set, its residual, its rotated copy, the codes and the
 *   partials are resident for the call; one device; synchronous.  Not done: the parametric initialisation, seeding (qadc_kmeans_seed_host below),
 *   16-bit codebooks.  Empty-cluster repair: qadc_opq_train_repair_host below.  qadc_opq_train_device: the vectors already in device memory (read only, by kernels). */
int qadc_opq_train_host(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                        float* rotation, float* codebooks, int outer, int inner, void* codes_out, uint64_t* empty_out,
                        int* rounds_done_out, int div_mode, int sum_mode, int device_id);
int qadc_opq_train_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                          float* rotation, float* codebooks, int outer, int inner, void* codes_out, uint64_t* empty_out,
                          int* rounds_done_out, int div_mode, int sum_mode, int device_id);

/* ---- k-means++ seeding: D^2 picks in every sub-space at once, the seed of the learning calls above. ----
 *
 * vectors [n][dim]; sq_count sub-spaces of dsub = dim / sq_count columns; k centres per sub-space; a 64-bit seed.  K_coarse,
 * coarse, rotation: the learning set first goes through the trainers' front (qadc_pq_train_host's: residual to the nearest coarse
 * centroid, then rotated; sum_mode 1) — x below is its output.  Sub-space m is seeded on columns [m dsub, (m + 1) dsub), independently:
 *   Random numbers (splitmix64's finaliser, arithmetic mod 2^64):
 *     z = seed + 0x9E3779B97F4A7C15 * ((((uint64)m << 32) | t) + 1);  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *     z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31;  u(m, t) = (double)(z >> 11) * 2^-53, in [0, 1).
 *   Pick 0: row min(n - 1, (uint64)(u(m, 0) * (double)n)).
 *   Distance of row i to a centre c: ONE float chain acc = fmaf(x[i][d] - c[d], x[i][d] - c[d], acc) from 0.0f over ascending d (the
 *     direct form: a row's distance to itself is exactly 0).  mind_i starts at +inf and becomes d < mind_i ? d : mind_i after every
 *     pick (a NaN never replaces).  Weight w_i = mind_i if mind_i < +inf, else 0: rows with a NaN or overflowing distance are never
 *     drawn; picked rows and their exact duplicates weigh 0.
 *   Sum tree, radix 64, indexed by the row alone (no launch geometry enters): level 0 is (double)w_i; node j of level L + 1 is the
 *     balanced binary tree sum, in double, of nodes [64 j, 64 j + 64) of level L, missing nodes counting as 0.0 (a 64-lane
 *     xor-butterfly gives exactly this value: double addition commutes).  Levels 1 and 2 always exist; above them the tree goes up
 *     to the first level with a single node, the root.
 *   Pick t >= 1: target = u(m, t) * root, in double.  From the root down, at a node its children are walked in ascending order
 *     under a sequential double prefix c (c = c + child): the first child with target < c + child is entered and the walk goes on
 *     below it with target - c.  If rounding leaves no such child, the last child with a value > 0 is entered, with its own prefix.
 *     At level 0 the same rule names the row.  A zero child is never entered: the row has w > 0 and differs from every earlier centre.
 *   Fallback: root == 0 (fewer distinct finite sub-vectors than k, or pick 0 hit a non-finite row) — the pick is the smallest row
 *     index not yet picked in this sub-space; such picks are counted.
 * Outputs (host memory): centres_out [sq_count][k][dsub] = the picked rows' sub-vectors of x, copied bit for bit; rows_out
 * [sq_count][k] (nullable) their indices; fallbacks_out (nullable) the fallback picks of all sub-spaces.  Host twin:
 * host/kmeans_seed.hpp kmeans_seed (behind host/db_build.hpp's pq_train_front); the device result equals it bit for bit.
 * A run is k rounds on one stream (per round one pass over x for all sub-spaces, then one pick launch); synchronous.
 * Refused with QADC_E_ARG before the first HIP call, the message naming the cause: NULL vectors or centres_out; n == 0 or
 * n >= 2^32; k < 1 or k > n; sq_count outside [1, 32]; dim not a positive multiple of sq_count; dim > 4096; K_coarse < 0, or > 0
 * without coarse; d_vectors not 4-byte aligned.  Limits: the learning set, its front copy, sq_count * n floats of distances and the
 * tree are resident for the call; one device.  Empty-cluster repair inside the training rounds: qadc_pq_train_repair_host below.  Not done: cv::kmeans' own variant
 * (its local trials, its RNG), k-means||, learning sets larger than device memory, more than one device.
 * qadc_kmeans_seed_device: the vectors already in device memory (read only, by kernels); every other pointer is host memory. */
int qadc_kmeans_seed_host(const float* vectors, uint64_t n, int dim, int sq_count, int64_t k, int K_coarse, const float* coarse,
                          const float* rotation, uint64_t seed, float* centres_out, uint32_t* rows_out, uint64_t* fallbacks_out,
                          int device_id);
int qadc_kmeans_seed_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int64_t k, int K_coarse, const float* coarse,
                            const float* rotation, uint64_t seed, float* centres_out, uint32_t* rows_out, uint64_t* fallbacks_out,
                            int device_id);

/* ---- Empty-cluster repair: a step between the assignment and the update of a training round. ----
 *
 * Why: the assignment is pinned to the reference's heap as compiled — a NaN distance replaces the kept centroid and any later
 * value replaces a NaN — so ONE NaN centroid at index j hides every centroid below j from every vector of the next round, and the
 * returned codebook encodes by the same rule.  The repair is defined per sub-space m, independently.  Inputs: x, the learning set as
 * the quantizer sees it (behind the trainers' residual and rotation front); cb, the codebooks this round's assignment used; the
 * round's codes.  K = 2^sq_bits, c_i = the code of vector i in sub-space m.
 *   1. count[k] = the number of i with c_i == k; first[k] = the smallest such i.  The empties are the k with count[k] == 0 in
 *      ascending order, e_0 < e_1 < ... < e_{E-1}.  E == 0 changes nothing.
 *   2. d_i = ONE float chain acc = fmaf(t, t, acc), t = x[i][d] - cb[m][c_i][d], from 0.0f over the ascending columns d of
 *      sub-space m (the seeding's direct form).
 *   3. Vector i is eligible iff d_i is finite (neither NaN nor +inf), d_i > 0, and i != first[c_i]: every cluster keeps its
 *      lowest-index member, so a repair never empties a cluster.
 *   4. key_i = ((uint64)bits(d_i) << 32) | (0xFFFFFFFF - i).  Chosen are the min(E, number eligible) eligible vectors with the
 *      largest keys: farthest first, among equal distances the lower index.
 *   5. The chosen vectors in ascending index are s_0 < s_1 < ...; c_{s_j} = e_j.  moved[m] = the number chosen.  Empties beyond
 *      that stay empty: they become NaN in the update and are counted by empty_out as before.
 * A repaired round is assign, repair, update.  The update is unchanged and sees the rewritten codes: a filled cluster's centroid
 * is exactly its one vector's sub-vector, the donor's mean loses that vector, every sum keeps its pinned order, and no float meets
 * an atomic.  codes_out reports the repaired codes of the last round.  Host twin: host/pq_repair.hpp pq_repair, and the `repair`
 * overloads of pq_train_iterations, pq_train16_iterations, opq_train_iterations (host/db_build.hpp); the device equals them bit for
 * bit.
 *
 * qadc_pq_repair_host: the step alone on the caller's codes (the counterpart of qadc_pq_update16_host).  vectors [n][dim] as the
 *   quantizer sees them, codebooks [sq_count][2^sq_bits][dsub], codes in and out in the encoder's layout (sq_bits 4: packed nibbles
 *   [n][sq_count / 2], the even sub-quantizer in the low nibble; 8: bytes [n][sq_count]; 16: little-endian uint16 [n][sq_count]),
 *   moved_out [sq_count] (nullable).  Refused with QADC_E_ARG before the first HIP call, the message naming the cause: sq_bits
 *   outside {4, 8, 16}; everything the trainer of that width refuses (qadc_pq_train_host at 4 and 8 bits, qadc_pq_train16_host at
 *   16); NULL codes.
 * qadc_pq_train_repair_host / _device, qadc_pq_train16_repair_host / _device, qadc_opq_train_repair_host / _device: the calls
 *   above with two more arguments.  repair 0: the call above, bit for bit (which is now a thin caller of these); 1: every round is
 *   a repaired round — for OPQ the contract stays "the loop of the public calls", now of the repaired ones.  repaired_out
 *   (nullable): the moves of all rounds and sub-spaces.  Another value of repair is refused (QADC_E_ARG).
 * Limits: with repair 1, sq_count * n keys of 8 bytes are resident for the call beside the trainer's own memory, plus count,
 *   first and the empties (12 bytes per centroid), the histograms and one word per 1024 vectors and sub-space.  A round on a
 *   codebook without an empty cluster costs one integer pass over the codes and launches that return at once: nothing waits on
 *   the host inside a round, E stays in device memory.  Not done: the coarse k-means qadc_kmeans_iterations_host (int32
 *   assignment, arbitrary K, its own update: a follow-up on the same kernels); splitting large clusters by any other rule;
 *   learning sets larger than device memory. */
int qadc_pq_repair_host(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, const float* codebooks, void* codes,
                        uint32_t* moved_out, int device_id);
int qadc_pq_train_repair_host(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                              const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode,
                              int sum_mode, int repair, uint64_t* repaired_out, int device_id);
int qadc_pq_train_repair_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse,
                                const float* coarse, const float* rotation, float* codebooks, int iters, void* codes_out,
                                uint64_t* empty_out, int div_mode, int sum_mode, int repair, uint64_t* repaired_out, int device_id);
int qadc_pq_train16_repair_host(const float* vectors, uint64_t n, int dim, int sq_count, int K_coarse, const float* coarse,
                                const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode,
                                int sum_mode, int repair, uint64_t* repaired_out, int device_id);
int qadc_pq_train16_repair_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int K_coarse, const float* coarse,
                                  const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out,
                                  int div_mode, int sum_mode, int repair, uint64_t* repaired_out, int device_id);
int qadc_opq_train_repair_host(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                               float* rotation, float* codebooks, int outer, int inner, void* codes_out, uint64_t* empty_out,
                               int* rounds_done_out, int div_mode, int sum_mode, int repair, uint64_t* repaired_out, int device_id);
int qadc_opq_train_repair_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse,
                                 const float* coarse, float* rotation, float* codebooks, int outer, int inner, void* codes_out,
                                 uint64_t* empty_out, int* rounds_done_out, int div_mode, int sum_mode, int repair,
                                 uint64_t* repaired_out, int device_id);

/* Host-only helper (no GPU involved): push (keys[i], vals[i]), i = 0..n-1, in order into an empty
 * heap of capacity R with kv_binheap<unsigned,int8_t>::push semantics (binheap.hpp:75-116), after
 * an optional (0,127) sentinel (db_query_4.cpp:276), and return the heap arrays.  This is the
 * replay the other entry points apply to the device's candidate stream. */
int qadc_replay_i8(uint64_t n, const uint32_t* keys, const int8_t* vals, int R, int push_sentinel,
                   uint32_t* out_keys, int8_t* out_vals, int32_t* out_size);

/* Host-only helper: kv_binheap<unsigned,int8_t>::sort_keys (binheap.hpp:129-137) of a heap whose arrays are
 * heap_keys / heap_vals[size] (as returned by the entry points above): the keys ascending by value, tied values in
 * the order std::sort leaves them on that array — what a caller of the reference gets from bh.sort_keys(). */
int qadc_sort_keys_i8(int size, const uint32_t* heap_keys, const int8_t* heap_vals, uint32_t* out_keys);

/* Host half of the multi-GPU merge: `gathered` = the world int32 buffers of buflen words each that the ranks
 * contributed to ONE all-gather, each laid out as [nq counts][cap keys][ceil(cap/4) words of int8 values]
 * [only when ma > 1: ceil(cap/2) words of u16 assign slots][anything else].  Replays queries q_first, q_first + q_step, ... in
 * global scan order (assign slot, rank, position) after the (0,127) sentinel; keys/vals are [nq][R], rows of other
 * queries are left untouched.  No GPU needed. */
int qadc_merge_streams_i8(int world, int nq, int R, uint64_t cap, int ma, const int32_t* gathered, uint64_t buflen,
                          int q_first, int q_step, const int32_t* status, uint32_t* keys, int8_t* vals, int32_t* sizes);

/* Diagnostic: all candidate values min(127, sum) of one partition for one int8 table [M][16]. */
int qadc_candidates_i8(qadc_index* idx, int part, const int8_t* qtable, int8_t* out);

/* Diagnostic / recall ground truth: the exact float-ADC nearest code of one
 * partition for one float table [M*16]: smallest distance (scan_4<M> summation order), lowest
 * position on ties.  key = label, or key_base + position. */
int qadc_float_top1(qadc_index* idx, int part, const float* table, uint32_t* out_key, uint32_t* out_pos, float* out_dist);

/* ---------------------------------------------------------------------------------------------
 * Measurement (bench.py): HIP-event timing of the int8 scan kernel on the index's stream.
 * Enabled with qadc_set_option(idx, "profile", 1).  Totals since the last reset.
 * ------------------------------------------------------------------------------------------- */
/* ---- Multi-GPU (north star: "the code list shards across the 8 GPUs of one node with a final RCCL
 * allgather of per-shard top-k over xGMI").  One process per GPU; every rank holds a contiguous range of every
 * partition (qadc_index_add_partition_shard) and submits the same batches.  What is gathered is each shard's ordered
 * PUSH STREAM, not its final top-R: re-pushing final heaps is not exact under ties (binheap.hpp:75-116 resolves ties by
 * push order).  qadc_dist_collect replaces qadc_query_scan_collect: it packs this rank's streams (already in device
 * memory), runs ONE ncclAllGather (device to device, no host staging), and replays the world's streams in global
 * scan order (assign slot, rank, position) on the GPU, one wave per query — at collect time every rank replays every query
 * (no second collective); a merge enqueued with its batch (below) shards the replay by query and shares the heaps with a
 * second, small all-gather.  `extra` (optional, extra_n floats per rank) rides in the same all-gather and comes
 * back as extra_out[world][extra_n]: the multi-rank loop of bench.py ships the next batch's sharded pre-scan values
 * this way (qadc_prescan_submit).  RCCL is loaded with dlopen by qadc_dist_unique_id / qadc_dist_init; a single-GPU
 * user never loads it.  world <= 16.  Any R: the device merge (one wave per query, heap in registers) holds R <= 320,
 * larger heaps take the host-share replay.  A query some rank could not order on the device (> 16384 candidates) is
 * sorted on that rank's host and shipped in the same gather.  A rank whose batch failed locally still takes part in the
 * gather with a failure flag in its header, so every rank returns an error instead of one rank leaving the others
 * blocked.  A batch submitted after qadc_dist_init may still be collected with the plain collect calls (host replay
 * of this rank's streams only).  Large batches (>= "dist_device_nq" queries: IVF; on either scan path) have their merge —
 * pack, all-gather, interleave, replay — ENQUEUED WITH THE BATCH, behind its scan, so qadc_dist_collect only waits for it
 * (option "dist_async", default 1): after qadc_dist_init every rank must therefore SUBMIT the same batches in the same
 * order, not just collect them (the all-gather of such a batch is issued by its submit call).  Such merges SHARD THEIR REPLAY
 * (option "dist_shard_replay", default 1: rank r replays queries q = r (mod world); the heap shares' all-gather is issued by a later
 * submit call, or by collect).  qadc_search batches of that kind also SHARD THEIR FRONT (option "dist_shard_front", default 1): what is per query rather than per code — coarse
 * assignment, residual tables, pre-scan, select, quantizer — runs on rank r for queries [r * ceil(nq / world), ...) only, and
 * one more all-gather (issued by the submit call as well) ships assign[], the int8 tables and (flags, qmin, qmax) of every
 * query to every rank before the sharded scan.
 *   rank 0:      qadc_dist_unique_id(id)  ... ship the 128 bytes to the other ranks by any means ...
 *   every rank:  qadc_dist_init(idx, rank, world, id);  then per batch  qadc_query_scan_submit(...); qadc_dist_collect(...) */
#define QADC_DIST_ID_BYTES 128
int qadc_dist_unique_id(uint8_t* id128);
int qadc_dist_init(qadc_index* idx, int rank, int world, const uint8_t* id128);
int qadc_dist_collect(qadc_index* idx, int slot, uint32_t* keys, int8_t* values, int32_t* sizes, int32_t* status,
                      const float* extra, int extra_n, float* extra_out);
int qadc_dist_shutdown(qadc_index* idx);
/* The same merge over a caller-supplied all-gather instead of RCCL (no counterpart in the reference): `fn` gathers
 * bytes_per_rank bytes of DEVICE memory from every rank into d_recv[world][bytes_per_rank] (rank order), is called with
 * the producing work already enqueued on hip_stream, and must have completed (or be ordered on hip_stream) when it
 * returns 0; any other return value fails the collect on this rank.  Every rank must call it the same number of times
 * with the same size — qadc_dist_collect guarantees that, including on its retry and failure paths.  Uses: ranks that
 * share one GPU (a single-GPU box exercising world > 1), hosts without librccl, MPI or other fabrics. */
typedef int (*qadc_allgather_fn)(void* ctx, const void* d_send, void* d_recv, uint64_t bytes_per_rank, void* hip_stream);
int qadc_dist_init_transport(qadc_index* idx, int rank, int world, qadc_allgather_fn fn, void* ctx);
/* Measurement aid: ONE process stands in for rank `rank` of `world` — the transport copies this rank's block into every
 * slot of the gather, so the merge replays a world's worth of entries while only this rank's shard is scanned.  Results
 * are NOT the database's answers (every stream counts `world` times); tools/ivf_shard_sizes.py times one of 8 ranks' step
 * on one GPU this way. */
int qadc_dist_init_loopback(qadc_index* idx, int rank, int world);
/* Built-in transport for qadc_dist_init_transport: host-staged all-gather through a POSIX shared-memory segment `name`
 * ("/something", unique per run; rank 0 creates it, the others wait up to timeout_s seconds — 0 = 120 s — for it).
 * slot_bytes = largest block a rank may contribute (a gather beyond it fails on every rank alike).  Barriers time out
 * after timeout_s and poison the segment, so a missing rank turns into an error instead of a hang.
 *   qadc_shm_transport_open(name, rank, world, slot_bytes, timeout_s, &ctx);
 *   qadc_dist_init_transport(idx, rank, world, qadc_shm_transport_allgather, ctx);  ...  qadc_shm_transport_close(ctx);
 * _allgather_host exchanges host buffers (no GPU): the CPU-side test of the protocol. */
int qadc_shm_transport_open(const char* name, int rank, int world, uint64_t slot_bytes, double timeout_s, void** out_ctx);
int qadc_shm_transport_allgather(void* ctx, const void* d_send, void* d_recv, uint64_t bytes_per_rank, void* hip_stream);
int qadc_shm_transport_allgather_host(void* ctx, const void* send, void* recv, uint64_t bytes_per_rank);
int qadc_shm_transport_close(void* ctx);
const char* qadc_shm_transport_error(void);
/* The probed partitions of the batch last collected from `slot` (qadc_search_submit computes assign[] on the GPU;
 * qadc_dist_collect has no assign_out): assign_out [nq][ma]. */
int qadc_slot_assign(qadc_index* idx, int slot, int32_t* assign_out);
/* The int8 tables (QuantizerMAX<int8_t> output, db_query_4.cpp:277-284) of queries [q_first, q_first + q_count) of the
 * batch last collected from `slot`, [q_count][ma][M][16] — still resident on the GPU until the slot is submitted again.
 * qadc_search builds its float tables on the device and returns no tables; this is how a caller (the parity tests: the
 * reference's own scan_avx_4 on the same int8 tables) gets at them. */
int qadc_slot_qtables(qadc_index* idx, int slot, int q_first, int q_count, int8_t* out);
/* Size-balanced placement of whole partitions on `world` ranks (IVF option 1): partitions in descending
 * size order, each to the currently lightest rank (ties: lowest rank).  owner_out[p] = rank of partition p.  A rank adds
 * the partitions it owns in full and the others with local_n = 0 (starts replica only, qadc_index_add_partition_shard),
 * so partition numbering — and assign[] — is the same on every rank and the merge order (assign slot, rank, position)
 * degenerates to (assign slot, position).  Host-only. */
int qadc_place_partitions(int part_count, const uint32_t* sizes, int world, int32_t* owner_out);
/* The merge half of qadc_dist_collect on a caller-assembled gather result (host memory; `world` blocks of block_words
 * u64 each: [nq x {offset, count, flags, 0} as u32][entries = key | value << 32 | assign slot << 40]...): lets a single
 * GPU check the multi-rank replay order.  sizes[q] = -1 when a block reports an overflow / unordered query. */
int qadc_dist_merge_blocks(int device_id, int world, int nq, int ma, int R, const uint64_t* gathered, uint64_t block_words,
                           uint32_t* keys, int8_t* values, int32_t* sizes);
/* The host half of the same merge (few-query batches: every rank replays its share of the queries between two
 * all-gathers), executed for all `world` ranks in turn on the caller's thread — no GPU, no RCCL: the test hook of the
 * code path 2/4/8-rank runs of 32-query batches take. */
int qadc_dist_merge_blocks_host(int world, int nq, int ma, int R, const uint64_t* gathered, uint64_t block_words,
                                uint32_t* keys, int8_t* values, int32_t* sizes);

typedef struct qadc_profile {
    uint64_t scan_launches;   /* launches of the streaming int8 scan kernels (scan_i8_kernel, scan_i8_mq_kernel) */
    uint64_t scan_codes;      /* codes those launches scanned (algorithmic bytes = codes * M/2) */
    double scan_ms;           /* HIP-event time of those launches (one event pair per run of consecutive launches,
                                 i.e. including the ~2 us hand-over between them) */
    uint64_t small_launches;  /* launches of the small-run int8 scan kernel (scan_i8_small_kernel): counted, */
    uint64_t small_codes;     /* not event-timed (an event pair costs as much stream time as such a launch) */
    double small_ms;          /* always 0; per-kernel times of these launches come from rocprofv3 */
    uint64_t start_codes;     /* codes scanned by the float pre-scan */
    double start_ms;          /* float pre-scan + select + quantize, HIP-event duration */
    uint64_t candidates;      /* candidates returned by the device (before padding duplicates) */
    uint64_t regrows;         /* batches re-run because the candidate buffer overflowed */
    double host_replay_ms;    /* host wall time assembling the ordered candidate streams */
    double host_plan_ms;      /* host wall time planning + enqueueing batches */
    double host_heap_ms;      /* host wall time replaying streams through the heap */
    uint64_t host_sorted_queries; /* queries whose candidates the host had to sort (> 16384 candidates) */
    uint64_t mq_launches;     /* of scan_launches: multi-query launches (scan_i8_mq_kernel, 8 queries per pass) */
    uint64_t pass_codes;      /* codes the streaming launches READ: a run's codes once per query, or once per group
                                 of 8 queries in a multi-query launch (LDS row reads = pass_codes * M there) */
    uint64_t wgq_launches;    /* batches scanned by scan_query_kernel (one workgroup per query) */
    uint64_t wgq_queries;     /* queries in them */
    uint64_t wgq_codes;       /* codes they probed (algorithmic bytes = codes * M/2) */
    double wgq_ms;            /* HIP-event time of those launches */
    uint64_t wgq_front_cycles; /* shader cycles the query workgroups spent in pre-scan + select + quantizer (summed over queries) */
    uint64_t wgq_scan_cycles;  /* ... in the int8 scan */
    uint64_t wgq_sort_cycles;  /* ... and in the final candidate sort + ordered stream write */
    uint64_t head_launches;    /* level path: batches whose first bound levels were scanned by one head launch */
    uint64_t group_launches;   /* large IVF batches that took the partition-major second phase ... */
    uint64_t group_fallbacks;  /* ... and those of them whose candidate regions overflowed (redone on the level path) */
    /* the partition-major second phase in detail (profile on): HIP-event times of its three launches and the work in them */
    double group_head_ms;      /* scan_query_kernel in HEAD mode: front (pre-scan, select, quantizer) + the head probes */
    double group_scan_ms;      /* scan_i8_mq_kernel over the regrouped (query, probe) pairs */
    double group_order_ms;     /* order_cands_kernel */
    uint64_t group_head_codes; /* codes the heads walked (algorithmic HBM bytes = codes * M/2) */
    uint64_t group_pairs;      /* (query, probe) pairs of the second phase */
    uint64_t group_seats;      /* seats of their groups (8 per group, 4 for a narrow remainder group): fill = pairs / seats */
    uint64_t group_pass_codes8; /* codes read by 8-seat passes (LDS cycles = codes * M * 4 / 64) */
    uint64_t group_pass_codes4; /* ... by 4-seat passes (LDS cycles = codes * M * 2 / 64) */
    uint64_t group_batches;    /* batches the above figures cover */
    uint64_t front_sharded_batches; /* multi-GPU: qadc_search batches whose front ran on 1/world of the queries per rank */
    uint64_t dist_async_collects;   /* multi-GPU: qadc_dist_collect calls served by a merge enqueued with the batch (one event wait) */
    uint64_t lone_front_launches;   /* lone queries on one long partition whose front ran sliced over workgroups, in a launch of its own
                                       in front of the walk (counted with or without "profile") */
    uint64_t split_launches;        /* of scan_launches: launches of the split form (16x4 runs read from the byte-plane copy) */
    uint64_t split_codes;           /* codes those launches scanned (they read 7 bytes per code, plus byte 7 of the survivors) */
    uint64_t split_copy_bytes;      /* device bytes of the byte-plane copies qadc_index_finalize built (kept across resets) */
    uint64_t split_copy_failed;     /* partitions whose copy could not be allocated: their runs take the row-major form */
    uint64_t split6_launches;       /* of split_launches: launches of the 6-plane form (qadc_index_set_split6) */
    uint64_t split6_codes;          /* of split_codes: codes those scanned (6 bytes per code, plus one row-major line per survivor) */
    uint64_t split_survivors;       /* (code, query) pairs of the 6-plane launches whose 6-byte partial sum was below the bound,
                                       i.e. whose two deferred bytes were read (counted on the device, with "profile" on only) */
    uint64_t split5_launches;       /* of split_launches: launches of the 5-plane form (qadc_index_set_split5); a launch is counted
                                       here or under split6_*, never both */
    uint64_t split5_codes;          /* of split_codes: codes those scanned (5 bytes per code, plus one row-major line per survivor) */
    uint64_t split5_survivors;      /* (code, query) pairs of the 5-plane launches whose 5-byte partial sum was below the bound less
                                       the table's slack, i.e. whose three deferred bytes were read (with "profile" on only) */
    uint64_t nib_copy_bytes;        /* device bytes of the nibble-plane copies qadc_index_finalize built (8 per code; kept across resets) */
    uint64_t nib_copy_failed;       /* partitions whose nibble-plane copy could not be allocated: their runs take the other forms */
    uint64_t nib_launches;          /* of split_launches: launches of the nibble form that streamed 9 or 10 of the 16 sub-quantizers
                                       (qadc_index_set_split_nib); a launch is counted here, under nib8_*, split5_* or split6_*, never two */
    uint64_t nib_codes;             /* of split_codes: codes those scanned (4.5 or 5 bytes per code, plus one row-major line per survivor) */
    uint64_t nib_survivors;         /* (code, query) pairs of those launches whose partial sum was below the bound less the slack */
    uint64_t nib8_launches;         /* ... the same three for the launches that streamed 8 of 16 (4 bytes per code) */
    uint64_t nib8_codes;
    uint64_t nib8_survivors;
    uint64_t bkt_copy_bytes;        /* device bytes of the bucket copies qadc_index_finalize built (tiles and side arrays; kept across resets) */
    uint64_t bkt_copy_slots;        /* slots of those copies: codes plus padding (kept across resets) */
    uint64_t bkt_copy_failed;       /* partitions whose bucket copy could not be allocated: their runs take the other forms */
    uint64_t bkt_copy_padded_out;   /* partitions left without because padding inflated a block beyond bkt_max_pad x its codes */
    uint64_t bkt_launches;          /* of split_launches: launches of the bucket form (qadc_index_set_split_bkt); counted here and nowhere else */
    uint64_t bkt_codes;             /* of split_codes: codes their runs cover */
    uint64_t bkt_slots;             /* slots they streamed: those codes plus the padding copies */
    uint64_t bkt_survivors;         /* (slot, query) pairs of those launches whose partial sum was below the bound less the slack */
    uint64_t bkt4_launches;         /* of bkt_launches: those that paid for 4 of sub-quantizers 4-15 (host/level_plan.hpp: bkt_planes), */
    uint64_t bkt5_launches;         /* ... for 5, */
    uint64_t bkt6_launches;         /* ... for 6 */
    uint64_t bkt7_launches;         /* ... and for 7: the four add up to bkt_launches */
    uint64_t bktw_copy_bytes;       /* device bytes of the bucket copies' wide octaves (tiles and side arrays; kept across resets; not in bkt_copy_bytes) */
    uint64_t bktw_copy_slots;       /* slots of those octaves (kept across resets; not in bkt_copy_slots) */
    uint64_t bktw_copy_fallback;    /* octaves that padding inflated beyond bkt_wide_max_pad x their codes: stored as narrow blocks (kept across resets) */
    uint64_t bktw_launches;         /* of split_launches: launches of the wide form (qadc_index_set_split_bkt_wide); not in bkt_launches */
    uint64_t bktw_codes;            /* of split_codes: codes their runs cover */
    uint64_t bktw_slots;            /* slots they streamed */
    uint64_t bktw_survivors;        /* (slot, query) pairs of those launches whose partial sum was below the bound less the slack */
    uint64_t bktw3_launches;        /* of bktw_launches: those that paid for 3 of sub-quantizers 5-15 (host/level_plan.hpp: bktw_planes), */
    uint64_t bktw4_launches;        /* ... for 4, */
    uint64_t bktw5_launches;        /* ... for 5 */
    uint64_t bktw6_launches;        /* ... and for 6: the four add up to bktw_launches */
    uint64_t bktw_prune_skipped;    /* wide launches with the group test (qadc_index_set_bkt_prune): wave iterations (64 lane groups of 16 slots) that loaded no plane, */
    uint64_t bktw_prune_run;        /* ... wave iterations that ran (skipped + run = bktw_slots / 1024 of those launches) */
    uint64_t bktw_prune_groups;     /* ... and lane groups whose free rows reached the bound, in skipped and in run iterations */
    uint64_t bktw_prune_quarters;   /* ... with qadc_index_set_bkt_prune_lanes(16): aligned 16-lane quarters of the iterations that ran which loaded no plane */
} qadc_profile;

int qadc_profile_read(qadc_index* idx, qadc_profile* out);
int qadc_profile_reset(qadc_index* idx);

/* Split scan (16x4): qadc_index_finalize builds a byte-plane copy of code bytes 0-6 (7 bytes per code
 * held, padded to 16 Ki-code tiles) for every partition of at least min_codes codes (default 2^25; 0 = never), and the
 * one-query-per-pass level launches read it for their runs of at least min_run codes (default 2^23) that start on a tile.
 * min_codes must be set before qadc_index_finalize.  The copy is made from the codes as they are at finalize; partitions of
 * borrowed device codes (qadc_index_add_partition_device) get none.  Defaults: profiles/r07_split_sweep.txt. */
int qadc_index_set_split(qadc_index* idx, uint64_t min_codes, uint64_t min_run);

/* 6-plane form of the split scan: a split launch whose runs all have at least min_run6 codes streams
 * 6 of the copy's 7 planes; per query table, the byte whose pair-table entries are smallest is deferred together with byte 7
 * and read, from the row-major codes, for the survivors only.  It needs no memory beyond the copy and changes no result.
 * 0 = never.  May be set at any time; applies to batches submitted afterwards.  Default 2^25: profiles/r08_split6_sweep.txt. */
int qadc_index_set_split6(qadc_index* idx, uint64_t min_run6);

/* 5-plane form of the split scan: a split launch whose runs all have at least min_run5 codes streams
 * 5 of the copy's 7 planes and is preferred to the 6-plane form.  Per query table, two of the bytes 0..6 are deferred with
 * byte 7: the two whose pair-table entries rise least above their minimum.  The sum c of the three deferred pair tables'
 * minima is known before the scan and is a part of every code's sum, so only codes whose 5-byte partial sum is below
 * bound - c are survivors; they are finished with all 8 bytes and compared with the bound itself.  No memory beyond the
 * copy, no result changes.  0 = never.  May be set at any time; applies to batches submitted afterwards.  The
 * QADC_SPLIT5_MIN_RUN environment variable overrides the default at qadc_index_create.
 * Default 2^25: profiles/r09_split5_sweep.txt. */
int qadc_index_set_split5(qadc_index* idx, uint64_t min_run5);

/* Nibble form of the split scan (16x4): launches whose runs all have at least min_run codes stream ns = 9 or 10 of the 16
 * sub-quantizers (4.5 or 5 of the 8 code bytes) from a nibble-plane copy, those with at least min_run8 codes 8 of them; which
 * ones is chosen per table, byte 7's included, and the survivor test uses the deferred minima as the 5-plane form does.
 * Preferred over 5 planes where both qualify; no result changes.  0 = never.  qadc_index_finalize builds the nibble-plane
 * copy, 8 device bytes per code beside the byte-plane copy, for partitions of at least the smaller non-zero threshold in
 * force THEN: set the thresholds before finalize; afterwards they may be changed at any time, but partitions without the
 * copy keep the other forms.  QADC_NIB_MIN_RUN / QADC_NIB8_MIN_RUN / QADC_NIB_NS override the defaults at
 * qadc_index_create (with QADC_TEST_HOOKS=1).  Defaults: profiles/r10_nib_sweep.txt. */
int qadc_index_set_split_nib(qadc_index* idx, uint64_t min_run, uint64_t min_run8, int ns);

/* Bucket form of the split scan (16x4): qadc_index_finalize builds a bucket copy of every partition that
 * has a byte-plane copy and at least bkt_min_run codes (0 = the form is off, no copy).  The partition is cut into blocks of
 * bkt_block codes (a power of two from 16384 to 2^30; 0 = keep) and every block is stored grouped by its codes' first two bytes,
 * so that sub-quantizers 0-3 cost 2 bytes per 16 codes; the copy holds about 18.4 bytes per code (6.125 streamed planes, the
 * 8-byte code for survivors, a 4-byte position for candidates, 2 to 3 % padding on uniform codes).  A block whose slots exceed
 * bkt_max_pad x its codes (0 = keep; default 1.125) leaves its partition without the copy.  Level launches whose runs all have
 * at least bkt_min_run codes, start on a block and end on one or at the partition's end stream 7 of the other 12 sub-quantizers,
 * those of at least min_run6 / min_run5 / min_run4 codes 6 / 5 / 4 (0 = never); preferred over the nibble form; runs that do not
 * qualify keep the other forms, and no result changes.  The copy is built by qadc_index_finalize: turning the form on or off and
 * bkt_block must be set before; the thresholds may change at any time.  QADC_BKT_MIN_RUN / QADC_BKT6_MIN_RUN /
 * QADC_BKT5_MIN_RUN / QADC_BKT4_MIN_RUN override the defaults at qadc_index_create (with QADC_TEST_HOOKS=1).
 * Defaults: profiles/r11_bkt_ab.txt. */
int qadc_index_set_split_bkt(qadc_index* idx, uint64_t bkt_min_run, uint64_t bkt_block, uint64_t min_run6, uint64_t min_run5,
                             uint64_t min_run4, double bkt_max_pad);

/* Wide blocks of the bucket copy: positions from wide_block = W on (0 = none; a power of two, a multiple
 * of bkt_block; default 2^27) are stored in octave blocks [W 2^j, W 2^(j+1)), the last clipped at the partition's end, grouped by
 * the codes' first 20 bits, so that sub-quantizers 0-4 cost 3 bytes per 16 codes; 17.69 bytes per slot.  An octave whose
 * padded slots exceed wide_max_pad x its codes (0 = keep; default 1.08) keeps narrow blocks; a range stored wide has no narrow
 * blocks.  Level launches whose runs all have at least min_run codes, start on an octave, end on one or at the partition's end and
 * cover wide octaves only stream 6 of the other 11 sub-quantizers, those of at least min_run5 / min_run4 / min_run3 codes 5 / 4 / 3
 * (0 = never); preferred over the narrow form; no result changes.  The bucket form itself must be on (bkt_min_run != 0).
 * wide_block and wide_max_pad must be set before qadc_index_finalize; the thresholds may change at any time.  A bkt_block raised above
 * wide_block afterwards (qadc_index_set_split_bkt, or the env hooks) raises the octaves' start to bkt_block at finalize:
 * qadc_index_bktw_info reports the W in use.
 * QADC_BKT_WIDE_BLOCK / QADC_BKTW_MIN_RUN / QADC_BKTW5_MIN_RUN / QADC_BKTW4_MIN_RUN / QADC_BKTW3_MIN_RUN override the defaults at
 * qadc_index_create (with QADC_TEST_HOOKS=1).  Defaults: min_run = 2^27 and no other threshold (6 paid planes) since the group test
 * below: profiles/r13_prune_ab.txt (4 planes from 2^27 on before it: profiles/r12_bktw_ab.txt). */
int qadc_index_set_split_bkt_wide(qadc_index* idx, uint64_t wide_block, uint64_t min_run, uint64_t min_run5, uint64_t min_run4,
                                  uint64_t min_run3, double wide_max_pad);

/* Group test of the wide form ("pruned groups"): mode 1 = a wave iteration whose 64 lane groups all have
 * (their five free rows' entries) + (the paid rows' minima) >= bound - c loads no plane and looks nothing up; 0 = the form as it
 * was, the same kernels.  Exact for any codes and tables: no result, survivor count or candidate changes.  May be set at any time;
 * applies to batches submitted afterwards.  QADC_BKT_PRUNE overrides the default at qadc_index_create (with QADC_TEST_HOOKS=1).
 * Default 1: profiles/r13_prune_ab.txt. */
int qadc_index_set_bkt_prune(qadc_index* idx, int mode);

/* Granularity of the group test's loads ("pruned groups"; only with bkt_prune = 1): lanes 16 = in a wave
 * iteration that runs, an aligned 16-lane quarter (128 contiguous bytes of each plane) none of whose lane groups passes the test
 * loads no plane either; its lanes go through the pair loop with index 0, which cannot make a survivor of them.  64 = whole wave
 * iterations only.  Any other value: QADC_E_ARG.  Exact; no result, survivor count, candidate or other counter changes.  May be set at
 * any time.  QADC_BKT_PRUNE_LANES overrides the default at qadc_index_create (with QADC_TEST_HOOKS=1).
 * Default: profiles/r14_bkt_tiles_lanes.txt. */
int qadc_index_set_bkt_prune_lanes(qadc_index* idx, int lanes);

/* Tile order of the bucket launches, narrow and wide: mode 1 = a workgroup walks the run's tiles strided by the workgroups of the
 * run, whatever bit 3 (chunks) of the "variant" option says; 0 = they follow variant like every other streaming launch.  The copy
 * is key-ordered, so a chunk is one stretch of keys.  Any other value: QADC_E_ARG.  No result changes.  May be set at any time.
 * QADC_BKT_TILES overrides the default at qadc_index_create (with QADC_TEST_HOOKS=1).  Default: profiles/r14_bkt_tiles_lanes.txt. */
int qadc_index_set_bkt_tiles(qadc_index* idx, int mode);

/* The wide form's choice: out[16 t + 4 (NSP - 3) ..] = the deferred set among sub-quantizers 5-15 for NSP = 3, 4, 5, 6 paid
 * planes as a 16-bit mask (low byte first), the slack c, 0.  A diagnostic. */
int qadc_bktw_choice(int device_id, const int8_t* tables, int ntables, uint8_t* out);

/* Diagnostics of a partition's wide octaves: W (0 = none), octaves and slots; and the copy itself: octave_off [octaves + 1]
 * first slot of every octave (an octave without slots has narrow blocks), tiles [slots / 16384][93184] (11 nibble planes of
 * 8 KiB, sub-quantizers 5-15; 1024 uint16 ids; 1024 bytes, sub-quantizer 4), side as in qadc_index_bkt_read; each may be null. */
int qadc_index_bktw_info(qadc_index* idx, int part, uint64_t* wide_block, uint64_t* noctaves, uint64_t* slots);
int qadc_index_bktw_read(qadc_index* idx, int part, uint64_t* octave_off, uint8_t* tiles, uint8_t* side);

/* The bucket form's choice for ntables 16x4 int8 tables: out[16 t + 4 (NSP - 4) ..] = the deferred set among sub-quantizers
 * 4-15 for NSP = 4, 5, 6, 7 paid planes as a 16-bit mask (low byte first), the slack c, 0.  A diagnostic. */
int qadc_bkt_choice(int device_id, const int8_t* tables, int ntables, uint8_t* out);

/* Diagnostics of a partition's bucket copy: its block size (0 = no copy), blocks and slots; and the copy itself: block_off
 * [blocks + 1] first slot of every block, tiles [slots / 16384][100352] (12 nibble planes of 8 KiB, then 1024 uint16 ids), side
 * [slots / 16384][196608] (16384 8-byte codes, then 16384 uint32 positions, 0xffffffff = padding); each may be null. */
int qadc_index_bkt_info(qadc_index* idx, int part, uint64_t* block, uint64_t* nblocks, uint64_t* slots);
int qadc_index_bkt_read(qadc_index* idx, int part, uint64_t* block_off, uint8_t* tiles, uint8_t* side);

/* The nibble form's choice for ntables 16x4 int8 tables ([ntables][16][16]), as the device computes it for every table of
 * a batch: out[12 t + 4 (NS - 8) ..] = the deferred set of NS = 8, 9, 10 streamed sub-quantizers as a 16-bit mask (low byte
 * first), the slack c, 0.  A diagnostic: the scan never needs it from the caller. */
int qadc_nib_choice(int device_id, const int8_t* tables, int ntables, uint8_t* out);

/* ---------------------------------------------------------------------------------------------
 * Float ADC — the reference's OTHER query front end, db_query's plain scanner_simple
 * (db_query.cpp:17-46): over whole-byte PQ codes with scan_standard<uint8_t, NSQ> and
 * scan_standard<uint16_t, NSQ> (query_common.hpp:92-146) in a database of its own
 * (qadc_adc_index_create, qadc_adc_index_create16), and over the 4-bit
 * codes of a qadc_index with scan_4<M> (query_common.hpp:59-90) as a VIEW of that index
 * (qadc_adc_index_create_view), which reads the index's partitions in place.
 * A separate engine: it shares no state or option with qadc_index above.  Float tables come from
 * the caller, as scanner_simple receives them (qadc_adc_query_scan*), or are built on the GPU from
 * query vectors (qadc_adc_search*).  Candidates are summed in the grouping of the reference as
 * compiled (sum_mode 1) or in source order (sum_mode 0); DESIGN.md section 11.
 * ------------------------------------------------------------------------------------------- */
#define QADC_ADC_MAX_R 65536  /* largest heap capacity the qadc_adc_query_* calls take (larger R -> QADC_E_ARG) */
/* Candidate entries one qadc_adc_query_* call may hold on the device (12 bytes each).  Each query gets a region of
 * max(R, 512) + 32 R (levels - 1) + 4096 entries, at most its probed code count; a region that overflows is grown to hold
 * its query's whole candidate stream and the batch re-runs (a query whose scan order is sorted descending keeps every code).
 * A batch whose regions would exceed this many entries returns QADC_E_CAPACITY: split it. */
#define QADC_ADC_MAX_ENTRIES (1ull << 34)

/* Threading: one host thread at a time per index (its staging buffers and results belong to the index); several indexes
 * may be driven from several threads.  Every qadc_adc_* call selects the index's device and restores the calling thread's
 * current device before it returns. */

typedef struct qadc_adc_index qadc_adc_index;

/* scanner_simple::prepare_database + get_scan_func (db_query.cpp:21-24, query_common.hpp:120-146): sq_bits 8 with
 * sq_count 4, 8 or 16.  Anything else -> QADC_E_ARG with the reference's list of configurations (the 16-bit ones have a
 * constructor of their own, qadc_adc_index_create16; a 4-bit database is not uploaded a second time here: see
 * qadc_adc_index_create_view). */
int qadc_adc_index_create(qadc_adc_index** out, int sq_count, int sq_bits, int device_id);
/* The same for 16-bit sub-quantizers, scan_standard<uint16_t, NSQ>: sq_count 2, 4 or 8, 65536 centroids each.  Anything else ->
 * QADC_E_ARG with the reference's list of configurations.  The result is an ordinary owned index: every qadc_adc_* call that
 * takes one works on it, with the layouts scaled from 256 to 65536 centroids per sub-quantizer:
 *   codes      [n][sq_count] little-endian uint16, passed as bytes: rows of 2 * sq_count bytes (qadc_adc_index_add_partitions)
 *   tables     [nq][ma][sq_count * 65536] floats: 512 KiB, 1 MiB or 2 MiB per (query, probe) (qadc_adc_query_scan*, _search_tables)
 *   codebooks  [sq_count][65536][dim / sq_count] (qadc_adc_index_set_pq)
 *   the table budget counts sq_count * 256 KiB per (query, probe) (qadc_adc_index_set_table_budget)
 * sum_mode 1 is the grouping of the uint16_t instances as compiled (2: t0 + t1; 4 and 8: as the uint8_t instances), 0 the source
 * order.  The tables are not staged in LDS but read from global memory through the L2.
 * qadc_adc_encode16_host makes the codes from vectors (qadc_adc_encode_host is the 8-bit encoder). */
int qadc_adc_index_create16(qadc_adc_index** out, int sq_count, int device_id);
int qadc_adc_index_destroy(qadc_adc_index* idx);

/* db_query on the database db_query_4 has open: an ADC index that is a view of the finalized 4-bit index `src` — sq_count = M
 * (16 or 32), 4 bits, scan_4<M> (query_common.hpp:59-90, 121-125), on src's device, with src's all-or-none labels.  Nothing is
 * copied: the view snapshots src's partition table (device pointers, sizes, key_base) and its scans read src's codes and
 * labels where they lie, borrowed partitions (qadc_index_add_partition_device) included.  Keys are the label, else key_base +
 * position (scan_4's key where key_base is 0).
 *   src must be finalized (any keep) and hold every partition whole, on one GPU: an unfinalized or a sharded source ->
 *   QADC_E_ARG, the message says which.
 *   Every query call takes a view, with tables [nq][ma][M * 16] (table_dim = sq_count * 16): qadc_adc_query_scan, _device,
 *   _candidates, qadc_adc_index_set_finish, _reruns, _host_finishes, _set_table_budget; sum_mode 1 is scan_4's grouping as
 *   compiled, 0 its source order.  The qadc_adc_search* calls run src's quantizers (qadc_index_set_pq / _set_rotation /
 *   _set_coarse, codebooks [M][16][dim / M]) as they stand at the call, with the call's table_form and sum_mode; no set_pq on
 *   src -> QADC_E_ARG.  The table budget counts M * 16 * 4 bytes per (query, probe).
 *   qadc_adc_index_add_partitions, _set_pq, _set_rotation and _set_coarse on a view -> QADC_E_ARG.
 *   Lifetime: src counts its views.  qadc_index_destroy(src) with a live view -> QADC_E_ARG, src stays intact;
 *   qadc_adc_index_destroy of the view releases the count and frees only the view's own buffers.  Partitions added to src
 *   after the view was created are not seen by it.
 * A view's calls run on the view's own stream and touch no slot, option or profile of src. */
int qadc_adc_index_create_view(qadc_adc_index** out, qadc_index* src);

/* Append partitions as base_db::get_partition() yields them (databases.hpp:50-55): row-major codes [sizes[p]][sq_count]
 * (bytes; an index of qadc_adc_index_create16: little-endian 16-bit words, 2 * sq_count bytes per code),
 * labels[p] = u32[sizes[p]] or labels == NULL (key = position inside the partition, as scan_standard keys).  All-or-none
 * labels over every call and every non-empty partition (QADC_E_ARG otherwise); empty partitions are legal, their label
 * pointer may be NULL either way.  Host buffers are copied to the GPU. */
int qadc_adc_index_add_partitions(qadc_adc_index* idx, int part_count, const uint8_t* const* codes,
                                  const uint32_t* const* labels, const uint32_t* sizes);
int qadc_adc_index_partition_count(const qadc_adc_index* idx);
uint32_t qadc_adc_index_partition_size(const qadc_adc_index* idx, int part);
/* Diagnostics (no reference counterpart): how many query calls on this index were re-run because a candidate region overflowed. */
uint64_t qadc_adc_index_reruns(const qadc_adc_index* idx);

/* Where a query call is finished after its scan.  QADC_ADC_FINISH_HOST (the default): the kept candidates
 * come back to the host, which orders them and replays the heaps.  QADC_ADC_FINISH_DEVICE: qadc_adc_query_scan and qadc_adc_search
 * order and replay on the GPU and fetch only keys[nq][R], values[nq][R] and sizes[nq]; the arrays are the same bit for bit.  The
 * device replay keeps its heap in LDS and covers R <= 4096; a call with a larger R is finished on the host whatever the mode.
 * The *_candidates calls return the stream itself and are always finished on the host.  Any other mode -> QADC_E_ARG. */
#define QADC_ADC_FINISH_HOST 0
#define QADC_ADC_FINISH_DEVICE 1
int qadc_adc_index_set_finish(qadc_adc_index* idx, int mode);
/* Diagnostics: how many queries were finished on the host while the device finish was asked for (QADC_ADC_FINISH_DEVICE in force, or a
 * *_device call), since the index was created.  The length of a query's candidate stream never causes one; R > 4096 does. */
uint64_t qadc_adc_index_host_finishes(const qadc_adc_index* idx);

/* scanner_simple::query_scan (db_query.cpp:26-45) for nq queries:
 *   assign  [nq][ma]                   probed partitions, each in [0, partition_count); duplicates legal; 1 <= ma < 16384
 *   tables  [nq][ma][sq_count*256]     float tables, NOT mutated (a 16-bit index: [sq_count*65536]; a view: [sq_count*16])
 *   R                                  heap capacity, 1 .. QADC_ADC_MAX_R
 *   sum_mode                           1 = the reference's grouping as compiled, 0 = source order
 * Outputs (any may be NULL): keys[q][R], values[q][R], sizes[q] = the ARRAYS of the reference's
 * kv_binheap<unsigned,float>(R) after the query (R sentinel pushes (0, FLT_MAX - t) first, db_query.cpp:31-33).
 * A query may probe at most 2^32 - 1 codes in all.  QADC_E_CAPACITY: see QADC_ADC_MAX_ENTRIES.
 * A batch whose tables exceed the table budget (qadc_adc_index_set_table_budget) is scanned in sub-batches of whole queries, so
 * that the library never stages more than one sub-batch's tables, on the host or on the device. */
int qadc_adc_query_scan(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R,
                        int sum_mode, uint32_t* keys, float* values, int32_t* sizes);
/* The same with tables and outputs in device memory of the index's device: d_tables [nq][ma][sq_count*256] (as a kernel of the
 * caller left them: nothing is uploaded but assign, which stays host memory), d_keys [nq][R], d_values [nq][R], d_sizes [nq], all
 * required.  Always the device finish (a batch with R > 4096 is finished on the host and its arrays uploaded into the outputs).
 * Synchronous for the host: the inputs must be complete before the call; the outputs are complete on return, the index's stream
 * synchronised, so any stream may read them.  Arguments are checked and refused as by qadc_adc_query_scan. */
int qadc_adc_query_scan_device(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* d_tables, int R,
                               int sum_mode, uint32_t* d_keys, float* d_values, int32_t* d_sizes);
/* The ordered candidate stream instead: pushing (cand_keys[i], cand_vals[i]) for i in [offsets[q], offsets[q+1]) in
 * order into the reference's kv_binheap<unsigned,float>(R), after its R sentinel pushes, leaves it in exactly the state
 * the reference's scan would (a superset of its successful pushes, in scan order).  What a ScannerType wrapper pushes into
 * the caller's own heap (host/scanner_simple_hip.hpp).  offsets has nq + 1 entries.  cand_capacity = entries available in
 * cand_keys / cand_vals; if too small: QADC_E_CAPACITY, offsets filled, offsets[nq] = the entries needed (call again). */
int qadc_adc_query_scan_candidates(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables,
                                   int R, int sum_mode, uint64_t cand_capacity, uint32_t* cand_keys,
                                   float* cand_vals, uint64_t* offsets);

/* ---- float ADC from query vectors: the feeders of nns_engine(_batch)::process_query (query_common.hpp:194-213, 283-297) on
 * the GPU, so that no table crosses the bus.  assign_compute_residuals, rotate_multiple_vectors and the distance tables of
 * every (query, probe) are computed in device memory and scanned there. ---- */

/* base_pq with 8-bit sub-quantizers (quantizers.hpp:96-246): codebooks [sq_count][256][dim / sq_count] (a 16-bit index:
 * [sq_count][65536][dim / sq_count]), copied.  dim must be a
 * multiple of sq_count, at most 4096 (QADC_E_ARG otherwise).  A new dim drops the rotation and the coarse centroids. */
int qadc_adc_index_set_pq(qadc_adc_index* idx, int dim, const float* codebooks);
/* opq (quantizers.hpp:248-324): rotation [dim][dim], applied as rotate_multiple_vectors does (289-301):
 * rotated[r] = sum_c x[c] * rotation[r][c], one sequential float sum.  NULL = plain PQ.  After qadc_adc_index_set_pq. */
int qadc_adc_index_set_rotation(qadc_adc_index* idx, const float* rotation);
/* index_db's coarse centroids (databases.hpp:176-211): centroids [K][dim]; K must equal the partition count when a search
 * runs.  Not called, or K = 0: a flat index (flat_db::assign_compute_residuals, databases.hpp:93-101: every probe is
 * partition 0, the residual is the query).  After qadc_adc_index_set_pq. */
int qadc_adc_index_set_coarse(qadc_adc_index* idx, int K, const float* centroids);
/* Device memory for the tables of one pass, in bytes (default 1 GiB, the reference's TABLES_BUFFER_SIZE, query_common.hpp:147;
 * 0 = that default).  A batch whose tables need more is processed in sub-batches of whole queries, at least one query each;
 * no result depends on it.  It governs the tables qadc_adc_search* build and the caller's host tables qadc_adc_query_scan and
 * qadc_adc_query_scan_candidates upload; tables already in device memory (qadc_adc_query_scan_device) are read where they lie. */
int qadc_adc_index_set_table_budget(qadc_adc_index* idx, uint64_t bytes);

/* process_query + query_scan for nq queries [nq][dim]: find_k_neighbors(k = ma) on the coarse centroids (neighbors.cpp:30-76,
 * exact ties and NaN as the reference's heaps select them), residual, rotation, tables, scan.
 *   table_form  0 = direct (compute_dists_single_simd_cg, distances.hpp:294-311: what nns_engine builds for ma == 1),
 *               1 = BLAS expansion (compute_dists_multiple_blas_cg, 277-292: nns_engine for ma > 1, nns_engine_batch always),
 *               2 = nns_engine's rule (query_common.hpp:292-297)
 *   sum_mode    of the table sums, the coarse distances and the candidates alike
 * keys / values / sizes: exactly the outputs of qadc_adc_query_scan;  assign_out [nq][ma] (may be NULL): the probed
 * partitions, nearest first.  QADC_E_ARG: no qadc_adc_index_set_pq yet; K differs from the partition count; ma > K; a flat
 * index without a partition; a query whose coarse distances hold a NaN while ma > 256. */
int qadc_adc_search(qadc_adc_index* idx, int nq, const float* queries, int ma, int R, int table_form, int sum_mode,
                    uint32_t* keys, float* values, int32_t* sizes, int32_t* assign_out);
/* The same from and to device memory of the index's device: d_queries [nq][dim], d_keys [nq][R], d_values [nq][R], d_sizes [nq],
 * all required; no assign_out.  Always the device finish, synchronous for the host, as qadc_adc_query_scan_device; arguments are
 * checked and refused as by qadc_adc_search (the NaN row with ma > 256 included) and the table budget applies unchanged. */
int qadc_adc_search_device(qadc_adc_index* idx, int nq, const float* d_queries, int ma, int R, int table_form, int sum_mode,
                           uint32_t* d_keys, float* d_values, int32_t* d_sizes);
/* The same with the ordered candidate stream for output, as qadc_adc_query_scan_candidates returns it. */
int qadc_adc_search_candidates(qadc_adc_index* idx, int nq, const float* queries, int ma, int R, int table_form,
                               int sum_mode, uint64_t cand_capacity, uint32_t* cand_keys, float* cand_vals,
                               uint64_t* offsets, int32_t* assign_out);
/* Diagnostics: the feeders alone.  assign_out [nq][ma], tables_out [nq][ma][sq_count*256] (either may be NULL): what
 * qadc_adc_search scans, fetched to the host. */
int qadc_adc_search_tables(qadc_adc_index* idx, int nq, const float* queries, int ma, int table_form, int sum_mode,
                           int32_t* assign_out, float* tables_out);

/* Database build for 8-bit sub-quantizers, stateless: index_db::add_vectors' compute (databases.hpp:270-298) around
 * base_pq::encode_multiple_vectors (quantizers.hpp:222-245).  Per vector: with K > 0 find_k_neighbors(k = 1) on coarse [K][dim]
 * and the residual; the rotation if not NULL; per sub-quantizer the expansion distances to its 256 centroids and the pick of
 * the capacity-1 heap as compiled (the first smallest distance after the last NaN; 255 if distance 255 is NaN).
 * vectors [n][dim] -> codes [n][sq_count], assign_out [n] (may be NULL; written when K > 0).  sq_count 4, 8 or 16.
 * 8-bit only: the 16-bit sub-quantizers of qadc_adc_index_create16 have an encoder of their own, qadc_adc_encode16_host. */
int qadc_adc_encode_host(int sq_count, int dim, const float* codebooks, const float* rotation, int K, const float* coarse,
                         const float* vectors, uint64_t n, int sum_mode, int32_t* assign_out, uint8_t* codes, int device_id);

/* The same for 16-bit sub-quantizers: sq_count 2, 4 or 8, codebooks [sq_count][65536][dim / sq_count].  codes [n][sq_count]
 * little-endian uint16, passed as 2 * sq_count bytes per vector: the rows qadc_adc_index_add_partitions takes on an index of
 * qadc_adc_index_create16.  The coarse assignment, the residual, the rotation, assign_out and every refusal are those of
 * qadc_adc_encode_host (all arguments are checked before the device is touched).  Per (vector, sub-quantizer) the 65536
 * expansion distances — (||v||^2 + ||c||^2) + (-2 v.c), the entry qadc_adc_search_tables returns for table_form 1 under the same
 * sum_mode — go through find_k_neighbors(k = 1): one capacity-1 heap fed in centroid order over the 256 blocks of BLOCK_NEIGHS,
 * not reset between blocks, replace test as compiled !(s >= kept).  The code is the first smallest distance among the
 * centroids after the last NaN distance; 65535 if distance 65535 is NaN.
 * Block b is taken to be centroids 256 b .. 256 b + 255, as everywhere in this library (coarse assignment with K > 256): the
 * reference's text advances its neighbour pointer by block_count_neigh floats instead of rows (neighbors.cpp:64).
 * The call uploads, assigns, rotates and encodes in passes of QADC_ADC_ENCODE16_CHUNK vectors, so its device memory is bounded
 * by one pass and the codebooks (dim * 256 KiB) whatever n is; no result depends on the pass size. */
#define QADC_ADC_ENCODE16_CHUNK 262144   /* vectors encoded per pass; bounds the device memory of a call */
int qadc_adc_encode16_host(int sq_count, int dim, const float* codebooks, const float* rotation, int K, const float* coarse,
                           const float* vectors, uint64_t n, int sum_mode, int32_t* assign_out, uint8_t* codes, int device_id);

/* ---- db_add: vectors in, index grown, on the GPU.  The quantizers are those the index holds at the
 * call (qadc_adc_index_set_pq, _set_rotation, _set_coarse); an index of qadc_adc_index_create or _create16, never a view. ---- */

/* index_db::add_vectors (databases.hpp:270-298) on an index with a coarse quantizer (K > 0), flat_db::add_vectors (136-156) on
 * one without.  vectors [count][dim], host memory.
 *   K > 0: per vector find_k_neighbors(k = 1) on the coarse centroids, the residual, the rotation if one is set, the code —
 *     the steps and kernels of qadc_adc_encode_host / qadc_adc_encode16_host under the same sum_mode.  The code of vector i is
 *     appended to partition assign[i] with label labels_offset + i; within a partition the new rows stand in input order, after
 *     the rows already there.  The index holds 0 partitions (K empty ones are created) or exactly K, and is labelled or still
 *     undecided.
 *   K = 0: one partition, created if absent.  The code of vector i is written at row labels_offset + i; the partition's size
 *     becomes max(size, labels_offset + count), also for count 0; rows of a gap are zero bytes (std::vector::resize); rows that
 *     exist are overwritten.  The partition is unlabelled.
 * QADC_E_ARG, the message says which: a view; no set_pq yet; sum_mode not 0 or 1; vectors NULL with count > 0; labels_offset +
 * count above 2^32 - 1; a partition that would pass 2^32 - 1 codes; a partition count that is neither 0 nor K (flat: more than
 * one); unlabelled non-empty partitions with K > 0; labelled ones with K = 0.  The arguments are checked before the device is
 * touched, and a refused or failed call leaves the partitions and their contents as they were.
 * Synchronous, on the index's own stream: when it returns every query call sees the new rows.  The call works in passes of
 * QADC_ADC_ADD_CHUNK vectors, so its device scratch is bounded whatever count is; no result depends on the pass size. */
#define QADC_ADC_ADD_CHUNK 262144   /* vectors per pass; bounds the device memory of a call */
int qadc_adc_index_add_vectors(qadc_adc_index* idx, const float* vectors, uint64_t count, uint32_t labels_offset, int sum_mode);
/* The same with d_vectors [count][dim] in device memory of the index's device, complete before the call.  They are read where
 * they lie and only by kernels, so memory of another HIP runtime (a framework's tensor) is legal, as for qadc_adc_search_device. */
int qadc_adc_index_add_vectors_device(qadc_adc_index* idx, const float* d_vectors, uint64_t count, uint32_t labels_offset, int sum_mode);
/* qadc_adc_index_add_vectors with the caller's label of every vector (no reference counterpart: index_db::add_vectors numbers
 * them).  labels [count], host memory.  The index after the call is the index after qadc_adc_index_add_vectors(vectors, count,
 * labels_offset = 0, sum_mode) with the stored label i of every new row replaced by labels[i]: the same codes, partition sizes,
 * order within a partition, passes, relocations and reserve behaviour.  Any uint32_t is a label, 0xFFFFFFFF included, and labels
 * may repeat, as under qadc_adc_index_add_partitions (qadc_adc_index_remove_labels takes out every row that carries a label);
 * there is no labels_offset, so the bound labels_offset + count <= 2^32 - 1 is a bound on count alone.  The labels of a pass are
 * uploaded beside its vectors.
 * QADC_E_STATE, the index left as it was: an index without a coarse quantizer (K = 0) or one that holds unlabelled partitions —
 * its keys are positions.  Otherwise refused as qadc_adc_index_add_vectors is, with the same codes; labels NULL with count > 0 is
 * QADC_E_ARG. */
int qadc_adc_index_add_vectors_labelled(qadc_adc_index* idx, const float* vectors, const uint32_t* labels, uint64_t count, int sum_mode);
/* The same with d_vectors [count][dim] and d_labels [count] in device memory of the index's device, complete before the call.
 * Both are read where they lie and only by kernels (the labels by the scatter kernel of each pass), so memory of another HIP
 * runtime is legal. */
int qadc_adc_index_add_vectors_labelled_device(qadc_adc_index* idx, const float* d_vectors, const uint32_t* d_labels, uint64_t count,
                                               int sum_mode);
/* base_db::get_partition (databases.hpp:50-55) read back: rows [first, first + count) of partition `part` of an owned index,
 * however it was filled: codes_out [count][code bytes], labels_out [count] (either may be NULL; labels_out is filled only on a
 * labelled index).  A range outside the partition, a partition that does not exist, a view -> QADC_E_ARG. */
int qadc_adc_index_read_partition(qadc_adc_index* idx, int part, uint32_t first, uint32_t count, uint8_t* codes_out, uint32_t* labels_out);
/* std::vector::reserve on the partitions index_db::add_vectors pushes to (databases.hpp:291-297): capacities [part_count], in
 * codes, are minimum capacities of the first part_count partitions; empty partitions are created up to part_count on an index
 * that has fewer.  A capacity never shrinks.  qadc_adc_index_add_vectors writes in place while every partition it touches has
 * room, else it moves the whole database once into a layout where every partition holds at least 1.5 times its new size: after
 * a reserve of the final sizes a build never relocates. */
int qadc_adc_index_reserve(qadc_adc_index* idx, int part_count, const uint32_t* capacities);
/* Diagnostics (no reference counterpart; std::vector reallocates silently in databases.hpp:291-297): the qadc_adc_index_add_vectors
 * calls that had to move the database to grow it. */
uint64_t qadc_adc_index_relocations(const qadc_adc_index* idx);

/* ---- Reconstruction: PQ codes back to vectors, on the GPU.  No reference counterpart (the reference
 * never decodes), so every bit is defined here and pinned to a CPU twin, host/pq_decode.hpp pq_decode; the device equals it bit
 * for bit. ----
 *
 * Row i has the sub-quantizer codes code(i, m), m < sq_count, and with a coarse quantizer (K > 0) a partition p(i).
 *   1. Gather.  y[b] = codebooks[m][code(i, m)][b - m dsub], m = b / dsub, dsub = dim / sq_count: a copy, no arithmetic.  The code
 *      layouts are the encoders': sq_bits 4 packed nibbles [n][sq_count / 2], the even sub-quantizer in the low nibble; 8: bytes
 *      [n][sq_count]; 16: little-endian uint16 [n][sq_count].  Accepted (sq_count, sq_bits): 16 x 4, 32 x 4; 4 x 8, 8 x 8, 16 x 8;
 *      2 x 16, 4 x 16, 8 x 16.  codebooks [sq_count][2^sq_bits][dsub].
 *   2. Un-rotate.  With a rotation [dim][dim], z[c] = ONE float chain acc = fmaf(y[r], rotation[r][c], acc) over ascending r from
 *      0.0f: the transpose of the encoders' rotated[r] = sum_c x[c] rotation[r][c], hence the inverse for the orthogonal matrices the
 *      trainers return.  For any other matrix it is still exactly this chain (the transpose, not an inverse).  Without a rotation
 *      z = y bit for bit.  Consequence: under a rotation ONE NaN (or infinite: 0 * inf) component of y makes the whole row NaN,
 *      since every chain passes every component; without one only that component is NaN.
 *   3. Coarse centroid.  With K > 0, x[c] = z[c] + coarse[p(i)][c], one float add — the inverse of the encoder's
 *      x[d] - coarse[best][d]; with K = 0, x = z.
 *   4. Error (optional).  Given the originals v, err[i] = ONE chain acc = fmaf(d, d, acc), d = v[c] - x[c], over ascending c from
 *      0.0f: the k-means objective of row i.  No total is formed on the device (pyqadc.quant_error sums in float64, ascending i).
 * A MISSING row (below: a partition outside [0, K), a key no row holds) is 0x7FC00000 in every float of its out row; its err, where
 * asked for, follows from the chain (NaN).  NaN payloads: wherever arithmetic was done — steps 2, 3 and 4 — a NaN result is written
 * as 0x7FC00000 (payloads differ between processors); the copy of step 1 alone, no rotation and K = 0, keeps a centroid's bits.
 *
 * qadc_pq_decode_host: stateless, the inverse of qadc_ivf_encode_host, qadc_adc_encode_host and qadc_adc_encode16_host.
 *   assign [n] (the encoders' assign_out; read with K > 0 only), codes [n][code bytes], vectors [n][dim] (nullable: read for
 *   err_out only) -> out [n][dim], err_out [n] (nullable).  An assign entry outside [0, K) is not a refusal: that row is a missing
 *   row.  Works in passes of QADC_DECODE_CHUNK rows: the device scratch is bounded by one pass and the quantizers whatever n is, and
 *   no result depends on the pass size.  n = 0 is legal and touches nothing.  Synchronous.
 *   Refused with QADC_E_ARG before the first HIP call, the message naming the cause: a (sq_count, sq_bits) pair outside the list;
 *   dim not a positive multiple of sq_count; dim > 2048 at 4 bits, > 4096 at 8 and 16 bits (the encoders' limits); NULL codebooks;
 *   K < 0; NULL coarse or NULL assign with K > 0; NULL vectors with err_out given; NULL codes or out with n > 0.
 * qadc_pq_decode_device: d_assign, d_codes, d_vectors, d_out and d_err_out in device memory of device_id, read and written where
 *   they lie and only by kernels ("Device pointers of the caller" above: 4-byte aligned, d_codes 1 byte; a d_out on a 16-byte
 *   boundary with dim a multiple of 4 is written with 16-byte stores); every out float and err entry is written and no other
 *   byte.  codebooks, rotation and coarse are host memory. */
#define QADC_DECODE_CHUNK 262144   /* rows decoded per pass; bounds the device scratch of a call */
int qadc_pq_decode_host(int sq_count, int sq_bits, int dim, const float* codebooks, const float* rotation, int K, const float* coarse,
                        const int32_t* assign, const void* codes, uint64_t n, const float* vectors, float* out, float* err_out, int device_id);
int qadc_pq_decode_device(int sq_count, int sq_bits, int dim, const float* codebooks, const float* rotation, int K, const float* coarse,
                          const int32_t* d_assign, const void* d_codes, uint64_t n, const float* d_vectors, float* d_out, float* d_err_out,
                          int device_id);
/* qadc_adc_index_reconstruct: the vectors behind keys.  The KEY of a row is what the scan emits for it: the label on a labelled
 *   index, else key_base + position (an owned index: the position), so the keys of qadc_adc_search* can be fed back unchanged.
 *   keys [count] -> out [count][dim], where_out [count] (nullable): ((uint64)partition << 32) | row of the row taken.  On an owned
 *   8-bit or 16-bit index and on a view of a 4-bit index (which reads the source's partitions in place).  The quantizers are those
 *   the index holds at the call, on a view the source's, as for qadc_adc_search*; with K > 0 a row's coarse centroid is its
 *   partition's.  A key held by several rows (labels may repeat; unlabelled partitions share positions) takes the row with the
 *   smallest (partition, row); repeats in keys each get their row; a key no row holds is a missing row, its where_out
 *   QADC_RECONSTRUCT_MISSING.  Filters set on the index are ignored — a lookup, not a search — and nothing in the index changes.
 *   How: a bitmap over [min key, max key] (at most 512 MiB, as for qadc_adc_index_remove_labels), one pass over the index's keys in
 *   which a marked row finds its key among the sorted distinct requested keys and lowers that key's slot with a 64-bit atomicMin
 *   (the minimum makes the result independent of scheduling), then the found rows' codes are gathered into a pass of
 *   QADC_DECODE_CHUNK rows and decoded by qadc_pq_decode_device's kernels.  The distinct keys are ordered on the host.
 *   Refused with QADC_E_ARG before the device is touched: a null index; no set_pq (a view: on its source); a coarse K that is
 *   neither 0 nor the partition count; a dim above the decoder's limit; NULL keys or out with count > 0; count >= 2^32; more than
 *   65535 partitions.  count = 0 is legal.  Synchronous, on the index's own stream; selects and restores the device.
 * qadc_adc_index_reconstruct_device: d_keys, d_out and d_where_out (4-byte aligned, all three) in device memory of the index's device, read
 *   and written by kernels only; every out float and where entry is written, missing rows included, and no other byte.
 * qadc_adc_index_reconstruct_rows / _device: rows [first, first + count) of partition `part`, no lookup -> out [count][dim].  A
 *   range outside the partition or a partition that does not exist is QADC_E_ARG, as for qadc_adc_index_read_partition; on a view
 *   too.
 * Not done: removing or overwriting by reconstruction; sharded or multi-GPU indexes (a view of one cannot be created); an error
 * total on the device; the shortcut for a single unlabelled partition (it takes the general pass). */
#define QADC_RECONSTRUCT_MISSING (~0ull)
int qadc_adc_index_reconstruct(qadc_adc_index* idx, const uint32_t* keys, uint64_t count, float* out, uint64_t* where_out);
int qadc_adc_index_reconstruct_device(qadc_adc_index* idx, const uint32_t* d_keys, uint64_t count, float* d_out, uint64_t* d_where_out);
int qadc_adc_index_reconstruct_rows(qadc_adc_index* idx, int part, uint32_t first, uint32_t count, float* out);
int qadc_adc_index_reconstruct_rows_device(qadc_adc_index* idx, int part, uint32_t first, uint32_t count, float* d_out);

/* ---- db_add on the 4-bit index: vectors in, index grown, on the GPU.  The quantizers are those the
 * index holds at the call (qadc_index_set_pq, _set_rotation, _set_coarse). ---- */

/* index_db::add_vectors (databases.hpp:270-298) on an index with a coarse quantizer (K > 0), flat_db::add_vectors (136-156) on
 * one without.  vectors [count][dim], host memory.
 *   K > 0: per vector find_k_neighbors(k = 1) on the coarse centroids, the residual, the rotation if one is set, the 4-bit code:
 *     the steps and kernels of qadc_ivf_encode_host_mode(encode_form = 1, sum_mode).  The code of vector i is appended to
 *     partition assign[i] with label labels_offset + i; within a partition the new rows stand in input order, behind the rows
 *     already there.  The index holds 0 partitions (K empty ones are created) or exactly K, and is labelled or still undecided.
 *     A call of n vectors equals any split of it into calls.
 *   K = 0: one unlabelled partition, created if absent.  The code of vector i is written at row labels_offset + i; the size
 *     becomes max(size, labels_offset + count), also for count 0; rows of a gap are zero bytes; rows that exist are overwritten.
 * The call leaves the index not finalized, as every qadc_index_add_* does: call qadc_index_finalize again before querying.
 * QADC_E_STATE while a submission slot is busy.  QADC_E_ARG, the message says which: no set_pq yet; sum_mode not 0 or 1; vectors
 * NULL with count > 0; labels_offset + count above 2^32 - 1; a partition that would pass 2^32 - 1 codes; a partition count that
 * is neither 0 nor K (flat: more than one); unlabelled non-empty partitions with K > 0; labelled ones with K = 0; a live float-ADC
 * view (qadc_adc_index_create_view: it keeps the partitions' addresses, which a relocation changes); an index under
 * qadc_dist_init, or one holding a shard or a starts replica; a borrowed partition (qadc_index_add_partition_device); a vector
 * assigned outside [0, K).  The arguments are checked before the device is touched, and a refused call leaves the partitions and
 * their contents as they were.  A call that fails later (a HIP error, no memory for a relocation or for a pass) leaves every
 * partition with the number of rows it held and, with a coarse quantizer, with their contents: it only ever wrote behind them.
 * Without one (K = 0) rows that existed and that the call was to overwrite may already hold the new codes.  Such a failed call may
 * have moved the partitions or changed their rows, and then leaves the index not finalized: call qadc_index_finalize before the
 * next query, as after a call that succeeded.
 * Synchronous, on the index's scan stream, in passes of QADC_INDEX_ADD_CHUNK vectors: the device scratch of a call is bounded
 * whatever count is, and no result depends on the pass size.
 * Storage: the first call moves partitions that qadc_index_add_partitions / _interleaved / _synthetic allocated one by one into
 * one arena of the index and frees them; an append that fits its partition's capacity writes in place, otherwise the whole
 * database moves once into an arena where every partition holds 1.5 times its new size.  While it moves, the device holds the
 * old and the new database at once. */
#define QADC_INDEX_ADD_CHUNK 262144   /* vectors per pass; bounds the device memory of a call */
int qadc_index_add_vectors(qadc_index* idx, const float* vectors, uint64_t count, uint32_t labels_offset, int sum_mode);
/* The same with d_vectors [count][dim] in device memory of the index's device, complete before the call.  They are read where
 * they lie and only by kernels, so memory of another HIP runtime (a framework's tensor) is legal. */
int qadc_index_add_vectors_device(qadc_index* idx, const float* d_vectors, uint64_t count, uint32_t labels_offset, int sum_mode);
/* qadc_index_add_vectors with the caller's label of every vector, as qadc_adc_index_add_vectors_labelled: labels [count], host
 * memory; the index after the call is the index after qadc_index_add_vectors(vectors, count, 0, sum_mode) with the stored label i
 * of every new row replaced by labels[i].  Any uint32_t is a label and labels may repeat.  The call leaves the index not finalized,
 * as the plain call does.  QADC_E_STATE on an index without a coarse quantizer or with unlabelled partitions (its keys are
 * positions), the index left as it was, finalized if it was; otherwise refused as qadc_index_add_vectors is, with the same codes. */
int qadc_index_add_vectors_labelled(qadc_index* idx, const float* vectors, const uint32_t* labels, uint64_t count, int sum_mode);
/* The same with d_vectors and d_labels [count] in device memory of the index's device, read where they lie and only by kernels. */
int qadc_index_add_vectors_labelled_device(qadc_index* idx, const float* d_vectors, const uint32_t* d_labels, uint64_t count, int sum_mode);
/* base_db::get_partition (databases.hpp:50-55) read back: rows [first, first + count) of partition `part`, however it was filled,
 * as long as it is held whole: codes_out [count][M / 2], labels_out [count] (either may be NULL; labels_out is filled only on a
 * labelled index).  A range outside the partition, a partition that does not exist, a shard -> QADC_E_ARG. */
int qadc_index_read_partition(qadc_index* idx, int part, uint32_t first, uint32_t count, uint8_t* codes_out, uint32_t* labels_out);
/* std::vector::reserve on the partitions index_db::add_vectors pushes to (databases.hpp:291-297): capacities [part_count], in
 * codes, are minimum capacities of the first part_count partitions; empty partitions are created up to part_count on an index
 * that has fewer.  A capacity never shrinks.  After a reserve of the final sizes a build never relocates.  Refused as
 * qadc_index_add_vectors is (busy slots, views, multi-GPU, shards, borrowed partitions).  A reserve that moves the partitions
 * leaves the index not finalized. */
int qadc_index_reserve(qadc_index* idx, int part_count, const uint32_t* capacities);
/* Diagnostics (std::vector reallocates silently in databases.hpp:291-297): the qadc_index_add_vectors calls that had to move the
 * database to grow it. */
uint64_t qadc_index_relocations(const qadc_index* idx);

/* ---- remove by label: vectors out, partitions compacted in place on the GPU.  No reference counterpart:
 * its index_db only ever push_backs (databases.hpp:270-298).  After a removal the index is the index that would have been built
 * had the removed vectors never been added, so every query returns what a freshly built index returns, bit for bit. ---- */

/* Removes every row whose label is in labels [count] (host memory) from whichever partitions hold it: all rows of a label that
 * was added more than once go; duplicates in the list and labels the index does not hold are ignored.  *removed_out (may be
 * NULL) = the rows removed.  The survivors of a partition keep their relative order and move to the front of its region;
 * capacities, offsets and buffers are unchanged, nothing relocates (qadc_adc_index_relocations does not move), and a later
 * qadc_adc_index_add_vectors that fits the freed room appends in place.
 * QADC_E_ARG, the message says which, checked before the device is touched, the index left as it was: idx NULL; labels NULL with
 * count > 0; an index that holds rows and is not labelled (a flat index, unlabelled qadc_adc_index_add_partitions: it keys its
 * vectors by position); a view (remove on the 4-bit index it views, after destroying the view).  count = 0, and a list that hits
 * no row, change nothing: no byte of the database is written.
 * Synchronous, on the index's own stream; every copy and memset of the call is asynchronous on that stream.  The call allocates a
 * bitmap over [smallest label of the list, largest label]: at most 2^32 bits, 512 MiB, freed before it returns.
 * QADC_E_HIP: a failure before the compaction started leaves the index as it was; after it started the contents of the partitions
 * that hold a listed label are unspecified, their sizes are the old ones (sizes are committed only when the compaction has
 * completed), and the index should be rebuilt. */
int qadc_adc_index_remove_labels(qadc_adc_index* idx, const uint32_t* labels, uint64_t count, uint64_t* removed_out);
/* The same with d_labels [count] in device memory of the index's device, complete before the call: read where they lie and only
 * by kernels, so memory of another HIP runtime (a framework's tensor — the keys qadc_adc_search_device returned) is legal.  The
 * span of the list is known only after a reduction kernel has run (one synchronise more than the host form), so a bitmap that
 * cannot be allocated is refused (QADC_E_HIP) after the device was touched; no row is touched by then. */
int qadc_adc_index_remove_labels_device(qadc_adc_index* idx, const uint32_t* d_labels, uint64_t count, uint64_t* removed_out);
/* qadc_adc_index_remove_labels on the 4-bit index, over its partitions where they lie — in the arena of an index that has grown,
 * or in the allocations qadc_index_add_partitions made.  Nothing moves between regions: qadc_index_relocations does not move, and a
 * later qadc_index_add_vectors that fits the freed room of an arena appends in place.
 * A call that removed at least one row leaves the index not finalized (the start sizes, the partition table and the byte-plane
 * copies describe the old rows): call qadc_index_finalize before the next query.  Behind every touched partition's new last row
 * the bytes [n * M/2, align16(n * M/2) + 64) are zero, as qadc_index_add_partitions and qadc_index_add_vectors leave them.
 * count = 0, and a list that hits no row, change nothing: a finalized index stays finalized and answers queries.
 * Refused before the device is touched, the index left as it was: what qadc_adc_index_remove_labels refuses, and what
 * qadc_index_add_vectors refuses of a growing call, with the same codes — QADC_E_STATE while a submission slot is busy;
 * QADC_E_ARG for a live float-ADC view, an index under qadc_dist_init, a shard or a starts replica, a borrowed partition.
 * QADC_E_HIP as above; after a failure behind the start of the compaction the index is left not finalized. */
int qadc_index_remove_labels(qadc_index* idx, const uint32_t* labels, uint64_t count, uint64_t* removed_out);
/* The same with d_labels [count] in device memory of the index's device, as qadc_adc_index_remove_labels_device. */
int qadc_index_remove_labels_device(qadc_index* idx, const uint32_t* d_labels, uint64_t count, uint64_t* removed_out);

/* ---- filtered float-ADC search: allow and exclude key sets ----
 * The KEY of a row is what the scan emits for it: labels[i] on a labelled partition, else key_base + position (key_base 0 on an
 * owned index; a view's qadc_index_set_key_base).  A filter is a set S of keys and a mode:
 *   QADC_ADC_FILTER_EXCLUDE  a row is dropped iff its key is in S      (tombstones, "not these ids", access control)
 *   QADC_ADC_FILTER_ALLOW    a row is dropped iff its key is not in S  ("only among these ids")
 * With a filter set on an index, every scanning call — qadc_adc_query_scan, _query_scan_device, _query_scan_candidates, qadc_adc_search,
 * _search_device, _search_candidates — returns what scanner_simple::query_scan (db_query.cpp:26-45) returns over partitions from which
 * the dropped rows have been deleted, the surviving rows' keys given as labels: in the loops of scan_standard (query_common.hpp:92-118)
 * and scan_4 (59-90) a dropped row is skipped before `candidate < min` is looked at, so it is never pushed and never lowers min for a
 * later row.  On a labelled index under EXCLUDE these are the arrays after qadc_adc_index_remove_labels of S, with the index untouched.
 * The *_candidates calls return the reference's pushes on that reduced database (a superset of them, as without a filter), in scan
 * order.  qadc_adc_search_tables does not scan and is unaffected.  Every code is still read: a filter saves no scan time, and a very
 * selective ALLOW set costs a full scan and a label read per row until R survivors have been seen. */
#define QADC_ADC_FILTER_EXCLUDE 0
#define QADC_ADC_FILTER_ALLOW 1
typedef struct qadc_adc_filter qadc_adc_filter;
/* A filter over keys [count] in host memory, on device_id: a bitmap over [lo, hi] of the keys in device memory (one bit per key of the
 * span: at most 512 MiB, the whole key space), built on the GPU from the list uploaded once.  Duplicates are legal.  count = 0 is legal
 * (keys may be NULL then): EXCLUDE of nothing filters nothing, ALLOW of nothing lets no row pass and every heap holds its R sentinels, as
 * the reference's on empty partitions.  The filter is immutable and independent of any index; the call is synchronous.
 * QADC_E_ARG before the device is touched: out NULL, a mode other than the two, keys NULL with count > 0.  QADC_E_HIP: the bitmap or
 * the list could not be allocated; nothing is left behind. */
int qadc_adc_filter_create(qadc_adc_filter** out, int mode, const uint32_t* keys, uint64_t count, int device_id);
/* The same with d_keys [count] in device memory of device_id, complete before the call: read where they lie and only by kernels, so
 * memory of another HIP runtime (the keys qadc_adc_search_device returned) is legal.  lo and hi come from a reduction kernel and one
 * synchronise more than the host form. */
int qadc_adc_filter_create_device(qadc_adc_filter** out, int mode, const uint32_t* d_keys, uint64_t count, int device_id);
/* What the filter holds (any output may be NULL): its mode, the smallest and largest key of the set (an empty set: lo = 2^32 - 1,
 * hi = 0) and the bytes of its bitmap, 4 * ceil((hi - lo + 1) / 32) (an empty set: 4). */
int qadc_adc_filter_info(const qadc_adc_filter* f, int* mode, uint32_t* lo, uint32_t* hi, uint64_t* bitmap_bytes);
/* Frees the filter.  QADC_E_STATE while it is set on an index (the filter stays intact); NULL is a no-op. */
int qadc_adc_filter_destroy(qadc_adc_filter* f);
/* Sets the filter every later scanning call of idx applies (an owned 8-bit or 16-bit index, or a view), or clears it (f NULL: the
 * calls return what they returned before, bit for bit).  The index counts a use on the filter until it is cleared, replaced or the
 * index destroyed; one filter may be set on several indexes of its device.  Applied in the scan kernel in front of the emit of every
 * level launch, so levels, bounds, re-runs, sub-batches and both finishes (qadc_adc_index_set_finish) hold as they are on the reduced
 * database.  qadc_adc_index_add_vectors* and _remove_labels* are legal while a filter is set: the filter is about keys, not rows, and
 * stays as it is.  QADC_E_ARG: idx NULL, a filter of another device.  This filter holds for every query of a batch; the *_filtered
 * calls below add one per query and compose with it.  Not on the int8 4-bit engine (qadc_query_scan, qadc_search), whose users filter
 * through a view (qadc_adc_index_create_view). */
int qadc_adc_index_set_filter(qadc_adc_index* idx, const qadc_adc_filter* f);

/* ---- one filter per query of a batch ----
 * The _filtered form of a scanning call takes the arguments of its plain form and filters [nq] in HOST memory (in the _device forms
 * too: the call uploads one small table entry per query next to assign), filters[q] the filter of query q or NULL for none.  A row is
 * emitted for query q iff it passes the index's filter (qadc_adc_index_set_filter), if one is set, AND filters[q], if that is not NULL:
 * for every query the outputs are those of the definition above on the partitions from which the rows dropped for THAT query have been
 * deleted — the standing use is an index-wide EXCLUDE of tombstones with a per-query ALLOW of a tenant's keys.  One filter may stand at
 * any number of positions; both modes and empty sets mix freely in a batch.  filters NULL, or every entry NULL, is the plain call: the
 * same kernels are launched and the same outputs returned, bit for bit.  The calls are synchronous and take no use count: a filter
 * need only stay alive for the call, and qadc_adc_filter_destroy never fails because of one.  Levels, bounds, re-runs, sub-batches of
 * the table budget and both finishes hold per query as they are; qadc_adc_index_add_vectors* and _remove_labels* between calls are
 * legal.  QADC_E_ARG before the first HIP call: an entry that is not NULL and lies on another device than the index; every other
 * argument is checked and refused as by the plain form.  Every code is still read, nq distinct wide filters are nq bitmaps in device
 * memory (they are the caller's), and there is no such form on the int8 4-bit engine or on sharded / multi-GPU indexes. */
int qadc_adc_query_scan_filtered(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R, int sum_mode,
                                 uint32_t* keys, float* values, int32_t* sizes, const qadc_adc_filter* const* filters);
/* qadc_adc_query_scan_device with filters [nq] (host memory). */
int qadc_adc_query_scan_device_filtered(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* d_tables, int R,
                                        int sum_mode, uint32_t* d_keys, float* d_values, int32_t* d_sizes,
                                        const qadc_adc_filter* const* filters);
/* qadc_adc_query_scan_candidates with filters [nq]: every query's stream holds the pushes on the database reduced for that query. */
int qadc_adc_query_scan_candidates_filtered(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R,
                                            int sum_mode, uint64_t cand_capacity, uint32_t* cand_keys, float* cand_vals,
                                            uint64_t* offsets, const qadc_adc_filter* const* filters);
/* qadc_adc_search with filters [nq]; filters[q] belongs to queries[q] whatever sub-batches the table budget cuts the call into. */
int qadc_adc_search_filtered(qadc_adc_index* idx, int nq, const float* queries, int ma, int R, int table_form, int sum_mode,
                             uint32_t* keys, float* values, int32_t* sizes, int32_t* assign_out, const qadc_adc_filter* const* filters);
/* qadc_adc_search_device with filters [nq] (host memory). */
int qadc_adc_search_device_filtered(qadc_adc_index* idx, int nq, const float* d_queries, int ma, int R, int table_form, int sum_mode,
                                    uint32_t* d_keys, float* d_values, int32_t* d_sizes, const qadc_adc_filter* const* filters);
/* qadc_adc_search_candidates with filters [nq]. */
int qadc_adc_search_candidates_filtered(qadc_adc_index* idx, int nq, const float* queries, int ma, int R, int table_form, int sum_mode,
                                        uint64_t cand_capacity, uint32_t* cand_keys, float* cand_vals, uint64_t* offsets,
                                        int32_t* assign_out, const qadc_adc_filter* const* filters);

/* ---- range search: every row within a radius, sorted on the GPU ----
 * The other query of a PQ index: for query q, every row of its probed partitions that passes the filters and whose candidate — the
 * float sum query_scan compares with the heap's maximum, same grouping, same sum_mode — is < radius[q] as a float compare.  A NaN
 * candidate or a NaN radius keeps nothing, radius +inf keeps every candidate but NaN and +inf, a candidate equal to the radius is not
 * kept.  Query q's rows are ordered ascending by the 64-bit word (image(candidate) << 32) | key, image = the order-preserving integer
 * image of a float (-0 before +0); nothing is deduplicated, and two rows with the same key and candidate are both present.  There is no
 * R, no heap and no cap on a query's rows.  The written definition is scanner_simple::range_scan (quick-adc_amd/host/scanner_simple.hpp),
 * to which every output is held bit for bit.
 *   radius [nq], filters [nq], lims [nq + 1]   HOST memory in every form.  filters may be NULL and may hold NULL entries; it composes
 *                                              with qadc_adc_index_set_filter as in the _filtered calls above.
 *   lims                                       out: query q's rows are [lims[q], lims[q + 1]) of the held result; lims[nq] = its rows.
 * The result stays ON THE INDEX, in device memory no other call writes, until the next range call (which drops it, also when it fails)
 * or qadc_adc_index_destroy; qadc_adc_range_collect* copies it out, any number of times, and query_scan / search / add / remove calls
 * in between leave it as it is.  The calls are synchronous.  Each pass (the whole call, or a sub-batch of the table budget) scans
 * once with a region of min(probed codes, 4096) entries per query and, where a region overflowed, a second time with regions of exactly
 * the counted sizes (counted in qadc_adc_index_reruns).  Works on 8-bit, 16-bit and view indexes.  QADC_E_ARG as the plain calls, and
 * for radius or lims NULL or a filter of another device; QADC_E_CAPACITY when the regions of one pass exceed QADC_ADC_MAX_ENTRIES. */
#define QADC_ADC_RANGE_SORT_LDS 4096   /* a query's rows up to this many are sorted in LDS, more by radix passes through device memory */
/* tables [nq][ma][table floats] in host memory, as qadc_adc_query_scan takes them. */
int qadc_adc_range_scan(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, const float* radius, int sum_mode,
                        const qadc_adc_filter* const* filters, uint64_t* lims);
/* d_tables in device memory, as qadc_adc_query_scan_device takes them. */
int qadc_adc_range_scan_device(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* d_tables, const float* radius,
                               int sum_mode, const qadc_adc_filter* const* filters, uint64_t* lims);
/* From query vectors (host memory), tables built on the GPU as qadc_adc_search builds them; assign_out [nq][ma] may be NULL. */
int qadc_adc_range_search(qadc_adc_index* idx, int nq, const float* queries, int ma, const float* radius, int table_form, int sum_mode,
                          const qadc_adc_filter* const* filters, int32_t* assign_out, uint64_t* lims);
/* d_queries in device memory; assign_out is host memory and may be NULL. */
int qadc_adc_range_search_device(qadc_adc_index* idx, int nq, const float* d_queries, int ma, const float* radius, int table_form,
                                 int sum_mode, const qadc_adc_filter* const* filters, int32_t* assign_out, uint64_t* lims);
/* Copies the held result into keys / values [capacity] (host memory).  QADC_E_CAPACITY when capacity < lims[nq]: nothing is copied
 * and the result stays held.  QADC_E_STATE when no result is held. */
int qadc_adc_range_collect(qadc_adc_index* idx, uint64_t capacity, uint32_t* keys, float* values);
/* The same into device memory, copied by a kernel (the buffers may belong to another copy of the HIP runtime). */
int qadc_adc_range_collect_device(qadc_adc_index* idx, uint64_t capacity, uint32_t* d_keys, float* d_values);

/* ---- exact re-ranking: the vectors on the GPU, candidates reordered by L2 ----
 * Both engines rank by a quantized distance.  A refine store keeps the original vectors in device memory, and a rerank call reorders
 * the candidate keys a search returned — with a larger R than wanted — by the true squared L2 distance to those vectors.  The store
 * belongs to no index: it consumes uint32 keys, whoever produced them, and is DENSE over a key range: row r holds the vector of key
 * lo + r, which is how qadc_adc_index_add_vectors and qadc_index_add_vectors label (labels_offset + i) and how a flat index's
 * position keys run.  Everything below is held, bit for bit, to the host twin quick-adc_amd/host/refine.hpp:
 *   distance   D(q, x) in binary32, every operation rounded by itself, no fused multiply-add: 64 partial sums p[l] over the
 *              components 64 j + l in ascending j (t = q[i] - x[i]; p[l] = p[l] + t * t), then p[l] = p[l] + p[l + s] for l < s at
 *              s = 32, 16, 8, 4, 2, 1; D = p[0].  A row of an F16 store is the float value of the stored half, the stored half the
 *              round-to-nearest-even conversion of the input float (subnormals kept, overflow to +-inf).
 *   selection  of keys[q][0 .. count_q): an entry is skipped where values are given and values[q][i] == FLT_MAX (the float-ADC heap's
 *              sentinel), missing (dropped, counted) where its key is outside [lo, lo + rows); the others are ordered ascending by
 *              (distance, key) — a NaN distance behind +inf, returned as 0x7FC00000 — a key listed several times kept once, and the
 *              first min(R, survivors) come out; the slots behind out_sizes[q] hold key 0xFFFFFFFF and distance +inf.
 * The output is a sorted list, not a heap array, and depends only on the set of candidate keys.  Limits: keys dense from lo; rows are
 * neither removed nor overwritten; r_in <= QADC_REFINE_MAX_IN; squared L2 unless the store's metric says inner product
 * (qadc_refine_set_metric, below); one device; every call is synchronous. */
#define QADC_REFINE_F32 0
#define QADC_REFINE_F16 1
#define QADC_REFINE_MAX_IN 8192   /* most candidates per query a rerank call takes */
#define QADC_REFINE_MAX_DIM 4096
typedef struct qadc_refine qadc_refine;
/* An empty store of dim-float vectors (1 .. QADC_REFINE_MAX_DIM) kept as floats or halves on device_id.  QADC_E_ARG before the device
 * is touched: out NULL, a bad dim or dtype. */
int qadc_refine_create(qadc_refine** out, int dim, int dtype, int device_id);
/* Frees the store; NULL is a no-op. */
int qadc_refine_destroy(qadc_refine* r);
/* Appends vectors [count][dim] from host memory as the rows of the keys first_key .. first_key + count - 1.  The first add fixes
 * lo = first_key; a later one must continue at lo + rows.  The F16 conversion runs on the GPU.  The allocation grows by 1.5 x (or to
 * what the call needs) with one device-to-device copy.  count = 0 is a no-op.  QADC_E_ARG before the device is touched, the store
 * left as it was: r NULL, vectors NULL, a first_key that does not continue the store, first_key + count above 2^32. */
int qadc_refine_add(qadc_refine* r, const float* vectors, uint64_t count, uint32_t first_key);
/* The same with d_vectors in device memory of the store's device, complete before the call: read where they lie and only by a
 * kernel, so memory of another HIP runtime is legal — and the library cannot tell which device a pointer belongs to: as with
 * qadc_adc_filter_create_device, the store names the device. */
int qadc_refine_add_device(qadc_refine* r, const float* d_vectors, uint64_t count, uint32_t first_key);
/* Room for `rows` rows in all (no-op where the allocation holds them already): the adds up to there relocate nothing. */
int qadc_refine_reserve(qadc_refine* r, uint64_t rows);
/* Any output may be NULL: dim, dtype, lo (0 while empty), the rows held and the bytes of the allocation (capacity x row size). */
int qadc_refine_info(const qadc_refine* r, int* dim, int* dtype, uint32_t* lo, uint64_t* rows, uint64_t* bytes);
/* Adds that moved the rows held to grow the allocation. */
uint64_t qadc_refine_relocations(const qadc_refine* r);
/* Re-ranks, host arrays: queries [nq][dim], keys [nq][r_in], counts [nq] or NULL (every list is full), values [nq][r_in] or NULL ->
 * out_keys [nq][R], out_dist [nq][R], out_sizes [nq], *missing_out (may be NULL) = the missing entries of all queries.
 * 1 <= r_in <= QADC_REFINE_MAX_IN, 1 <= R (R > r_in is legal), nq = 0 is a no-op.  QADC_E_ARG before the device is touched: r NULL,
 * a bad r_in or R, a required array NULL, a counts[q] outside [0, r_in]. */
int qadc_refine_rerank(qadc_refine* r, int nq, const float* queries, int r_in, const uint32_t* keys, const int32_t* counts,
                       const float* values, int R, uint32_t* out_keys, float* out_dist, int32_t* out_sizes, uint64_t* missing_out);
/* The same with every array in device memory of the store's device (see qadc_refine_add_device), inputs complete before the call;
 * missing_out stays a host pointer.  A d_counts[q] outside [0, r_in] is clamped to it.  Nothing but the missing count crosses the bus. */
int qadc_refine_rerank_device(qadc_refine* r, int nq, const float* d_queries, int r_in, const uint32_t* d_keys, const int32_t* d_counts,
                              const float* d_values, int R, uint32_t* d_out_keys, float* d_out_dist, int32_t* d_out_sizes,
                              uint64_t* missing_out);

/* ---- the keyed refine store: put, overwrite and remove by label ----
 * A second kind of store holds a map from key to vector in place of a dense range, for an index whose labels the caller chose
 * (qadc_adc_index_add_vectors_labelled) and whose rows come and go (qadc_adc_index_remove_labels).  qadc_refine_rerank and
 * _rerank_device work on it as above, word for word, with "the store holds the key" = "the map has the key now": the output is a
 * function of the map's contents and the call's arguments alone.  The twin is refine::keyed_store of quick-adc_amd/host/refine.hpp.
 * In device memory the map is the row array of a dense store, a key and a free list per row, and an open-addressing hash table of
 * 2^bits slots (key, row) with linear probing, at most half used; which slot and which row a key occupies shows in no result.
 * The kinds do not mix: qadc_refine_add* on a keyed store and qadc_refine_put* / _remove* / _keyed_info on a dense one are
 * QADC_E_STATE.  On a keyed store qadc_refine_info reports lo = 0 and rows = the keys held, qadc_refine_reserve(rows) makes room
 * for `rows` keys in the row arrays and in the table, and qadc_refine_relocations counts the puts that moved the rows.
 * Limits: memory is reused, never returned (no shrink); at most 2^30 keys; key 0xFFFFFFFF cannot be held (it is rerank's filler
 * key); one device; every call is synchronous.  The key 0 a 4-bit heap's sentinel carries is missing on a store that does not
 * hold key 0. */
int qadc_refine_create_keyed(qadc_refine** out, int dim, int dtype, int device_id);
/* For i ascending the vector of key labels[i] becomes vectors[i] ([count][dim], host memory), converted as qadc_refine_add
 * converts: a key not held becomes held, a key held is overwritten, the last occurrence of a key within the call wins.  A call
 * whose keys are all held allocates nothing and moves nothing.  New keys take the rows that removals freed first.
 * QADC_E_ARG, the store left exactly as it was: a label 0xFFFFFFFF (checked over the whole call before anything is written);
 * vectors or labels NULL with count > 0; more than 2^30 keys.  count = 0 is a no-op. */
int qadc_refine_put(qadc_refine* r, const float* vectors, const uint32_t* labels, uint64_t count);
/* The same with d_vectors and d_labels in device memory of the store's device, complete before the call, read where they lie and
 * only by kernels (the label 0xFFFFFFFF is looked for by a kernel before anything is written). */
int qadc_refine_put_device(qadc_refine* r, const float* d_vectors, const uint32_t* d_labels, uint64_t count);
/* Every key of labels [count] (host memory) that is held leaves; keys not held are ignored.  *removed_out (may be NULL) = the
 * keys that left: a key listed twice counts once.  The rows are reused by later puts. */
int qadc_refine_remove(qadc_refine* r, const uint32_t* labels, uint64_t count, uint64_t* removed_out);
/* The same with d_labels in device memory of the store's device, read only by kernels. */
int qadc_refine_remove_device(qadc_refine* r, const uint32_t* d_labels, uint64_t count, uint64_t* removed_out);
/* Any output may be NULL: the keys held; the rows allocated so far (held or free) and those of them that are free; the table's
 * slots and how many are used (by a key held or by one removed since the last rebuild; at most half); the bytes of all
 * allocations (capacity x (row size + 8) + slots x 12). */
int qadc_refine_keyed_info(const qadc_refine* r, uint64_t* live, uint64_t* rows_allocated, uint64_t* rows_free, uint64_t* table_slots,
                           uint64_t* table_used, uint64_t* bytes);
/* The home slot of a key in a table of 2^table_bits slots — the hash, exported for tests and tools: the upper table_bits bits of
 * MurmurHash3's 32-bit finalizer of the key. */
uint32_t qadc_refine_keyed_slot(uint32_t key, int table_bits);

/* ---- exhaustive search: the R nearest rows of a whole store ----
 * For every query: of every key the store holds — dense or keyed, F32 or F16 — that passes `filter`, the word (image of D(q, x_key))
 * << 32 | key, D and the image exactly as above; the words sorted ascending, the first min(R, n) returned as (key, distance), the
 * slots behind them key 0xFFFFFFFF and distance +inf, out_sizes[q] = min(R, n).  That is qadc_refine_rerank with keys[q] = every
 * held key that passes and no r_in limit, bit for bit; the twin is refine::knn of quick-adc_amd/host/refine.hpp.  filter NULL: every
 * key passes; else qadc_adc_filter's rule: EXCLUDE drops the listed keys, ALLOW keeps only the listed keys (an empty ALLOW set keeps
 * nothing).  The filter need only be alive for the call and no use is counted on it.  An empty store gives sizes 0 and fillers; R
 * above the rows held is legal.  The result is a function of the store's contents and the arguments alone: no chunk, tile, pass or
 * arrival order shows in it.
 * Limits: every row is read whatever the filter says (a filter saves no time); R <= QADC_REFINE_KNN_MAX_R; L2 or inner product
 * (qadc_refine_set_metric); one device; one
 * filter per call; synchronous, on the store's stream. */
#define QADC_REFINE_KNN_MAX_R 1024
/* Host arrays: queries [nq][dim] -> out_keys [nq][R], out_dist [nq][R], out_sizes [nq].  nq = 0 is a no-op.  QADC_E_ARG before the
 * device is touched: r NULL, R outside [1, QADC_REFINE_KNN_MAX_R], a required array NULL with nq > 0, a filter of another device. */
int qadc_refine_knn(qadc_refine* r, int nq, const float* queries, int R, const qadc_adc_filter* filter, uint32_t* out_keys, float* out_dist,
                    int32_t* out_sizes);
/* The same with every array in device memory of the store's device (see qadc_refine_rerank_device), the queries complete before the
 * call: the arrays are touched by kernels only and nothing crosses the bus.  4-byte alignment of every array is checked first. */
int qadc_refine_knn_device(qadc_refine* r, int nq, const float* d_queries, int R, const qadc_adc_filter* filter, uint32_t* d_out_keys,
                           float* d_out_dist, int32_t* d_out_sizes);
/* A tuning and test knob: the rows of a group per launch (1 .. 7168) and the queries per pass of the later knn calls; 0 = the plan's
 * default (quick-adc_amd/host/refine_knn_plan.hpp).  No value changes a result.  QADC_E_ARG: r NULL, chunk_rows above 7168, a
 * negative pass_nq. */
int qadc_refine_set_knn_plan(qadc_refine* r, uint64_t chunk_rows, int pass_nq);

/* ---- probed exact search: the R nearest rows among the partitions a query probes ----
 * IVF-Flat (IVF-F16, IVF-SQ8) from the pieces that are resident: the index gives, per partition, its rows' keys; the store maps a
 * key to a row.  For query q with the probe list assign[q][0 .. ma):
 *   probes      P_q = the distinct partition numbers of the list; a repeat counts once.
 *   candidates  every row i of every p in P_q is one entry; its key is the partition's label i on a labelled index, else
 *               key_base + i — the key the scan gives the row.  A key that fails the index's filter (qadc_adc_index_set_filter) or
 *               `filter` is no entry: both must pass (EXCLUDE / ALLOW as above).
 *   result      qadc_refine_rerank fed q's entries with no r_in limit, bit for bit: D, its image and the NaN image as above; an entry
 *               whose key the store does not hold is missing and counted in *missing_out, per entry; a key that occurs several times
 *               (labels may repeat, within and across partitions) is kept once; the survivors ascending by (image(D) << 32) | key,
 *               the first min(R, survivors) returned, behind them key 0xFFFFFFFF and distance +inf; out_sizes[q].
 * The twin is refine::knn_probed of quick-adc_amd/host/refine.hpp.  The result is a function of the index's rows, the store's
 * contents and the arguments: no chunk, tile, pass, group or arrival order shows in it.  The index is read as it is at the call.
 * idx: an owned 8-bit or 16-bit index, or a view of a 4-bit index.  Dense and keyed stores; F32, F16 and SQ8 rows.
 * 1 <= R <= QADC_REFINE_KNN_MAX_R, 1 <= ma <= the index's partitions.  qadc_refine_set_knn_plan keeps its meaning for these calls
 * (chunk_rows: the rows a (query, group) buffer is offered between two selects; a query's probes share min(8, 8192 / R, ma) groups,
 * and chunk_rows below the probes of a group is refused); no value changes a result.
 * QADC_E_ARG: what qadc_refine_knn refuses; idx NULL; an index of another device than the store's; ma out of range; a view whose
 * source is sharded or holds borrowed partitions.  QADC_E_STATE: a view whose 4-bit source is not finalized.
 * Limits: no probed range search; L2 or inner product (qadc_refine_set_metric; the probes of qadc_adc_search_exact stay L2); R <= 1024; one device; one filter per call; synchronous; the rows are gathered through
 * the store (there is no partition-ordered copy of them); a single very long partition means many thin launches. */
/* Host arrays: queries [nq][dim], assign [nq][ma] -> out_keys [nq][R], out_dist [nq][R], out_sizes [nq]; missing_out may be NULL.
 * An entry of assign outside [0, partitions) is QADC_E_ARG before the device is touched. */
int qadc_refine_knn_probed(qadc_refine* r, const qadc_adc_index* idx, int nq, const float* queries, int ma, const int32_t* assign, int R,
                           const qadc_adc_filter* filter, uint32_t* out_keys, float* out_dist, int32_t* out_sizes, uint64_t* missing_out);
/* The same with every array, d_assign included, in device memory of the store's device, complete before the call and touched by
 * kernels only; 4-byte alignment of every array is checked first.  An entry of d_assign outside [0, partitions) is skipped.  What
 * crosses the bus: the nq x ma probe numbers, device to host (the planner inverts them there), the work lists they become, host to
 * device, and the missing count. */
int qadc_refine_knn_probed_device(qadc_refine* r, const qadc_adc_index* idx, int nq, const float* d_queries, int ma, const int32_t* d_assign,
                                  int R, const qadc_adc_filter* filter, uint32_t* d_out_keys, float* d_out_dist, int32_t* d_out_sizes,
                                  uint64_t* missing_out);
/* The coarse step of qadc_adc_search alone, with its kernels and refusals: assign_out [nq][ma] = the probe lists qadc_adc_search
 * reports in its assign_out.  An index without coarse centroids is flat: every probe 0.  A NaN coarse row with ma > 256 is refused. */
int qadc_adc_index_assign(qadc_adc_index* idx, int nq, const float* queries, int ma, int sum_mode, int32_t* assign_out);
/* The same with d_queries and d_assign_out in device memory of the index's device (4-byte aligned; written by a kernel). */
int qadc_adc_index_assign_device(qadc_adc_index* idx, int nq, const float* d_queries, int ma, int sum_mode, int32_t* d_assign_out);
/* qadc_adc_index_assign, then qadc_refine_knn_probed on its lists: the exact result over the partitions qadc_adc_search would
 * probe — the ceiling of a re-ranked search at the same ma.  assign_out [nq][ma] may be NULL. */
int qadc_adc_search_exact(qadc_adc_index* idx, qadc_refine* store, int nq, const float* queries, int ma, int R, int sum_mode,
                          const qadc_adc_filter* filter, uint32_t* out_keys, float* out_dist, int32_t* out_sizes, uint64_t* missing_out,
                          int32_t* assign_out);
/* The same on arrays in device memory (d_assign_out may be NULL); what crosses the bus is what the two device calls let cross. */
int qadc_adc_search_exact_device(qadc_adc_index* idx, qadc_refine* store, int nq, const float* d_queries, int ma, int R, int sum_mode,
                                 const qadc_adc_filter* filter, uint32_t* d_out_keys, float* d_out_dist, int32_t* d_out_sizes,
                                 uint64_t* missing_out, int32_t* d_assign_out);

/* ---- SQ8 rows: one byte per component under a per-dimension range; read-back ----
 * A third element type: a store of dim bytes per row (no padding) with the parameters vmin[dim] and step[dim], both finite,
 * step >= 0.  The store derives inv[i] = 1.0f / step[i] where step[i] > 0 (+inf for a subnormal step), else 0, on the host, once.
 * All arithmetic is binary32, every operation rounded by itself, no fused multiply-add; the twin is sq_encode, sq_decode and
 * sq_range of quick-adc_amd/host/refine.hpp, and the GPU equals it bit for bit (stored bytes and the clamp counter included).
 *   encode   component x of dimension i: d = x - vmin[i]; u = d * inv[i]; byte 0 where !(u > 0) (NaN, below the range, a constant
 *            dimension), else 255 where u >= 255, else u rounded to the nearest integer, ties to even.
 *   decode   vmin[i] + (float)byte * step[i]: the product rounded, then the sum.  D(q, x) and the selection are those above with the
 *            row's i-th component decoded so; nothing else of rerank or knn changes.
 *   clamped  a component written to a row counts where step[i] > 0 and (!(d >= 0) or !(u <= 255)), or where step[i] == 0 and x
 *            differs in value from vmin[i] (a NaN does; -0 does not differ from +0).  Only what reaches a row counts: of equal keys
 *            within one put, the winner.  A sum, so no order shows in it.
 *   range    per dimension the minimum and maximum over the finite components of a learning set, in the order of the
 *            sign-magnitude image (-0 below +0); none: 0 and 0.  vmin = the minimum, step = (max - min) / 255.0f, divided on the
 *            host.  A function of the set alone.  step is +inf where max - min overflows: no store takes such a range.
 * Every call above works on such a store unchanged; qadc_refine_info reports dtype 2 and bytes = capacity x dim.
 * Limits: the range is fixed at creation (no re-encoding); uniform steps only; L2 or inner product
 * (qadc_refine_set_metric); one device. */
#define QADC_REFINE_SQ8 2
/* An empty SQ8 store on device_id, dense (keyed = 0) or keyed.  qadc_refine_create and _create_keyed refuse dtype 2: the type needs
 * its parameters.  QADC_E_ARG before the device is touched: out, vmin or step NULL, a bad dim, a vmin[i] or step[i] that is not
 * finite, a negative step[i]. */
int qadc_refine_create_sq8(qadc_refine** out, int dim, const float* vmin, const float* step, int keyed, int device_id);
/* The range of vectors [n][dim] (host memory) -> vmin_out [dim], step_out [dim] (host memory), minimum and maximum found on
 * device_id.  n = 0 is legal and gives zeros.  QADC_E_ARG: a bad dim, an output NULL, vectors NULL with n > 0. */
int qadc_refine_sq_range_host(const float* vectors, uint64_t n, int dim, int device_id, float* vmin_out, float* step_out);
/* The same with d_vectors in device memory of device_id, complete before the call, read by a kernel only; the outputs stay host
 * memory. */
int qadc_refine_sq_range_device(const float* d_vectors, uint64_t n, int dim, int device_id, float* vmin_out, float* step_out);
/* Any output may be NULL: the store's vmin [dim] and step [dim] and the clamped components counted so far.  QADC_E_STATE on an F32
 * or F16 store. */
int qadc_refine_sq_info(const qadc_refine* r, float* vmin_out, float* step_out, uint64_t* clamped_out);
/* Read-back, on stores of every kind and element type: out_vectors [count][dim] (host memory) = the rows of keys [count] as floats,
 * decoded by the store's type (an F32 row as it is, an F16 row as the float value of the stored half); a key the store does not
 * hold gives a row of 0x7FC00000 and found_out[i] = 0, else found_out[i] = 1.  found_out may be NULL; count = 0 is a no-op.
 * QADC_E_ARG: r NULL, keys or out_vectors NULL with count > 0. */
int qadc_refine_get(qadc_refine* r, const uint32_t* keys, uint64_t count, float* out_vectors, uint8_t* found_out);
/* The same with every array in device memory of the store's device (see qadc_refine_add_device), d_keys complete before the call;
 * d_keys and d_out_vectors are checked for 4-byte alignment first. */
int qadc_refine_get_device(qadc_refine* r, const uint32_t* d_keys, uint64_t count, float* d_out_vectors, uint8_t* d_found_out);

/* ---- exact range search: every row within an exact radius; range results re-ranked by L2 ----
 * The other query of a refine store, dense or keyed, F32, F16 or SQ8.  A row is KEPT for query q where its key is held by the store,
 * passes the filter (qadc_adc_filter's rule, as in qadc_refine_knn) and D(q, x) < radius[q] as a binary32 compare, D exactly the
 * distance above.  A NaN distance or a NaN radius keeps nothing; a radius <= 0 of either sign keeps nothing (D is +0, positive or NaN);
 * a distance equal to the radius is not kept; radius +inf keeps every finite distance and no +inf one.  Query q's kept rows are ordered
 * ascending by the 64-bit word (bits(D) << 32) | key.  There is no R, no heap and no cap on a query's rows.  The written definition is
 * refine::range and refine::rerank_range of quick-adc_amd/host/refine.hpp, to which keys, the distances' bit patterns, lims and the
 * missing count are held bit for bit; the result is a function of the store's contents and the arguments alone: no region size,
 * chunk, pass, rerun or arrival order shows in it.
 *   radius [nq], lims [nq + 1], in_lims [nq + 1]   HOST memory in every form.
 *   lims                                           out: query q's rows are [lims[q], lims[q + 1]) of the held result; lims[nq] = its rows.
 * The result stays ON THE STORE, in device memory no other call writes, until the next qadc_refine_range* or _rerank_range* call (which
 * drops it, also when it fails) or qadc_refine_destroy; qadc_refine_range_collect* copies it out, any number of times, and add, put,
 * remove, rerank, knn and get calls in between leave it as it is.  Every call is synchronous on the store's stream.  A pass of the
 * exhaustive form runs once with a region of min(rows, 4096) words per query and, where a region overflowed, a second time with regions
 * of exactly the counted sizes (counted in qadc_refine_range_reruns).  nq = 0 is a no-op that holds an empty result (lims[0] = 0 where
 * lims is given); an empty store gives all-zero lims.
 * QADC_E_ARG before the device is touched: r NULL, nq < 0, a required array NULL with nq > 0, a filter of another device, a device
 * array that is not 4-byte aligned, an in_lims that does not start at 0 or decreases.  QADC_E_CAPACITY before anything is allocated for
 * them: the regions of one run of a pass, the candidates of one query, or the rows of the call's whole result exceed
 * QADC_REFINE_RANGE_MAX_ENTRIES.
 * Limits: every row is read, whatever the filter and the radius; the held result and a pass's regions are resident in device memory;
 * a query that keeps more than QADC_REFINE_RANGE_SORT_LDS rows pays the radix passes; L2 only (a store whose metric is QADC_REFINE_IP
 * refuses the four range calls with QADC_E_STATE); one device; one filter per call;
 * synchronous. */
#define QADC_REFINE_RANGE_MAX_ENTRIES (1ull << 31) /* most words the regions of one run, and most rows a call's result, may hold */
#define QADC_REFINE_RANGE_SORT_LDS 4096            /* a query's words up to this many are sorted in LDS, more by radix passes */
/* Exhaustive, host arrays: queries [nq][dim] -> the kept rows of the whole store.  filter may be NULL. */
int qadc_refine_range(qadc_refine* r, int nq, const float* queries, const float* radius, const qadc_adc_filter* filter, uint64_t* lims);
/* The same with d_queries in device memory of the store's device (see qadc_refine_add_device), complete before the call and touched
 * only by kernels. */
int qadc_refine_range_device(qadc_refine* r, int nq, const float* d_queries, const float* radius, const qadc_adc_filter* filter,
                             uint64_t* lims);
/* The same rule restricted to the candidates keys[in_lims[q] .. in_lims[q + 1]) of query q — the CSR result of a range search of an
 * index, for instance — with no limit on their number.  A key the store does not hold is missing: dropped and counted in *missing_out
 * (may be NULL); a keyed store never holds key 0xFFFFFFFF; a key listed several times is kept once.  keys is host memory [in_lims[nq]]. */
int qadc_refine_rerank_range(qadc_refine* r, int nq, const float* queries, const uint64_t* in_lims, const uint32_t* keys, const float* radius,
                             uint64_t* lims, uint64_t* missing_out);
/* The same with d_queries and d_keys in device memory of the store's device, as qadc_adc_range_collect_device writes the keys; both
 * are touched only by kernels.  Only in_lims, lims and the missing count cross the bus. */
int qadc_refine_rerank_range_device(qadc_refine* r, int nq, const float* d_queries, const uint64_t* in_lims, const uint32_t* d_keys,
                                    const float* radius, uint64_t* lims, uint64_t* missing_out);
/* Copies the held result into keys / dist [capacity] (host memory).  QADC_E_CAPACITY when capacity < lims[nq]: nothing is copied and
 * the result stays held.  QADC_E_STATE when no result is held. */
int qadc_refine_range_collect(qadc_refine* r, uint64_t capacity, uint32_t* keys, float* dist);
/* The same into device memory, copied by a kernel (the buffers may belong to another copy of the HIP runtime): exactly lims[nq]
 * entries of each are written. */
int qadc_refine_range_collect_device(qadc_refine* r, uint64_t capacity, uint32_t* d_keys, float* d_dist);
/* A tuning and test knob of the later range calls: the words of a query's region in the first run, the rows of a group per launch
 * (at most 2^24) and the queries per pass (also of rerank_range); 0 = the plan's default (quick-adc_amd/host/refine_range_plan.hpp).
 * No value changes a result.  QADC_E_ARG: r NULL, chunk_rows above 2^24, a negative pass_nq. */
int qadc_refine_set_range_plan(qadc_refine* r, uint64_t region_rows, uint64_t chunk_rows, int pass_nq);
/* Passes that were run a second time because a region overflowed. */
uint64_t qadc_refine_range_reruns(const qadc_refine* r);

/* ---- the metric of a store: squared L2 or inner product ----
 * A property of the store handle, host state only: no device call, no effect on the rows, changeable at any time, QADC_REFINE_L2 at
 * creation.  Under QADC_REFINE_IP qadc_refine_rerank, _rerank_device, _knn, _knn_device, _knn_probed, _knn_probed_device and what is
 * composed from them (qadc_adc_search_exact*, a search followed by a rerank) rank by the inner product — maximum-inner-product
 * search; cosine through rows and queries normalised before add.  Held bit for bit to refine::rerank, ::knn and ::knn_probed of
 * quick-adc_amd/host/refine.hpp with metric kIP:
 *   score      S(q, x) in binary32, every operation rounded by itself, no fused multiply-add: 64 partial sums p[l] = +0, over the
 *              components 64 j + l in ascending j (m = q[i] * x[i]; p[l] = p[l] + m), then p[l] = p[l] + p[l + s] for l < s at
 *              s = 32, 16, 8, 4, 2, 1; S = p[0] — the strips and the tree of D.  A row's component is what D reads: the float of
 *              the stored half, or the decoded byte of an SQ8 row.  A component that does not exist contributes nothing.  S is
 *              never -0: a p starts at +0 and an IEEE sum is -0 only where both operands are.
 *   order      larger S first, ties by ascending key: the word is (img_ip(S) << 32) | key, sorted ascending.  img_ip(S) is
 *              0xFFC00000 for every NaN; else, with b the bit pattern of S, b where its sign bit is set and ~b & 0x7FFFFFFF where
 *              it is clear: +inf 0x007FFFFF, +0 0x7FFFFFFF, -0 0x80000000, -inf 0xFF800000, a NaN behind -inf.
 *   outputs    out_dist[q][i] holds S itself (the inverse of the image; a NaN as 0x7FC00000), descending; the slots behind
 *              out_sizes[q] hold key 0xFFFFFFFF and score -inf (0xFF800000).
 * Everything else is the L2 rule word for word: the skip of values == FLT_MAX, missing keys and their count, a key listed several
 * times kept once, filters, the probed entry rule, the limits on R and r_in.  Setting the metric back to QADC_REFINE_L2 gives the L2
 * results exactly.
 * Under QADC_REFINE_IP qadc_refine_range, _range_device, _rerank_range and _rerank_range_device return QADC_E_STATE before the device
 * is touched and leave a held result as it is (the radius rules assume D >= 0); qadc_refine_range_collect* of a result held from
 * before still works.
 * Not covered: range search by inner product; inner-product coarse assignment (qadc_adc_index_assign and with it
 * qadc_adc_search_exact probe by L2 to the centroids — a caller who wants other probes passes their own lists to
 * qadc_refine_knn_probed); inner-product tables from qadc_adc_search (a caller's own tables through qadc_adc_query_scan* serve);
 * cosine as a metric of its own. */
#define QADC_REFINE_L2 0
#define QADC_REFINE_IP 1
/* QADC_E_ARG: r NULL, a metric that is neither QADC_REFINE_L2 nor QADC_REFINE_IP (the store keeps the metric it had). */
int qadc_refine_set_metric(qadc_refine* r, int metric);
/* *metric_out = the store's metric.  QADC_E_ARG: r or metric_out NULL. */
int qadc_refine_metric(const qadc_refine* r, int* metric_out);

#ifdef __cplusplus
}
#endif
#endif /* QADC_H_ */
