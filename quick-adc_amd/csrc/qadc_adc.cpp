// Host side of the float-ADC engine for whole-byte PQ codes (qadc_adc_* in include/qadc.h): the GPU scanner_simple
// (db_query.cpp:17-46) over scan_standard<uint8_t, NSQ> (query_common.hpp:92-118), NSQ 4, 8 or 16, and over
// scan_standard<uint16_t, NSQ>, NSQ 2, 4 or 8 (qadc_adc_index_create16).
//
// A call scans the probed partitions of nq queries in bound levels: level 0 is the first
// max(R, 512) codes of every query's scan order, each following level 16 times as far; the runs of a level are filtered
// by the R-th smallest value the query emitted in the levels before it (FLT_MAX while fewer than R), which is the R-th
// smallest of a subset of the codes that precede every code of the level.  The kept candidates come back to the host,
// are put in scan order and pushed into kv_heap<unsigned, float>(R) after the R sentinels — or, with the device finish
// (qadc_adc_index_set_finish, the *_device entry points), are ordered and replayed by two more kernels, so
// that only the heaps' arrays leave device memory, or nothing does.  On the query side this engine shares nothing
// with the 4-bit index but the device's stream set (qadc_device_prepare), the coarse-assignment kernels and the float sums
// of the feeders; it has no qadc_set_option names.  The owned database is a RowStore (csrc/qadc_host.h), and what changes it —
// add_vectors, reserve, read_partition (csrc/qadc_append.h) and remove_labels (csrc/qadc_remove.h) — is the host flow both
// engines run: this file supplies the move step of a relocation and the encoders' last launch (DESIGN.md sections 11.5, 11.7).
//
// The tables of a call come from the caller (qadc_adc_query_scan*) or are built on the device from query vectors
// (qadc_adc_search*: coarse assignment, residual, OPQ rotation, tables — what nns_engine(_batch)::process_query does before
// query_scan, query_common.hpp:194-213, 283-297); both share everything after the tables are in device memory.
//
// A VIEW (qadc_adc_index_create_view) is the same engine over the 4-bit codes of a finalized
// qadc_index — db_query's scan_4<M> (query_common.hpp:59-90) on the database db_query_4 has resident.  It owns no codes: it
// snapshots the index's partition table, scans with adc_scan_kernel over NibbleCodes<M> (tables [M][16]) and, for the search
// calls, reads the index's quantizers (FeederState) through launch_coarse_assign and launch_build_tables on its own stream.  Levels, bounds,
// regions, re-runs and both finishes are the ones above, unchanged: nothing in them depends on how a candidate is summed.
#include "../../include/qadc.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../host/adc_append_plan.hpp"
#include "../host/qadc_heap.hpp"
#include "../host/worker_pool.hpp"
#include "qadc_adc_kernels.h"
#include "qadc_append.h"
#include "qadc_decode.h"
#include "qadc_host.h"
#include "qadc_remove.h"

using qadc::host::fail;
using qadc::host::DevBuf;
using qadc::host::PinBuf;

namespace {

constexpr uint64_t kSpeculativeEntries = 1 << 16;   // regions up to this many entries in all come back with the counts
constexpr uint64_t kMaxEntries = QADC_ADC_MAX_ENTRIES;   // candidate entries of one batch (12 B of device memory each)

}  // namespace

// A key filter (qadc_adc_filter_create*): the bitmap of the caller's key set in device memory, immutable
// once created, and the number of indexes it is set on.
struct qadc_adc_filter {
    int device = 0, mode = QADC_ADC_FILTER_EXCLUDE;
    uint32_t lo = 0xffffffffu, hi = 0;              // the smallest and largest key of the set (an empty set: lo > hi)
    qadc::adc::RemoveSpan span;                     // the bitmap's span: [lo, hi], or the one zero word [0, 0] of an empty set
    uint32_t* bitmap = nullptr;                     // span.words words, owned by mem
    qadc::host::Scratch mem;
    mutable std::atomic<int> uses{0};               // indexes that hold it (qadc_adc_index_set_filter)
};

struct qadc_adc_index {
    int nsq = 0, device = 0;
    const qadc_adc_filter* filter = nullptr;        // set: every scan launch drops the rows whose key does not pass it
    int centroids = 256;                            // per sub-quantizer: a table is [nsq][centroids] floats (16: a view; 65536: 16-bit codes)
    int code_size() const { return centroids == 65536 ? 2 * nsq : nsq; }   // bytes of one code of the owned database
    // A view (qadc_adc_index_create_view): the 4-bit index whose partitions, labels and quantizers it reads in place, counted
    // in src->adc_views, and the partition table the nibble kernel takes — a snapshot of src->parts at creation.
    qadc_index* src = nullptr;
    DevBuf<qadc::adc::Part4> d_parts4;
    std::vector<qadc::adc::Part4> parts4;           // the same table on the host (the reconstruction reads a view's partitions through it)
    hipStream_t stream = nullptr;
    int labeled = -1;                               // unknown until the first non-empty add
    std::vector<uint32_t> sizes;                    // rows each partition holds (a view: of the index it reads)
    qadc::host::RowStore store;                     // the owned database: region_pad 0, code_bytes + kAppendTailPad bytes of codes
    // per call
    DevBuf<uint8_t> d_in;                           // [bound | count | assign | items | tables]
    DevBuf<float> d_vals;
    DevBuf<uint32_t> d_keys, d_sidx, d_packed;
    PinBuf<uint8_t> h_in;
    PinBuf<uint32_t> h_count, h_packed;
    uint64_t reruns = 0;                            // batches re-run because a candidate region overflowed
    // device finish
    int finish = QADC_ADC_FINISH_HOST;
    uint64_t host_finishes = 0;                     // queries finished on the host although the device finish was asked for
    DevBuf<float> d_ovals;                          // the ordered stream, region by region
    DevBuf<uint32_t> d_okeys;
    DevBuf<uint64_t> d_tmp_a, d_tmp_b;              // radix scratch of the order kernel (streams too long for LDS)
    DevBuf<uint32_t> d_hkeys;                       // heap arrays of a call whose outputs are host memory
    DevBuf<float> d_hvals;
    DevBuf<int32_t> d_hsizes;
    // feeders (qadc_adc_search*): quantizer, coarse centroids and the per-call buffers
    int dim = 0, K = 0;                             // dim 0: no set_pq yet;  K 0: flat (no coarse quantizer)
    bool rotated = false;
    uint64_t table_budget = 1ull << 30;             // bytes of device tables per sub-batch (TABLES_BUFFER_SIZE, query_common.hpp:147)
    DevBuf<float> d_codebooks, d_cbnorm;            // [nsq][centroids][dim/nsq];  [2][nsq*centroids] ||c||^2 under sum_mode 0 and 1
    DevBuf<float> d_rotation, d_coarse, d_cnorm;    // [dim][dim];  [K][dim];  [2][K]
    DevBuf<float> d_queries, d_qnorm, d_cdist, d_tables;
    const float* cur_queries = nullptr;             // the queries of the call: d_queries, or the caller's device memory
    DevBuf<int32_t> d_assign;
    PinBuf<int32_t> h_assign;
    hipEvent_t ev_assign = nullptr;
    std::vector<uint64_t> stream_off;               // [nq + 1] the ordered stream of the last call
    std::vector<uint32_t> stream_keys;
    std::vector<float> stream_vals;
    // range search (qadc_adc_range_*): the held result, in buffers no other call writes
    DevBuf<uint32_t> d_rkeys;
    DevBuf<float> d_rvals;
    PinBuf<float> h_radius;
    std::vector<uint64_t> range_lims;               // [nq + 1] rows of each query of the last range call; empty: nothing to collect
    qadc::WorkerPool pool;
};

namespace {

using namespace qadc::adc;

template <typename T>
int grow_device(DevBuf<T>& buf, uint64_t used, uint64_t need, hipStream_t s) {
    if (need <= buf.cap) return QADC_OK;
    DevBuf<T> nb;
    HIPCHECK(nb.ensure(std::max<uint64_t>(need, buf.cap + buf.cap / 2)));
    if (used && buf.p) HIPCHECK(hipMemcpyAsync(nb.p, buf.p, used * sizeof(T), hipMemcpyDeviceToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));
    buf.release();
    buf = nb;
    return QADC_OK;
}

int check_R(int R) {
    return R < 1 || R > QADC_ADC_MAX_R ? fail(QADC_E_ARG, "R must be in [1, " + std::to_string(QADC_ADC_MAX_R) + "]") : QADC_OK;
}

int check_query_args(const qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const void* tables, int R, int sum_mode) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (nq < 1 || ma < 1 || ma >= 16384) return fail(QADC_E_ARG, "need nq >= 1 and 1 <= ma < 16384");
    if (int rc = check_R(R)) return rc;
    if (sum_mode != 0 && sum_mode != 1) return fail(QADC_E_ARG, "sum_mode is 0 (source order) or 1 (as compiled)");
    if (!assign || !tables) return fail(QADC_E_ARG, "assign and tables are required");
    const int parts = (int)idx->sizes.size();
    for (size_t i = 0; i < (size_t)nq * ma; ++i)
        if (assign[i] < 0 || assign[i] >= parts)
            return fail(QADC_E_ARG, "assign[" + std::to_string(i) + "] = " + std::to_string(assign[i]) + " is not a partition (" +
                                        std::to_string(parts) + " partitions)");
    return QADC_OK;
}

// Where the device finish leaves the heaps' arrays of a batch: device memory, keys / values [nq][R], sizes [nq].
struct DeviceOut { uint32_t* keys; float* values; int32_t* sizes; };

// A filter as the kernels read it — the index's, or the table entry of one query of a *_filtered call; none (bitmap null) for NULL.
ScanFilter scan_filter(const qadc_adc_filter* f) { return f ? ScanFilter{f->bitmap, f->span.lo, f->span.last, f->mode} : ScanFilter{}; }

}  // namespace

void qadc::host::adc_filter_view(const qadc_adc_filter* f, qadc::adc::ScanFilter* out, int* device) {
    *out = scan_filter(f);
    *device = f ? f->device : -1;
}

int qadc::host::adc_probe_view(const qadc_adc_index* idx, std::vector<AdcProbePart>* parts, int* device, qadc::adc::ScanFilter* filter) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    parts->clear();
    if (idx->src) {
        if (!idx->src->finalized) return fail(QADC_E_STATE, "the view's source index is not finalized");
        if (idx->src->dist) return fail(QADC_E_ARG, "the view's source index takes part in a multi-GPU merge");
        if (idx->src->parts.size() != idx->parts4.size()) return fail(QADC_E_STATE, "the view's source index has changed its partitions");
        for (size_t p = 0; p < idx->src->parts.size(); ++p) {
            const Part& pt = idx->src->parts[p];
            if (pt.n != pt.global_n || pt.first_pos != 0 || pt.d_starts) return fail(QADC_E_ARG, "the view's source index is sharded");
            if (!pt.own) return fail(QADC_E_ARG, "partition " + std::to_string(p) + " of the view's source index is borrowed");
            parts->push_back(AdcProbePart{idx->parts4[p].labels, idx->parts4[p].key_base, idx->sizes[p]});
        }
    } else {
        for (size_t p = 0; p < idx->sizes.size(); ++p) {
            const uint32_t n = idx->sizes[p];
            parts->push_back(AdcProbePart{n && idx->labeled == 1 ? idx->store.part_labels(p) : nullptr, 0, n});
        }
    }
    *device = idx->device;
    *filter = scan_filter(idx->filter);
    return QADC_OK;
}

namespace {

// The database as the scan launcher takes it: the owned codes, or the partition table of a view.
ScanDb scan_db(const qadc_adc_index* idx) {
    const ScanFilter filter = scan_filter(idx->filter);
    if (idx->src) return ScanDb{idx->nsq, idx->centroids, Db{}, idx->d_parts4.p, filter};
    return ScanDb{idx->nsq, idx->centroids, Db{idx->store.codes.p, idx->store.d_off.p, idx->labeled == 1 ? idx->store.labels.p : nullptr,
                                                  idx->store.d_lab_off.p}, nullptr, filter};
}

// One batch on its way through scan_batch: the plan, where the batch lies in the staging buffers idx->h_in / idx->d_in, uploaded in one copy —
//   bound (FLT_MAX) | count (0) | region sizes | region bases | assign | items | query filters (a *_filtered call with one at least) |
//   tables (the caller's, unless already on the device)
// of which the first four, bytes [0, o_assign), are the state a re-run writes again — and what the levels left.
struct Batch {
    Plan plan;
    size_t o_count, o_cap, o_base, o_assign;
    uint64_t entries = 0, n_stored = 0;   // entries of all regions together;  candidates they hold after the levels
    float* d_bound;
    const int32_t* d_assign;
    const Item* d_items;
    const float* d_tables;
    Emit emit;                      // the regions: count, base and cap lie in d_in, vals / keys / sidx are set by every attempt
    const ScanFilter* d_qfilters = nullptr;   // [nq] the filters of the batch's queries (the *_filtered calls), behind the items in d_in: outside
                                              // the state bytes, so every re-run scans under the same table.  Null: no query has one
    std::vector<uint32_t> stored;   // [nq] candidates each query's region holds after the levels (n_stored in all)
};

// bound, counts and the regions of plan.cap into the host staging buffer
void fill_state(qadc_adc_index* idx, Batch& b) {
    uint8_t* h = idx->h_in.p;
    const size_t nq = b.plan.cap.size();
    std::fill(reinterpret_cast<float*>(h), reinterpret_cast<float*>(h) + nq, FLT_MAX);
    std::memset(h + b.o_count, 0, nq * 4);
    std::memcpy(h + b.o_cap, b.plan.cap.data(), nq * 4);
    uint64_t* base = reinterpret_cast<uint64_t*>(h + b.o_base);
    b.entries = 0;
    for (size_t q = 0; q < nq; ++q) {
        base[q] = b.entries;
        b.entries += b.plan.cap[q];
    }
}

// The filters of queries [0, nq) hold one at least.
bool any_filter(const qadc_adc_filter* const* filters, int nq) {
    return filters && std::any_of(filters, filters + nq, [](const qadc_adc_filter* f) { return f != nullptr; });
}

// Lays the batch out and enqueues its upload.  d_ready: the tables are in device memory already (tables is null then).  qfilters: the
// filters of the batch's nq queries, one of them at least not null, or null.
int stage_batch(qadc_adc_index* idx, Batch& b, int nq, int ma, const int32_t* assign, const float* tables, const float* d_ready,
                const qadc_adc_filter* const* qfilters) {
    const std::vector<Item>& items = b.plan.items;
    const size_t table_bytes = d_ready ? 0 : (size_t)nq * ma * idx->nsq * idx->centroids * 4;
    b.o_count = align_up((size_t)nq * 4, 256);
    b.o_cap = b.o_count + align_up((size_t)nq * 4, 256);
    b.o_base = b.o_cap + align_up((size_t)nq * 4, 256);
    b.o_assign = b.o_base + align_up((size_t)nq * 8, 256);
    const size_t o_items = b.o_assign + align_up((size_t)nq * ma * 4, 256);
    const size_t o_qfilters = o_items + align_up(items.size() * sizeof(Item), 256);
    const size_t o_tables = o_qfilters + (qfilters ? align_up((size_t)nq * sizeof(ScanFilter), 256) : 0);
    const size_t in_bytes = o_tables + table_bytes;
    HIPCHECK(idx->h_in.ensure(std::max<size_t>(in_bytes, 256)));
    HIPCHECK(idx->d_in.ensure(std::max<size_t>(in_bytes, 256)));
    uint8_t *h = idx->h_in.p, *d = idx->d_in.p;
    fill_state(idx, b);
    std::memcpy(h + b.o_assign, assign, (size_t)nq * ma * 4);
    if (!items.empty()) std::memcpy(h + o_items, items.data(), items.size() * sizeof(Item));
    if (qfilters) {
        ScanFilter* table = reinterpret_cast<ScanFilter*>(h + o_qfilters);
        for (int q = 0; q < nq; ++q) table[q] = scan_filter(qfilters[q]);
        b.d_qfilters = reinterpret_cast<const ScanFilter*>(d + o_qfilters);
    }
    if (table_bytes) std::memcpy(h + o_tables, tables, table_bytes);
    b.d_bound = reinterpret_cast<float*>(d);
    b.d_assign = reinterpret_cast<const int32_t*>(d + b.o_assign);
    b.d_items = reinterpret_cast<const Item*>(d + o_items);
    b.d_tables = d_ready ? d_ready : reinterpret_cast<const float*>(d + o_tables);
    b.emit = Emit{reinterpret_cast<uint32_t*>(d + b.o_count), nullptr, nullptr, nullptr, reinterpret_cast<const uint64_t*>(d + b.o_base),
                  reinterpret_cast<const uint32_t*>(d + b.o_cap)};
    HIPCHECK(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, idx->stream));
    return QADC_OK;
}

// Runs the levels and reads the counts back; while a region overflowed, grows it and re-runs the whole batch.  fetch: the stored records come
// back too, packed into idx->h_packed (three words each) — those of a small batch speculatively, with the counts, in one round trip.
int run_levels(qadc_adc_index* idx, Batch& b, int nq, int ma, int R, int sum_mode, bool fetch) {
    ScanDb db = scan_db(idx);
    db.qfilters = b.d_qfilters;
    const std::vector<uint32_t>& first = b.plan.level_first;
    const int levels = b.plan.levels();
    b.stored.resize(nq);
    bool speculative = false;
    for (;;) {
        if (b.entries > kMaxEntries)
            return fail(QADC_E_CAPACITY, "the candidate regions of this batch need " + std::to_string(b.entries) + " entries (at most " +
                                             std::to_string(kMaxEntries) + "): split the batch");
        HIPCHECK(idx->d_vals.ensure(b.entries));
        HIPCHECK(idx->d_keys.ensure(b.entries));
        HIPCHECK(idx->d_sidx.ensure(b.entries));
        b.emit.vals = idx->d_vals.p;
        b.emit.keys = idx->d_keys.p;
        b.emit.sidx = idx->d_sidx.p;
        for (int l = 0; l < levels; ++l) {
            HIPCHECK(launch_adc_scan(db, sum_mode, b.d_items, first[l], first[l + 1] - first[l], b.d_assign, ma, b.d_tables, b.d_bound, b.emit,
                                     idx->stream));
            if (l + 1 < levels) HIPCHECK(launch_adc_select(nq, R, b.emit, b.d_bound, idx->stream));
        }
        HIPCHECK(idx->h_count.ensure(nq));
        speculative = fetch && b.entries <= kSpeculativeEntries;
        if (speculative) {
            HIPCHECK(idx->d_packed.ensure(3 * b.entries));
            HIPCHECK(idx->h_packed.ensure(3 * b.entries));
            HIPCHECK(launch_adc_pack(nq, b.emit, idx->d_packed.p, idx->stream));
        }
        HIPCHECK(hipMemcpyAsync(idx->h_count.p, b.emit.count, (size_t)nq * 4, hipMemcpyDeviceToHost, idx->stream));
        if (speculative) HIPCHECK(hipMemcpyAsync(idx->h_packed.p, idx->d_packed.p, 3 * b.entries * 4, hipMemcpyDeviceToHost, idx->stream));
        HIPCHECK(hipStreamSynchronize(idx->stream));
        bool overflow = false;
        b.n_stored = 0;
        for (int q = 0; q < nq; ++q) {
            uint32_t& cap = b.plan.cap[q];
            const uint32_t c = idx->h_count.p[q];
            b.stored[q] = std::min(c, cap);
            b.n_stored += b.stored[q];
            if (c > cap) {   // every emitted candidate was counted: this region takes them all in the re-run
                overflow = true;
                cap = (uint32_t)std::min<uint64_t>(b.plan.total[q], std::max<uint64_t>((uint64_t)c + c / 2, 2ull * cap));
            }
        }
        if (!overflow) break;
        ++idx->reruns;
        fill_state(idx, b);
        HIPCHECK(hipMemcpyAsync(idx->d_in.p, idx->h_in.p, b.o_assign, hipMemcpyHostToDevice, idx->stream));
    }
    if (fetch && !speculative) {
        HIPCHECK(idx->d_packed.ensure(std::max<uint64_t>(3 * b.n_stored, 3)));
        HIPCHECK(idx->h_packed.ensure(std::max<uint64_t>(3 * b.n_stored, 3)));
        HIPCHECK(launch_adc_pack(nq, b.emit, idx->d_packed.p, idx->stream));
        if (b.n_stored) HIPCHECK(hipMemcpyAsync(idx->h_packed.p, idx->d_packed.p, 3 * b.n_stored * 4, hipMemcpyDeviceToHost, idx->stream));
        HIPCHECK(hipStreamSynchronize(idx->stream));
    }
    return QADC_OK;
}

// The device finish: order, replay.  The heaps' arrays are in `out` and the stream synchronised on return; idx->stream_* is empty.
int finish_on_device(qadc_adc_index* idx, const Batch& b, int nq, int R, const DeviceOut& out) {
    idx->stream_off.assign((size_t)nq + 1, 0);
    idx->stream_keys.clear();
    idx->stream_vals.clear();
    HIPCHECK(idx->d_ovals.ensure(b.entries));
    HIPCHECK(idx->d_okeys.ensure(b.entries));
    int bits = 0;
    while (bits < 32 && ((b.plan.max_total - 1) >> bits)) ++bits;   // (max_total >= 1 where anything was stored)
    if (*std::max_element(b.stored.begin(), b.stored.end()) > (uint32_t)kOrderLds) {
        if (bits > 8) HIPCHECK(idx->d_tmp_a.ensure(b.entries));
        if (bits > 16) HIPCHECK(idx->d_tmp_b.ensure(b.entries));
    }
    HIPCHECK(launch_adc_order(nq, b.emit, bits, idx->d_ovals.p, idx->d_okeys.p, idx->d_tmp_a.p, idx->d_tmp_b.p, idx->stream));
    HIPCHECK(launch_adc_replay(nq, R, b.emit, idx->d_ovals.p, idx->d_okeys.p, out.keys, out.values, out.sizes, idx->stream));
    HIPCHECK(hipStreamSynchronize(idx->stream));
    return QADC_OK;
}

// Every query's records of idx->h_packed into idx->stream_* in scan order (scan indices are distinct within a query).
void order_on_host(qadc_adc_index* idx, const std::vector<uint32_t>& stored, uint64_t n_stored, int nq) {
    idx->stream_off.assign((size_t)nq + 1, 0);
    for (int q = 0; q < nq; ++q) idx->stream_off[q + 1] = idx->stream_off[q] + stored[q];
    idx->stream_keys.resize(n_stored);
    idx->stream_vals.resize(n_stored);
    const uint32_t* rec = idx->h_packed.p;
    // (an LSD radix sort of (scan index, record) pairs, 11-bit digits over the bits the largest scan index needs: a
    // comparison sort of the ~5000 records of a lone query on 10^6 codes cost more host time than the whole device part)
    auto order = [&](int q) {
        const uint64_t o = idx->stream_off[q], n = stored[q];
        const uint32_t* r = rec + 3 * o;
        std::vector<uint64_t> a(n), b(n);
        uint32_t top = 1;
        for (uint64_t i = 0; i < n; ++i) {
            a[i] = ((uint64_t)r[3 * i + 2] << 32) | i;
            top |= r[3 * i + 2];
        }
        int bits = 0;
        while (bits < 32 && (top >> bits)) ++bits;
        for (int shift = 32; shift < 32 + bits; shift += 11) {
            uint32_t count[2049] = {0};
            for (uint64_t i = 0; i < n; ++i) ++count[((a[i] >> shift) & 2047) + 1];
            for (int d = 0; d < 2048; ++d) count[d + 1] += count[d];
            for (uint64_t i = 0; i < n; ++i) b[count[(a[i] >> shift) & 2047]++] = a[i];
            a.swap(b);
        }
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t j = (uint32_t)a[i];
            float v;
            std::memcpy(&v, &r[3 * j], 4);
            idx->stream_vals[o + i] = v;
            idx->stream_keys[o + i] = r[3 * j + 1];
        }
    };
    idx->pool.run(nq, n_stored > 65536 ? 16 : 1, order);
}

// Scans the batch on the device and leaves the ordered candidate stream of every query in idx->stream_* — or, given `out`
// (R <= kAdcReplayMaxR), orders and replays the streams on the device.  The tables are the caller's (`tables`, uploaded with the
// items) or already in device memory (`d_ready`, enqueued on the index's stream before this call; tables is null then).  filters:
// null, or the filters of these nq queries (entry 0 = the batch's first query; NULL entries legal) — a batch in which no query has
// one is staged and scanned as a call without `filters`.
int scan_batch(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, const float* d_ready, int R,
               int sum_mode, const DeviceOut* out = nullptr, const qadc_adc_filter* const* filters = nullptr) {
    if (int rc = check_query_args(idx, nq, ma, assign, d_ready ? static_cast<const void*>(d_ready) : tables, R, sum_mode)) return rc;
    HIPCHECK(hipSetDevice(idx->device));
    Batch b;
    b.plan = plan_levels(idx->sizes.data(), nq, ma, assign, R);
    if (!b.plan.refused.empty()) return fail(QADC_E_ARG, b.plan.refused);
    if (int rc = stage_batch(idx, b, nq, ma, assign, tables, d_ready, any_filter(filters, nq) ? filters : nullptr)) return rc;
    if (int rc = run_levels(idx, b, nq, ma, R, sum_mode, !out)) return rc;
    if (out) return finish_on_device(idx, b, nq, R, *out);
    order_on_host(idx, b.stored, b.n_stored, nq);
    return QADC_OK;
}

// The heap arrays of every query from the ordered stream of the last scan (db_query.cpp:31-33: the R sentinels first).
void replay_heaps(qadc_adc_index* idx, int nq, int R, uint32_t* keys, float* values, int32_t* sizes) {
    auto replay = [&](int q) {
        qadc::kv_heap<unsigned, float> bh(R);
        for (int t = 0; t < R; ++t) bh.push(0, std::numeric_limits<float>::max() - t);   // db_query.cpp:31-33
        for (uint64_t i = idx->stream_off[q]; i < idx->stream_off[q + 1]; ++i) bh.push(idx->stream_keys[i], idx->stream_vals[i]);
        if (keys) std::copy(bh.keys(), bh.keys() + bh.size(), keys + (size_t)q * R);
        if (values) std::copy(bh.values(), bh.values() + bh.size(), values + (size_t)q * R);
        if (sizes) sizes[q] = bh.size();
    };
    idx->pool.run(nq, idx->stream_off[nq] > 65536 ? 16 : 1, replay);
}

// The ordered stream of the last scan into the caller's buffers (qadc_adc_query_scan_candidates' contract).
int copy_stream(qadc_adc_index* idx, int nq, uint64_t cand_capacity, uint32_t* cand_keys, float* cand_vals, uint64_t* offsets) {
    std::copy(idx->stream_off.begin(), idx->stream_off.end(), offsets);
    const uint64_t n = idx->stream_off[nq];
    if (n > cand_capacity)
        return fail(QADC_E_CAPACITY, "the candidate stream has " + std::to_string(n) + " entries (offsets[nq]); the buffers hold " +
                                         std::to_string(cand_capacity));
    if (n && (!cand_keys || !cand_vals)) return fail(QADC_E_ARG, "cand_keys and cand_vals are required");
    std::copy(idx->stream_keys.begin(), idx->stream_keys.end(), cand_keys);
    std::copy(idx->stream_vals.begin(), idx->stream_vals.end(), cand_vals);
    return QADC_OK;
}

// queries per sub-batch: whole queries whose tables fit the budget, at least one
int queries_per_pass(const qadc_adc_index* idx, int nq, int ma) {
    const uint64_t per_query = (uint64_t)ma * idx->nsq * idx->centroids * 4;
    return (int)std::min<uint64_t>((uint64_t)nq, std::max<uint64_t>(1, idx->table_budget / per_query));
}

// The ordered streams of the sub-batches of one call, appended pass by pass; a single pass leaves its stream where scan_batch put it.
struct StreamGather {
    bool on;
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> keys;
    std::vector<float> vals;
    explicit StreamGather(bool on_) : on(on_) {}
    void append(const qadc_adc_index* idx, int n) {
        if (!on) return;
        const uint64_t base = off.back();
        for (int q = 1; q <= n; ++q) off.push_back(base + idx->stream_off[q]);
        keys.insert(keys.end(), idx->stream_keys.begin(), idx->stream_keys.end());
        vals.insert(vals.end(), idx->stream_vals.begin(), idx->stream_vals.end());
    }
    void publish(qadc_adc_index* idx) {
        if (!on) return;
        idx->stream_off.swap(off);
        idx->stream_keys.swap(keys);
        idx->stream_vals.swap(vals);
    }
};

// scan_batch on the caller's host tables, in sub-batches of whole queries whose tables fit the table budget: the host and the
// device staging buffers never hold more than one pass's tables (a 16-bit table is up to 2 MiB per (query, probe)).
int scan_host_tables(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R, int sum_mode,
                     const DeviceOut* out = nullptr, const qadc_adc_filter* const* filters = nullptr) {
    if (int rc = check_query_args(idx, nq, ma, assign, tables, R, sum_mode)) return rc;
    const int per = queries_per_pass(idx, nq, ma);
    if (per >= nq) return scan_batch(idx, nq, ma, assign, tables, nullptr, R, sum_mode, out, filters);
    const size_t per_query = (size_t)ma * idx->nsq * idx->centroids;
    StreamGather gather(!out);
    for (int q0 = 0; q0 < nq; q0 += per) {
        const int n = std::min(per, nq - q0);
        const DeviceOut sub = out ? DeviceOut{out->keys + (size_t)q0 * R, out->values + (size_t)q0 * R, out->sizes + q0} : DeviceOut{};
        if (int rc = scan_batch(idx, n, ma, assign + (size_t)q0 * ma, tables + (size_t)q0 * per_query, nullptr, R, sum_mode, out ? &sub : nullptr,
                                filters ? filters + q0 : nullptr))   // (a sub-batch numbers its queries from 0: its table starts at query q0 of the call)
            return rc;
        gather.append(idx, n);
    }
    gather.publish(idx);
    return QADC_OK;
}

// ---- feeders: query vectors -> assign + device tables (qadc_adc_search*) ----


// The quantizers of one search call, read only: the index's own, or — a view — its source's as they stand when the call is
// made.  Nothing of them is written into a view.
struct Feeders {
    int dim, K;                        // K 0: flat (no coarse quantizer)
    const float *codebooks, *cbnorm;   // cbnorm: ||c||^2 of the codebook rows under the call's sum_mode (null for a view: its builder takes none)
    const float *rotation, *coarse;    // [dim][dim], null: plain PQ;  [K][dim], null: flat
    const float* cnorm;                // [K] ||centroid||^2 under the call's sum_mode
};

int refuse_on_view(const qadc_adc_index* idx, const char* call) {
    if (idx && idx->src)
        return fail(QADC_E_ARG, std::string(call) + ": the index is a view of a 4-bit index and takes its database and its quantizers from "
                                                    "that index (qadc_index_add_partitions, qadc_index_set_pq / _set_rotation / _set_coarse)");
    return QADC_OK;
}

int check_search_args(const qadc_adc_index* idx, const Feeders& f, int nq, const float* queries, int ma, int table_form, int sum_mode) {
    if (nq < 1 || ma < 1 || ma >= 16384 || !queries) return fail(QADC_E_ARG, "need queries, nq >= 1 and 1 <= ma < 16384");
    if (table_form < 0 || table_form > 2) return fail(QADC_E_ARG, "table_form is 0 (direct), 1 (BLAS expansion) or 2 (nns_engine's rule)");
    if (sum_mode != 0 && sum_mode != 1) return fail(QADC_E_ARG, "sum_mode is 0 (source order) or 1 (as compiled)");
    const int parts = (int)idx->sizes.size();
    if (f.K) {
        if (f.K != parts)
            return fail(QADC_E_ARG, "the coarse quantizer has " + std::to_string(f.K) + " centroids and the index " +
                                        std::to_string(parts) + " partitions");
        if (ma > f.K) return fail(QADC_E_ARG, "ma = " + std::to_string(ma) + " exceeds the " + std::to_string(f.K) + " coarse centroids");
    } else if (parts < 1) {
        return fail(QADC_E_ARG, "a flat index (no coarse quantizer) probes partition 0: the index has no partition");
    }
    return QADC_OK;
}

// Opens a search call: resolves the quantizers, checks the call's arguments against them and makes the index's device current.  A view's
// ||centroid||^2 are computed here, under this call's sum_mode, on the index's stream (the source may have replaced its centroids).
int resolve_feeders(qadc_adc_index* idx, int nq, const float* queries, int ma, int table_form, int sum_mode, Feeders* f) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    const size_t mode = sum_mode == 1;   // (a sum_mode that is neither 0 nor 1 is refused below)
    if (idx->src) {
        const FeederState& s = idx->src->feed;
        *f = Feeders{s.dim, s.K, s.d_codebooks.p, nullptr, s.has_rotation ? s.d_rotation.p : nullptr, s.K ? s.d_coarse.p : nullptr, nullptr};
    } else {
        *f = Feeders{idx->dim, idx->K, idx->d_codebooks.p, idx->d_cbnorm.p + mode * idx->nsq * idx->centroids, idx->rotated ? idx->d_rotation.p : nullptr,
                     idx->K ? idx->d_coarse.p : nullptr, idx->d_cnorm.p + mode * idx->K};
    }
    if (!f->dim)
        return fail(QADC_E_ARG, idx->src ? "qadc_index_set_pq has not been called on the view's source index: it has no codebooks"
                                         : "qadc_adc_index_set_pq has not been called: the index has no codebooks");
    if (int rc = check_search_args(idx, *f, nq, queries, ma, table_form, sum_mode)) return rc;
    HIPCHECK(hipSetDevice(idx->device));
    if (idx->src && f->K) {
        HIPCHECK(idx->d_cnorm.ensure((size_t)f->K));
        qadc::launch_row_sqnorm(f->coarse, f->K, f->dim, sum_mode, idx->d_cnorm.p, idx->stream);
        f->cnorm = idx->d_cnorm.p;
    }
    return QADC_OK;
}

// Uploads the queries (d_side: they are device memory already and are read where they lie) and leaves assign [nq][ma] in idx->d_assign, its copy to idx->h_assign enqueued with idx->ev_assign
// recorded behind it: find_k_neighbors (neighbors.cpp:30-76) through the coarse kernels of the 4-bit index, or all zero for a
// flat index (flat_db::assign_compute_residuals, databases.hpp:93-101).
int enqueue_assign(qadc_adc_index* idx, const Feeders& f, int nq, const float* queries, int ma, int sum_mode, bool d_side = false) {
    HIPCHECK(idx->d_queries.ensure((size_t)nq * f.dim));
    HIPCHECK(idx->d_assign.ensure((size_t)nq * ma));
    HIPCHECK(idx->h_assign.ensure((size_t)nq * ma));
    if (d_side) {   // read where they are (no memcpy on a caller's device pointer: see launch_adc_copy_words)
        idx->cur_queries = queries;
    } else {
        HIPCHECK(hipMemcpyAsync(idx->d_queries.p, queries, (size_t)nq * f.dim * 4, hipMemcpyHostToDevice, idx->stream));
        idx->cur_queries = idx->d_queries.p;
    }
    if (f.K) {
        const int chunk = std::min(nq, kCoarseChunk);
        HIPCHECK(idx->d_cdist.ensure((size_t)chunk * f.K));
        HIPCHECK(idx->d_qnorm.ensure(chunk));
        if (ma > 256) HIPCHECK(qadc::coarse_nan_unreplayed_reset(idx->stream));
        for (int o = 0; o < nq; o += kCoarseChunk)
            qadc::launch_coarse_assign(idx->cur_queries + (size_t)o * f.dim, f.coarse, std::min(kCoarseChunk, nq - o), f.K, f.dim, ma,
                                       idx->d_qnorm.p, f.cnorm, sum_mode, idx->d_cdist.p, idx->d_assign.p + (size_t)o * ma, idx->stream);
        HIPCHECK(hipGetLastError());
    } else {
        HIPCHECK(hipMemsetAsync(idx->d_assign.p, 0, (size_t)nq * ma * 4, idx->stream));
    }
    HIPCHECK(hipMemcpyAsync(idx->h_assign.p, idx->d_assign.p, (size_t)nq * ma * 4, hipMemcpyDeviceToHost, idx->stream));
    HIPCHECK(hipEventRecord(idx->ev_assign, idx->stream));
    return QADC_OK;
}

// Waits for the assign copy; refuses a NaN coarse row the selection could not replay (ma > 256: the counter of launch_coarse_assign).
int wait_assign(qadc_adc_index* idx, const Feeders& f, int ma) {
    HIPCHECK(hipEventSynchronize(idx->ev_assign));
    if (f.K && ma > 256) {
        HIPCHECK(hipStreamSynchronize(idx->stream));
        unsigned int unreplayed = 0;
        HIPCHECK(qadc::coarse_nan_unreplayed_read(&unreplayed));
        if (unreplayed)
            return fail(QADC_E_ARG, "a query has a NaN coarse distance and ma > 256: the reference's heap replay is not available");
    }
    return QADC_OK;
}

// The tables of queries [q0, q0 + nq) of the call into idx->d_tables.
int enqueue_tables(qadc_adc_index* idx, const Feeders& f, int q0, int nq, int ma, int table_form, int sum_mode) {
    const int expansion = table_form == 2 ? (ma > 1) : table_form;   // nns_engine: direct for ma == 1 (query_common.hpp:292-297)
    const float* queries = idx->cur_queries + (size_t)q0 * f.dim;
    const int32_t* assign = idx->d_assign.p + (size_t)q0 * ma;
    if (idx->src) {   // a view: the 16-centroid builder of the 4-bit index, [nq][ma][M][16]
        qadc::launch_build_tables(queries, f.coarse, assign, f.codebooks, f.rotation, nq, ma, idx->nsq, f.dim, expansion, sum_mode,
                                  idx->d_tables.p, idx->stream);
        HIPCHECK(hipGetLastError());
        return QADC_OK;
    }
    HIPCHECK(launch_adc_tables(queries, f.coarse, assign, f.codebooks, f.cbnorm, f.rotation, nq, ma, idx->nsq, idx->centroids, f.dim, expansion,
                                          sum_mode, idx->d_tables.p, idx->stream));
    return QADC_OK;
}

// Feeders + scan of the whole batch in sub-batches; leaves the ordered stream of all nq queries in idx->stream_*, or, given
// `out`, the heaps' arrays of all nq queries there (scan_batch's device finish, sub-batch by sub-batch).  d_side: the queries
// are in device memory.  filters: null, or the filters of the call's nq queries.
int search_batch(qadc_adc_index* idx, int nq, const float* queries, int ma, int R, int table_form, int sum_mode, int32_t* assign_out,
                 const DeviceOut* out = nullptr, bool d_side = false, const qadc_adc_filter* const* filters = nullptr) {
    Feeders f;
    if (int rc = resolve_feeders(idx, nq, queries, ma, table_form, sum_mode, &f)) return rc;
    if (int rc = check_R(R)) return rc;
    const int per = queries_per_pass(idx, nq, ma);
    HIPCHECK(idx->d_tables.ensure((size_t)per * ma * idx->nsq * idx->centroids));
    if (int rc = enqueue_assign(idx, f, nq, queries, ma, sum_mode, d_side)) return rc;
    if (int rc = enqueue_tables(idx, f, 0, per, ma, table_form, sum_mode)) return rc;   // (runs while the host plans the first scan)
    if (int rc = wait_assign(idx, f, ma)) return rc;
    if (assign_out) std::memcpy(assign_out, idx->h_assign.p, (size_t)nq * ma * 4);
    StreamGather gather(!out && per < nq);
    for (int q0 = 0; q0 < nq; q0 += per) {
        const int n = std::min(per, nq - q0);
        if (q0)   // (the scan before it has been waited for: the table buffer is free)
            if (int rc = enqueue_tables(idx, f, q0, n, ma, table_form, sum_mode)) return rc;
        const DeviceOut sub = out ? DeviceOut{out->keys + (size_t)q0 * R, out->values + (size_t)q0 * R, out->sizes + q0} : DeviceOut{};
        if (int rc = scan_batch(idx, n, ma, idx->h_assign.p + (size_t)q0 * ma, nullptr, idx->d_tables.p, R, sum_mode, out ? &sub : nullptr,
                                filters ? filters + q0 : nullptr))
            return rc;
        gather.append(idx, n);
    }
    gather.publish(idx);
    return QADC_OK;
}

// ---- the device finish of the entry points ----

bool device_replay_covers(int R) { return R >= 1 && R <= kAdcReplayMaxR; }

// The device buffers for the heaps' arrays of a call whose outputs are host memory.
int host_call_out(qadc_adc_index* idx, int nq, int R, DeviceOut* out) {
    HIPCHECK(hipSetDevice(idx->device));
    HIPCHECK(idx->d_hkeys.ensure((size_t)nq * R));
    HIPCHECK(idx->d_hvals.ensure((size_t)nq * R));
    HIPCHECK(idx->d_hsizes.ensure(nq));
    *out = DeviceOut{idx->d_hkeys.p, idx->d_hvals.p, idx->d_hsizes.p};
    return QADC_OK;
}

// A batch the device replay does not cover (R > kAdcReplayMaxR), finished on the host from idx->stream_* and uploaded into
// the caller's device arrays (staged in the index's own buffers, then copied by a kernel): the *_device contract stays uniform.
int upload_host_heaps(qadc_adc_index* idx, int nq, int R, const DeviceOut& out) {
    std::vector<uint32_t> keys((size_t)nq * R);
    std::vector<float> values((size_t)nq * R);
    std::vector<int32_t> sizes(nq);
    replay_heaps(idx, nq, R, keys.data(), values.data(), sizes.data());
    idx->host_finishes += (uint64_t)nq;
    DeviceOut own;
    if (int rc = host_call_out(idx, nq, R, &own)) return rc;
    HIPCHECK(hipMemcpyAsync(own.keys, keys.data(), keys.size() * 4, hipMemcpyHostToDevice, idx->stream));
    HIPCHECK(hipMemcpyAsync(own.values, values.data(), values.size() * 4, hipMemcpyHostToDevice, idx->stream));
    HIPCHECK(hipMemcpyAsync(own.sizes, sizes.data(), sizes.size() * 4, hipMemcpyHostToDevice, idx->stream));
    HIPCHECK(launch_adc_copy_words(own.keys, out.keys, keys.size(), idx->stream));
    HIPCHECK(launch_adc_copy_words(own.values, out.values, values.size(), idx->stream));
    HIPCHECK(launch_adc_copy_words(own.sizes, out.sizes, sizes.size(), idx->stream));
    HIPCHECK(hipStreamSynchronize(idx->stream));
    return QADC_OK;
}

// The three shapes of the query entry points.  `produce(out)` runs the batch — scan_batch or search_batch bound to the call's
// arguments — with the device finish into `out`, or, out null, leaving the ordered stream in idx->stream_*.

// Heaps into host arrays: the device finish and a copy of its arrays when it is asked for and covers R, else the host replay.
template <typename Produce>
int heaps_to_host(qadc_adc_index* idx, int nq, int R, uint32_t* keys, float* values, int32_t* sizes, Produce produce) {
    DeviceGuard guard;
    if (idx && idx->finish == QADC_ADC_FINISH_DEVICE && nq >= 1 && device_replay_covers(R)) {
        DeviceOut out;
        if (int rc = host_call_out(idx, nq, R, &out)) return rc;
        if (int rc = produce(&out)) return rc;   // nq R keys, nq R values and nq sizes (any may be null) are all that crosses the bus
        if (keys) HIPCHECK(hipMemcpyAsync(keys, out.keys, (size_t)nq * R * 4, hipMemcpyDeviceToHost, idx->stream));
        if (values) HIPCHECK(hipMemcpyAsync(values, out.values, (size_t)nq * R * 4, hipMemcpyDeviceToHost, idx->stream));
        if (sizes) HIPCHECK(hipMemcpyAsync(sizes, out.sizes, (size_t)nq * 4, hipMemcpyDeviceToHost, idx->stream));
        HIPCHECK(hipStreamSynchronize(idx->stream));
        return QADC_OK;
    }
    if (int rc = produce(nullptr)) return rc;
    replay_heaps(idx, nq, R, keys, values, sizes);
    if (idx->finish == QADC_ADC_FINISH_DEVICE) idx->host_finishes += (uint64_t)nq;
    return QADC_OK;
}

// Heaps into the caller's device arrays.
template <typename Produce>
int heaps_to_device(qadc_adc_index* idx, int nq, int R, uint32_t* d_keys, float* d_values, int32_t* d_sizes, Produce produce) {
    if (int rc = check_R(R)) return rc;
    if (!d_keys || !d_values || !d_sizes) return fail(QADC_E_ARG, "d_keys, d_values and d_sizes are required");
    DeviceGuard guard;
    const DeviceOut out{d_keys, d_values, d_sizes};
    if (device_replay_covers(R)) return produce(&out);
    if (int rc = produce(nullptr)) return rc;
    return upload_host_heaps(idx, nq, R, out);
}

// The ordered candidate stream into the caller's buffers.
template <typename Produce>
int stream_to_host(qadc_adc_index* idx, int nq, uint64_t cand_capacity, uint32_t* cand_keys, float* cand_vals, uint64_t* offsets, Produce produce) {
    if (!offsets) return fail(QADC_E_ARG, "offsets is required");
    DeviceGuard guard;
    if (int rc = produce(nullptr)) return rc;
    return copy_stream(idx, nq, cand_capacity, cand_keys, cand_vals, offsets);
}

// The filters of a *_filtered call, checked before the first HIP call: every entry that is not NULL is on the
// index's device.
int check_query_filters(const qadc_adc_index* idx, int nq, const qadc_adc_filter* const* filters) {
    if (!idx || !filters) return QADC_OK;   // (a null index is refused by the call's own checks)
    for (int q = 0; q < nq; ++q)
        if (filters[q] && filters[q]->device != idx->device)
            return fail(QADC_E_ARG, "filters[" + std::to_string(q) + "] is on device " + std::to_string(filters[q]->device) + " and the index on device " +
                                        std::to_string(idx->device));
    return QADC_OK;
}

// The heaps' arrays in the caller's device memory: written word by word (adc_replay_kernel, adc_copy_words_kernel).
int check_device_heaps(const uint32_t* d_keys, const float* d_values, const int32_t* d_sizes) {
    if (int rc = check_aligned(d_keys, 4, "d_keys")) return rc;
    if (int rc = check_aligned(d_values, 4, "d_values")) return rc;
    return check_aligned(d_sizes, 4, "d_sizes");
}

// The six scanning calls, each entered by its plain form (filters null) and by its _filtered form.
int query_scan_call(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R, int sum_mode, uint32_t* keys,
                    float* values, int32_t* sizes, const qadc_adc_filter* const* filters) {
    if (int rc = check_query_filters(idx, nq, filters)) return rc;
    return heaps_to_host(idx, nq, R, keys, values, sizes,
                         [&](const DeviceOut* out) { return scan_host_tables(idx, nq, ma, assign, tables, R, sum_mode, out, filters); });
}

int query_scan_device_call(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* d_tables, int R, int sum_mode,
                           uint32_t* d_keys, float* d_values, int32_t* d_sizes, const qadc_adc_filter* const* filters) {
    if (int rc = check_aligned(d_tables, 16, "d_tables")) return rc;   // (adc_scan_body stages a table with 16-byte loads)
    if (int rc = check_device_heaps(d_keys, d_values, d_sizes)) return rc;
    if (int rc = check_query_filters(idx, nq, filters)) return rc;
    return heaps_to_device(idx, nq, R, d_keys, d_values, d_sizes,
                           [&](const DeviceOut* out) { return scan_batch(idx, nq, ma, assign, nullptr, d_tables, R, sum_mode, out, filters); });
}

int query_scan_candidates_call(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R, int sum_mode,
                               uint64_t cand_capacity, uint32_t* cand_keys, float* cand_vals, uint64_t* offsets,
                               const qadc_adc_filter* const* filters) {
    if (int rc = check_query_filters(idx, nq, filters)) return rc;
    return stream_to_host(idx, nq, cand_capacity, cand_keys, cand_vals, offsets,
                          [&](const DeviceOut*) { return scan_host_tables(idx, nq, ma, assign, tables, R, sum_mode, nullptr, filters); });
}

int search_call(qadc_adc_index* idx, int nq, const float* queries, int ma, int R, int table_form, int sum_mode, uint32_t* keys, float* values,
                int32_t* sizes, int32_t* assign_out, const qadc_adc_filter* const* filters) {
    if (int rc = check_query_filters(idx, nq, filters)) return rc;
    return heaps_to_host(idx, nq, R, keys, values, sizes, [&](const DeviceOut* out) {
        return search_batch(idx, nq, queries, ma, R, table_form, sum_mode, assign_out, out, false, filters);
    });
}

int search_device_call(qadc_adc_index* idx, int nq, const float* d_queries, int ma, int R, int table_form, int sum_mode, uint32_t* d_keys,
                       float* d_values, int32_t* d_sizes, const qadc_adc_filter* const* filters) {
    if (int rc = check_aligned(d_queries, 4, "d_queries")) return rc;
    if (int rc = check_device_heaps(d_keys, d_values, d_sizes)) return rc;
    if (int rc = check_query_filters(idx, nq, filters)) return rc;
    return heaps_to_device(idx, nq, R, d_keys, d_values, d_sizes, [&](const DeviceOut* out) {
        return search_batch(idx, nq, d_queries, ma, R, table_form, sum_mode, nullptr, out, true, filters);
    });
}

int search_candidates_call(qadc_adc_index* idx, int nq, const float* queries, int ma, int R, int table_form, int sum_mode,
                           uint64_t cand_capacity, uint32_t* cand_keys, float* cand_vals, uint64_t* offsets, int32_t* assign_out,
                           const qadc_adc_filter* const* filters) {
    if (int rc = check_query_filters(idx, nq, filters)) return rc;
    return stream_to_host(idx, nq, cand_capacity, cand_keys, cand_vals, offsets, [&](const DeviceOut*) {
        return search_batch(idx, nq, queries, ma, R, table_form, sum_mode, assign_out, nullptr, false, filters);
    });
}

// ---- range search: qadc_adc_range_*  ----

static_assert(kRangeSortLds == QADC_ADC_RANGE_SORT_LDS, "include/qadc.h names the LDS threshold of adc_range_sort_kernel");

// One pass of a range call: queries [0, nq) scanned over one level under bound[q] = radius[q], their kept rows sorted and appended to the
// held result behind lims.back(); lims grows by nq entries.  Tables as scan_batch takes them.  The first attempt gives every query a
// region of kRangeFirstCap entries; the scan counts every kept row, so a second attempt, if one region overflowed, has room for exactly
// what it keeps (host/adc_plan.hpp: plan_range, plan_range_rerun).
int range_pass(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, const float* d_ready, const float* radius,
               int sum_mode, const qadc_adc_filter* const* filters, std::vector<uint64_t>& lims) {
    if (int rc = check_query_args(idx, nq, ma, assign, d_ready ? static_cast<const void*>(d_ready) : tables, 1, sum_mode)) return rc;
    HIPCHECK(hipSetDevice(idx->device));
    Batch b;
    b.plan = plan_range(idx->sizes.data(), nq, ma, assign);
    if (!b.plan.refused.empty()) return fail(QADC_E_ARG, b.plan.refused);
    uint64_t entries = 0;
    std::string over = range_entries(b.plan.cap, kMaxEntries, &entries);
    if (!over.empty()) return fail(QADC_E_CAPACITY, over);
    if (int rc = stage_batch(idx, b, nq, ma, assign, tables, d_ready, any_filter(filters, nq) ? filters : nullptr)) return rc;
    ScanDb db = scan_db(idx);
    db.qfilters = b.d_qfilters;
    HIPCHECK(idx->h_count.ensure(nq));
    HIPCHECK(idx->h_radius.ensure(nq));
    std::memcpy(idx->h_radius.p, radius, (size_t)nq * 4);
    for (int attempt = 0;; ++attempt) {
        HIPCHECK(hipMemcpyAsync(b.d_bound, idx->h_radius.p, (size_t)nq * 4, hipMemcpyHostToDevice, idx->stream));   // over the staged FLT_MAX
        HIPCHECK(idx->d_vals.ensure(b.entries));
        HIPCHECK(idx->d_keys.ensure(b.entries));
        HIPCHECK(idx->d_sidx.ensure(b.entries));
        b.emit.vals = idx->d_vals.p;
        b.emit.keys = idx->d_keys.p;
        b.emit.sidx = idx->d_sidx.p;
        HIPCHECK(launch_adc_scan(db, sum_mode, b.d_items, 0, (uint32_t)b.plan.items.size(), b.d_assign, ma, b.d_tables, b.d_bound, b.emit, idx->stream));
        HIPCHECK(hipMemcpyAsync(idx->h_count.p, b.emit.count, (size_t)nq * 4, hipMemcpyDeviceToHost, idx->stream));
        HIPCHECK(hipStreamSynchronize(idx->stream));
        if (!plan_range_rerun(b.plan, idx->h_count.p)) break;
        if (attempt) return fail(QADC_E_STATE, "a range pass kept more rows in its second scan than its first scan counted");
        ++idx->reruns;
        over = range_entries(b.plan.cap, kMaxEntries, &entries);
        if (!over.empty()) return fail(QADC_E_CAPACITY, over);
        fill_state(idx, b);
        HIPCHECK(hipMemcpyAsync(idx->d_in.p, idx->h_in.p, b.o_assign, hipMemcpyHostToDevice, idx->stream));
    }
    const uint64_t held = lims.back();
    uint64_t n_stored = 0;
    uint32_t longest = 0;
    for (int q = 0; q < nq; ++q) {
        n_stored += idx->h_count.p[q];
        longest = std::max(longest, idx->h_count.p[q]);
    }
    if (int rc = grow_device(idx->d_rkeys, held, held + n_stored, idx->stream)) return rc;
    if (int rc = grow_device(idx->d_rvals, held, held + n_stored, idx->stream)) return rc;
    if (longest > (uint32_t)kRangeSortLds) {
        HIPCHECK(idx->d_tmp_a.ensure(b.entries));
        HIPCHECK(idx->d_tmp_b.ensure(b.entries));
    }
    if (n_stored) {
        HIPCHECK(launch_adc_range_sort(nq, b.emit, held, idx->d_rkeys.p, idx->d_rvals.p, idx->d_tmp_a.p, idx->d_tmp_b.p, idx->stream));
        HIPCHECK(hipStreamSynchronize(idx->stream));
    }
    for (int q = 0; q < nq; ++q) lims.push_back(lims.back() + idx->h_count.p[q]);
    return QADC_OK;
}

int check_range_args(const qadc_adc_index* idx, int nq, const float* radius, const uint64_t* lims, const qadc_adc_filter* const* filters) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (nq >= 1 && (!radius || !lims)) return fail(QADC_E_ARG, "radius [nq] and lims [nq + 1] are required");
    return check_query_filters(idx, nq, filters);
}

// Closes a range call: the result is held (range_lims) and its row offsets go to the caller.
int publish_range(qadc_adc_index* idx, std::vector<uint64_t>& lims, uint64_t* out) {
    std::copy(lims.begin(), lims.end(), out);
    idx->range_lims.swap(lims);
    return QADC_OK;
}

// The passes of a range call on the caller's tables: host tables in sub-batches of the table budget (scan_host_tables' cut), device
// tables in one.
int range_scan_call(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, const float* d_tables, const float* radius,
                    int sum_mode, const qadc_adc_filter* const* filters, uint64_t* lims_out) {
    if (int rc = check_range_args(idx, nq, radius, lims_out, filters)) return rc;
    if (int rc = check_query_args(idx, nq, ma, assign, d_tables ? static_cast<const void*>(d_tables) : tables, 1, sum_mode)) return rc;
    DeviceGuard guard;
    idx->range_lims.clear();
    std::vector<uint64_t> lims(1, 0);
    const int per = d_tables ? nq : queries_per_pass(idx, nq, ma);
    const size_t per_query = (size_t)ma * idx->nsq * idx->centroids;
    for (int q0 = 0; q0 < nq; q0 += per) {
        const int n = std::min(per, nq - q0);
        if (int rc = range_pass(idx, n, ma, assign + (size_t)q0 * ma, tables ? tables + (size_t)q0 * per_query : nullptr, d_tables, radius + q0,
                                sum_mode, filters ? filters + q0 : nullptr, lims))
            return rc;
    }
    return publish_range(idx, lims, lims_out);
}

// search_batch's feeders in front of range_pass, sub-batch by sub-batch.
int range_search_call(qadc_adc_index* idx, int nq, const float* queries, int ma, const float* radius, int table_form, int sum_mode,
                      const qadc_adc_filter* const* filters, int32_t* assign_out, uint64_t* lims_out, bool d_side) {
    if (int rc = check_range_args(idx, nq, radius, lims_out, filters)) return rc;
    DeviceGuard guard;
    Feeders f;
    if (int rc = resolve_feeders(idx, nq, queries, ma, table_form, sum_mode, &f)) return rc;
    idx->range_lims.clear();
    std::vector<uint64_t> lims(1, 0);
    const int per = queries_per_pass(idx, nq, ma);
    HIPCHECK(idx->d_tables.ensure((size_t)per * ma * idx->nsq * idx->centroids));
    if (int rc = enqueue_assign(idx, f, nq, queries, ma, sum_mode, d_side)) return rc;
    if (int rc = enqueue_tables(idx, f, 0, per, ma, table_form, sum_mode)) return rc;
    if (int rc = wait_assign(idx, f, ma)) return rc;
    if (assign_out) std::memcpy(assign_out, idx->h_assign.p, (size_t)nq * ma * 4);
    for (int q0 = 0; q0 < nq; q0 += per) {
        const int n = std::min(per, nq - q0);
        if (q0)   // (the pass before it has been waited for: the table buffer is free)
            if (int rc = enqueue_tables(idx, f, q0, n, ma, table_form, sum_mode)) return rc;
        if (int rc = range_pass(idx, n, ma, idx->h_assign.p + (size_t)q0 * ma, nullptr, idx->d_tables.p, radius + q0, sum_mode,
                                filters ? filters + q0 : nullptr, lims))
            return rc;
    }
    return publish_range(idx, lims, lims_out);
}

// The held result into the caller's buffers: host memory by copies, device memory by a kernel (launch_adc_copy_words).
int range_collect(qadc_adc_index* idx, uint64_t capacity, uint32_t* keys, float* values, bool d_side) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (idx->range_lims.empty()) return fail(QADC_E_STATE, "no range result is held: call qadc_adc_range_scan* or qadc_adc_range_search* first");
    const uint64_t n = idx->range_lims.back();
    if (capacity < n)
        return fail(QADC_E_CAPACITY, "the range result has " + std::to_string(n) + " rows (lims[nq]); the buffers hold " + std::to_string(capacity));
    if (n == 0) return QADC_OK;
    if (!keys || !values) return fail(QADC_E_ARG, "keys and values are required");
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(idx->device));
    if (d_side) {
        HIPCHECK(launch_adc_copy_words(idx->d_rkeys.p, keys, n, idx->stream));
        HIPCHECK(launch_adc_copy_words(idx->d_rvals.p, values, n, idx->stream));
    } else {
        HIPCHECK(hipMemcpyAsync(keys, idx->d_rkeys.p, n * 4, hipMemcpyDeviceToHost, idx->stream));
        HIPCHECK(hipMemcpyAsync(values, idx->d_rvals.p, n * 4, hipMemcpyDeviceToHost, idx->stream));
    }
    HIPCHECK(hipStreamSynchronize(idx->stream));
    return QADC_OK;
}

// ---- db_add: qadc_adc_index_add_vectors, _reserve, _read_partition.  The flow is csrc/qadc_append.h's, shared
// with the 4-bit index, over idx->store; here are the move step of a relocation and the encoders' last step ----

// The move step of a relocation: every partition from the old buffers, by their offset tables, into the new ones.
int move_parts(const qadc_adc_index* idx, const Relocation& r) {
    const RowStore& st = idx->store;
    const size_t parts = r.plan.cap.size();
    const uint32_t longest = parts ? *std::max_element(r.sizes.begin(), r.sizes.end()) : 0;
    uint32_t* d_sizes = nullptr;
    HIPCHECK(r.tmp.alloc(&d_sizes, parts * 4));
    if (parts) HIPCHECK(hipMemcpyAsync(d_sizes, r.sizes.data(), parts * 4, hipMemcpyHostToDevice, idx->stream));   // (drained before the sizes change)
    if (longest)   // (a partition that holds rows lies in the old buffers and in the old tables)
        HIPCHECK(launch_adc_move_partitions((int)parts, st.code_size, d_sizes, longest, st.codes.p, st.d_off.p, idx->labeled == 1 ? st.labels.p : nullptr,
                                            st.d_lab_off.p, r.codes, r.d_off, idx->labeled == 1 ? r.labels : nullptr, r.d_lab_off, idx->stream));
    return QADC_OK;
}

// The index as the shared flow takes it.  sum_mode: the call's (which of the cached norms the encoders read).
AppendJob make_job(qadc_adc_index* idx, int sum_mode) {
    const size_t mode = sum_mode == 1;
    AppendJob job;
    job.store = &idx->store;
    job.stream = idx->stream;
    job.device = idx->device;
    job.labeled = &idx->labeled;
    job.sizes = idx->sizes;
    job.dim = idx->dim;
    job.K = idx->K;
    job.set_pq = "qadc_adc_index_set_pq";
    job.d_coarse = idx->d_coarse.p;
    job.d_rotation = idx->rotated ? idx->d_rotation.p : nullptr;
    job.d_cnorm = idx->d_cnorm.p + mode * idx->K;
    job.move = [idx](const Relocation& r) { return move_parts(idx, r); };
    job.set_sizes = [idx](const std::vector<uint32_t>& sizes) { idx->sizes = sizes; };
    // the steps and kernels of qadc_adc_encode_host / qadc_adc_encode16_host on the index's own quantizers; the 16-bit encoder's partial
    // picks: the slices of the largest pass and of the last one (a shorter pass is cut finer)
    if (idx->centroids == 65536)
        job.prepare = [idx](AddEncoder& enc, uint64_t count) {
            const int ds = idx->dim / idx->nsq;
            const uint64_t last = count % kAddChunk ? count % kAddChunk : enc.pass;
            const uint64_t entries = std::max(enc.pass * encode16_slices((uint32_t)enc.pass, idx->nsq, ds), last * encode16_slices((uint32_t)last, idx->nsq, ds));
            HIPCHECK(enc.mem.alloc(&enc.d_part, entries * idx->nsq * 8));
            return QADC_OK;
        };
    job.encode = [idx, sum_mode, mode](AddEncoder& enc, const float* d_enc, uint64_t cnt) {
        const float* cbnorm = idx->d_cbnorm.p + mode * idx->nsq * idx->centroids;
        if (idx->centroids == 65536)
            HIPCHECK(launch_adc_encode16(d_enc, (uint32_t)cnt, idx->nsq, idx->dim, idx->d_codebooks.p, cbnorm, sum_mode, enc.d_part,
                                         reinterpret_cast<uint16_t*>(enc.d_codes), idx->stream));
        else
            HIPCHECK(launch_adc_encode(d_enc, cnt, idx->nsq, idx->dim, idx->d_codebooks.p, cbnorm, sum_mode, enc.d_codes, idx->stream));
        return QADC_OK;
    };
    return job;
}

// labelled: the call is qadc_adc_index_add_vectors_labelled / _device, which takes labels [count] and no labels_offset.
int add_vectors(qadc_adc_index* idx, const float* vectors, const uint32_t* labels, bool labelled, uint64_t count, uint32_t labels_offset,
                int sum_mode, bool d_side, const char* call) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (int rc = refuse_on_view(idx, call)) return rc;
    AppendJob job = make_job(idx, sum_mode);
    return append_vectors(job, vectors, labels, labelled, count, labels_offset, sum_mode, d_side, call);
}

// Remove by label over the regions of the owned database (idx->store).
// Capacities, offsets and buffers stay as they are; the sizes are committed once the compaction has completed.
int remove_labels(qadc_adc_index* idx, const uint32_t* list, uint64_t count, uint64_t* removed_out, bool d_side, const char* call) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (idx->src)
        return fail(QADC_E_ARG, std::string(call) + ": the index is a view of a 4-bit index and owns no rows: destroy the view and remove "
                                                    "on the index it views (qadc_index_remove_labels)");
    if (count && !list) return fail(QADC_E_ARG, std::string(call) + ": labels is null");
    const bool holds = std::any_of(idx->sizes.begin(), idx->sizes.end(), [](uint32_t n) { return n != 0; });
    if (holds && idx->labeled != 1)
        return fail(QADC_E_ARG, std::string(call) + ": the index is not labelled: it keys its vectors by position, and a removal would renumber them");
    if (removed_out) *removed_out = 0;
    if (count == 0 || !holds) return QADC_OK;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(idx->device));
    qadc::host::RemoveJob job;
    job.stream = idx->stream;
    job.code_size = idx->code_size();
    job.sizes = idx->sizes;
    job.pinned = &idx->store.h_add;
    for (size_t p = 0; p < idx->sizes.size(); ++p) {
        job.codes.push_back(idx->store.part_codes(p));
        job.labels.push_back(idx->store.part_labels(p));
    }
    if (int rc = qadc::host::remove_rows(job, list, count, d_side)) {
        const std::string msg = qadc::host::g_err;
        (void)hipStreamSynchronize(idx->stream);
        qadc::host::g_err = msg;
        return rc;   // (QADC_E_HIP: where the compaction had started, the touched partitions' contents are unspecified)
    }
    idx->sizes = job.plan.sizes;
    if (removed_out) *removed_out = job.plan.removed;
    return QADC_OK;
}

// The index lets go of its filter (qadc_adc_index_set_filter, qadc_adc_index_destroy): no scan of the index is in flight, every
// scanning call is synchronous.
void release_filter(qadc_adc_index* idx) {
    if (idx->filter) idx->filter->uses.fetch_sub(1);
    idx->filter = nullptr;
}

// qadc_adc_filter_create / _create_device: the bitmap through the mark step of remove-by-label (mark_list, csrc/qadc_remove.h) on a
// stream of the call's own, drained before the call returns — the filter is complete, and immutable, from then on.
int create_filter(qadc_adc_filter** out, int mode, const uint32_t* keys, uint64_t count, int device_id, bool d_side) {
    if (!out) return fail(QADC_E_ARG, "out is null");
    *out = nullptr;
    if (mode != QADC_ADC_FILTER_EXCLUDE && mode != QADC_ADC_FILTER_ALLOW)
        return fail(QADC_E_ARG, "filter mode is 0 (QADC_ADC_FILTER_EXCLUDE) or 1 (QADC_ADC_FILTER_ALLOW)");
    if (count && !keys) return fail(QADC_E_ARG, "keys is null");
    if (d_side)
        if (int rc = check_aligned(keys, 4, "d_keys")) return rc;
    DeviceGuard guard;
    if (int rc = qadc_device_prepare(device_id)) return rc;
    HIPCHECK(hipSetDevice(device_id));
    qadc_adc_filter* f = new qadc_adc_filter();
    f->device = device_id;
    f->mode = mode;
    hipStream_t s = nullptr;
    Scratch tmp;
    PinBuf<uint32_t> pinned;
    auto run = [&]() -> int {
        HIPCHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        if (count == 0) {   // no key: one zero word, in which no key is marked
            f->span = remove_span(0, 0);
            HIPCHECK(f->mem.alloc(&f->bitmap, 4));
            HIPCHECK(hipMemsetAsync(f->bitmap, 0, 4, s));
        } else {
            if (int rc = qadc::host::mark_list(s, keys, count, d_side, &pinned, tmp, f->mem, &f->span, &f->bitmap)) return rc;
            f->lo = f->span.lo;
            f->hi = f->span.lo + f->span.last;
        }
        HIPCHECK(hipStreamSynchronize(s));
        return QADC_OK;
    };
    const int rc = run();
    const std::string msg = qadc::host::g_err;
    if (s) {
        (void)hipStreamSynchronize(s);   // (tmp is freed behind the stream's work on every path)
        (void)hipStreamDestroy(s);
    }
    pinned.release();
    if (rc != QADC_OK) {
        delete f;
        qadc::host::g_err = msg;
        return rc;
    }
    *out = f;
    return QADC_OK;
}

// ---- Reconstruction: the index forms of the PQ decode.  A call first produces a contiguous pass of
// (partition or -1, code row) in scratch and then runs the stateless form's kernels (decode_passes, csrc/qadc_decode.cpp). ----

struct Reconstruct {
    qadc::DecodeQuantizers q;
    int sq_bits = 0, code_bytes = 0, dim = 0;
    std::vector<qadc::DecodePart> parts;
};

// The quantizers and partitions as they stand at the call, and every refusal: before the device is touched.
int reconstruct_open(const qadc_adc_index* idx, const char* call, Reconstruct* rc) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (idx->src) {
        const FeederState& s = idx->src->feed;
        rc->dim = s.dim;
        rc->q = qadc::DecodeQuantizers{s.d_codebooks.p, s.has_rotation ? s.d_rotation.p : nullptr, s.K ? s.d_coarse.p : nullptr, s.K};
    } else {
        rc->dim = idx->dim;
        rc->q = qadc::DecodeQuantizers{idx->d_codebooks.p, idx->rotated ? idx->d_rotation.p : nullptr, idx->K ? idx->d_coarse.p : nullptr, idx->K};
    }
    if (!rc->dim)
        return fail(QADC_E_ARG, std::string(call) + (idx->src ? ": qadc_index_set_pq has not been called on the view's source index: it has no codebooks"
                                                              : ": qadc_adc_index_set_pq has not been called: the index has no codebooks"));
    const size_t parts = idx->sizes.size();
    if (rc->q.K && (size_t)rc->q.K != parts)
        return fail(QADC_E_ARG, std::string(call) + ": the coarse quantizer has " + std::to_string(rc->q.K) + " centroids and the index " +
                                    std::to_string(parts) + " partitions");
    rc->sq_bits = idx->centroids == 16 ? 4 : idx->centroids == 256 ? 8 : 16;
    rc->code_bytes = idx->src ? idx->nsq / 2 : idx->code_size();
    if (int e = qadc::host::decode_shape_check(idx->nsq, rc->sq_bits, rc->dim)) return e;
    rc->parts.resize(parts);
    for (size_t p = 0; p < parts; ++p) {
        const uint32_t n = idx->sizes[p];
        if (idx->src)
            rc->parts[p] = qadc::DecodePart{idx->parts4[p].codes, idx->parts4[p].labels, idx->parts4[p].key_base, n};
        else
            rc->parts[p] = qadc::DecodePart{n ? idx->store.part_codes(p) : nullptr, n && idx->labeled == 1 ? idx->store.part_labels(p) : nullptr, 0, n};
    }
    return QADC_OK;
}

// d_where [count] -> out [count][dim] (d_side: device memory, written by kernels only) in passes of kDecodeChunk rows
int reconstruct_decode(qadc_adc_index* idx, const Reconstruct& rc, const qadc::DecodePart* d_parts, const unsigned long long* d_where,
                       uint64_t count, float* out, bool d_side, Scratch& mem) {
    hipStream_t s = idx->stream;
    const uint64_t chunk = std::min<uint64_t>(qadc::kDecodeChunk, count);
    int32_t* d_assign = nullptr;
    uint8_t* d_codes = nullptr;
    float* d_out = nullptr;
    HIPCHECK(mem.alloc(&d_assign, sizeof(int32_t) * chunk));
    HIPCHECK(mem.alloc(&d_codes, chunk * (uint64_t)rc.code_bytes));
    if (!d_side) HIPCHECK(mem.alloc(&d_out, sizeof(float) * chunk * (uint64_t)rc.dim));
    for (uint64_t first = 0; first < count; first += chunk) {
        const uint64_t rows = std::min(chunk, count - first);
        float* dst = d_side ? out + first * (uint64_t)rc.dim : d_out;
        HIPCHECK(qadc::launch_reconstruct_gather(d_parts, d_where + first, rows, rc.code_bytes, d_assign, d_codes, s));
        if (int e = qadc::host::decode_passes(idx->nsq, rc.sq_bits, rc.dim, rc.q, d_assign, d_codes, rows, nullptr, dst, nullptr, s)) return e;
        if (!d_side) HIPCHECK(hipMemcpyAsync(out + first * (uint64_t)rc.dim, d_out, sizeof(float) * rows * (uint64_t)rc.dim, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));                        // the pass buffers are reused
    }
    return QADC_OK;
}

int upload_parts(const Reconstruct& rc, hipStream_t s, Scratch& mem, qadc::DecodePart** d_parts) {
    HIPCHECK(mem.alloc(d_parts, std::max<size_t>(rc.parts.size(), 1) * sizeof(qadc::DecodePart)));
    if (!rc.parts.empty())
        HIPCHECK(hipMemcpyAsync(*d_parts, rc.parts.data(), rc.parts.size() * sizeof(qadc::DecodePart), hipMemcpyHostToDevice, s));
    return QADC_OK;
}

// keys [count] -> out [count][dim], where_out [count] (nullable).  d_side: keys, out and where_out are device memory of the index's
// device, read and written by kernels only.
int reconstruct_keys(qadc_adc_index* idx, const uint32_t* keys, uint64_t count, float* out, uint64_t* where_out, bool d_side, const char* call) {
    Reconstruct rc;
    if (int e = reconstruct_open(idx, call, &rc)) return e;
    if (count && (!keys || !out)) return fail(QADC_E_ARG, std::string(call) + ": keys and out must not be null with count > 0");
    if (count >= (1ull << 32)) return fail(QADC_E_ARG, std::string(call) + ": count must be below 2^32");
    if (rc.parts.size() > 65535) return fail(QADC_E_ARG, std::string(call) + ": the lookup takes an index of at most 65535 partitions");
    if (count == 0) return QADC_OK;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(idx->device));
    hipStream_t s = idx->stream;
    Scratch mem;
    qadc::DecodePart* d_parts = nullptr;
    if (int e = upload_parts(rc, s, mem, &d_parts)) return e;
    // the sorted distinct keys: ordered on the host.  The device form's list is copied into scratch by a kernel first (the caller's
    // memory is only ever touched by kernels) — the call's one download before the results
    std::vector<uint32_t> sorted(count);
    uint32_t* d_list = nullptr;
    HIPCHECK(mem.alloc(&d_list, count * 4));
    if (d_side) {
        HIPCHECK(qadc::launch_decode_copy_u32(keys, count, d_list, s));
        HIPCHECK(hipMemcpyAsync(sorted.data(), d_list, count * 4, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
    } else {
        std::copy(keys, keys + count, sorted.begin());
        HIPCHECK(hipMemcpyAsync(d_list, keys, count * 4, hipMemcpyHostToDevice, s));
    }
    std::sort(sorted.begin(), sorted.end());
    sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
    const uint64_t distinct = sorted.size();
    const RemoveSpan span = remove_span(sorted.front(), sorted.back());
    uint32_t *d_bitmap = nullptr, *d_sorted = nullptr;
    unsigned long long *d_slots = nullptr, *d_where = nullptr;
    HIPCHECK(mem.alloc(&d_bitmap, span.words * 4));
    HIPCHECK(hipMemsetAsync(d_bitmap, 0, span.words * 4, s));
    HIPCHECK(launch_remove_mark(d_list, count, span.lo, d_bitmap, s));
    HIPCHECK(mem.alloc(&d_sorted, distinct * 4));
    HIPCHECK(hipMemcpyAsync(d_sorted, sorted.data(), distinct * 4, hipMemcpyHostToDevice, s));
    HIPCHECK(mem.alloc(&d_slots, distinct * 8));
    HIPCHECK(hipMemsetAsync(d_slots, 0xff, distinct * 8, s));
    uint32_t longest = 0;
    for (const qadc::DecodePart& p : rc.parts) longest = std::max(longest, p.size);
    HIPCHECK(qadc::launch_reconstruct_find(d_parts, (int)rc.parts.size(), longest, d_bitmap, span.lo, span.last, d_sorted, distinct, d_slots, s));
    HIPCHECK(mem.alloc(&d_where, count * 8));
    HIPCHECK(qadc::launch_reconstruct_read(d_list, count, d_sorted, distinct, d_slots, d_where, s));
    if (where_out) {
        if (d_side)
            HIPCHECK(qadc::launch_decode_copy_where(d_where, count, reinterpret_cast<uint32_t*>(where_out), s));
        else
            HIPCHECK(hipMemcpyAsync(where_out, d_where, count * 8, hipMemcpyDeviceToHost, s));
    }
    const int e = reconstruct_decode(idx, rc, d_parts, d_where, count, out, d_side, mem);
    const std::string msg = qadc::host::g_err;
    (void)hipStreamSynchronize(s);                                // `sorted` and the scratch outlive the stream's work
    qadc::host::g_err = msg;
    return e;
}

// rows [first, first + count) of partition `part`: no lookup
int reconstruct_rows(qadc_adc_index* idx, int part, uint32_t first, uint32_t count, float* out, bool d_side, const char* call) {
    Reconstruct rc;
    if (int e = reconstruct_open(idx, call, &rc)) return e;
    if (part < 0 || part >= (int)rc.parts.size()) return fail(QADC_E_ARG, std::string(call) + ": partition " + std::to_string(part) + " does not exist");
    if ((uint64_t)first + count > rc.parts[(size_t)part].size)
        return fail(QADC_E_ARG, std::string(call) + ": rows [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + count) +
                                    ") lie outside partition " + std::to_string(part) + " of " + std::to_string(rc.parts[(size_t)part].size) + " rows");
    if (count && !out) return fail(QADC_E_ARG, std::string(call) + ": out must not be null with count > 0");
    if (count == 0) return QADC_OK;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(idx->device));
    hipStream_t s = idx->stream;
    Scratch mem;
    qadc::DecodePart* d_parts = nullptr;
    unsigned long long* d_where = nullptr;
    if (int e = upload_parts(rc, s, mem, &d_parts)) return e;
    HIPCHECK(mem.alloc(&d_where, (uint64_t)count * 8));
    HIPCHECK(qadc::launch_reconstruct_iota((uint32_t)part, first, count, d_where, s));
    const int e = reconstruct_decode(idx, rc, d_parts, d_where, count, out, d_side, mem);
    const std::string msg = qadc::host::g_err;
    (void)hipStreamSynchronize(s);
    qadc::host::g_err = msg;
    return e;
}

}  // namespace

extern "C" {

int qadc_adc_index_reconstruct(qadc_adc_index* idx, const uint32_t* keys, uint64_t count, float* out, uint64_t* where_out) {
    return reconstruct_keys(idx, keys, count, out, where_out, false, "qadc_adc_index_reconstruct");
}

int qadc_adc_index_reconstruct_device(qadc_adc_index* idx, const uint32_t* d_keys, uint64_t count, float* d_out, uint64_t* d_where_out) {
    if (int rc = check_aligned(d_keys, 4, "d_keys")) return rc;
    if (int rc = check_aligned(d_out, 4, "d_out")) return rc;
    if (int rc = check_aligned(d_where_out, 4, "d_where_out")) return rc;
    return reconstruct_keys(idx, d_keys, count, d_out, d_where_out, true, "qadc_adc_index_reconstruct_device");
}

int qadc_adc_index_reconstruct_rows(qadc_adc_index* idx, int part, uint32_t first, uint32_t count, float* out) {
    return reconstruct_rows(idx, part, first, count, out, false, "qadc_adc_index_reconstruct_rows");
}

int qadc_adc_index_reconstruct_rows_device(qadc_adc_index* idx, int part, uint32_t first, uint32_t count, float* d_out) {
    if (int rc = check_aligned(d_out, 4, "d_out")) return rc;
    return reconstruct_rows(idx, part, first, count, d_out, true, "qadc_adc_index_reconstruct_rows_device");
}

int qadc_adc_filter_create(qadc_adc_filter** out, int mode, const uint32_t* keys, uint64_t count, int device_id) {
    return create_filter(out, mode, keys, count, device_id, false);
}

int qadc_adc_filter_create_device(qadc_adc_filter** out, int mode, const uint32_t* d_keys, uint64_t count, int device_id) {
    return create_filter(out, mode, d_keys, count, device_id, true);
}

int qadc_adc_filter_info(const qadc_adc_filter* f, int* mode, uint32_t* lo, uint32_t* hi, uint64_t* bitmap_bytes) {
    if (!f) return fail(QADC_E_ARG, "filter is null");
    if (mode) *mode = f->mode;
    if (lo) *lo = f->lo;
    if (hi) *hi = f->hi;
    if (bitmap_bytes) *bitmap_bytes = f->span.words * 4;
    return QADC_OK;
}

int qadc_adc_filter_destroy(qadc_adc_filter* f) {
    if (!f) return QADC_OK;
    const int uses = f->uses.load();
    if (uses)
        return fail(QADC_E_STATE, "the filter is set on " + std::to_string(uses) + " index(es): clear it there first (qadc_adc_index_set_filter "
                                  "with NULL, or destroy the index)");
    DeviceGuard guard;
    (void)hipSetDevice(f->device);
    delete f;
    return QADC_OK;
}

int qadc_adc_index_set_filter(qadc_adc_index* idx, const qadc_adc_filter* f) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (f && f->device != idx->device)
        return fail(QADC_E_ARG, "the filter is on device " + std::to_string(f->device) + " and the index on device " + std::to_string(idx->device));
    if (f) f->uses.fetch_add(1);   // (before the release: setting the filter that is set already keeps it)
    release_filter(idx);
    idx->filter = f;
    return QADC_OK;
}

// An index that owns its codes: nsq sub-quantizers of `centroids` centroids each (256: one byte per sub-quantizer, 65536: two).
static int create_owned(qadc_adc_index** out, int nsq, int centroids, int device_id) {
    if (int rc = qadc_device_prepare(device_id)) return rc;   // (the device's stream set first: DESIGN.md section 5)
    qadc_adc_index* idx = new qadc_adc_index();
    idx->nsq = nsq;
    idx->centroids = centroids;
    idx->store.code_size = idx->code_size();
    idx->device = device_id;
    const hipError_t e = hipStreamCreateWithFlags(&idx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete idx;
        return fail(QADC_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    const hipError_t ee = hipEventCreateWithFlags(&idx->ev_assign, hipEventDisableTiming);
    if (ee != hipSuccess) {
        (void)hipStreamDestroy(idx->stream);
        delete idx;
        return fail(QADC_E_HIP, std::string("hipEventCreate: ") + hipGetErrorString(ee));
    }
    *out = idx;
    return QADC_OK;
}

int qadc_adc_index_create(qadc_adc_index** out, int sq_count, int sq_bits, int device_id) {
    if (!out) return fail(QADC_E_ARG, "out is null");
    DeviceGuard guard;
    *out = nullptr;
    if (sq_bits != 8 || (sq_count != 4 && sq_count != 8 && sq_count != 16))
        return fail(QADC_E_ARG,
                    "Unsupported (nsq,nsq_bits) configuration. Supported configurations are: (16,4) (4,8) (8,8) (16,8) (2,16) (4,16) "
                    "(8,16); this engine takes (4,8) (8,8) (16,8) here, (2,16) (4,16) (8,16) through qadc_adc_index_create16 and (16,4) "
                    "(32,4) as a view (qadc_adc_index_create_view)");
    return create_owned(out, sq_count, 256, device_id);
}

int qadc_adc_index_create16(qadc_adc_index** out, int sq_count, int device_id) {
    if (!out) return fail(QADC_E_ARG, "out is null");
    DeviceGuard guard;
    *out = nullptr;
    if (sq_count != 2 && sq_count != 4 && sq_count != 8)
        return fail(QADC_E_ARG,
                    "Unsupported (nsq,nsq_bits) configuration. Supported configurations are: (16,4) (4,8) (8,8) (16,8) (2,16) (4,16) "
                    "(8,16); qadc_adc_index_create16 takes (2,16) (4,16) (8,16)");
    return create_owned(out, sq_count, 65536, device_id);
}

int qadc_adc_index_create_view(qadc_adc_index** out, qadc_index* src) {
    if (!out) return fail(QADC_E_ARG, "out is null");
    *out = nullptr;
    if (!src) return fail(QADC_E_ARG, "the source index is null");
    if (!src->finalized) return fail(QADC_E_ARG, "the source index is not finalized: call qadc_index_finalize before creating a view");
    if (src->dist) return fail(QADC_E_ARG, "the source index takes part in a multi-GPU merge: a view reads an index that lives on one GPU");
    for (size_t p = 0; p < src->parts.size(); ++p) {
        const Part& pt = src->parts[p];
        if (pt.n != pt.global_n || pt.first_pos != 0 || pt.d_starts)
            return fail(QADC_E_ARG, "the source index is sharded: partition " + std::to_string(p) + " holds " + std::to_string(pt.n) + " of its " +
                                        std::to_string(pt.global_n) + " codes here; a view needs every partition whole");
    }
    DeviceGuard guard;
    if (int rc = qadc_device_prepare(src->device)) return rc;
    HIPCHECK(hipSetDevice(src->device));
    qadc_adc_index* idx = new qadc_adc_index();
    idx->nsq = src->M;
    idx->centroids = 16;
    idx->device = src->device;
    idx->labeled = src->labeled;
    std::vector<Part4> table(src->parts.size());
    for (size_t p = 0; p < src->parts.size(); ++p) {
        const Part& pt = src->parts[p];
        idx->sizes.push_back(pt.n);
        table[p] = Part4{pt.d_codes, src->labeled == 1 ? pt.d_labels : nullptr, pt.key_base, 0};
    }
    hipError_t e = hipStreamCreateWithFlags(&idx->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&idx->ev_assign, hipEventDisableTiming);
    if (e == hipSuccess) e = idx->d_parts4.ensure(std::max<size_t>(table.size(), 1));
    if (e == hipSuccess && !table.empty())
        e = hipMemcpy(idx->d_parts4.p, table.data(), table.size() * sizeof(Part4), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)qadc_adc_index_destroy(idx);
        return fail(QADC_E_HIP, std::string("qadc_adc_index_create_view: ") + hipGetErrorString(e));
    }
    idx->parts4 = table;
    idx->src = src;     // (only now: a failed creation above releases no count)
    ++src->adc_views;
    *out = idx;
    return QADC_OK;
}

int qadc_adc_index_destroy(qadc_adc_index* idx) {
    if (!idx) return QADC_OK;
    DeviceGuard guard;
    (void)hipSetDevice(idx->device);
    if (idx->stream) (void)hipStreamSynchronize(idx->stream);
    if (idx->src) --idx->src->adc_views;   // the view's scans are over: the source may be destroyed again
    release_filter(idx);
    idx->d_parts4.release();
    idx->store.release();
    idx->d_in.release();
    idx->d_vals.release();
    idx->d_keys.release();
    idx->d_sidx.release();
    idx->d_packed.release();
    idx->d_ovals.release();
    idx->d_okeys.release();
    idx->d_tmp_a.release();
    idx->d_tmp_b.release();
    idx->d_hkeys.release();
    idx->d_hvals.release();
    idx->d_hsizes.release();
    idx->d_rkeys.release();
    idx->d_rvals.release();
    idx->h_radius.release();
    idx->h_in.release();
    idx->h_count.release();
    idx->h_packed.release();
    idx->d_codebooks.release();
    idx->d_cbnorm.release();
    idx->d_rotation.release();
    idx->d_coarse.release();
    idx->d_cnorm.release();
    idx->d_queries.release();
    idx->d_qnorm.release();
    idx->d_cdist.release();
    idx->d_tables.release();
    idx->d_assign.release();
    idx->h_assign.release();
    if (idx->ev_assign) (void)hipEventDestroy(idx->ev_assign);
    if (idx->stream) (void)hipStreamDestroy(idx->stream);
    delete idx;
    return QADC_OK;
}

int qadc_adc_index_add_partitions(qadc_adc_index* idx, int part_count, const uint8_t* const* codes, const uint32_t* const* labels,
                                  const uint32_t* sizes) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (int rc = refuse_on_view(idx, "qadc_adc_index_add_partitions")) return rc;
    if (part_count < 0 || (part_count > 0 && (!codes || !sizes))) return fail(QADC_E_ARG, "bad partition arrays");
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(idx->device));
    // all-or-none labels (scanner_simple keys by labels when the database has them: query_common.hpp:106); an empty
    // partition has nothing to key, so its label pointer (often the null data() of an empty vector) is not looked at
    int lab = idx->labeled;
    for (int p = 0; p < part_count; ++p) {
        if (!sizes[p]) continue;
        const int has = labels && labels[p] ? 1 : 0;
        if (!codes[p]) return fail(QADC_E_ARG, "partition " + std::to_string(p) + " has no codes");
        if (lab == -1) lab = has;
        else if (lab != has) return fail(QADC_E_ARG, "Some partitions have labels and some have not");
    }
    RowStore& st = idx->store;
    uint64_t bytes = st.code_bytes, nlab = st.label_count;
    std::vector<uint64_t> off(part_count), loff(part_count);
    for (int p = 0; p < part_count; ++p) {
        off[p] = bytes;
        loff[p] = nlab;
        bytes += align_up((uint64_t)sizes[p] * idx->code_size(), 16);
        if (lab == 1) nlab += sizes[p];
    }
    if (int rc = grow_device(st.codes, st.code_bytes, bytes + 16, idx->stream)) return rc;
    if (lab == 1)
        if (int rc = grow_device(st.labels, st.label_count, std::max<uint64_t>(nlab, 1), idx->stream)) return rc;
    for (int p = 0; p < part_count; ++p) {
        if (!sizes[p]) continue;
        HIPCHECK(hipMemcpy(st.codes.p + off[p], codes[p], (size_t)sizes[p] * idx->code_size(), hipMemcpyHostToDevice));
        if (lab == 1) HIPCHECK(hipMemcpy(st.labels.p + loff[p], labels[p], (size_t)sizes[p] * 4, hipMemcpyHostToDevice));
    }
    HIPCHECK(hipMemset(st.codes.p + bytes, 0, 16));
    idx->labeled = lab;
    st.code_bytes = bytes;
    st.label_count = nlab;
    for (int p = 0; p < part_count; ++p) {
        idx->sizes.push_back(sizes[p]);
        st.caps.push_back(sizes[p]);   // (the region is the aligned size: an append to it relocates)
        st.off.push_back(off[p]);
        st.lab_off.push_back(loff[p]);
    }
    const size_t np = idx->sizes.size();
    HIPCHECK(st.d_off.ensure(std::max<size_t>(np, 1)));
    HIPCHECK(st.d_lab_off.ensure(std::max<size_t>(np, 1)));
    if (np) {
        HIPCHECK(hipMemcpy(st.d_off.p, st.off.data(), np * 8, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(st.d_lab_off.p, st.lab_off.data(), np * 8, hipMemcpyHostToDevice));
    }
    return QADC_OK;
}

int qadc_adc_index_add_vectors(qadc_adc_index* idx, const float* vectors, uint64_t count, uint32_t labels_offset, int sum_mode) {
    return add_vectors(idx, vectors, nullptr, false, count, labels_offset, sum_mode, false, "qadc_adc_index_add_vectors");
}

int qadc_adc_index_add_vectors_device(qadc_adc_index* idx, const float* d_vectors, uint64_t count, uint32_t labels_offset, int sum_mode) {
    if (int rc = check_aligned(d_vectors, 16, "d_vectors")) return rc;   // (adc_encode16_kernel loads a lane's sub-vector 16 bytes at a time)
    return add_vectors(idx, d_vectors, nullptr, false, count, labels_offset, sum_mode, true, "qadc_adc_index_add_vectors_device");
}

int qadc_adc_index_add_vectors_labelled(qadc_adc_index* idx, const float* vectors, const uint32_t* labels, uint64_t count, int sum_mode) {
    return add_vectors(idx, vectors, labels, true, count, 0, sum_mode, false, "qadc_adc_index_add_vectors_labelled");
}

int qadc_adc_index_add_vectors_labelled_device(qadc_adc_index* idx, const float* d_vectors, const uint32_t* d_labels, uint64_t count,
                                               int sum_mode) {
    if (int rc = check_aligned(d_vectors, 16, "d_vectors")) return rc;
    if (int rc = check_aligned(d_labels, 4, "d_labels")) return rc;
    return add_vectors(idx, d_vectors, d_labels, true, count, 0, sum_mode, true, "qadc_adc_index_add_vectors_labelled_device");
}

int qadc_adc_index_remove_labels(qadc_adc_index* idx, const uint32_t* labels, uint64_t count, uint64_t* removed_out) {
    return remove_labels(idx, labels, count, removed_out, false, "qadc_adc_index_remove_labels");
}

int qadc_adc_index_remove_labels_device(qadc_adc_index* idx, const uint32_t* d_labels, uint64_t count, uint64_t* removed_out) {
    if (int rc = check_aligned(d_labels, 4, "d_labels")) return rc;
    return remove_labels(idx, d_labels, count, removed_out, true, "qadc_adc_index_remove_labels_device");
}

int qadc_adc_index_read_partition(qadc_adc_index* idx, int part, uint32_t first, uint32_t count, uint8_t* codes_out, uint32_t* labels_out) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (int rc = refuse_on_view(idx, "qadc_adc_index_read_partition")) return rc;
    const AppendJob job = make_job(idx, 1);
    const bool exists = part >= 0 && part < (int)idx->sizes.size();
    return read_rows(job, part, first, count, exists ? idx->store.part_codes(part) : nullptr,
                     exists && idx->labeled == 1 ? idx->store.part_labels(part) : nullptr, codes_out, labels_out);
}

int qadc_adc_index_reserve(qadc_adc_index* idx, int part_count, const uint32_t* capacities) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (int rc = refuse_on_view(idx, "qadc_adc_index_reserve")) return rc;
    AppendJob job = make_job(idx, 1);
    return reserve_rows(job, part_count, capacities);
}

uint64_t qadc_adc_index_relocations(const qadc_adc_index* idx) { return idx ? idx->store.relocations : 0; }

int qadc_adc_index_partition_count(const qadc_adc_index* idx) { return idx ? (int)idx->sizes.size() : 0; }

uint64_t qadc_adc_index_reruns(const qadc_adc_index* idx) { return idx ? idx->reruns : 0; }

int qadc_adc_index_set_finish(qadc_adc_index* idx, int mode) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (mode != QADC_ADC_FINISH_HOST && mode != QADC_ADC_FINISH_DEVICE)
        return fail(QADC_E_ARG, "finish mode is 0 (host: QADC_ADC_FINISH_HOST) or 1 (device: QADC_ADC_FINISH_DEVICE)");
    idx->finish = mode;
    return QADC_OK;
}

uint64_t qadc_adc_index_host_finishes(const qadc_adc_index* idx) { return idx ? idx->host_finishes : 0; }

uint32_t qadc_adc_index_partition_size(const qadc_adc_index* idx, int part) {
    if (!idx || part < 0 || part >= (int)idx->sizes.size()) return 0;
    return idx->sizes[part];
}

int qadc_adc_query_scan(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R, int sum_mode,
                        uint32_t* keys, float* values, int32_t* sizes) {
    return query_scan_call(idx, nq, ma, assign, tables, R, sum_mode, keys, values, sizes, nullptr);
}

int qadc_adc_query_scan_filtered(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R, int sum_mode,
                                 uint32_t* keys, float* values, int32_t* sizes, const qadc_adc_filter* const* filters) {
    return query_scan_call(idx, nq, ma, assign, tables, R, sum_mode, keys, values, sizes, filters);
}

int qadc_adc_query_scan_device(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* d_tables, int R, int sum_mode,
                               uint32_t* d_keys, float* d_values, int32_t* d_sizes) {
    return query_scan_device_call(idx, nq, ma, assign, d_tables, R, sum_mode, d_keys, d_values, d_sizes, nullptr);
}

int qadc_adc_query_scan_device_filtered(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* d_tables, int R, int sum_mode,
                                        uint32_t* d_keys, float* d_values, int32_t* d_sizes, const qadc_adc_filter* const* filters) {
    return query_scan_device_call(idx, nq, ma, assign, d_tables, R, sum_mode, d_keys, d_values, d_sizes, filters);
}

int qadc_adc_query_scan_candidates(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R,
                                   int sum_mode, uint64_t cand_capacity, uint32_t* cand_keys, float* cand_vals, uint64_t* offsets) {
    return query_scan_candidates_call(idx, nq, ma, assign, tables, R, sum_mode, cand_capacity, cand_keys, cand_vals, offsets, nullptr);
}

int qadc_adc_query_scan_candidates_filtered(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R,
                                            int sum_mode, uint64_t cand_capacity, uint32_t* cand_keys, float* cand_vals, uint64_t* offsets,
                                            const qadc_adc_filter* const* filters) {
    return query_scan_candidates_call(idx, nq, ma, assign, tables, R, sum_mode, cand_capacity, cand_keys, cand_vals, offsets, filters);
}

int qadc_adc_index_set_pq(qadc_adc_index* idx, int dim, const float* codebooks) {
    if (!idx || !codebooks) return fail(QADC_E_ARG, "index or codebooks is null");
    if (int rc = refuse_on_view(idx, "qadc_adc_index_set_pq")) return rc;
    if (dim < 1 || dim % idx->nsq != 0)
        return fail(QADC_E_ARG, "dim = " + std::to_string(dim) + " is not a multiple of sq_count = " + std::to_string(idx->nsq));
    if (dim > kAdcMaxDim) return fail(QADC_E_ARG, "dim must be <= " + std::to_string(kAdcMaxDim));
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(idx->device));
    const size_t rows = (size_t)idx->nsq * idx->centroids;
    HIPCHECK(idx->d_codebooks.ensure(rows * (dim / idx->nsq)));
    HIPCHECK(idx->d_cbnorm.ensure(2 * rows));
    HIPCHECK(hipMemcpyAsync(idx->d_codebooks.p, codebooks, rows * (dim / idx->nsq) * 4, hipMemcpyHostToDevice, idx->stream));
    for (int mode = 0; mode < 2; ++mode)   // ||c||^2 as compute_cross_dists_blas adds it, once per codebook set
        qadc::launch_row_sqnorm(idx->d_codebooks.p, (int)rows, dim / idx->nsq, mode, idx->d_cbnorm.p + mode * rows, idx->stream);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(idx->stream));
    if (dim != idx->dim) {   // a rotation and coarse centroids of another dimension do not carry over
        idx->rotated = false;
        idx->K = 0;
    }
    idx->dim = dim;
    return QADC_OK;
}

int qadc_adc_index_set_rotation(qadc_adc_index* idx, const float* rotation) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (int rc = refuse_on_view(idx, "qadc_adc_index_set_rotation")) return rc;
    if (!idx->dim) return fail(QADC_E_ARG, "qadc_adc_index_set_pq comes first: the rotation is [dim][dim]");
    if (!rotation) {
        idx->rotated = false;
        return QADC_OK;
    }
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(idx->device));
    HIPCHECK(idx->d_rotation.ensure((size_t)idx->dim * idx->dim));
    HIPCHECK(hipMemcpyAsync(idx->d_rotation.p, rotation, (size_t)idx->dim * idx->dim * 4, hipMemcpyHostToDevice, idx->stream));
    HIPCHECK(hipStreamSynchronize(idx->stream));
    idx->rotated = true;
    return QADC_OK;
}

int qadc_adc_index_set_coarse(qadc_adc_index* idx, int K, const float* centroids) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (int rc = refuse_on_view(idx, "qadc_adc_index_set_coarse")) return rc;
    if (!idx->dim) return fail(QADC_E_ARG, "qadc_adc_index_set_pq comes first: the centroids are [K][dim]");
    if (K < 0 || (K > 0 && !centroids)) return fail(QADC_E_ARG, "need K >= 1 centroids (K = 0: a flat index)");
    if (K == 0) {
        idx->K = 0;
        return QADC_OK;
    }
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(idx->device));
    HIPCHECK(idx->d_coarse.ensure((size_t)K * idx->dim));
    HIPCHECK(idx->d_cnorm.ensure(2 * (size_t)K));
    HIPCHECK(hipMemcpyAsync(idx->d_coarse.p, centroids, (size_t)K * idx->dim * 4, hipMemcpyHostToDevice, idx->stream));
    for (int mode = 0; mode < 2; ++mode) qadc::launch_row_sqnorm(idx->d_coarse.p, K, idx->dim, mode, idx->d_cnorm.p + (size_t)mode * K, idx->stream);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(idx->stream));
    idx->K = K;
    return QADC_OK;
}

int qadc_adc_index_set_table_budget(qadc_adc_index* idx, uint64_t bytes) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    idx->table_budget = bytes ? bytes : 1ull << 30;
    return QADC_OK;
}

int qadc_adc_search(qadc_adc_index* idx, int nq, const float* queries, int ma, int R, int table_form, int sum_mode, uint32_t* keys,
                    float* values, int32_t* sizes, int32_t* assign_out) {
    return search_call(idx, nq, queries, ma, R, table_form, sum_mode, keys, values, sizes, assign_out, nullptr);
}

int qadc_adc_search_filtered(qadc_adc_index* idx, int nq, const float* queries, int ma, int R, int table_form, int sum_mode, uint32_t* keys,
                             float* values, int32_t* sizes, int32_t* assign_out, const qadc_adc_filter* const* filters) {
    return search_call(idx, nq, queries, ma, R, table_form, sum_mode, keys, values, sizes, assign_out, filters);
}

int qadc_adc_search_device(qadc_adc_index* idx, int nq, const float* d_queries, int ma, int R, int table_form, int sum_mode,
                           uint32_t* d_keys, float* d_values, int32_t* d_sizes) {
    return search_device_call(idx, nq, d_queries, ma, R, table_form, sum_mode, d_keys, d_values, d_sizes, nullptr);
}

int qadc_adc_search_device_filtered(qadc_adc_index* idx, int nq, const float* d_queries, int ma, int R, int table_form, int sum_mode,
                                    uint32_t* d_keys, float* d_values, int32_t* d_sizes, const qadc_adc_filter* const* filters) {
    return search_device_call(idx, nq, d_queries, ma, R, table_form, sum_mode, d_keys, d_values, d_sizes, filters);
}

// The coarse step of qadc_adc_search alone: resolve_feeders' refusals, enqueue_assign's kernels, wait_assign's NaN refusal.
static int assign_call(qadc_adc_index* idx, int nq, const float* queries, int ma, int sum_mode, int32_t* assign_out, bool d_side) {
    if (!assign_out) return fail(QADC_E_ARG, "assign_out is null");
    if (d_side) {
        if (int rc = check_aligned(queries, 4, "d_queries")) return rc;
        if (int rc = check_aligned(assign_out, 4, "d_assign_out")) return rc;
    }
    DeviceGuard guard;
    Feeders f;
    if (int rc = resolve_feeders(idx, nq, queries, ma, 0, sum_mode, &f)) return rc;
    if (int rc = enqueue_assign(idx, f, nq, queries, ma, sum_mode, d_side)) return rc;
    if (int rc = wait_assign(idx, f, ma)) return rc;
    if (d_side) {
        HIPCHECK(launch_adc_copy_words(idx->d_assign.p, assign_out, (size_t)nq * ma, idx->stream));
        HIPCHECK(hipStreamSynchronize(idx->stream));
    } else {
        std::memcpy(assign_out, idx->h_assign.p, (size_t)nq * ma * 4);
    }
    return QADC_OK;
}

int qadc_adc_index_assign(qadc_adc_index* idx, int nq, const float* queries, int ma, int sum_mode, int32_t* assign_out) {
    return assign_call(idx, nq, queries, ma, sum_mode, assign_out, false);
}

int qadc_adc_index_assign_device(qadc_adc_index* idx, int nq, const float* d_queries, int ma, int sum_mode, int32_t* d_assign_out) {
    return assign_call(idx, nq, d_queries, ma, sum_mode, d_assign_out, true);
}

// assign, then probed: the two calls one behind the other, each with its own refusals
int qadc_adc_search_exact(qadc_adc_index* idx, qadc_refine* store, int nq, const float* queries, int ma, int R, int sum_mode,
                          const qadc_adc_filter* filter, uint32_t* out_keys, float* out_dist, int32_t* out_sizes, uint64_t* missing_out,
                          int32_t* assign_out) {
    if (nq < 1 || ma < 1) return fail(QADC_E_ARG, "need nq >= 1 and ma >= 1");
    std::vector<int32_t> own;
    if (!assign_out) {
        own.resize((size_t)nq * ma);
        assign_out = own.data();
    }
    if (int rc = assign_call(idx, nq, queries, ma, sum_mode, assign_out, false)) return rc;
    return qadc_refine_knn_probed(store, idx, nq, queries, ma, assign_out, R, filter, out_keys, out_dist, out_sizes, missing_out);
}

int qadc_adc_search_exact_device(qadc_adc_index* idx, qadc_refine* store, int nq, const float* d_queries, int ma, int R, int sum_mode,
                                 const qadc_adc_filter* filter, uint32_t* d_out_keys, float* d_out_dist, int32_t* d_out_sizes,
                                 uint64_t* missing_out, int32_t* d_assign_out) {
    if (nq < 1 || ma < 1) return fail(QADC_E_ARG, "need nq >= 1 and ma >= 1");
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (d_assign_out) {
        if (int rc = assign_call(idx, nq, d_queries, ma, sum_mode, d_assign_out, true)) return rc;
        return qadc_refine_knn_probed_device(store, idx, nq, d_queries, ma, d_assign_out, R, filter, d_out_keys, d_out_dist, d_out_sizes, missing_out);
    }
    // no assign_out: the index's own probe lists, which enqueue_assign leaves in idx->d_assign
    if (int rc = check_aligned(d_queries, 4, "d_queries")) return rc;
    {
        DeviceGuard guard;
        Feeders f;
        if (int rc = resolve_feeders(idx, nq, d_queries, ma, 0, sum_mode, &f)) return rc;
        if (int rc = enqueue_assign(idx, f, nq, d_queries, ma, sum_mode, true)) return rc;
        if (int rc = wait_assign(idx, f, ma)) return rc;
        HIPCHECK(hipStreamSynchronize(idx->stream));
    }
    return qadc_refine_knn_probed_device(store, idx, nq, d_queries, ma, idx->d_assign.p, R, filter, d_out_keys, d_out_dist, d_out_sizes, missing_out);
}

int qadc_adc_search_candidates(qadc_adc_index* idx, int nq, const float* queries, int ma, int R, int table_form, int sum_mode,
                               uint64_t cand_capacity, uint32_t* cand_keys, float* cand_vals, uint64_t* offsets, int32_t* assign_out) {
    return search_candidates_call(idx, nq, queries, ma, R, table_form, sum_mode, cand_capacity, cand_keys, cand_vals, offsets, assign_out, nullptr);
}

int qadc_adc_search_candidates_filtered(qadc_adc_index* idx, int nq, const float* queries, int ma, int R, int table_form, int sum_mode,
                                        uint64_t cand_capacity, uint32_t* cand_keys, float* cand_vals, uint64_t* offsets, int32_t* assign_out,
                                        const qadc_adc_filter* const* filters) {
    return search_candidates_call(idx, nq, queries, ma, R, table_form, sum_mode, cand_capacity, cand_keys, cand_vals, offsets, assign_out, filters);
}

int qadc_adc_range_scan(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, const float* radius, int sum_mode,
                        const qadc_adc_filter* const* filters, uint64_t* lims) {
    if (!tables) return fail(QADC_E_ARG, "assign and tables are required");
    return range_scan_call(idx, nq, ma, assign, tables, nullptr, radius, sum_mode, filters, lims);
}

int qadc_adc_range_scan_device(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* d_tables, const float* radius,
                               int sum_mode, const qadc_adc_filter* const* filters, uint64_t* lims) {
    if (!d_tables) return fail(QADC_E_ARG, "assign and tables are required");
    if (int rc = check_aligned(d_tables, 16, "d_tables")) return rc;
    return range_scan_call(idx, nq, ma, assign, nullptr, d_tables, radius, sum_mode, filters, lims);
}

int qadc_adc_range_search(qadc_adc_index* idx, int nq, const float* queries, int ma, const float* radius, int table_form, int sum_mode,
                          const qadc_adc_filter* const* filters, int32_t* assign_out, uint64_t* lims) {
    return range_search_call(idx, nq, queries, ma, radius, table_form, sum_mode, filters, assign_out, lims, false);
}

int qadc_adc_range_search_device(qadc_adc_index* idx, int nq, const float* d_queries, int ma, const float* radius, int table_form,
                                 int sum_mode, const qadc_adc_filter* const* filters, int32_t* assign_out, uint64_t* lims) {
    if (int rc = check_aligned(d_queries, 4, "d_queries")) return rc;
    return range_search_call(idx, nq, d_queries, ma, radius, table_form, sum_mode, filters, assign_out, lims, true);
}

int qadc_adc_range_collect(qadc_adc_index* idx, uint64_t capacity, uint32_t* keys, float* values) {
    return range_collect(idx, capacity, keys, values, false);
}

int qadc_adc_range_collect_device(qadc_adc_index* idx, uint64_t capacity, uint32_t* d_keys, float* d_values) {
    if (int rc = check_aligned(d_keys, 4, "d_keys")) return rc;
    if (int rc = check_aligned(d_values, 4, "d_values")) return rc;
    return range_collect(idx, capacity, d_keys, d_values, true);
}

int qadc_adc_search_tables(qadc_adc_index* idx, int nq, const float* queries, int ma, int table_form, int sum_mode, int32_t* assign_out,
                           float* tables_out) {
    DeviceGuard guard;
    Feeders f;
    if (int rc = resolve_feeders(idx, nq, queries, ma, table_form, sum_mode, &f)) return rc;
    const int per = queries_per_pass(idx, nq, ma);
    const size_t per_query = (size_t)ma * idx->nsq * idx->centroids;
    HIPCHECK(idx->d_tables.ensure((size_t)per * per_query));
    if (int rc = enqueue_assign(idx, f, nq, queries, ma, sum_mode)) return rc;
    if (int rc = wait_assign(idx, f, ma)) return rc;
    if (assign_out) std::memcpy(assign_out, idx->h_assign.p, (size_t)nq * ma * 4);
    for (int q0 = 0; q0 < nq && tables_out; q0 += per) {
        const int n = std::min(per, nq - q0);
        if (int rc = enqueue_tables(idx, f, q0, n, ma, table_form, sum_mode)) return rc;
        HIPCHECK(hipMemcpyAsync(tables_out + (size_t)q0 * per_query, idx->d_tables.p, (size_t)n * per_query * 4, hipMemcpyDeviceToHost, idx->stream));
        HIPCHECK(hipStreamSynchronize(idx->stream));
    }
    return QADC_OK;
}

int qadc_adc_encode_host(int sq_count, int dim, const float* codebooks, const float* rotation, int K, const float* coarse,
                         const float* vectors, uint64_t n, int sum_mode, int32_t* assign_out, uint8_t* codes, int device_id) {
    if ((sq_count != 4 && sq_count != 8 && sq_count != 16) || dim < 1 || dim % sq_count != 0 || dim > kAdcMaxDim || !codebooks ||
        K < 0 || (K > 0 && !coarse) || (n && (!vectors || !codes)) || (sum_mode != 0 && sum_mode != 1))
        return fail(QADC_E_ARG, "bad arguments (sq_count 4, 8 or 16; dim a multiple of it, at most " + std::to_string(kAdcMaxDim) +
                                    "; sum_mode 0 or 1)");
    DeviceGuard guard;
    if (int rc = qadc_device_prepare(device_id)) return rc;
    HIPCHECK(hipSetDevice(device_id));
    if (!n) return QADC_OK;
    Scratch mem;
    const int ds = dim / sq_count;
    const size_t rows = (size_t)sq_count * 256;
    float *d_cb = nullptr, *d_cbnorm = nullptr, *d_rot = nullptr, *d_coarse = nullptr, *d_v = nullptr, *d_x = nullptr, *d_dist = nullptr;
    int32_t* d_assign = nullptr;
    uint8_t* d_codes = nullptr;
    HIPCHECK(mem.alloc(&d_cb, rows * ds * 4));
    HIPCHECK(mem.alloc(&d_cbnorm, rows * 4));
    HIPCHECK(hipMemcpy(d_cb, codebooks, rows * ds * 4, hipMemcpyHostToDevice));
    qadc::launch_row_sqnorm(d_cb, (int)rows, ds, sum_mode, d_cbnorm, nullptr);
    if (rotation) {
        HIPCHECK(mem.alloc(&d_rot, (size_t)dim * dim * 4));
        HIPCHECK(hipMemcpy(d_rot, rotation, (size_t)dim * dim * 4, hipMemcpyHostToDevice));
    }
    HIPCHECK(mem.alloc(&d_v, n * dim * 4));
    HIPCHECK(mem.alloc(&d_codes, n * sq_count));
    HIPCHECK(hipMemcpy(d_v, vectors, n * dim * 4, hipMemcpyHostToDevice));
    const float* d_enc = d_v;
    if (K > 0) {   // find_k_neighbors(k = 1) on the coarse centroids, chunk by chunk: [chunk][K] distances | chunk norms | K norms
        const uint64_t chunk = std::min<uint64_t>(kCoarseChunk, n);
        HIPCHECK(mem.alloc(&d_coarse, (size_t)K * dim * 4));
        HIPCHECK(hipMemcpy(d_coarse, coarse, (size_t)K * dim * 4, hipMemcpyHostToDevice));
        HIPCHECK(mem.alloc(&d_dist, (chunk * ((uint64_t)K + 1) + K) * 4));
        HIPCHECK(mem.alloc(&d_assign, n * 4));
        float* d_qnorm = d_dist + chunk * (uint64_t)K;
        float* d_cnorm = d_qnorm + chunk;
        qadc::launch_row_sqnorm(d_coarse, K, dim, sum_mode, d_cnorm, nullptr);
        for (uint64_t o = 0; o < n; o += kCoarseChunk)
            qadc::launch_coarse_assign(d_v + o * dim, d_coarse, (int)std::min<uint64_t>(kCoarseChunk, n - o), K, dim, 1, d_qnorm, d_cnorm, sum_mode,
                                       d_dist, d_assign + o, nullptr);
        HIPCHECK(hipGetLastError());
    }
    if (K > 0 || rotation) {
        HIPCHECK(mem.alloc(&d_x, n * dim * 4));
        qadc::launch_residual_rotate(d_v, n, dim, d_coarse, d_assign, d_rot, d_x, nullptr);
        d_enc = d_x;
    }
    HIPCHECK(launch_adc_encode(d_enc, n, sq_count, dim, d_cb, d_cbnorm, sum_mode, d_codes, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(codes, d_codes, n * sq_count, hipMemcpyDeviceToHost));
    if (assign_out && K > 0) HIPCHECK(hipMemcpy(assign_out, d_assign, n * 4, hipMemcpyDeviceToHost));
    return QADC_OK;
}

int qadc_adc_encode16_host(int sq_count, int dim, const float* codebooks, const float* rotation, int K, const float* coarse,
                           const float* vectors, uint64_t n, int sum_mode, int32_t* assign_out, uint8_t* codes, int device_id) {
    if ((sq_count != 2 && sq_count != 4 && sq_count != 8) || dim < 1 || dim % sq_count != 0 || dim > kAdcMaxDim || !codebooks ||
        K < 0 || (K > 0 && !coarse) || (n && (!vectors || !codes)) || (sum_mode != 0 && sum_mode != 1))
        return fail(QADC_E_ARG, "bad arguments (sq_count 2, 4 or 8; dim a multiple of it, at most " + std::to_string(kAdcMaxDim) +
                                    "; sum_mode 0 or 1)");
    DeviceGuard guard;
    if (int rc = qadc_device_prepare(device_id)) return rc;
    HIPCHECK(hipSetDevice(device_id));
    if (!n) return QADC_OK;
    Scratch mem;
    const int ds = dim / sq_count;
    const size_t rows = (size_t)sq_count * 65536;
    const uint64_t pass = std::min<uint64_t>(QADC_ADC_ENCODE16_CHUNK, n);   // vectors in device memory at a time
    float *d_cb = nullptr, *d_cbnorm = nullptr, *d_rot = nullptr, *d_coarse = nullptr, *d_v = nullptr, *d_x = nullptr, *d_dist = nullptr;
    float *d_qnorm = nullptr, *d_cnorm = nullptr;
    int32_t* d_assign = nullptr;
    uint16_t* d_codes = nullptr;
    unsigned long long* d_part = nullptr;
    HIPCHECK(mem.alloc(&d_cb, rows * ds * 4));
    HIPCHECK(mem.alloc(&d_cbnorm, rows * 4));
    HIPCHECK(hipMemcpy(d_cb, codebooks, rows * ds * 4, hipMemcpyHostToDevice));
    qadc::launch_row_sqnorm(d_cb, (int)rows, ds, sum_mode, d_cbnorm, nullptr);   // once per call, not per pass
    if (rotation) {
        HIPCHECK(mem.alloc(&d_rot, (size_t)dim * dim * 4));
        HIPCHECK(hipMemcpy(d_rot, rotation, (size_t)dim * dim * 4, hipMemcpyHostToDevice));
    }
    if (K > 0) {   // [chunk][K] distances | chunk norms | K norms, as qadc_adc_encode_host
        const uint64_t chunk = std::min<uint64_t>(kCoarseChunk, n);
        HIPCHECK(mem.alloc(&d_coarse, (size_t)K * dim * 4));
        HIPCHECK(hipMemcpy(d_coarse, coarse, (size_t)K * dim * 4, hipMemcpyHostToDevice));
        HIPCHECK(mem.alloc(&d_dist, (chunk * ((uint64_t)K + 1) + K) * 4));
        HIPCHECK(mem.alloc(&d_assign, pass * 4));
        d_qnorm = d_dist + chunk * (uint64_t)K;
        d_cnorm = d_qnorm + chunk;
        qadc::launch_row_sqnorm(d_coarse, K, dim, sum_mode, d_cnorm, nullptr);
    }
    HIPCHECK(mem.alloc(&d_v, pass * dim * 4));
    if (K > 0 || rotation) HIPCHECK(mem.alloc(&d_x, pass * dim * 4));
    HIPCHECK(mem.alloc(&d_codes, pass * sq_count * 2));
    // the partial picks of a pass: the slices of the largest pass and of the last one (a shorter pass is cut finer)
    const uint64_t last = n % QADC_ADC_ENCODE16_CHUNK ? n % QADC_ADC_ENCODE16_CHUNK : pass;
    const uint64_t part_entries = std::max(pass * encode16_slices((uint32_t)pass, sq_count, ds), last * encode16_slices((uint32_t)last, sq_count, ds));
    HIPCHECK(mem.alloc(&d_part, part_entries * sq_count * 8));
    HIPCHECK(hipGetLastError());
    for (uint64_t o = 0; o < n; o += QADC_ADC_ENCODE16_CHUNK) {
        const uint64_t cnt = std::min<uint64_t>(QADC_ADC_ENCODE16_CHUNK, n - o);
        HIPCHECK(hipMemcpy(d_v, vectors + o * dim, cnt * dim * 4, hipMemcpyHostToDevice));
        const float* d_enc = d_v;
        if (K > 0) {   // find_k_neighbors(k = 1) on the coarse centroids
            for (uint64_t c = 0; c < cnt; c += kCoarseChunk)
                qadc::launch_coarse_assign(d_v + c * dim, d_coarse, (int)std::min<uint64_t>(kCoarseChunk, cnt - c), K, dim, 1, d_qnorm, d_cnorm,
                                           sum_mode, d_dist, d_assign + c, nullptr);
            HIPCHECK(hipGetLastError());
        }
        if (K > 0 || rotation) {
            qadc::launch_residual_rotate(d_v, cnt, dim, d_coarse, d_assign, d_rot, d_x, nullptr);
            d_enc = d_x;
        }
        HIPCHECK(launch_adc_encode16(d_enc, (uint32_t)cnt, sq_count, dim, d_cb, d_cbnorm, sum_mode, d_part, d_codes, nullptr));
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(hipMemcpy(codes + o * sq_count * 2, d_codes, cnt * sq_count * 2, hipMemcpyDeviceToHost));
        if (assign_out && K > 0) HIPCHECK(hipMemcpy(assign_out + o, d_assign, cnt * 4, hipMemcpyDeviceToHost));
    }
    return QADC_OK;
}

}  // extern "C"
