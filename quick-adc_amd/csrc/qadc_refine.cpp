// Host side of exact re-ranking (qadc_refine_* in include/qadc.h; DESIGN.md sections 11.11 and 11.14): a store of the original
// vectors in device memory, dense over a key range or keyed by label through a hash table, and the call that reorders the candidate
// keys a search returned by their L2 distance to those vectors.  The store belongs to no index and shares nothing with either engine but the device's stream set
// (qadc_device_prepare): it consumes uint32 keys, whoever produced them.  The definition it is held to is host/refine.hpp, the
// launch geometry host/refine_plan.hpp, the kernels csrc/qadc_refine_kernel.hip.  qadc_refine_knn is the
// exhaustive form of the same call, every held key of the store against a batch of queries: geometry host/refine_knn_plan.hpp,
// kernels csrc/qadc_refine_knn_kernel.hip.  qadc_refine_range and qadc_refine_rerank_range are the radius
// query over the same rows — every row, or the candidates of a range result — whose result stays on the store until it is collected:
// geometry host/refine_range_plan.hpp, kernels csrc/qadc_refine_range_kernel.hip.  qadc_refine_knn_probed is
// knn over the rows of the partitions of a float-ADC index that each query probes, keyed as the scan keys them and gathered through
// the store: geometry host/refine_probe_plan.hpp, kernels csrc/qadc_refine_probe_kernel.hip; the index is read through adc_probe_view.
// qadc_refine_set_metric is host state of the handle: every pass of rerank, knn and knn_probed carries it to
// the launchers, which pick the kernels' L2 or inner-product instantiation; the range calls refuse a store whose metric is not L2.
//
// Every array of the *_device calls is read and written by kernels only, so memory of another HIP runtime (torch tensors) is
// legal; for the same reason the library cannot ask which device such a pointer lives on, and does not: as for
// qadc_adc_filter_create_device, the caller names the device by the store it hands the pointers to.
#include "../../include/qadc.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../host/refine.hpp"
#include "qadc_host.h"
#include "qadc_refine.h"

using qadc::host::check_aligned;
using qadc::host::fail;
using qadc::host::DevBuf;
using qadc::host::DeviceGuard;

static_assert(QADC_REFINE_MAX_IN == qadc::refine::kRefinePlanMaxIn && QADC_REFINE_MAX_IN == qadc::refine::kMaxIn, "one limit on r_in");
static_assert(QADC_REFINE_MAX_DIM == qadc::refine::kRefinePlanMaxDim && QADC_REFINE_MAX_DIM == qadc::refine::kMaxDim, "one limit on dim");
static_assert(QADC_REFINE_KNN_MAX_R == qadc::refine::kKnnMaxR, "one limit on the R of knn");
static_assert(QADC_REFINE_RANGE_MAX_ENTRIES == qadc::refine::kRangeMaxEntries, "one limit on the words of a range pass");
static_assert(QADC_REFINE_RANGE_SORT_LDS == qadc::refine::kRangeSortLds, "include/qadc.h names the LDS threshold of refine_range_sort_kernel");
static_assert(QADC_ADC_FILTER_EXCLUDE == qadc::adc::kFilterExclude && QADC_ADC_FILTER_ALLOW == qadc::adc::kFilterAllow &&
                  QADC_ADC_FILTER_EXCLUDE == qadc::refine::kFilterExclude && QADC_ADC_FILTER_ALLOW == qadc::refine::kFilterAllow,
              "the filter modes of the scan, of knn and of its twin");
static_assert(QADC_REFINE_F32 == qadc::refine::kF32 && QADC_REFINE_F16 == qadc::refine::kF16 && QADC_REFINE_SQ8 == qadc::refine::kSQ8,
              "the twin's element types");
static_assert(QADC_REFINE_F32 == (int)qadc::refine::Elem::kF32 && QADC_REFINE_F16 == (int)qadc::refine::Elem::kF16 &&
                  QADC_REFINE_SQ8 == (int)qadc::refine::Elem::kSQ8,
              "the kernels' element types");

static_assert(QADC_REFINE_L2 == qadc::refine::kMetricL2 && QADC_REFINE_IP == qadc::refine::kMetricIP && QADC_REFINE_L2 == qadc::refine::kL2 &&
                  QADC_REFINE_IP == qadc::refine::kIP,
              "the kernels' metrics");

struct qadc_refine {
    int dim = 0, dtype = QADC_REFINE_F32, device = 0;
    int metric = QADC_REFINE_L2;                    // qadc_refine_set_metric: host state, read by every exact call
    uint32_t lo = 0;                                // key of row 0 (fixed by the first add)
    uint64_t rows = 0, cap = 0;                     // rows held / rows the allocation holds
    void* data = nullptr;                           // [cap][dim] floats, halves or bytes
    // an SQ8 store (qadc_refine_create_sq8): vmin, step, inv [dim] each in one allocation, the clamp counter
    float* d_sq = nullptr;
    unsigned long long* d_clamped = nullptr;
    std::vector<float> sq_vmin, sq_step;            // what qadc_refine_sq_info reports
    DevBuf<float> d_get_out;                        // qadc_refine_get: a pass of rows on their way to host memory
    DevBuf<uint8_t> d_get_found;
    uint64_t relocations = 0;                       // adds that moved the rows to grow the allocation
    hipStream_t stream = nullptr;
    // a keyed store (qadc_refine_create_keyed): `rows` are the rows allocated so far, each live or on the free list
    bool keyed = false;
    uint64_t live = 0, used = 0, free_rows = 0;     // keys held / slots live or dead / rows on the free list
    uint32_t *row_key = nullptr, *free_list = nullptr;   // [cap] each: a row's key (0xFFFFFFFF: free) / the free rows' numbers
    qadc::refine::KeyedTable table{nullptr, nullptr, nullptr, 0};
    DevBuf<unsigned long long> d_cnt;               // the counters of a put or a remove
    DevBuf<uint32_t> d_labels, d_slot_of, d_dst;    // a pass of a put: its labels (host form), slots and destination rows
    // per call
    DevBuf<float> d_stage;                          // add from host memory: floats on their way to the convert kernel
    DevBuf<uint64_t> d_words;                       // [pass_nq][r_in]
    DevBuf<unsigned long long> d_missing;
    DevBuf<float> d_queries, d_values, d_out_dist;  // the host form's arrays in device memory
    DevBuf<uint32_t> d_keys, d_out_keys;
    DevBuf<int32_t> d_counts, d_out_sizes;
    // exhaustive search (qadc_refine_knn): the plan's knobs (0: its default) and the scratch of a pass
    uint64_t knn_chunk_rows = 0;
    int knn_pass_nq = 0;
    DevBuf<uint64_t> d_knn_buf, d_knn_bound;        // [pass_nq][groups][buf_cap] / [pass_nq][groups]
    DevBuf<uint32_t> d_knn_cnt;                     // [pass_nq][groups]
    // probed exact search (qadc_refine_knn_probed): knn's knobs and scratch, and beside them the index's
    // partition table, a pass's work and the probe lists on their way to the host (device form) or to the device (search_exact)
    DevBuf<qadc::refine::ProbePart> d_probe_parts;
    DevBuf<qadc::refine::ProbeItem> d_probe_items;
    DevBuf<uint32_t> d_probe_slots;
    DevBuf<int32_t> d_probe_assign;
    // exact range search (qadc_refine_range*): the plan's knobs (0: its default), the held result in buffers
    // no other call writes, and the scratch of a pass
    uint64_t range_region_rows = 0, range_chunk_rows = 0, range_reruns = 0;
    int range_pass_nq = 0;
    std::vector<uint64_t> range_lims;               // [nq + 1] of the last range call; empty: nothing to collect
    DevBuf<uint32_t> d_rkeys;                       // the held rows' keys
    DevBuf<float> d_rdist;                          // ... and distances
    DevBuf<uint64_t> d_rbuf, d_rtmp;                // the regions of a pass and the radix passes' scratch
    DevBuf<uint64_t> d_rmeta;                       // [5][pass_nq]: limit, base, cap, counters, output offsets
    DevBuf<uint32_t> d_rkept;                       // [pass_nq]
    DevBuf<qadc::refine::RangeChunk> d_rchunks;     // the chunk table of a candidate pass
    qadc::refine::Elem elem_type() const { return (qadc::refine::Elem)dtype; }
    size_t elem() const { return qadc::refine::elem_bytes(elem_type()); }
    size_t row_bytes() const { return (size_t)dim * elem(); }
    qadc::refine::SqParams sq() const {
        return d_sq ? qadc::refine::SqParams{d_sq, d_sq + dim, d_sq + 2 * (size_t)dim, d_clamped} : qadc::refine::SqParams{nullptr, nullptr, nullptr, nullptr};
    }
};

namespace {

using namespace qadc::refine;

constexpr uint64_t kStageFloats = 1ull << 24;   // floats of host memory uploaded per pass of an add (64 MiB)

// room for `need` rows: 1.5 x the allocation or `need`, one device-to-device copy of the rows held
int ensure_rows(qadc_refine* r, uint64_t need, bool exact) {
    if (need <= r->cap) return QADC_OK;
    const uint64_t cap = exact ? need : std::max<uint64_t>(need, r->cap + r->cap / 2);
    if (cap > (1ull << 32)) return fail(QADC_E_ARG, "a store holds at most 2^32 rows");
    void* p = nullptr;
    HIPCHECK(hipMalloc(&p, std::max<size_t>((size_t)cap * r->row_bytes(), 16)));
    if (r->rows) {
        hipError_t e = hipMemcpyAsync(p, r->data, (size_t)r->rows * r->row_bytes(), hipMemcpyDeviceToDevice, r->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return fail(QADC_E_HIP, std::string("moving the rows: ") + hipGetErrorString(e));
        }
        ++r->relocations;
    }
    if (r->data) (void)hipFree(r->data);
    r->data = p;
    r->cap = cap;
    return QADC_OK;
}

// ---- the keyed store ----

uint64_t table_bytes(int bits) { return bits ? (1ull << bits) * kKeyedSlotBytes : 0; }

void free_table(KeyedTable& t) {
    if (t.key) (void)hipFree(t.key);
    if (t.row) (void)hipFree(t.row);
    if (t.win) (void)hipFree(t.win);
    t = KeyedTable{nullptr, nullptr, nullptr, 0};
}

// A cleared table of 2^bits slots holding the live rows of the store; it replaces the store's table, whose dead slots are gone.
int rebuild_table(qadc_refine* r, int bits) {
    KeyedTable t{nullptr, nullptr, nullptr, bits};
    const size_t bytes = (size_t)4 << bits;
    auto run = [&]() -> int {
        HIPCHECK(hipMalloc((void**)&t.key, bytes));
        HIPCHECK(hipMalloc((void**)&t.row, bytes));
        HIPCHECK(hipMalloc((void**)&t.win, bytes));
        HIPCHECK(hipMemsetAsync(t.key, 0xFF, bytes, r->stream));
        HIPCHECK(hipMemsetAsync(t.row, 0xFF, bytes, r->stream));
        HIPCHECK(hipMemsetAsync(t.win, 0, bytes, r->stream));
        HIPCHECK(launch_keyed_rebuild(r->row_key, (uint32_t)r->rows, t, r->stream));
        HIPCHECK(hipStreamSynchronize(r->stream));
        return QADC_OK;
    };
    if (int rc = run()) {
        (void)hipStreamSynchronize(r->stream);
        free_table(t);
        return rc;
    }
    free_table(r->table);
    r->table = t;
    r->used = r->live;
    return QADC_OK;
}

// room for `need` allocated rows of a keyed store: the rows, their keys and the free list, moved by one copy each
int ensure_keyed_rows(qadc_refine* r, uint64_t need, bool exact) {
    if (need <= r->cap) return QADC_OK;
    const uint64_t cap = exact ? need : std::max<uint64_t>(need, r->cap + r->cap / 2);
    void* data = nullptr;
    uint32_t *row_key = nullptr, *free_list = nullptr;
    auto run = [&]() -> int {
        HIPCHECK(hipMalloc(&data, std::max<size_t>((size_t)cap * r->row_bytes(), 16)));
        HIPCHECK(hipMalloc((void**)&row_key, (size_t)cap * 4));
        HIPCHECK(hipMalloc((void**)&free_list, (size_t)cap * 4));
        HIPCHECK(hipMemsetAsync(row_key + r->rows, 0xFF, (size_t)(cap - r->rows) * 4, r->stream));
        if (r->rows) {
            HIPCHECK(hipMemcpyAsync(data, r->data, (size_t)r->rows * r->row_bytes(), hipMemcpyDeviceToDevice, r->stream));
            HIPCHECK(hipMemcpyAsync(row_key, r->row_key, (size_t)r->rows * 4, hipMemcpyDeviceToDevice, r->stream));
        }
        if (r->free_rows) HIPCHECK(hipMemcpyAsync(free_list, r->free_list, (size_t)r->free_rows * 4, hipMemcpyDeviceToDevice, r->stream));
        HIPCHECK(hipStreamSynchronize(r->stream));
        return QADC_OK;
    };
    if (int rc = run()) {
        (void)hipStreamSynchronize(r->stream);
        if (data) (void)hipFree(data);
        if (row_key) (void)hipFree(row_key);
        if (free_list) (void)hipFree(free_list);
        return rc;
    }
    if (r->rows) ++r->relocations;
    if (r->data) (void)hipFree(r->data);
    if (r->row_key) (void)hipFree(r->row_key);
    if (r->free_list) (void)hipFree(r->free_list);
    r->data = data;
    r->row_key = row_key;
    r->free_list = free_list;
    r->cap = cap;
    return QADC_OK;
}

int read_counters(qadc_refine* r, unsigned long long* h) {
    HIPCHECK(hipMemcpyAsync(h, r->d_cnt.p, kKeyedCounters * sizeof(unsigned long long), hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipStreamSynchronize(r->stream));
    return QADC_OK;
}

int keyed_call(qadc_refine* r, const char* call, bool want_keyed) {
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (r->keyed != want_keyed)
        return fail(QADC_E_STATE, std::string(call) + (want_keyed ? ": the store is dense over a key range (qadc_refine_create): it takes qadc_refine_add"
                                                                  : ": the store is keyed (qadc_refine_create_keyed): it takes qadc_refine_put"));
    return QADC_OK;
}

int put_rows(qadc_refine* r, const float* vectors, const uint32_t* labels, uint64_t count, bool d_side, const char* call) {
    if (int rc = keyed_call(r, call, true)) return rc;
    if (count == 0) return QADC_OK;
    if (!vectors || !labels) return fail(QADC_E_ARG, "vectors and labels must not be null");
    if (!d_side)
        for (uint64_t i = 0; i < count; ++i)
            if (labels[i] == kKeyedEmpty)
                return fail(QADC_E_ARG, "labels[" + std::to_string(i) + "] is 0xFFFFFFFF, the filler key of qadc_refine_rerank: no vector can be kept under it");
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    const uint64_t pass = keyed_pass(r->dim);
    HIPCHECK(r->d_cnt.ensure(kKeyedCounters));
    HIPCHECK(r->d_slot_of.ensure((size_t)std::min(pass, count)));
    HIPCHECK(r->d_dst.ensure((size_t)std::min(pass, count)));
    if (!d_side) {
        HIPCHECK(r->d_labels.ensure((size_t)std::min(pass, count)));
        HIPCHECK(r->d_stage.ensure((size_t)(std::min(pass, count) * r->dim)));
    }
    unsigned long long h[kKeyedCounters];
    // before anything is written: the filler key among the labels (device form), and the keys the table does not know
    HIPCHECK(hipMemsetAsync(r->d_cnt.p, 0, kKeyedCounters * sizeof(unsigned long long), r->stream));
    for (uint64_t o = 0; o < count; o += pass) {
        const uint64_t cnt = std::min(pass, count - o);
        const uint32_t* d_lab = labels + o;
        if (!d_side) {
            HIPCHECK(hipMemcpyAsync(r->d_labels.p, labels + o, (size_t)cnt * 4, hipMemcpyHostToDevice, r->stream));
            d_lab = r->d_labels.p;
        }
        HIPCHECK(launch_keyed_precheck(d_lab, cnt, r->table, r->d_cnt.p, r->stream));
        if (!d_side) HIPCHECK(hipStreamSynchronize(r->stream));   // (the label stage is written again by the next pass)
    }
    if (int rc = read_counters(r, h)) return rc;
    if (h[kKeyedCntBad])
        return fail(QADC_E_ARG, std::to_string(h[kKeyedCntBad]) + " labels are 0xFFFFFFFF, the filler key of qadc_refine_rerank: no vector can be kept under it");
    const KeyedPutPlan plan = plan_put(r->table.bits, r->live, r->used - r->live, h[kKeyedCntAbsent]);
    if (plan.refused) return fail(QADC_E_ARG, "a keyed store holds at most 2^30 keys");
    if (plan.rebuild)
        if (int rc = rebuild_table(r, plan.bits)) return rc;
    for (uint64_t o = 0; o < count; o += pass) {
        const uint32_t cnt = (uint32_t)std::min(pass, count - o);
        const uint32_t* d_lab = labels + o;
        const float* d_vec = vectors + o * r->dim;
        if (!d_side) {
            HIPCHECK(hipMemcpyAsync(r->d_labels.p, labels + o, (size_t)cnt * 4, hipMemcpyHostToDevice, r->stream));
            HIPCHECK(hipMemcpyAsync(r->d_stage.p, vectors + o * r->dim, (size_t)cnt * r->dim * 4, hipMemcpyHostToDevice, r->stream));
            d_lab = r->d_labels.p;
            d_vec = r->d_stage.p;
        }
        HIPCHECK(hipMemsetAsync(r->d_cnt.p, 0, kKeyedCounters * sizeof(unsigned long long), r->stream));
        HIPCHECK(launch_keyed_claim(d_lab, cnt, r->table, r->d_slot_of.p, r->d_cnt.p, r->stream));
        HIPCHECK(launch_keyed_count(cnt, r->table, r->d_slot_of.p, r->d_dst.p, r->d_cnt.p, r->stream));
        if (int rc = read_counters(r, h)) return rc;
        r->used += h[kKeyedCntClaimed];                      // (claimed slots stay, dead, if the pass fails from here on)
        const uint64_t need = h[kKeyedCntNeed], fresh = need > r->free_rows ? need - r->free_rows : 0;
        int rc = r->rows + fresh > kKeyedMaxKeys ? fail(QADC_E_ARG, "a keyed store allocates at most 2^30 rows") : QADC_OK;
        if (rc == QADC_OK && fresh) rc = ensure_keyed_rows(r, r->rows + fresh, false);   // exactly the rows of the new keys; an overwrite allocates nothing
        if (rc != QADC_OK) {
            const std::string msg = qadc_last_error();
            (void)launch_keyed_reset(cnt, r->table, r->d_slot_of.p, r->stream);
            (void)hipStreamSynchronize(r->stream);
            return fail(rc, msg);
        }
        HIPCHECK(launch_keyed_assign(d_lab, cnt, r->table, r->d_slot_of.p, r->d_dst.p, r->row_key, r->free_list, (uint32_t)r->free_rows,
                                     (uint32_t)r->rows, r->d_cnt.p, r->stream));
        HIPCHECK(launch_keyed_store(d_vec, r->d_dst.p, cnt, r->dim, r->data, r->elem_type(), r->sq(), r->stream));
        HIPCHECK(hipStreamSynchronize(r->stream));
        r->live += need;
        r->free_rows -= need - fresh;
        r->rows += fresh;
    }
    return QADC_OK;
}

int remove_rows(qadc_refine* r, const uint32_t* labels, uint64_t count, uint64_t* removed_out, bool d_side, const char* call) {
    if (int rc = keyed_call(r, call, true)) return rc;
    if (removed_out) *removed_out = 0;
    if (count == 0) return QADC_OK;
    if (!labels) return fail(QADC_E_ARG, "labels is null");
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    const uint64_t pass = keyed_pass(0);
    HIPCHECK(r->d_cnt.ensure(kKeyedCounters));
    if (!d_side) HIPCHECK(r->d_labels.ensure((size_t)std::min(pass, count)));
    uint64_t removed = 0;
    for (uint64_t o = 0; o < count && r->live; o += pass) {
        const uint32_t cnt = (uint32_t)std::min(pass, count - o);
        const uint32_t* d_lab = labels + o;
        if (!d_side) {
            HIPCHECK(hipMemcpyAsync(r->d_labels.p, labels + o, (size_t)cnt * 4, hipMemcpyHostToDevice, r->stream));
            d_lab = r->d_labels.p;
        }
        HIPCHECK(hipMemsetAsync(r->d_cnt.p, 0, kKeyedCounters * sizeof(unsigned long long), r->stream));
        HIPCHECK(launch_keyed_remove(d_lab, cnt, r->table, r->row_key, r->free_list, (uint32_t)r->free_rows, r->d_cnt.p, r->stream));
        unsigned long long h[kKeyedCounters];
        if (int rc = read_counters(r, h)) return rc;
        r->live -= h[kKeyedCntRemoved];
        r->free_rows += h[kKeyedCntRemoved];
        removed += h[kKeyedCntRemoved];
    }
    if (removed_out) *removed_out = removed;
    return QADC_OK;
}

// the parameters of an SQ8 store into device memory: inv derived here, once, by the host's division
int upload_sq(qadc_refine* r, const float* vmin, const float* step) {
    const size_t dim = (size_t)r->dim;
    std::vector<float> h(3 * dim);
    std::copy(vmin, vmin + dim, h.begin());
    std::copy(step, step + dim, h.begin() + dim);
    sq_derive_inv(step, r->dim, h.data() + 2 * dim);   // (IEEE division whatever the calling thread's floating-point mode)
    r->sq_vmin.assign(vmin, vmin + dim);
    r->sq_step.assign(step, step + dim);
    HIPCHECK(hipMalloc((void**)&r->d_sq, 3 * dim * sizeof(float)));
    HIPCHECK(hipMalloc((void**)&r->d_clamped, sizeof(unsigned long long)));
    HIPCHECK(hipMemcpyAsync(r->d_sq, h.data(), 3 * dim * sizeof(float), hipMemcpyHostToDevice, r->stream));
    HIPCHECK(hipMemsetAsync(r->d_clamped, 0, sizeof(unsigned long long), r->stream));
    HIPCHECK(hipStreamSynchronize(r->stream));   // (h leaves with this call)
    return QADC_OK;
}

// vmin and step: null but for an SQ8 store (qadc_refine_create_sq8), whose parameters they are
int create_store(qadc_refine** out, int dim, int dtype, int device_id, bool keyed, const float* vmin = nullptr, const float* step = nullptr) {
    if (!out) return fail(QADC_E_ARG, "out is null");
    *out = nullptr;
    if (dim < 1 || dim > QADC_REFINE_MAX_DIM) return fail(QADC_E_ARG, "dim is 1 .. " + std::to_string(QADC_REFINE_MAX_DIM));
    if (dtype == QADC_REFINE_SQ8) {
        if (!vmin || !step)
            return fail(QADC_E_ARG, "dtype 2 (QADC_REFINE_SQ8) needs the range of its rows: qadc_refine_create_sq8");
        if (!sq_params_ok(vmin, step, dim)) return fail(QADC_E_ARG, "vmin and step must be finite and step not negative");
    } else if (dtype != QADC_REFINE_F32 && dtype != QADC_REFINE_F16) {
        return fail(QADC_E_ARG, "dtype is 0 (QADC_REFINE_F32) or 1 (QADC_REFINE_F16)");
    }
    DeviceGuard guard;
    if (int rc = qadc_device_prepare(device_id)) return rc;   // (the device's stream set first: DESIGN.md section 5)
    HIPCHECK(hipSetDevice(device_id));
    qadc_refine* r = new qadc_refine();
    r->dim = dim;
    r->dtype = dtype;
    r->device = device_id;
    r->keyed = keyed;
    const hipError_t e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete r;
        return fail(QADC_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    int rc = QADC_OK;
    if (keyed) rc = rebuild_table(r, kKeyedMinBits);   // the smallest table from the start: every rerank finds one to probe
    if (rc == QADC_OK && dtype == QADC_REFINE_SQ8) rc = upload_sq(r, vmin, step);
    if (rc != QADC_OK) {
        const std::string msg = qadc_last_error();
        qadc_refine_destroy(r);
        return fail(rc, msg);
    }
    *out = r;
    return QADC_OK;
}

int add_rows(qadc_refine* r, const float* vectors, uint64_t count, uint32_t first_key, bool d_side) {
    if (int rc = keyed_call(r, "qadc_refine_add", false)) return rc;
    if (count == 0) return QADC_OK;
    if (!vectors) return fail(QADC_E_ARG, "vectors is null");
    if (r->rows && (uint64_t)first_key != (uint64_t)r->lo + r->rows)
        return fail(QADC_E_ARG, "first_key " + std::to_string(first_key) + " does not continue the store, which holds the keys [" +
                                    std::to_string(r->lo) + ", " + std::to_string((uint64_t)r->lo + r->rows) + ")");
    if ((uint64_t)first_key + count > (1ull << 32)) return fail(QADC_E_ARG, "first_key + count passes 2^32");
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    if (int rc = ensure_rows(r, r->rows + count, false)) return rc;
    char* dst = static_cast<char*>(r->data) + (size_t)r->rows * r->row_bytes();
    const Elem elem = r->elem_type();
    const uint64_t n = count * (uint64_t)r->dim;
    if (d_side) {
        HIPCHECK(launch_refine_convert(vectors, dst, elem, r->sq(), r->dim, n, r->stream));
    } else if (elem == Elem::kF32) {
        HIPCHECK(hipMemcpyAsync(dst, vectors, (size_t)n * 4, hipMemcpyHostToDevice, r->stream));
    } else {
        const uint64_t stage = kStageFloats / (uint64_t)r->dim * (uint64_t)r->dim;   // whole rows: a pass starts at a row's component 0
        HIPCHECK(r->d_stage.ensure((size_t)std::min(n, stage)));
        for (uint64_t i = 0; i < n; i += stage) {
            const uint64_t m = std::min(stage, n - i);
            HIPCHECK(hipMemcpyAsync(r->d_stage.p, vectors + i, (size_t)m * 4, hipMemcpyHostToDevice, r->stream));
            HIPCHECK(launch_refine_convert(r->d_stage.p, dst + (size_t)i * r->elem(), elem, r->sq(), r->dim, m, r->stream));
            HIPCHECK(hipStreamSynchronize(r->stream));   // (the stage is written again by the next pass)
        }
    }
    HIPCHECK(hipStreamSynchronize(r->stream));
    if (r->rows == 0) r->lo = first_key;
    r->rows += count;
    return QADC_OK;
}

int check_rerank(const qadc_refine* r, int nq, const float* queries, int r_in, const uint32_t* keys, int R, const uint32_t* out_keys,
                 const float* out_dist, const int32_t* out_sizes) {
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (nq < 0) return fail(QADC_E_ARG, "nq is negative");
    if (r_in < 1 || r_in > QADC_REFINE_MAX_IN) return fail(QADC_E_ARG, "r_in is 1 .. " + std::to_string(QADC_REFINE_MAX_IN) + " (QADC_REFINE_MAX_IN)");
    if (R < 1) return fail(QADC_E_ARG, "R is at least 1");
    if (nq && (!queries || !keys || !out_keys || !out_dist || !out_sizes))
        return fail(QADC_E_ARG, "queries, keys, out_keys, out_dist and out_sizes must not be null");
    return QADC_OK;
}

// The passes of a call on arrays in device memory; the stream is drained before the call returns.
int rerank_passes(qadc_refine* r, int nq, const float* queries, int r_in, const uint32_t* keys, const int32_t* counts, const float* values,
                  int R, uint32_t* out_keys, float* out_dist, int32_t* out_sizes, uint64_t* missing_out) {
    RefinePlan plan;
    if (!refine_plan(nq, r_in, r->dim, &plan)) return fail(QADC_E_ARG, "no launch geometry for this call");
    HIPCHECK(r->d_words.ensure((size_t)plan.pass_nq * r_in));
    HIPCHECK(r->d_missing.ensure(1));
    HIPCHECK(hipMemsetAsync(r->d_missing.p, 0, sizeof(unsigned long long), r->stream));
    for (int q0 = 0; q0 < nq; q0 += plan.pass_nq) {
        RefinePass p;
        p.rows = r->data;
        p.elem = r->elem_type();
        p.metric = r->metric;
        p.sq = r->sq();
        p.lo = r->lo;
        p.nrows = r->rows;
        p.tkey = r->keyed ? r->table.key : nullptr;
        p.trow = r->table.row;
        p.tbits = r->table.bits;
        p.dim = r->dim;
        p.nq = std::min(plan.pass_nq, nq - q0);
        p.r_in = r_in;
        p.R = R;
        p.queries = queries + (size_t)q0 * r->dim;
        p.keys = keys + (size_t)q0 * r_in;
        p.counts = counts ? counts + q0 : nullptr;
        p.values = values ? values + (size_t)q0 * r_in : nullptr;
        p.words = r->d_words.p;
        p.missing = r->d_missing.p;
        p.out_keys = out_keys + (size_t)q0 * R;
        p.out_dist = out_dist + (size_t)q0 * R;
        p.out_sizes = out_sizes + q0;
        HIPCHECK(launch_refine_dist(p, plan, r->stream));
        HIPCHECK(launch_refine_select(p, plan, r->stream));
    }
    unsigned long long missing = 0;
    HIPCHECK(hipMemcpyAsync(&missing, r->d_missing.p, sizeof(missing), hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipStreamSynchronize(r->stream));
    if (missing_out) *missing_out = missing;
    return QADC_OK;
}

int check_knn(const qadc_refine* r, int nq, const float* queries, int R, const qadc_adc_filter* filter, adc::ScanFilter* scan,
              const uint32_t* out_keys, const float* out_dist, const int32_t* out_sizes) {
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (nq < 0) return fail(QADC_E_ARG, "nq is negative");
    if (R < 1 || R > QADC_REFINE_KNN_MAX_R) return fail(QADC_E_ARG, "R is 1 .. " + std::to_string(QADC_REFINE_KNN_MAX_R) + " (QADC_REFINE_KNN_MAX_R)");
    if (nq && (!queries || !out_keys || !out_dist || !out_sizes))
        return fail(QADC_E_ARG, "queries, out_keys, out_dist and out_sizes must not be null");
    int fdev = -1;
    adc_filter_view(filter, scan, &fdev);
    if (filter && fdev != r->device)
        return fail(QADC_E_ARG, "the filter is on device " + std::to_string(fdev) + " and the store on device " + std::to_string(r->device));
    return QADC_OK;
}

// The passes of an exhaustive search on arrays in device memory; the stream is drained before the call returns.
int knn_passes(qadc_refine* r, int nq, const float* queries, int R, const adc::ScanFilter& filter, uint32_t* out_keys, float* out_dist,
               int32_t* out_sizes) {
    KnnPlan plan;
    if (!knn_plan(nq, r->rows, r->dim, r->dtype, R, r->knn_chunk_rows, r->knn_pass_nq, &plan))
        return fail(QADC_E_ARG, "no launch geometry for this call (qadc_refine_set_knn_plan: R + chunk_rows is at most " +
                                    std::to_string(kKnnMaxSort) + ")");
    const size_t slots = (size_t)plan.pass_nq * plan.groups;
    HIPCHECK(r->d_knn_buf.ensure(slots * (size_t)plan.buf_cap));
    HIPCHECK(r->d_knn_bound.ensure(slots));
    HIPCHECK(r->d_knn_cnt.ensure(slots));
    for (int q0 = 0; q0 < nq; q0 += plan.pass_nq) {
        KnnPass p;
        p.rows = r->data;
        p.elem = r->elem_type();
        p.metric = r->metric;
        p.sq = r->sq();
        p.dim = r->dim;
        p.lo = r->lo;
        p.nrows = r->rows;
        p.row_key = r->keyed ? r->row_key : nullptr;
        p.filter = filter;
        p.nq = std::min(plan.pass_nq, nq - q0);
        p.R = R;
        p.queries = queries + (size_t)q0 * r->dim;
        p.buf = r->d_knn_buf.p;
        p.cnt = r->d_knn_cnt.p;
        p.bound = r->d_knn_bound.p;
        p.out_keys = out_keys + (size_t)q0 * R;
        p.out_dist = out_dist + (size_t)q0 * R;
        p.out_sizes = out_sizes + q0;
        HIPCHECK(hipMemsetAsync(p.cnt, 0, slots * sizeof(uint32_t), r->stream));
        HIPCHECK(hipMemsetAsync(p.bound, 0xFF, slots * sizeof(uint64_t), r->stream));
        for (uint64_t l = 0; l < plan.launches; ++l) {
            HIPCHECK(launch_knn_dist(p, plan, l, r->stream));
            HIPCHECK(launch_knn_select(p, plan, l, r->stream));
        }
        HIPCHECK(launch_knn_final(p, plan, r->stream));
    }
    HIPCHECK(hipStreamSynchronize(r->stream));
    return QADC_OK;
}

// What a probed call reads of its index: the partitions and the set filter (qadc_host.h: adc_probe_view)
struct ProbeIndex {
    std::vector<qadc::host::AdcProbePart> parts;
    adc::ScanFilter filter;
};

int check_probed(const qadc_refine* r, const qadc_adc_index* idx, int nq, const float* queries, int ma, const int32_t* assign, int R,
                 const qadc_adc_filter* filter, adc::ScanFilter* scan, const uint32_t* out_keys, const float* out_dist, const int32_t* out_sizes,
                 ProbeIndex* pi) {
    if (int rc = check_knn(r, nq, queries, R, filter, scan, out_keys, out_dist, out_sizes)) return rc;
    int idev = -1;
    if (int rc = qadc::host::adc_probe_view(idx, &pi->parts, &idev, &pi->filter)) return rc;
    if (idev != r->device)
        return fail(QADC_E_ARG, "the index is on device " + std::to_string(idev) + " and the store on device " + std::to_string(r->device));
    if (ma < 1 || (size_t)ma > pi->parts.size())
        return fail(QADC_E_ARG, "ma is 1 .. the index's partitions (" + std::to_string(pi->parts.size()) + ")");
    if (nq && !assign) return fail(QADC_E_ARG, "assign must not be null");
    return QADC_OK;
}

// The passes of a probed search: every array in device memory but assign [nq][ma], which the planner reads on the host; the stream
// is drained before the call returns.
int probed_passes(qadc_refine* r, const ProbeIndex& pi, int nq, const float* queries, int ma, const int32_t* assign, int R,
                  const adc::ScanFilter& filter, uint32_t* out_keys, float* out_dist, int32_t* out_sizes, uint64_t* missing_out) {
    ProbePlan plan;
    if (!probe_plan(nq, ma, r->dim, R, r->knn_chunk_rows, r->knn_pass_nq, &plan))
        return fail(QADC_E_ARG, "no launch geometry for this call (qadc_refine_set_knn_plan: R + chunk_rows is at most " + std::to_string(kKnnMaxSort) +
                                    ", and chunk_rows at least the probes of a query that share a group, ceil(ma / groups))");
    const int parts = (int)pi.parts.size();
    std::vector<ProbePart> table((size_t)parts);
    std::vector<uint32_t> part_rows((size_t)parts);
    for (int p = 0; p < parts; ++p) {
        table[p] = ProbePart{pi.parts[p].labels, pi.parts[p].key_base, pi.parts[p].rows};
        part_rows[p] = pi.parts[p].rows;
    }
    const size_t slots = (size_t)plan.pass_nq * plan.groups;
    HIPCHECK(r->d_knn_buf.ensure(slots * (size_t)plan.buf_cap));
    HIPCHECK(r->d_knn_bound.ensure(slots));
    HIPCHECK(r->d_knn_cnt.ensure(slots));
    HIPCHECK(r->d_probe_parts.ensure(std::max<size_t>(parts, 1)));
    HIPCHECK(r->d_probe_items.ensure((size_t)plan.pass_nq * ma));
    HIPCHECK(r->d_probe_slots.ensure((size_t)plan.pass_nq * ma));
    HIPCHECK(r->d_missing.ensure(1));
    HIPCHECK(hipMemsetAsync(r->d_missing.p, 0, sizeof(unsigned long long), r->stream));
    if (parts) HIPCHECK(hipMemcpyAsync(r->d_probe_parts.p, table.data(), (size_t)parts * sizeof(ProbePart), hipMemcpyHostToDevice, r->stream));
    std::vector<ProbeWork> works((size_t)plan.passes);   // (alive until the stream is drained: their arrays are uploaded from where they lie)
    for (int q0 = 0, pass = 0; q0 < nq; q0 += plan.pass_nq, ++pass) {
        ProbeWork& w = works[pass];
        ProbePass p;
        p.nq = std::min(plan.pass_nq, nq - q0);
        probe_work(plan, p.nq, ma, assign + (size_t)q0 * ma, part_rows.data(), parts, &w);
        p.rows = r->data;
        p.elem = r->elem_type();
        p.metric = r->metric;
        p.sq = r->sq();
        p.dim = r->dim;
        p.lo = r->lo;
        p.nrows = r->rows;
        p.tkey = r->keyed ? r->table.key : nullptr;
        p.trow = r->table.row;
        p.tbits = r->table.bits;
        p.parts = r->d_probe_parts.p;
        p.index_filter = pi.filter;
        p.filter = filter;
        p.R = R;
        p.queries = queries + (size_t)q0 * r->dim;
        p.items = r->d_probe_items.p;
        p.slots = r->d_probe_slots.p;
        p.buf = r->d_knn_buf.p;
        p.cnt = r->d_knn_cnt.p;
        p.bound = r->d_knn_bound.p;
        p.missing = r->d_missing.p;
        p.out_keys = out_keys + (size_t)q0 * R;
        p.out_dist = out_dist + (size_t)q0 * R;
        p.out_sizes = out_sizes + q0;
        if (!w.items.empty()) {
            HIPCHECK(hipMemcpyAsync(r->d_probe_items.p, w.items.data(), w.items.size() * sizeof(ProbeItem), hipMemcpyHostToDevice, r->stream));
            HIPCHECK(hipMemcpyAsync(r->d_probe_slots.p, w.slots.data(), w.slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice, r->stream));
        }
        HIPCHECK(hipMemsetAsync(p.cnt, 0, slots * sizeof(uint32_t), r->stream));
        HIPCHECK(hipMemsetAsync(p.bound, 0xFF, slots * sizeof(uint64_t), r->stream));
        for (uint64_t l = 0; l < w.launches; ++l) {
            HIPCHECK(launch_probe_dist(p, plan, ProbeLaunch{w.launch_items[(size_t)l], w.launch_slices[(size_t)l], w.slice_rows, l}, r->stream));
            HIPCHECK(launch_probe_select(p, plan, r->stream));
        }
        HIPCHECK(launch_probe_final(p, plan, r->stream));
    }
    unsigned long long missing = 0;
    HIPCHECK(hipMemcpyAsync(&missing, r->d_missing.p, sizeof(missing), hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipStreamSynchronize(r->stream));
    if (missing_out) *missing_out = missing;
    return QADC_OK;
}

// The passes of a read-back: keys in device memory; out and found in device memory (d_side) or in host memory, by way of a stage.
int get_rows(qadc_refine* r, const uint32_t* d_keys, uint64_t count, float* out, uint8_t* found, bool d_side) {
    RefinePass p{};
    p.rows = r->data;
    p.elem = r->elem_type();
    p.sq = r->sq();
    p.lo = r->lo;
    p.nrows = r->rows;
    p.tkey = r->keyed ? r->table.key : nullptr;
    p.trow = r->table.row;
    p.tbits = r->table.bits;
    p.dim = r->dim;
    if (d_side) {
        HIPCHECK(launch_refine_get(p, d_keys, count, out, found, r->stream));
        HIPCHECK(hipStreamSynchronize(r->stream));
        return QADC_OK;
    }
    const uint64_t pass = std::max<uint64_t>(1, kStageFloats / (uint64_t)r->dim);
    HIPCHECK(r->d_get_out.ensure((size_t)(std::min(pass, count) * r->dim)));
    HIPCHECK(r->d_get_found.ensure((size_t)std::min(pass, count)));
    for (uint64_t o = 0; o < count; o += pass) {
        const uint64_t cnt = std::min(pass, count - o);
        HIPCHECK(launch_refine_get(p, d_keys + o, cnt, r->d_get_out.p, r->d_get_found.p, r->stream));
        HIPCHECK(hipMemcpyAsync(out + o * r->dim, r->d_get_out.p, (size_t)cnt * r->dim * 4, hipMemcpyDeviceToHost, r->stream));
        if (found) HIPCHECK(hipMemcpyAsync(found + o, r->d_get_found.p, (size_t)cnt, hipMemcpyDeviceToHost, r->stream));
        HIPCHECK(hipStreamSynchronize(r->stream));   // (the stage is written again by the next pass)
    }
    return QADC_OK;
}

// The range of `n` vectors, in device memory (d_side) or in host memory, which goes through a stage in passes of whole rows: the
// extremes of every launch meet in the same two arrays.  On a stream of the call's own.
int sq_range(const float* vectors, uint64_t n, int dim, bool d_side, float* vmin_out, float* step_out) {
    std::vector<uint32_t> h(2 * (size_t)dim);
    const uint64_t pass = std::max<uint64_t>(1, kStageFloats / (uint64_t)dim);
    Scratch scratch;
    uint32_t* d_ext = nullptr;
    float* d_stage = nullptr;
    HIPCHECK(scratch.alloc(&d_ext, 2 * (size_t)dim * 4));
    if (!d_side && n) HIPCHECK(scratch.alloc(&d_stage, (size_t)(std::min(pass, n) * dim) * 4));
    hipStream_t stream = nullptr;
    HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    auto run = [&]() -> int {
        HIPCHECK(hipMemsetAsync(d_ext, 0xFF, (size_t)dim * 4, stream));
        HIPCHECK(hipMemsetAsync(d_ext + dim, 0, (size_t)dim * 4, stream));
        if (d_side) {
            HIPCHECK(launch_refine_sq_range(vectors, n, dim, d_ext, d_ext + dim, stream));
        } else {
            for (uint64_t o = 0; o < n; o += pass) {
                const uint64_t cnt = std::min(pass, n - o);
                HIPCHECK(hipMemcpyAsync(d_stage, vectors + o * dim, (size_t)cnt * dim * 4, hipMemcpyHostToDevice, stream));
                HIPCHECK(launch_refine_sq_range(d_stage, cnt, dim, d_ext, d_ext + dim, stream));
                HIPCHECK(hipStreamSynchronize(stream));   // (the stage is written again by the next pass)
            }
        }
        HIPCHECK(hipMemcpyAsync(h.data(), d_ext, 2 * (size_t)dim * 4, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        return QADC_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(stream);
    (void)hipStreamDestroy(stream);
    if (rc != QADC_OK) return rc;
    sq_range_finish(h.data(), h.data() + dim, dim, vmin_out, step_out);
    return QADC_OK;
}

int check_sq_range(const float* vectors, uint64_t n, int dim, const float* vmin_out, const float* step_out) {
    if (dim < 1 || dim > QADC_REFINE_MAX_DIM) return fail(QADC_E_ARG, "dim is 1 .. " + std::to_string(QADC_REFINE_MAX_DIM));
    if (!vmin_out || !step_out) return fail(QADC_E_ARG, "vmin_out and step_out must not be null");
    if (n && !vectors) return fail(QADC_E_ARG, "vectors is null");
    return QADC_OK;
}

// ---- exact range search ----

RangeStore range_store(const qadc_refine* r, bool candidates) {
    RangeStore s{};
    s.rows = r->data;
    s.elem = r->elem_type();
    s.sq = r->sq();
    s.dim = r->dim;
    s.lo = r->lo;
    s.nrows = r->rows;
    s.row_key = r->keyed && !candidates ? r->row_key : nullptr;
    s.tkey = r->keyed && candidates ? r->table.key : nullptr;
    s.trow = r->table.row;
    s.tbits = r->table.bits;
    return s;
}

// room for `need` held rows, the first `held` kept: 1.5 x the allocation or `need`, one device-to-device copy each
template <typename T>
int grow_held(qadc_refine* r, DevBuf<T>& b, uint64_t held, uint64_t need) {
    if (need <= b.cap) return QADC_OK;
    DevBuf<T> n;
    HIPCHECK(n.ensure((size_t)std::max<uint64_t>(need, b.cap + b.cap / 2)));
    if (held) {
        hipError_t e = hipMemcpyAsync(n.p, b.p, (size_t)held * sizeof(T), hipMemcpyDeviceToDevice, r->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
        if (e != hipSuccess) {
            n.release();
            return fail(QADC_E_HIP, std::string("moving the held rows: ") + hipGetErrorString(e));
        }
    }
    b.release();
    b = n;
    return QADC_OK;
}

// The five arrays of a pass's meta block, host side and device side
struct RangeMeta {
    std::vector<uint64_t> h;       // [5][n]
    int n = 0;
    uint64_t* limit() { return h.data(); }
    uint64_t* base() { return h.data() + n; }
    uint64_t* cap() { return h.data() + 2 * (size_t)n; }
    uint64_t* cnt() { return h.data() + 3 * (size_t)n; }
    uint64_t* off() { return h.data() + 4 * (size_t)n; }
};

RangeRegions range_regions_of(qadc_refine* r, int n) {
    RangeRegions g{};
    g.nq = n;
    uint64_t* m = r->d_rmeta.p;
    g.limit = m;
    g.base = m + n;
    g.cap = m + 2 * (size_t)n;
    g.cnt = reinterpret_cast<unsigned long long*>(m + 3 * (size_t)n);
    g.buf = r->d_rbuf.p;
    g.tmp = r->d_rtmp.p;
    return g;
}

// The end of a pass, both forms: the regions sorted, the survivors counted, summed into lims and written behind the held rows.
int range_finish_pass(qadc_refine* r, RangeMeta& m, uint64_t entries, std::vector<uint64_t>& lims) {
    const int n = m.n;
    uint64_t longest = 0;
    for (int q = 0; q < n; ++q) longest = std::max(longest, std::min(m.cnt()[q], m.cap()[q]));
    if (const uint64_t scratch = range_scratch_entries(entries, longest)) HIPCHECK(r->d_rtmp.ensure((size_t)scratch));
    HIPCHECK(r->d_rkept.ensure((size_t)n));
    const RangeRegions g = range_regions_of(r, n);
    std::vector<uint32_t> kept((size_t)n);
    HIPCHECK(launch_range_sort(g, r->d_rkept.p, r->stream));
    HIPCHECK(hipMemcpyAsync(kept.data(), r->d_rkept.p, (size_t)n * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipStreamSynchronize(r->stream));
    const uint64_t held = lims.back();
    uint64_t at = held;
    for (int q = 0; q < n; ++q) {
        m.off()[q] = at;
        at += kept[(size_t)q];
        lims.push_back(at);
    }
    if (at == held) return QADC_OK;
    if (!range_held_fits(held, at - held, kRangeMaxEntries))
        return fail(QADC_E_CAPACITY, "the range result of this call exceeds QADC_REFINE_RANGE_MAX_ENTRIES rows");
    if (int rc = grow_held(r, r->d_rkeys, held, at)) return rc;
    if (int rc = grow_held(r, r->d_rdist, held, at)) return rc;
    uint64_t* d_off = r->d_rmeta.p + 4 * (size_t)n;
    HIPCHECK(hipMemcpyAsync(d_off, m.off(), (size_t)n * 8, hipMemcpyHostToDevice, r->stream));
    HIPCHECK(launch_range_compact(g, d_off, r->d_rkeys.p, r->d_rdist.p, r->stream));
    HIPCHECK(hipStreamSynchronize(r->stream));
    return QADC_OK;
}

// One pass of the exhaustive form over n queries in device memory: the first run with regions of plan.region_rows words, a second
// with regions of exactly the counted sizes where one overflowed.
int range_pass(qadc_refine* r, int n, const float* d_queries, const float* radius, const adc::ScanFilter& filter, const RangePlan& plan,
               std::vector<uint64_t>& lims) {
    RangeMeta m;
    m.n = n;
    m.h.assign(5 * (size_t)n, 0);
    for (int q = 0; q < n; ++q) {
        m.limit()[q] = range_limit_word(radius[q]);
        m.cap()[q] = plan.region_rows;
    }
    const RangeStore s = range_store(r, false);
    uint64_t entries = 0;
    for (int attempt = 0;; ++attempt) {
        if (!range_regions(m.cap(), n, kRangeMaxEntries, m.base(), &entries))   // (before anything is allocated for the run)
            return fail(QADC_E_CAPACITY, "the regions of a range pass exceed QADC_REFINE_RANGE_MAX_ENTRIES words (a smaller radius, or fewer queries per "
                                         "pass: qadc_refine_set_range_plan)");
        HIPCHECK(r->d_rmeta.ensure(5 * (size_t)n));
        HIPCHECK(r->d_rbuf.ensure((size_t)entries));
        std::fill(m.cnt(), m.cnt() + n, 0);
        HIPCHECK(hipMemcpyAsync(r->d_rmeta.p, m.h.data(), 4 * (size_t)n * 8, hipMemcpyHostToDevice, r->stream));   // limit, base, cap, zeroed counters
        const RangeRegions g = range_regions_of(r, n);
        for (uint64_t l = 0; l < plan.launches; ++l) HIPCHECK(launch_range_dist(s, filter, d_queries, g, plan, l, r->stream));
        HIPCHECK(hipMemcpyAsync(m.cnt(), g.cnt, (size_t)n * 8, hipMemcpyDeviceToHost, r->stream));
        HIPCHECK(hipStreamSynchronize(r->stream));
        if (!range_rerun(m.cap(), m.cnt(), n)) break;
        if (attempt) return fail(QADC_E_STATE, "a range pass kept more rows in its second run than its first run counted");
        ++r->range_reruns;
    }
    return range_finish_pass(r, m, entries, lims);
}

int check_range(const qadc_refine* r, int nq, const void* queries, const float* radius, const uint64_t* lims, const qadc_adc_filter* filter,
                adc::ScanFilter* scan) {
    if (const char* why = range_refusal(r != nullptr, nq, queries != nullptr, radius != nullptr, lims != nullptr)) return fail(QADC_E_ARG, why);
    int fdev = -1;
    adc_filter_view(filter, scan, &fdev);
    if (filter && fdev != r->device)
        return fail(QADC_E_ARG, "the filter is on device " + std::to_string(fdev) + " and the store on device " + std::to_string(r->device));
    return QADC_OK;
}

// Closes a range call: the result is held and its row offsets go to the caller.
int publish_range(qadc_refine* r, std::vector<uint64_t>& lims, uint64_t* out) {
    if (out) std::copy(lims.begin(), lims.end(), out);
    r->range_lims.swap(lims);
    return QADC_OK;
}

// The passes of the exhaustive form on queries in device memory
int range_call(qadc_refine* r, int nq, const float* d_queries, const float* radius, const adc::ScanFilter& filter, uint64_t* lims_out) {
    std::vector<uint64_t> lims(1, 0);
    const uint64_t walk = r->keyed ? (r->live ? r->rows : 0) : r->rows;   // (a keyed store walks the rows allocated so far)
    if (nq == 0 || walk == 0) {
        lims.resize((size_t)nq + 1, 0);
        return publish_range(r, lims, lims_out);
    }
    RangePlan plan;
    if (!range_plan(nq, walk, r->dim, r->range_region_rows, r->range_chunk_rows, r->range_pass_nq, &plan))
        return fail(QADC_E_ARG, "no launch geometry for this call");
    for (int q0 = 0; q0 < nq; q0 += plan.pass_nq) {
        const int n = std::min(plan.pass_nq, nq - q0);
        if (int rc = range_pass(r, n, d_queries + (size_t)q0 * r->dim, radius + q0, filter, plan, lims)) return rc;
    }
    return publish_range(r, lims, lims_out);
}

// The passes of the candidate form on queries and keys in device memory; in_lims is host memory
int rerank_range_call(qadc_refine* r, int nq, const float* d_queries, const uint64_t* in_lims, const uint32_t* d_keys, const float* radius,
                      uint64_t* lims_out, uint64_t* missing_out) {
    std::vector<uint64_t> lims(1, 0);
    if (nq == 0) return publish_range(r, lims, lims_out);
    std::vector<RangeCandPass> passes;
    if (!range_cand_passes(in_lims, nq, r->range_pass_nq, kRangeMaxEntries, &passes))
        return fail(QADC_E_CAPACITY, "one query has more than QADC_REFINE_RANGE_MAX_ENTRIES candidates");
    HIPCHECK(r->d_missing.ensure(1));
    HIPCHECK(hipMemsetAsync(r->d_missing.p, 0, sizeof(unsigned long long), r->stream));
    const RangeStore s = range_store(r, true);
    std::vector<RangeChunk> chunks;
    for (const RangeCandPass& ps : passes) {
        const int n = ps.q1 - ps.q0;
        const uint64_t first = in_lims[ps.q0], entries = in_lims[ps.q1] - first;
        RangeMeta m;
        m.n = n;
        m.h.assign(5 * (size_t)n, 0);
        for (int q = 0; q < n; ++q) {
            m.limit()[q] = range_limit_word(radius[ps.q0 + q]);
            m.base()[q] = in_lims[ps.q0 + q] - first;
            m.cap()[q] = m.cnt()[q] = in_lims[ps.q0 + q + 1] - in_lims[ps.q0 + q];
        }
        range_cand_chunks(in_lims, ps.q0, ps.q1, range_cands_per_wg(in_lims, ps.q0, ps.q1), &chunks);
        HIPCHECK(r->d_rmeta.ensure(5 * (size_t)n));
        HIPCHECK(r->d_rbuf.ensure((size_t)entries));
        HIPCHECK(r->d_rchunks.ensure(chunks.size()));
        HIPCHECK(hipMemcpyAsync(r->d_rmeta.p, m.h.data(), 4 * (size_t)n * 8, hipMemcpyHostToDevice, r->stream));
        if (!chunks.empty())
            HIPCHECK(hipMemcpyAsync(r->d_rchunks.p, chunks.data(), chunks.size() * sizeof(RangeChunk), hipMemcpyHostToDevice, r->stream));
        const RangeRegions g = range_regions_of(r, n);
        HIPCHECK(launch_range_cand(s, d_queries + (size_t)ps.q0 * r->dim, d_keys + first, r->d_rchunks.p, (uint32_t)chunks.size(), g, r->d_missing.p,
                                   r->stream));
        HIPCHECK(hipStreamSynchronize(r->stream));   // (the chunk table and the meta block leave with this iteration)
        if (int rc = range_finish_pass(r, m, entries, lims)) return rc;
    }
    unsigned long long missing = 0;
    HIPCHECK(hipMemcpyAsync(&missing, r->d_missing.p, sizeof(missing), hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipStreamSynchronize(r->stream));
    if (missing_out) *missing_out = missing;
    return publish_range(r, lims, lims_out);
}

// The held result into the caller's buffers: host memory by copies, device memory by a kernel (launch_adc_copy_words).
int range_collect(qadc_refine* r, uint64_t capacity, uint32_t* keys, float* dist, bool d_side) {
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (r->range_lims.empty()) return fail(QADC_E_STATE, "no range result is held: call qadc_refine_range* or qadc_refine_rerank_range* first");
    const uint64_t n = r->range_lims.back();
    if (capacity < n)
        return fail(QADC_E_CAPACITY, "the range result has " + std::to_string(n) + " rows (lims[nq]); the buffers hold " + std::to_string(capacity));
    if (n == 0) return QADC_OK;
    if (!keys || !dist) return fail(QADC_E_ARG, "keys and dist are required");
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    if (d_side) {
        HIPCHECK(adc::launch_adc_copy_words(r->d_rkeys.p, keys, (size_t)n, r->stream));
        HIPCHECK(adc::launch_adc_copy_words(r->d_rdist.p, dist, (size_t)n, r->stream));
    } else {
        HIPCHECK(hipMemcpyAsync(keys, r->d_rkeys.p, (size_t)n * 4, hipMemcpyDeviceToHost, r->stream));
        HIPCHECK(hipMemcpyAsync(dist, r->d_rdist.p, (size_t)n * 4, hipMemcpyDeviceToHost, r->stream));
    }
    HIPCHECK(hipStreamSynchronize(r->stream));
    return QADC_OK;
}

// Range search has no inner-product form: refused before the device or the held result is touched
int range_metric_refusal(const qadc_refine* r) {
    if (r && r->metric != QADC_REFINE_L2)
        return fail(QADC_E_STATE, "range search is L2 only: the store's metric is QADC_REFINE_IP (qadc_refine_set_metric)");
    return QADC_OK;
}

}  // namespace

extern "C" {

int qadc_refine_set_metric(qadc_refine* r, int metric) {
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (metric != QADC_REFINE_L2 && metric != QADC_REFINE_IP) return fail(QADC_E_ARG, "metric is QADC_REFINE_L2 or QADC_REFINE_IP");
    r->metric = metric;
    return QADC_OK;
}

int qadc_refine_metric(const qadc_refine* r, int* metric_out) {
    if (!r || !metric_out) return fail(QADC_E_ARG, "store and metric_out must not be null");
    *metric_out = r->metric;
    return QADC_OK;
}

int qadc_refine_range(qadc_refine* r, int nq, const float* queries, const float* radius, const qadc_adc_filter* filter, uint64_t* lims) {
    if (int rc = range_metric_refusal(r)) return rc;
    if (r) r->range_lims.clear();   // (the held result is dropped, also when this call fails)
    adc::ScanFilter scan;
    if (int rc = check_range(r, nq, queries, radius, lims, filter, &scan)) return rc;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    if (nq) {
        HIPCHECK(r->d_queries.ensure((size_t)nq * r->dim));
        HIPCHECK(hipMemcpyAsync(r->d_queries.p, queries, (size_t)nq * r->dim * 4, hipMemcpyHostToDevice, r->stream));
    }
    return range_call(r, nq, r->d_queries.p, radius, scan, lims);
}

int qadc_refine_range_device(qadc_refine* r, int nq, const float* d_queries, const float* radius, const qadc_adc_filter* filter, uint64_t* lims) {
    if (int rc = range_metric_refusal(r)) return rc;
    if (r) r->range_lims.clear();
    if (int rc = check_aligned(d_queries, 4, "d_queries")) return rc;
    adc::ScanFilter scan;
    if (int rc = check_range(r, nq, d_queries, radius, lims, filter, &scan)) return rc;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    return range_call(r, nq, d_queries, radius, scan, lims);
}

int qadc_refine_rerank_range(qadc_refine* r, int nq, const float* queries, const uint64_t* in_lims, const uint32_t* keys, const float* radius,
                             uint64_t* lims, uint64_t* missing_out) {
    if (int rc = range_metric_refusal(r)) return rc;
    if (r) r->range_lims.clear();
    if (missing_out) *missing_out = 0;
    if (const char* why = rerank_range_refusal(r != nullptr, nq, queries != nullptr, in_lims, keys != nullptr, radius != nullptr, lims != nullptr))
        return fail(QADC_E_ARG, why);
    const std::vector<uint64_t> in(in_lims ? in_lims : lims, (in_lims ? in_lims : lims) + (nq ? nq + 1 : 0));   // (lims may be in_lims itself)
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    if (nq) {
        HIPCHECK(r->d_queries.ensure((size_t)nq * r->dim));
        HIPCHECK(hipMemcpyAsync(r->d_queries.p, queries, (size_t)nq * r->dim * 4, hipMemcpyHostToDevice, r->stream));
        HIPCHECK(r->d_keys.ensure((size_t)in[nq]));
        if (in[nq]) HIPCHECK(hipMemcpyAsync(r->d_keys.p, keys, (size_t)in[nq] * 4, hipMemcpyHostToDevice, r->stream));
    }
    return rerank_range_call(r, nq, r->d_queries.p, in.data(), r->d_keys.p, radius, lims, missing_out);
}

int qadc_refine_rerank_range_device(qadc_refine* r, int nq, const float* d_queries, const uint64_t* in_lims, const uint32_t* d_keys,
                                    const float* radius, uint64_t* lims, uint64_t* missing_out) {
    if (int rc = range_metric_refusal(r)) return rc;
    if (r) r->range_lims.clear();
    if (missing_out) *missing_out = 0;
    if (int rc = check_aligned(d_queries, 4, "d_queries")) return rc;
    if (int rc = check_aligned(d_keys, 4, "d_keys")) return rc;
    if (const char* why = rerank_range_refusal(r != nullptr, nq, d_queries != nullptr, in_lims, d_keys != nullptr, radius != nullptr, lims != nullptr))
        return fail(QADC_E_ARG, why);
    const std::vector<uint64_t> in(in_lims ? in_lims : lims, (in_lims ? in_lims : lims) + (nq ? nq + 1 : 0));
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    return rerank_range_call(r, nq, d_queries, in.data(), d_keys, radius, lims, missing_out);
}

int qadc_refine_range_collect(qadc_refine* r, uint64_t capacity, uint32_t* keys, float* dist) { return range_collect(r, capacity, keys, dist, false); }

int qadc_refine_range_collect_device(qadc_refine* r, uint64_t capacity, uint32_t* d_keys, float* d_dist) {
    if (int rc = check_aligned(d_keys, 4, "d_keys")) return rc;
    if (int rc = check_aligned(d_dist, 4, "d_dist")) return rc;
    return range_collect(r, capacity, d_keys, d_dist, true);
}

int qadc_refine_set_range_plan(qadc_refine* r, uint64_t region_rows, uint64_t chunk_rows, int pass_nq) {
    if (const char* why = range_plan_refusal(r != nullptr, chunk_rows, pass_nq)) return fail(QADC_E_ARG, why);
    r->range_region_rows = region_rows;
    r->range_chunk_rows = chunk_rows;
    r->range_pass_nq = pass_nq;
    return QADC_OK;
}

uint64_t qadc_refine_range_reruns(const qadc_refine* r) { return r ? r->range_reruns : 0; }

int qadc_refine_create_sq8(qadc_refine** out, int dim, const float* vmin, const float* step, int keyed, int device_id) {
    if (out) *out = nullptr;
    if (!vmin || !step) return fail(QADC_E_ARG, "vmin and step must not be null");
    return create_store(out, dim, QADC_REFINE_SQ8, device_id, keyed != 0, vmin, step);
}

int qadc_refine_sq_range_device(const float* d_vectors, uint64_t n, int dim, int device_id, float* vmin_out, float* step_out) {
    if (int rc = check_aligned(d_vectors, 4, "d_vectors")) return rc;
    if (int rc = check_sq_range(d_vectors, n, dim, vmin_out, step_out)) return rc;
    DeviceGuard guard;
    if (int rc = qadc_device_prepare(device_id)) return rc;
    HIPCHECK(hipSetDevice(device_id));
    return sq_range(d_vectors, n, dim, true, vmin_out, step_out);
}

int qadc_refine_sq_range_host(const float* vectors, uint64_t n, int dim, int device_id, float* vmin_out, float* step_out) {
    if (int rc = check_sq_range(vectors, n, dim, vmin_out, step_out)) return rc;
    DeviceGuard guard;
    if (int rc = qadc_device_prepare(device_id)) return rc;
    HIPCHECK(hipSetDevice(device_id));
    return sq_range(vectors, n, dim, false, vmin_out, step_out);
}

int qadc_refine_sq_info(const qadc_refine* r, float* vmin_out, float* step_out, uint64_t* clamped_out) {
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (r->dtype != QADC_REFINE_SQ8) return fail(QADC_E_STATE, "qadc_refine_sq_info: the store's rows are not SQ8 (qadc_refine_create_sq8)");
    if (vmin_out) std::copy(r->sq_vmin.begin(), r->sq_vmin.end(), vmin_out);
    if (step_out) std::copy(r->sq_step.begin(), r->sq_step.end(), step_out);
    if (clamped_out) {
        DeviceGuard guard;
        HIPCHECK(hipSetDevice(r->device));
        unsigned long long c = 0;
        HIPCHECK(hipMemcpyAsync(&c, r->d_clamped, sizeof(c), hipMemcpyDeviceToHost, r->stream));
        HIPCHECK(hipStreamSynchronize(r->stream));
        *clamped_out = c;
    }
    return QADC_OK;
}

int qadc_refine_get(qadc_refine* r, const uint32_t* keys, uint64_t count, float* out_vectors, uint8_t* found_out) {
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (count == 0) return QADC_OK;
    if (!keys || !out_vectors) return fail(QADC_E_ARG, "keys and out_vectors must not be null");
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    HIPCHECK(r->d_keys.ensure((size_t)count));
    HIPCHECK(hipMemcpyAsync(r->d_keys.p, keys, (size_t)count * 4, hipMemcpyHostToDevice, r->stream));
    return get_rows(r, r->d_keys.p, count, out_vectors, found_out, false);
}

int qadc_refine_get_device(qadc_refine* r, const uint32_t* d_keys, uint64_t count, float* d_out_vectors, uint8_t* d_found_out) {
    if (int rc = check_aligned(d_keys, 4, "d_keys")) return rc;
    if (int rc = check_aligned(d_out_vectors, 4, "d_out_vectors")) return rc;
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (count == 0) return QADC_OK;
    if (!d_keys || !d_out_vectors) return fail(QADC_E_ARG, "d_keys and d_out_vectors must not be null");
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    return get_rows(r, d_keys, count, d_out_vectors, d_found_out, true);
}

int qadc_refine_create(qadc_refine** out, int dim, int dtype, int device_id) { return create_store(out, dim, dtype, device_id, false); }

int qadc_refine_create_keyed(qadc_refine** out, int dim, int dtype, int device_id) { return create_store(out, dim, dtype, device_id, true); }

int qadc_refine_put(qadc_refine* r, const float* vectors, const uint32_t* labels, uint64_t count) {
    return put_rows(r, vectors, labels, count, false, "qadc_refine_put");
}

int qadc_refine_put_device(qadc_refine* r, const float* d_vectors, const uint32_t* d_labels, uint64_t count) {
    if (int rc = check_aligned(d_vectors, 4, "d_vectors")) return rc;
    if (int rc = check_aligned(d_labels, 4, "d_labels")) return rc;
    return put_rows(r, d_vectors, d_labels, count, true, "qadc_refine_put_device");
}

int qadc_refine_remove(qadc_refine* r, const uint32_t* labels, uint64_t count, uint64_t* removed_out) {
    return remove_rows(r, labels, count, removed_out, false, "qadc_refine_remove");
}

int qadc_refine_remove_device(qadc_refine* r, const uint32_t* d_labels, uint64_t count, uint64_t* removed_out) {
    if (int rc = check_aligned(d_labels, 4, "d_labels")) return rc;
    return remove_rows(r, d_labels, count, removed_out, true, "qadc_refine_remove_device");
}

int qadc_refine_keyed_info(const qadc_refine* r, uint64_t* live, uint64_t* rows_allocated, uint64_t* rows_free, uint64_t* table_slots,
                           uint64_t* table_used, uint64_t* bytes) {
    if (int rc = keyed_call(const_cast<qadc_refine*>(r), "qadc_refine_keyed_info", true)) return rc;
    if (live) *live = r->live;
    if (rows_allocated) *rows_allocated = r->rows;
    if (rows_free) *rows_free = r->free_rows;
    if (table_slots) *table_slots = 1ull << r->table.bits;
    if (table_used) *table_used = r->used;
    if (bytes) *bytes = r->cap * ((uint64_t)r->row_bytes() + 8) + table_bytes(r->table.bits);
    return QADC_OK;
}

uint32_t qadc_refine_keyed_slot(uint32_t key, int table_bits) { return qadc::refine::keyed_slot(key, table_bits); }

int qadc_refine_destroy(qadc_refine* r) {
    if (!r) return QADC_OK;
    DeviceGuard guard;
    (void)hipSetDevice(r->device);
    if (r->stream) {
        (void)hipStreamSynchronize(r->stream);
        (void)hipStreamDestroy(r->stream);
    }
    if (r->data) (void)hipFree(r->data);
    if (r->row_key) (void)hipFree(r->row_key);
    if (r->free_list) (void)hipFree(r->free_list);
    if (r->d_sq) (void)hipFree(r->d_sq);
    if (r->d_clamped) (void)hipFree(r->d_clamped);
    r->d_get_out.release(); r->d_get_found.release();
    free_table(r->table);
    r->d_cnt.release(); r->d_labels.release(); r->d_slot_of.release(); r->d_dst.release();
    r->d_stage.release(); r->d_words.release(); r->d_missing.release(); r->d_queries.release(); r->d_values.release();
    r->d_out_dist.release(); r->d_keys.release(); r->d_out_keys.release(); r->d_counts.release(); r->d_out_sizes.release();
    r->d_knn_buf.release(); r->d_knn_bound.release(); r->d_knn_cnt.release();
    r->d_probe_parts.release(); r->d_probe_items.release(); r->d_probe_slots.release(); r->d_probe_assign.release();
    r->d_rkeys.release(); r->d_rdist.release(); r->d_rbuf.release(); r->d_rtmp.release(); r->d_rmeta.release(); r->d_rkept.release();
    r->d_rchunks.release();
    delete r;
    return QADC_OK;
}

int qadc_refine_add(qadc_refine* r, const float* vectors, uint64_t count, uint32_t first_key) {
    return add_rows(r, vectors, count, first_key, false);
}

int qadc_refine_add_device(qadc_refine* r, const float* d_vectors, uint64_t count, uint32_t first_key) {
    if (int rc = check_aligned(d_vectors, 4, "d_vectors")) return rc;
    return add_rows(r, d_vectors, count, first_key, true);
}

int qadc_refine_reserve(qadc_refine* r, uint64_t rows) {
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (rows > (1ull << 32)) return fail(QADC_E_ARG, "a store holds at most 2^32 rows");
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    if (r->keyed) {   // room for `rows` live keys in the row arrays and in the table
        const KeyedPutPlan plan = plan_reserve(r->table.bits, rows);
        if (plan.refused) return fail(QADC_E_ARG, "a keyed store holds at most 2^30 keys");
        if (int rc = ensure_keyed_rows(r, rows, true)) return rc;
        return plan.rebuild ? rebuild_table(r, plan.bits) : QADC_OK;
    }
    return ensure_rows(r, rows, true);
}

int qadc_refine_info(const qadc_refine* r, int* dim, int* dtype, uint32_t* lo, uint64_t* rows, uint64_t* bytes) {
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (dim) *dim = r->dim;
    if (dtype) *dtype = r->dtype;
    if (lo) *lo = r->keyed ? 0 : r->lo;
    if (rows) *rows = r->keyed ? r->live : r->rows;
    if (bytes) *bytes = r->keyed ? r->cap * ((uint64_t)r->row_bytes() + 8) + table_bytes(r->table.bits) : r->cap * (uint64_t)r->row_bytes();
    return QADC_OK;
}

uint64_t qadc_refine_relocations(const qadc_refine* r) { return r ? r->relocations : 0; }

int qadc_refine_rerank(qadc_refine* r, int nq, const float* queries, int r_in, const uint32_t* keys, const int32_t* counts,
                       const float* values, int R, uint32_t* out_keys, float* out_dist, int32_t* out_sizes, uint64_t* missing_out) {
    if (int rc = check_rerank(r, nq, queries, r_in, keys, R, out_keys, out_dist, out_sizes)) return rc;
    if (counts)
        for (int q = 0; q < nq; ++q)
            if (counts[q] < 0 || counts[q] > r_in)
                return fail(QADC_E_ARG, "counts[" + std::to_string(q) + "] = " + std::to_string(counts[q]) + " is outside [0, r_in]");
    if (missing_out) *missing_out = 0;
    if (nq == 0) return QADC_OK;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    const size_t nin = (size_t)nq * r_in, nout = (size_t)nq * R;
    HIPCHECK(r->d_queries.ensure((size_t)nq * r->dim));
    HIPCHECK(r->d_keys.ensure(nin));
    HIPCHECK(r->d_out_keys.ensure(nout));
    HIPCHECK(r->d_out_dist.ensure(nout));
    HIPCHECK(r->d_out_sizes.ensure(nq));
    HIPCHECK(hipMemcpyAsync(r->d_queries.p, queries, (size_t)nq * r->dim * 4, hipMemcpyHostToDevice, r->stream));
    HIPCHECK(hipMemcpyAsync(r->d_keys.p, keys, nin * 4, hipMemcpyHostToDevice, r->stream));
    if (counts) {
        HIPCHECK(r->d_counts.ensure(nq));
        HIPCHECK(hipMemcpyAsync(r->d_counts.p, counts, (size_t)nq * 4, hipMemcpyHostToDevice, r->stream));
    }
    if (values) {
        HIPCHECK(r->d_values.ensure(nin));
        HIPCHECK(hipMemcpyAsync(r->d_values.p, values, nin * 4, hipMemcpyHostToDevice, r->stream));
    }
    uint64_t missing = 0;
    if (int rc = rerank_passes(r, nq, r->d_queries.p, r_in, r->d_keys.p, counts ? r->d_counts.p : nullptr, values ? r->d_values.p : nullptr, R,
                               r->d_out_keys.p, r->d_out_dist.p, r->d_out_sizes.p, &missing))
        return rc;
    HIPCHECK(hipMemcpyAsync(out_keys, r->d_out_keys.p, nout * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipMemcpyAsync(out_dist, r->d_out_dist.p, nout * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipMemcpyAsync(out_sizes, r->d_out_sizes.p, (size_t)nq * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipStreamSynchronize(r->stream));
    if (missing_out) *missing_out = missing;
    return QADC_OK;
}

int qadc_refine_rerank_device(qadc_refine* r, int nq, const float* d_queries, int r_in, const uint32_t* d_keys, const int32_t* d_counts,
                              const float* d_values, int R, uint32_t* d_out_keys, float* d_out_dist, int32_t* d_out_sizes,
                              uint64_t* missing_out) {
    const void* const d_ptrs[] = {d_queries, d_keys, d_counts, d_values, d_out_keys, d_out_dist, d_out_sizes};
    const char* const d_names[] = {"d_queries", "d_keys", "d_counts", "d_values", "d_out_keys", "d_out_dist", "d_out_sizes"};
    for (int i = 0; i < 7; ++i)
        if (int rc = check_aligned(d_ptrs[i], 4, d_names[i])) return rc;
    if (int rc = check_rerank(r, nq, d_queries, r_in, d_keys, R, d_out_keys, d_out_dist, d_out_sizes)) return rc;
    if (missing_out) *missing_out = 0;
    if (nq == 0) return QADC_OK;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    return rerank_passes(r, nq, d_queries, r_in, d_keys, d_counts, d_values, R, d_out_keys, d_out_dist, d_out_sizes, missing_out);
}

int qadc_refine_set_knn_plan(qadc_refine* r, uint64_t chunk_rows, int pass_nq) {
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (chunk_rows > kKnnDefaultChunk)
        return fail(QADC_E_ARG, "chunk_rows is at most " + std::to_string(kKnnDefaultChunk) + " (a select sorts R + chunk_rows <= " +
                                    std::to_string(kKnnMaxSort) + " words)");
    if (pass_nq < 0) return fail(QADC_E_ARG, "pass_nq is negative");
    r->knn_chunk_rows = chunk_rows;
    r->knn_pass_nq = pass_nq;
    return QADC_OK;
}

int qadc_refine_knn(qadc_refine* r, int nq, const float* queries, int R, const qadc_adc_filter* filter, uint32_t* out_keys, float* out_dist,
                    int32_t* out_sizes) {
    adc::ScanFilter scan;
    if (int rc = check_knn(r, nq, queries, R, filter, &scan, out_keys, out_dist, out_sizes)) return rc;
    if (nq == 0) return QADC_OK;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    const size_t nout = (size_t)nq * R;
    HIPCHECK(r->d_queries.ensure((size_t)nq * r->dim));
    HIPCHECK(r->d_out_keys.ensure(nout));
    HIPCHECK(r->d_out_dist.ensure(nout));
    HIPCHECK(r->d_out_sizes.ensure(nq));
    HIPCHECK(hipMemcpyAsync(r->d_queries.p, queries, (size_t)nq * r->dim * 4, hipMemcpyHostToDevice, r->stream));
    if (int rc = knn_passes(r, nq, r->d_queries.p, R, scan, r->d_out_keys.p, r->d_out_dist.p, r->d_out_sizes.p)) return rc;
    HIPCHECK(hipMemcpyAsync(out_keys, r->d_out_keys.p, nout * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipMemcpyAsync(out_dist, r->d_out_dist.p, nout * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipMemcpyAsync(out_sizes, r->d_out_sizes.p, (size_t)nq * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipStreamSynchronize(r->stream));
    return QADC_OK;
}

int qadc_refine_knn_device(qadc_refine* r, int nq, const float* d_queries, int R, const qadc_adc_filter* filter, uint32_t* d_out_keys,
                           float* d_out_dist, int32_t* d_out_sizes) {
    const void* const d_ptrs[] = {d_queries, d_out_keys, d_out_dist, d_out_sizes};
    const char* const d_names[] = {"d_queries", "d_out_keys", "d_out_dist", "d_out_sizes"};
    for (int i = 0; i < 4; ++i)
        if (int rc = check_aligned(d_ptrs[i], 4, d_names[i])) return rc;
    adc::ScanFilter scan;
    if (int rc = check_knn(r, nq, d_queries, R, filter, &scan, d_out_keys, d_out_dist, d_out_sizes)) return rc;
    if (nq == 0) return QADC_OK;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    return knn_passes(r, nq, d_queries, R, scan, d_out_keys, d_out_dist, d_out_sizes);
}

int qadc_refine_knn_probed(qadc_refine* r, const qadc_adc_index* idx, int nq, const float* queries, int ma, const int32_t* assign, int R,
                           const qadc_adc_filter* filter, uint32_t* out_keys, float* out_dist, int32_t* out_sizes, uint64_t* missing_out) {
    adc::ScanFilter scan;
    ProbeIndex pi;
    if (int rc = check_probed(r, idx, nq, queries, ma, assign, R, filter, &scan, out_keys, out_dist, out_sizes, &pi)) return rc;
    for (size_t i = 0; i < (size_t)nq * ma; ++i)
        if (assign[i] < 0 || (size_t)assign[i] >= pi.parts.size())
            return fail(QADC_E_ARG, "assign[" + std::to_string(i) + "] = " + std::to_string(assign[i]) + " is not a partition (" +
                                        std::to_string(pi.parts.size()) + " partitions)");
    if (missing_out) *missing_out = 0;
    if (nq == 0) return QADC_OK;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    const size_t nout = (size_t)nq * R;
    HIPCHECK(r->d_queries.ensure((size_t)nq * r->dim));
    HIPCHECK(r->d_out_keys.ensure(nout));
    HIPCHECK(r->d_out_dist.ensure(nout));
    HIPCHECK(r->d_out_sizes.ensure(nq));
    HIPCHECK(hipMemcpyAsync(r->d_queries.p, queries, (size_t)nq * r->dim * 4, hipMemcpyHostToDevice, r->stream));
    uint64_t missing = 0;
    if (int rc = probed_passes(r, pi, nq, r->d_queries.p, ma, assign, R, scan, r->d_out_keys.p, r->d_out_dist.p, r->d_out_sizes.p, &missing)) return rc;
    HIPCHECK(hipMemcpyAsync(out_keys, r->d_out_keys.p, nout * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipMemcpyAsync(out_dist, r->d_out_dist.p, nout * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipMemcpyAsync(out_sizes, r->d_out_sizes.p, (size_t)nq * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipStreamSynchronize(r->stream));
    if (missing_out) *missing_out = missing;
    return QADC_OK;
}

int qadc_refine_knn_probed_device(qadc_refine* r, const qadc_adc_index* idx, int nq, const float* d_queries, int ma, const int32_t* d_assign, int R,
                                  const qadc_adc_filter* filter, uint32_t* d_out_keys, float* d_out_dist, int32_t* d_out_sizes,
                                  uint64_t* missing_out) {
    const void* const d_ptrs[] = {d_queries, d_assign, d_out_keys, d_out_dist, d_out_sizes};
    const char* const d_names[] = {"d_queries", "d_assign", "d_out_keys", "d_out_dist", "d_out_sizes"};
    for (int i = 0; i < 5; ++i)
        if (int rc = check_aligned(d_ptrs[i], 4, d_names[i])) return rc;
    adc::ScanFilter scan;
    ProbeIndex pi;
    if (int rc = check_probed(r, idx, nq, d_queries, ma, d_assign, R, filter, &scan, d_out_keys, d_out_dist, d_out_sizes, &pi)) return rc;
    if (missing_out) *missing_out = 0;
    if (nq == 0) return QADC_OK;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    // the probe numbers cross the bus: the planner inverts them on the host (a kernel copies them out of the caller's memory first)
    const size_t n = (size_t)nq * ma;
    std::vector<int32_t> assign(n);
    HIPCHECK(r->d_probe_assign.ensure(n));
    HIPCHECK(adc::launch_adc_copy_words(d_assign, r->d_probe_assign.p, n, r->stream));
    HIPCHECK(hipMemcpyAsync(assign.data(), r->d_probe_assign.p, n * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipStreamSynchronize(r->stream));
    return probed_passes(r, pi, nq, d_queries, ma, assign.data(), R, scan, d_out_keys, d_out_dist, d_out_sizes, missing_out);
}

}  // extern "C"
