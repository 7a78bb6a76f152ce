// Host side of the float-ADC engine for whole-byte PQ codes (qadc_adc_* in include/qadc.h): the GPU scanner_simple
// (db_query.cpp:17-46) over scan_standard<uint8_t, NSQ> (query_common.hpp:92-118), NSQ 4, 8 or 16.
//
// A call scans the probed partitions of nq queries in bound levels: level 0 is the first
// max(R, 512) codes of every query's scan order, each following level 16 times as far; the runs of a level are filtered
// by the R-th smallest value the query emitted in the levels before it (FLT_MAX while fewer than R), which is the R-th
// smallest of a subset of the codes that precede every code of the level.  The kept candidates come back to the host,
// are put in scan order and pushed into kv_heap<unsigned, float>(R) after the R sentinels.  This engine shares nothing
// with the 4-bit index but the device's stream set (qadc_device_prepare) and has no qadc_set_option names.
#include "../../include/qadc.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../host/qadc_heap.hpp"
#include "../host/worker_pool.hpp"
#include "qadc_adc_kernels.h"
#include "qadc_host.h"

using qadc::host::fail;
using qadc::host::DevBuf;
using qadc::host::PinBuf;

namespace {

constexpr uint32_t kLevel0 = 512;      // codes of level 0 (at least R)
constexpr uint32_t kLevelGrowth = 16;  // each level spans 16 times the scan order before it
constexpr uint32_t kWgTarget = 2048;   // workgroups a level is cut into, roughly
constexpr uint32_t kRunMin = 2048, kRunMax = 65536;
constexpr uint64_t kSpeculativeEntries = 1 << 16;   // regions up to this many entries in all come back with the counts
constexpr uint64_t kMaxEntries = QADC_ADC_MAX_ENTRIES;   // candidate entries of one batch (12 B of device memory each)

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Every entry point works on the index's device and gives the calling thread its current device back.
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace

struct qadc_adc_index {
    int nsq = 0, device = 0;
    hipStream_t stream = nullptr;
    int labeled = -1;                               // unknown until the first non-empty add
    std::vector<uint32_t> sizes;
    std::vector<uint64_t> off, lab_off;             // byte offset of each partition's codes / first label
    uint64_t code_bytes = 0, label_count = 0;
    DevBuf<uint8_t> codes;                          // code_bytes + 16 bytes of tail padding
    DevBuf<uint32_t> labels;
    DevBuf<uint64_t> d_off, d_lab_off;
    // per call
    DevBuf<uint8_t> d_in;                           // [bound | count | assign | items | tables]
    DevBuf<float> d_vals;
    DevBuf<uint32_t> d_keys, d_sidx, d_packed;
    PinBuf<uint8_t> h_in;
    PinBuf<uint32_t> h_count, h_packed;
    uint64_t reruns = 0;                            // batches re-run because a candidate region overflowed
    std::vector<uint64_t> stream_off;               // [nq + 1] the ordered stream of the last call
    std::vector<uint32_t> stream_keys;
    std::vector<float> stream_vals;
    qadc::WorkerPool pool;
};

namespace {

using qadc::adc::Item;

int grow_device(DevBuf<uint8_t>& buf, uint64_t used, uint64_t need, hipStream_t s) {
    if (need <= buf.cap) return QADC_OK;
    DevBuf<uint8_t> nb;
    HIPCHECK(nb.ensure(std::max<uint64_t>(need, buf.cap + buf.cap / 2)));
    if (used) HIPCHECK(hipMemcpyAsync(nb.p, buf.p, used, hipMemcpyDeviceToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));
    buf.release();
    buf = nb;
    return QADC_OK;
}

int grow_labels(DevBuf<uint32_t>& buf, uint64_t used, uint64_t need, hipStream_t s) {
    if (need <= buf.cap) return QADC_OK;
    DevBuf<uint32_t> nb;
    HIPCHECK(nb.ensure(std::max<uint64_t>(need, buf.cap + buf.cap / 2)));
    if (used) HIPCHECK(hipMemcpyAsync(nb.p, buf.p, used * 4, hipMemcpyDeviceToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));
    buf.release();
    buf = nb;
    return QADC_OK;
}

int check_query_args(const qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R, int sum_mode) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (nq < 1 || ma < 1 || ma >= 16384) return fail(QADC_E_ARG, "need nq >= 1 and 1 <= ma < 16384");
    if (R < 1 || R > QADC_ADC_MAX_R) return fail(QADC_E_ARG, "R must be in [1, " + std::to_string(QADC_ADC_MAX_R) + "]");
    if (sum_mode != 0 && sum_mode != 1) return fail(QADC_E_ARG, "sum_mode is 0 (source order) or 1 (as compiled)");
    if (!assign || !tables) return fail(QADC_E_ARG, "assign and tables are required");
    const int parts = (int)idx->sizes.size();
    for (size_t i = 0; i < (size_t)nq * ma; ++i)
        if (assign[i] < 0 || assign[i] >= parts)
            return fail(QADC_E_ARG, "assign[" + std::to_string(i) + "] = " + std::to_string(assign[i]) + " is not a partition (" +
                                        std::to_string(parts) + " partitions)");
    return QADC_OK;
}

// Scans the batch on the device and leaves the ordered candidate stream of every query in idx->stream_*.
int scan_batch(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R, int sum_mode) {
    if (int rc = check_query_args(idx, nq, ma, assign, tables, R, sum_mode)) return rc;
    HIPCHECK(hipSetDevice(idx->device));
    // scan-order length of every query, and the levels
    std::vector<uint64_t> total(nq, 0);
    uint64_t max_total = 0;
    for (int q = 0; q < nq; ++q) {
        for (int a = 0; a < ma; ++a) total[q] += idx->sizes[assign[(size_t)q * ma + a]];
        if (total[q] > 0xffffffffull)
            return fail(QADC_E_ARG, "query " + std::to_string(q) + " probes " + std::to_string(total[q]) +
                                        " codes: at most 2^32 - 1 per query");
        max_total = std::max(max_total, total[q]);
    }
    std::vector<uint64_t> edge{0, std::max<uint64_t>((uint64_t)R, kLevel0)};
    while (edge.back() < max_total) edge.push_back(edge.back() * kLevelGrowth);
    const int levels = (int)edge.size() - 1;
    // the runs of every level: per query, the level's stretch of the scan order cut at partition ends and into runs
    std::vector<Item> items;
    std::vector<uint32_t> level_first(levels + 1, 0);
    for (int l = 0; l < levels; ++l) {
        level_first[l] = (uint32_t)items.size();
        uint64_t span = 0;
        for (int q = 0; q < nq; ++q)
            if (total[q] > edge[l]) span += std::min(total[q], edge[l + 1]) - edge[l];
        const uint64_t run = std::min<uint64_t>(kRunMax, std::max<uint64_t>(kRunMin, align_up((span + kWgTarget - 1) / kWgTarget, 1024)));
        for (int q = 0; q < nq; ++q) {
            const uint64_t lo = edge[l], hi = std::min(total[q], edge[l + 1]);
            uint64_t pbase = 0;
            for (int a = 0; a < ma && pbase < hi; ++a) {
                const uint64_t sz = idx->sizes[assign[(size_t)q * ma + a]];
                const uint64_t s0 = std::max(lo, pbase), s1 = std::min(hi, pbase + sz);
                for (uint64_t s = s0; s < s1; s += run) {
                    Item it{};
                    it.query = (uint32_t)q;
                    it.slot = (uint32_t)a;
                    it.start = (uint32_t)(s - pbase);
                    it.count = (uint32_t)std::min<uint64_t>(run, s1 - s);
                    it.sbase = (uint32_t)s;
                    items.push_back(it);
                }
                pbase += sz;
            }
        }
    }
    level_first[levels] = (uint32_t)items.size();

    // Per-query regions: the expected stream (level 0 whole, then ~15 R per level) with room to spare, at most the query's
    // code count.  They are sized per call, so nothing one call needed carries over to the next.
    const uint64_t expect = std::max<uint64_t>((uint64_t)R, kLevel0) + 32ull * R * (levels - 1) + 4096;
    std::vector<uint32_t> cap(nq);
    for (int q = 0; q < nq; ++q) cap[q] = (uint32_t)std::max<uint64_t>(1, std::min(total[q], expect));

    // one upload: bound (FLT_MAX) | count (0) | region sizes | region bases | assign | items | tables
    const size_t table_floats = (size_t)idx->nsq * 256;
    const size_t o_count = align_up((size_t)nq * 4, 256);
    const size_t o_cap = o_count + align_up((size_t)nq * 4, 256);
    const size_t o_base = o_cap + align_up((size_t)nq * 4, 256);
    const size_t o_assign = o_base + align_up((size_t)nq * 8, 256);
    const size_t o_items = o_assign + align_up((size_t)nq * ma * 4, 256);
    const size_t o_tables = o_items + align_up(items.size() * sizeof(Item), 256);
    const size_t in_bytes = o_tables + (size_t)nq * ma * table_floats * 4;
    HIPCHECK(idx->h_in.ensure(in_bytes));
    HIPCHECK(idx->d_in.ensure(in_bytes));
    uint8_t* h = idx->h_in.p;
    uint64_t* h_base = reinterpret_cast<uint64_t*>(h + o_base);
    // bound, counts and regions: written again before a re-run
    auto fill_state = [&]() -> uint64_t {
        std::fill(reinterpret_cast<float*>(h), reinterpret_cast<float*>(h) + nq, FLT_MAX);
        std::memset(h + o_count, 0, (size_t)nq * 4);
        std::memcpy(h + o_cap, cap.data(), (size_t)nq * 4);
        uint64_t entries = 0;
        for (int q = 0; q < nq; ++q) {
            h_base[q] = entries;
            entries += cap[q];
        }
        return entries;
    };
    uint64_t entries = fill_state();
    std::memcpy(h + o_assign, assign, (size_t)nq * ma * 4);
    if (!items.empty()) std::memcpy(h + o_items, items.data(), items.size() * sizeof(Item));
    std::memcpy(h + o_tables, tables, (size_t)nq * ma * table_floats * 4);
    uint8_t* d = idx->d_in.p;
    float* d_bound = reinterpret_cast<float*>(d);
    uint32_t* d_count = reinterpret_cast<uint32_t*>(d + o_count);
    const uint32_t* d_cap = reinterpret_cast<const uint32_t*>(d + o_cap);
    const uint64_t* d_base = reinterpret_cast<const uint64_t*>(d + o_base);
    const int32_t* d_assign = reinterpret_cast<const int32_t*>(d + o_assign);
    const Item* d_items = reinterpret_cast<const Item*>(d + o_items);
    const float* d_tables = reinterpret_cast<const float*>(d + o_tables);
    HIPCHECK(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, idx->stream));

    qadc::adc::Db db{idx->codes.p, idx->d_off.p, idx->labeled == 1 ? idx->labels.p : nullptr, idx->d_lab_off.p};
    std::vector<uint32_t> stored(nq);
    uint64_t n_stored = 0;
    bool speculative = false;
    for (;;) {
        if (entries > kMaxEntries)
            return fail(QADC_E_CAPACITY, "the candidate regions of this batch need " + std::to_string(entries) + " entries (at most " +
                                             std::to_string(kMaxEntries) + "): split the batch");
        HIPCHECK(idx->d_vals.ensure(entries));
        HIPCHECK(idx->d_keys.ensure(entries));
        HIPCHECK(idx->d_sidx.ensure(entries));
        const qadc::adc::Emit emit{d_count, idx->d_vals.p, idx->d_keys.p, idx->d_sidx.p, d_base, d_cap};
        for (int l = 0; l < levels; ++l) {
            HIPCHECK(qadc::adc::launch_adc_scan(idx->nsq, sum_mode, d_items, level_first[l], level_first[l + 1] - level_first[l], db,
                                                d_assign, ma, d_tables, d_bound, emit, idx->stream));
            if (l + 1 < levels) HIPCHECK(qadc::adc::launch_adc_select(nq, R, emit, d_bound, idx->stream));
        }
        HIPCHECK(idx->h_count.ensure(nq));
        // small batches: pack and fetch all regions speculatively, with the counts, in one round trip
        speculative = entries <= kSpeculativeEntries;
        if (speculative) {
            HIPCHECK(idx->d_packed.ensure(3 * entries));
            HIPCHECK(idx->h_packed.ensure(3 * entries));
            HIPCHECK(qadc::adc::launch_adc_pack(nq, emit, idx->d_packed.p, idx->stream));
        }
        HIPCHECK(hipMemcpyAsync(idx->h_count.p, d_count, (size_t)nq * 4, hipMemcpyDeviceToHost, idx->stream));
        if (speculative) HIPCHECK(hipMemcpyAsync(idx->h_packed.p, idx->d_packed.p, 3 * entries * 4, hipMemcpyDeviceToHost, idx->stream));
        HIPCHECK(hipStreamSynchronize(idx->stream));
        bool overflow = false;
        n_stored = 0;
        for (int q = 0; q < nq; ++q) {
            const uint32_t c = idx->h_count.p[q];
            stored[q] = std::min(c, cap[q]);
            n_stored += stored[q];
            if (c > cap[q]) {   // every emitted candidate was counted: this region takes them all in the re-run
                overflow = true;
                cap[q] = (uint32_t)std::min<uint64_t>(total[q], std::max<uint64_t>((uint64_t)c + c / 2, 2ull * cap[q]));
            }
        }
        if (!overflow) break;
        ++idx->reruns;
        entries = fill_state();   // re-run the whole batch with the grown regions
        HIPCHECK(hipMemcpyAsync(d, h, o_assign, hipMemcpyHostToDevice, idx->stream));
    }
    if (!speculative) {
        HIPCHECK(idx->d_packed.ensure(std::max<uint64_t>(3 * n_stored, 3)));
        HIPCHECK(idx->h_packed.ensure(std::max<uint64_t>(3 * n_stored, 3)));
        const qadc::adc::Emit emit{d_count, idx->d_vals.p, idx->d_keys.p, idx->d_sidx.p, d_base, d_cap};
        HIPCHECK(qadc::adc::launch_adc_pack(nq, emit, idx->d_packed.p, idx->stream));
        if (n_stored)
            HIPCHECK(hipMemcpyAsync(idx->h_packed.p, idx->d_packed.p, 3 * n_stored * 4, hipMemcpyDeviceToHost, idx->stream));
        HIPCHECK(hipStreamSynchronize(idx->stream));
    }

    // put every query's candidates in scan order (scan indices are distinct within a query)
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
    return QADC_OK;
}

}  // namespace

extern "C" {

int qadc_adc_index_create(qadc_adc_index** out, int sq_count, int sq_bits, int device_id) {
    if (!out) return fail(QADC_E_ARG, "out is null");
    DeviceGuard guard;
    *out = nullptr;
    if (sq_bits != 8 || (sq_count != 4 && sq_count != 8 && sq_count != 16))
        return fail(QADC_E_ARG,
                    "Unsupported (nsq,nsq_bits) configuration. Supported configurations are: (16,4) (4,8) (8,8) (16,8) (2,16) (4,16) "
                    "(8,16); this engine takes (4,8) (8,8) (16,8)");
    if (int rc = qadc_device_prepare(device_id)) return rc;   // (the device's stream set first: DESIGN.md section 5)
    qadc_adc_index* idx = new qadc_adc_index();
    idx->nsq = sq_count;
    idx->device = device_id;
    const hipError_t e = hipStreamCreateWithFlags(&idx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete idx;
        return fail(QADC_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    *out = idx;
    return QADC_OK;
}

int qadc_adc_index_destroy(qadc_adc_index* idx) {
    if (!idx) return QADC_OK;
    DeviceGuard guard;
    (void)hipSetDevice(idx->device);
    if (idx->stream) (void)hipStreamSynchronize(idx->stream);
    idx->codes.release();
    idx->labels.release();
    idx->d_off.release();
    idx->d_lab_off.release();
    idx->d_in.release();
    idx->d_vals.release();
    idx->d_keys.release();
    idx->d_sidx.release();
    idx->d_packed.release();
    idx->h_in.release();
    idx->h_count.release();
    idx->h_packed.release();
    if (idx->stream) (void)hipStreamDestroy(idx->stream);
    delete idx;
    return QADC_OK;
}

int qadc_adc_index_add_partitions(qadc_adc_index* idx, int part_count, const uint8_t* const* codes, const uint32_t* const* labels,
                                  const uint32_t* sizes) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
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
    uint64_t bytes = idx->code_bytes, nlab = idx->label_count;
    std::vector<uint64_t> off(part_count), loff(part_count);
    for (int p = 0; p < part_count; ++p) {
        off[p] = bytes;
        loff[p] = nlab;
        bytes += align_up((uint64_t)sizes[p] * idx->nsq, 16);
        if (lab == 1) nlab += sizes[p];
    }
    if (int rc = grow_device(idx->codes, idx->code_bytes, bytes + 16, idx->stream)) return rc;
    if (lab == 1)
        if (int rc = grow_labels(idx->labels, idx->label_count, std::max<uint64_t>(nlab, 1), idx->stream)) return rc;
    for (int p = 0; p < part_count; ++p) {
        if (!sizes[p]) continue;
        HIPCHECK(hipMemcpy(idx->codes.p + off[p], codes[p], (size_t)sizes[p] * idx->nsq, hipMemcpyHostToDevice));
        if (lab == 1) HIPCHECK(hipMemcpy(idx->labels.p + loff[p], labels[p], (size_t)sizes[p] * 4, hipMemcpyHostToDevice));
    }
    HIPCHECK(hipMemset(idx->codes.p + bytes, 0, 16));
    idx->labeled = lab;
    idx->code_bytes = bytes;
    idx->label_count = nlab;
    for (int p = 0; p < part_count; ++p) {
        idx->sizes.push_back(sizes[p]);
        idx->off.push_back(off[p]);
        idx->lab_off.push_back(loff[p]);
    }
    const size_t np = idx->sizes.size();
    HIPCHECK(idx->d_off.ensure(std::max<size_t>(np, 1)));
    HIPCHECK(idx->d_lab_off.ensure(std::max<size_t>(np, 1)));
    if (np) {
        HIPCHECK(hipMemcpy(idx->d_off.p, idx->off.data(), np * 8, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(idx->d_lab_off.p, idx->lab_off.data(), np * 8, hipMemcpyHostToDevice));
    }
    return QADC_OK;
}

int qadc_adc_index_partition_count(const qadc_adc_index* idx) { return idx ? (int)idx->sizes.size() : 0; }

uint64_t qadc_adc_index_reruns(const qadc_adc_index* idx) { return idx ? idx->reruns : 0; }

uint32_t qadc_adc_index_partition_size(const qadc_adc_index* idx, int part) {
    if (!idx || part < 0 || part >= (int)idx->sizes.size()) return 0;
    return idx->sizes[part];
}

int qadc_adc_query_scan(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R, int sum_mode,
                        uint32_t* keys, float* values, int32_t* sizes) {
    DeviceGuard guard;
    if (int rc = scan_batch(idx, nq, ma, assign, tables, R, sum_mode)) return rc;
    auto replay = [&](int q) {
        qadc::kv_heap<unsigned, float> bh(R);
        for (int t = 0; t < R; ++t) bh.push(0, std::numeric_limits<float>::max() - t);   // db_query.cpp:31-33
        for (uint64_t i = idx->stream_off[q]; i < idx->stream_off[q + 1]; ++i) bh.push(idx->stream_keys[i], idx->stream_vals[i]);
        if (keys) std::copy(bh.keys(), bh.keys() + bh.size(), keys + (size_t)q * R);
        if (values) std::copy(bh.values(), bh.values() + bh.size(), values + (size_t)q * R);
        if (sizes) sizes[q] = bh.size();
    };
    idx->pool.run(nq, idx->stream_off[nq] > 65536 ? 16 : 1, replay);
    return QADC_OK;
}

int qadc_adc_query_scan_candidates(qadc_adc_index* idx, int nq, int ma, const int32_t* assign, const float* tables, int R,
                                   int sum_mode, uint64_t cand_capacity, uint32_t* cand_keys, float* cand_vals, uint64_t* offsets) {
    if (!offsets) return fail(QADC_E_ARG, "offsets is required");
    DeviceGuard guard;
    if (int rc = scan_batch(idx, nq, ma, assign, tables, R, sum_mode)) return rc;
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

}  // extern "C"
