// db_add: the flow both engines share — qadc_adc_index_add_vectors*, _reserve and _read_partition
// (csrc/qadc_adc.cpp) over the owned float-ADC database, qadc_index_add_vectors*, _reserve and _read_partition
// (csrc/qadc_index_add.cpp) over the partitions of a 4-bit index.  Internal header, shaped like csrc/qadc_remove.h: the engine
// fills an AppendJob and one function runs it.  The storage is the engine's RowStore (csrc/qadc_host.h), the layout decisions are
// plan_append's (host/adc_append_plan.hpp, host/index_append_plan.hpp), the refusals host/append_check.hpp's, the kernels those of
// csrc/qadc_adc_kernel.hip and csrc/qadc_kernels.hip.
//
//   encode    the vectors of a pass (kAddChunk at most) are uploaded (host form) or read where they lie; launch_coarse_assign in
//             kCoarseChunk steps and launch_residual_rotate give what the engine's encoder takes (AppendJob::encode);
//   dispatch  with a coarse quantizer: count (launch_adc_add_count), the K + 1 counts come back in one pinned copy — the pass's one
//             synchronise before its rows are written — the host plans the room (make_room: nothing where the rows fit, else ONE
//             relocation) and the bases, launch_adc_add_scatter writes rows and labels in (assign, i) order.  Without: the rows go
//             to [labels_offset, labels_offset + count) of the one partition (launch_adc_copy_words);
//   tails     where the layout has a region pad, bytes [n * cs, index_padded_end(n * cs)) of every partition are zeroed
//             (launch_index_zero_tails) before the pass's closing synchronise.
// Every copy and memset is the Async form on the job's stream; the calls are synchronous.  A failed call leaves the partitions
// holding the rows they held (a relocation it made stands).
#pragma once
#include "../host/append_check.hpp"
#include "../host/index_append_plan.hpp"
#include "qadc_adc_kernels.h"
#include "qadc_host.h"

namespace qadc {
namespace host {

constexpr uint64_t kAddChunk = QADC_ADC_ADD_CHUNK;   // vectors of a pass
static_assert(QADC_INDEX_ADD_CHUNK == QADC_ADC_ADD_CHUNK, "both engines add in passes of one size");

// A relocation as the engine's move step sees it: the new buffers, allocated, with their offset tables uploaded (enqueued).
struct Relocation {
    const adc::AppendPlan& plan;
    const std::vector<uint32_t>& sizes;     // [parts] the rows every partition holds now
    uint8_t* codes;
    uint32_t* labels;                       // null: the new layout has no label buffer
    const uint64_t *d_off, *d_lab_off;
    Scratch& tmp;                           // device and host memory of the move step's own tables: both live until the move
    std::vector<unsigned char>& h_tmp;      // has completed
};

// The device scratch of one call's encoder, sized for its largest pass.
struct AddEncoder {
    Scratch mem;
    uint64_t pass = 0;   // vectors of the largest pass
    float *d_v = nullptr, *d_x = nullptr, *d_dist = nullptr, *d_qnorm = nullptr;
    const float* d_cnorm = nullptr;
    int32_t* d_assign = nullptr;
    uint8_t* d_codes = nullptr;
    unsigned long long* d_part = nullptr;   // the partial picks of the float-ADC engine's 16-bit encoder (its `prepare`)
};

struct AppendJob {
    RowStore* store = nullptr;
    hipStream_t stream = nullptr;
    int device = 0;
    int* labeled = nullptr;                 // the index's flag: -1 unknown, 0 keyed by position, 1 labelled
    bool* finalized = nullptr;              // the 4-bit index: cleared whenever rows or their addresses change
    std::vector<uint32_t> sizes;            // [parts] rows held; the flow advances them and hands them to set_sizes
    // the quantizers the index holds
    int dim = 0, K = 0;                     // dim 0: no set_pq yet;  K 0: flat (no coarse quantizer)
    int max_dim = 0;                        // the widest vector `encode` takes (0: any)
    const char* set_pq = "";                // the engine's set_pq entry point, for the refusal that names it
    const float *d_coarse = nullptr, *d_rotation = nullptr;   // [K][dim];  [dim][dim] or null
    const float* d_cnorm = nullptr;         // [K] the centroids' norms under the call's sum_mode; null: launch_row_sqnorm per call
    // what the engine does itself
    std::function<bool()> resident;         // every partition lies in the store (not set: the store's tables cover them)
    std::function<int(const Relocation&)> move;   // enqueues the move of every partition's rows and labels into the new buffers
    std::function<void()> rebind;           // not set, or: the new buffers are in the store and the old storage may be freed
    std::function<void(const std::vector<uint32_t>&)> set_sizes;   // the index has these partitions, holding these rows
    std::function<int(AddEncoder&, uint64_t count)> prepare;       // not set, or: scratch of the engine's encoder
    std::function<int(AddEncoder&, const float* d_enc, uint64_t cnt)> encode;   // d_enc [cnt][dim] -> enc.d_codes [cnt]

    bool is_resident() const { return resident ? resident() : store->covers(sizes.size()); }
    uint64_t tail_pad() const { return store->region_pad ? 0 : adc::kAppendTailPad; }   // bytes behind the last region
};

// Puts the database into the layout of `plan`, on the job's stream: new buffers, the offset tables uploaded, every partition moved
// by the engine's kernel (sizes [parts]: the rows each holds now), the tail padding zeroed; once the move is complete the new
// buffers are swapped in and the old storage is freed.  labels: the new layout has a label buffer.  A failure leaves the store and
// the index as they were.
inline int relocate(AppendJob& job, const adc::AppendPlan& plan, const std::vector<uint32_t>& sizes, bool labels) {
    RowStore& st = *job.store;
    const size_t parts = plan.cap.size();
    DevBuf<uint8_t> codes;
    DevBuf<uint32_t> labs;
    DevBuf<uint64_t> d_off, d_lab_off;
    Scratch tmp;
    std::vector<unsigned char> h_tmp;
    auto run = [&]() -> int {
        HIPCHECK(codes.ensure(std::max<uint64_t>(plan.code_bytes + job.tail_pad(), 16)));
        if (labels) HIPCHECK(labs.ensure(std::max<uint64_t>(plan.label_count, 1)));
        HIPCHECK(d_off.ensure(std::max<size_t>(parts, 1)));
        HIPCHECK(d_lab_off.ensure(std::max<size_t>(parts, 1)));
        if (parts) {
            HIPCHECK(hipMemcpyAsync(d_off.p, plan.off.data(), parts * 8, hipMemcpyHostToDevice, job.stream));
            HIPCHECK(hipMemcpyAsync(d_lab_off.p, plan.lab_off.data(), parts * 8, hipMemcpyHostToDevice, job.stream));
        }
        if (int rc = job.move(Relocation{plan, sizes, codes.p, labs.p, d_off.p, d_lab_off.p, tmp, h_tmp})) return rc;
        if (job.tail_pad()) HIPCHECK(adc::launch_adc_fill_words(codes.p + plan.code_bytes, job.tail_pad() / 4, 0u, job.stream));
        HIPCHECK(hipStreamSynchronize(job.stream));
        return QADC_OK;
    };
    const int rc = run();
    if (rc != QADC_OK) {
        (void)hipStreamSynchronize(job.stream);
    } else {   // the new buffers into the store; what the four locals hold from here on is the old storage
        std::swap(st.codes, codes);
        std::swap(st.labels, labs);
        std::swap(st.d_off, d_off);
        std::swap(st.d_lab_off, d_lab_off);
        st.caps = plan.cap;
        st.off = plan.off;
        st.lab_off = plan.lab_off;
        st.code_bytes = plan.code_bytes;
        st.label_count = plan.label_count;
        if (job.rebind) job.rebind();
        if (job.finalized) *job.finalized = false;   // (the partition table and the byte-plane copies of qadc_index_finalize describe the old storage)
    }
    codes.release();
    labs.release();
    d_off.release();
    d_lab_off.release();
    return rc;
}

// The capacities plan_append starts from (a partition outside the store holds exactly its rows).
inline std::vector<uint32_t> current_caps(const AppendJob& job) { return job.is_resident() ? job.store->caps : job.sizes; }

// Room for add[p] more rows behind the sizes[p] every partition holds: nothing to do where they fit and the store is resident, else
// one relocation.
inline int make_room(AppendJob& job, const std::vector<uint64_t>& add, bool labels, bool* moved) {
    RowStore& st = *job.store;
    const std::vector<uint32_t> caps = current_caps(job);
    const adc::AppendPlan plan = adc::plan_append(st.code_size, job.sizes.size(), job.sizes.data(), caps.data(), add.data(), nullptr, true, st.region_pad);
    if (!plan.refused.empty()) return fail(QADC_E_ARG, plan.refused);
    if (!plan.in_place) *moved = true;
    if (!plan.in_place || !job.is_resident()) return relocate(job, plan, job.sizes, labels);
    if (labels && st.labels.cap < std::max<uint64_t>(st.label_count, 1))   // (room reserved before the index had labels)
        HIPCHECK(st.labels.ensure(std::max<uint64_t>(st.label_count, 1)));
    return QADC_OK;
}

// The encoder's scratch for a call of `count` vectors; the centroids' norms where the engine has none cached.
inline int prepare_encoder(AppendJob& job, AddEncoder& enc, uint64_t count, int sum_mode, bool d_side) {
    enc.pass = std::min<uint64_t>(kAddChunk, count);
    if (!d_side) HIPCHECK(enc.mem.alloc(&enc.d_v, enc.pass * job.dim * 4));
    if (job.K || job.d_rotation) HIPCHECK(enc.mem.alloc(&enc.d_x, enc.pass * job.dim * 4));
    HIPCHECK(enc.mem.alloc(&enc.d_codes, enc.pass * job.store->code_size));
    if (job.K) {
        const uint64_t chunk = std::min<uint64_t>(kCoarseChunk, enc.pass), K = (uint64_t)job.K;
        HIPCHECK(enc.mem.alloc(&enc.d_dist, (chunk * (K + 1) + (job.d_cnorm ? 0 : K)) * 4));
        enc.d_qnorm = enc.d_dist + chunk * K;
        enc.d_cnorm = job.d_cnorm;
        HIPCHECK(enc.mem.alloc(&enc.d_assign, enc.pass * 4));
        if (!job.d_cnorm) {
            float* d_norm = enc.d_qnorm + chunk;
            launch_row_sqnorm(job.d_coarse, job.K, job.dim, sum_mode, d_norm, job.stream);   // (the call's sum_mode, not a search option's)
            HIPCHECK(hipGetLastError());
            enc.d_cnorm = d_norm;
        }
    }
    return job.prepare ? job.prepare(enc, count) : QADC_OK;
}

// vectors [cnt][dim] (host memory, or device memory read where it lies) -> enc.d_assign [cnt] (with a coarse quantizer), enc.d_codes [cnt]
inline int encode_pass(AppendJob& job, AddEncoder& enc, const float* vectors, uint64_t cnt, int sum_mode, bool d_side) {
    const int dim = job.dim;
    const float* src = vectors;
    if (!d_side) {
        HIPCHECK(hipMemcpyAsync(enc.d_v, vectors, cnt * dim * 4, hipMemcpyHostToDevice, job.stream));
        src = enc.d_v;
    }
    const float* d_enc = src;
    if (job.K) {   // find_k_neighbors(k = 1) on the coarse centroids
        for (uint64_t c = 0; c < cnt; c += kCoarseChunk)
            launch_coarse_assign(src + c * dim, job.d_coarse, (int)std::min<uint64_t>(kCoarseChunk, cnt - c), job.K, dim, 1, enc.d_qnorm, enc.d_cnorm,
                                 sum_mode, enc.d_dist, enc.d_assign + c, job.stream);
        HIPCHECK(hipGetLastError());
    }
    if (job.K || job.d_rotation) {
        launch_residual_rotate(src, cnt, dim, job.K ? job.d_coarse : nullptr, enc.d_assign, job.d_rotation, enc.d_x, job.stream);
        HIPCHECK(hipGetLastError());
        d_enc = enc.d_x;
    }
    return job.encode(enc, d_enc, cnt);
}

// Where the layout has a region pad: bytes [n * cs, index_padded_end(n * cs)) behind the last row of every partition zeroed, for the
// sizes given; the stream is drained on return (h_stage is written again).
inline int zero_tails(AppendJob& job, const std::vector<uint32_t>& sizes, uint32_t* h_stage, uint32_t* d_sizes) {
    const RowStore& st = *job.store;
    std::copy(sizes.begin(), sizes.end(), h_stage);
    HIPCHECK(hipMemcpyAsync(d_sizes, h_stage, sizes.size() * 4, hipMemcpyHostToDevice, job.stream));
    HIPCHECK(adc::launch_index_zero_tails(st.codes.p, st.d_off.p, d_sizes, (uint32_t)sizes.size(), st.code_size, job.stream));
    HIPCHECK(hipStreamSynchronize(job.stream));
    return QADC_OK;
}

// index_db::add_vectors (databases.hpp:270-298) pass by pass: encode, count, plan, relocate if needed, scatter.  job.sizes advance
// pass by pass.  labels [count] (host or device memory, as the vectors) or null: the label of vector i, in place of labels_offset + i.
inline int append_ivf(AppendJob& job, const float* vectors, const uint32_t* labels, uint64_t count, uint32_t labels_offset, int sum_mode, bool d_side,
                      bool* moved) {
    using namespace qadc::adc;
    RowStore& st = *job.store;
    const uint32_t K = (uint32_t)job.K;
    const bool pad = st.region_pad != 0;
    std::vector<uint64_t> add(K, 0);
    if (count == 0) return job.is_resident() ? QADC_OK : make_room(job, add, *job.labeled == 1, moved);
    AddEncoder enc;
    if (int rc = prepare_encoder(job, enc, count, sum_mode, d_side)) return rc;
    uint32_t *d_count = nullptr, *d_base = nullptr, *d_sizes = nullptr, *d_hist = nullptr, *d_perm_a = nullptr, *d_perm_b = nullptr;
    HIPCHECK(enc.mem.alloc(&d_count, ((size_t)K + 1) * 4));
    HIPCHECK(enc.mem.alloc(&d_base, (size_t)K * 4));
    if (pad) HIPCHECK(enc.mem.alloc(&d_sizes, (size_t)K * 4));
    HIPCHECK(enc.mem.alloc(&d_hist, (enc.pass / kAddTile + 1) * 256 * 4));
    if (K > 256) HIPCHECK(enc.mem.alloc(&d_perm_a, enc.pass * 4));
    if (K > 65536) HIPCHECK(enc.mem.alloc(&d_perm_b, enc.pass * 4));
    uint32_t* d_lab = nullptr;   // the labels of a pass, uploaded beside its vectors
    if (labels && !d_side) HIPCHECK(enc.mem.alloc(&d_lab, enc.pass * 4));
    HIPCHECK(st.h_add.ensure(3 * (size_t)K + 1));
    uint32_t *h_count = st.h_add.p, *h_base = h_count + K + 1, *h_sizes = h_base + K;
    for (uint64_t o = 0; o < count; o += kAddChunk) {
        const uint64_t cnt = std::min<uint64_t>(kAddChunk, count - o);
        if (int rc = encode_pass(job, enc, vectors + o * job.dim, cnt, sum_mode, d_side)) return rc;
        const uint32_t* d_pass_lab = labels ? labels + o : nullptr;
        if (d_lab) {
            HIPCHECK(hipMemcpyAsync(d_lab, labels + o, cnt * 4, hipMemcpyHostToDevice, job.stream));
            d_pass_lab = d_lab;
        }
        HIPCHECK(hipMemsetAsync(d_count, 0, ((size_t)K + 1) * 4, job.stream));
        HIPCHECK(launch_adc_add_count(enc.d_assign, (uint32_t)cnt, K, d_count, job.stream));
        HIPCHECK(hipMemcpyAsync(h_count, d_count, ((size_t)K + 1) * 4, hipMemcpyDeviceToHost, job.stream));
        HIPCHECK(hipStreamSynchronize(job.stream));
        if (h_count[K])
            return fail(QADC_E_ARG, std::to_string(h_count[K]) + " vectors were assigned outside the " + std::to_string(K) + " partitions");
        std::copy(h_count, h_count + K, add.begin());
        append_bases(K, job.sizes.data(), h_count, h_base);
        if (int rc = make_room(job, add, true, moved)) return rc;
        HIPCHECK(hipMemcpyAsync(d_base, h_base, (size_t)K * 4, hipMemcpyHostToDevice, job.stream));
        const AddDst dst{st.codes.p, st.d_off.p, st.labels.p, st.d_lab_off.p, d_base};
        HIPCHECK(launch_adc_add_scatter(enc.d_assign, (uint32_t)cnt, K, st.code_size, enc.d_codes, labels_offset + (uint32_t)o, d_pass_lab, dst, d_hist,
                                        d_perm_a, d_perm_b, job.stream));
        if (pad) {
            for (uint32_t p = 0; p < K; ++p) h_sizes[p] = job.sizes[p] + h_count[p];
            HIPCHECK(hipMemcpyAsync(d_sizes, h_sizes, (size_t)K * 4, hipMemcpyHostToDevice, job.stream));
            HIPCHECK(launch_index_zero_tails(st.codes.p, st.d_off.p, d_sizes, K, st.code_size, job.stream));
        }
        HIPCHECK(hipStreamSynchronize(job.stream));   // (the pinned block is written again by the next pass)
        for (uint32_t p = 0; p < K; ++p) job.sizes[p] += h_count[p];
    }
    return QADC_OK;
}

// flat_db::add_vectors (databases.hpp:136-156): the rows go to [labels_offset, labels_offset + count) of the one partition.
inline int append_flat(AppendJob& job, const float* vectors, uint64_t count, uint32_t labels_offset, int sum_mode, bool d_side, bool* moved) {
    using namespace qadc::adc;
    RowStore& st = *job.store;
    const uint32_t old = job.sizes[0];
    const uint32_t size = (uint32_t)std::max<uint64_t>(old, (uint64_t)labels_offset + count);
    const int cs = st.code_size;
    if (int rc = make_room(job, std::vector<uint64_t>{(uint64_t)size - old}, false, moved)) return rc;
    uint8_t* part = st.part_codes(0);
    if (job.finalized) *job.finalized = false;   // (rows that exist may be overwritten from here on: a byte-plane copy would disagree with them)
    if (labels_offset > old)   // the rows of the gap are zero bytes, as std::vector::resize leaves them
        HIPCHECK(launch_adc_fill_words(part + (uint64_t)old * cs, ((uint64_t)labels_offset - old) * cs / 4, 0u, job.stream));
    AddEncoder enc;
    uint32_t* d_size = nullptr;
    if (st.region_pad) HIPCHECK(enc.mem.alloc(&d_size, 4));
    if (count) {
        if (int rc = prepare_encoder(job, enc, count, sum_mode, d_side)) return rc;
        for (uint64_t o = 0; o < count; o += kAddChunk) {
            const uint64_t cnt = std::min<uint64_t>(kAddChunk, count - o);
            if (int rc = encode_pass(job, enc, vectors + o * job.dim, cnt, sum_mode, d_side)) return rc;
            HIPCHECK(launch_adc_copy_words(enc.d_codes, part + ((uint64_t)labels_offset + o) * cs, cnt * cs / 4, job.stream));
        }
    }
    job.sizes[0] = size;
    if (!st.region_pad) {
        HIPCHECK(hipStreamSynchronize(job.stream));
        return QADC_OK;
    }
    HIPCHECK(st.h_add.ensure(4));
    return zero_tails(job, job.sizes, st.h_add.p, d_size);
}

// add_vectors of both engines, after the engine's own refusals.  labelled: the call is *_add_vectors_labelled / _device, which takes
// labels [count] and no labels_offset.
inline int append_vectors(AppendJob& job, const float* vectors, const uint32_t* labels, bool labelled, uint64_t count, uint32_t labels_offset,
                          int sum_mode, bool d_side, const char* call) {
    RowStore& st = *job.store;
    adc::AppendCall c;
    c.call = call;
    c.set_pq = job.set_pq;
    c.dim = job.dim;
    c.K = job.K;
    c.max_dim = job.max_dim;
    c.labeled = *job.labeled;
    c.sizes = job.sizes.data();
    c.parts = job.sizes.size();
    c.labelled = labelled;
    c.has_vectors = vectors != nullptr;
    c.has_labels = labels != nullptr;
    c.count = count;
    c.labels_offset = labels_offset;
    c.sum_mode = sum_mode;
    const adc::AppendRefusal refusal = adc::check_add_vectors(c);
    if (refusal.status != QADC_OK) return fail(refusal.status, refusal.text);
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(job.device));
    // what a failed call puts back: the rows of every partition (rows written behind them are not part of the database)
    const std::vector<uint32_t> sizes0 = job.sizes;
    const int labeled0 = *job.labeled;
    const bool fresh = sizes0.empty();
    if (fresh) {
        job.sizes.assign(job.K ? (size_t)job.K : 1, 0);
        job.set_sizes(job.sizes);
    }
    if (job.K) {
        if (count) *job.labeled = 1;
    } else if (std::max<uint64_t>(job.sizes[0], (uint64_t)labels_offset + count)) {
        *job.labeled = 0;
    }
    bool moved = false;
    const int rc = job.K ? append_ivf(job, vectors, labels, count, labels_offset, sum_mode, d_side, &moved)
                         : append_flat(job, vectors, count, labels_offset, sum_mode, d_side, &moved);
    if (rc != QADC_OK) {
        const std::string msg = g_err;
        (void)hipStreamSynchronize(job.stream);
        *job.labeled = labeled0;
        job.sizes = sizes0;
        job.set_sizes(sizes0);
        if (fresh) {   // the index held no partition: it holds none again
            st.release();
        } else if (st.region_pad && job.is_resident()) {   // (a relocation of this call stands; its partitions hold the rows they held)
            uint32_t* d_sizes = nullptr;
            Scratch mem;
            if (mem.alloc(&d_sizes, sizes0.size() * 4) == hipSuccess && st.h_add.ensure(sizes0.size()) == hipSuccess)
                (void)zero_tails(job, sizes0, st.h_add.p, d_sizes);
        }
        g_err = msg;
        return rc;
    }
    job.set_sizes(job.sizes);
    if (moved) ++st.relocations;
    if (job.finalized) *job.finalized = false;
    return QADC_OK;
}

// *_reserve of both engines, after the engine's own refusals: at least part_count partitions, partition p with room for
// capacities[p] rows.
inline int reserve_rows(AppendJob& job, int part_count, const uint32_t* capacities) {
    const adc::AppendRefusal refusal = adc::check_reserve(part_count, capacities != nullptr);
    if (refusal.status != QADC_OK) return fail(refusal.status, refusal.text);
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(job.device));
    RowStore& st = *job.store;
    const size_t before = job.sizes.size(), parts = std::max(before, (size_t)part_count);
    if (parts == 0) return QADC_OK;
    const std::vector<uint32_t> sizes0 = job.sizes;
    std::vector<uint32_t> floor(parts, 0), caps = current_caps(job);
    std::copy(capacities, capacities + part_count, floor.begin());
    caps.resize(parts, 0);
    job.sizes.resize(parts, 0);
    const std::vector<uint64_t> add(parts, 0);
    const adc::AppendPlan plan = adc::plan_append(st.code_size, parts, job.sizes.data(), caps.data(), add.data(), floor.data(), false, st.region_pad);
    if (!plan.refused.empty()) return fail(QADC_E_ARG, plan.refused);
    if (plan.in_place && parts == before && job.is_resident()) return QADC_OK;
    job.set_sizes(job.sizes);
    const int rc = relocate(job, plan, job.sizes, *job.labeled == 1);
    if (rc != QADC_OK) job.set_sizes(sizes0);
    return rc;
}

// *_read_partition of both engines, after the engine's own refusals: rows [first, first + count) of partition `part` into host memory.
// d_codes / d_labels: where the partition's rows and labels lie (anything for a partition that does not exist; labels null: the
// index has none to read).
inline int read_rows(const AppendJob& job, int part, uint32_t first, uint32_t count, const uint8_t* d_codes, const uint32_t* d_labels,
                     uint8_t* codes_out, uint32_t* labels_out) {
    const adc::AppendRefusal refusal = adc::check_read_partition(job.sizes.data(), job.sizes.size(), part, first, count);
    if (refusal.status != QADC_OK) return fail(refusal.status, refusal.text);
    if (!count) return QADC_OK;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(job.device));
    const size_t cs = (size_t)job.store->code_size;
    if (codes_out) HIPCHECK(hipMemcpyAsync(codes_out, d_codes + first * cs, count * cs, hipMemcpyDeviceToHost, job.stream));
    if (labels_out && d_labels) HIPCHECK(hipMemcpyAsync(labels_out, d_labels + first, (size_t)count * 4, hipMemcpyDeviceToHost, job.stream));
    HIPCHECK(hipStreamSynchronize(job.stream));
    return QADC_OK;
}

}  // namespace host
}  // namespace qadc
