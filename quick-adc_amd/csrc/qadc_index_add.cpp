// db_add on the 4-bit index: qadc_index_add_vectors / _add_vectors_device encode vectors with the
// quantizers the index holds (FeederState) and append the codes to partitions that grow in device memory; qadc_index_reserve,
// _read_partition and _relocations complete the set, and qadc_index_remove_labels (section 11.7) takes rows out again.  index_db::add_vectors (databases.hpp:270-298) with a coarse quantizer,
// flat_db::add_vectors (136-156) without.
//
// The encoder is the chain of qadc_ivf_encode_host_mode(encode_form = 1) — launch_coarse_assign, launch_residual_rotate,
// launch_pq_encode — in passes of QADC_INDEX_ADD_CHUNK vectors on the index's stream; the dispatch is the float-ADC engine's
// (launch_adc_add_count, launch_adc_add_scatter: a stable radix sort of (assign, i), csrc/qadc_adc_kernels.h) over the offset
// tables of the index's arena.  The arena (ArenaState, csrc/qadc_host.h) holds every partition of an index that has grown, in
// the layout of host/index_append_plan.hpp; the first growing call moves partitions that are allocations of their own into it
// (launch_index_move) and frees them.  One stream synchronise per pass brings the K + 1 counts to the host, which plans the room.
#include "qadc_host.h"

#include "../host/index_append_plan.hpp"
#include "qadc_adc_kernels.h"
#include "qadc_remove.h"

using namespace qadc;
using namespace qadc::host;
using namespace qadc::adc;

namespace {

// What every growing call refuses, before the device is touched.  `call`: the entry point's name.
int refuse(const qadc_index* idx, const char* call) {
    for (int i = 0; i < kSlots; ++i)
        if (idx->slot[i].busy) return fail(QADC_E_STATE, std::string(call) + ": slot " + std::to_string(i) + " holds a batch that has not been collected");
    if (idx->pre_slot[0].busy || idx->pre_slot[1].busy) return fail(QADC_E_STATE, std::string(call) + ": a sharded pre-scan has not been collected");
    if (idx->adc_views > 0)
        return fail(QADC_E_ARG, std::string(call) + ": the index has " + std::to_string(idx->adc_views) +
                                    " live float-ADC view(s), which keep the partitions' addresses: destroy them first");
    if (idx->dist) return fail(QADC_E_ARG, std::string(call) + ": the index takes part in a multi-GPU merge (qadc_dist_init)");
    for (size_t p = 0; p < idx->parts.size(); ++p) {
        const Part& pt = idx->parts[p];
        if (pt.d_starts || pt.n != pt.global_n || pt.first_pos != 0)
            return fail(QADC_E_ARG, std::string(call) + ": partition " + std::to_string(p) + " is a shard or holds a starts replica");
        if (!pt.own) return fail(QADC_E_ARG, std::string(call) + ": partition " + std::to_string(p) + " is borrowed (qadc_index_add_partition_device)");
    }
    return QADC_OK;
}

bool resident(const qadc_index* idx) {   // every partition lies in the arena
    if (!idx->arena.active() || idx->arena.caps.size() != idx->parts.size()) return false;
    return std::all_of(idx->parts.begin(), idx->parts.end(), [](const Part& p) { return p.arena; });
}

std::vector<uint32_t> current_caps(const qadc_index* idx) {   // (a partition outside the arena holds exactly its rows)
    std::vector<uint32_t> caps(idx->parts.size());
    const bool in = resident(idx);
    for (size_t p = 0; p < caps.size(); ++p) caps[p] = in ? idx->arena.caps[p] : idx->parts[p].n;
    return caps;
}

// The partitions' pointers from the arena's tables; their sizes where `sizes` is given.
void bind_parts(qadc_index* idx, const std::vector<uint32_t>* sizes) {
    ArenaState& a = idx->arena;
    for (size_t p = 0; p < idx->parts.size(); ++p) {
        Part& pt = idx->parts[p];
        pt.d_codes = a.codes.p + a.off[p];
        pt.d_labels = idx->labeled == 1 && a.labels.p ? a.labels.p + a.lab_off[p] : nullptr;
        pt.arena = true;
        if (sizes) pt.n = (*sizes)[p];
        pt.global_n = pt.n;
        pt.starts_cap = pt.n;
    }
}

// Puts the database into the layout of `plan`, on the index's stream: a new arena, every partition gathered into its region by one
// kernel (sizes [parts]: the rows each holds now), then the old storage — the partitions' own allocations, or the old arena —
// freed.  labels: the new layout has a label arena.  A failure leaves the index as it was.
int relocate(qadc_index* idx, const AppendPlan& plan, const std::vector<uint32_t>& sizes, bool labels) {
    ArenaState& a = idx->arena;
    const size_t parts = plan.cap.size();
    DevBuf<uint8_t> codes;
    DevBuf<uint32_t> labs;
    DevBuf<uint64_t> d_off, d_lab_off;
    DevBuf<IndexMove> d_moves;
    std::vector<IndexMove> moves(parts);
    auto drop = [&]() { codes.release(); labs.release(); d_off.release(); d_lab_off.release(); d_moves.release(); };
    auto run = [&]() -> int {
        HIPCHECK(codes.ensure(std::max<uint64_t>(plan.code_bytes, 16)));
        if (labels) HIPCHECK(labs.ensure(std::max<uint64_t>(plan.label_count, 1)));
        HIPCHECK(d_off.ensure(std::max<size_t>(parts, 1)));
        HIPCHECK(d_lab_off.ensure(std::max<size_t>(parts, 1)));
        HIPCHECK(d_moves.ensure(std::max<size_t>(parts, 1)));
        uint32_t longest = 0;
        for (size_t p = 0; p < parts; ++p) {
            const Part& pt = idx->parts[p];
            const bool move_labels = labels && sizes[p] && pt.d_labels && idx->labeled == 1;
            moves[p] = IndexMove{sizes[p] ? pt.d_codes : nullptr, codes.p + plan.off[p], move_labels ? pt.d_labels : nullptr,
                                 move_labels ? labs.p + plan.lab_off[p] : nullptr, sizes[p], 0};
            longest = std::max(longest, sizes[p]);
        }
        if (parts) {
            HIPCHECK(hipMemcpyAsync(d_off.p, plan.off.data(), parts * 8, hipMemcpyHostToDevice, idx->stream));
            HIPCHECK(hipMemcpyAsync(d_lab_off.p, plan.lab_off.data(), parts * 8, hipMemcpyHostToDevice, idx->stream));
            HIPCHECK(hipMemcpyAsync(d_moves.p, moves.data(), parts * sizeof(IndexMove), hipMemcpyHostToDevice, idx->stream));
            HIPCHECK(launch_index_move(d_moves.p, (int)parts, idx->cs, longest, idx->stream));
        }
        HIPCHECK(hipStreamSynchronize(idx->stream));
        return QADC_OK;
    };
    if (int rc = run()) {
        (void)hipStreamSynchronize(idx->stream);
        drop();
        return rc;
    }
    d_moves.release();
    for (Part& pt : idx->parts) {   // the old storage
        if (!pt.arena) {
            if (pt.d_codes) (void)hipFree(pt.d_codes);
            if (pt.d_labels) (void)hipFree(pt.d_labels);
        }
        pt.d_codes = nullptr;
        pt.d_labels = nullptr;
    }
    a.codes.release();
    a.labels.release();
    a.d_off.release();
    a.d_lab_off.release();
    a.codes = codes;
    a.labels = labs;
    a.d_off = d_off;
    a.d_lab_off = d_lab_off;
    a.caps = plan.cap;
    a.off = plan.off;
    a.lab_off = plan.lab_off;
    a.code_bytes = plan.code_bytes;
    a.label_count = plan.label_count;
    bind_parts(idx, nullptr);
    idx->finalized = false;   // (the partition table and the byte-plane copies of qadc_index_finalize describe the old storage)
    return QADC_OK;
}

// Room for add[p] more rows behind the sizes[p] every partition holds: nothing to do where they fit in the arena, else one relocation.
int make_room(qadc_index* idx, const std::vector<uint32_t>& sizes, const std::vector<uint64_t>& add, bool labels, bool* moved) {
    ArenaState& a = idx->arena;
    const std::vector<uint32_t> caps = current_caps(idx);
    const AppendPlan plan = plan_index_append(idx->cs, sizes.size(), sizes.data(), caps.data(), add.data(), nullptr, true);
    if (!plan.refused.empty()) return fail(QADC_E_ARG, plan.refused);
    if (!plan.in_place) *moved = true;
    if (!plan.in_place || !resident(idx)) return relocate(idx, plan, sizes, labels);
    if (labels && a.labels.cap < std::max<uint64_t>(a.label_count, 1))   // (room reserved before the index had labels)
        HIPCHECK(a.labels.ensure(std::max<uint64_t>(a.label_count, 1)));
    return QADC_OK;
}

// The encoder of one call: the steps and kernels of qadc_ivf_encode_host_mode(encode_form = 1, sum_mode) on the index's quantizers
// and stream, into device scratch sized for one pass.
struct AddEncoder {
    Scratch mem;
    uint64_t pass = 0;   // vectors of the largest pass
    float *d_v = nullptr, *d_x = nullptr, *d_dist = nullptr, *d_qnorm = nullptr, *d_cnorm = nullptr;
    int32_t* d_assign = nullptr;
    uint8_t* d_codes = nullptr;

    int prepare(const qadc_index* idx, uint64_t count, int sum_mode, bool d_side) {
        const FeederState& f = idx->feed;
        pass = std::min<uint64_t>(QADC_INDEX_ADD_CHUNK, count);
        if (!d_side) HIPCHECK(mem.alloc(&d_v, pass * f.dim * 4));
        if (f.K || f.has_rotation) HIPCHECK(mem.alloc(&d_x, pass * f.dim * 4));
        HIPCHECK(mem.alloc(&d_codes, pass * idx->cs));
        if (f.K) {
            const uint64_t chunk = std::min<uint64_t>(kCoarseChunk, pass);
            HIPCHECK(mem.alloc(&d_dist, (chunk * ((uint64_t)f.K + 1) + (uint64_t)f.K) * 4));
            d_qnorm = d_dist + chunk * (uint64_t)f.K;
            d_cnorm = d_qnorm + chunk;
            HIPCHECK(mem.alloc(&d_assign, pass * 4));
            launch_row_sqnorm(f.d_coarse.p, f.K, f.dim, sum_mode, d_cnorm, idx->stream);   // (the call's sum_mode, not the search option's)
            HIPCHECK(hipGetLastError());
        }
        return QADC_OK;
    }

    // vectors [cnt][dim] (host memory, or device memory read where it lies) -> d_assign [cnt] (with a coarse quantizer), d_codes [cnt]
    int encode(qadc_index* idx, const float* vectors, uint64_t cnt, int sum_mode, bool d_side) {
        const FeederState& f = idx->feed;
        const float* src = vectors;
        if (!d_side) {
            HIPCHECK(hipMemcpyAsync(d_v, vectors, cnt * f.dim * 4, hipMemcpyHostToDevice, idx->stream));
            src = d_v;
        }
        const float* d_enc = src;
        if (f.K) {   // find_k_neighbors(k = 1) on the coarse centroids
            for (uint64_t c = 0; c < cnt; c += kCoarseChunk)
                launch_coarse_assign(src + c * f.dim, f.d_coarse.p, (int)std::min<uint64_t>(kCoarseChunk, cnt - c), f.K, f.dim, 1, d_qnorm, d_cnorm,
                                     sum_mode, d_dist, d_assign + c, idx->stream);
            HIPCHECK(hipGetLastError());
        }
        if (f.K || f.has_rotation) {
            launch_residual_rotate(src, cnt, f.dim, f.K ? f.d_coarse.p : nullptr, d_assign, f.has_rotation ? f.d_rotation.p : nullptr, d_x, idx->stream);
            HIPCHECK(hipGetLastError());
            d_enc = d_x;
        }
        launch_pq_encode(d_enc, cnt, idx->M, f.dim, f.d_codebooks.p, 1, sum_mode, d_codes, idx->stream);
        HIPCHECK(hipGetLastError());
        return QADC_OK;
    }
};

// bytes [n * cs, align16(n * cs) + 64) behind the last row of every partition zeroed, for the sizes given
int zero_tails(qadc_index* idx, const std::vector<uint32_t>& sizes, uint32_t* h_stage, uint32_t* d_sizes) {
    std::copy(sizes.begin(), sizes.end(), h_stage);
    HIPCHECK(hipMemcpyAsync(d_sizes, h_stage, sizes.size() * 4, hipMemcpyHostToDevice, idx->stream));
    HIPCHECK(launch_index_zero_tails(idx->arena.codes.p, idx->arena.d_off.p, d_sizes, (uint32_t)sizes.size(), idx->cs, idx->stream));
    HIPCHECK(hipStreamSynchronize(idx->stream));   // (h_stage is written again)
    return QADC_OK;
}

// index_db::add_vectors (databases.hpp:270-298) pass by pass: encode, count, plan, relocate if needed, scatter.  sizes: the rows
// every partition holds, advanced pass by pass (the partitions take them when the call has succeeded).  labels [count] (host or
// device memory, as the vectors) or null: the label of vector i, in place of labels_offset + i.
int add_ivf(qadc_index* idx, std::vector<uint32_t>& sizes, const float* vectors, const uint32_t* labels, uint64_t count, uint32_t labels_offset,
            int sum_mode, bool d_side, bool* moved) {
    const uint32_t K = (uint32_t)idx->feed.K;
    std::vector<uint64_t> add(K, 0);
    if (count == 0) return resident(idx) ? QADC_OK : make_room(idx, sizes, add, idx->labeled == 1, moved);
    AddEncoder enc;
    if (int rc = enc.prepare(idx, count, sum_mode, d_side)) return rc;
    uint32_t *d_count = nullptr, *d_base = nullptr, *d_sizes = nullptr, *d_hist = nullptr, *d_perm_a = nullptr, *d_perm_b = nullptr;
    HIPCHECK(enc.mem.alloc(&d_count, ((size_t)K + 1) * 4));
    HIPCHECK(enc.mem.alloc(&d_base, (size_t)K * 4));
    HIPCHECK(enc.mem.alloc(&d_sizes, (size_t)K * 4));
    HIPCHECK(enc.mem.alloc(&d_hist, (enc.pass / kAddTile + 1) * 256 * 4));
    if (K > 256) HIPCHECK(enc.mem.alloc(&d_perm_a, enc.pass * 4));
    if (K > 65536) HIPCHECK(enc.mem.alloc(&d_perm_b, enc.pass * 4));
    uint32_t* d_lab = nullptr;   // the labels of a pass, uploaded beside its vectors
    if (labels && !d_side) HIPCHECK(enc.mem.alloc(&d_lab, enc.pass * 4));
    HIPCHECK(idx->arena.h_add.ensure(3 * (size_t)K + 1));
    uint32_t *h_count = idx->arena.h_add.p, *h_base = h_count + K + 1, *h_sizes = h_base + K;
    for (uint64_t o = 0; o < count; o += QADC_INDEX_ADD_CHUNK) {
        const uint64_t cnt = std::min<uint64_t>(QADC_INDEX_ADD_CHUNK, count - o);
        if (int rc = enc.encode(idx, vectors + o * idx->feed.dim, cnt, sum_mode, d_side)) return rc;
        const uint32_t* d_pass_lab = labels ? labels + o : nullptr;
        if (d_lab) {
            HIPCHECK(hipMemcpyAsync(d_lab, labels + o, cnt * 4, hipMemcpyHostToDevice, idx->stream));
            d_pass_lab = d_lab;
        }
        HIPCHECK(hipMemsetAsync(d_count, 0, ((size_t)K + 1) * 4, idx->stream));
        HIPCHECK(launch_adc_add_count(enc.d_assign, (uint32_t)cnt, K, d_count, idx->stream));
        HIPCHECK(hipMemcpyAsync(h_count, d_count, ((size_t)K + 1) * 4, hipMemcpyDeviceToHost, idx->stream));
        HIPCHECK(hipStreamSynchronize(idx->stream));
        if (h_count[K])
            return fail(QADC_E_ARG, std::to_string(h_count[K]) + " vectors were assigned outside the " + std::to_string(K) + " partitions");
        uint32_t below = 0;
        for (uint32_t p = 0; p < K; ++p) {
            add[p] = h_count[p];
            h_base[p] = sizes[p] - below;   // (modulo 2^32: the kernel adds the position in (assign, i) order)
            below += h_count[p];
        }
        if (int rc = make_room(idx, sizes, add, true, moved)) return rc;
        for (uint32_t p = 0; p < K; ++p) h_sizes[p] = sizes[p] + h_count[p];
        HIPCHECK(hipMemcpyAsync(d_base, h_base, (size_t)K * 4, hipMemcpyHostToDevice, idx->stream));
        const ArenaState& a = idx->arena;
        const AddDst dst{a.codes.p, a.d_off.p, a.labels.p, a.d_lab_off.p, d_base};
        HIPCHECK(launch_adc_add_scatter(enc.d_assign, (uint32_t)cnt, K, idx->cs, enc.d_codes, labels_offset + (uint32_t)o, d_pass_lab, dst, d_hist,
                                        d_perm_a, d_perm_b, idx->stream));
        HIPCHECK(hipMemcpyAsync(d_sizes, h_sizes, (size_t)K * 4, hipMemcpyHostToDevice, idx->stream));
        HIPCHECK(launch_index_zero_tails(a.codes.p, a.d_off.p, d_sizes, K, idx->cs, idx->stream));
        HIPCHECK(hipStreamSynchronize(idx->stream));   // (the pinned block is written again by the next pass)
        for (uint32_t p = 0; p < K; ++p) sizes[p] += h_count[p];
    }
    return QADC_OK;
}

// flat_db::add_vectors (databases.hpp:136-156): the rows go to [labels_offset, labels_offset + count) of the one partition.
int add_flat(qadc_index* idx, std::vector<uint32_t>& sizes, const float* vectors, uint64_t count, uint32_t labels_offset, int sum_mode, bool d_side,
             bool* moved) {
    const uint32_t old = sizes[0];
    const uint32_t size = (uint32_t)std::max<uint64_t>(old, (uint64_t)labels_offset + count);
    const int cs = idx->cs;
    if (int rc = make_room(idx, sizes, std::vector<uint64_t>{(uint64_t)size - old}, false, moved)) return rc;
    uint8_t* part = idx->arena.codes.p + idx->arena.off[0];
    idx->finalized = false;   // (rows that exist may be overwritten from here on: a byte-plane copy would disagree with them)
    if (labels_offset > old)   // the rows of the gap are zero bytes, as std::vector::resize leaves them
        HIPCHECK(launch_adc_fill_words(part + (uint64_t)old * cs, ((uint64_t)labels_offset - old) * cs / 4, 0u, idx->stream));
    AddEncoder enc;
    uint32_t* d_size = nullptr;
    HIPCHECK(enc.mem.alloc(&d_size, 4));
    if (count) {
        if (int rc = enc.prepare(idx, count, sum_mode, d_side)) return rc;
        for (uint64_t o = 0; o < count; o += QADC_INDEX_ADD_CHUNK) {
            const uint64_t cnt = std::min<uint64_t>(QADC_INDEX_ADD_CHUNK, count - o);
            if (int rc = enc.encode(idx, vectors + o * idx->feed.dim, cnt, sum_mode, d_side)) return rc;
            HIPCHECK(launch_adc_copy_words(enc.d_codes, part + ((uint64_t)labels_offset + o) * cs, cnt * cs / 4, idx->stream));
        }
    }
    sizes[0] = size;
    HIPCHECK(idx->arena.h_add.ensure(4));
    return zero_tails(idx, sizes, idx->arena.h_add.p, d_size);
}

// labelled: the call is qadc_index_add_vectors_labelled / _device, which takes labels [count] and no labels_offset.
int add_vectors(qadc_index* idx, const float* vectors, const uint32_t* labels, bool labelled, uint64_t count, uint32_t labels_offset, int sum_mode,
                bool d_side, const char* call) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (int rc = refuse(idx, call)) return rc;
    const FeederState& f = idx->feed;
    if (labelled) {   // (the keys of a flat or unlabelled index are positions: it has no label to set)
        if (f.dim && !f.K)
            return fail(QADC_E_STATE, std::string(call) + ": a flat index (no coarse quantizer) keys its vectors by position and takes no labels");
        if (idx->labeled == 0 && std::any_of(idx->parts.begin(), idx->parts.end(), [](const Part& p) { return p.n != 0; }))
            return fail(QADC_E_STATE, std::string(call) + ": the index holds unlabelled partitions, whose keys are positions");
        if (count && !labels) return fail(QADC_E_ARG, "labels is null");
    }
    if (!f.dim) return fail(QADC_E_ARG, "qadc_index_set_pq has not been called: the index has no codebooks");
    if (f.dim > kPqEncodeMaxDim) return fail(QADC_E_ARG, "dim must be <= 2048 (the encoder keeps the codebooks in LDS)");
    if (sum_mode != 0 && sum_mode != 1) return fail(QADC_E_ARG, "sum_mode is 0 (source order) or 1 (as compiled)");
    if (count && !vectors) return fail(QADC_E_ARG, "vectors is null");
    if ((uint64_t)labels_offset + count > kAppendMaxRows)
        return fail(QADC_E_ARG, "labels_offset + count = " + std::to_string((uint64_t)labels_offset + count) + " exceeds 2^32 - 1");
    const size_t parts = idx->parts.size();
    const bool holds = std::any_of(idx->parts.begin(), idx->parts.end(), [](const Part& p) { return p.n != 0; });
    if (f.K) {
        if (parts != 0 && parts != (size_t)f.K)
            return fail(QADC_E_ARG, "the coarse quantizer has " + std::to_string(f.K) + " centroids and the index " + std::to_string(parts) + " partitions");
        if (idx->labeled == 0 && holds) return fail(QADC_E_ARG, "the index holds unlabelled partitions: vectors added through a coarse quantizer are labelled");
    } else {
        if (parts > 1) return fail(QADC_E_ARG, "a flat index (no coarse quantizer) has one partition: the index has " + std::to_string(parts));
        if (idx->labeled == 1 && holds) return fail(QADC_E_ARG, "the index is labelled: a flat index keys its vectors by position");
    }
    DeviceGuard guard;
    if (int rc = use_device(idx)) return rc;
    // what a failed call puts back: the rows of every partition (rows written behind them are not part of the database)
    std::vector<uint32_t> sizes0(parts);
    for (size_t p = 0; p < parts; ++p) sizes0[p] = idx->parts[p].n;
    const int labeled0 = idx->labeled;
    const bool fresh = parts == 0;
    if (fresh) {
        idx->parts.assign(f.K ? (size_t)f.K : 1, Part{});
        sizes0.assign(idx->parts.size(), 0);
    }
    std::vector<uint32_t> sizes = sizes0;
    if (f.K) {
        if (count) idx->labeled = 1;
    } else if (std::max<uint64_t>(sizes[0], (uint64_t)labels_offset + count)) {
        idx->labeled = 0;
    }
    bool moved = false;
    const int rc = f.K ? add_ivf(idx, sizes, vectors, labels, count, labels_offset, sum_mode, d_side, &moved)
                       : add_flat(idx, sizes, vectors, count, labels_offset, sum_mode, d_side, &moved);
    if (rc != QADC_OK) {
        const std::string msg = g_err;
        (void)hipStreamSynchronize(idx->stream);
        idx->labeled = labeled0;
        if (fresh) {   // the index held no partition: it holds none again
            idx->parts.clear();
            idx->arena.release();
        } else if (resident(idx)) {   // (a relocation of this call stands; its partitions hold the rows they held)
            bind_parts(idx, &sizes0);
            uint32_t* d_sizes = nullptr;
            Scratch mem;
            if (mem.alloc(&d_sizes, parts * 4) == hipSuccess && idx->arena.h_add.ensure(parts) == hipSuccess)
                (void)zero_tails(idx, sizes0, idx->arena.h_add.p, d_sizes);
        }
        g_err = msg;
        return rc;
    }
    bind_parts(idx, &sizes);
    if (moved) ++idx->arena.relocations;
    idx->finalized = false;
    return QADC_OK;
}

// Remove by label over Part::d_codes / d_labels, in the arena or in allocations of their own: nothing
// moves between regions, so neither the arena nor relocations() changes.  A call that removed a row leaves the index not
// finalized — the start sizes, the partition table and the byte-plane copies describe the old rows — with the zeroed span of
// alloc_part / index_padded_end behind every touched partition's new last row.
int remove_labels(qadc_index* idx, const uint32_t* list, uint64_t count, uint64_t* removed_out, bool d_side, const char* call) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (int rc = refuse(idx, call)) return rc;
    if (count && !list) return fail(QADC_E_ARG, std::string(call) + ": labels is null");
    const bool holds = std::any_of(idx->parts.begin(), idx->parts.end(), [](const Part& p) { return p.n != 0; });
    if (holds && idx->labeled != 1)
        return fail(QADC_E_ARG, std::string(call) + ": the index is not labelled: it keys its vectors by position, and a removal would renumber them");
    if (removed_out) *removed_out = 0;
    if (count == 0 || !holds) return QADC_OK;
    DeviceGuard guard;
    if (int rc = use_device(idx)) return rc;
    RemoveJob job;
    job.stream = idx->stream;
    job.code_size = idx->cs;
    job.zero_tail = true;
    job.pinned = &idx->arena.h_add;
    for (const Part& pt : idx->parts) {
        job.codes.push_back(pt.d_codes);
        job.labels.push_back(pt.d_labels);
        job.sizes.push_back(pt.n);
    }
    if (int rc = remove_rows(job, list, count, d_side)) {
        const std::string msg = g_err;
        (void)hipStreamSynchronize(idx->stream);
        if (job.wrote) idx->finalized = false;   // (the touched partitions' contents are unspecified: nothing recorded of them is scanned)
        g_err = msg;
        return rc;
    }
    if (job.plan.removed == 0) return QADC_OK;   // no row was hit: nothing was written, a finalized index stays finalized
    for (const RemoveEntry& e : job.plan.touched) {   // (as bind_parts sets them)
        Part& pt = idx->parts[e.part];
        pt.n = e.n_new;
        pt.global_n = pt.n;
        pt.starts_cap = pt.n;
    }
    idx->finalized = false;
    if (removed_out) *removed_out = job.plan.removed;
    return QADC_OK;
}

}  // namespace

extern "C" {

int qadc_index_remove_labels(qadc_index* idx, const uint32_t* labels, uint64_t count, uint64_t* removed_out) {
    return remove_labels(idx, labels, count, removed_out, false, "qadc_index_remove_labels");
}

int qadc_index_remove_labels_device(qadc_index* idx, const uint32_t* d_labels, uint64_t count, uint64_t* removed_out) {
    return remove_labels(idx, d_labels, count, removed_out, true, "qadc_index_remove_labels_device");
}

int qadc_index_add_vectors(qadc_index* idx, const float* vectors, uint64_t count, uint32_t labels_offset, int sum_mode) {
    return add_vectors(idx, vectors, nullptr, false, count, labels_offset, sum_mode, false, "qadc_index_add_vectors");
}

int qadc_index_add_vectors_device(qadc_index* idx, const float* d_vectors, uint64_t count, uint32_t labels_offset, int sum_mode) {
    return add_vectors(idx, d_vectors, nullptr, false, count, labels_offset, sum_mode, true, "qadc_index_add_vectors_device");
}

int qadc_index_add_vectors_labelled(qadc_index* idx, const float* vectors, const uint32_t* labels, uint64_t count, int sum_mode) {
    return add_vectors(idx, vectors, labels, true, count, 0, sum_mode, false, "qadc_index_add_vectors_labelled");
}

int qadc_index_add_vectors_labelled_device(qadc_index* idx, const float* d_vectors, const uint32_t* d_labels, uint64_t count, int sum_mode) {
    return add_vectors(idx, d_vectors, d_labels, true, count, 0, sum_mode, true, "qadc_index_add_vectors_labelled_device");
}

int qadc_index_read_partition(qadc_index* idx, int part, uint32_t first, uint32_t count, uint8_t* codes_out, uint32_t* labels_out) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (part < 0 || part >= (int)idx->parts.size())
        return fail(QADC_E_ARG, "partition " + std::to_string(part) + " does not exist (" + std::to_string(idx->parts.size()) + " partitions)");
    const Part& pt = idx->parts[part];
    if (pt.n != pt.global_n || pt.first_pos != 0) return fail(QADC_E_ARG, "partition " + std::to_string(part) + " is a shard: only a partition held whole is read");
    if ((uint64_t)first + count > pt.n)
        return fail(QADC_E_ARG, "rows [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + count) + ") are outside partition " +
                                    std::to_string(part) + " of " + std::to_string(pt.n) + " codes");
    if (!count) return QADC_OK;
    DeviceGuard guard;
    if (int rc = use_device(idx)) return rc;
    const size_t cs = (size_t)idx->cs;
    if (codes_out) HIPCHECK(hipMemcpyAsync(codes_out, pt.d_codes + first * cs, count * cs, hipMemcpyDeviceToHost, idx->stream));
    if (labels_out && idx->labeled == 1 && pt.d_labels)
        HIPCHECK(hipMemcpyAsync(labels_out, pt.d_labels + first, (size_t)count * 4, hipMemcpyDeviceToHost, idx->stream));
    HIPCHECK(hipStreamSynchronize(idx->stream));
    return QADC_OK;
}

int qadc_index_reserve(qadc_index* idx, int part_count, const uint32_t* capacities) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (int rc = refuse(idx, "qadc_index_reserve")) return rc;
    if (part_count < 0 || (part_count > 0 && !capacities)) return fail(QADC_E_ARG, "bad capacity array");
    DeviceGuard guard;
    if (int rc = use_device(idx)) return rc;
    const size_t before = idx->parts.size(), parts = std::max(before, (size_t)part_count);
    if (parts == 0) return QADC_OK;
    std::vector<uint32_t> floor(parts, 0), sizes(parts, 0), caps = current_caps(idx);
    std::copy(capacities, capacities + part_count, floor.begin());
    for (size_t p = 0; p < before; ++p) sizes[p] = idx->parts[p].n;
    caps.resize(parts, 0);
    const std::vector<uint64_t> add(parts, 0);
    const AppendPlan plan = plan_index_append(idx->cs, parts, sizes.data(), caps.data(), add.data(), floor.data(), false);
    if (!plan.refused.empty()) return fail(QADC_E_ARG, plan.refused);
    if (plan.in_place && parts == before && resident(idx)) return QADC_OK;
    idx->parts.resize(parts);
    const int rc = relocate(idx, plan, sizes, idx->labeled == 1);
    if (rc != QADC_OK) idx->parts.resize(before);
    return rc;
}

uint64_t qadc_index_relocations(const qadc_index* idx) { return idx ? idx->arena.relocations : 0; }

}  // extern "C"
