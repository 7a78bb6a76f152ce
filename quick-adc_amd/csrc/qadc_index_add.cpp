// db_add on the 4-bit index: qadc_index_add_vectors / _add_vectors_device encode vectors with the
// quantizers the index holds (FeederState) and append the codes to partitions that grow in device memory; qadc_index_reserve,
// _read_partition and _relocations complete the set, and qadc_index_remove_labels (section 11.7) takes rows out again.
// index_db::add_vectors (databases.hpp:270-298) with a coarse quantizer, flat_db::add_vectors (136-156) without.
//
// The flow — passes, room, relocation, rollback — is the one of csrc/qadc_append.h, shared with the float-ADC engine, over the
// index's RowStore (the arena, csrc/qadc_host.h; region_pad kIndexRegionPad).  This file holds what only the 4-bit index has: what
// a growing call refuses (busy slots, live views, shards, borrowed partitions), partitions that are still allocations of their own
// and move into the arena on the first growing call (launch_index_move over an IndexMove table, then freed), the Part table bound
// to the arena's regions, and the encoder's last step (launch_pq_encode, the chain of qadc_ivf_encode_host_mode(encode_form = 1)).
#include "qadc_host.h"

#include "../host/index_append_plan.hpp"
#include "qadc_adc_kernels.h"
#include "qadc_append.h"
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

// The partitions' pointers from the arena's tables; their sizes where `sizes` is given.
void bind_parts(qadc_index* idx, const std::vector<uint32_t>* sizes) {
    RowStore& a = idx->arena;
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

// The move step of a relocation: every partition from where it lies — an allocation of its own, or the old arena — into its region
// of the new one, by one kernel over an IndexMove table.
int move_parts(const qadc_index* idx, const Relocation& r) {
    const size_t parts = r.plan.cap.size();
    if (!parts) return QADC_OK;
    r.h_tmp.resize(parts * sizeof(IndexMove));   // (the table is read by an asynchronous copy)
    IndexMove* moves = reinterpret_cast<IndexMove*>(r.h_tmp.data());
    uint32_t longest = 0;
    for (size_t p = 0; p < parts; ++p) {
        const Part& pt = idx->parts[p];
        const bool move_labels = r.labels && r.sizes[p] && pt.d_labels && idx->labeled == 1;
        moves[p] = IndexMove{r.sizes[p] ? pt.d_codes : nullptr, r.codes + r.plan.off[p], move_labels ? pt.d_labels : nullptr,
                             move_labels ? r.labels + r.plan.lab_off[p] : nullptr, r.sizes[p], 0};
        longest = std::max(longest, r.sizes[p]);
    }
    IndexMove* d_moves = nullptr;
    HIPCHECK(r.tmp.alloc(&d_moves, parts * sizeof(IndexMove)));
    HIPCHECK(hipMemcpyAsync(d_moves, moves, parts * sizeof(IndexMove), hipMemcpyHostToDevice, idx->stream));
    HIPCHECK(launch_index_move(d_moves, (int)parts, idx->cs, longest, idx->stream));
    return QADC_OK;
}

// The index as the shared flow takes it.  sum_mode: the call's (the centroids' norms are computed per call under it).
AppendJob make_job(qadc_index* idx, int sum_mode) {
    const FeederState& f = idx->feed;
    AppendJob job;
    job.store = &idx->arena;
    job.stream = idx->stream;
    job.device = idx->device;
    job.labeled = &idx->labeled;
    job.finalized = &idx->finalized;
    for (const Part& pt : idx->parts) job.sizes.push_back(pt.n);
    job.dim = f.dim;
    job.K = f.K;
    job.max_dim = kPqEncodeMaxDim;
    job.set_pq = "qadc_index_set_pq";
    job.d_coarse = f.d_coarse.p;
    job.d_rotation = f.has_rotation ? f.d_rotation.p : nullptr;
    job.resident = [idx]() { return resident(idx); };
    job.move = [idx](const Relocation& r) { return move_parts(idx, r); };
    job.rebind = [idx]() {   // the partitions' own allocations are the old storage
        for (Part& pt : idx->parts)
            if (!pt.arena) {
                if (pt.d_codes) (void)hipFree(pt.d_codes);
                if (pt.d_labels) (void)hipFree(pt.d_labels);
            }
        bind_parts(idx, nullptr);
    };
    job.set_sizes = [idx](const std::vector<uint32_t>& sizes) {
        idx->parts.resize(sizes.size());
        if (resident(idx)) bind_parts(idx, &sizes);
    };
    job.encode = [idx, sum_mode](AddEncoder& enc, const float* d_enc, uint64_t cnt) {
        launch_pq_encode(d_enc, cnt, idx->M, idx->feed.dim, idx->feed.d_codebooks.p, 1, sum_mode, enc.d_codes, idx->stream);
        HIPCHECK(hipGetLastError());
        return QADC_OK;
    };
    return job;
}

// labelled: the call is qadc_index_add_vectors_labelled / _device, which takes labels [count] and no labels_offset.
int add_vectors(qadc_index* idx, const float* vectors, const uint32_t* labels, bool labelled, uint64_t count, uint32_t labels_offset, int sum_mode,
                bool d_side, const char* call) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (int rc = refuse(idx, call)) return rc;
    AppendJob job = make_job(idx, sum_mode);
    return append_vectors(job, vectors, labels, labelled, count, labels_offset, sum_mode, d_side, call);
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
    if (int rc = check_aligned(d_labels, 4, "d_labels")) return rc;
    return remove_labels(idx, d_labels, count, removed_out, true, "qadc_index_remove_labels_device");
}

int qadc_index_add_vectors(qadc_index* idx, const float* vectors, uint64_t count, uint32_t labels_offset, int sum_mode) {
    return add_vectors(idx, vectors, nullptr, false, count, labels_offset, sum_mode, false, "qadc_index_add_vectors");
}

int qadc_index_add_vectors_device(qadc_index* idx, const float* d_vectors, uint64_t count, uint32_t labels_offset, int sum_mode) {
    if (int rc = check_aligned(d_vectors, 4, "d_vectors")) return rc;   // (every kernel of the 4-bit encoder reads single floats)
    return add_vectors(idx, d_vectors, nullptr, false, count, labels_offset, sum_mode, true, "qadc_index_add_vectors_device");
}

int qadc_index_add_vectors_labelled(qadc_index* idx, const float* vectors, const uint32_t* labels, uint64_t count, int sum_mode) {
    return add_vectors(idx, vectors, labels, true, count, 0, sum_mode, false, "qadc_index_add_vectors_labelled");
}

int qadc_index_add_vectors_labelled_device(qadc_index* idx, const float* d_vectors, const uint32_t* d_labels, uint64_t count, int sum_mode) {
    if (int rc = check_aligned(d_vectors, 4, "d_vectors")) return rc;
    if (int rc = check_aligned(d_labels, 4, "d_labels")) return rc;
    return add_vectors(idx, d_vectors, d_labels, true, count, 0, sum_mode, true, "qadc_index_add_vectors_labelled_device");
}

int qadc_index_read_partition(qadc_index* idx, int part, uint32_t first, uint32_t count, uint8_t* codes_out, uint32_t* labels_out) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    const AppendJob job = make_job(idx, 1);
    const Part* pt = part >= 0 && part < (int)idx->parts.size() ? &idx->parts[part] : nullptr;
    if (pt && (pt->n != pt->global_n || pt->first_pos != 0))
        return fail(QADC_E_ARG, "partition " + std::to_string(part) + " is a shard: only a partition held whole is read");
    return read_rows(job, part, first, count, pt ? pt->d_codes : nullptr, pt && idx->labeled == 1 ? pt->d_labels : nullptr, codes_out, labels_out);
}

int qadc_index_reserve(qadc_index* idx, int part_count, const uint32_t* capacities) {
    if (!idx) return fail(QADC_E_ARG, "index is null");
    if (int rc = refuse(idx, "qadc_index_reserve")) return rc;
    AppendJob job = make_job(idx, 1);
    return reserve_rows(job, part_count, capacities);
}

uint64_t qadc_index_relocations(const qadc_index* idx) { return idx ? idx->arena.relocations : 0; }

}  // extern "C"
