// Launch geometry of the probed exact search over a refine store (qadc_refine_knn_probed; csrc/qadc_refine_probe_kernel.hip;
// DESIGN.md section 11.22) — HIP-free and pure, so that tests/cpp/refine_probe_plan_host.cpp can check it on the CPU.  The launches of
// csrc/qadc_refine.cpp do exactly what this plan says.
//
// Queries.  A call runs in passes of at most pass_nq whole queries (refine_knn_plan.hpp's rule and scratch bound).  qt, jregs and the
// LDS mode of a tile are knn_plan's.
//
// Work.  probe_work inverts a pass's probe lists: for every partition that holds rows and is probed, the queries that probe it, cut
// into tiles of at most qt (the last tile of a partition is short).  An item is (partition, tile); each query of a tile carries the
// slot query * groups + group its words go to.  Probe j of a query — the first occurrence of a partition in its list; repeats and
// numbers outside [0, partitions) give nothing — goes to group j % groups, so at most per_group = ceil(ma / groups) probes of a query
// share a (query, group) buffer.  The items are ordered by their partition's rows, longest first.
//
// Rows.  Launch L walks the rows [L * launch_rows, (L + 1) * launch_rows) of every partition, launch_rows = chunk_rows / per_group
// (0: refused), so between two selects a (query, group) buffer is offered at most per_group * launch_rows <= chunk_rows rows: the
// invariant knn's selection rests on (buf_cap = R + chunk_rows).  The grid of launch L is (items whose partition holds more than
// L * launch_rows rows — a prefix of the item list —, slices of slice_rows rows, 1): workgroup (i, s) takes the rows
// [L * launch_rows + s * slice_rows, ... + slice_rows) of item i's partition that lie in the launch and in the partition
// (probe_slice); wave w of it the rows first + w, first + w + kKnnWaves, ...  So every (query, probed partition, row) lies in exactly
// one (launch, item, wave slot), grid.y <= launch_rows / kKnnMinSlice + 1 <= 65535, and the scratch (buffers, counters, bounds,
// items and slots) depends on pass_nq, ma, R and chunk_rows alone, not on the rows.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "refine_knn_plan.hpp"

namespace qadc {
namespace refine {

struct ProbePlan {
    int qt, jregs;
    size_t dist_lds_bytes;
    int pass_nq, passes;
    uint64_t chunk_rows;
    int groups;             // (query, group) buffers per query: at most kKnnMaxGroups, kKnnMaxSort / R and ma
    int per_group;          // ceil(ma / groups)
    uint64_t launch_rows;   // rows of a partition per launch: chunk_rows / per_group >= 1
    uint64_t buf_cap;       // R + chunk_rows <= kKnnMaxSort
    int mid_sort_n, final_sort_n, select_threads;
    size_t select_lds_bytes;
    uint64_t scratch_bytes; // buffers, counters, bounds, items and slots of a pass
};

struct ProbeItem {
    uint32_t part;          // the partition
    uint32_t rows;          // rows it holds
    uint32_t first, count;  // the tile: slots[first .. first + count), 1 <= count <= qt
};

// The work of one pass
struct ProbeWork {
    std::vector<ProbeItem> items;          // by rows descending (ties: partition, then tile, ascending)
    std::vector<uint32_t> slots;           // query of the pass * groups + group
    int slice_rows = kKnnMaxSlice;
    uint64_t launches = 0;                 // ceil(rows of the longest probed partition / launch_rows)
    std::vector<uint32_t> launch_items;    // [launches] grid.x of launch L
    std::vector<uint32_t> launch_slices;   // [launches] grid.y of launch L
};

// the rows [*first, *last) of (launch, slice) in a partition of `rows` rows; empty where first >= last
QADC_KNN_HD inline void probe_slice(uint32_t rows, uint64_t launch_rows, int slice_rows, uint64_t launch, uint32_t slice, uint64_t* first,
                                    uint64_t* last) {
    const uint64_t c0 = launch * launch_rows;
    uint64_t c1 = c0 + launch_rows;
    if (c1 > rows) c1 = rows;
    const uint64_t f = c0 + (uint64_t)slice * (uint64_t)slice_rows;
    uint64_t l = f + (uint64_t)slice_rows;
    if (l > c1) l = c1;
    *first = f;
    *last = l;
}

// chunk_rows / pass_nq 0: the plan's default.  false: a shape the kernels do not take (the caller refuses it).
inline bool probe_plan(int nq, int ma, int dim, int R, uint64_t chunk_rows, int pass_nq, ProbePlan* p) {
    if (nq <= 0 || ma < 1 || R < 1 || R > kKnnMaxR) return false;
    KnnPlan k;
    if (!knn_plan(nq, 0, dim, 0, R, chunk_rows, pass_nq, &k)) return false;
    p->qt = k.qt;
    p->jregs = k.jregs;
    p->dist_lds_bytes = k.dist_lds_bytes;
    p->chunk_rows = k.chunk_rows;
    p->groups = std::min(k.groups, ma);
    p->per_group = (ma + p->groups - 1) / p->groups;
    p->launch_rows = k.chunk_rows / (uint64_t)p->per_group;
    if (p->launch_rows == 0) return false;
    p->buf_cap = k.buf_cap;
    p->mid_sort_n = k.mid_sort_n;
    p->final_sort_n = knn_pow2_at_least((uint64_t)p->groups * R);
    const int sort_n = std::max(p->mid_sort_n, p->final_sort_n);
    p->select_threads = std::min(1024, std::max(64, sort_n / 2));
    p->select_lds_bytes = (size_t)sort_n * sizeof(uint64_t);
    // per query: the groups' buffers, counters and bounds; an item and a slot per probe at most
    const uint64_t per_query = (uint64_t)p->groups * (p->buf_cap * 8 + 4 + 8) + (uint64_t)ma * (sizeof(ProbeItem) + 4);
    if (pass_nq == 0) pass_nq = (int)std::max<uint64_t>(1, kKnnScratchBytes / per_query);
    p->pass_nq = std::min(nq, pass_nq);
    p->passes = (nq + p->pass_nq - 1) / p->pass_nq;
    p->scratch_bytes = (uint64_t)p->pass_nq * per_query;
    return p->select_lds_bytes <= kRefineLdsDefault;
}

// The work of the pass over the queries whose probe lists are assign [nq][ma]; part_rows [parts].
inline void probe_work(const ProbePlan& plan, int nq, int ma, const int32_t* assign, const uint32_t* part_rows, int parts, ProbeWork* w) {
    // per partition the slots of the queries that probe it, in query order
    std::vector<uint32_t> count((size_t)parts + 1, 0);
    std::vector<int32_t> seen((size_t)parts, -1);   // the last query that listed the partition
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            uint32_t at = 0;
            for (int p = 0; p <= parts; ++p) {
                const uint32_t c = count[p];
                count[p] = at;
                at += c;
            }
            w->slots.assign(at, 0);
            std::fill(seen.begin(), seen.end(), -1);
        }
        for (int q = 0; q < nq; ++q)
            for (int j = 0; j < ma; ++j) {
                const int32_t p = assign[(size_t)q * ma + j];
                if (p < 0 || p >= parts || seen[p] == q) continue;
                seen[p] = q;
                if (part_rows[p] == 0) continue;
                if (pass == 0) ++count[p];
                else w->slots[count[p]++] = (uint32_t)q * (uint32_t)plan.groups + (uint32_t)(j % plan.groups);
            }
    }
    // (after the second pass count[p] is the end of partition p's slots; its start is the end of the one before it)
    std::vector<int> order;
    for (int p = 0; p < parts; ++p)
        if (count[p] > (p ? count[p - 1] : 0u)) order.push_back(p);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return part_rows[a] > part_rows[b]; });
    w->items.clear();
    for (int p : order) {
        const uint32_t begin = p ? count[p - 1] : 0u, end = count[p];
        for (uint32_t f = begin; f < end; f += (uint32_t)plan.qt)
            w->items.push_back(ProbeItem{(uint32_t)p, part_rows[p], f, std::min<uint32_t>((uint32_t)plan.qt, end - f)});
    }
    const uint64_t longest = w->items.empty() ? 0 : w->items[0].rows;
    w->launches = (longest + plan.launch_rows - 1) / plan.launch_rows;
    const uint64_t walk = std::min<uint64_t>(plan.launch_rows, std::max<uint64_t>(longest, 1));
    int slice = kKnnMaxSlice;
    while (slice > kKnnMinSlice && (uint64_t)w->items.size() * ((walk + slice - 1) / slice) < (uint64_t)kKnnWgFloor) slice /= 2;
    w->slice_rows = slice;
    w->launch_items.assign((size_t)w->launches, 0);
    w->launch_slices.assign((size_t)w->launches, 0);
    size_t live = w->items.size();
    for (uint64_t L = 0; L < w->launches; ++L) {
        while (live > 0 && (uint64_t)w->items[live - 1].rows <= L * plan.launch_rows) --live;
        const uint64_t rows = std::min<uint64_t>(plan.launch_rows, longest - L * plan.launch_rows);
        w->launch_items[(size_t)L] = (uint32_t)live;
        w->launch_slices[(size_t)L] = (uint32_t)((rows + slice - 1) / slice);
    }
}

}  // namespace refine
}  // namespace qadc
