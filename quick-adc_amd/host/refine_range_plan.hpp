// Launch geometry of the exact range search over a refine store (qadc_refine_range, qadc_refine_rerank_range;
// csrc/qadc_refine_range_kernel.hip) — HIP-free, so that tests/cpp/refine_range_plan_host.cpp can check it
// on the CPU.  The launches of csrc/qadc_refine.cpp do exactly what this plan says.
//
// Exhaustive form.  A call runs in `passes` of at most pass_nq whole queries.  A pass is cut into tiles of `qt` queries, kept in
// registers or in LDS exactly as the exhaustive k-NN keeps them (refine_knn_plan.hpp: knn_plan's qt and jregs), and the rows [0, rows) are walked
// in `launches` launches of groups * chunk_rows rows: row r of launch L lies at o = r - L * groups * chunk_rows, in group
// o / chunk_rows and in slice (o % chunk_rows) / slice_rows — knn_launch_groups() and knn_slice() of refine_knn_plan.hpp give the
// live groups of a launch and the rows of (launch, group, slice).  The grid of a pass of n queries is (ceil(n / qt),
// groups_of(launch) * slices) workgroups of kKnnWaves waves.
//
// Regions.  Every query of a pass owns a region of cap[q] words at base[q] = the sum of the caps before it, and a counter.  A kept
// row's word is appended through the counter; a word beyond cap[q] is counted and not written.  The first run of a pass gives every
// query region_rows words (default min(rows, kRangeDefaultRegion)); where a counter passed its cap the pass runs a second time with
// cap[q] = the counted size of every query (range_rerun).  The words of one run are at most kRangeMaxEntries (range_regions).
//
// Candidate form.  The candidates keys[in_lims[q] .. in_lims[q + 1]) are flattened: a pass is a run of whole queries
// (range_cand_passes: at most pass_nq queries and, unless one query alone has more, kRangePassCands candidates), the region of a
// query is its segment, and a workgroup owns a chunk of at most cands_per_wg candidates of one segment (range_cand_chunks): wave w
// takes kRefineInFlight candidates side by side, as refine_dist_kernel does.  A segment of no candidates has no chunk.
//
// Sort and compact.  One workgroup of kRangeSortThreads threads per query: a region of at most kRangeSortLds words is sorted in LDS,
// a longer one by radix passes between the region and a scratch of the same size; it leaves the region sorted and the number of
// survivors (words that are not ~0 and differ from the word before them).  The scratch is range_scratch_entries words.  The host sums
// the survivors into the offsets of the held result — at most kRangeMaxEntries rows for a whole call (range_held_fits) — and the
// compact kernel, one workgroup per query, writes them there.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "refine_knn_plan.hpp"

namespace qadc {
namespace refine {

constexpr uint64_t kRangeMaxEntries = 1ull << 31;      // = QADC_REFINE_RANGE_MAX_ENTRIES (asserted where both are seen)
constexpr uint64_t kRangeDefaultRegion = 4096;         // words of a query's region in the first run of a pass
constexpr int kRangeSortLds = 4096;                    // = QADC_REFINE_RANGE_SORT_LDS: longer regions take the radix passes
constexpr int kRangeSortThreads = 256;                 // one radix digit per thread
constexpr uint64_t kRangeDefaultChunk = kKnnDefaultChunk;   // rows of a group per launch: the k-NN's, so that the walk is the same
constexpr uint64_t kRangeMaxChunk = 1ull << 24;
constexpr uint64_t kRangeScratchBytes = 256ull << 20;  // the default pass keeps the first run's regions within this
constexpr uint64_t kRangePassCands = 1ull << 24;       // candidates of a pass of the candidate form (128 MiB of words)
constexpr uint64_t kRangeNoLimit = 0;                  // the limit word of a query that keeps nothing

struct RangePlan {
    int qt, jregs;          // the tile, as KnnPlan's
    size_t dist_lds_bytes;
    int pass_nq, passes;
    uint64_t region_rows;   // words of a query's region in the first run
    uint64_t chunk_rows;
    int groups, slice_rows, slices;
    uint64_t launches;
};

// The limit word of a radius: a row is kept where its word (bits(D) << 32 | key) is below it.  D is +0, positive or NaN, so for a
// radius that is positive and not NaN "bits(D) < bits(radius)" is "D < radius" (a NaN's image lies above +inf's); every other
// radius — NaN, zero of either sign, negative — keeps nothing.  Decided on the bits, not by a float compare: the calling thread may
// run with subnormals treated as zero ("The host's floating-point mode"), and a subnormal radius is positive.
inline uint64_t range_limit_word(float radius) {
    uint32_t u;
    std::memcpy(&u, &radius, 4);
    const bool positive = u != 0u && u <= 0x7F800000u;   // sign clear, not zero, not NaN: +subnormal .. +inf
    return positive ? (uint64_t)u << 32 : kRangeNoLimit;
}

// region_rows / chunk_rows / pass_nq 0: the plan's default.  false: a shape the kernels do not take.
inline bool range_plan(int nq, uint64_t rows, int dim, uint64_t region_rows, uint64_t chunk_rows, int pass_nq, RangePlan* p) {
    if (nq <= 0 || dim <= 0 || dim > kRefinePlanMaxDim || pass_nq < 0 || chunk_rows > kRangeMaxChunk) return false;
    KnnPlan k;
    if (!knn_plan(nq, rows, dim, 0, 1, 0, 0, &k)) return false;   // (the tile depends on nq and dim alone)
    p->qt = k.qt;
    p->jregs = k.jregs;
    p->dist_lds_bytes = k.dist_lds_bytes;
    if (chunk_rows == 0) chunk_rows = kRangeDefaultChunk;
    if (region_rows == 0) region_rows = kRangeDefaultRegion;
    region_rows = std::max<uint64_t>(1, std::min(region_rows, rows));   // (a query keeps at most `rows` rows)
    p->region_rows = region_rows;
    p->chunk_rows = chunk_rows;
    p->groups = kKnnMaxGroups;
    if (pass_nq == 0) pass_nq = (int)std::max<uint64_t>(1, std::min<uint64_t>(1u << 30, kRangeScratchBytes / (region_rows * 8)));
    p->pass_nq = std::min(nq, pass_nq);
    p->passes = (nq + p->pass_nq - 1) / p->pass_nq;
    p->launches = (rows + (uint64_t)p->groups * chunk_rows - 1) / ((uint64_t)p->groups * chunk_rows);
    const int64_t tiles = (p->pass_nq + p->qt - 1) / p->qt;
    const int64_t live_groups = (int64_t)std::min<uint64_t>((uint64_t)p->groups, std::max<uint64_t>(1, (rows + chunk_rows - 1) / chunk_rows));
    int slice = kKnnMaxSlice;
    while (slice > kKnnMinSlice && tiles * live_groups * (int64_t)((chunk_rows + slice - 1) / slice) < kKnnWgFloor) slice /= 2;
    p->slice_rows = slice;
    p->slices = (int)((chunk_rows + slice - 1) / slice);
    return true;
}

// base[q] = the sum of cap[0 .. q), *entries = the sum of all.  false: more than max_entries words (nothing is to be allocated).
inline bool range_regions(const uint64_t* cap, int n, uint64_t max_entries, uint64_t* base, uint64_t* entries) {
    uint64_t at = 0;
    for (int q = 0; q < n; ++q) {
        base[q] = at;
        if (cap[q] > max_entries || at + cap[q] > max_entries) return false;
        at += cap[q];
    }
    *entries = at;
    return true;
}

// Where a counter passed its cap: true, and every cap becomes exactly the counted size (the second run's regions).
inline bool range_rerun(uint64_t* cap, const uint64_t* count, int n) {
    bool over = false;
    for (int q = 0; q < n; ++q) over = over || count[q] > cap[q];
    if (over) std::copy(count, count + n, cap);
    return over;
}

// Words of the radix passes' scratch a run of `entries` words needs, its longest region holding `longest`: as many as the regions
// where one of them exceeds kRangeSortLds (a region's scratch lies at the region's own offset), none where every region sorts in LDS.
inline uint64_t range_scratch_entries(uint64_t entries, uint64_t longest) { return longest > (uint64_t)kRangeSortLds ? entries : 0; }

// The held result: `held` rows of the passes before, `kept` more of this one.  false: the call's result would exceed max_entries
// rows (nothing is to be allocated for them).
inline bool range_held_fits(uint64_t held, uint64_t kept, uint64_t max_entries) { return held <= max_entries && kept <= max_entries - held; }

// in_lims [nq + 1] is monotone from 0
inline bool range_in_lims_ok(const uint64_t* in_lims, int nq) {
    if (in_lims[0] != 0) return false;
    for (int q = 0; q < nq; ++q)
        if (in_lims[q + 1] < in_lims[q]) return false;
    return true;
}

struct RangeCandPass {
    int q0, q1;             // the queries [q0, q1)
};

// The passes of the candidate form: whole queries in order, a pass closed at pass_nq queries (0: no such limit) or before the
// query that would take it past kRangePassCands candidates (a pass holds one query at least).  false: one pass — one query — has
// more than max_entries candidates.
inline bool range_cand_passes(const uint64_t* in_lims, int nq, int pass_nq, uint64_t max_entries, std::vector<RangeCandPass>* out) {
    out->clear();
    const uint64_t most = std::min(kRangePassCands, max_entries);
    for (int q = 0; q < nq;) {
        int e = q + 1;
        while (e < nq && (pass_nq == 0 || e - q < pass_nq) && in_lims[e + 1] - in_lims[q] <= most) ++e;
        if (in_lims[e] - in_lims[q] > max_entries) return false;
        out->push_back(RangeCandPass{q, e});
        q = e;
    }
    return true;
}

struct RangeChunk {
    uint32_t q;             // the query, counted from the pass's first
    uint32_t first;         // the chunk's first candidate, counted from the pass's first
    uint32_t count;         // 1 .. cands_per_wg
};

// candidates of a workgroup: kRefineMaxCandsPerWg, cut finer while the pass has fewer than kRefineWgFloor workgroups
inline int range_cands_per_wg(const uint64_t* in_lims, int q0, int q1) {
    int cpw = kRefineMaxCandsPerWg;
    for (; cpw > kRefineInFlight; cpw /= 2) {
        uint64_t chunks = 0;
        for (int q = q0; q < q1 && chunks < (uint64_t)kRefineWgFloor; ++q) chunks += (in_lims[q + 1] - in_lims[q] + cpw - 1) / cpw;
        if (chunks >= (uint64_t)kRefineWgFloor) break;
    }
    return cpw;
}

// The chunk table of the pass [q0, q1): every candidate of every segment in exactly one chunk, chunks in order.
inline void range_cand_chunks(const uint64_t* in_lims, int q0, int q1, int cands_per_wg, std::vector<RangeChunk>* out) {
    out->clear();
    for (int q = q0; q < q1; ++q)
        for (uint64_t c = in_lims[q]; c < in_lims[q + 1]; c += (uint64_t)cands_per_wg)
            out->push_back(RangeChunk{(uint32_t)(q - q0), (uint32_t)(c - in_lims[q0]),
                                      (uint32_t)std::min<uint64_t>((uint64_t)cands_per_wg, in_lims[q + 1] - c)});
}

// What the entry points refuse before the device is touched (QADC_E_ARG): the reason, or null.  device arrays: checked for 4-byte
// alignment by the caller.
inline const char* range_refusal(bool store, int nq, bool queries, bool radius, bool lims) {
    if (!store) return "store is null";
    if (nq < 0) return "nq is negative";
    if (nq > 0 && (!queries || !radius || !lims)) return "queries, radius and lims must not be null";
    return nullptr;
}

inline const char* rerank_range_refusal(bool store, int nq, bool queries, const uint64_t* in_lims, bool keys, bool radius, bool lims) {
    if (const char* why = range_refusal(store, nq, queries, radius, lims)) return why;
    if (nq > 0 && !in_lims) return "in_lims must not be null";
    if (nq > 0 && !range_in_lims_ok(in_lims, nq)) return "in_lims must start at 0 and must not decrease";
    if (nq > 0 && in_lims[nq] > 0 && !keys) return "keys must not be null";
    return nullptr;
}

inline const char* range_plan_refusal(bool store, uint64_t chunk_rows, int pass_nq) {
    if (!store) return "store is null";
    if (chunk_rows > kRangeMaxChunk) return "chunk_rows is at most 2^24";
    if (pass_nq < 0) return "pass_nq is negative";
    return nullptr;
}

}  // namespace refine
}  // namespace qadc
