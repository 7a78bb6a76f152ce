// Launch geometry of the exhaustive search over a refine store (qadc_refine_knn; csrc/qadc_refine_knn_kernel.hip; DESIGN.md section
// 11.16) — HIP-free, so that tests/cpp/refine_knn_plan_host.cpp can check it on the CPU.  The launches of csrc/qadc_refine.cpp do
// exactly what this plan says.
//
// Queries.  A call runs in `passes` of at most pass_nq whole queries, so that the scratch stays bounded; a pass is cut into tiles
// of `qt` queries (the last tile of a pass may be short).  Lane l of a wave keeps the components 64 j + l of every query of its
// tile: in registers (jregs = ceil(dim / 64) > 0) where qt * jregs fits kKnnRegBudget VGPRs, else in LDS (jregs = 0) with qt cut so
// that qt * dim floats fit kKnnTileLdsBytes.  Calls of at most kKnnSmallNq queries take tiles of kKnnSmallQt.
//
// Rows.  The rows [0, rows) — of a keyed store: the rows allocated so far, free ones skipped by the kernel — are walked in
// `launches` launches of groups * chunk_rows rows.  Row r of launch L lies at o = r - L * groups * chunk_rows, in group
// o / chunk_rows and in slice (o % chunk_rows) / slice_rows of that group's chunk: knn_slice() gives the rows of (launch, group,
// slice).  (More groups per launch for a call of few queries were tried, 32 for 8: fewer launches, but every wave then walks four
// times the rows one after the other, and a lone query over 10^6 rows went from 1.13 ms to 1.74 ms.)
// The distance grid of a pass of n queries is (ceil(n / qt), groups_of(launch) * slices) workgroups of kKnnWaves waves; wave w
// takes the rows first + w, first + w + kKnnWaves, ... of its slice.
//
// Selection.  Every (query, group) has a buffer of buf_cap = R + chunk_rows words, a counter and a bound word (~0 at first).  The
// distance kernel appends the words <= the bound; after each launch the select kernel, one workgroup per (query, group), sorts a
// buffer that holds at least R words (sort size: the power of two >= its count, at most mid_sort_n), keeps the first R and lowers
// the bound to the R-th.  The final select, one workgroup per query, sorts the groups' lists (at most groups * R <= final_sort_n
// words) and writes the outputs.  Both sort in LDS with select_threads threads.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "refine_plan.hpp"

#if defined(__HIPCC__)
#define QADC_KNN_HD __host__ __device__
#else
#define QADC_KNN_HD
#endif

namespace qadc {
namespace refine {

constexpr int kKnnMaxR = 1024;                       // = QADC_REFINE_KNN_MAX_R (asserted where both are seen)
constexpr int kKnnMaxSort = 8192;                    // words of the largest sort: kRefinePlanMaxIn, refine_select_kernel's
constexpr int kKnnWaves = 4;                         // waves of a distance workgroup (256 threads)
constexpr int kKnnRegBudget = 64;                    // VGPRs a lane spends on its tile's query components
constexpr int kKnnMaxQt = 32;
constexpr int kKnnSmallNq = 4, kKnnSmallQt = 4;      // a call of a few queries: small tiles, less idle arithmetic per row
constexpr int kKnnMaxJregs = 4;                      // register tiles up to dim 256
constexpr size_t kKnnTileLdsBytes = 64 * 1024;       // an LDS tile: qt * dim floats (= kRefineLdsDefault: no raised limit)
constexpr uint64_t kKnnDefaultChunk = kKnnMaxSort - kKnnMaxR;   // 7168: R + chunk_rows <= 8192 whatever R
constexpr int kKnnMaxGroups = 8;
constexpr int kKnnMaxSlice = 512, kKnnMinSlice = 16; // rows of a distance workgroup
constexpr int kKnnWgFloor = 1024;                    // fewer distance workgroups than this: the chunks are cut finer
constexpr uint64_t kKnnScratchBytes = 256ull << 20;  // the default pass keeps the buffers within this

struct KnnPlan {
    int qt;                 // queries of a tile: a power of two <= kKnnMaxQt
    int jregs;              // ceil(dim / 64) where the tile lives in registers, 0 where it lives in LDS
    size_t dist_lds_bytes;  // dynamic LDS of the distance kernel: qt * dim floats in LDS mode, else 0
    int pass_nq, passes;
    uint64_t chunk_rows;    // rows of a group per launch
    int groups;             // row groups in flight per launch: groups * R <= kKnnMaxSort, at most kKnnMaxGroups
    int slice_rows, slices; // slices = ceil(chunk_rows / slice_rows) per group
    uint64_t launches;      // ceil(rows / (groups * chunk_rows))
    uint64_t buf_cap;       // words of a (query, group) buffer: R + chunk_rows <= kKnnMaxSort
    int mid_sort_n;         // the power of two >= buf_cap
    int final_sort_n;       // the power of two >= groups * R
    int select_threads;
    size_t select_lds_bytes;   // max(mid_sort_n, final_sort_n) words
    uint64_t scratch_bytes; // buffers, counters and bounds of a pass: independent of rows
};

inline int knn_pow2_at_least(uint64_t n) {
    int p = 64;
    while ((uint64_t)p < n) p <<= 1;
    return p;
}

// groups of launch L (the last launch may have fewer)
QADC_KNN_HD inline int knn_launch_groups(uint64_t rows, uint64_t chunk_rows, int groups, uint64_t launch) {
    const uint64_t first = launch * (uint64_t)groups * chunk_rows;
    if (first >= rows) return 0;
    const uint64_t left = rows - first, g = (left + chunk_rows - 1) / chunk_rows;
    return g < (uint64_t)groups ? (int)g : groups;
}

// the rows [*first, *last) of (launch, group, slice); empty where first >= last
QADC_KNN_HD inline void knn_slice(uint64_t rows, uint64_t chunk_rows, int groups, int slice_rows, uint64_t launch, int group, int slice,
                                  uint64_t* first, uint64_t* last) {
    const uint64_t c0 = (launch * (uint64_t)groups + (uint64_t)group) * chunk_rows;
    uint64_t c1 = c0 + chunk_rows;
    if (c1 > rows) c1 = rows;
    const uint64_t f = c0 + (uint64_t)slice * (uint64_t)slice_rows;
    uint64_t l = f + (uint64_t)slice_rows;
    if (l > c1) l = c1;
    *first = f;
    *last = l;
}

// chunk_rows / pass_nq 0: the plan's default.  false: a shape the kernels do not take (the caller refuses it).
inline bool knn_plan(int nq, uint64_t rows, int dim, int dtype, int R, uint64_t chunk_rows, int pass_nq, KnnPlan* p) {
    (void)dtype;   // (both element types take the same geometry: a row is read once per tile whatever its width)
    if (nq <= 0 || dim <= 0 || dim > kRefinePlanMaxDim || R < 1 || R > kKnnMaxR || pass_nq < 0) return false;
    if (chunk_rows == 0) chunk_rows = kKnnDefaultChunk;
    if (chunk_rows + (uint64_t)R > (uint64_t)kKnnMaxSort) return false;
    const int j = (dim + 63) / 64;
    int qt = nq <= kKnnSmallNq ? kKnnSmallQt : kKnnMaxQt;
    if (j <= kKnnMaxJregs) {
        while (qt * j > kKnnRegBudget) qt /= 2;
        p->jregs = j;
        p->dist_lds_bytes = 0;
    } else {
        while ((size_t)qt * dim * sizeof(float) > kKnnTileLdsBytes) qt /= 2;
        p->jregs = 0;
        p->dist_lds_bytes = (size_t)qt * dim * sizeof(float);
    }
    p->qt = qt;
    p->chunk_rows = chunk_rows;
    p->groups = std::max(1, std::min(kKnnMaxGroups, kKnnMaxSort / R));
    p->buf_cap = (uint64_t)R + chunk_rows;
    p->mid_sort_n = knn_pow2_at_least(p->buf_cap);
    p->final_sort_n = knn_pow2_at_least((uint64_t)p->groups * R);
    const int sort_n = std::max(p->mid_sort_n, p->final_sort_n);
    p->select_threads = std::min(1024, std::max(64, sort_n / 2));
    p->select_lds_bytes = (size_t)sort_n * sizeof(uint64_t);
    const uint64_t per_query = (uint64_t)p->groups * (p->buf_cap * 8 + 4 + 8);
    if (pass_nq == 0) pass_nq = (int)std::max<uint64_t>(1, kKnnScratchBytes / per_query);
    p->pass_nq = std::min(nq, pass_nq);
    p->passes = (nq + p->pass_nq - 1) / p->pass_nq;
    p->scratch_bytes = (uint64_t)p->pass_nq * per_query;
    p->launches = (rows + (uint64_t)p->groups * chunk_rows - 1) / ((uint64_t)p->groups * chunk_rows);
    const int64_t tiles = (p->pass_nq + qt - 1) / qt;
    const int64_t live_groups = (int64_t)std::min<uint64_t>((uint64_t)p->groups, std::max<uint64_t>(1, (rows + chunk_rows - 1) / chunk_rows));
    int slice = kKnnMaxSlice;
    while (slice > kKnnMinSlice && tiles * live_groups * (int64_t)((chunk_rows + slice - 1) / slice) < kKnnWgFloor) slice /= 2;
    p->slice_rows = slice;
    p->slices = (int)((chunk_rows + slice - 1) / slice);
    return p->dist_lds_bytes <= kRefineLdsDefault && p->select_lds_bytes <= kRefineLdsDefault;
}

}  // namespace refine
}  // namespace qadc
