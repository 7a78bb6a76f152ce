// Geometry of the k-means++ seeding kernels (csrc/qadc_kmeans_seed_kernel.hip) — HIP-free, so that
// tests/cpp/kmeans_seed_plan_host.cpp can check it on the CPU.
//
// The sum tree of include/qadc.h has radix kSeedRadix and is indexed by the row alone: node j of level L covers rows
// [j 64^L, (j + 1) 64^L).  Levels 1 and 2 always exist; above them the tree goes up to the first level with one node, the root.
// seed_update_kernel gives a workgroup whole level-2 nodes (kSeedRowsPerWG rows): a wave takes a level-1 node at a time, lane <-> row
// for the distance chains and the butterfly; the rows' components reach the lanes through an LDS window of kSeedCols columns,
// loaded with the lanes along the components.  seed_pick_kernel is one workgroup per sub-space.
#pragma once
#include <cstddef>
#include <cstdint>

namespace qadc {

constexpr int kSeedRadix = 64;               // children of a tree node = lanes of a wave
constexpr int kSeedWG = 256;                 // lanes of a workgroup of both kernels = their __launch_bounds__
constexpr int kSeedWaves = kSeedWG / kSeedRadix;
constexpr int kSeedRowsPerWG = kSeedRadix * kSeedRadix;   // one level-2 node
constexpr int kSeedNodesPerWave = kSeedRadix / kSeedWaves; // level-1 nodes a wave walks
constexpr int kSeedCols = 32;                // columns of the staged window
constexpr int kSeedColStride = kSeedCols + 1; // floats between two rows of the window: odd, so that lane <-> row reads hit every bank once
constexpr int kSeedMaxDim = 4096;
constexpr int kSeedMaxSq = 32;
constexpr int kSeedMaxLevels = 7;            // levels 0..6: 64^6 >= 2^32
constexpr size_t kSeedLdsLimit = 64 * 1024;  // what a launch may ask for without opting in to more

// why a call is refused (kSeedOk: it is not); the C-ABI turns each into QADC_E_ARG with kmeans_seed_refusal_text
enum KmeansSeedRefusal {
    kSeedOk = 0, kSeedNullVectors, kSeedNullCentres, kSeedRows, kSeedK, kSeedSqCount, kSeedDimSplit, kSeedDim, kSeedCoarse
};

inline KmeansSeedRefusal kmeans_seed_refusal(bool has_vectors, bool has_centres, uint64_t n, int dim, int sq_count, int64_t k, int K_coarse,
                                             bool has_coarse) {
    if (!has_vectors) return kSeedNullVectors;
    if (!has_centres) return kSeedNullCentres;
    if (n == 0 || n >= (1ull << 32)) return kSeedRows;
    if (k < 1 || (uint64_t)k > n) return kSeedK;
    if (sq_count < 1 || sq_count > kSeedMaxSq) return kSeedSqCount;
    if (dim <= 0 || dim % sq_count != 0) return kSeedDimSplit;
    if (dim > kSeedMaxDim) return kSeedDim;
    if (K_coarse < 0 || (K_coarse > 0 && !has_coarse)) return kSeedCoarse;
    return kSeedOk;
}

inline const char* kmeans_seed_refusal_text(KmeansSeedRefusal r) {
    switch (r) {
        case kSeedOk: return "";
        case kSeedNullVectors: return "vectors must not be NULL";
        case kSeedNullCentres: return "centres_out must not be NULL";
        case kSeedRows: return "need 0 < n < 2^32 vectors";
        case kSeedK: return "need 1 <= k <= n centres per sub-space";
        case kSeedSqCount: return "sq_count must be in [1, 32]";
        case kSeedDimSplit: return "dim must be a positive multiple of sq_count";
        case kSeedDim: return "dim must be <= 4096 (the update kernel keeps a round's centres in LDS)";
        default: return "K_coarse must be >= 0, and K_coarse > 0 needs the coarse centroids";
    }
}

// nodes of level L over n rows: ceil(n / 64^L)
inline uint64_t kmeans_seed_nodes(uint64_t n, int level) {
    uint64_t c = n;
    for (int l = 0; l < level; ++l) c = (c + kSeedRadix - 1) / kSeedRadix;
    return c;
}

struct KmeansSeedPlan {
    int dim, dsub, sq_count;
    int wg, rows_per_wg, cols;
    unsigned update_grid;              // ceil(n / rows_per_wg) workgroups
    unsigned pick_grid;                // sq_count workgroups
    size_t lds_bytes;                  // the waves' windows and a round's centres
    int root_level;                    // >= 2
    uint64_t nodes[kSeedMaxLevels];    // per level; 0 above the root
    uint64_t upper_nodes;              // nodes of levels 3..root per sub-space (seed_pick_kernel's scratch)
    uint64_t upper_offset[kSeedMaxLevels];  // where level L >= 3 starts in it
    uint64_t bitmap_words;             // 32-bit words of a sub-space's picked bitmap
    uint64_t scratch_bytes;            // everything the run allocates beside the learning set's front: see kmeans_seed_plan
};

// the window row a lane loads in step `step` of a window, and its column: lanes along the components, two rows per step
constexpr int kmeans_seed_load_row(int step, int lane) { return step * (kSeedRadix / kSeedCols) + lane / kSeedCols; }
constexpr int kmeans_seed_load_col(int lane) { return lane % kSeedCols; }
constexpr int kSeedLoadSteps = kSeedRadix / (kSeedRadix / kSeedCols);   // steps that fill a window of 64 rows
// the row that lane `lane` of wave `wave` of workgroup `wg` owns in the wave's `node`-th level-1 node
constexpr uint64_t kmeans_seed_row(uint64_t wg, int wave, int node, int lane) {
    return wg * (uint64_t)kSeedRowsPerWG + (uint64_t)((node * kSeedWaves + wave) * kSeedRadix + lane);
}

// false: arguments the kernels do not take (kmeans_seed_refusal says why)
inline bool kmeans_seed_plan(uint64_t n, int dim, int sq_count, uint64_t k, KmeansSeedPlan* p) {
    if (kmeans_seed_refusal(true, true, n, dim, sq_count, (int64_t)(k > (1ull << 62) ? -1 : (int64_t)k), 0, false) != kSeedOk) return false;
    p->dim = dim;
    p->sq_count = sq_count;
    p->dsub = dim / sq_count;
    p->wg = kSeedWG;
    p->rows_per_wg = kSeedRowsPerWG;
    p->cols = kSeedCols;
    p->update_grid = (unsigned)((n + kSeedRowsPerWG - 1) / kSeedRowsPerWG);
    p->pick_grid = (unsigned)sq_count;
    p->lds_bytes = sizeof(float) * ((size_t)kSeedWaves * kSeedRadix * kSeedColStride + (size_t)dim);
    p->root_level = 2;
    while (kmeans_seed_nodes(n, p->root_level) > 1) ++p->root_level;
    p->upper_nodes = 0;
    for (int l = 0; l < kSeedMaxLevels; ++l) {
        p->nodes[l] = l <= p->root_level ? kmeans_seed_nodes(n, l) : 0;
        p->upper_offset[l] = p->upper_nodes;
        if (l >= 3) p->upper_nodes += p->nodes[l];
    }
    p->bitmap_words = (n + 31) / 32;
    const uint64_t S = (uint64_t)sq_count;
    p->scratch_bytes = S * n * sizeof(float)                                     // mind
                     + S * (p->nodes[1] + p->nodes[2] + p->upper_nodes) * sizeof(double)   // the tree above level 0
                     + S * p->bitmap_words * sizeof(uint32_t)                    // picked
                     + S * (sizeof(uint32_t) + sizeof(uint64_t))                 // fallback cursor and count
                     + S * k * (uint64_t)p->dsub * sizeof(float)                 // centres
                     + S * k * sizeof(uint32_t);                                 // rows
    return p->lds_bytes <= kSeedLdsLimit;
}

}  // namespace qadc
