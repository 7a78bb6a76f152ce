// CPU driver of tests/test_kmeans_seed_plan_host.py: the geometry of the k-means++ seeding kernels (host/kmeans_seed_plan.hpp).
// Header-only.
//   kmeans_seed_plan_host plan N DIM SQ_COUNT K   prints the plan, or "refused <why>"
//   kmeans_seed_plan_host rows N                  `owned`: 1 where every row below N is owned by exactly one lane of one wave of one
//                                                 workgroup of the update launch (the kernel's own indexing), no slot of a workgroup
//                                                 leaves its level-2 node, and a window's loads fill each of its cells once
//   kmeans_seed_plan_host sweep N                 for every (SQ_COUNT, DIM) the call admits: the plan's LDS, and the kernel's walk over
//                                                 the columns — every column once, ascending, a sub-space closed exactly at its end;
//                                                 prints the number of shapes, the largest LDS and `ok`
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../quick-adc_amd/host/kmeans_seed_plan.hpp"

using namespace qadc;

static bool rows_owned_once(std::uint64_t n) {
    KmeansSeedPlan p;
    if (!kmeans_seed_plan(n, 8, 1, 1, &p)) return false;
    std::vector<unsigned char> owners(n, 0);
    for (std::uint64_t wg = 0; wg < p.update_grid; ++wg)
        for (int wave = 0; wave < kSeedWaves; ++wave)
            for (int node = 0; node < kSeedNodesPerWave; ++node)
                for (int lane = 0; lane < kSeedRadix; ++lane) {
                    const std::uint64_t row = kmeans_seed_row(wg, wave, node, lane);
                    if (row / kSeedRowsPerWG != wg) return false;                       // a workgroup stays inside its level-2 node
                    if ((row / kSeedRadix) % kSeedWaves != (std::uint64_t)wave || row % kSeedRadix != (std::uint64_t)lane) return false;
                    if (row < n && owners[row]++) return false;
                }
    for (unsigned char o : owners)
        if (o != 1) return false;
    std::vector<unsigned char> cell((size_t)kSeedRadix * kSeedCols, 0);               // a window: 64 rows x kSeedCols columns
    for (int s = 0; s < kSeedLoadSteps; ++s)
        for (int lane = 0; lane < kSeedRadix; ++lane) {
            const int r = kmeans_seed_load_row(s, lane), c = kmeans_seed_load_col(lane);
            if (r < 0 || r >= kSeedRadix || c < 0 || c >= kSeedCols || cell[(size_t)r * kSeedCols + c]++) return false;
        }
    for (unsigned char o : cell)
        if (o != 1) return false;
    return true;
}

// seed_update_kernel's loop over the columns of a row
static bool columns_walk(const KmeansSeedPlan& p) {
    int m = 0, left = p.dsub, next = 0;
    for (int c0 = 0; c0 < p.dim; c0 += kSeedCols) {
        const int cols = p.dim - c0 < kSeedCols ? p.dim - c0 : kSeedCols;
        for (int cc = 0; cc < cols; ++cc) {
            if (c0 + cc != next++) return false;
            if (--left == 0) {
                if (c0 + cc != (m + 1) * p.dsub - 1) return false;
                ++m;
                left = p.dsub;
            }
        }
    }
    return next == p.dim && m == p.sq_count && left == p.dsub;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plan" && argc == 6) {
        const std::uint64_t n = std::strtoull(argv[2], nullptr, 10);
        const int dim = std::atoi(argv[3]), sq_count = std::atoi(argv[4]);
        const long long k = std::atoll(argv[5]);
        const KmeansSeedRefusal r = kmeans_seed_refusal(true, true, n, dim, sq_count, k, 0, false);
        KmeansSeedPlan p;
        if (r != kSeedOk || !kmeans_seed_plan(n, dim, sq_count, (std::uint64_t)k, &p)) {
            std::cout << "refused " << (int)r << " " << kmeans_seed_refusal_text(r) << std::endl;
            return 0;
        }
        std::cout << "wg=" << p.wg << " rows_per_wg=" << p.rows_per_wg << " cols=" << p.cols << " dim=" << p.dim << " dsub=" << p.dsub
                  << " update_grid=" << p.update_grid << " pick_grid=" << p.pick_grid << " lds=" << p.lds_bytes << " lds_limit=" << kSeedLdsLimit
                  << " root_level=" << p.root_level << " upper_nodes=" << p.upper_nodes << " bitmap_words=" << p.bitmap_words
                  << " scratch_bytes=" << p.scratch_bytes;
        for (int l = 0; l < kSeedMaxLevels; ++l) std::cout << " nodes" << l << "=" << p.nodes[l];
        for (int l = 3; l < kSeedMaxLevels; ++l) std::cout << " offset" << l << "=" << p.upper_offset[l];
        std::cout << std::endl;
        return 0;
    }
    if (mode == "rows" && argc == 3) {
        std::cout << "owned=" << (rows_owned_once(std::strtoull(argv[2], nullptr, 10)) ? 1 : 0) << std::endl;
        return 0;
    }
    if (mode == "sweep" && argc == 3) {
        const std::uint64_t n = std::strtoull(argv[2], nullptr, 10);
        long shapes = 0;
        size_t max_lds = 0;
        bool ok = true;
        for (int sq_count = 1; sq_count <= kSeedMaxSq; ++sq_count)
            for (int dim = sq_count; dim <= kSeedMaxDim; dim += sq_count) {
                KmeansSeedPlan p;
                if (!kmeans_seed_plan(n, dim, sq_count, 1, &p)) { ok = false; continue; }
                ++shapes;
                if (p.lds_bytes > max_lds) max_lds = p.lds_bytes;
                ok = ok && p.lds_bytes <= kSeedLdsLimit && p.lds_bytes == sizeof(float) * ((size_t)kSeedWaves * kSeedRadix * kSeedColStride + dim);
                ok = ok && p.dsub * sq_count == dim && p.pick_grid == (unsigned)sq_count && columns_walk(p);
            }
        std::cout << "shapes=" << shapes << " max_lds=" << max_lds << " ok=" << (ok ? 1 : 0) << std::endl;
        return 0;
    }
    std::fprintf(stderr, "usage: %s plan N DIM SQ_COUNT K | rows N | sweep N\n", argv[0]);
    return 2;
}
