// CPU driver of tests/test_opq_plan_host.py: the geometry of the OPQ cross-matrix kernels (host/opq_plan.hpp).  Header-only.
//   opq_plan_host plan SQ_COUNT SQ_BITS DIM N     prints the plan, or "refused"
//   opq_plan_host sweep SQ_COUNT SQ_BITS N        one line for every dim = SQ_COUNT * dsub <= kOpqMaxDim: the plan and `owned`, 1 where
//                                                 every (a, b) of the matrix is owned by exactly one register of one lane of one
//                                                 workgroup of a block, and no register owns a cell twice
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "../../quick-adc_amd/host/opq_plan.hpp"

static void print_plan(const qadc::OpqCrossPlan& p) {
    std::cout << "wg=" << qadc::kOpqWG << " lanes=" << qadc::kOpqLanes << " block=" << qadc::kOpqBlock << " max_dim=" << qadc::kOpqMaxDim
              << " dim=" << p.dim << " dsub=" << p.dsub << " K=" << p.K << " code_bytes=" << p.code_bytes << " reg=" << p.reg
              << " tile=" << p.tile << " tiles=" << p.tiles << " stage=" << p.stage << " lds=" << p.lds_bytes << " blocks=" << p.blocks
              << " grid=" << p.grid << " partial_bytes=" << p.partial_bytes << " reduce_grid=" << p.reduce_grid
              << " reduce_wg=" << qadc::kOpqReduceWG;
}

// the kernel's own indexing, over every workgroup of one block
static bool owned_once(const qadc::OpqCrossPlan& p) {
    std::vector<unsigned char> owners((size_t)p.dim * p.dim, 0);
    for (int ta = 0; ta < p.tiles; ++ta)
        for (int tb = 0; tb < p.tiles; ++tb)
            for (int lane = 0; lane < qadc::kOpqWG; ++lane)
                for (int ra = 0; ra < p.reg; ++ra)
                    for (int rb = 0; rb < p.reg; ++rb) {
                        const int a = qadc::opq_cross_row(p.reg, ta, lane, ra), b = qadc::opq_cross_col(p.reg, tb, lane, rb);
                        if (a < 0 || b < 0) return false;
                        if (a >= p.dim || b >= p.dim) continue;       // outside the matrix: not written
                        if (a >= (ta + 1) * p.tile || b >= (tb + 1) * p.tile || a < ta * p.tile || b < tb * p.tile) return false;   // outside the staged window
                        if (owners[(size_t)a * p.dim + b]++) return false;
                    }
    for (unsigned char o : owners)
        if (o != 1) return false;
    return true;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plan" && argc == 6) {
        qadc::OpqCrossPlan p;
        if (!qadc::opq_cross_plan(std::atoi(argv[4]), std::atoi(argv[2]), std::atoi(argv[3]), std::strtoull(argv[5], nullptr, 10), &p)) {
            std::cout << "refused" << std::endl;
            return 0;
        }
        print_plan(p);
        std::cout << std::endl;
        return 0;
    }
    if (mode == "sweep" && argc == 5) {
        const int sq_count = std::atoi(argv[2]), sq_bits = std::atoi(argv[3]);
        const std::uint64_t n = std::strtoull(argv[4], nullptr, 10);
        for (int dim = sq_count; dim <= qadc::kOpqMaxDim; dim += sq_count) {
            qadc::OpqCrossPlan p;
            if (!qadc::opq_cross_plan(dim, sq_count, sq_bits, n, &p)) {
                std::cout << "refused" << std::endl;
                continue;
            }
            print_plan(p);
            std::cout << " owned=" << (owned_once(p) ? 1 : 0) << std::endl;
        }
        return 0;
    }
    std::fprintf(stderr, "usage: %s plan SQ_COUNT SQ_BITS DIM N | sweep SQ_COUNT SQ_BITS N\n", argv[0]);
    return 2;
}
