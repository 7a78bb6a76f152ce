// CPU driver of tests/test_pq_decode_plan_host.py: the launch geometry of the PQ decode kernels (host/pq_decode_plan.hpp) for one
// shape per input line.  Header-only.
//   pq_decode_plan_host < lines "sq_count sq_bits dim n out_aligned16"    one output line per input line: "refused", or the fields
//   dim dsub centroids code_bytes vec lanes_per_row rows_per_wg cb_in_lds cb_bytes gather_lds row_blocks gather_grid reg tile col_tiles
//   row_tiles rot_grid rot_lds err_grid, then cover: 1 when the rotation kernel's chains (pq_decode_rot_row / _col over every tile,
//   lane and register) cover every (row, column) of the pass exactly once (checked for passes of at most 4096 chains per tile row,
//   else -1)
#include <cstdint>
#include <iostream>
#include <vector>

#include "../../quick-adc_amd/host/pq_decode_plan.hpp"

static int cover(const qadc::PqDecodePlan& p, unsigned long long n) {
    if (n * (unsigned long long)p.dim > (1ull << 22)) return -1;
    std::vector<unsigned char> seen((size_t)n * p.dim, 0);
    for (unsigned long long ta = 0; ta < p.row_tiles; ++ta)
        for (int tb = 0; tb < p.col_tiles; ++tb)
            for (int lane = 0; lane < qadc::kDecodeWG; ++lane)
                for (int ra = 0; ra < p.reg; ++ra)
                    for (int rb = 0; rb < p.reg; ++rb) {
                        const unsigned long long i = qadc::pq_decode_rot_row(p.reg, ta, lane, ra);
                        const int c = qadc::pq_decode_rot_col(p.reg, tb, lane, rb);
                        if (i >= n || c >= p.dim) continue;
                        if (seen[(size_t)i * p.dim + c]++) return 0;
                    }
    for (unsigned char s : seen)
        if (s != 1) return 0;
    return 1;
}

int main() {
    unsigned long long n;
    int sq_count, sq_bits, dim, aligned;
    while (std::cin >> sq_count >> sq_bits >> dim >> n >> aligned) {
        qadc::PqDecodePlan p;
        if (!qadc::pq_decode_plan(sq_count, sq_bits, dim, n, aligned != 0, &p)) {
            std::cout << "refused\n";
            continue;
        }
        std::cout << p.dim << ' ' << p.dsub << ' ' << p.centroids << ' ' << p.code_bytes << ' ' << p.vec << ' ' << p.lanes_per_row << ' '
                  << p.rows_per_wg << ' ' << p.cb_in_lds << ' ' << p.cb_bytes << ' ' << p.gather_lds << ' ' << p.row_blocks << ' ' << p.gather_grid
                  << ' ' << p.reg << ' ' << p.tile << ' ' << p.col_tiles << ' ' << p.row_tiles << ' ' << p.rot_grid << ' ' << p.rot_lds << ' '
                  << p.err_grid << ' ' << cover(p, n) << '\n';
    }
    return 0;
}
