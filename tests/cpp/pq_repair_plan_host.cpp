// CPU driver of tests/test_pq_repair_plan_host.py: the launch geometry of the empty-cluster repair (host/pq_repair_plan.hpp) for one
// shape per input line.  Header-only.
//   pq_repair_plan_host < lines "n dim sq_count sq_bits"    one output line per input line: "refused", or the plan's fields
//   n dim sq_count sq_bits dsub K units_per_row unit_bytes units row_blocks unit_blocks count_in_lds count_lds_bytes ctl hist count
//   first empties blockcnt key total  (the last eight in bytes), then sizeof(PqRepairCtl)
#include <cstdint>
#include <iostream>

#include "../../quick-adc_amd/host/pq_repair_plan.hpp"

int main() {
    unsigned long long n;
    int dim, sq_count, sq_bits;
    while (std::cin >> n >> dim >> sq_count >> sq_bits) {
        qadc::PqRepairPlan p;
        if (!qadc::pq_repair_plan(n, dim, sq_count, sq_bits, &p)) {
            std::cout << "refused\n";
            continue;
        }
        std::cout << p.n << ' ' << p.dim << ' ' << p.sq_count << ' ' << p.sq_bits << ' ' << p.dsub << ' ' << p.K << ' ' << p.units_per_row << ' '
                  << p.unit_bytes << ' ' << p.units << ' ' << p.row_blocks << ' ' << p.unit_blocks << ' ' << p.count_in_lds << ' '
                  << p.count_lds_bytes << ' ' << p.ctl_bytes << ' ' << p.hist_bytes << ' ' << p.count_bytes << ' ' << p.first_bytes << ' '
                  << p.empties_bytes << ' ' << p.blockcnt_bytes << ' ' << p.key_bytes << ' ' << p.total_bytes << ' ' << sizeof(qadc::PqRepairCtl)
                  << '\n';
    }
    return 0;
}
