// TEST DRIVER (CPU only): the plan of the keyed refine store as the library compiles it (host/refine_keyed_plan.hpp; DESIGN.md
// section 11.14), evaluated on rows read from a file.  tests/test_refine_keyed_plan_host.py holds the outputs to the invariants the
// host unit and the kernels rely on.  C++14, header only.
//   usage: refine_keyed_plan_host IN OUT
//   IN : rows of int64 [kind, a, b, c, d]
//        0 keyed_slot(key a, bits b)   1 plan_put(bits a, live b, dead c, absent d)   2 plan_reserve(bits a, rows b)
//        3 keyed_pass(dim a)           4 keyed_grid(n a)                              5 keyed_bits_for(keys a)
//   OUT: rows of int64 [x, y, z]: the value in x (y = z = 0), or a plan as refused, rebuild, bits
//   prints "ok <rows> <kKeyedMinBits> <kKeyedMaxBits> <kKeyedMaxKeys> <kKeyedPass> <kKeyedPassFloats> <kKeyedThreads> <kKeyedMaxGrid> <kKeyedSlotBytes>"
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <vector>

#include "../../quick-adc_amd/host/refine_keyed_plan.hpp"

using namespace qadc::refine;

int main(int argc, char** argv) {
    if (argc != 3) {
        std::cerr << "usage: refine_keyed_plan_host IN OUT" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::int64_t row[5];
    std::uint64_t rows = 0;
    while (std::fread(row, 8, 5, in) == 5) {
        std::int64_t res[3] = {0, 0, 0};
        KeyedPutPlan p{false, false, 0};
        switch (row[0]) {
            case 0: res[0] = keyed_slot((std::uint32_t)row[1], (int)row[2]); break;
            case 1: p = plan_put((int)row[1], (std::uint64_t)row[2], (std::uint64_t)row[3], (std::uint64_t)row[4]); break;
            case 2: p = plan_reserve((int)row[1], (std::uint64_t)row[2]); break;
            case 3: res[0] = (std::int64_t)keyed_pass((int)row[1]); break;
            case 4: res[0] = keyed_grid((std::uint64_t)row[1]); break;
            case 5: res[0] = keyed_bits_for((std::uint64_t)row[1]); break;
            default: std::cerr << "unknown row kind" << std::endl; return 2;
        }
        if (row[0] == 1 || row[0] == 2) {
            res[0] = p.refused;
            res[1] = p.rebuild;
            res[2] = p.bits;
        }
        std::fwrite(res, 8, 3, out);
        ++rows;
    }
    std::fclose(in);
    std::fclose(out);
    std::cout << "ok " << rows << " " << kKeyedMinBits << " " << kKeyedMaxBits << " " << kKeyedMaxKeys << " " << kKeyedPass << " " << kKeyedPassFloats
              << " " << kKeyedThreads << " " << kKeyedMaxGrid << " " << kKeyedSlotBytes << std::endl;
    return 0;
}
