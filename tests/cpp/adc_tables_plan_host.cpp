// CPU driver of the float-ADC feeders' launch geometry (host/adc_tables_plan.hpp; tests/test_adc_tables_plan_host.py): plans every
// row of the input as the library compiles the header and writes the plans out for the test to check.  No HIP, no library.
//   in : int64 rows of 7: kind | a0 .. a5
//          kind 0 = adc_tables_plan(nq, ma, nsq, centroids, dim, rotated)
//          kind 1 = adc_encode_plan(n, nsq, dim)
//   out: int64 rows of 12: accepted |
//          kind 0: probes, pgroups, msplit, mper, cper, cslices, DS, grid x, y, z, lds_bytes
//          kind 1: vper, DS, grid, lds_bytes, 0 ...
// stdout: "ok <rows>".
#include <cstdio>
#include <vector>

#include "../../quick-adc_amd/host/adc_tables_plan.hpp"

using namespace qadc::adc;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<int64_t> rows;
    int64_t row[7];
    while (fread(row, sizeof(int64_t), 7, in) == 7) rows.insert(rows.end(), row, row + 7);
    fclose(in);
    const size_t n = rows.size() / 7;
    std::vector<int64_t> out(n * 12, 0);
    for (size_t i = 0; i < n; ++i) {
        const int64_t* a = rows.data() + i * 7;
        int64_t* o = out.data() + i * 12;
        if (a[0] == 0) {
            AdcTablesPlan p{};
            o[0] = adc_tables_plan((int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], a[6] != 0, &p);
            const int64_t v[11] = {p.probes, p.pgroups, p.msplit, p.mper, p.cper, p.cslices, p.DS, p.grid_x, p.grid_y, p.grid_z, (int64_t)p.lds_bytes};
            for (int j = 0; j < 11; ++j) o[1 + j] = v[j];
        } else if (a[0] == 1) {
            AdcEncodePlan p{};
            o[0] = adc_encode_plan((uint64_t)a[1], (int)a[2], (int)a[3], &p);
            o[1] = p.vper; o[2] = p.DS; o[3] = p.grid; o[4] = (int64_t)p.lds_bytes;
        } else {
            return 5;
        }
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || (n && fwrite(out.data(), sizeof(int64_t), out.size(), f) != out.size()) || fclose(f) != 0) return 4;
    printf("ok %zu\n", n);
    return 0;
}
