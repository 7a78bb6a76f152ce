// CPU driver of the re-ranking launch geometry (host/refine_plan.hpp; tests/test_refine_plan_host.py): plans every row of the input
// as the library compiles the header and writes the plans out for the test to check.  No HIP, no library.
//   in : int64 rows of 3: nq, r_in, dim
//   out: int64 rows of 9: accepted | pass_nq, passes, cands_per_wg, chunks, dist_lds_bytes, sort_n, sort_threads, select_lds_bytes
// stdout: "ok <rows>".
#include <cstdio>
#include <vector>

#include "../../quick-adc_amd/host/refine_plan.hpp"

using namespace qadc::refine;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<int64_t> rows;
    int64_t row[3];
    while (fread(row, sizeof(int64_t), 3, in) == 3) rows.insert(rows.end(), row, row + 3);
    fclose(in);
    const size_t n = rows.size() / 3;
    std::vector<int64_t> out(n * 9, 0);
    for (size_t i = 0; i < n; ++i) {
        const int64_t* a = rows.data() + i * 3;
        int64_t* o = out.data() + i * 9;
        RefinePlan p{};
        o[0] = refine_plan((int)a[0], (int)a[1], (int)a[2], &p);
        const int64_t v[8] = {p.pass_nq, p.passes, p.cands_per_wg, p.chunks, (int64_t)p.dist_lds_bytes, p.sort_n, p.sort_threads,
                              (int64_t)p.select_lds_bytes};
        for (int j = 0; j < 8; ++j) o[1 + j] = v[j];
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || (n && fwrite(out.data(), sizeof(int64_t), out.size(), f) != out.size()) || fclose(f) != 0) return 4;
    printf("ok %zu\n", n);
    return 0;
}
