// CPU driver of the exhaustive search's launch geometry (host/refine_knn_plan.hpp; tests/test_refine_knn_plan_host.py): plans every
// row of the input as the library compiles the header, walks the rows as the launches and the kernel's loops do — launches, the
// groups of a launch, the slices of a group, the waves of a workgroup, through knn_launch_groups and knn_slice — and writes the plan
// and what the walk saw out for the test to check.  No HIP, no library.
//   in : int64 rows of 7: nq, rows, dim, dtype, R, chunk_rows, pass_nq
//   out: int64 rows of 20: accepted | qt, jregs, dist_lds_bytes, pass_nq, passes, chunk_rows, groups, slice_rows, slices, launches,
//        buf_cap, mid_sort_n, final_sort_n, select_threads, select_lds_bytes, scratch_bytes |
//        the fewest and the most visits of a row | the most rows one (launch, group) appends from
// stdout: "ok <rows>".
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../quick-adc_amd/host/refine_knn_plan.hpp"

using namespace qadc::refine;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<int64_t> rows;
    int64_t row[7];
    while (fread(row, sizeof(int64_t), 7, in) == 7) rows.insert(rows.end(), row, row + 7);
    fclose(in);
    const size_t n = rows.size() / 7;
    std::vector<int64_t> out(n * 20, 0);
    for (size_t i = 0; i < n; ++i) {
        const int64_t* a = rows.data() + i * 7;
        int64_t* o = out.data() + i * 20;
        KnnPlan p{};
        o[0] = knn_plan((int)a[0], (uint64_t)a[1], (int)a[2], (int)a[3], (int)a[4], (uint64_t)a[5], (int)a[6], &p);
        if (!o[0]) continue;
        const int64_t v[16] = {p.qt, p.jregs, (int64_t)p.dist_lds_bytes, p.pass_nq, p.passes, (int64_t)p.chunk_rows, p.groups, p.slice_rows,
                               p.slices, (int64_t)p.launches, (int64_t)p.buf_cap, p.mid_sort_n, p.final_sort_n, p.select_threads,
                               (int64_t)p.select_lds_bytes, (int64_t)p.scratch_bytes};
        for (int j = 0; j < 16; ++j) o[1 + j] = v[j];
        const uint64_t nrows = (uint64_t)a[1];
        std::vector<uint8_t> seen((size_t)nrows, 0);
        int64_t most_group = 0;
        for (uint64_t l = 0; l < p.launches; ++l) {
            const int live = knn_launch_groups(nrows, p.chunk_rows, p.groups, l);
            for (int g = 0; g < live; ++g) {
                int64_t in_group = 0;
                for (int s = 0; s < p.slices; ++s) {
                    uint64_t first, last;
                    knn_slice(nrows, p.chunk_rows, p.groups, p.slice_rows, l, g, s, &first, &last);
                    for (int w = 0; w < kKnnWaves; ++w)
                        for (uint64_t r = first + w; r < last; r += kKnnWaves) {
                            if (r >= nrows) return 5;   // (the kernel would read past the store)
                            if (seen[(size_t)r] < 255) ++seen[(size_t)r];
                            ++in_group;
                        }
                }
                most_group = std::max(most_group, in_group);
            }
        }
        o[17] = nrows ? *std::min_element(seen.begin(), seen.end()) : 1;
        o[18] = nrows ? *std::max_element(seen.begin(), seen.end()) : 1;
        o[19] = most_group;
    }
    FILE* f = fopen(argv[2], "wb");
    if (!f || (n && fwrite(out.data(), sizeof(int64_t), out.size(), f) != out.size()) || fclose(f) != 0) return 4;
    printf("ok %zu\n", n);
    return 0;
}
