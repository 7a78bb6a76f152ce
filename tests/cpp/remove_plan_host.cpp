// CPU driver of the remove-by-label planner (host/remove_plan.hpp; tests/test_remove_plan_host.py): reads spans and one call's
// counts, plans them as qadc_adc_index_remove_labels and qadc_index_remove_labels do, and writes the plans out for the test to
// check.  No HIP, no library.
//   in : int32 code_size, parts, tile, zero_tail, spans | uint32 lo_hi[spans][2] | uint32 sizes[parts] | uint32 hits[parts]
//        | uint32 first[parts]
//   out: spans x { uint32 lo, last | uint64 bits, words } | uint64 touched, removed | uint32 new_sizes[parts]
//        | touched x { uint32 part, n, first_tile, n_new | uint64 zero_first, zero_last, padded_end (index_padded_end of the new rows) }
// stdout: "ok".
#include <cstdio>
#include <vector>

#include "../../quick-adc_amd/host/remove_plan.hpp"

using namespace qadc::adc;

template <typename T>
static bool get(FILE* f, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T>
static bool put(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    std::vector<int32_t> head(5);
    if (!in || !get(in, head)) return 3;
    const int code_size = head[0], parts = head[1], tile = head[2], zero_tail = head[3], spans = head[4];
    std::vector<uint32_t> lohi(2 * (size_t)spans), sizes(parts), hits(parts), first(parts);
    if (!get(in, lohi) || !get(in, sizes) || !get(in, hits) || !get(in, first)) return 3;
    fclose(in);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 4;
    for (int s = 0; s < spans; ++s) {
        const RemoveSpan sp = remove_span(lohi[2 * s], lohi[2 * s + 1]);
        if (!put(out, std::vector<uint32_t>{sp.lo, sp.last}) || !put(out, std::vector<uint64_t>{sp.bits, sp.words})) return 4;
    }
    const RemovePlan p = plan_remove(code_size, (size_t)parts, sizes.data(), hits.data(), first.data(), (uint32_t)tile, zero_tail != 0);
    if (!put(out, std::vector<uint64_t>{p.touched.size(), p.removed}) || !put(out, p.sizes)) return 4;
    for (const RemoveEntry& e : p.touched)
        if (!put(out, std::vector<uint32_t>{e.part, e.n, e.first_tile, e.n_new}) ||
            !put(out, std::vector<uint64_t>{e.zero_first, e.zero_last, index_padded_end((uint64_t)e.n_new * code_size)}))
            return 4;
    if (fclose(out) != 0) return 4;
    printf("ok\n");
    return 0;
}
