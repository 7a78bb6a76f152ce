// CPU driver of the 4-bit index's append planner (host/index_append_plan.hpp; tests/test_index_append_plan_host.py): reads a
// sequence of appends, plans each on the state the one before left, as qadc_index_add_vectors and qadc_index_reserve do, and
// writes every plan out for the test to check.  No HIP, no library.
//   in : int32 code_size, parts, steps | uint32 sizes[parts] | uint32 caps[parts]
//        | steps x { int32 grow, has_floor | uint64 add[parts] | uint32 floor[parts] }
//   out: steps x { int32 status (0 in place, 1 moved, 2 refused) | unless refused: uint32 cap[parts] | uint64 off[parts]
//        | uint64 lab_off[parts] | uint64 code_bytes, label_count | uint64 region_bytes[parts] | uint64 zero_first[parts]
//        | uint64 zero_last[parts] (the span kept zero behind the rows each partition holds after the step) }
// A refused step changes nothing.  stdout: "ok <kIndexRegionPad>", then one line "refused <step>: <message>" per refused step.
#include <cstdio>
#include <string>
#include <vector>

#include "../../quick-adc_amd/host/index_append_plan.hpp"

using namespace qadc::adc;

template <typename T>
static bool get(FILE* f, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T>
static bool put(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    std::vector<int32_t> head(3);
    if (!in || !get(in, head)) return 3;
    const int code_size = head[0], parts = head[1], steps = head[2];
    std::vector<uint32_t> sizes(parts), caps(parts), floor(parts);
    std::vector<uint64_t> add(parts);
    if (!get(in, sizes) || !get(in, caps)) return 3;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 4;
    std::string refusals;
    for (int s = 0; s < steps; ++s) {
        std::vector<int32_t> flags(2);
        if (!get(in, flags) || !get(in, add) || !get(in, floor)) return 3;
        const AppendPlan p = plan_index_append(code_size, (size_t)parts, sizes.data(), caps.data(), add.data(), flags[1] ? floor.data() : nullptr, flags[0] != 0);
        const std::vector<int32_t> status{!p.refused.empty() ? 2 : p.in_place ? 0 : 1};
        if (!put(out, status)) return 4;
        if (!p.refused.empty()) {
            refusals += "refused " + std::to_string(s) + ": " + p.refused + "\n";
            continue;
        }
        const std::vector<uint64_t> totals{p.code_bytes, p.label_count};
        if (!put(out, p.cap) || !put(out, p.off) || !put(out, p.lab_off) || !put(out, totals)) return 4;
        std::vector<uint64_t> region(parts), zfirst(parts), zlast(parts);
        for (int i = 0; i < parts; ++i) {
            sizes[i] += (uint32_t)add[i];
            region[i] = index_region_bytes(p.cap[i], code_size);
            index_zero_span(sizes[i], code_size, &zfirst[i], &zlast[i]);
        }
        if (!put(out, region) || !put(out, zfirst) || !put(out, zlast)) return 4;
        caps = p.cap;
    }
    fclose(in);
    if (fclose(out) != 0) return 4;
    printf("ok %llu\n%s", (unsigned long long)kIndexRegionPad, refusals.c_str());
    return 0;
}
