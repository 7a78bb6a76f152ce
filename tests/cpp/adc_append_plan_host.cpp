// CPU driver of the float-ADC append planner (host/adc_append_plan.hpp; tests/test_adc_append_plan_host.py): reads a sequence of
// appends, plans each on the state the one before left, as qadc_adc_index_add_vectors and qadc_adc_index_reserve do, and writes
// every plan out for the test to check.  No HIP, no library.
//   in : int32 code_size, parts, steps | uint32 sizes[parts] | uint32 caps[parts]
//        | steps x { int32 grow, has_floor | uint64 add[parts] | uint32 floor[parts] }
//   out: steps x { int32 status (0 in place, 1 moved, 2 refused) | unless refused: uint32 cap[parts] | uint64 off[parts]
//        | uint64 lab_off[parts] | uint64 code_bytes, label_count }
// A refused step changes nothing.  stdout: "ok", then one line "refused <step>: <message>" per refused step.
//   bases <sizes: a,b,...> <counts: a,b,...>: the bases of one add_vectors pass (append_bases), one per line on stdout.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../quick-adc_amd/host/adc_append_plan.hpp"

using namespace qadc::adc;

template <typename T>
static bool get(FILE* f, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T>
static bool put(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

static std::vector<uint32_t> list(const std::string& s) {
    std::vector<uint32_t> v;
    for (size_t at = 0; at <= s.size();) {
        const size_t comma = s.find(',', at) == std::string::npos ? s.size() : s.find(',', at);
        v.push_back((uint32_t)std::strtoull(s.substr(at, comma - at).c_str(), nullptr, 10));
        at = comma + 1;
    }
    return v;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "bases") {
        const std::vector<uint32_t> sizes = list(argv[2]), count = list(argv[3]);
        if (sizes.size() != count.size()) return 2;
        std::vector<uint32_t> base(sizes.size());
        append_bases(sizes.size(), sizes.data(), count.data(), base.data());
        for (uint32_t b : base) printf("%u\n", b);
        return 0;
    }
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
        const AppendPlan p = plan_append(code_size, (size_t)parts, sizes.data(), caps.data(), add.data(), flags[1] ? floor.data() : nullptr, flags[0] != 0);
        const std::vector<int32_t> status{!p.refused.empty() ? 2 : p.in_place ? 0 : 1};
        if (!put(out, status)) return 4;
        if (!p.refused.empty()) {
            refusals += "refused " + std::to_string(s) + ": " + p.refused + "\n";
            continue;
        }
        const std::vector<uint64_t> totals{p.code_bytes, p.label_count};
        if (!put(out, p.cap) || !put(out, p.off) || !put(out, p.lab_off) || !put(out, totals)) return 4;
        for (int i = 0; i < parts; ++i) sizes[i] += (uint32_t)add[i];
        caps = p.cap;
    }
    fclose(in);
    if (fclose(out) != 0) return 4;
    printf("ok\n%s", refusals.c_str());
    return 0;
}
