// CPU driver of the float-ADC level planner (host/adc_plan.hpp; tests/test_adc_plan_host.py): reads one case, plans it and
// writes the whole plan out for the test to check.  No HIP, no library.
//   in : int32 R, nq, ma, parts | uint32 sizes[parts] | int32 assign[nq][ma]
//   out: uint32 kLevel0, kLevelGrowth, kWgTarget, kRunMin, kRunMax, levels, items | uint64 total[nq] | uint64 edge[levels + 1]
//        | uint32 level_first[levels + 1] | uint32 cap[nq] | items x 8 uint32
// stdout: "ok", or "refused: <message>" (nothing written).
#include <cstdio>
#include <vector>

#include "../../quick-adc_amd/host/adc_plan.hpp"

using namespace qadc::adc;

static_assert(sizeof(Item) == 32, "an Item is eight words");

template <typename T>
static bool get(FILE* f, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T>
static bool put(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    std::vector<int32_t> head(4);
    if (!in || !get(in, head)) return 3;
    const int R = head[0], nq = head[1], ma = head[2], parts = head[3];
    std::vector<uint32_t> sizes(parts);
    std::vector<int32_t> assign((size_t)nq * ma);
    if (!get(in, sizes) || !get(in, assign)) return 3;
    fclose(in);
    const Plan p = plan_levels(sizes.data(), nq, ma, assign.data(), R);
    if (!p.refused.empty()) {
        printf("refused: %s\n", p.refused.c_str());
        return 0;
    }
    FILE* out = fopen(argv[2], "wb");
    const std::vector<uint32_t> consts{kLevel0, kLevelGrowth, kWgTarget, kRunMin, kRunMax, (uint32_t)p.levels(), (uint32_t)p.items.size()};
    if (!out || !put(out, consts) || !put(out, p.total) || !put(out, p.edge) || !put(out, p.level_first) || !put(out, p.cap) ||
        !put(out, p.items) || fclose(out) != 0)
        return 4;
    printf("ok\n");
    return 0;
}
