// CPU driver of the int8 level-path planner (host/level_plan.hpp; tests/test_level_plan_host.py): reads one case, plans it and
// writes the whole plan out for the test to check.  No HIP, no library.  Partition "pointers" are fake bases: nothing is dereferenced.
//   in : int64 M, level_base, level_growth, head_level, small_run, wgs_per_item, share_variant, mq, prescan_sample, split_min_run,
//              split6_min_run, nq, ma, R, mode, float_path, full_prescan, pre_slice, pre_nslices, inj_n, parts
//        | parts x uint64 {d_codes, d_labels, d_starts, d_split, n, global_n, first_pos, start_n, key_base} | int32 assign[nq][ma]
//   out: uint64 kSplitTile, kSplitBytes, kMaxLevels, items, A items, B items, launches, fc_stride, head_codes, start_codes
//        | items x uint64 {codes, labels, n, pos0, key_base, table, query, order, dup_pos, dup_reps, split}
//        | (A items, then B items) x uint64 {codes, n, table, query, out_off, filter} | uint64 fc_init[2 nq]
//        | launches x uint64 {first, nitems, wgs, codes, small, shared, mq, split, split6, maxn}
// stdout: "ok", or "refused: <message>" (nothing written).
#include <cstdio>
#include <vector>

#include "../../quick-adc_amd/host/level_plan.hpp"

using namespace qadc;
using namespace qadc::host;

static_assert(sizeof(ScanItem) == 56 && sizeof(StartItem) == 32, "the layouts the kernels read");

template <typename T>
static bool get(FILE* f, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
static uint64_t u(const void* p) { return (uint64_t)reinterpret_cast<uintptr_t>(p); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    std::vector<int64_t> h(21);
    if (!in || !get(in, h)) return 3;
    const LevelOptions o{(int)h[0], (uint64_t)h[1], (uint64_t)h[2], (int)h[3], (uint32_t)h[4], (int)h[5], (int)h[6], (int)h[7],
                         (uint32_t)h[8], (uint64_t)h[9], (uint64_t)h[10]};
    const int nq = (int)h[11], ma = (int)h[12];
    std::vector<uint64_t> raw(9 * (size_t)h[20]);
    std::vector<int32_t> assign((size_t)nq * ma);
    if (!get(in, raw) || !get(in, assign)) return 3;
    fclose(in);
    std::vector<LevelPart> parts(raw.size() / 9);
    for (size_t i = 0; i < parts.size(); ++i) {
        const uint64_t* r = &raw[9 * i];
        LevelPart& p = parts[i];
        p.d_codes = reinterpret_cast<uint8_t*>((uintptr_t)r[0]);
        p.d_labels = reinterpret_cast<uint32_t*>((uintptr_t)r[1]);
        p.d_starts = reinterpret_cast<uint8_t*>((uintptr_t)r[2]);
        p.d_split = reinterpret_cast<uint8_t*>((uintptr_t)r[3]);
        p.n = (uint32_t)r[4];
        p.global_n = (uint32_t)r[5];
        p.first_pos = (uint32_t)r[6];
        p.start_n = (uint32_t)r[7];
        p.key_base = (uint32_t)r[8];
    }
    const LevelBatch b{nq, ma, assign.data(), (int)h[13], (int)h[14], h[15] != 0, h[16] != 0, (int)h[17], (int)h[18], (uint32_t)h[19]};
    const BatchPlan p = plan_levels(parts.data(), parts.size(), o, b);
    if (!p.refused.empty()) {
        printf("refused: %s\n", p.refused.c_str());
        return 0;
    }
    std::vector<uint64_t> w{kSplitTile, kSplitBytes, (uint64_t)kMaxLevels, p.all_items.size(), p.sitems_a.size(), p.sitems_b.size(),
                            p.launches.size(), p.fc_stride, p.head_codes, p.start_codes};
    for (const ScanItem& it : p.all_items)
        w.insert(w.end(), {u(it.codes), u(it.labels), it.n, it.pos0, it.key_base, it.table, it.query, it.order, it.dup_pos, it.dup_reps, u(it.split)});
    for (const std::vector<StartItem>* v : {&p.sitems_a, &p.sitems_b})
        for (const StartItem& si : *v) w.insert(w.end(), {u(si.codes), si.n, si.table, si.query, si.out_off, si.filter});
    w.insert(w.end(), p.fc_init.begin(), p.fc_init.end());
    for (const LevelLaunch& ll : p.launches)
        w.insert(w.end(), {(uint64_t)ll.first, (uint64_t)ll.nitems, (uint64_t)ll.wgs, ll.codes, ll.small, ll.shared, ll.mq, ll.split, ll.split6, ll.maxn});
    FILE* out = fopen(argv[2], "wb");
    if (!out || fwrite(w.data(), sizeof(uint64_t), w.size(), out) != w.size() || fclose(out) != 0) return 4;
    printf("ok\n");
    return 0;
}
