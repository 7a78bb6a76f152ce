// CPU driver of the planner's nibble-form field (host/level_plan.hpp; tests/test_level_plan_nib_host.py): plans one batch over
// partitions that all have a byte-plane copy, some of them a nibble-plane copy as well, and writes out the form fields of every
// launch beside the lengths of its runs.  No HIP, no library.  Partition "pointers" are fake bases: nothing is dereferenced.
//   in : int64 small_run, share_variant, split_min_run, split5_min_run, nib_min_run, nib8_min_run, nib_ns (-1: the three nibble
//              members are left out of the initialiser), nq, ma, parts | parts x int64 n | parts x int64 has_nib | int32 assign[nq][ma]
//   out: uint64 launches | launches x uint64 {first, nitems, small, shared, split, split5, nib, min n, max n, runs with a copy
//              pointer whose partition has a nibble-plane copy, of those: runs whose pointer is the tile of their first code in the
//              copy the launch reads (nib: the nibble-plane copy, else the byte-plane copy)}
// stdout: "ok", or "refused: <message>" (nothing written).
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../quick-adc_amd/host/level_plan.hpp"

using namespace qadc;
using namespace qadc::host;

template <typename T>
static bool get(FILE* f, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    std::vector<int64_t> h(10);
    if (!in || !get(in, h)) return 3;
    LevelOptions o{16, 512, 4, 0, (uint32_t)h[0], 0, (int)h[1], 1, 1u << 16, (uint64_t)h[2], 0, (uint64_t)h[3]};
    if (h[6] >= 0)
        o = LevelOptions{16, 512, 4, 0, (uint32_t)h[0], 0, (int)h[1], 1, 1u << 16, (uint64_t)h[2], 0, (uint64_t)h[3],
                         (uint64_t)h[4], (uint64_t)h[5], (int)h[6]};
    const int nq = (int)h[7], ma = (int)h[8];
    std::vector<int64_t> sizes((size_t)h[9]), has_nib((size_t)h[9]);
    std::vector<int32_t> assign((size_t)nq * ma);
    if (!get(in, sizes) || !get(in, has_nib) || !get(in, assign)) return 3;
    fclose(in);
    std::vector<LevelPart> parts(sizes.size());
    for (size_t i = 0; i < parts.size(); ++i) {
        LevelPart& p = parts[i];
        p.d_codes = reinterpret_cast<uint8_t*>((uintptr_t)((4 * i + 1) << 40));
        p.d_split = reinterpret_cast<uint8_t*>((uintptr_t)((4 * i + 2) << 40));
        if (has_nib[i]) p.d_nib = reinterpret_cast<uint8_t*>((uintptr_t)((4 * i + 3) << 40));
        p.n = p.global_n = (uint32_t)sizes[i];
        p.start_n = std::max<uint32_t>(1, p.n / 100);
    }
    const LevelBatch b{nq, ma, assign.data(), 100, 0, true, false, 0, 1, 0};
    const BatchPlan p = plan_levels(parts.data(), parts.size(), o, b);
    if (!p.refused.empty()) {
        printf("refused: %s\n", p.refused.c_str());
        return 0;
    }
    std::vector<uint64_t> w{p.launches.size()};
    for (const LevelLaunch& ll : p.launches) {
        uint64_t mn = ~0ull, mx = 0, with = 0, on_tile = 0;
        for (int i = 0; i < ll.nitems; ++i) {
            const ScanItem& it = p.all_items[ll.first + i];
            mn = std::min<uint64_t>(mn, it.n);
            mx = std::max<uint64_t>(mx, it.n);
            const size_t part = (size_t)((uintptr_t)it.codes >> 40) / 4;
            if (!it.split || part >= parts.size() || !parts[part].d_nib) continue;
            ++with;
            const uint64_t tile = it.pos0 / kSplitTile;
            on_tile += it.pos0 % kSplitTile == 0 &&
                       it.split == (ll.nib ? parts[part].d_nib + tile * kNibTileBytes : parts[part].d_split + tile * kSplitBytes * kSplitTile);
        }
        w.insert(w.end(), {(uint64_t)ll.first, (uint64_t)ll.nitems, ll.small, ll.shared, ll.split, ll.split5, (uint64_t)ll.nib, mn, mx, with, on_tile});
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out || fwrite(w.data(), sizeof(uint64_t), w.size(), out) != w.size() || fclose(out) != 0) return 4;
    printf("ok\n");
    return 0;
}
