// CPU driver of the probed exact search's launch geometry (host/refine_probe_plan.hpp; tests/test_refine_probe_plan_host.py): plans
// every scenario of the input as the library compiles the header, builds the work of every pass and walks it as the launches and the
// kernel's loops do — launches, the items of a launch, the slices, the waves of a workgroup, the queries of a tile, through probe_slice
// — and writes the plan and what the walk saw out for the test to check.  No HIP, no library.
//   in : per scenario int64 nq, K, ma, dim, R, chunk_rows, pass_nq | int64 sizes [K] | int64 assign [nq][ma]
//   out: per scenario int64 rows of 24: accepted | qt, jregs, dist_lds_bytes, pass_nq, passes, chunk_rows, groups, per_group,
//        launch_rows, buf_cap, mid_sort_n, final_sort_n, select_threads, select_lds_bytes, scratch_bytes |
//        visits of (query, partition, row) triples in all | triples visited more than once | visits outside what is probed |
//        the most rows one (query, group) is offered in a launch | the largest grid.y | the most items and the most slots of a pass |
//        launches of all passes
// stdout: "ok <scenarios>".
#include <algorithm>
#include <cstdio>
#include <unordered_map>
#include <vector>

#include "../../quick-adc_amd/host/refine_probe_plan.hpp"

using namespace qadc::refine;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<int64_t> out;
    int64_t head[7];
    size_t n = 0;
    while (fread(head, sizeof(int64_t), 7, in) == 7) {
        const int nq = (int)head[0], K = (int)head[1], ma = (int)head[2];
        std::vector<int64_t> sizes64((size_t)std::max(K, 0)), assign64((size_t)std::max(nq, 0) * std::max(ma, 0));
        if (!sizes64.empty() && fread(sizes64.data(), 8, sizes64.size(), in) != sizes64.size()) return 3;
        if (!assign64.empty() && fread(assign64.data(), 8, assign64.size(), in) != assign64.size()) return 3;
        std::vector<uint32_t> sizes(sizes64.begin(), sizes64.end());
        std::vector<int32_t> assign(assign64.begin(), assign64.end());
        ++n;
        int64_t o[24] = {0};
        ProbePlan p{};
        o[0] = probe_plan(nq, ma, (int)head[3], (int)head[4], (uint64_t)head[5], (int)head[6], &p);
        if (!o[0]) {
            out.insert(out.end(), o, o + 24);
            continue;
        }
        const int64_t v[15] = {p.qt, p.jregs, (int64_t)p.dist_lds_bytes, p.pass_nq, p.passes, (int64_t)p.chunk_rows, p.groups, p.per_group,
                               (int64_t)p.launch_rows, (int64_t)p.buf_cap, p.mid_sort_n, p.final_sort_n, p.select_threads,
                               (int64_t)p.select_lds_bytes, (int64_t)p.scratch_bytes};
        for (int j = 0; j < 15; ++j) o[1 + j] = v[j];
        int64_t visits = 0, repeats = 0, strays = 0, most_offered = 0, most_y = 0, most_items = 0, most_slots = 0, launches = 0;
        for (int q0 = 0; q0 < nq; q0 += p.pass_nq) {
            const int pn = std::min(p.pass_nq, nq - q0);
            ProbeWork w;
            probe_work(p, pn, ma, assign.data() + (size_t)q0 * ma, sizes.data(), K, &w);
            most_items = std::max<int64_t>(most_items, (int64_t)w.items.size());
            most_slots = std::max<int64_t>(most_slots, (int64_t)w.slots.size());
            launches += (int64_t)w.launches;
            // what is probed: (query, partition) -> the rows seen so far
            std::unordered_map<uint64_t, std::vector<uint8_t>> seen;
            for (int q = 0; q < pn; ++q)
                for (int j = 0; j < ma; ++j) {
                    const int32_t part = assign[(size_t)(q0 + q) * ma + j];
                    if (part >= 0 && part < K) seen[(uint64_t)q * (uint64_t)K + (uint64_t)part].assign(sizes[part], 0);
                }
            for (uint64_t L = 0; L < w.launches; ++L) {
                std::unordered_map<uint32_t, int64_t> offered;   // slot -> rows of this launch
                const uint32_t gx = w.launch_items[(size_t)L], gy = w.launch_slices[(size_t)L];
                if (gx == 0 || gy == 0 || gx > w.items.size()) return 5;
                most_y = std::max<int64_t>(most_y, gy);
                for (uint32_t i = 0; i < gx; ++i) {
                    const ProbeItem& it = w.items[i];
                    if (it.count < 1 || it.count > (uint32_t)p.qt || it.first + it.count > w.slots.size() || it.part >= (uint32_t)K ||
                        it.rows != sizes[it.part])
                        return 5;
                    for (uint32_t s = 0; s < gy; ++s) {
                        uint64_t first, last;
                        probe_slice(it.rows, p.launch_rows, w.slice_rows, L, s, &first, &last);
                        for (int wave = 0; wave < kKnnWaves; ++wave)
                            for (uint64_t r = first + wave; r < last; r += kKnnWaves) {
                                if (r >= it.rows) return 5;   // (the kernel would read past the partition)
                                for (uint32_t t = 0; t < it.count; ++t) {
                                    const uint32_t slot = w.slots[it.first + t], q = slot / (uint32_t)p.groups;
                                    if (q >= (uint32_t)pn) return 5;
                                    ++offered[slot];
                                    ++visits;
                                    auto f = seen.find((uint64_t)q * (uint64_t)K + it.part);
                                    if (f == seen.end()) ++strays;
                                    else if (f->second[(size_t)r]++) ++repeats;
                                }
                            }
                    }
                }
                for (const auto& e : offered) most_offered = std::max(most_offered, e.second);
            }
            // (items behind a launch's prefix hold no row of it: the walk above would have missed their rows, and the test counts)
        }
        o[16] = visits; o[17] = repeats; o[18] = strays; o[19] = most_offered; o[20] = most_y; o[21] = most_items; o[22] = most_slots;
        o[23] = launches;
        out.insert(out.end(), o, o + 24);
    }
    fclose(in);
    FILE* f = fopen(argv[2], "wb");
    if (!f || (n && fwrite(out.data(), sizeof(int64_t), out.size(), f) != out.size()) || fclose(f) != 0) return 4;
    printf("ok %zu\n", n);
    return 0;
}
