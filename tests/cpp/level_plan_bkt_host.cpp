// CPU check of the planner's bucket-form fields (host/level_plan.hpp; tests/test_level_plan_bkt_host.py).  Every case plans one
// batch twice: over partitions with a bucket copy ("with") and over the same partitions without one ("today").  No HIP, no library.
// Partition "pointers" are fake bases and the blocks' slot offsets are made up (whole tiles, growing unevenly): nothing is
// dereferenced.  Checked per launch, which both plans have in the same order:
//   - LevelLaunch::bkt is non-zero exactly when the launch is split and not shared and every one of its runs, restated here from
//     today's plan, starts on a block of its partition's copy, ends on one or at the partition's end and has bkt_min_run codes;
//   - such a launch: bkt = the fewest paid planes whose threshold its shortest run reaches; every run's n = the slots between the
//     offsets of its first block and of the block behind its last, split / codes = that tile of the copy and of the side array;
//     pos0 and the other fields of the run, the launch's codes and maxn are today's; slots = the runs' slots and wgs derives from them;
//     nib is 0;
//   - every other launch, and every one of its runs, equals today's field for field.
// argv: sizes "n0,n1,..", block, level_base, level_growth, head_level, bkt_min_run, bkt6, bkt5, bkt4, nq, orders "p p p;p p p" (one
// probe list per query), small_run, share_variant.  stdout: "ok <launches> <bkt launches> <bkt runs>", or a line that starts with "FAIL".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../../quick-adc_amd/host/level_plan.hpp"

using namespace qadc;
using namespace qadc::host;

static int fail(const char* what, size_t launch, size_t run) {
    printf("FAIL %s (launch %zu, run %zu)\n", what, launch, run);
    return 1;
}

static bool same_item(const ScanItem& a, const ScanItem& b) {
    return a.codes == b.codes && a.labels == b.labels && a.n == b.n && a.pos0 == b.pos0 && a.key_base == b.key_base && a.table == b.table &&
           a.query == b.query && a.order == b.order && a.dup_pos == b.dup_pos && a.dup_reps == b.dup_reps && a.split == b.split;
}

int main(int argc, char** argv) {
    if (argc != 14) return 2;
    std::vector<uint64_t> sizes;
    {
        std::stringstream ss(argv[1]);
        std::string tok;
        while (std::getline(ss, tok, ',')) sizes.push_back(strtoull(tok.c_str(), nullptr, 10));
    }
    const uint64_t block = strtoull(argv[2], nullptr, 10);
    LevelOptions o{16, strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10), atoi(argv[5]), (uint32_t)strtoul(argv[12], nullptr, 10), 0,
                   atoi(argv[13]), 1, 1u << 16, 1, 1, 1, 1, 0, 9};
    o.bkt_min_run = strtoull(argv[6], nullptr, 10);
    o.bkt6_min_run = strtoull(argv[7], nullptr, 10);
    o.bkt5_min_run = strtoull(argv[8], nullptr, 10);
    o.bkt4_min_run = strtoull(argv[9], nullptr, 10);
    const int nq = atoi(argv[10]);
    std::vector<int32_t> assign;
    {
        std::stringstream ss(argv[11]);
        std::string q;
        while (std::getline(ss, q, ';')) {
            std::stringstream qs(q);
            int p;
            while (qs >> p) assign.push_back(p);
        }
    }
    if (nq <= 0 || assign.size() % (size_t)nq != 0) return 2;
    const int ma = (int)(assign.size() / (size_t)nq);
    std::vector<LevelPart> with(sizes.size()), today(sizes.size());
    for (size_t i = 0; i < sizes.size(); ++i) {
        LevelPart& p = with[i];
        p.d_codes = reinterpret_cast<uint8_t*>((uintptr_t)((8 * i + 1) << 40));
        p.d_split = reinterpret_cast<uint8_t*>((uintptr_t)((8 * i + 2) << 40));
        p.d_nib = reinterpret_cast<uint8_t*>((uintptr_t)((8 * i + 3) << 40));
        p.n = p.global_n = (uint32_t)sizes[i];
        p.start_n = std::max<uint32_t>(1, p.n / 100);
        today[i] = p;
        if (i % 3 == 2) continue;                                // every third partition has no bucket copy
        p.d_bkt = reinterpret_cast<uint8_t*>((uintptr_t)((8 * i + 4) << 40));
        p.d_bkt_side = reinterpret_cast<uint8_t*>((uintptr_t)((8 * i + 5) << 40));
        p.bkt_block = block;
        p.bkt_off.push_back(0);
        for (uint64_t b0 = 0, b = 0; b0 < p.n; b0 += block, ++b) {
            const uint64_t nb = std::min<uint64_t>(block, p.n - b0);
            p.bkt_off.push_back(p.bkt_off.back() + (nb + (b % 3) * 1000 + kSplitTile - 1) / kSplitTile * kSplitTile + (b % 2) * kSplitTile);
        }
    }
    const LevelBatch b{nq, ma, assign.data(), 100, 0, true, false, 0, 1, 0};
    const BatchPlan A = plan_levels(with.data(), with.size(), o, b), B = plan_levels(today.data(), today.size(), o, b);
    if (!A.refused.empty() || !B.refused.empty()) return fail("refused", 0, 0);
    if (A.launches.size() != B.launches.size() || A.all_items.size() != B.all_items.size()) return fail("launch or run count differs", 0, 0);
    size_t nbkt = 0, nruns = 0;
    for (size_t l = 0; l < A.launches.size(); ++l) {
        const LevelLaunch &x = A.launches[l], &y = B.launches[l];
        if (x.first != y.first || x.nitems != y.nitems || x.small != y.small || x.shared != y.shared || x.mq != y.mq || x.split != y.split ||
            x.split6 != y.split6 || x.split5 != y.split5 || x.codes != y.codes || x.maxn != y.maxn || x.early != y.early || y.bkt != 0 || y.slots != 0)
            return fail("launch fields that no form may change", l, 0);
        // restated from today's runs: does every run cover whole blocks of a partition that has the copy?
        bool all_ok = y.split && !y.shared && o.bkt_min_run != 0;
        uint64_t minn = ~0ull, slots = 0, max_slots = 0;
        std::vector<uint64_t> want_slots((size_t)y.nitems);
        std::vector<const uint8_t*> want_tiles((size_t)y.nitems), want_side((size_t)y.nitems);
        for (int r = 0; r < y.nitems && all_ok; ++r) {
            const ScanItem& it = B.all_items[y.first + r];
            const size_t pi = (size_t)((uintptr_t)it.codes >> 40) / 8;
            const LevelPart& p = with[pi];
            const uint64_t b0 = it.pos0, e = b0 + it.n;
            all_ok = p.d_bkt && it.split && it.n >= o.bkt_min_run && b0 % block == 0 && (e % block == 0 || e == p.n);
            if (!all_ok) break;
            const uint64_t s0 = p.bkt_off[b0 / block], s1 = p.bkt_off[(e + block - 1) / block];
            want_slots[r] = s1 - s0;
            want_tiles[r] = p.d_bkt + s0 / kSplitTile * (uint64_t)kBktTileBytes;
            want_side[r] = p.d_bkt_side + s0 / kSplitTile * (uint64_t)kBktSideBytes;
            minn = std::min<uint64_t>(minn, it.n);
            slots += want_slots[r];
            max_slots = std::max(max_slots, want_slots[r]);
        }
        if ((x.bkt != 0) != all_ok) return fail("bkt set on a launch that does not qualify, or not set on one that does", l, 0);
        if (!all_ok) {
            if (x.nib != y.nib || x.wgs != y.wgs || x.slots != 0) return fail("a launch that does not qualify differs from today's", l, 0);
            for (int r = 0; r < y.nitems; ++r)
                if (!same_item(A.all_items[x.first + r], B.all_items[y.first + r])) return fail("a run that does not qualify differs from today's", l, r);
            continue;
        }
        ++nbkt;
        const int planes = o.bkt4_min_run && minn >= o.bkt4_min_run ? 4 : o.bkt5_min_run && minn >= o.bkt5_min_run ? 5
                           : o.bkt6_min_run && minn >= o.bkt6_min_run ? 6 : 7;
        if (x.bkt != planes) return fail("paid planes", l, 0);
        if (x.nib != 0) return fail("nib beside bkt", l, 0);
        if (x.slots != slots) return fail("the launch's slots", l, 0);
        if (x.wgs != wgs_streaming(o, max_slots, max_slots, (size_t)y.nitems, true) || x.wgs < 1 || (uint64_t)x.wgs > max_slots / kSplitTile)
            return fail("workgroups are not derived from the slots", l, 0);
        for (int r = 0; r < y.nitems; ++r, ++nruns) {
            ScanItem a = A.all_items[x.first + r];
            const ScanItem& t = B.all_items[y.first + r];
            if (a.n != want_slots[r] || a.n % kSplitTile != 0) return fail("slot count", l, r);
            if (a.split != want_tiles[r] || a.codes != want_side[r]) return fail("tile pointers", l, r);
            a.n = t.n;
            a.split = t.split;
            a.codes = t.codes;
            if (!same_item(a, t)) return fail("the run's other fields", l, r);
        }
    }
    printf("ok %zu %zu %zu\n", A.launches.size(), nbkt, nruns);
    return 0;
}
