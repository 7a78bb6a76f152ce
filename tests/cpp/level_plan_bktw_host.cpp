// CPU check of the planner's wide-form fields (host/level_plan.hpp; tests/test_level_plan_bktw_host.py).  Every case plans one batch
// twice: over partitions whose bucket copy has wide octaves from W on ("with") and over the same partitions without any copy
// ("today").  No HIP, no library: partition "pointers" are fake bases, slot offsets are made up (whole tiles, growing unevenly).
// Octave j of a partition is stored wide unless bit j of the fallback mask is set; a narrow block inside a wide octave is empty.
// Checked per launch, which both plans have in the same order, with every run's qualification restated here from today's plan:
//   - LevelLaunch::bktw is non-zero exactly when the launch is split and not shared and every run starts on an octave, ends on one or
//     at the partition's end, covers only octaves stored wide and has bktw_min_run codes; then bktw = the fewest paid planes whose
//     threshold the shortest run reaches, bkt and nib are 0, every run's n = the slots between the octaves' offsets, split / codes =
//     that tile of the wide copy (kBktwTileBytes) and of its side array, the other fields, codes and maxn are today's, slots = the
//     runs' slots and wgs derives from them;
//   - else LevelLaunch::bkt is non-zero exactly when every run covers whole narrow blocks, has bkt_min_run codes and meets no octave
//     stored wide; its runs point into the narrow copy (kBktTileBytes);
//   - every other launch, and every one of its runs, equals today's field for field (a launch that mixes wide, narrow and other
//     runs falls back).
// argv: sizes "n0,n1,..", block, W, fallback mask, level_base, level_growth, head_level, bktw_min_run, bktw5, bktw4, bktw3, nq,
// orders "p p p;p p p", small_run, share_variant.  stdout: "ok <launches> <wide launches> <wide runs> <narrow launches> <paid planes
// of the wide launches, in order, as digits>", or a line that starts with "FAIL".
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
    if (argc != 16) return 2;
    std::vector<uint64_t> sizes;
    {
        std::stringstream ss(argv[1]);
        std::string tok;
        while (std::getline(ss, tok, ',')) sizes.push_back(strtoull(tok.c_str(), nullptr, 10));
    }
    const uint64_t block = strtoull(argv[2], nullptr, 10), W = strtoull(argv[3], nullptr, 10), fallback = strtoull(argv[4], nullptr, 10);
    LevelOptions o{16, strtoull(argv[5], nullptr, 10), strtoull(argv[6], nullptr, 10), atoi(argv[7]), (uint32_t)strtoul(argv[14], nullptr, 10), 0,
                   atoi(argv[15]), 1, 1u << 16, 1, 1, 1, 1, 0, 9};
    o.bkt_min_run = 1;
    o.bkt6_min_run = 1;
    o.bktw_min_run = strtoull(argv[8], nullptr, 10);
    o.bktw5_min_run = strtoull(argv[9], nullptr, 10);
    o.bktw4_min_run = strtoull(argv[10], nullptr, 10);
    o.bktw3_min_run = strtoull(argv[11], nullptr, 10);
    const int nq = atoi(argv[12]);
    std::vector<int32_t> assign;
    {
        std::stringstream ss(argv[13]);
        std::string q;
        while (std::getline(ss, q, ';')) {
            std::stringstream qs(q);
            int p;
            while (qs >> p) assign.push_back(p);
        }
    }
    if (nq <= 0 || assign.size() % (size_t)nq != 0 || W % block != 0) return 2;
    const int ma = (int)(assign.size() / (size_t)nq);
    std::vector<LevelPart> with(sizes.size()), today(sizes.size());
    // per partition: [lo, hi) of every octave, and whether it is stored wide
    std::vector<std::vector<uint64_t>> olo(sizes.size()), ohi(sizes.size());
    std::vector<std::vector<bool>> owide(sizes.size());
    for (size_t i = 0; i < sizes.size(); ++i) {
        LevelPart& p = with[i];
        p.d_codes = reinterpret_cast<uint8_t*>((uintptr_t)((8 * i + 1) << 40));
        p.d_split = reinterpret_cast<uint8_t*>((uintptr_t)((8 * i + 2) << 40));
        p.d_nib = reinterpret_cast<uint8_t*>((uintptr_t)((8 * i + 3) << 40));
        p.n = p.global_n = (uint32_t)sizes[i];
        p.start_n = std::max<uint32_t>(1, p.n / 100);
        today[i] = p;
        p.d_bkt = reinterpret_cast<uint8_t*>((uintptr_t)((8 * i + 4) << 40));
        p.d_bkt_side = reinterpret_cast<uint8_t*>((uintptr_t)((8 * i + 5) << 40));
        p.d_bktw = reinterpret_cast<uint8_t*>((uintptr_t)((8 * i + 6) << 40));
        p.d_bktw_side = reinterpret_cast<uint8_t*>((uintptr_t)((8 * i + 7) << 40));
        p.bkt_block = block;
        p.bktw_block = W;
        p.bktw_off.push_back(0);
        for (uint64_t lo = W, j = 0; W && lo < p.n; lo *= 2, ++j) {
            const uint64_t hi = std::min<uint64_t>(2 * lo, p.n);
            const bool wide = !((fallback >> j) & 1);
            olo[i].push_back(lo);
            ohi[i].push_back(hi);
            owide[i].push_back(wide);
            p.bktw_off.push_back(p.bktw_off.back() + (wide ? (hi - lo + (j % 3) * 900 + kSplitTile - 1) / kSplitTile * kSplitTile + (j % 2) * kSplitTile : 0));
        }
        if (p.bktw_off.back() == 0) {                            // no octave stored wide: no wide copy
            p.d_bktw = p.d_bktw_side = nullptr;
            p.bktw_block = 0;
            p.bktw_off.clear();
        }
        p.bkt_off.push_back(0);
        for (uint64_t b0 = 0, b = 0; b0 < p.n; b0 += block, ++b) {
            const uint64_t nb = std::min<uint64_t>(block, p.n - b0);
            bool covered = false;
            for (size_t j = 0; j < olo[i].size(); ++j) covered = covered || (owide[i][j] && b0 >= olo[i][j] && b0 < ohi[i][j]);
            p.bkt_off.push_back(p.bkt_off.back() + (covered ? 0 : (nb + (b % 3) * 1000 + kSplitTile - 1) / kSplitTile * kSplitTile + (b % 2) * kSplitTile));
        }
    }
    const LevelBatch b{nq, ma, assign.data(), 100, 0, true, false, 0, 1, 0};
    const BatchPlan A = plan_levels(with.data(), with.size(), o, b), B = plan_levels(today.data(), today.size(), o, b);
    if (!A.refused.empty() || !B.refused.empty()) return fail("refused", 0, 0);
    if (A.launches.size() != B.launches.size() || A.all_items.size() != B.all_items.size()) return fail("launch or run count differs", 0, 0);
    size_t nwide = 0, nruns = 0, nnarrow = 0;
    std::string planes_seen;
    for (size_t l = 0; l < A.launches.size(); ++l) {
        const LevelLaunch &x = A.launches[l], &y = B.launches[l];
        if (x.first != y.first || x.nitems != y.nitems || x.small != y.small || x.shared != y.shared || x.mq != y.mq || x.split != y.split ||
            x.split6 != y.split6 || x.split5 != y.split5 || x.codes != y.codes || x.maxn != y.maxn || x.early != y.early || y.bkt != 0 ||
            y.bktw != 0 || y.slots != 0)
            return fail("launch fields that no form may change", l, 0);
        bool all_wide = y.split && !y.shared && o.bktw_min_run != 0, all_narrow = y.split && !y.shared;
        uint64_t minn = ~0ull, slots = 0, max_slots = 0;
        std::vector<uint64_t> want_slots((size_t)y.nitems);
        std::vector<const uint8_t*> want_tiles((size_t)y.nitems), want_side((size_t)y.nitems);
        for (int r = 0; r < y.nitems; ++r) {
            const ScanItem& it = B.all_items[y.first + r];
            const size_t pi = (size_t)((uintptr_t)it.codes >> 40) / 8;
            const LevelPart& p = with[pi];
            const uint64_t b0 = it.pos0, e = b0 + it.n;
            // wide: whole octaves, all of them stored wide
            bool starts = false, ends = false, only_wide = true, meets_wide = false;
            uint64_t s0 = 0, s1 = 0;
            for (size_t j = 0; j < olo[pi].size(); ++j) {
                if (olo[pi][j] == b0) { starts = true; s0 = p.bktw_off[j]; }
                if (ohi[pi][j] == e) { ends = true; s1 = p.bktw_off[j + 1]; }
                const bool overlap = b0 < ohi[pi][j] && e > olo[pi][j];
                if (overlap && !owide[pi][j]) only_wide = false;
                if (overlap && owide[pi][j]) meets_wide = true;
            }
            const bool wide_ok = it.split && p.d_bktw && starts && ends && only_wide && it.n >= o.bktw_min_run;
            all_wide = all_wide && wide_ok;
            all_narrow = all_narrow && it.split && !meets_wide && b0 % block == 0 && (e % block == 0 || e == p.n);
            if (wide_ok) {
                want_slots[r] = s1 - s0;
                want_tiles[r] = p.d_bktw + s0 / kSplitTile * (uint64_t)kBktwTileBytes;
                want_side[r] = p.d_bktw_side + s0 / kSplitTile * (uint64_t)kBktSideBytes;
                slots += want_slots[r];
                max_slots = std::max(max_slots, want_slots[r]);
            }
            minn = std::min<uint64_t>(minn, it.n);
        }
        if ((x.bktw != 0) != all_wide) return fail("bktw set on a launch that does not qualify, or not set on one that does", l, 0);
        if (all_wide) {
            ++nwide;
            const int planes = o.bktw3_min_run && minn >= o.bktw3_min_run ? 3 : o.bktw4_min_run && minn >= o.bktw4_min_run ? 4
                               : o.bktw5_min_run && minn >= o.bktw5_min_run ? 5 : 6;
            planes_seen += (char)('0' + planes);
            if (x.bktw != planes) return fail("paid planes", l, 0);
            if (x.nib != 0 || x.bkt != 0) return fail("another form beside bktw", l, 0);
            if (x.slots != slots) return fail("the launch's slots", l, 0);
            if (x.wgs != wgs_streaming(o, max_slots, max_slots, (size_t)y.nitems, true) || x.wgs < 1 || (uint64_t)x.wgs > max_slots / kSplitTile)
                return fail("workgroups are not derived from the slots", l, 0);
            for (int r = 0; r < y.nitems; ++r, ++nruns) {
                ScanItem a = A.all_items[x.first + r];
                const ScanItem& t = B.all_items[y.first + r];
                if (a.n != want_slots[r] || a.n % kSplitTile != 0 || a.n == 0) return fail("slot count", l, r);
                if (a.split != want_tiles[r] || a.codes != want_side[r]) return fail("tile pointers", l, r);
                a.n = t.n;
                a.split = t.split;
                a.codes = t.codes;
                if (!same_item(a, t)) return fail("the run's other fields", l, r);
            }
            continue;
        }
        if ((x.bkt != 0) != all_narrow) return fail("bkt set over a wide octave or off the blocks, or not set on a narrow launch", l, 0);
        if (all_narrow) {
            ++nnarrow;
            for (int r = 0; r < y.nitems; ++r) {
                const ScanItem& a = A.all_items[x.first + r];
                const ScanItem& t = B.all_items[y.first + r];
                const LevelPart& p = with[(size_t)((uintptr_t)t.codes >> 40) / 8];
                const uint64_t s0 = p.bkt_off[t.pos0 / block], s1 = p.bkt_off[(t.pos0 + t.n + block - 1) / block];
                if (a.n != s1 - s0 || a.n == 0 || a.split != p.d_bkt + s0 / kSplitTile * (uint64_t)kBktTileBytes) return fail("narrow run", l, r);
            }
            continue;
        }
        if (x.nib != y.nib || x.wgs != y.wgs || x.slots != 0) return fail("a launch that does not qualify differs from today's", l, 0);
        for (int r = 0; r < y.nitems; ++r)
            if (!same_item(A.all_items[x.first + r], B.all_items[y.first + r])) return fail("a run that does not qualify differs from today's", l, r);
    }
    printf("ok %zu %zu %zu %zu %s\n", A.launches.size(), nwide, nruns, nnarrow, planes_seen.empty() ? "-" : planes_seen.c_str());
    return 0;
}
