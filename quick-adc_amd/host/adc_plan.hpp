// The level planner of the float-ADC engine: integer arithmetic on the partition sizes and the probe lists of
// a batch, on which every exactness argument of that section rests.  No HIP here: csrc/qadc_adc_kernels.h includes this header for
// Item, csrc/qadc_adc.cpp plans every batch with plan_levels, and tests/cpp/adc_plan_host.cpp checks the plan's invariants on a CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace qadc {
namespace adc {

constexpr uint32_t kLevel0 = 512;      // codes of level 0 (at least R)
constexpr uint32_t kLevelGrowth = 16;  // each level spans 16 times the scan order before it
constexpr uint32_t kWgTarget = 2048;   // workgroups a level is cut into, roughly
constexpr uint32_t kRunMin = 2048, kRunMax = 65536;

inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// One contiguous run of codes of one probed partition, scanned with the table of (query, slot).
struct Item {
    uint32_t query;
    uint32_t slot;    // position in assign[query][0 .. ma)
    uint32_t start;   // first code of the run, position inside the partition
    uint32_t count;   // codes in the run
    uint32_t sbase;   // scan-order index of the run's first code within its query (probe slots in assign[] order, then position)
    uint32_t pad[3];
};

struct Plan {
    std::string refused;                // not empty: the batch is not scanned, and why (nothing below is filled)
    std::vector<uint64_t> total;        // [nq] scan-order length of every query
    uint64_t max_total = 0;
    std::vector<uint64_t> edge;         // [levels + 1] level l is [edge[l], edge[l + 1]) of every query's scan order
    std::vector<Item> items;            // the runs of level 0, then of level 1, ...; within a level query by query in scan order
    std::vector<uint32_t> level_first;  // [levels + 1] first item of each level; the last = items.size()
    std::vector<uint32_t> cap;          // [nq] entries of each query's candidate region
    int levels() const { return (int)edge.size() - 1; }
};

// sizes[part] = codes of each partition; assign [nq][ma] = the partitions every query probes, in scan order.
inline Plan plan_levels(const uint32_t* sizes, int nq, int ma, const int32_t* assign, int R) {
    Plan p;
    p.total.assign(nq, 0);
    for (int q = 0; q < nq; ++q) {
        for (int a = 0; a < ma; ++a) p.total[q] += sizes[assign[(size_t)q * ma + a]];
        if (p.total[q] > 0xffffffffull) {
            p.refused = "query " + std::to_string(q) + " probes " + std::to_string(p.total[q]) + " codes: at most 2^32 - 1 per query";
            return p;
        }
        p.max_total = std::max(p.max_total, p.total[q]);
    }
    p.edge = {0, std::max<uint64_t>((uint64_t)R, kLevel0)};
    while (p.edge.back() < p.max_total) p.edge.push_back(p.edge.back() * kLevelGrowth);
    const int levels = p.levels();
    // the runs of every level: per query, the level's stretch of the scan order cut at partition ends and into runs
    for (int l = 0; l < levels; ++l) {
        p.level_first.push_back((uint32_t)p.items.size());
        uint64_t span = 0;
        for (int q = 0; q < nq; ++q)
            if (p.total[q] > p.edge[l]) span += std::min(p.total[q], p.edge[l + 1]) - p.edge[l];
        const uint64_t run = std::min<uint64_t>(kRunMax, std::max<uint64_t>(kRunMin, align_up((span + kWgTarget - 1) / kWgTarget, 1024)));
        for (int q = 0; q < nq; ++q) {
            const uint64_t lo = p.edge[l], hi = std::min(p.total[q], p.edge[l + 1]);
            uint64_t pbase = 0;
            for (int a = 0; a < ma && pbase < hi; ++a) {
                const uint64_t sz = sizes[assign[(size_t)q * ma + a]];
                const uint64_t s0 = std::max(lo, pbase), s1 = std::min(hi, pbase + sz);
                for (uint64_t s = s0; s < s1; s += run) {
                    Item it{};
                    it.query = (uint32_t)q;
                    it.slot = (uint32_t)a;
                    it.start = (uint32_t)(s - pbase);
                    it.count = (uint32_t)std::min<uint64_t>(run, s1 - s);
                    it.sbase = (uint32_t)s;
                    p.items.push_back(it);
                }
                pbase += sz;
            }
        }
    }
    p.level_first.push_back((uint32_t)p.items.size());
    // Per-query regions: the expected stream (level 0 whole, then ~15 R per level) with room to spare, at most the query's
    // code count.  They are sized per call, so nothing one call needed carries over to the next.
    const uint64_t expect = std::max<uint64_t>((uint64_t)R, kLevel0) + 32ull * R * (levels - 1) + 4096;
    p.cap.resize(nq);
    for (int q = 0; q < nq; ++q) p.cap[q] = (uint32_t)std::max<uint64_t>(1, std::min(p.total[q], expect));
    return p;
}

// ---- range search: one level over every query's whole scan order, scanned under a bound that never moves ----
constexpr uint32_t kRangeFirstCap = 4096;   // entries of a query's region in the first attempt (at most its code count)

// Adds up the regions of `cap`; refuses (not empty: why) above max_entries.
inline std::string range_entries(const std::vector<uint32_t>& cap, uint64_t max_entries, uint64_t* entries) {
    uint64_t n = 0;
    for (uint32_t c : cap) n += c;
    *entries = n;
    if (n > max_entries)
        return "the result regions of this pass need " + std::to_string(n) + " entries (at most " + std::to_string(max_entries) +
               "): split the batch or lower the radii";
    return std::string();
}

// The plan of a range pass: ONE level [0, max_total) whose runs are cut the way plan_levels cuts a level, and a first-attempt region of
// min(total[q], kRangeFirstCap) entries per query (0 for a query that probes no code).  Refuses like plan_levels above 2^32 - 1 codes
// per query.
inline Plan plan_range(const uint32_t* sizes, int nq, int ma, const int32_t* assign) {
    Plan p;
    p.total.assign(nq, 0);
    uint64_t span = 0;
    for (int q = 0; q < nq; ++q) {
        for (int a = 0; a < ma; ++a) p.total[q] += sizes[assign[(size_t)q * ma + a]];
        if (p.total[q] > 0xffffffffull) {
            p.refused = "query " + std::to_string(q) + " probes " + std::to_string(p.total[q]) + " codes: at most 2^32 - 1 per query";
            return p;
        }
        p.max_total = std::max(p.max_total, p.total[q]);
        span += p.total[q];
    }
    p.edge = {0, std::max<uint64_t>(p.max_total, 1)};
    const uint64_t run = std::min<uint64_t>(kRunMax, std::max<uint64_t>(kRunMin, align_up((span + kWgTarget - 1) / kWgTarget, 1024)));
    p.level_first.push_back(0);
    for (int q = 0; q < nq; ++q) {
        uint64_t pbase = 0;
        for (int a = 0; a < ma; ++a) {
            const uint64_t sz = sizes[assign[(size_t)q * ma + a]];
            for (uint64_t s = 0; s < sz; s += run) {
                Item it{};
                it.query = (uint32_t)q;
                it.slot = (uint32_t)a;
                it.start = (uint32_t)s;
                it.count = (uint32_t)std::min<uint64_t>(run, sz - s);
                it.sbase = (uint32_t)(pbase + s);
                p.items.push_back(it);
            }
            pbase += sz;
        }
    }
    p.level_first.push_back((uint32_t)p.items.size());
    p.cap.resize(nq);
    for (int q = 0; q < nq; ++q) p.cap[q] = (uint32_t)std::min<uint64_t>(p.total[q], kRangeFirstCap);
    return p;
}

// After an attempt: count[q] = rows query q emitted, counted past its region too.  Radius and filters are fixed, so the count is exact
// and the re-run's region holds exactly that many: a pass scans at most twice.  True: a region overflowed and the pass must re-run.
inline bool plan_range_rerun(Plan& p, const uint32_t* count) {
    bool overflow = false;
    for (size_t q = 0; q < p.cap.size(); ++q)
        if (count[q] > p.cap[q]) {
            overflow = true;
            p.cap[q] = count[q];   // (<= total[q]: a row is counted once)
        }
    return overflow;
}

}  // namespace adc
}  // namespace qadc
