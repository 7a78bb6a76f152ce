// The append planner of the float-ADC engine: where the partitions of an owned index lie after rows are
// added to them.  Integer arithmetic on sizes and capacities only.  No HIP here: the flow both engines share (csrc/qadc_append.h)
// plans every add_vectors pass and every reserve with plan_append and takes a pass's row bases from append_bases, and
// tests/cpp/adc_append_plan_host.cpp checks the layout's invariants and the bases on a CPU.
//
// Layout: partition p owns cap[p] code rows at byte offset off[p] of the code buffer and cap[p] labels from label lab_off[p];
// regions follow one another in partition order, each code region is align16(cap[p] * code_size) bytes — so every partition
// starts on a 16-byte boundary — and the code buffer ends in kAppendTailPad bytes that belong to no partition.  The scan kernels
// read whole 16-byte words up to the end of a partition's last row, which stays inside the region or the padding.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace qadc {
namespace adc {

constexpr uint64_t kAppendTailPad = 16;          // bytes after the last region
constexpr uint64_t kAppendMaxRows = 0xffffffffull;   // rows of one partition (positions and counts are 32-bit)

inline uint64_t append_align16(uint64_t v) { return (v + 15) / 16 * 16; }

struct AppendPlan {
    std::string refused;            // not empty: nothing may be appended, and why (nothing below is filled)
    bool in_place = true;           // every addition fits its partition's capacity: cap / off / lab_off are the old ones
    std::vector<uint32_t> cap;      // [parts] rows every partition may hold
    std::vector<uint64_t> off;      // [parts] byte offset of the partition's codes
    std::vector<uint64_t> lab_off;  // [parts] first label of the partition
    uint64_t code_bytes = 0;        // bytes of all regions (the buffer holds kAppendTailPad more)
    uint64_t label_count = 0;       // labels of all regions
};

// Regions of the given capacities, back to back.  region_pad: bytes every code region holds behind its rows (a multiple of 16;
// 0 here, host/index_append_plan.hpp has the 4-bit index's).
inline void append_layout(int code_size, AppendPlan* p, uint64_t region_pad = 0) {
    uint64_t bytes = 0, labels = 0;
    const size_t parts = p->cap.size();
    p->off.resize(parts);
    p->lab_off.resize(parts);
    for (size_t i = 0; i < parts; ++i) {
        p->off[i] = bytes;
        p->lab_off[i] = labels;
        bytes += append_align16((uint64_t)p->cap[i] * code_size) + region_pad;
        labels += p->cap[i];
    }
    p->code_bytes = bytes;
    p->label_count = labels;
}

// sizes / caps [parts]: rows held and rows allocated now (caps[p] >= sizes[p]); add [parts]: rows to append to each partition;
// floor [parts] or null: capacities asked for (qadc_adc_index_reserve).  In place when sizes[p] + add[p] <= caps[p] and
// floor[p] <= caps[p] everywhere.  Otherwise the database moves: with `grow` every partition gets at least 1.5 times its new
// size — one 16-byte word of rows at least, so that a first row does not relocate twice — and without it (a reserve) exactly
// what is needed; never less than its old capacity or its floor; rounded up to the rows its 16-byte-aligned region holds anyway,
// and never more than 2^32 - 1 rows.
inline AppendPlan plan_append(int code_size, size_t parts, const uint32_t* sizes, const uint32_t* caps, const uint64_t* add,
                              const uint32_t* floor, bool grow, uint64_t region_pad = 0) {
    AppendPlan p;
    bool fits = true;
    for (size_t i = 0; i < parts; ++i) {
        const uint64_t total = (uint64_t)sizes[i] + add[i];
        if (add[i] > kAppendMaxRows || total > kAppendMaxRows) {
            p.refused = "partition " + std::to_string(i) + " would hold " + std::to_string(total) + " codes: at most 2^32 - 1 per partition";
            return p;
        }
        if (total > caps[i] || (floor && floor[i] > caps[i])) fits = false;
    }
    p.cap.assign(caps, caps + parts);
    if (fits) {
        append_layout(code_size, &p, region_pad);
        return p;
    }
    p.in_place = false;
    const uint64_t word_rows = 16 / (uint64_t)code_size ? 16 / (uint64_t)code_size : 1;
    for (size_t i = 0; i < parts; ++i) {
        const uint64_t total = (uint64_t)sizes[i] + add[i];
        uint64_t want = std::max<uint64_t>(caps[i], total);
        if (floor) want = std::max<uint64_t>(want, floor[i]);
        if (grow) want = std::max<uint64_t>(want, std::max<uint64_t>(total + (total + 1) / 2, word_rows));
        want = append_align16(want * code_size) / code_size;   // the rows the aligned region holds
        p.cap[i] = (uint32_t)std::min<uint64_t>(want, kAppendMaxRows);
    }
    append_layout(code_size, &p, region_pad);
    return p;
}

// The bases of one add_vectors pass: sizes [parts] rows held, count [parts] rows the pass adds to each partition.  The scatter
// kernel (launch_adc_add_scatter) writes the vector at position j of the pass's (assign, i) order to row base[assign] + j, so
// base[p] is sizes[p] less the vectors of the partitions below p — modulo 2^32, as the kernel adds.
inline void append_bases(size_t parts, const uint32_t* sizes, const uint32_t* count, uint32_t* base) {
    uint32_t below = 0;
    for (size_t p = 0; p < parts; ++p) {
        base[p] = sizes[p] - below;
        below += count[p];
    }
}

}  // namespace adc
}  // namespace qadc
