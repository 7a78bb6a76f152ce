// The append planner of the 4-bit index: where the partitions of a qadc_index lie once they live in the
// index's arena and rows are added to them.  Integer arithmetic only, no HIP: the shared flow (csrc/qadc_append.h) plans every
// qadc_index_add_vectors pass and every qadc_index_reserve with plan_append at region_pad = kIndexRegionPad — plan_index_append
// here — and tests/cpp/index_append_plan_host.cpp checks the layout's invariants on a CPU.
//
// Layout: the one of host/adc_append_plan.hpp — partition p owns cap[p] >= n rows at byte offset off[p] of the code arena and
// cap[p] labels from label lab_off[p] of the label arena, regions back to back in partition order, capacities by plan_append's
// rule (1.5 times the new size, one 16-byte word of rows at least, never less than the old capacity or a reserve, a reserve
// applied exactly) — with what a partition of qadc_index_add_partitions has behind its rows (alloc_part, csrc/qadc_capi.cpp):
// every code region is align16(cap[p] * code_size) + kIndexRegionPad bytes, so it starts 16-byte aligned and is readable to
// align16(cap * cs) + 64 bytes, and bytes [n * cs, align16(n * cs) + 64) of it — the unused half of the last row's 16-byte word
// and 64 bytes more, the "80 bytes" alloc_part clears from 16 bytes before the end — are zero whenever a call returns
// (index_zero_span).  The scan kernels read whole 16-byte words up to align16(n * cs); DESIGN.md section 11.6 lists what was read.
//
// A relocation allocates the new arena, moves every partition by one kernel, and only then frees the old storage: while it runs
// the device holds the old and the new database at once.
#pragma once
#include "adc_append_plan.hpp"

namespace qadc {
namespace adc {

constexpr uint64_t kIndexRegionPad = 64;   // bytes behind the rows of every code region

// The end of what lies behind `bytes` bytes of rows: the 16-byte word they end in, and the pad.  With bytes = cap * code_size the
// length of a region; with bytes = n * code_size the end of the span kept zero behind the last row.  constexpr: the kernels that
// zero the span (index_move_kernel, index_zero_tails_kernel in csrc/qadc_adc_kernel.hip) and the planner share this one rule.
constexpr uint64_t index_padded_end(uint64_t bytes) { return (bytes + 15) / 16 * 16 + kIndexRegionPad; }

inline AppendPlan plan_index_append(int code_size, size_t parts, const uint32_t* sizes, const uint32_t* caps, const uint64_t* add,
                                    const uint32_t* floor, bool grow) {
    return plan_append(code_size, parts, sizes, caps, add, floor, grow, kIndexRegionPad);
}

// bytes of the code region of a partition of capacity `cap`
inline uint64_t index_region_bytes(uint64_t cap, int code_size) { return index_padded_end(cap * code_size); }

// the bytes [first, last) behind the last of n rows that are kept zero
inline void index_zero_span(uint64_t n, int code_size, uint64_t* first, uint64_t* last) {
    *first = n * code_size;
    *last = index_padded_end(n * code_size);
}

}  // namespace adc
}  // namespace qadc
