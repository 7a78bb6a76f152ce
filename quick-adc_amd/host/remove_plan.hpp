// The planner of remove-by-label: what qadc_adc_index_remove_labels and qadc_index_remove_labels decide on
// the host between their kernels.  Integer arithmetic only, no HIP: csrc/qadc_remove.h plans every call with it, and
// tests/cpp/remove_plan_host.cpp checks it on a CPU.
//
// A call marks the labels of its list in a bitmap over [lo, hi], the smallest and largest of them (remove_span), counts per
// partition the rows whose label is marked and the first tile that holds one (hits[], first[]: remove_count_kernel), and compacts
// every partition that was hit, from that tile on, in place (plan_remove: one RemoveEntry per touched partition).  On the 4-bit
// index the bytes [n' * cs, align16(n' * cs) + 64) behind the new last row are zeroed again — host/index_append_plan.hpp's rule,
// the one the append path keeps.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "index_append_plan.hpp"

namespace qadc {
namespace adc {

// The bitmap of a list whose labels lie in [lo, hi]: bit i stands for label lo + i.
struct RemoveSpan {
    uint32_t lo = 0;
    uint32_t last = 0;    // hi - lo: the largest bit of the span (a label l is inside when l - lo <= last, modulo 2^32)
    uint64_t bits = 0;    // hi - lo + 1: up to 2^32
    uint64_t words = 0;   // 32-bit words that hold them: up to 2^27 (512 MiB)
};

inline RemoveSpan remove_span(uint32_t lo, uint32_t hi) {
    RemoveSpan s;
    s.lo = lo;
    s.last = hi - lo;
    s.bits = (uint64_t)hi - lo + 1;
    s.words = (s.bits + 31) / 32;
    return s;
}

// One touched partition: the rows it holds, the tile the compaction starts at (every row before it stays where it is), the rows
// it keeps, and the bytes [zero_first, zero_last) behind them that are zeroed (an empty span where the engine keeps none).
struct RemoveEntry {
    uint32_t part = 0;
    uint32_t n = 0;
    uint32_t first_tile = 0;
    uint32_t n_new = 0;
    uint64_t zero_first = 0, zero_last = 0;
};

struct RemovePlan {
    std::vector<RemoveEntry> touched;   // in partition order
    std::vector<uint32_t> sizes;        // [parts] rows every partition holds after the call
    uint64_t removed = 0;
};

// sizes [parts]: rows held; hits [parts]: rows of each partition whose label is in the list; first [parts]: the first tile of
// `tile` rows with such a row (anything where hits is 0).  A partition is touched when it holds rows and was hit.  zero_tail: the
// 4-bit index's zeroed span behind the new end (index_zero_span).
inline RemovePlan plan_remove(int code_size, size_t parts, const uint32_t* sizes, const uint32_t* hits, const uint32_t* first, uint32_t tile,
                              bool zero_tail) {
    RemovePlan p;
    p.sizes.assign(sizes, sizes + parts);
    for (size_t i = 0; i < parts; ++i) {
        if (sizes[i] == 0 || hits[i] == 0) continue;
        RemoveEntry e;
        e.part = (uint32_t)i;
        e.n = sizes[i];
        e.first_tile = std::min(first[i], (sizes[i] - 1) / tile);   // never past the last tile
        e.n_new = sizes[i] - std::min(hits[i], sizes[i]);
        if (zero_tail) index_zero_span(e.n_new, code_size, &e.zero_first, &e.zero_last);
        p.sizes[i] = e.n_new;
        p.removed += e.n - e.n_new;
        p.touched.push_back(e);
    }
    return p;
}

}  // namespace adc
}  // namespace qadc
