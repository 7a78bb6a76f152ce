// Empty-cluster repair of PQ training.  Internal header shared by csrc/qadc_pq_repair_kernel.hip,
// csrc/qadc_build.cpp and csrc/qadc_opq.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../host/pq_repair_plan.hpp"

namespace qadc {

// the device state of a repair; every array is per sub-space m, in this order of m
struct PqRepairState {
    const float* x;              // [n][dim] the learning set as the quantizer sees it (read only)
    const float* cb;             // [S][K][dsub] the codebooks the assignment used (read only)
    void* codes;                 // [n] codes in the encoder's layout, rewritten in place
    uint8_t* zeroed;             // one block cleared at the start of a round: ctl, any_moved, hist, count
    size_t zeroed_bytes;
    PqRepairCtl* ctl;            // [kPqRepairMaxSq]
    uint32_t* any_moved;         // 1 word: some sub-space moved a vector in this round
    uint32_t* hist;              // [S][256]
    uint32_t* count;             // [S][K]
    uint32_t* first;             // [S][K], 0xFFFFFFFF at the start of a round
    uint32_t* empties;           // [S][K]: the first E[m] entries of row m
    uint32_t* blockcnt;          // [S][row_blocks]
    unsigned long long* keys;    // [S][n]
    unsigned long long* moved_total;   // [S]: moves of all rounds (cleared by the caller once)
};

constexpr size_t kPqRepairAnyBytes = 64;
inline size_t pq_repair_zeroed_bytes(const PqRepairPlan& p) { return p.ctl_bytes + kPqRepairAnyBytes + p.hist_bytes + p.count_bytes; }
// zeroed: a device block of pq_repair_zeroed_bytes(p), 16-byte aligned
inline void pq_repair_bind_zeroed(PqRepairState& st, const PqRepairPlan& p, void* zeroed) {
    st.zeroed = static_cast<uint8_t*>(zeroed);
    st.zeroed_bytes = pq_repair_zeroed_bytes(p);
    st.ctl = reinterpret_cast<PqRepairCtl*>(st.zeroed);
    st.any_moved = reinterpret_cast<uint32_t*>(st.zeroed + p.ctl_bytes);
    st.hist = reinterpret_cast<uint32_t*>(st.zeroed + p.ctl_bytes + kPqRepairAnyBytes);
    st.count = reinterpret_cast<uint32_t*>(st.zeroed + p.ctl_bytes + kPqRepairAnyBytes + p.hist_bytes);
}

// One repair of st.codes under st.cb, all sub-spaces in the same launches: count and first by integer atomics, the ordered list of
// the empties, the keys, the E-th largest key by eight radix passes (a histogram and a pick launch each), the ordered compaction of
// the chosen vectors (block counts, a scan, ballot ranks) and the rewrite, owned per code unit.  E[m] stays in device memory: every
// launch after the list returns at once for a sub-space with E[m] == 0, and the rewrite when nothing moved.  ctl[m].moved holds the
// round's moves and moved_total[m] grows by them.  Queued on `stream`; nothing waits for the device.
hipError_t launch_pq_repair(const PqRepairState& st, const PqRepairPlan& plan, hipStream_t stream);

}  // namespace qadc
