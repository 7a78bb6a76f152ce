// Empty-cluster repair of PQ training: the launch geometry and the scratch of csrc/qadc_pq_repair_kernel.hip —
// HIP-free C++14, so that every shape's grid and byte count can be swept on the CPU (tests/cpp/pq_repair_plan_host.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace qadc {

constexpr int kPqRepairWG = 256;                  // threads of every workgroup
constexpr int kPqRepairRowTile = 1024;            // vectors per workgroup of the row kernels (keys, histogram, mark, rank)
constexpr int kPqRepairUnitTile = 4096;           // code units per workgroup of the count and rewrite kernels
constexpr int kPqRepairMaxSq = 32;
constexpr uint32_t kPqRepairLdsBytes = 32768;     // the count kernel keeps count and first of every sub-space in LDS up to this
constexpr int kPqRepairDigits = 8;                // 8-bit digits of a key, most significant first

// per sub-space control words in device memory (zeroed at the start of a round)
struct PqRepairCtl {
    uint32_t E;                                   // empty clusters
    uint32_t eligible;                            // vectors with a key > 0
    uint32_t want;                                // the rank still looked for among the keys under `prefix`; 0: nothing is chosen
    uint32_t moved;                               // vectors chosen = clusters filled
    uint64_t prefix;                              // the digits of the threshold found so far
    uint64_t threshold;                           // chosen <=> key >= threshold and key != 0
};

struct PqRepairPlan {
    int sq_count, sq_bits, dim, dsub;
    uint32_t K;                                   // 2^sq_bits
    uint64_t n;
    uint32_t units_per_row;                       // code units of a vector: bytes at 4 and 8 bits, uint16 at 16
    uint32_t unit_bytes;
    uint64_t units;                               // n * units_per_row
    uint32_t row_blocks;                          // ceil(n / kPqRepairRowTile): grid.x of the row kernels, grid.y = sq_count
    uint32_t unit_blocks;                         // ceil(units / kPqRepairUnitTile): the grid of the count and rewrite kernels
    int count_in_lds;                             // count and first accumulate in LDS, then one global atomic per touched cluster
    uint32_t count_lds_bytes;
    // scratch, in bytes.  zero_bytes are cleared at the start of every round, first_bytes set to 0xFF.
    size_t ctl_bytes, hist_bytes, count_bytes, first_bytes, empties_bytes, blockcnt_bytes, key_bytes;
    size_t total_bytes;
};

// false: a shape the kernels do not take (the caller refuses it before the first HIP call)
inline bool pq_repair_plan(uint64_t n, int dim, int sq_count, int sq_bits, PqRepairPlan* p) {
    if (sq_bits != 4 && sq_bits != 8 && sq_bits != 16) return false;
    if (sq_count < 1 || sq_count > kPqRepairMaxSq || (sq_bits == 4 && sq_count % 2)) return false;
    if (dim <= 0 || dim % sq_count) return false;
    if (n == 0 || n >= (1ull << 32)) return false;
    p->sq_count = sq_count;
    p->sq_bits = sq_bits;
    p->dim = dim;
    p->dsub = dim / sq_count;
    p->K = 1u << sq_bits;
    p->n = n;
    p->units_per_row = sq_bits == 4 ? (uint32_t)sq_count / 2 : (uint32_t)sq_count;
    p->unit_bytes = sq_bits == 16 ? 2 : 1;
    p->units = n * p->units_per_row;
    p->row_blocks = (uint32_t)((n + kPqRepairRowTile - 1) / kPqRepairRowTile);
    p->unit_blocks = (uint32_t)((p->units + kPqRepairUnitTile - 1) / kPqRepairUnitTile);
    const size_t SK = (size_t)sq_count * p->K;
    p->count_lds_bytes = (uint32_t)(SK * 2 * sizeof(uint32_t) <= kPqRepairLdsBytes ? SK * 2 * sizeof(uint32_t) : 0);
    p->count_in_lds = p->count_lds_bytes != 0;
    p->ctl_bytes = (size_t)kPqRepairMaxSq * sizeof(PqRepairCtl);
    p->hist_bytes = (size_t)sq_count * 256 * sizeof(uint32_t);
    p->count_bytes = SK * sizeof(uint32_t);
    p->first_bytes = SK * sizeof(uint32_t);
    p->empties_bytes = SK * sizeof(uint32_t);
    p->blockcnt_bytes = (size_t)sq_count * p->row_blocks * sizeof(uint32_t);
    p->key_bytes = (size_t)sq_count * n * sizeof(uint64_t);
    p->total_bytes = p->ctl_bytes + p->hist_bytes + p->count_bytes + p->first_bytes + p->empties_bytes + p->blockcnt_bytes + p->key_bytes;
    return true;
}

}  // namespace qadc
