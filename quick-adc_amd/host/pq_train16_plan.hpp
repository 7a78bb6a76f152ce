// Geometry of the sorted centroid update for 16-bit sub-quantizers (csrc/qadc_pq_train16_kernel.hip) —
// HIP-free, so that tests/cpp/pq_train16_host.cpp can check it on the CPU.
//
// Per sub-quantizer the vectors are sorted by (code, index) — two stable 8-bit radix passes over tiles of kPqTrain16Tile entries —
// and cluster k owns the run perm[start[k] .. start[k + 1]).  The walk gives every (cluster, window of `width` components) — a
// unit — to one group of `width` = min(dsub, 64) lanes: a lane owns ONE chain, component window * width + lane of cluster k, and
// adds its members in list order.  A wave holds 64 / width groups, a workgroup four waves; units are numbered cluster-major
// (unit = k * dblocks + window) and dealt to the groups in order.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define QADC_PLAN_HD __host__ __device__
#else
#define QADC_PLAN_HD
#endif

namespace qadc {

constexpr int kPqTrain16WG = 256;          // lanes of a workgroup = every kernel's __launch_bounds__
constexpr int kPqTrain16K = 65536;         // centroids per sub-quantizer
constexpr int kPqTrain16Tile = 1024;       // entries one workgroup of a radix pass ranks
constexpr int kPqTrain16Unroll = 4;        // list steps whose loads are issued before the first add
constexpr int kPqTrain16MaxDsub = 2048;    // = the 16-bit encoder's limit: kAdcMaxDim / 2
constexpr size_t kPqTrain16SortLds = (256 + 4 * 256) * sizeof(uint32_t);   // the scatter pass: a position per digit, a count per (wave, digit)

struct PqTrain16Plan {
    int dsub;
    int width;          // lanes of a group = components of one window: min(dsub, 64)
    int dblocks;        // windows per cluster: ceil(dsub / width)
    int wave_groups;    // groups per wave: 64 / width (the lanes beyond wave_groups * width idle)
    int wg_groups;      // groups per workgroup: 4 * wave_groups
    uint32_t units;     // 65536 * dblocks
    unsigned walk_grid; // ceil(units / wg_groups)
    size_t lds_bytes;   // the largest static LDS of the update's kernels (the walk itself keeps none)
};

// false: a shape the update does not take (the caller refuses it).
inline bool pq_train16_plan(int sq_count, int dim, PqTrain16Plan* p) {
    if ((sq_count != 2 && sq_count != 4 && sq_count != 8) || dim <= 0 || dim % sq_count != 0) return false;
    const int dsub = dim / sq_count;
    if (dsub > kPqTrain16MaxDsub) return false;
    p->dsub = dsub;
    p->width = dsub < 64 ? dsub : 64;
    p->dblocks = (dsub + p->width - 1) / p->width;
    p->wave_groups = 64 / p->width;
    p->wg_groups = (kPqTrain16WG / 64) * p->wave_groups;
    p->units = (uint32_t)kPqTrain16K * (uint32_t)p->dblocks;
    p->walk_grid = (p->units + (uint32_t)p->wg_groups - 1) / (uint32_t)p->wg_groups;
    p->lds_bytes = kPqTrain16SortLds;
    return true;
}

// The chain of lane `tid` of workgroup `block` of the walk: component d of cluster k, or none.
struct PqTrain16Owner {
    bool owns;
    uint32_t k;
    int d;
};

QADC_PLAN_HD inline PqTrain16Owner pq_train16_owner(int dsub, int width, int dblocks, int wave_groups, uint32_t block, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const int g = lane / width, l = lane - g * width;
    PqTrain16Owner o = {false, 0u, 0};
    if (g >= wave_groups) return o;
    const uint64_t unit = ((uint64_t)block * (kPqTrain16WG / 64) + (uint64_t)wave) * (uint64_t)wave_groups + (uint64_t)g;
    if (unit >= (uint64_t)kPqTrain16K * (uint64_t)dblocks) return o;
    o.k = (uint32_t)(unit / (uint64_t)dblocks);
    o.d = (int)(unit % (uint64_t)dblocks) * width + l;
    o.owns = o.d < dsub;
    return o;
}

}  // namespace qadc
