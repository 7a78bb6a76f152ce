// k-means++ seeding.  Internal header shared by csrc/qadc_kmeans_seed_kernel.hip and
// csrc/qadc_kmeans_seed.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../host/kmeans_seed_plan.hpp"

namespace qadc {

// the device state of a seeding run; every array is per sub-space m, in this order of m
struct KmeansSeedState {
    const float* x;          // [n][dim] the learning set as the quantizer sees it (read only)
    uint64_t n, k, seed;
    float* mind;             // [S][n]
    double* level1;          // [S][nodes[1]]
    double* level2;          // [S][nodes[2]]
    double* upper;           // [S][upper_nodes]: levels 3..root
    uint32_t* picked;        // [S][bitmap_words], zero at the start
    uint32_t* cursor;        // [S], zero at the start
    unsigned long long* fallbacks;   // [S], zero at the start
    float* centres;          // [S][k][dsub]
    uint32_t* rows;          // [S][k]
};

// round t >= 1, first launch: mind = min(mind, distance to centre t - 1) for every row and sub-space (t == 1: mind starts at +inf
// and is not read), and the level-1 and level-2 sums of the weights.
hipError_t launch_kmeans_seed_update(const KmeansSeedState& st, const KmeansSeedPlan& plan, uint64_t t, hipStream_t stream);

// round t, second launch (t == 0: the only one): the levels above 2, the descent or the fallback; writes centres[m][t], rows[m][t]
// and the picked bit.
hipError_t launch_kmeans_seed_pick(const KmeansSeedState& st, const KmeansSeedPlan& plan, uint64_t t, hipStream_t stream);

}  // namespace qadc
