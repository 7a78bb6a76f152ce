// PQ training for 16-bit sub-quantizers: the sorted centroid update.  Internal header shared by
// csrc/qadc_pq_train16_kernel.hip and csrc/qadc_build.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../host/pq_train16_plan.hpp"

namespace qadc {

// words of d_hist for n vectors: 256 per tile of kPqTrain16Tile entries
inline size_t pq_train16_hist_words(uint32_t n) { return (((size_t)n + kPqTrain16Tile - 1) / kPqTrain16Tile) * 256; }

// kmeans_fast_iterations_thread's centroid update (databases.cpp:67-88) in every sub-space of 65536 centroids: centroid (m, k) =
// (the sub-vectors m of the vectors whose code m is k, summed in ascending vector index into one running float from 0.0f) times
// 1.0f / count (div_mode 1) or divided by the count (div_mode 0); an empty cluster becomes NaN.  Per sub-quantizer: a stable sort
// of the vector indices by code (two 8-bit radix passes), the clusters' first positions, then one chain per (cluster, component)
// over the cluster's run.  d_x [n][dim] is read in place; d_codes [n][sq_count] uint16; d_codebooks [sq_count][65536][dim /
// sq_count] is overwritten; d_counts [sq_count][65536] (nullable) receives the cluster sizes.  Scratch: d_perm_a, d_perm_b n words
// each, d_hist pq_train16_hist_words(n), d_start 65537 words; all reused across the sub-quantizers.  Everything is queued on
// `stream`, nothing waits for the device.  hipErrorInvalidValue: a shape pq_train16_plan refuses, or n == 0.
hipError_t launch_pq_train16_update(const float* d_x, uint32_t n, int dim, int sq_count, const uint16_t* d_codes, float* d_codebooks,
                                    uint32_t* d_counts, int div_mode, uint32_t* d_perm_a, uint32_t* d_perm_b, uint32_t* d_hist,
                                    uint32_t* d_start, hipStream_t stream);

}  // namespace qadc
