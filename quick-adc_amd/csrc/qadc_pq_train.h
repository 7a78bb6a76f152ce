// PQ training: the centroid update of every sub-space in one launch.  Internal header shared by
// csrc/qadc_pq_train_kernel.hip and csrc/qadc_pq_train.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../host/pq_train_plan.hpp"

namespace qadc {

// kmeans_fast_iterations_thread's centroid update (databases.cpp:67-88) in every sub-space at once: centroid (m, k) = (the
// sub-vectors m of the vectors whose code m is k, summed in ascending vector index into one running float from 0.0f) times
// 1.0f / count (div_mode 1, as the reference is compiled) or divided by the count (div_mode 0); an empty cluster becomes NaN.
// d_x [n][dim] is read in place; d_codes: sq_bits 4 — packed nibbles [n][sq_count / 2], the even sub-quantizer in the low nibble;
// sq_bits 8 — bytes [n][sq_count].  d_codebooks [sq_count][2^sq_bits][dim / sq_count] is overwritten.  hipErrorInvalidValue:
// a shape pq_train_plan refuses.
hipError_t launch_pq_train_update(const float* d_x, uint64_t n, int dim, int sq_count, int sq_bits, const uint8_t* d_codes,
                                  float* d_codebooks, int div_mode, hipStream_t stream);

}  // namespace qadc
