// OPQ learning: the cross matrix between the learning set and its reconstruction.  Internal header shared
// by csrc/qadc_opq_kernel.hip and csrc/qadc_opq.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../host/opq_plan.hpp"

namespace qadc {

// M[a][b] = sum over blocks j of kOpqBlock vectors, ascending, in double from 0.0, of (double)partial_j[a][b];
// partial_j[a][b] = the float chain acc = fmaf(x0[i][a], Y[i][b], acc) from 0.0f over the block's vectors in ascending i, with
// Y[i][b] = codebooks[m][code(i, m)][b - m dsub], m = b / dsub.  d_x0 [n][dim] and d_codes (sq_bits 4: packed nibbles
// [n][sq_count / 2], the even sub-quantizer in the low nibble; 8: bytes [n][sq_count]) are read in place; d_partials: scratch of
// OpqCrossPlan::partial_bytes; d_M [dim][dim] doubles, every entry written.  hipErrorInvalidValue: arguments opq_cross_plan refuses.
hipError_t launch_opq_cross(const float* d_x0, uint64_t n, int dim, int sq_count, int sq_bits, const uint8_t* d_codes,
                            const float* d_codebooks, float* d_partials, double* d_M, hipStream_t stream);

}  // namespace qadc
