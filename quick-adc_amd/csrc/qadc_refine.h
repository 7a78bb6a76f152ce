// Exact re-ranking (qadc_refine_* in include/qadc.h): what the host unit (qadc_refine.cpp) and the kernels
// (qadc_refine_kernel.hip) share.  The launch geometry is host/refine_plan.hpp; the definition the kernels are held to, bit for
// bit, is host/refine.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../host/refine_plan.hpp"

namespace qadc {
namespace refine {

// One re-ranking pass over nq queries (a pass of the plan).  Every pointer is device memory and is touched by kernels only, so
// memory of another HIP runtime is legal.  rows: the store, `f16` says which element type; counts and values may be null.
struct RefinePass {
    const void* rows;
    bool f16;
    uint32_t lo;
    uint64_t nrows;
    int dim, nq, r_in, R;
    const float* queries;          // [nq][dim]
    const uint32_t* keys;          // [nq][r_in]
    const int32_t* counts;         // [nq], clamped to [0, r_in] by the kernel
    const float* values;           // [nq][r_in]
    uint64_t* words;               // scratch [nq][r_in]
    unsigned long long* missing;   // += the missing entries of the pass
    uint32_t* out_keys;            // [nq][R]
    float* out_dist;               // [nq][R]
    int32_t* out_sizes;            // [nq]
};

// refine_dist_kernel<Row>: the word of every candidate of the pass into p.words
hipError_t launch_refine_dist(const RefinePass& p, const RefinePlan& plan, hipStream_t stream);
// refine_select_kernel<N>: sort, dedupe, the first R survivors and the tail of every query of the pass
hipError_t launch_refine_select(const RefinePass& p, const RefinePlan& plan, hipStream_t stream);
// refine_convert_kernel<Row>: dst[i] = Row(src[i]) for n floats (Row float: a copy; __half: round to nearest even)
hipError_t launch_refine_convert(const float* src, void* dst, bool f16, uint64_t n, hipStream_t stream);

}  // namespace refine
}  // namespace qadc
