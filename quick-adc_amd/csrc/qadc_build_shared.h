// What the database-build host units share (csrc/qadc_build.cpp defines it, csrc/qadc_opq.cpp uses it): the scratch owner, the
// nearest-centroid pass, the argument checks of PQ training and its round.
#pragma once
#include "qadc_host.h"

namespace qadc {
namespace build {

struct ScratchFree {                                           // hipFree on every exit path
    std::vector<void*> p;
    ~ScratchFree() { for (void* x : p) if (x) (void)hipFree(x); }
    template <typename T> hipError_t alloc(T** out, size_t bytes) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max<size_t>(bytes, 16));
        if (e == hipSuccess) { p.push_back(q); *out = static_cast<T*>(q); }
        return e;
    }
};
constexpr uint64_t kBuildChunk = 32768;                        // vectors per pass (the distance scratch is chunk x K floats)

// floats of the d_dist scratch assign_nearest needs for n vectors and K centroids
inline size_t assign_nearest_floats(uint64_t n, int K) {
    return (size_t)std::min<uint64_t>(kBuildChunk, std::max<uint64_t>(n, 1)) * (size_t)(K + 1) + (size_t)K;
}

int assign_nearest(const float* d_vectors, uint64_t n, int dim, int K, const float* d_coarse, float* d_dist, int32_t* d_assign, int sum_mode);

// the argument checks of qadc_pq_train_host / _device: before the first HIP call
int pq_train_check(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                   const float* codebooks, int iters, int div_mode, int sum_mode);

uint64_t nan_rows(const float* cb, size_t rows, int ds);

// `iters` rounds of PQ training on d_enc [n][dim], the learning set as the quantizer sees it: the encoder of the index the codebooks
// are for into d_codes, then launch_pq_train_update into d_cb.  d_cbnorm: (sq_count << sq_bits) floats at 8 bits, unused at 4.
// Queued on the default stream; nothing waits.
int pq_train_rounds(const float* d_enc, uint64_t n, int dim, int sq_count, int sq_bits, float* d_cb, float* d_cbnorm, uint8_t* d_codes,
                    int iters, int div_mode, int sum_mode);

}  // namespace build
}  // namespace qadc
