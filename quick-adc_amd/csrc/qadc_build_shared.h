// What the database-build host units share (csrc/qadc_build.cpp defines it, csrc/qadc_opq.cpp uses it): the scratch owner, the
// nearest-centroid pass, the argument checks of PQ training and its round.
#pragma once
#include "qadc_host.h"
#include "qadc_pq_repair.h"

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
// Queued on the default stream; nothing waits.  repair (nullable): every round becomes assign, launch_pq_repair, update.
struct PqRepairScratch;
int pq_train_rounds(const float* d_enc, uint64_t n, int dim, int sq_count, int sq_bits, float* d_cb, float* d_cbnorm, uint8_t* d_codes,
                    int iters, int div_mode, int sum_mode, PqRepairScratch* repair = nullptr);

// the scratch of launch_pq_repair for one call: sq_count * n keys of 8 bytes, count, first and the empties of every cluster, the
// histograms and the workgroup counts
struct PqRepairScratch {
    PqRepairPlan plan;
    PqRepairState st;
    int alloc(ScratchFree& mem, uint64_t n, int dim, int sq_count, int sq_bits) {
        st = PqRepairState();
        if (!pq_repair_plan(n, dim, sq_count, sq_bits, &plan)) return host::fail(QADC_E_ARG, "the repair kernels do not take this shape");
        uint8_t* zeroed = nullptr;
        HIPCHECK(mem.alloc(&zeroed, pq_repair_zeroed_bytes(plan)));
        pq_repair_bind_zeroed(st, plan, zeroed);
        HIPCHECK(mem.alloc(&st.first, plan.first_bytes));
        HIPCHECK(mem.alloc(&st.empties, plan.empties_bytes));
        HIPCHECK(mem.alloc(&st.blockcnt, plan.blockcnt_bytes));
        HIPCHECK(mem.alloc(&st.keys, plan.key_bytes));
        HIPCHECK(mem.alloc(&st.moved_total, sizeof(unsigned long long) * kPqRepairMaxSq));
        HIPCHECK(hipMemset(st.moved_total, 0, sizeof(unsigned long long) * kPqRepairMaxSq));
        return QADC_OK;
    }
    // one repair of d_codes under d_cb, queued on the default stream
    int run(const float* d_enc, const float* d_cb, void* d_codes) {
        st.x = d_enc;
        st.cb = d_cb;
        st.codes = d_codes;
        HIPCHECK(launch_pq_repair(st, plan, nullptr));
        return QADC_OK;
    }
    // after the device is idle: the moves of all rounds and sub-spaces
    int total(uint64_t* out) {
        unsigned long long per[kPqRepairMaxSq];
        HIPCHECK(hipMemcpy(per, st.moved_total, sizeof per, hipMemcpyDeviceToHost));
        *out = 0;
        for (int m = 0; m < plan.sq_count; ++m) *out += per[m];
        return QADC_OK;
    }
};

}  // namespace build
}  // namespace qadc
