// k-means++ seeding: qadc_kmeans_seed_host / _device.  The learning set goes through the trainers' front
// (assign_nearest + launch_residual_rotate: qadc_pq_train_*'s own floats), then k rounds are queued on one stream — per round
// seed_update_kernel and seed_pick_kernel (csrc/qadc_kmeans_seed_kernel.hip) — and nothing waits until the last pick is queued.
#include "qadc_build_shared.h"
#include "qadc_kmeans_seed.h"

using namespace qadc;
using namespace qadc::host;
using namespace qadc::build;

namespace {

// the argument checks of both entry points: before the first HIP call
int seed_check(const float* vectors, uint64_t n, int dim, int sq_count, int64_t k, int K_coarse, const float* coarse, const float* centres_out) {
    const KmeansSeedRefusal r = kmeans_seed_refusal(vectors != nullptr, centres_out != nullptr, n, dim, sq_count, k, K_coarse, coarse != nullptr);
    if (r != kSeedOk) return fail(QADC_E_ARG, kmeans_seed_refusal_text(r));
    KmeansSeedPlan plan;
    if (!kmeans_seed_plan(n, dim, sq_count, (uint64_t)k, &plan)) return fail(QADC_E_ARG, "the seeding kernels do not take this shape");
    return QADC_OK;
}

// what the quantizer sees of the learning set (pq_train_front_device's steps): *d_enc = d_vectors itself where neither is given
int seed_front(const float* d_vectors, uint64_t n, int dim, int K_coarse, const float* coarse, const float* rotation, ScratchFree& mem,
               const float** d_enc) {
    float *d_rot = nullptr, *d_coarse = nullptr, *d_x = nullptr, *d_dist = nullptr;
    int32_t* d_assign = nullptr;
    *d_enc = d_vectors;
    if (rotation) {
        HIPCHECK(mem.alloc(&d_rot, sizeof(float) * (size_t)dim * dim));
        HIPCHECK(hipMemcpy(d_rot, rotation, sizeof(float) * (size_t)dim * dim, hipMemcpyHostToDevice));
    }
    if (K_coarse > 0) {
        HIPCHECK(mem.alloc(&d_coarse, sizeof(float) * (size_t)K_coarse * dim));
        HIPCHECK(hipMemcpy(d_coarse, coarse, sizeof(float) * (size_t)K_coarse * dim, hipMemcpyHostToDevice));
        HIPCHECK(mem.alloc(&d_dist, sizeof(float) * assign_nearest_floats(n, K_coarse)));
        HIPCHECK(mem.alloc(&d_assign, sizeof(int32_t) * n));
        if (int rc = assign_nearest(d_vectors, n, dim, K_coarse, d_coarse, d_dist, d_assign, 1)) return rc;
    }
    if (K_coarse > 0 || rotation) {
        HIPCHECK(mem.alloc(&d_x, sizeof(float) * n * dim));
        launch_residual_rotate(d_vectors, n, dim, d_coarse, d_assign, d_rot, d_x, nullptr);
        *d_enc = d_x;
    }
    return QADC_OK;
}

// d_vectors: the learning set in device memory (read by kernels only)
int seed_run(const float* d_vectors, uint64_t n, int dim, int sq_count, uint64_t k, int K_coarse, const float* coarse, const float* rotation,
             uint64_t seed, float* centres_out, uint32_t* rows_out, uint64_t* fallbacks_out, ScratchFree& mem) {
    KmeansSeedPlan plan;
    if (!kmeans_seed_plan(n, dim, sq_count, k, &plan)) return fail(QADC_E_ARG, "the seeding kernels do not take this shape");
    const size_t S = (size_t)sq_count;
    KmeansSeedState st = {};
    st.n = n;
    st.k = k;
    st.seed = seed;
    if (int rc = seed_front(d_vectors, n, dim, K_coarse, coarse, rotation, mem, &st.x)) return rc;
    HIPCHECK(mem.alloc(&st.mind, S * n * sizeof(float)));
    HIPCHECK(mem.alloc(&st.level1, S * plan.nodes[1] * sizeof(double)));
    HIPCHECK(mem.alloc(&st.level2, S * plan.nodes[2] * sizeof(double)));
    HIPCHECK(mem.alloc(&st.upper, S * plan.upper_nodes * sizeof(double)));
    HIPCHECK(mem.alloc(&st.picked, S * plan.bitmap_words * sizeof(uint32_t)));
    HIPCHECK(mem.alloc(&st.cursor, S * sizeof(uint32_t)));
    HIPCHECK(mem.alloc(&st.fallbacks, S * sizeof(unsigned long long)));
    HIPCHECK(mem.alloc(&st.centres, S * k * plan.dsub * sizeof(float)));
    HIPCHECK(mem.alloc(&st.rows, S * k * sizeof(uint32_t)));
    HIPCHECK(hipMemsetAsync(st.picked, 0, S * plan.bitmap_words * sizeof(uint32_t), nullptr));
    HIPCHECK(hipMemsetAsync(st.cursor, 0, S * sizeof(uint32_t), nullptr));
    HIPCHECK(hipMemsetAsync(st.fallbacks, 0, S * sizeof(unsigned long long), nullptr));
    HIPCHECK(launch_kmeans_seed_pick(st, plan, 0, nullptr));
    for (uint64_t t = 1; t < k; ++t) {                         // queued on the default stream: nothing waits inside a round
        HIPCHECK(launch_kmeans_seed_update(st, plan, t, nullptr));
        HIPCHECK(launch_kmeans_seed_pick(st, plan, t, nullptr));
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(centres_out, st.centres, S * k * plan.dsub * sizeof(float), hipMemcpyDeviceToHost));
    if (rows_out) HIPCHECK(hipMemcpy(rows_out, st.rows, S * k * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (fallbacks_out) {
        std::vector<unsigned long long> per(S);
        HIPCHECK(hipMemcpy(per.data(), st.fallbacks, S * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        uint64_t total = 0;
        for (unsigned long long f : per) total += f;
        *fallbacks_out = total;
    }
    return QADC_OK;
}

}  // namespace

extern "C" {

int qadc_kmeans_seed_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int64_t k, int K_coarse, const float* coarse,
                            const float* rotation, uint64_t seed, float* centres_out, uint32_t* rows_out, uint64_t* fallbacks_out,
                            int device_id) {
    if (int rc = seed_check(d_vectors, n, dim, sq_count, k, K_coarse, coarse, centres_out)) return rc;
    if (int rc = check_aligned(d_vectors, 4, "d_vectors")) return rc;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;
    return seed_run(d_vectors, n, dim, sq_count, (uint64_t)k, K_coarse, coarse, rotation, seed, centres_out, rows_out, fallbacks_out, mem);
}

int qadc_kmeans_seed_host(const float* vectors, uint64_t n, int dim, int sq_count, int64_t k, int K_coarse, const float* coarse,
                          const float* rotation, uint64_t seed, float* centres_out, uint32_t* rows_out, uint64_t* fallbacks_out,
                          int device_id) {
    if (int rc = seed_check(vectors, n, dim, sq_count, k, K_coarse, coarse, centres_out)) return rc;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;                                           // the learning set goes up once, for every sub-space and round
    float* d_v = nullptr;
    HIPCHECK(mem.alloc(&d_v, sizeof(float) * n * dim));
    HIPCHECK(hipMemcpy(d_v, vectors, sizeof(float) * n * dim, hipMemcpyHostToDevice));
    return seed_run(d_v, n, dim, sq_count, (uint64_t)k, K_coarse, coarse, rotation, seed, centres_out, rows_out, fallbacks_out, mem);
}

}  // extern "C"
