// Database build entry points: PQ encode (quantizers.hpp:222-245), the compute of
// index_db::add_vectors (databases.hpp:270-298) and the k-means iterations (databases.cpp:50-90).  Stateless: host buffers
// (or device pointers) in and out, any device.
#include "qadc_build_shared.h"
#include "qadc_adc_kernels.h"   // launch_adc_encode: the assignment step of qadc_pq_train at 8 bits
#include "qadc_pq_train.h"
#include "qadc_pq_train16.h"

#include <cmath>

using namespace qadc;
using namespace qadc::host;
using namespace qadc::build;

extern "C" {

int qadc_pq_encode(int M, int dim, const float* codebooks, const void* d_vectors, uint64_t n, void* d_codes, int device_id) {
    return qadc_pq_encode_mode(M, dim, codebooks, d_vectors, n, d_codes, 1, 1, device_id);
}

int qadc_pq_encode_mode(int M, int dim, const float* codebooks, const void* d_vectors, uint64_t n, void* d_codes, int encode_form,
                        int sum_mode, int device_id) {
    if ((M != 16 && M != 32) || dim <= 0 || dim % M != 0 || !codebooks || (n && (!d_vectors || !d_codes)))
        return fail(QADC_E_ARG, "bad arguments");
    if (dim > kPqEncodeMaxDim) return fail(QADC_E_ARG, "dim must be <= 2048 (the encoder keeps the codebooks in LDS)");
    if (int rc = check_aligned(d_vectors, 4, "d_vectors")) return rc;   // (d_codes is written byte by byte: any address)
    HIPCHECK(hipSetDevice(device_id));
    const size_t ncb = (size_t)M * 16 * (dim / M);
    float* d_cb = nullptr;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_cb), ncb * sizeof(float)));
    HIPCHECK(hipMemcpy(d_cb, codebooks, ncb * sizeof(float), hipMemcpyHostToDevice));
    if (n) launch_pq_encode(static_cast<const float*>(d_vectors), n, M, dim, d_cb, encode_form != 0, sum_mode != 0,
                            static_cast<uint8_t*>(d_codes), nullptr);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipFree(d_cb));
    return QADC_OK;
}

int qadc_pq_encode_host(int M, int dim, const float* codebooks, const float* vectors, uint64_t n, uint8_t* codes, int device_id) {
    return qadc_pq_encode_host_mode(M, dim, codebooks, vectors, n, codes, 1, 1, device_id);
}

int qadc_pq_encode_host_mode(int M, int dim, const float* codebooks, const float* vectors, uint64_t n, uint8_t* codes, int encode_form,
                             int sum_mode, int device_id) {
    if (!vectors || !codes) return fail(QADC_E_ARG, "bad arguments");
    HIPCHECK(hipSetDevice(device_id));
    float* d_v = nullptr;
    uint8_t* d_c = nullptr;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_v), std::max<size_t>(1, n * dim * sizeof(float))));
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_c), std::max<size_t>(1, n * (M / 2))));
    HIPCHECK(hipMemcpy(d_v, vectors, n * dim * sizeof(float), hipMemcpyHostToDevice));
    const int rc = qadc_pq_encode_mode(M, dim, codebooks, d_v, n, d_c, encode_form, sum_mode, device_id);
    if (rc == QADC_OK) HIPCHECK(hipMemcpy(codes, d_c, n * (M / 2), hipMemcpyDeviceToHost));
    HIPCHECK(hipFree(d_v));
    HIPCHECK(hipFree(d_c));
    return rc;
}

/* ---- database build (N4): index_db::add_vectors' compute and the k-means iterations, host buffers in and out ---- */
extern "C++" {
namespace qadc {
namespace build {                                              // (shared with csrc/qadc_opq.cpp: qadc_build_shared.h)
// nearest centroid of every vector, chunk by chunk: the coarse kernels of qadc_search with ma = 1 (find_k_neighbors with k = 1 on the
// expansion distances).  d_dist: chunk x K distances + chunk query norms + K centroid norms (the centroids may have moved: each call).
int assign_nearest(const float* d_vectors, uint64_t n, int dim, int K, const float* d_coarse, float* d_dist, int32_t* d_assign, int sum_mode) {
    const uint64_t chunk = std::min<uint64_t>(kBuildChunk, std::max<uint64_t>(n, 1));
    float* d_qnorm = d_dist + chunk * (uint64_t)K;
    float* d_cnorm = d_qnorm + chunk;
    launch_row_sqnorm(d_coarse, K, dim, sum_mode, d_cnorm, nullptr);
    for (uint64_t o = 0; o < n; o += kBuildChunk) {
        const int cnt = (int)std::min<uint64_t>(kBuildChunk, n - o);
        launch_coarse_assign(d_vectors + o * dim, d_coarse, cnt, K, dim, 1, d_qnorm, d_cnorm, sum_mode, d_dist, d_assign + o, nullptr);
    }
    HIPCHECK(hipGetLastError());
    return QADC_OK;
}
}  // namespace build
}  // namespace qadc
}  // extern "C++"

int qadc_ivf_encode_host(int M, int dim, const float* codebooks, const float* rotation, int K, const float* coarse,
                         const float* vectors, uint64_t n, int32_t* assign_out, uint8_t* codes, int device_id) {
    return qadc_ivf_encode_host_mode(M, dim, codebooks, rotation, K, coarse, vectors, n, assign_out, codes, 1, 1, device_id);
}

int qadc_ivf_encode_host_mode(int M, int dim, const float* codebooks, const float* rotation, int K, const float* coarse,
                              const float* vectors, uint64_t n, int32_t* assign_out, uint8_t* codes, int encode_form, int sum_mode,
                              int device_id) {
    if ((M != 16 && M != 32) || dim <= 0 || dim % M != 0 || !codebooks || K < 0 || (K > 0 && !coarse) ||
        (n && (!vectors || !codes)))
        return fail(QADC_E_ARG, "bad arguments");
    if (dim > kPqEncodeMaxDim) return fail(QADC_E_ARG, "dim must be <= 2048 (the encoder keeps the codebooks in LDS)");
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;
    const size_t ncb = (size_t)M * 16 * (dim / M);
    float *d_cb = nullptr, *d_rot = nullptr, *d_coarse = nullptr, *d_v = nullptr, *d_x = nullptr, *d_dist = nullptr;
    int32_t* d_assign = nullptr;
    uint8_t* d_codes = nullptr;
    HIPCHECK(mem.alloc(&d_cb, ncb * sizeof(float)));
    HIPCHECK(hipMemcpy(d_cb, codebooks, ncb * sizeof(float), hipMemcpyHostToDevice));
    if (rotation) {
        HIPCHECK(mem.alloc(&d_rot, sizeof(float) * (size_t)dim * dim));
        HIPCHECK(hipMemcpy(d_rot, rotation, sizeof(float) * (size_t)dim * dim, hipMemcpyHostToDevice));
    }
    if (K > 0) {
        HIPCHECK(mem.alloc(&d_coarse, sizeof(float) * (size_t)K * dim));
        HIPCHECK(hipMemcpy(d_coarse, coarse, sizeof(float) * (size_t)K * dim, hipMemcpyHostToDevice));
        HIPCHECK(mem.alloc(&d_dist, sizeof(float) * ((size_t)std::min<uint64_t>(kBuildChunk, std::max<uint64_t>(n, 1)) * (K + 1) + K)));
        HIPCHECK(mem.alloc(&d_assign, sizeof(int32_t) * n));
    }
    HIPCHECK(mem.alloc(&d_v, sizeof(float) * n * dim));
    HIPCHECK(mem.alloc(&d_codes, n * (size_t)(M / 2)));
    HIPCHECK(hipMemcpy(d_v, vectors, sizeof(float) * n * dim, hipMemcpyHostToDevice));
    const float* d_enc = d_v;
    if (n && K > 0)
        if (int rc = assign_nearest(d_v, n, dim, K, d_coarse, d_dist, d_assign, sum_mode != 0)) return rc;
    if (n && (K > 0 || rotation)) {
        HIPCHECK(mem.alloc(&d_x, sizeof(float) * n * dim));
        launch_residual_rotate(d_v, n, dim, d_coarse, d_assign, d_rot, d_x, nullptr);
        d_enc = d_x;
    }
    if (n) launch_pq_encode(d_enc, n, M, dim, d_cb, encode_form != 0, sum_mode != 0, d_codes, nullptr);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(codes, d_codes, n * (size_t)(M / 2), hipMemcpyDeviceToHost));
    if (assign_out && K > 0) HIPCHECK(hipMemcpy(assign_out, d_assign, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return QADC_OK;
}

int qadc_coarse_assign_host(const float* queries, int nq, const float* coarse, int K, int dim, int ma, int32_t* assign_out,
                            int device_id) {
    if (!queries || !coarse || !assign_out || nq <= 0 || K <= 0 || dim <= 0 || ma <= 0 || ma > K || nq >= (1 << 24))
        return fail(QADC_E_ARG, "bad arguments (need nq > 0, 0 < ma <= K)");
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;
    float *d_q = nullptr, *d_c = nullptr, *d_dist = nullptr, *d_qnorm = nullptr, *d_cnorm = nullptr;
    int32_t* d_assign = nullptr;
    HIPCHECK(mem.alloc(&d_q, sizeof(float) * (size_t)nq * dim));
    HIPCHECK(mem.alloc(&d_c, sizeof(float) * (size_t)K * dim));
    HIPCHECK(mem.alloc(&d_dist, sizeof(float) * (size_t)nq * K));
    HIPCHECK(mem.alloc(&d_qnorm, sizeof(float) * (size_t)nq));
    HIPCHECK(mem.alloc(&d_cnorm, sizeof(float) * (size_t)K));
    HIPCHECK(mem.alloc(&d_assign, sizeof(int32_t) * (size_t)nq * ma));
    HIPCHECK(hipMemcpy(d_q, queries, sizeof(float) * (size_t)nq * dim, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_c, coarse, sizeof(float) * (size_t)K * dim, hipMemcpyHostToDevice));
    HIPCHECK(coarse_nan_unreplayed_reset(nullptr));
    launch_row_sqnorm(d_c, K, dim, 1, d_cnorm, nullptr);
    launch_coarse_assign(d_q, d_c, nq, K, dim, ma, d_qnorm, d_cnorm, 1, d_dist, d_assign, nullptr);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    unsigned int unreplayed = 0;
    HIPCHECK(coarse_nan_unreplayed_read(&unreplayed));
    if (unreplayed) return fail(QADC_E_ARG, "a query has a NaN coarse distance and ma > 256: the reference's heap replay is not available");
    HIPCHECK(hipMemcpy(assign_out, d_assign, sizeof(int32_t) * (size_t)nq * ma, hipMemcpyDeviceToHost));
    return QADC_OK;
}

int qadc_kmeans_iterations_host(const float* vectors, uint64_t n, int dim, int K, float* centroids, int iters, int32_t* assign_out,
                                int device_id) {
    return qadc_kmeans_iterations_host_mode(vectors, n, dim, K, centroids, iters, assign_out, 1, device_id);
}

int qadc_kmeans_iterations_host_mode(const float* vectors, uint64_t n, int dim, int K, float* centroids, int iters, int32_t* assign_out,
                                     int div_mode, int device_id) {
    if (!vectors || !centroids || n == 0 || dim <= 0 || dim > 2048 || K <= 0 || iters < 0) return fail(QADC_E_ARG, "bad arguments");
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;
    float *d_v = nullptr, *d_c = nullptr, *d_dist = nullptr;
    int32_t* d_assign = nullptr;
    HIPCHECK(mem.alloc(&d_v, sizeof(float) * n * dim));
    HIPCHECK(mem.alloc(&d_c, sizeof(float) * (size_t)K * dim));
    HIPCHECK(mem.alloc(&d_dist, sizeof(float) * ((size_t)std::min<uint64_t>(kBuildChunk, n) * (K + 1) + K)));
    HIPCHECK(mem.alloc(&d_assign, sizeof(int32_t) * n));
    HIPCHECK(hipMemcpy(d_v, vectors, sizeof(float) * n * dim, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_c, centroids, sizeof(float) * (size_t)K * dim, hipMemcpyHostToDevice));
    HIPCHECK(hipMemset(d_assign, 0, sizeof(int32_t) * n));
    for (int it = 0; it < iters; ++it) {                       // databases.cpp:57-89
        if (int rc = assign_nearest(d_v, n, dim, K, d_c, d_dist, d_assign, 1)) return rc;
        launch_kmeans_update(d_v, n, dim, K, d_assign, d_c, div_mode != 0, nullptr);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(centroids, d_c, sizeof(float) * (size_t)K * dim, hipMemcpyDeviceToHost));
    if (assign_out) HIPCHECK(hipMemcpy(assign_out, d_assign, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    return QADC_OK;
}

/* ---- PQ training: `iters` rounds of k-means in every sub-space at once.  A round = the encoder the index
   of that shape uses (launch_pq_encode at 4 bits, launch_adc_encode at 8: find_k_neighbors with k = 1 per sub-quantizer, norms of the
   moved centroids recomputed) and one launch_pq_train_update over all sq_count * 2^bits centroids. ---- */
extern "C++" {
namespace qadc {
namespace build {                                              // (shared with csrc/qadc_opq.cpp: qadc_build_shared.h)
// the argument checks of both entry points: before the first HIP call
int pq_train_check(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                   const float* codebooks, int iters, int div_mode, int sum_mode) {
    if (sq_bits == 16)
        return fail(QADC_E_ARG, "sq_bits 16 is not trained here (a follow-up: 65536 centroids per sub-quantizer need the sorted update); sq_bits 4 or 8");
    if (sq_bits != 4 && sq_bits != 8) return fail(QADC_E_ARG, "sq_bits must be 4 or 8");
    if (sq_bits == 4 && sq_count != 16 && sq_count != 32) return fail(QADC_E_ARG, "sq_bits 4 takes sq_count 16 or 32 (the 4-bit index's shapes)");
    if (sq_bits == 8 && sq_count != 4 && sq_count != 8 && sq_count != 16)
        return fail(QADC_E_ARG, "sq_bits 8 takes sq_count 4, 8 or 16 (the float-ADC index's shapes)");
    if (dim <= 0 || dim % sq_count != 0) return fail(QADC_E_ARG, "dim must be a positive multiple of sq_count");
    const int max_dim = sq_bits == 4 ? kPqEncodeMaxDim : adc::kAdcMaxDim;
    if (dim > max_dim) return fail(QADC_E_ARG, "dim must be <= " + std::to_string(max_dim) + " (the encoder's limit at " + std::to_string(sq_bits) + " bits)");
    PqTrainPlan plan;
    if (!pq_train_plan(sq_count, sq_bits, dim, &plan))
        return fail(QADC_E_ARG, "dim / sq_count must be <= " + std::to_string(kPqTrainMaxDsub) + " (the update kernel's staged window)");
    if (!vectors || !codebooks) return fail(QADC_E_ARG, "vectors and codebooks must not be NULL");
    if (n == 0 || n >= (1ull << 32)) return fail(QADC_E_ARG, "need 0 < n < 2^32 vectors");
    if (iters < 0) return fail(QADC_E_ARG, "iters must be >= 0");
    if (K_coarse < 0 || (K_coarse > 0 && !coarse)) return fail(QADC_E_ARG, "K_coarse > 0 needs the coarse centroids");
    if ((div_mode != 0 && div_mode != 1) || (sum_mode != 0 && sum_mode != 1)) return fail(QADC_E_ARG, "div_mode and sum_mode are 0 or 1");
    return QADC_OK;
}

uint64_t nan_rows(const float* cb, size_t rows, int ds) {
    uint64_t bad = 0;
    for (size_t r = 0; r < rows; ++r) {
        bool nan = false;
        for (int d = 0; d < ds; ++d) nan = nan || std::isnan(cb[r * ds + d]);
        bad += nan;
    }
    return bad;
}

// the rounds themselves, on the learning set as the quantizer sees it: qadc_pq_train_* and the outer rounds of qadc_opq_train_* run these
int pq_train_rounds(const float* d_enc, uint64_t n, int dim, int sq_count, int sq_bits, float* d_cb, float* d_cbnorm, uint8_t* d_codes,
                    int iters, int div_mode, int sum_mode, PqRepairScratch* repair) {
    const int ds = dim / sq_count;
    const size_t rows = (size_t)sq_count << sq_bits;
    for (int it = 0; it < iters; ++it) {
        if (sq_bits == 4) {
            launch_pq_encode(d_enc, n, sq_count, dim, d_cb, 1, sum_mode, d_codes, nullptr);
        } else {
            launch_row_sqnorm(d_cb, (int)rows, ds, sum_mode, d_cbnorm, nullptr);
            HIPCHECK(adc::launch_adc_encode(d_enc, n, sq_count, dim, d_cb, d_cbnorm, sum_mode, d_codes, nullptr));
        }
        if (repair)                                            // the codes are rewritten before the update reads them
            if (int rc = repair->run(d_enc, d_cb, d_codes)) return rc;
        HIPCHECK(launch_pq_train_update(d_enc, n, dim, sq_count, sq_bits, d_codes, d_cb, div_mode, nullptr));
    }
    return QADC_OK;
}
}  // namespace build
}  // namespace qadc

namespace {
// What the quantizer sees of the learning set, in device memory: with K_coarse > 0 the residual to the nearest coarse centroid, with a
// rotation those rotated (as qadc_ivf_encode_host prepares its input).  *d_enc = d_vectors itself where neither is given.
int pq_train_front_device(const float* d_vectors, uint64_t n, int dim, int K_coarse, const float* coarse, const float* rotation,
                          int sum_mode, ScratchFree& mem, const float** d_enc) {
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
        HIPCHECK(mem.alloc(&d_dist, sizeof(float) * ((size_t)std::min<uint64_t>(kBuildChunk, n) * (K_coarse + 1) + K_coarse)));
        HIPCHECK(mem.alloc(&d_assign, sizeof(int32_t) * n));
        if (int rc = assign_nearest(d_vectors, n, dim, K_coarse, d_coarse, d_dist, d_assign, sum_mode)) return rc;
    }
    if (K_coarse > 0 || rotation) {
        HIPCHECK(mem.alloc(&d_x, sizeof(float) * n * dim));
        launch_residual_rotate(d_vectors, n, dim, d_coarse, d_assign, d_rot, d_x, nullptr);
        *d_enc = d_x;
    }
    return QADC_OK;
}

// d_vectors: the learning set in device memory (read by kernels only: it may belong to another HIP runtime of the process)
int pq_train_run(const float* d_vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                 const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode, int sum_mode,
                 int repair, uint64_t* repaired_out, ScratchFree& mem) {
    const int ds = dim / sq_count;
    const size_t rows = (size_t)sq_count << sq_bits, code_bytes = sq_bits == 4 ? sq_count / 2 : sq_count;
    float *d_cb = nullptr, *d_cbnorm = nullptr;
    uint8_t* d_codes = nullptr;
    PqRepairScratch rp;
    if (repair)
        if (int rc = rp.alloc(mem, n, dim, sq_count, sq_bits)) return rc;
    HIPCHECK(mem.alloc(&d_cb, rows * ds * sizeof(float)));
    HIPCHECK(hipMemcpy(d_cb, codebooks, rows * ds * sizeof(float), hipMemcpyHostToDevice));
    if (sq_bits == 8) HIPCHECK(mem.alloc(&d_cbnorm, rows * sizeof(float)));
    HIPCHECK(mem.alloc(&d_codes, n * code_bytes));
    const float* d_enc = nullptr;
    if (int rc = pq_train_front_device(d_vectors, n, dim, K_coarse, coarse, rotation, sum_mode, mem, &d_enc)) return rc;
    if (int rc = pq_train_rounds(d_enc, n, dim, sq_count, sq_bits, d_cb, d_cbnorm, d_codes, iters, div_mode, sum_mode, repair ? &rp : nullptr))
        return rc;
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(codebooks, d_cb, rows * ds * sizeof(float), hipMemcpyDeviceToHost));
    if (codes_out) HIPCHECK(hipMemcpy(codes_out, d_codes, n * code_bytes, hipMemcpyDeviceToHost));
    if (empty_out) *empty_out = nan_rows(codebooks, rows, ds);
    if (repair && repaired_out)
        if (int rc = rp.total(repaired_out)) return rc;
    return QADC_OK;
}
}  // namespace
}  // extern "C++"

int qadc_pq_train_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                         const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode,
                         int sum_mode, int device_id) {
    return qadc_pq_train_repair_device(d_vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, codebooks, iters, codes_out, empty_out,
                                       div_mode, sum_mode, 0, nullptr, device_id);
}

int qadc_pq_train_host(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                       const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode,
                       int sum_mode, int device_id) {
    return qadc_pq_train_repair_host(vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, codebooks, iters, codes_out, empty_out,
                                     div_mode, sum_mode, 0, nullptr, device_id);
}

int qadc_pq_train_repair_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                                const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode,
                                int sum_mode, int repair, uint64_t* repaired_out, int device_id) {
    if (int rc = pq_train_check(d_vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, codebooks, iters, div_mode, sum_mode)) return rc;
    if (repair != 0 && repair != 1) return fail(QADC_E_ARG, "repair is 0 or 1");
    if (int rc = check_aligned(d_vectors, 4, "d_vectors")) return rc;
    if (repaired_out) *repaired_out = 0;
    if (iters == 0) {                                          // the seed untouched, no code written
        if (empty_out) *empty_out = nan_rows(codebooks, (size_t)sq_count << sq_bits, dim / sq_count);
        return QADC_OK;
    }
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;
    return pq_train_run(d_vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, codebooks, iters, codes_out, empty_out,
                        div_mode, sum_mode, repair, repaired_out, mem);
}

int qadc_pq_train_repair_host(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                              const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode,
                              int sum_mode, int repair, uint64_t* repaired_out, int device_id) {
    if (int rc = pq_train_check(vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, codebooks, iters, div_mode, sum_mode)) return rc;
    if (repair != 0 && repair != 1) return fail(QADC_E_ARG, "repair is 0 or 1");
    if (repaired_out) *repaired_out = 0;
    if (iters == 0) {
        if (empty_out) *empty_out = nan_rows(codebooks, (size_t)sq_count << sq_bits, dim / sq_count);
        return QADC_OK;
    }
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;                                           // the learning set goes up once, for every sub-space and round
    float* d_v = nullptr;
    HIPCHECK(mem.alloc(&d_v, sizeof(float) * n * dim));
    HIPCHECK(hipMemcpy(d_v, vectors, sizeof(float) * n * dim, hipMemcpyHostToDevice));
    return pq_train_run(d_v, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, codebooks, iters, codes_out, empty_out, div_mode,
                        sum_mode, repair, repaired_out, mem);
}

/* ---- PQ training for 16-bit sub-quantizers: a round = launch_adc_encode16 over the resident learning set
   in passes of QADC_ADC_ENCODE16_CHUNK vectors (norms of the moved centroids recomputed), then launch_pq_train16_update: per
   sub-quantizer a stable sort of the vectors by code and one chain per (cluster, component). ---- */
extern "C++" {
namespace {
// the argument checks the three entry points share: before the first HIP call
int pq_train16_check_shape(const float* vectors, uint64_t n, int dim, int sq_count, const float* codebooks, int div_mode) {
    if (sq_count != 2 && sq_count != 4 && sq_count != 8) return fail(QADC_E_ARG, "sq_count must be 2, 4 or 8 (the 16-bit index's shapes)");
    if (dim <= 0 || dim % sq_count != 0) return fail(QADC_E_ARG, "dim must be a positive multiple of sq_count");
    if (dim > adc::kAdcMaxDim) return fail(QADC_E_ARG, "dim must be <= " + std::to_string(adc::kAdcMaxDim) + " (the 16-bit encoder's limit)");
    PqTrain16Plan plan;
    if (!pq_train16_plan(sq_count, dim, &plan))
        return fail(QADC_E_ARG, "dim / sq_count must be <= " + std::to_string(kPqTrain16MaxDsub) + " (the sorted update's plan)");
    if (!vectors || !codebooks) return fail(QADC_E_ARG, "vectors and codebooks must not be NULL");
    if (n == 0 || n >= (1ull << 32)) return fail(QADC_E_ARG, "need 0 < n < 2^32 vectors");
    if (div_mode != 0 && div_mode != 1) return fail(QADC_E_ARG, "div_mode and sum_mode are 0 or 1");
    return QADC_OK;
}

int pq_train16_check(const float* vectors, uint64_t n, int dim, int sq_count, int K_coarse, const float* coarse, const float* codebooks,
                     int iters, int div_mode, int sum_mode) {
    if (int rc = pq_train16_check_shape(vectors, n, dim, sq_count, codebooks, div_mode)) return rc;
    if (iters < 0) return fail(QADC_E_ARG, "iters must be >= 0");
    if (K_coarse < 0 || (K_coarse > 0 && !coarse)) return fail(QADC_E_ARG, "K_coarse > 0 needs the coarse centroids");
    if (sum_mode != 0 && sum_mode != 1) return fail(QADC_E_ARG, "div_mode and sum_mode are 0 or 1");
    return QADC_OK;
}

// the scratch of launch_pq_train16_update
struct Train16Scratch {
    uint32_t *perm_a = nullptr, *perm_b = nullptr, *hist = nullptr, *start = nullptr;
    hipError_t alloc(ScratchFree& mem, uint64_t n) {
        if (hipError_t e = mem.alloc(&perm_a, sizeof(uint32_t) * n)) return e;
        if (hipError_t e = mem.alloc(&perm_b, sizeof(uint32_t) * n)) return e;
        if (hipError_t e = mem.alloc(&hist, sizeof(uint32_t) * pq_train16_hist_words((uint32_t)n))) return e;
        return mem.alloc(&start, sizeof(uint32_t) * (kPqTrain16K + 1));
    }
};

// d_vectors: the learning set in device memory (read by kernels only)
int pq_train16_run(const float* d_vectors, uint64_t n, int dim, int sq_count, int K_coarse, const float* coarse, const float* rotation,
                   float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode, int sum_mode, int repair,
                   uint64_t* repaired_out, ScratchFree& mem) {
    const int ds = dim / sq_count;
    const size_t rows = (size_t)sq_count * kPqTrain16K;
    float *d_cb = nullptr, *d_cbnorm = nullptr;
    uint16_t* d_codes = nullptr;
    unsigned long long* d_part = nullptr;
    Train16Scratch sc;
    PqRepairScratch rp;
    if (repair)
        if (int rc = rp.alloc(mem, n, dim, sq_count, 16)) return rc;
    HIPCHECK(mem.alloc(&d_cb, rows * ds * sizeof(float)));
    HIPCHECK(hipMemcpy(d_cb, codebooks, rows * ds * sizeof(float), hipMemcpyHostToDevice));
    HIPCHECK(mem.alloc(&d_cbnorm, rows * sizeof(float)));
    HIPCHECK(mem.alloc(&d_codes, n * sq_count * sizeof(uint16_t)));
    HIPCHECK(sc.alloc(mem, n));
    // the encoder's partial picks of a pass: the slices of the largest pass and of the last one (a shorter pass is cut finer)
    const uint64_t pass = std::min<uint64_t>(QADC_ADC_ENCODE16_CHUNK, n);
    const uint64_t last = n % QADC_ADC_ENCODE16_CHUNK ? n % QADC_ADC_ENCODE16_CHUNK : pass;
    const uint64_t part_entries = std::max(pass * adc::encode16_slices((uint32_t)pass, sq_count, ds), last * adc::encode16_slices((uint32_t)last, sq_count, ds));
    HIPCHECK(mem.alloc(&d_part, part_entries * sq_count * sizeof(unsigned long long)));
    const float* d_enc = nullptr;
    if (int rc = pq_train_front_device(d_vectors, n, dim, K_coarse, coarse, rotation, sum_mode, mem, &d_enc)) return rc;
    for (int it = 0; it < iters; ++it) {                       // queued on the default stream: nothing waits inside a round
        launch_row_sqnorm(d_cb, (int)rows, ds, sum_mode, d_cbnorm, nullptr);
        for (uint64_t o = 0; o < n; o += QADC_ADC_ENCODE16_CHUNK) {
            const uint64_t cnt = std::min<uint64_t>(QADC_ADC_ENCODE16_CHUNK, n - o);
            HIPCHECK(adc::launch_adc_encode16(d_enc + o * dim, (uint32_t)cnt, sq_count, dim, d_cb, d_cbnorm, sum_mode, d_part,
                                              d_codes + o * sq_count, nullptr));
        }
        if (repair)                                            // the codes are rewritten before the update sorts them
            if (int rc = rp.run(d_enc, d_cb, d_codes)) return rc;
        HIPCHECK(launch_pq_train16_update(d_enc, (uint32_t)n, dim, sq_count, d_codes, d_cb, nullptr, div_mode, sc.perm_a, sc.perm_b, sc.hist,
                                          sc.start, nullptr));
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(codebooks, d_cb, rows * ds * sizeof(float), hipMemcpyDeviceToHost));
    if (codes_out) HIPCHECK(hipMemcpy(codes_out, d_codes, n * sq_count * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (empty_out) *empty_out = nan_rows(codebooks, rows, ds);
    if (repair && repaired_out)
        if (int rc = rp.total(repaired_out)) return rc;
    return QADC_OK;
}
}  // namespace
}  // extern "C++"

int qadc_pq_train16_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int K_coarse, const float* coarse,
                           const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode,
                           int sum_mode, int device_id) {
    return qadc_pq_train16_repair_device(d_vectors, n, dim, sq_count, K_coarse, coarse, rotation, codebooks, iters, codes_out, empty_out, div_mode,
                                         sum_mode, 0, nullptr, device_id);
}

int qadc_pq_train16_host(const float* vectors, uint64_t n, int dim, int sq_count, int K_coarse, const float* coarse,
                         const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode,
                         int sum_mode, int device_id) {
    return qadc_pq_train16_repair_host(vectors, n, dim, sq_count, K_coarse, coarse, rotation, codebooks, iters, codes_out, empty_out, div_mode,
                                       sum_mode, 0, nullptr, device_id);
}

int qadc_pq_train16_repair_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int K_coarse, const float* coarse,
                                  const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode,
                                  int sum_mode, int repair, uint64_t* repaired_out, int device_id) {
    if (int rc = pq_train16_check(d_vectors, n, dim, sq_count, K_coarse, coarse, codebooks, iters, div_mode, sum_mode)) return rc;
    if (repair != 0 && repair != 1) return fail(QADC_E_ARG, "repair is 0 or 1");
    if (repaired_out) *repaired_out = 0;
    if (int rc = check_aligned(d_vectors, 16, "d_vectors")) return rc;   // (the 16-bit encoder of a round: adc_encode16_kernel's 16-byte loads)
    if (iters == 0) {                                          // the seed untouched, no code written
        if (empty_out) *empty_out = nan_rows(codebooks, (size_t)sq_count * kPqTrain16K, dim / sq_count);
        return QADC_OK;
    }
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;
    return pq_train16_run(d_vectors, n, dim, sq_count, K_coarse, coarse, rotation, codebooks, iters, codes_out, empty_out, div_mode,
                          sum_mode, repair, repaired_out, mem);
}

int qadc_pq_train16_repair_host(const float* vectors, uint64_t n, int dim, int sq_count, int K_coarse, const float* coarse,
                                const float* rotation, float* codebooks, int iters, void* codes_out, uint64_t* empty_out, int div_mode,
                                int sum_mode, int repair, uint64_t* repaired_out, int device_id) {
    if (int rc = pq_train16_check(vectors, n, dim, sq_count, K_coarse, coarse, codebooks, iters, div_mode, sum_mode)) return rc;
    if (repair != 0 && repair != 1) return fail(QADC_E_ARG, "repair is 0 or 1");
    if (repaired_out) *repaired_out = 0;
    if (iters == 0) {
        if (empty_out) *empty_out = nan_rows(codebooks, (size_t)sq_count * kPqTrain16K, dim / sq_count);
        return QADC_OK;
    }
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;                                           // the learning set goes up once, for every sub-space and round
    float* d_v = nullptr;
    HIPCHECK(mem.alloc(&d_v, sizeof(float) * n * dim));
    HIPCHECK(hipMemcpy(d_v, vectors, sizeof(float) * n * dim, hipMemcpyHostToDevice));
    return pq_train16_run(d_v, n, dim, sq_count, K_coarse, coarse, rotation, codebooks, iters, codes_out, empty_out, div_mode, sum_mode,
                          repair, repaired_out, mem);
}

int qadc_pq_update16_host(const float* vectors, uint64_t n, int dim, int sq_count, const uint16_t* codes, float* codebooks_out,
                          uint32_t* counts_out, int div_mode, int device_id) {
    if (int rc = pq_train16_check_shape(vectors, n, dim, sq_count, codebooks_out, div_mode)) return rc;
    if (!codes) return fail(QADC_E_ARG, "codes must not be NULL");
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;
    const int ds = dim / sq_count;
    const size_t rows = (size_t)sq_count * kPqTrain16K;
    float *d_v = nullptr, *d_cb = nullptr;
    uint16_t* d_codes = nullptr;
    uint32_t* d_counts = nullptr;
    Train16Scratch sc;
    HIPCHECK(mem.alloc(&d_v, sizeof(float) * n * dim));
    HIPCHECK(mem.alloc(&d_cb, rows * ds * sizeof(float)));
    HIPCHECK(mem.alloc(&d_codes, n * sq_count * sizeof(uint16_t)));
    if (counts_out) HIPCHECK(mem.alloc(&d_counts, rows * sizeof(uint32_t)));
    HIPCHECK(sc.alloc(mem, n));
    HIPCHECK(hipMemcpy(d_v, vectors, sizeof(float) * n * dim, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_codes, codes, n * sq_count * sizeof(uint16_t), hipMemcpyHostToDevice));
    HIPCHECK(launch_pq_train16_update(d_v, (uint32_t)n, dim, sq_count, d_codes, d_cb, d_counts, div_mode, sc.perm_a, sc.perm_b, sc.hist,
                                      sc.start, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(codebooks_out, d_cb, rows * ds * sizeof(float), hipMemcpyDeviceToHost));
    if (counts_out) HIPCHECK(hipMemcpy(counts_out, d_counts, rows * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return QADC_OK;
}

/* ---- empty-cluster repair alone: launch_pq_repair on the caller's codes ---- */
int qadc_pq_repair_host(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, const float* codebooks, void* codes,
                        uint32_t* moved_out, int device_id) {
    if (sq_bits != 4 && sq_bits != 8 && sq_bits != 16) return fail(QADC_E_ARG, "sq_bits must be 4, 8 or 16");
    if (sq_bits == 16) {
        if (int rc = pq_train16_check_shape(vectors, n, dim, sq_count, codebooks, 1)) return rc;
    } else if (int rc = pq_train_check(vectors, n, dim, sq_count, sq_bits, 0, nullptr, codebooks, 0, 1, 1)) {
        return rc;
    }
    if (!codes) return fail(QADC_E_ARG, "codes must not be NULL");
    PqRepairPlan plan;
    if (!pq_repair_plan(n, dim, sq_count, sq_bits, &plan)) return fail(QADC_E_ARG, "the repair kernels do not take this shape");
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;
    const size_t cb_bytes = (size_t)sq_count * plan.K * plan.dsub * sizeof(float), code_bytes = (size_t)plan.units * plan.unit_bytes;
    float *d_v = nullptr, *d_cb = nullptr;
    uint8_t* d_codes = nullptr;
    PqRepairScratch rp;
    HIPCHECK(mem.alloc(&d_v, sizeof(float) * n * dim));
    HIPCHECK(mem.alloc(&d_cb, cb_bytes));
    HIPCHECK(mem.alloc(&d_codes, code_bytes));
    if (int rc = rp.alloc(mem, n, dim, sq_count, sq_bits)) return rc;
    HIPCHECK(hipMemcpy(d_v, vectors, sizeof(float) * n * dim, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_cb, codebooks, cb_bytes, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_codes, codes, code_bytes, hipMemcpyHostToDevice));
    if (int rc = rp.run(d_v, d_cb, d_codes)) return rc;
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(codes, d_codes, code_bytes, hipMemcpyDeviceToHost));
    if (moved_out) {
        unsigned long long per[kPqRepairMaxSq];
        HIPCHECK(hipMemcpy(per, rp.st.moved_total, sizeof per, hipMemcpyDeviceToHost));
        for (int m = 0; m < sq_count; ++m) moved_out[m] = (uint32_t)per[m];
    }
    return QADC_OK;
}

}  // extern "C"
