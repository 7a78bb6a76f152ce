// Learning the OPQ rotation: non-parametric OPQ (Ge et al.) around the PQ training rounds.  An outer
// round = the rotated copy of the learning set refreshed (launch_residual_rotate on the inputs of qadc_pq_train_*'s front),
// `inner` training rounds (build::pq_train_rounds: the training call's own kernels), the cross matrix M = X0^T Y on the GPU
// (csrc/qadc_opq_kernel.hip) and the orthogonal Procrustes solve on the host (host/procrustes.hpp).  The learning set, its residual,
// its rotated copy, the codes and the codebooks stay in device memory for the call; only M comes down and only R goes up.
#include "qadc_build_shared.h"
#include "qadc_opq.h"
#include "qadc_pq_train.h"
#include "../host/procrustes.hpp"

#include <cmath>

using namespace qadc;
using namespace qadc::host;
using namespace qadc::build;

namespace {

// the argument checks of the cross and training entry points: before the first HIP call
int opq_check(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
              const float* codebooks, int div_mode, int sum_mode) {
    if (sq_bits == 16)
        return fail(QADC_E_ARG, "sq_bits 16 is not learned here (a follow-up on the sorted update of qadc_pq_train16_host); sq_bits 4 or 8");
    if (int rc = pq_train_check(vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, codebooks, 1, div_mode, sum_mode)) return rc;
    if (dim > kOpqMaxDim)
        return fail(QADC_E_ARG, "dim must be <= " + std::to_string(kOpqMaxDim) + " (the host Procrustes solve costs O(dim^3) per sweep)");
    OpqCrossPlan plan;
    if (!opq_cross_plan(dim, sq_count, sq_bits, n, &plan)) return fail(QADC_E_ARG, "the cross kernel does not take this shape");
    return QADC_OK;
}

// X0 in device memory: with K_coarse > 0 the residual to the nearest coarse centroid (pq_train_front_device with rotation == NULL),
// else d_vectors itself.  *d_coarse / *d_assign: what the rotated copy is later made from (NULL without a coarse quantizer).
int opq_front(const float* d_vectors, uint64_t n, int dim, int K_coarse, const float* coarse, int sum_mode, ScratchFree& mem,
              const float** d_x0, float** d_coarse, int32_t** d_assign) {
    *d_x0 = d_vectors;
    *d_coarse = nullptr;
    *d_assign = nullptr;
    if (K_coarse <= 0) return QADC_OK;
    float *d_dist = nullptr, *d_res = nullptr;
    HIPCHECK(mem.alloc(d_coarse, sizeof(float) * (size_t)K_coarse * dim));
    HIPCHECK(hipMemcpy(*d_coarse, coarse, sizeof(float) * (size_t)K_coarse * dim, hipMemcpyHostToDevice));
    HIPCHECK(mem.alloc(&d_dist, sizeof(float) * assign_nearest_floats(n, K_coarse)));
    HIPCHECK(mem.alloc(d_assign, sizeof(int32_t) * n));
    if (int rc = assign_nearest(d_vectors, n, dim, K_coarse, *d_coarse, d_dist, *d_assign, sum_mode)) return rc;
    HIPCHECK(mem.alloc(&d_res, sizeof(float) * n * dim));
    launch_residual_rotate(d_vectors, n, dim, *d_coarse, *d_assign, nullptr, d_res, nullptr);
    *d_x0 = d_res;
    return QADC_OK;
}

// the scratch of launch_opq_cross and M on both sides
struct CrossScratch {
    float* d_partials = nullptr;
    double* d_M = nullptr;
    int alloc(ScratchFree& mem, uint64_t n, int dim, int sq_count, int sq_bits) {
        OpqCrossPlan plan;
        if (!opq_cross_plan(dim, sq_count, sq_bits, n, &plan)) return fail(QADC_E_ARG, "the cross kernel does not take this shape");
        HIPCHECK(mem.alloc(&d_partials, (size_t)plan.partial_bytes));
        HIPCHECK(mem.alloc(&d_M, sizeof(double) * (size_t)dim * dim));
        return QADC_OK;
    }
};

int cross_run(const float* d_vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse, const void* codes,
              const float* codebooks, double* M_out, int sum_mode, ScratchFree& mem) {
    const size_t cb_floats = ((size_t)sq_count << sq_bits) * (size_t)(dim / sq_count);
    const size_t code_bytes = sq_bits == 4 ? sq_count / 2 : sq_count;
    const float* d_x0 = nullptr;
    float *d_coarse = nullptr, *d_cb = nullptr;
    int32_t* d_assign = nullptr;
    uint8_t* d_codes = nullptr;
    CrossScratch sc;
    if (int rc = opq_front(d_vectors, n, dim, K_coarse, coarse, sum_mode, mem, &d_x0, &d_coarse, &d_assign)) return rc;
    HIPCHECK(mem.alloc(&d_cb, cb_floats * sizeof(float)));
    HIPCHECK(hipMemcpy(d_cb, codebooks, cb_floats * sizeof(float), hipMemcpyHostToDevice));
    HIPCHECK(mem.alloc(&d_codes, n * code_bytes));
    HIPCHECK(hipMemcpy(d_codes, codes, n * code_bytes, hipMemcpyHostToDevice));
    if (int rc = sc.alloc(mem, n, dim, sq_count, sq_bits)) return rc;
    HIPCHECK(launch_opq_cross(d_x0, n, dim, sq_count, sq_bits, d_codes, d_cb, sc.d_partials, sc.d_M, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(M_out, sc.d_M, sizeof(double) * (size_t)dim * dim, hipMemcpyDeviceToHost));
    return QADC_OK;
}

int procrustes_rc(int rc) {
    switch (rc) {
        case kProcrustesOk: return QADC_OK;
        case kProcrustesNotFinite: return fail(QADC_E_ARG, "M has a non-finite entry");
        case kProcrustesNoConvergence:
            return fail(QADC_E_STATE, "the Jacobi sweeps did not converge within " + std::to_string(kProcrustesMaxSweeps) + " sweeps: no rotation is returned");
        default: return fail(QADC_E_ARG, "need M, rotation_out and 0 < dim <= " + std::to_string(kProcrustesMaxDim));
    }
}

int train_check(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                const float* rotation, const float* codebooks, int outer, int inner, int div_mode, int sum_mode) {
    if (int rc = opq_check(vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, codebooks, div_mode, sum_mode)) return rc;
    if (!rotation) return fail(QADC_E_ARG, "rotation must not be NULL (pass the identity for none)");
    if (outer < 0) return fail(QADC_E_ARG, "outer must be >= 0");
    if (inner < 1) return fail(QADC_E_ARG, "inner must be >= 1");
    return QADC_OK;
}

// d_vectors: the learning set in device memory (read by kernels only)
int train_run(const float* d_vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse, float* rotation,
              float* codebooks, int outer, int inner, void* codes_out, uint64_t* empty_out, int* rounds_done_out, int div_mode,
              int sum_mode, int repair, uint64_t* repaired_out, ScratchFree& mem) {
    const int ds = dim / sq_count;
    const size_t rows = (size_t)sq_count << sq_bits, code_bytes = sq_bits == 4 ? sq_count / 2 : sq_count;
    const size_t rot_bytes = sizeof(float) * (size_t)dim * dim;
    const float* d_x0 = nullptr;
    float *d_coarse = nullptr, *d_cb = nullptr, *d_cbnorm = nullptr, *d_rot = nullptr, *d_x = nullptr;
    int32_t* d_assign = nullptr;
    uint8_t* d_codes = nullptr;
    CrossScratch sc;
    PqRepairScratch rp;
    if (repair)
        if (int rc = rp.alloc(mem, n, dim, sq_count, sq_bits)) return rc;
    HIPCHECK(mem.alloc(&d_cb, rows * ds * sizeof(float)));
    HIPCHECK(hipMemcpy(d_cb, codebooks, rows * ds * sizeof(float), hipMemcpyHostToDevice));
    if (sq_bits == 8) HIPCHECK(mem.alloc(&d_cbnorm, rows * sizeof(float)));
    HIPCHECK(mem.alloc(&d_codes, n * code_bytes));
    HIPCHECK(mem.alloc(&d_rot, rot_bytes));
    HIPCHECK(mem.alloc(&d_x, sizeof(float) * n * dim));
    if (outer > 0)
        if (int rc = sc.alloc(mem, n, dim, sq_count, sq_bits)) return rc;
    // the coarse assignment does not depend on the rotation: once
    if (int rc = opq_front(d_vectors, n, dim, K_coarse, coarse, sum_mode, mem, &d_x0, &d_coarse, &d_assign)) return rc;
    std::vector<double> M((size_t)dim * dim);
    int done = 0;
    bool closing = outer == 0;                                 // the closing rounds: the codebooks fit the returned rotation
    for (;;) {
        HIPCHECK(hipMemcpy(d_rot, rotation, rot_bytes, hipMemcpyHostToDevice));
        launch_residual_rotate(d_vectors, n, dim, d_coarse, d_assign, d_rot, d_x, nullptr);   // pq_train_front_device's own floats
        if (int rc = pq_train_rounds(d_x, n, dim, sq_count, sq_bits, d_cb, d_cbnorm, d_codes, inner, div_mode, sum_mode, repair ? &rp : nullptr))
            return rc;
        if (closing) break;
        HIPCHECK(launch_opq_cross(d_x0, n, dim, sq_count, sq_bits, d_codes, d_cb, sc.d_partials, sc.d_M, nullptr));
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(hipMemcpy(M.data(), sc.d_M, sizeof(double) * M.size(), hipMemcpyDeviceToHost));
        bool finite = true;
        for (double m : M) finite = finite && std::isfinite(m);
        if (!finite) {                                          // the rotation stays as it is; the closing rounds still run
            closing = true;
            continue;
        }
        if (int rc = procrustes_rc(procrustes(M.data(), dim, rotation, nullptr))) return rc;
        closing = ++done == outer;
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(codebooks, d_cb, rows * ds * sizeof(float), hipMemcpyDeviceToHost));
    if (codes_out) HIPCHECK(hipMemcpy(codes_out, d_codes, n * code_bytes, hipMemcpyDeviceToHost));
    if (empty_out) *empty_out = nan_rows(codebooks, rows, ds);
    if (rounds_done_out) *rounds_done_out = done;
    if (repair && repaired_out)
        if (int rc = rp.total(repaired_out)) return rc;
    return QADC_OK;
}

}  // namespace

extern "C" {

int qadc_procrustes_host(const double* M, int dim, float* rotation_out, int* sweeps_out) {
    return procrustes_rc(procrustes(M, dim, rotation_out, sweeps_out));
}

int qadc_opq_cross_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                          const void* codes, const float* codebooks, double* M_out, int sum_mode, int device_id) {
    if (int rc = opq_check(d_vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, codebooks, 1, sum_mode)) return rc;
    if (!codes || !M_out) return fail(QADC_E_ARG, "codes and M_out must not be NULL");
    if (int rc = check_aligned(d_vectors, 4, "d_vectors")) return rc;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;
    return cross_run(d_vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, codes, codebooks, M_out, sum_mode, mem);
}

int qadc_opq_cross_host(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                        const void* codes, const float* codebooks, double* M_out, int sum_mode, int device_id) {
    if (int rc = opq_check(vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, codebooks, 1, sum_mode)) return rc;
    if (!codes || !M_out) return fail(QADC_E_ARG, "codes and M_out must not be NULL");
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;
    float* d_v = nullptr;
    HIPCHECK(mem.alloc(&d_v, sizeof(float) * n * dim));
    HIPCHECK(hipMemcpy(d_v, vectors, sizeof(float) * n * dim, hipMemcpyHostToDevice));
    return cross_run(d_v, n, dim, sq_count, sq_bits, K_coarse, coarse, codes, codebooks, M_out, sum_mode, mem);
}

int qadc_opq_train_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                          float* rotation, float* codebooks, int outer, int inner, void* codes_out, uint64_t* empty_out,
                          int* rounds_done_out, int div_mode, int sum_mode, int device_id) {
    return qadc_opq_train_repair_device(d_vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, codebooks, outer, inner, codes_out,
                                        empty_out, rounds_done_out, div_mode, sum_mode, 0, nullptr, device_id);
}

int qadc_opq_train_host(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                        float* rotation, float* codebooks, int outer, int inner, void* codes_out, uint64_t* empty_out,
                        int* rounds_done_out, int div_mode, int sum_mode, int device_id) {
    return qadc_opq_train_repair_host(vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, codebooks, outer, inner, codes_out,
                                      empty_out, rounds_done_out, div_mode, sum_mode, 0, nullptr, device_id);
}

int qadc_opq_train_repair_device(const float* d_vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                                 float* rotation, float* codebooks, int outer, int inner, void* codes_out, uint64_t* empty_out,
                                 int* rounds_done_out, int div_mode, int sum_mode, int repair, uint64_t* repaired_out, int device_id) {
    if (int rc = train_check(d_vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, codebooks, outer, inner, div_mode, sum_mode))
        return rc;
    if (repair != 0 && repair != 1) return fail(QADC_E_ARG, "repair is 0 or 1");
    if (repaired_out) *repaired_out = 0;
    if (int rc = check_aligned(d_vectors, 4, "d_vectors")) return rc;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;
    return train_run(d_vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, codebooks, outer, inner, codes_out, empty_out,
                     rounds_done_out, div_mode, sum_mode, repair, repaired_out, mem);
}

int qadc_opq_train_repair_host(const float* vectors, uint64_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                               float* rotation, float* codebooks, int outer, int inner, void* codes_out, uint64_t* empty_out,
                               int* rounds_done_out, int div_mode, int sum_mode, int repair, uint64_t* repaired_out, int device_id) {
    if (int rc = train_check(vectors, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, codebooks, outer, inner, div_mode, sum_mode))
        return rc;
    if (repair != 0 && repair != 1) return fail(QADC_E_ARG, "repair is 0 or 1");
    if (repaired_out) *repaired_out = 0;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;                                           // the learning set goes up once, for every outer round
    float* d_v = nullptr;
    HIPCHECK(mem.alloc(&d_v, sizeof(float) * n * dim));
    HIPCHECK(hipMemcpy(d_v, vectors, sizeof(float) * n * dim, hipMemcpyHostToDevice));
    return train_run(d_v, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, codebooks, outer, inner, codes_out, empty_out,
                     rounds_done_out, div_mode, sum_mode, repair, repaired_out, mem);
}

}  // extern "C"
