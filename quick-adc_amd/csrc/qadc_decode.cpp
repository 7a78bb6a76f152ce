// PQ decode, stateless (include/qadc.h "Reconstruction"): qadc_pq_decode_host / _device, the inverse of
// qadc_ivf_encode_host, qadc_adc_encode_host and qadc_adc_encode16_host, and the pass loop the index forms (csrc/qadc_adc.cpp)
// share.  The kernels are in csrc/qadc_decode_kernel.hip, their geometry in host/pq_decode_plan.hpp, the CPU twin in
// host/pq_decode.hpp.
#include "qadc_build_shared.h"
#include "qadc_decode.h"

using namespace qadc;
using namespace qadc::host;
using namespace qadc::build;

static_assert(kDecodeChunk == QADC_DECODE_CHUNK, "include/qadc.h names the pass size");

namespace qadc {
namespace host {

int decode_shape_check(int sq_count, int sq_bits, int dim) {
    if (sq_bits != 4 && sq_bits != 8 && sq_bits != 16) return fail(QADC_E_ARG, "sq_bits must be 4, 8 or 16");
    if (!pq_decode_plan_shape_ok(sq_count, sq_bits))
        return fail(QADC_E_ARG, "sq_count must be 16 or 32 at 4 bits, 4, 8 or 16 at 8 bits, 2, 4 or 8 at 16 bits (the encoders' configurations)");
    if (dim <= 0 || dim % sq_count != 0) return fail(QADC_E_ARG, "dim must be a positive multiple of sq_count");
    if (dim > pq_decode_max_dim(sq_bits))
        return fail(QADC_E_ARG, "dim must be <= " + std::to_string(pq_decode_max_dim(sq_bits)) + " at " + std::to_string(sq_bits) + " bits (the encoder's limit)");
    return QADC_OK;
}

int decode_passes(int sq_count, int sq_bits, int dim, const DecodeQuantizers& q, const int32_t* d_assign, const uint8_t* d_codes, uint64_t n,
                  const float* d_vectors, float* d_out, float* d_err, hipStream_t stream) {
    const uint64_t code_bytes = sq_bits == 4 ? sq_count / 2 : sq_bits == 8 ? sq_count : 2 * sq_count;
    for (uint64_t first = 0; first < n; first += kDecodeChunk) {
        const uint64_t rows = std::min<uint64_t>(kDecodeChunk, n - first);
        float* out = d_out + first * (uint64_t)dim;
        PqDecodePlan plan;
        if (!pq_decode_plan(sq_count, sq_bits, dim, rows, (reinterpret_cast<uintptr_t>(out) & 15) == 0, &plan))
            return fail(QADC_E_ARG, "the decode kernels do not take this shape");
        HIPCHECK(launch_pq_decode(plan, q, d_assign ? d_assign + first : nullptr, d_codes + first * code_bytes, rows, out, stream));
        if (d_err) HIPCHECK(launch_pq_decode_err(d_vectors + first * (uint64_t)dim, out, rows, dim, d_err + first, stream));
    }
    return QADC_OK;
}

}  // namespace host
}  // namespace qadc

namespace {

// before the first HIP call
int decode_check(int sq_count, int sq_bits, int dim, const float* codebooks, int K, const float* coarse, const int32_t* assign, const void* codes,
                 uint64_t n, const float* vectors, const float* out, const float* err_out) {
    if (int rc = decode_shape_check(sq_count, sq_bits, dim)) return rc;
    if (!codebooks) return fail(QADC_E_ARG, "codebooks must not be NULL");
    if (K < 0) return fail(QADC_E_ARG, "K must be >= 0");
    if (K > 0 && !coarse) return fail(QADC_E_ARG, "coarse must not be NULL with K > 0");
    if (K > 0 && !assign) return fail(QADC_E_ARG, "assign must not be NULL with K > 0: a row's coarse centroid is assign[i]");
    if (err_out && !vectors) return fail(QADC_E_ARG, "vectors must not be NULL with err_out given: the error is taken against them");
    if (n > 0 && (!codes || !out)) return fail(QADC_E_ARG, "codes and out must not be NULL with n > 0");
    return QADC_OK;
}

// the quantizers into device memory for the call
int upload_quantizers(int sq_count, int sq_bits, int dim, const float* codebooks, const float* rotation, int K, const float* coarse,
                      ScratchFree& mem, DecodeQuantizers* q) {
    const size_t cb_bytes = sizeof(float) * ((size_t)1 << sq_bits) * (size_t)dim;
    float *d_cb = nullptr, *d_rot = nullptr, *d_coarse = nullptr;
    HIPCHECK(mem.alloc(&d_cb, cb_bytes));
    HIPCHECK(hipMemcpy(d_cb, codebooks, cb_bytes, hipMemcpyHostToDevice));
    if (rotation) {
        HIPCHECK(mem.alloc(&d_rot, sizeof(float) * (size_t)dim * dim));
        HIPCHECK(hipMemcpy(d_rot, rotation, sizeof(float) * (size_t)dim * dim, hipMemcpyHostToDevice));
    }
    if (K > 0) {
        HIPCHECK(mem.alloc(&d_coarse, sizeof(float) * (size_t)K * dim));
        HIPCHECK(hipMemcpy(d_coarse, coarse, sizeof(float) * (size_t)K * dim, hipMemcpyHostToDevice));
    }
    *q = DecodeQuantizers{d_cb, d_rot, d_coarse, K};
    return QADC_OK;
}

}  // namespace

extern "C" {

int qadc_pq_decode_device(int sq_count, int sq_bits, int dim, const float* codebooks, const float* rotation, int K, const float* coarse,
                          const int32_t* d_assign, const void* d_codes, uint64_t n, const float* d_vectors, float* d_out, float* d_err_out,
                          int device_id) {
    if (int rc = decode_check(sq_count, sq_bits, dim, codebooks, K, coarse, d_assign, d_codes, n, d_vectors, d_out, d_err_out)) return rc;
    if (int rc = check_aligned(d_assign, 4, "d_assign")) return rc;
    if (int rc = check_aligned(d_vectors, 4, "d_vectors")) return rc;
    if (int rc = check_aligned(d_out, 4, "d_out")) return rc;
    if (int rc = check_aligned(d_err_out, 4, "d_err_out")) return rc;
    if (n == 0) return QADC_OK;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;
    DecodeQuantizers q;
    if (int rc = upload_quantizers(sq_count, sq_bits, dim, codebooks, rotation, K, coarse, mem, &q)) return rc;
    if (int rc = decode_passes(sq_count, sq_bits, dim, q, K > 0 ? d_assign : nullptr, static_cast<const uint8_t*>(d_codes), n, d_vectors, d_out,
                               d_err_out, nullptr))
        return rc;
    HIPCHECK(hipDeviceSynchronize());
    return QADC_OK;
}

int qadc_pq_decode_host(int sq_count, int sq_bits, int dim, const float* codebooks, const float* rotation, int K, const float* coarse,
                        const int32_t* assign, const void* codes, uint64_t n, const float* vectors, float* out, float* err_out, int device_id) {
    if (int rc = decode_check(sq_count, sq_bits, dim, codebooks, K, coarse, assign, codes, n, vectors, out, err_out)) return rc;
    if (n == 0) return QADC_OK;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(device_id));
    ScratchFree mem;
    DecodeQuantizers q;
    if (int rc = upload_quantizers(sq_count, sq_bits, dim, codebooks, rotation, K, coarse, mem, &q)) return rc;
    const uint64_t code_bytes = sq_bits == 4 ? sq_count / 2 : sq_bits == 8 ? sq_count : 2 * sq_count;
    const uint64_t chunk = std::min<uint64_t>(kDecodeChunk, n);   // one pass of scratch, whatever n is
    uint8_t* d_codes = nullptr;
    int32_t* d_assign = nullptr;
    float *d_vectors = nullptr, *d_out = nullptr, *d_err = nullptr;
    HIPCHECK(mem.alloc(&d_codes, chunk * code_bytes));
    HIPCHECK(mem.alloc(&d_out, sizeof(float) * chunk * dim));
    if (K > 0) HIPCHECK(mem.alloc(&d_assign, sizeof(int32_t) * chunk));
    if (err_out) {
        HIPCHECK(mem.alloc(&d_vectors, sizeof(float) * chunk * dim));
        HIPCHECK(mem.alloc(&d_err, sizeof(float) * chunk));
    }
    const uint8_t* src = static_cast<const uint8_t*>(codes);
    for (uint64_t first = 0; first < n; first += chunk) {
        const uint64_t rows = std::min(chunk, n - first);
        HIPCHECK(hipMemcpy(d_codes, src + first * code_bytes, rows * code_bytes, hipMemcpyHostToDevice));
        if (K > 0) HIPCHECK(hipMemcpy(d_assign, assign + first, sizeof(int32_t) * rows, hipMemcpyHostToDevice));
        if (err_out) HIPCHECK(hipMemcpy(d_vectors, vectors + first * dim, sizeof(float) * rows * dim, hipMemcpyHostToDevice));
        if (int rc = decode_passes(sq_count, sq_bits, dim, q, d_assign, d_codes, rows, d_vectors, d_out, d_err, nullptr)) return rc;
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(hipMemcpy(out + first * dim, d_out, sizeof(float) * rows * dim, hipMemcpyDeviceToHost));
        if (err_out) HIPCHECK(hipMemcpy(err_out + first, d_err, sizeof(float) * rows, hipMemcpyDeviceToHost));
    }
    return QADC_OK;
}

}  // extern "C"
