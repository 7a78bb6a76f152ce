// Host side of exact re-ranking (qadc_refine_* in include/qadc.h): a store of the original vectors in
// device memory, dense over a key range, and the call that reorders the candidate keys a search returned by their L2 distance to
// those vectors.  The store belongs to no index and shares nothing with either engine but the device's stream set
// (qadc_device_prepare): it consumes uint32 keys, whoever produced them.  The definition it is held to is host/refine.hpp, the
// launch geometry host/refine_plan.hpp, the kernels csrc/qadc_refine_kernel.hip.
//
// Every array of the *_device calls is read and written by kernels only, so memory of another HIP runtime (torch tensors) is
// legal; for the same reason the library cannot ask which device such a pointer lives on, and does not: as for
// qadc_adc_filter_create_device, the caller names the device by the store it hands the pointers to.
#include "../../include/qadc.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../host/refine.hpp"
#include "qadc_host.h"
#include "qadc_refine.h"

using qadc::host::fail;
using qadc::host::DevBuf;
using qadc::host::DeviceGuard;

static_assert(QADC_REFINE_MAX_IN == qadc::refine::kRefinePlanMaxIn && QADC_REFINE_MAX_IN == qadc::refine::kMaxIn, "one limit on r_in");
static_assert(QADC_REFINE_MAX_DIM == qadc::refine::kRefinePlanMaxDim && QADC_REFINE_MAX_DIM == qadc::refine::kMaxDim, "one limit on dim");
static_assert(QADC_REFINE_F32 == qadc::refine::kF32 && QADC_REFINE_F16 == qadc::refine::kF16, "the twin's element types");

struct qadc_refine {
    int dim = 0, dtype = QADC_REFINE_F32, device = 0;
    uint32_t lo = 0;                                // key of row 0 (fixed by the first add)
    uint64_t rows = 0, cap = 0;                     // rows held / rows the allocation holds
    void* data = nullptr;                           // [cap][dim] floats or halves
    uint64_t relocations = 0;                       // adds that moved the rows to grow the allocation
    hipStream_t stream = nullptr;
    // per call
    DevBuf<float> d_stage;                          // add from host memory: floats on their way to the convert kernel
    DevBuf<uint64_t> d_words;                       // [pass_nq][r_in]
    DevBuf<unsigned long long> d_missing;
    DevBuf<float> d_queries, d_values, d_out_dist;  // the host form's arrays in device memory
    DevBuf<uint32_t> d_keys, d_out_keys;
    DevBuf<int32_t> d_counts, d_out_sizes;
    size_t elem() const { return dtype == QADC_REFINE_F16 ? 2 : 4; }
    size_t row_bytes() const { return (size_t)dim * elem(); }
};

namespace {

using namespace qadc::refine;

constexpr uint64_t kStageFloats = 1ull << 24;   // floats of host memory uploaded per pass of an add (64 MiB)

// room for `need` rows: 1.5 x the allocation or `need`, one device-to-device copy of the rows held
int ensure_rows(qadc_refine* r, uint64_t need, bool exact) {
    if (need <= r->cap) return QADC_OK;
    const uint64_t cap = exact ? need : std::max<uint64_t>(need, r->cap + r->cap / 2);
    if (cap > (1ull << 32)) return fail(QADC_E_ARG, "a store holds at most 2^32 rows");
    void* p = nullptr;
    HIPCHECK(hipMalloc(&p, std::max<size_t>((size_t)cap * r->row_bytes(), 16)));
    if (r->rows) {
        hipError_t e = hipMemcpyAsync(p, r->data, (size_t)r->rows * r->row_bytes(), hipMemcpyDeviceToDevice, r->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(r->stream);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return fail(QADC_E_HIP, std::string("moving the rows: ") + hipGetErrorString(e));
        }
        ++r->relocations;
    }
    if (r->data) (void)hipFree(r->data);
    r->data = p;
    r->cap = cap;
    return QADC_OK;
}

int add_rows(qadc_refine* r, const float* vectors, uint64_t count, uint32_t first_key, bool d_side) {
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (count == 0) return QADC_OK;
    if (!vectors) return fail(QADC_E_ARG, "vectors is null");
    if (r->rows && (uint64_t)first_key != (uint64_t)r->lo + r->rows)
        return fail(QADC_E_ARG, "first_key " + std::to_string(first_key) + " does not continue the store, which holds the keys [" +
                                    std::to_string(r->lo) + ", " + std::to_string((uint64_t)r->lo + r->rows) + ")");
    if ((uint64_t)first_key + count > (1ull << 32)) return fail(QADC_E_ARG, "first_key + count passes 2^32");
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    if (int rc = ensure_rows(r, r->rows + count, false)) return rc;
    char* dst = static_cast<char*>(r->data) + (size_t)r->rows * r->row_bytes();
    const bool f16 = r->dtype == QADC_REFINE_F16;
    const uint64_t n = count * (uint64_t)r->dim;
    if (d_side) {
        HIPCHECK(launch_refine_convert(vectors, dst, f16, n, r->stream));
    } else if (!f16) {
        HIPCHECK(hipMemcpyAsync(dst, vectors, (size_t)n * 4, hipMemcpyHostToDevice, r->stream));
    } else {
        HIPCHECK(r->d_stage.ensure((size_t)std::min(n, kStageFloats)));
        for (uint64_t i = 0; i < n; i += kStageFloats) {
            const uint64_t m = std::min(kStageFloats, n - i);
            HIPCHECK(hipMemcpyAsync(r->d_stage.p, vectors + i, (size_t)m * 4, hipMemcpyHostToDevice, r->stream));
            HIPCHECK(launch_refine_convert(r->d_stage.p, dst + (size_t)i * 2, true, m, r->stream));
            HIPCHECK(hipStreamSynchronize(r->stream));   // (the stage is written again by the next pass)
        }
    }
    HIPCHECK(hipStreamSynchronize(r->stream));
    if (r->rows == 0) r->lo = first_key;
    r->rows += count;
    return QADC_OK;
}

int check_rerank(const qadc_refine* r, int nq, const float* queries, int r_in, const uint32_t* keys, int R, const uint32_t* out_keys,
                 const float* out_dist, const int32_t* out_sizes) {
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (nq < 0) return fail(QADC_E_ARG, "nq is negative");
    if (r_in < 1 || r_in > QADC_REFINE_MAX_IN) return fail(QADC_E_ARG, "r_in is 1 .. " + std::to_string(QADC_REFINE_MAX_IN) + " (QADC_REFINE_MAX_IN)");
    if (R < 1) return fail(QADC_E_ARG, "R is at least 1");
    if (nq && (!queries || !keys || !out_keys || !out_dist || !out_sizes))
        return fail(QADC_E_ARG, "queries, keys, out_keys, out_dist and out_sizes must not be null");
    return QADC_OK;
}

// The passes of a call on arrays in device memory; the stream is drained before the call returns.
int rerank_passes(qadc_refine* r, int nq, const float* queries, int r_in, const uint32_t* keys, const int32_t* counts, const float* values,
                  int R, uint32_t* out_keys, float* out_dist, int32_t* out_sizes, uint64_t* missing_out) {
    RefinePlan plan;
    if (!refine_plan(nq, r_in, r->dim, &plan)) return fail(QADC_E_ARG, "no launch geometry for this call");
    HIPCHECK(r->d_words.ensure((size_t)plan.pass_nq * r_in));
    HIPCHECK(r->d_missing.ensure(1));
    HIPCHECK(hipMemsetAsync(r->d_missing.p, 0, sizeof(unsigned long long), r->stream));
    for (int q0 = 0; q0 < nq; q0 += plan.pass_nq) {
        RefinePass p;
        p.rows = r->data;
        p.f16 = r->dtype == QADC_REFINE_F16;
        p.lo = r->lo;
        p.nrows = r->rows;
        p.dim = r->dim;
        p.nq = std::min(plan.pass_nq, nq - q0);
        p.r_in = r_in;
        p.R = R;
        p.queries = queries + (size_t)q0 * r->dim;
        p.keys = keys + (size_t)q0 * r_in;
        p.counts = counts ? counts + q0 : nullptr;
        p.values = values ? values + (size_t)q0 * r_in : nullptr;
        p.words = r->d_words.p;
        p.missing = r->d_missing.p;
        p.out_keys = out_keys + (size_t)q0 * R;
        p.out_dist = out_dist + (size_t)q0 * R;
        p.out_sizes = out_sizes + q0;
        HIPCHECK(launch_refine_dist(p, plan, r->stream));
        HIPCHECK(launch_refine_select(p, plan, r->stream));
    }
    unsigned long long missing = 0;
    HIPCHECK(hipMemcpyAsync(&missing, r->d_missing.p, sizeof(missing), hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipStreamSynchronize(r->stream));
    if (missing_out) *missing_out = missing;
    return QADC_OK;
}

}  // namespace

extern "C" {

int qadc_refine_create(qadc_refine** out, int dim, int dtype, int device_id) {
    if (!out) return fail(QADC_E_ARG, "out is null");
    *out = nullptr;
    if (dim < 1 || dim > QADC_REFINE_MAX_DIM) return fail(QADC_E_ARG, "dim is 1 .. " + std::to_string(QADC_REFINE_MAX_DIM));
    if (dtype != QADC_REFINE_F32 && dtype != QADC_REFINE_F16) return fail(QADC_E_ARG, "dtype is 0 (QADC_REFINE_F32) or 1 (QADC_REFINE_F16)");
    DeviceGuard guard;
    if (int rc = qadc_device_prepare(device_id)) return rc;   // (the device's stream set first: DESIGN.md section 5)
    HIPCHECK(hipSetDevice(device_id));
    qadc_refine* r = new qadc_refine();
    r->dim = dim;
    r->dtype = dtype;
    r->device = device_id;
    const hipError_t e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete r;
        return fail(QADC_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    *out = r;
    return QADC_OK;
}

int qadc_refine_destroy(qadc_refine* r) {
    if (!r) return QADC_OK;
    DeviceGuard guard;
    (void)hipSetDevice(r->device);
    if (r->stream) {
        (void)hipStreamSynchronize(r->stream);
        (void)hipStreamDestroy(r->stream);
    }
    if (r->data) (void)hipFree(r->data);
    r->d_stage.release(); r->d_words.release(); r->d_missing.release(); r->d_queries.release(); r->d_values.release();
    r->d_out_dist.release(); r->d_keys.release(); r->d_out_keys.release(); r->d_counts.release(); r->d_out_sizes.release();
    delete r;
    return QADC_OK;
}

int qadc_refine_add(qadc_refine* r, const float* vectors, uint64_t count, uint32_t first_key) {
    return add_rows(r, vectors, count, first_key, false);
}

int qadc_refine_add_device(qadc_refine* r, const float* d_vectors, uint64_t count, uint32_t first_key) {
    return add_rows(r, d_vectors, count, first_key, true);
}

int qadc_refine_reserve(qadc_refine* r, uint64_t rows) {
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (rows > (1ull << 32)) return fail(QADC_E_ARG, "a store holds at most 2^32 rows");
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    return ensure_rows(r, rows, true);
}

int qadc_refine_info(const qadc_refine* r, int* dim, int* dtype, uint32_t* lo, uint64_t* rows, uint64_t* bytes) {
    if (!r) return fail(QADC_E_ARG, "store is null");
    if (dim) *dim = r->dim;
    if (dtype) *dtype = r->dtype;
    if (lo) *lo = r->lo;
    if (rows) *rows = r->rows;
    if (bytes) *bytes = r->cap * (uint64_t)r->row_bytes();
    return QADC_OK;
}

uint64_t qadc_refine_relocations(const qadc_refine* r) { return r ? r->relocations : 0; }

int qadc_refine_rerank(qadc_refine* r, int nq, const float* queries, int r_in, const uint32_t* keys, const int32_t* counts,
                       const float* values, int R, uint32_t* out_keys, float* out_dist, int32_t* out_sizes, uint64_t* missing_out) {
    if (int rc = check_rerank(r, nq, queries, r_in, keys, R, out_keys, out_dist, out_sizes)) return rc;
    if (counts)
        for (int q = 0; q < nq; ++q)
            if (counts[q] < 0 || counts[q] > r_in)
                return fail(QADC_E_ARG, "counts[" + std::to_string(q) + "] = " + std::to_string(counts[q]) + " is outside [0, r_in]");
    if (missing_out) *missing_out = 0;
    if (nq == 0) return QADC_OK;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    const size_t nin = (size_t)nq * r_in, nout = (size_t)nq * R;
    HIPCHECK(r->d_queries.ensure((size_t)nq * r->dim));
    HIPCHECK(r->d_keys.ensure(nin));
    HIPCHECK(r->d_out_keys.ensure(nout));
    HIPCHECK(r->d_out_dist.ensure(nout));
    HIPCHECK(r->d_out_sizes.ensure(nq));
    HIPCHECK(hipMemcpyAsync(r->d_queries.p, queries, (size_t)nq * r->dim * 4, hipMemcpyHostToDevice, r->stream));
    HIPCHECK(hipMemcpyAsync(r->d_keys.p, keys, nin * 4, hipMemcpyHostToDevice, r->stream));
    if (counts) {
        HIPCHECK(r->d_counts.ensure(nq));
        HIPCHECK(hipMemcpyAsync(r->d_counts.p, counts, (size_t)nq * 4, hipMemcpyHostToDevice, r->stream));
    }
    if (values) {
        HIPCHECK(r->d_values.ensure(nin));
        HIPCHECK(hipMemcpyAsync(r->d_values.p, values, nin * 4, hipMemcpyHostToDevice, r->stream));
    }
    uint64_t missing = 0;
    if (int rc = rerank_passes(r, nq, r->d_queries.p, r_in, r->d_keys.p, counts ? r->d_counts.p : nullptr, values ? r->d_values.p : nullptr, R,
                               r->d_out_keys.p, r->d_out_dist.p, r->d_out_sizes.p, &missing))
        return rc;
    HIPCHECK(hipMemcpyAsync(out_keys, r->d_out_keys.p, nout * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipMemcpyAsync(out_dist, r->d_out_dist.p, nout * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipMemcpyAsync(out_sizes, r->d_out_sizes.p, (size_t)nq * 4, hipMemcpyDeviceToHost, r->stream));
    HIPCHECK(hipStreamSynchronize(r->stream));
    if (missing_out) *missing_out = missing;
    return QADC_OK;
}

int qadc_refine_rerank_device(qadc_refine* r, int nq, const float* d_queries, int r_in, const uint32_t* d_keys, const int32_t* d_counts,
                              const float* d_values, int R, uint32_t* d_out_keys, float* d_out_dist, int32_t* d_out_sizes,
                              uint64_t* missing_out) {
    if (int rc = check_rerank(r, nq, d_queries, r_in, d_keys, R, d_out_keys, d_out_dist, d_out_sizes)) return rc;
    if (missing_out) *missing_out = 0;
    if (nq == 0) return QADC_OK;
    DeviceGuard guard;
    HIPCHECK(hipSetDevice(r->device));
    return rerank_passes(r, nq, d_queries, r_in, d_keys, d_counts, d_values, R, d_out_keys, d_out_dist, d_out_sizes, missing_out);
}

}  // extern "C"
