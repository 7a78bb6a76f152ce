// PQ training: the centroid update of all sq_count * K centroids in one launch.
//
// The contract fixes the order of every float sum: per (sub-quantizer m, centroid k, component d) ONE running sum over the
// learning set in ascending vector index (kmeans_fast_iterations_thread, databases.cpp:67-88, on the columns of m).  So a lane
// owns one such chain and walks the whole learning set: acc = (code == k) ? acc + x : acc.  No float atomics, no tree, no
// per-wave partial sums.  The workgroup stages `chunk` vectors' columns and codes through LDS per step; the next step's
// global loads are issued into registers before the walk over the current one, so the walk hides them.  Geometry:
// host/pq_train_plan.hpp.  Built with -ffp-contract=off like every kernel whose sums are pinned.
#include "qadc_pq_train.h"

#include <algorithm>

namespace qadc {

namespace {
constexpr int kXRegs = kPqTrainStage / kPqTrainWG;          // 16 staged floats per lane and step
constexpr int kCRegs = kPqTrainCodeStage / kPqTrainWG;      // 16 staged codes per lane and step
constexpr uint32_t kNone = 0xFFFFFFFFu;
}  // namespace

__global__ __launch_bounds__(kPqTrainWG) void pq_train_update_kernel(const float* __restrict__ x, uint64_t n, int dim, int sq_count,
                                                                     int sq_bits, const uint8_t* __restrict__ codes,
                                                                     float* __restrict__ codebooks, PqTrainPlan p, int div_mode) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    float* xs = reinterpret_cast<float*>(dyn);                                    // [chunk][cols] of this step
    uint8_t* cs = dyn + (size_t)p.chunk * p.cols * sizeof(float);                 // [chunk][mhere] codes of this step
    const int tid = threadIdx.x, b = blockIdx.x;
    const int db = b % p.dblocks, kbi = (b / p.dblocks) % p.kblocks, mb = b / (p.dblocks * p.kblocks);
    const int m0 = mb * p.mper, k0 = kbi * p.kper, d0 = db * p.width;
    const int mhere = min(p.mper, sq_count - m0);                                 // (the last block of sub-quantizers may be short)
    const int cbase = m0 * p.dsub + d0;                                           // first staged column
    const int cols = p.mper > 1 ? mhere * p.dsub : min(p.width, p.dsub - d0);     // staged columns: cbase + cols <= dim
    const int code_bytes = sq_bits == 4 ? sq_count / 2 : sq_count;
    const uint32_t code_mask = sq_bits == 4 ? 15u : 255u;

    // this lane's chain: (m0 + ml, k0 + kl, d0 + dl), d fastest
    const int per = p.kper * p.width;
    const int ml = tid / per, rem = tid - ml * per, kl = rem / p.width, dl = rem - kl * p.width;
    const bool owns = ml < mhere && k0 + kl < p.K && d0 + dl < p.dsub;
    const int kk = owns ? k0 + kl : -1;                                           // (-1 matches no code)
    const float* xp = xs + (owns ? ml * p.dsub + dl : 0);
    const uint8_t* cp = cs + (owns ? ml : 0);

    // what this lane stages per step, fixed for the whole walk: entries tid + 256 r of the window (row-major [j][column]) and of the
    // codes ([j][sub-quantizer]).  xoff: byte offset from the step's first vector; coff: (byte offset << 1) | high nibble.
    uint32_t xoff[kXRegs], coff[kCRegs];
#pragma unroll
    for (int r = 0; r < kXRegs; ++r) {
        const int idx = tid + kPqTrainWG * r;
        xoff[r] = kNone;
        if (idx < p.chunk * cols) {
            const int j = idx / cols, c = idx - j * cols;
            xoff[r] = ((uint32_t)j * (uint32_t)dim + (uint32_t)(cbase + c)) * 4u;     // (< 256 * 4096 * 4)
        }
    }
#pragma unroll
    for (int r = 0; r < kCRegs; ++r) {
        const int idx = tid + kPqTrainWG * r;
        coff[r] = kNone;
        if (idx < p.chunk * mhere) {
            const int j = idx / mhere, m = m0 + (idx - j * mhere);
            coff[r] = sq_bits == 4 ? ((uint32_t)(j * code_bytes + (m >> 1)) << 1) | (uint32_t)(m & 1)
                                   : (uint32_t)(j * code_bytes + m) << 1;
        }
    }
    const uint64_t xbytes = n * (uint64_t)dim * 4u, cbytes = n * (uint64_t)code_bytes;
    float xv[kXRegs];
    uint32_t cv[kCRegs];
    // Every load is issued: an entry this lane does not stage, or one of a row >= n (its offset is not below what is left of the
    // array: column < dim, byte < code_bytes), reads the step's first element instead, which exists.  What it returns is never used.
#define QADC_PQ_TRAIN_PREFETCH(i0_)                                                                                   \
    do {                                                                                                              \
        const uint64_t xb_ = (i0_) * (uint64_t)dim * 4u, cb_ = (i0_) * (uint64_t)code_bytes;                          \
        const uint32_t xleft_ = (uint32_t)min(xbytes - xb_, (uint64_t)kNone), cleft_ = (uint32_t)min(cbytes - cb_, (uint64_t)kNone); \
        const char* xsrc_ = reinterpret_cast<const char*>(x) + xb_;                                                   \
        const uint8_t* csrc_ = codes + cb_;                                                                           \
        _Pragma("unroll") for (int r = 0; r < kXRegs; ++r)                                                            \
            xv[r] = *reinterpret_cast<const float*>(xsrc_ + (xoff[r] < xleft_ ? xoff[r] : 0u));                       \
        _Pragma("unroll") for (int r = 0; r < kCRegs; ++r)                                                            \
            cv[r] = csrc_[(coff[r] >> 1) < cleft_ ? (coff[r] >> 1) : 0u];                                             \
    } while (0)

    float acc = 0.0f;
    uint32_t count = 0;
    QADC_PQ_TRAIN_PREFETCH((uint64_t)0);
    for (uint64_t i0 = 0; i0 < n; i0 += (uint64_t)p.chunk) {
        __syncthreads();                                                          // the walk over the previous step is over
#pragma unroll
        for (int r = 0; r < kXRegs; ++r)
            if (xoff[r] != kNone) xs[tid + kPqTrainWG * r] = xv[r];
#pragma unroll
        for (int r = 0; r < kCRegs; ++r)
            if (coff[r] != kNone) cs[tid + kPqTrainWG * r] = (uint8_t)((cv[r] >> (4 * (coff[r] & 1))) & code_mask);
        __syncthreads();
        if (i0 + (uint64_t)p.chunk < n) QADC_PQ_TRAIN_PREFETCH(i0 + (uint64_t)p.chunk);
        const int steps = (int)min((uint64_t)p.chunk, n - i0);
#pragma unroll 8
        for (int j = 0; j < steps; ++j) {                                         // ascending vector index: the pinned order
            const bool hit = (int)cp[j * mhere] == kk;
            const float v = xp[j * cols];
            acc = hit ? acc + v : acc;
            count += hit ? 1u : 0u;
        }
    }
#undef QADC_PQ_TRAIN_PREFETCH
    if (owns) {
        const float cf = (float)(int)count;
        codebooks[((size_t)(m0 + ml) * p.K + kk) * p.dsub + d0 + dl] = div_mode ? acc * (1.0f / cf) : acc / cf;
    }
}

hipError_t launch_pq_train_update(const float* d_x, uint64_t n, int dim, int sq_count, int sq_bits, const uint8_t* d_codes,
                                  float* d_codebooks, int div_mode, hipStream_t stream) {
    PqTrainPlan p;
    if (!pq_train_plan(sq_count, sq_bits, dim, &p) || n == 0 || !d_x || !d_codes || !d_codebooks) return hipErrorInvalidValue;
    if (sq_bits == 4 && sq_count % 2 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pq_train_update_kernel, dim3(p.grid), dim3(kPqTrainWG), p.lds_bytes, stream, d_x, n, dim, sq_count, sq_bits,
                       d_codes, d_codebooks, p, div_mode);
    return hipGetLastError();
}

}  // namespace qadc
