// OPQ learning: the cross matrix M = X0^T Y between the learning set and its reconstruction.
//
// The contract fixes every float: per block j of kOpqBlock vectors and per (a, b) ONE chain acc = fmaf(X0[i][a], Y[i][b], acc) in
// ascending i from 0.0f, then the blocks' partials added in ascending j in double.  So a lane owns whole chains (a REG x REG tile
// of them in registers) and walks its block; no float atomics, no tree, no split chain.  The workgroup stages kOpqStage vectors'
// X0 columns and gathered Y columns through LDS per step.  The codebook rows are gathered through the L2 while staging: at 8 x 8
// and dim 128 the codebooks are 128 KB, more than a workgroup's LDS, and every staged Y entry is read once from memory and
// REG * kOpqLanes times from LDS.  Geometry: host/opq_plan.hpp.  Built with -ffp-contract=off; the fused operation is explicit.
#include "qadc_opq.h"

namespace qadc {

template <int REG>
__global__ __launch_bounds__(kOpqWG) void opq_cross_kernel(const float* __restrict__ x0, uint64_t n, const uint8_t* __restrict__ codes,
                                                           const float* __restrict__ codebooks, int sq_bits, OpqCrossPlan p,
                                                           float* __restrict__ partials) {
    constexpr int TILE = kOpqLanes * REG;
    constexpr int kStageRegs = kOpqStage * TILE / kOpqWG;         // staged entries per lane and window: 2, 4 or 8
    __shared__ __attribute__((aligned(16))) float xs[kOpqStage][TILE];
    __shared__ __attribute__((aligned(16))) float ys[kOpqStage][TILE];
    const int tid = threadIdx.x;
    const uint32_t per_block = (uint32_t)(p.tiles * p.tiles);
    const uint64_t j = blockIdx.x / per_block;                    // the block of vectors
    const int t = (int)(blockIdx.x % per_block), ta = t / p.tiles, tb = t - ta * p.tiles;
    const int a0 = ta * TILE, b0 = tb * TILE;
    const uint64_t i_begin = j * (uint64_t)kOpqBlock, i_end = min(n, i_begin + (uint64_t)kOpqBlock);
    const int la = tid / kOpqLanes, lb = tid % kOpqLanes;
    const uint32_t code_mask = sq_bits == 4 ? 15u : 255u;

    float acc[REG][REG];
#pragma unroll
    for (int ra = 0; ra < REG; ++ra)
#pragma unroll
        for (int rb = 0; rb < REG; ++rb) acc[ra][rb] = 0.0f;

    for (uint64_t i0 = i_begin; i0 < i_end; i0 += (uint64_t)kOpqStage) {
        const int steps = (int)min((uint64_t)kOpqStage, i_end - i0);
        __syncthreads();                                          // the walk over the previous step is over
#pragma unroll
        for (int r = 0; r < kStageRegs; ++r) {
            const int e = tid + kOpqWG * r, s = e / TILE, c = e - s * TILE;
            const uint64_t i = i0 + (uint64_t)s;                  // read only where s < steps: i < i_end <= n
            const int a = a0 + c, b = b0 + c;
            float xv = 0.0f, yv = 0.0f;
            if (s < steps && a < p.dim) xv = x0[i * (uint64_t)p.dim + (uint64_t)a];
            if (s < steps && b < p.dim) {
                const int m = b / p.dsub, d = b - m * p.dsub;
                const uint32_t byte = codes[i * (uint64_t)p.code_bytes + (uint64_t)(sq_bits == 4 ? m >> 1 : m)];
                const uint32_t code = (sq_bits == 4 ? byte >> (4 * (m & 1)) : byte) & code_mask;   // < K: the gather stays inside
                yv = codebooks[((size_t)m * p.K + code) * p.dsub + d];
            }
            xs[s][c] = xv;
            ys[s][c] = yv;
        }
        __syncthreads();
        for (int s = 0; s < steps; ++s) {                         // ascending vector index: the pinned order
            float xr[REG], yr[REG];
#pragma unroll
            for (int r = 0; r < REG; ++r) {
                xr[r] = xs[s][la * REG + r];
                yr[r] = ys[s][lb * REG + r];
            }
#pragma unroll
            for (int ra = 0; ra < REG; ++ra)
#pragma unroll
                for (int rb = 0; rb < REG; ++rb) acc[ra][rb] = __fmaf_rn(xr[ra], yr[rb], acc[ra][rb]);
        }
    }
    float* out = partials + j * (uint64_t)p.dim * (uint64_t)p.dim;
#pragma unroll
    for (int ra = 0; ra < REG; ++ra)
#pragma unroll
        for (int rb = 0; rb < REG; ++rb) {
            const int a = opq_cross_row(REG, ta, tid, ra), b = opq_cross_col(REG, tb, tid, rb);
            if (a < p.dim && b < p.dim) out[(size_t)a * p.dim + b] = acc[ra][rb];
        }
}

// one lane per (a, b): the blocks' partials in ascending j, in double from 0.0
__global__ __launch_bounds__(kOpqReduceWG) void opq_cross_reduce_kernel(const float* __restrict__ partials, uint64_t blocks, int dim,
                                                                        double* __restrict__ M) {
    const uint32_t e = blockIdx.x * (uint32_t)kOpqReduceWG + threadIdx.x, cells = (uint32_t)(dim * dim);
    if (e >= cells) return;
    double sum = 0.0;
    for (uint64_t j = 0; j < blocks; ++j) sum += (double)partials[j * (uint64_t)cells + e];
    M[e] = sum;
}

hipError_t launch_opq_cross(const float* d_x0, uint64_t n, int dim, int sq_count, int sq_bits, const uint8_t* d_codes,
                            const float* d_codebooks, float* d_partials, double* d_M, hipStream_t stream) {
    OpqCrossPlan p;
    if (!opq_cross_plan(dim, sq_count, sq_bits, n, &p) || !d_x0 || !d_codes || !d_codebooks || !d_partials || !d_M)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)p.grid), wg(kOpqWG);
    if (p.reg == 1)
        hipLaunchKernelGGL(opq_cross_kernel<1>, grid, wg, 0, stream, d_x0, n, d_codes, d_codebooks, sq_bits, p, d_partials);
    else if (p.reg == 2)
        hipLaunchKernelGGL(opq_cross_kernel<2>, grid, wg, 0, stream, d_x0, n, d_codes, d_codebooks, sq_bits, p, d_partials);
    else
        hipLaunchKernelGGL(opq_cross_kernel<4>, grid, wg, 0, stream, d_x0, n, d_codes, d_codebooks, sq_bits, p, d_partials);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(opq_cross_reduce_kernel, dim3(p.reduce_grid), dim3(kOpqReduceWG), 0, stream, d_partials, p.blocks, dim, d_M);
    return hipGetLastError();
}

}  // namespace qadc
