// Kernels of exact re-ranking (qadc_refine_*), gfx950, built with -ffp-contract=off: every result is held
// bit for bit to host/refine.hpp.
//   refine_dist_kernel<Row>     one candidate per wave: the 64-bit word (image of the L2 distance << 32 | key) of every candidate
//   refine_select_kernel<N, T>  one workgroup per query: bitonic sort of the words in LDS, equal words kept once, the first R out
//   refine_convert_kernel<Row>  the append: float -> the store's element type
#include "qadc_refine.h"

#include <hip/hip_fp16.h>

#include <cfloat>

namespace qadc {
namespace refine {

namespace {

constexpr uint32_t kNanImage = 0x7FC00000u;
constexpr uint32_t kInfImage = 0x7F800000u;
constexpr uint64_t kNoWord = ~0ull;

__device__ inline float row_value(const float* x, int i) { return x[i]; }
__device__ inline float row_value(const __half* x, int i) { return __half2float(x[i]); }

// Lane l of a wave owns the partial sum p[l] of the definition: the components 64 j + l, in ascending j, then the tree at the
// strides 32 .. 1 (lane l < s adds lane l + s; what the lanes at and above s compute is never read by a lane below).
template <typename Row>
__global__ __launch_bounds__(kRefineWaves * 64) void refine_dist_kernel(const Row* __restrict__ rows, uint32_t lo, uint64_t nrows, int dim,
                                                                        const float* __restrict__ queries, int r_in,
                                                                        const uint32_t* __restrict__ keys, const int32_t* __restrict__ counts,
                                                                        const float* __restrict__ values, int cands_per_wg, int chunks,
                                                                        uint64_t* __restrict__ words, unsigned long long* __restrict__ missing) {
    extern __shared__ float s_query[];   // [dim]
    __shared__ unsigned s_missing;
    const int q = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* qv = queries + (size_t)q * dim;
    for (int i = tid; i < dim; i += kRefineWaves * 64) s_query[i] = qv[i];
    if (tid == 0) s_missing = 0;
    __syncthreads();

    const int count = counts ? min(max(counts[q], 0), r_in) : r_in;
    const int c0 = chunk * cands_per_wg, c1 = min(r_in, c0 + cands_per_wg);
    const size_t list = (size_t)q * r_in;
    unsigned lost = 0;
    for (int base = c0 + wave * kRefineInFlight; base < c1; base += kRefineWaves * kRefineInFlight) {
        const Row* x[kRefineInFlight];
        uint32_t key[kRefineInFlight];
        float p[kRefineInFlight];
#pragma unroll
        for (int c = 0; c < kRefineInFlight; ++c) {   // (everything here is uniform over the wave)
            const int i = base + c;
            x[c] = nullptr;
            key[c] = 0;
            p[c] = 0.0f;
            if (i < c1 && i < count && !(values && values[list + i] == FLT_MAX)) {
                key[c] = keys[list + i];
                const uint64_t row = (uint64_t)key[c] - lo;
                if (key[c] >= lo && row < nrows)
                    x[c] = rows + row * (uint64_t)dim;
                else
                    ++lost;
            }
        }
        for (int j = lane; j < dim; j += 64) {
            const float qj = s_query[j];
#pragma unroll
            for (int c = 0; c < kRefineInFlight; ++c)
                if (x[c]) {
                    const float t = qj - row_value(x[c], j);
                    const float tt = t * t;
                    p[c] = p[c] + tt;
                }
        }
#pragma unroll
        for (int c = 0; c < kRefineInFlight; ++c) {
            float v = p[c];
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s, 64);
            const int i = base + c;
            if (lane == 0 && i < c1) {
                uint32_t img = __float_as_uint(v);
                if (v != v) img = kNanImage;
                words[list + i] = x[c] ? ((uint64_t)img << 32) | key[c] : kNoWord;
            }
        }
    }
    if (lane == 0 && lost) atomicAdd(&s_missing, lost);
    __syncthreads();
    if (tid == 0 && s_missing) atomicAdd(missing, (unsigned long long)s_missing);
}

// N words (the list, padded with ~0) sorted ascending by T threads; a word survives where it differs from the one before it and
// is not ~0; the survivors' ranks come from a prefix sum over the threads' segments of N / T consecutive words.
template <int N, int T>
__global__ __launch_bounds__(T) void refine_select_kernel(const uint64_t* __restrict__ words, int r_in, int R, uint32_t* __restrict__ out_keys,
                                                          float* __restrict__ out_dist, int32_t* __restrict__ out_sizes) {
    extern __shared__ uint64_t s_words[];             // [N], then uint32 [T]
    uint32_t* s_scan = reinterpret_cast<uint32_t*>(s_words + N);
    const int q = blockIdx.x, tid = threadIdx.x;
    const uint64_t* list = words + (size_t)q * r_in;
    for (int i = tid; i < N; i += T) s_words[i] = i < r_in ? list[i] : kNoWord;
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = tid; t < N / 2; t += T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint64_t a = s_words[i], b = s_words[l];
                if ((a > b) == ((i & k) == 0)) {
                    s_words[i] = b;
                    s_words[l] = a;
                }
            }
        }
    __syncthreads();
    constexpr int S = N / T;
    const int first = tid * S;
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const uint64_t w = s_words[first + i];
        mine += (w != kNoWord && (first + i == 0 || w != s_words[first + i - 1])) ? 1u : 0u;
    }
    s_scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < T; d <<= 1) {                 // inclusive scan over the threads' counts
        const uint32_t add = tid >= d ? s_scan[tid - d] : 0u;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    const uint32_t total = s_scan[T - 1];
    uint32_t rank = s_scan[tid] - mine;
    uint32_t* ok = out_keys + (size_t)q * R;
    float* od = out_dist + (size_t)q * R;
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const uint64_t w = s_words[first + i];
        if (w != kNoWord && (first + i == 0 || w != s_words[first + i - 1])) {
            if (rank < (uint32_t)R) {
                ok[rank] = (uint32_t)w;
                od[rank] = __uint_as_float((uint32_t)(w >> 32));
            }
            ++rank;
        }
    }
    const uint32_t size = min(total, (uint32_t)R);
    for (uint32_t k = size + tid; k < (uint32_t)R; k += T) {
        ok[k] = 0xFFFFFFFFu;
        od[k] = __uint_as_float(kInfImage);
    }
    if (tid == 0) out_sizes[q] = (int32_t)size;
}

__device__ inline void store_as(float* dst, size_t i, float v) { dst[i] = v; }
__device__ inline void store_as(__half* dst, size_t i, float v) { dst[i] = __float2half_rn(v); }

template <typename Row>
__global__ __launch_bounds__(256) void refine_convert_kernel(const float* __restrict__ src, Row* __restrict__ dst, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) store_as(dst, i, src[i]);
}

template <int N, int T>
hipError_t launch_select(const RefinePass& p, const RefinePlan& plan, hipStream_t stream) {
    if (plan.select_lds_bytes > kRefineLdsDefault) {   // the largest instantiation: above the default limit of dynamic LDS
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&refine_select_kernel<N, T>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.select_lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((refine_select_kernel<N, T>), dim3((unsigned)p.nq), dim3(T), plan.select_lds_bytes, stream, p.words, p.r_in, p.R,
                       p.out_keys, p.out_dist, p.out_sizes);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_refine_dist(const RefinePass& p, const RefinePlan& plan, hipStream_t stream) {
    const dim3 grid((unsigned)((uint64_t)p.nq * plan.chunks)), block(kRefineWaves * 64);
    if (p.f16)
        hipLaunchKernelGGL(refine_dist_kernel<__half>, grid, block, plan.dist_lds_bytes, stream, static_cast<const __half*>(p.rows), p.lo,
                           p.nrows, p.dim, p.queries, p.r_in, p.keys, p.counts, p.values, plan.cands_per_wg, plan.chunks, p.words, p.missing);
    else
        hipLaunchKernelGGL(refine_dist_kernel<float>, grid, block, plan.dist_lds_bytes, stream, static_cast<const float*>(p.rows), p.lo,
                           p.nrows, p.dim, p.queries, p.r_in, p.keys, p.counts, p.values, plan.cands_per_wg, plan.chunks, p.words, p.missing);
    return hipGetLastError();
}

hipError_t launch_refine_select(const RefinePass& p, const RefinePlan& plan, hipStream_t stream) {
    switch (plan.sort_n) {
        case 512: return launch_select<512, 256>(p, plan, stream);
        case 2048: return launch_select<2048, 1024>(p, plan, stream);
        case 8192: return launch_select<8192, 1024>(p, plan, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_refine_convert(const float* src, void* dst, bool f16, uint64_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<uint64_t>((n + 255) / 256, 65536)), block(256);
    if (f16)
        hipLaunchKernelGGL(refine_convert_kernel<__half>, grid, block, 0, stream, src, static_cast<__half*>(dst), n);
    else
        hipLaunchKernelGGL(refine_convert_kernel<float>, grid, block, 0, stream, src, static_cast<float*>(dst), n);
    return hipGetLastError();
}

}  // namespace refine
}  // namespace qadc
