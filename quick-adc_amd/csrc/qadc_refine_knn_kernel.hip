// Kernels of the exhaustive search over a refine store (qadc_refine_knn), gfx950, built with
// -ffp-contract=off: every result is held bit for bit to refine::knn of host/refine.hpp.  The geometry is host/refine_knn_plan.hpp.
//   refine_knn_dist_kernel<M, Row, QT, J>  a workgroup owns a tile of QT queries and a slice of rows; a wave reads a row once and forms
//                                       its distance to every query of the tile; the words that pass the bound are appended
//   refine_knn_select_kernel            one workgroup per (query, group): the buffer's first R words, the bound lowered to the R-th
//   refine_knn_final_kernel<M>          one workgroup per query: the groups' lists merged, the outputs written
// M is the store's metric (csrc/qadc_refine_dev.h: MetricL2, MetricIP).
#include "qadc_refine_dev.h"

#include <type_traits>

namespace qadc {
namespace refine {

namespace {

// Lane l keeps the components 64 j + l of the tile's queries and of the row, so p[q] is lane l's partial sum p[l] of the definition
// for query q: j ascending, t = q - x, t * t and p + tt each rounded alone.  A component that does not exist is 0 in both (register
// tile) or is left out (LDS tile): p is +0, positive or NaN, and p + (+0) is p.  Under MetricIP the term is q * x rounded alone and p
// takes either sign; a component that does not exist is 0 * 0 = +0 on the register tile, and p + (+0) is p there too: a lane's p
// starts at +0 and IEEE addition gives -0 only from two -0 operands, so p is never -0 (nor is any value of the fold).
//
// The fold.  The definition's tree is p[l] = p[l] + p[l + s] for l < s at s = 32 .. 1.  Folding QT values one by one costs six
// shuffles each; instead the wave folds them as a transpose: at stride s the lanes with bit s clear finish the lower half of the
// values they hold — p[l] + p[l + s], the definition's operands in the definition's order — and the lanes with bit s set the upper
// half, as p[l] + p[l - s]: the same two operands, and IEEE addition is commutative (only a NaN's payload can tell, and every NaN
// becomes 0x7FC00000).  After log2(QT) strides a lane holds one value, that of query lane >> (6 - log2(QT)) of the tile; the
// remaining strides fold it the plain way and the lanes whose low 6 - log2(QT) bits are zero hold D.
//
// SQ8 rows: a register tile keeps vmin and step of the lane's components in registers beside the queries' (2 J more); an LDS tile,
// which may fill the LDS by itself, reads them from global memory with the row's bytes (coalesced, and the same for every row).
// The row's bytes are loaded one per lane and component here: the dword-and-exchange form of refine_dist_kernel was measured in this
// kernel too and is slower in it.
template <typename M, typename Row, int QT, int J>
__global__ __launch_bounds__(kKnnWaves * 64) void refine_knn_dist_kernel(const Row* __restrict__ rows, uint32_t lo, uint64_t nrows,
                                                                         const uint32_t* __restrict__ row_key, adc::ScanFilter filter, int dim,
                                                                         const float* __restrict__ sq_vmin, const float* __restrict__ sq_step,
                                                                         const float* __restrict__ queries, int nq, uint64_t chunk_rows,
                                                                         int groups, int slice_rows, int slices, uint64_t launch, uint64_t buf_cap,
                                                                         uint64_t* __restrict__ buf, uint32_t* __restrict__ cnt,
                                                                         const uint64_t* __restrict__ bound) {
    extern __shared__ float s_tile[];   // LDS tile (J == 0): [QT][dim]
    constexpr int kShift = 6 - knn_log2(QT), JR = J > 0 ? J : 1;
    constexpr bool kSq = std::is_same<Row, sq8_t>::value;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int q0 = blockIdx.x * QT, group = blockIdx.y / slices, slice = blockIdx.y % slices;

    float qr[QT][JR], vr[JR], sr[JR];
#pragma unroll
    for (int j = 0; j < JR; ++j) {
        const int i = 64 * j + lane;
        vr[j] = (kSq && J > 0 && i < dim) ? sq_vmin[i] : 0.0f;
        sr[j] = (kSq && J > 0 && i < dim) ? sq_step[i] : 0.0f;
    }
    if (J > 0) {
#pragma unroll
        for (int q = 0; q < QT; ++q)
#pragma unroll
            for (int j = 0; j < JR; ++j) {
                const int i = 64 * j + lane;
                qr[q][j] = (q0 + q < nq && i < dim) ? queries[(size_t)(q0 + q) * dim + i] : 0.0f;
            }
    } else {
        for (int e = tid; e < QT * dim; e += kKnnWaves * 64) {
            const int q = e / dim;
            s_tile[e] = q0 + q < nq ? queries[(size_t)q0 * dim + e] : 0.0f;
        }
        __syncthreads();
    }

    const int myq = q0 + (lane >> kShift);
    const bool emitter = (lane & ((1 << kShift) - 1)) == 0 && myq < nq;
    const size_t slot = (size_t)(emitter ? myq : q0) * groups + group;
    const uint64_t my_bound = emitter ? bound[slot] : 0ull;

    uint64_t first, last;
    knn_slice(nrows, chunk_rows, groups, slice_rows, launch, group, slice, &first, &last);
    for (uint64_t r = first + wave; r < last; r += kKnnWaves) {
        // (the row, its key and the filter's verdict are the same in every lane of the wave)
        const uint32_t key = __builtin_amdgcn_readfirstlane(row_key ? row_key[r] : lo + (uint32_t)r);
        if (row_key && key == kKeyedEmpty) continue;
        if (filter.bitmap && !knn_passes(filter, key)) continue;
        const Row* x = rows + r * (uint64_t)dim;
        float p[QT];
#pragma unroll
        for (int q = 0; q < QT; ++q) p[q] = 0.0f;
        if (J > 0) {
#pragma unroll
            for (int j = 0; j < JR; ++j) {
                const int i = 64 * j + lane;
                const float xv = i < dim ? row_value(x, i, vr[j], sr[j]) : 0.0f;
#pragma unroll
                for (int q = 0; q < QT; ++q) {
                    const float tt = M::term(qr[q][j], xv);
                    p[q] = p[q] + tt;
                }
            }
        } else {
            for (int i = lane; i < dim; i += 64) {
                const float xv = row_value(x, i, kSq ? sq_vmin[i] : 0.0f, kSq ? sq_step[i] : 0.0f);
#pragma unroll
                for (int q = 0; q < QT; ++q) {
                    const float tt = M::term(s_tile[q * dim + i], xv);
                    p[q] = p[q] + tt;
                }
            }
        }
        const float v = knn_fold<QT>(p, lane);
        if (emitter) {
            const uint64_t word = ((uint64_t)M::image(v) << 32) | key;
            if (word <= my_bound) {
                const uint32_t pos = atomicAdd(cnt + slot, 1u);
                if (pos < buf_cap) buf[slot * buf_cap + pos] = word;   // (a launch appends at most chunk_rows words to at most R)
            }
        }
    }
}

// grid (nq, groups of the launch).  A buffer with fewer than R words, or with the R words the last select left, stays as it is.
// The words of a buffer differ (a store holds a key once), so the first R are the R smallest whatever order they arrived in.
__global__ __launch_bounds__(1024) void refine_knn_select_kernel(int R, int groups, uint64_t buf_cap, uint64_t* __restrict__ buf,
                                                                 uint32_t* __restrict__ cnt, uint64_t* __restrict__ bound) {
    extern __shared__ uint64_t s_words[];
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t slot = (size_t)blockIdx.x * groups + blockIdx.y;
    const uint32_t n = min(cnt[slot], (uint32_t)buf_cap);
    if (n < (uint32_t)R || (n == (uint32_t)R && bound[slot] != kNoWord)) return;
    uint64_t* list = buf + slot * buf_cap;
    const int N = knn_sort_size(n);
    for (int i = tid; i < N; i += T) s_words[i] = (uint32_t)i < n ? list[i] : kNoWord;
    knn_sort(s_words, N, tid, T);
    for (int i = tid; i < R; i += T) list[i] = s_words[i];
    if (tid == 0) {
        cnt[slot] = (uint32_t)R;
        bound[slot] = s_words[R - 1];
    }
}

// grid nq.  Every group's buffer holds at most R words here (the select ran behind every distance launch).
template <typename M>
__global__ __launch_bounds__(1024) void refine_knn_final_kernel(int R, int groups, int live_groups, uint64_t buf_cap,
                                                                const uint64_t* __restrict__ buf, const uint32_t* __restrict__ cnt,
                                                                uint32_t* __restrict__ out_keys, float* __restrict__ out_dist,
                                                                int32_t* __restrict__ out_sizes) {
    extern __shared__ uint64_t s_words[];
    const int tid = threadIdx.x, T = blockDim.x, q = blockIdx.x;
    uint32_t total = 0;
    for (int g = 0; g < live_groups; ++g) {
        const size_t slot = (size_t)q * groups + g;
        const uint32_t n = min(cnt[slot], (uint32_t)R);
        for (uint32_t i = tid; i < n; i += T) s_words[total + i] = buf[slot * buf_cap + i];
        total += n;
    }
    const int N = knn_sort_size(total);
    for (int i = total + tid; i < N; i += T) s_words[i] = kNoWord;
    knn_sort(s_words, N, tid, T);
    const uint32_t size = min(total, (uint32_t)R);
    uint32_t* ok = out_keys + (size_t)q * R;
    float* od = out_dist + (size_t)q * R;
    for (uint32_t i = tid; i < (uint32_t)R; i += T) {
        const bool held = i < size;
        const uint64_t w = held ? s_words[i] : 0ull;
        ok[i] = held ? (uint32_t)w : 0xFFFFFFFFu;
        od[i] = held ? M::value((uint32_t)(w >> 32)) : __uint_as_float(M::kFillerBits);
    }
    if (tid == 0) out_sizes[q] = (int32_t)size;
}

template <typename M, typename Row, int QT, int J>
hipError_t launch_dist(const KnnPass& p, const KnnPlan& plan, uint64_t launch, int live, hipStream_t stream) {
    const dim3 grid((unsigned)((p.nq + QT - 1) / QT), (unsigned)(live * plan.slices)), block(kKnnWaves * 64);
    hipLaunchKernelGGL((refine_knn_dist_kernel<M, Row, QT, J>), grid, block, plan.dist_lds_bytes, stream, static_cast<const Row*>(p.rows), p.lo,
                       p.nrows, p.row_key, p.filter, p.dim, p.sq.vmin, p.sq.step, p.queries, p.nq, plan.chunk_rows, plan.groups, plan.slice_rows, plan.slices, launch,
                       plan.buf_cap, p.buf, p.cnt, p.bound);
    return hipGetLastError();
}

template <typename M, typename Row>
hipError_t dispatch_dist(const KnnPass& p, const KnnPlan& plan, uint64_t launch, int live, hipStream_t stream) {
#define QADC_KNN(QT, J) \
    if (plan.qt == QT && plan.jregs == J) return launch_dist<M, Row, QT, J>(p, plan, launch, live, stream)
    QADC_KNN(32, 1); QADC_KNN(32, 2); QADC_KNN(16, 3); QADC_KNN(16, 4);
    QADC_KNN(4, 1); QADC_KNN(4, 2); QADC_KNN(4, 3); QADC_KNN(4, 4);
    QADC_KNN(32, 0); QADC_KNN(16, 0); QADC_KNN(8, 0); QADC_KNN(4, 0);
#undef QADC_KNN
    return hipErrorInvalidValue;   // (a tile the plan does not make)
}

template <typename M>
hipError_t dispatch_rows(const KnnPass& p, const KnnPlan& plan, uint64_t launch, int live, hipStream_t stream) {
    if (p.elem == Elem::kSQ8) return dispatch_dist<M, sq8_t>(p, plan, launch, live, stream);
    return p.elem == Elem::kF16 ? dispatch_dist<M, __half>(p, plan, launch, live, stream) : dispatch_dist<M, float>(p, plan, launch, live, stream);
}

template <typename M>
hipError_t launch_final(const KnnPass& p, const KnnPlan& plan, int live, hipStream_t stream) {
    hipLaunchKernelGGL(refine_knn_final_kernel<M>, dim3((unsigned)p.nq), dim3(plan.select_threads), plan.select_lds_bytes, stream, p.R,
                       plan.groups, live, plan.buf_cap, p.buf, p.cnt, p.out_keys, p.out_dist, p.out_sizes);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_knn_dist(const KnnPass& p, const KnnPlan& plan, uint64_t launch, hipStream_t stream) {
    const int live = knn_launch_groups(p.nrows, plan.chunk_rows, plan.groups, launch);
    if (live == 0 || p.nq == 0) return hipSuccess;
    return p.metric == kMetricIP ? dispatch_rows<MetricIP>(p, plan, launch, live, stream) : dispatch_rows<MetricL2>(p, plan, launch, live, stream);
}

hipError_t launch_knn_select(const KnnPass& p, const KnnPlan& plan, uint64_t launch, hipStream_t stream) {
    const int live = knn_launch_groups(p.nrows, plan.chunk_rows, plan.groups, launch);
    if (live == 0 || p.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(refine_knn_select_kernel, dim3((unsigned)p.nq, (unsigned)live), dim3(plan.select_threads), plan.select_lds_bytes, stream,
                       p.R, plan.groups, plan.buf_cap, p.buf, p.cnt, p.bound);
    return hipGetLastError();
}

hipError_t launch_knn_final(const KnnPass& p, const KnnPlan& plan, hipStream_t stream) {
    if (p.nq == 0) return hipSuccess;
    const int live = knn_launch_groups(p.nrows, plan.chunk_rows, plan.groups, 0);
    return p.metric == kMetricIP ? launch_final<MetricIP>(p, plan, live, stream) : launch_final<MetricL2>(p, plan, live, stream);
}

}  // namespace refine
}  // namespace qadc
