// Kernels of the probed exact search over a refine store (qadc_refine_knn_probed), gfx950, built with
// -ffp-contract=off: every result is held bit for bit to refine::knn_probed of host/refine.hpp.  The geometry is
// host/refine_probe_plan.hpp.
//   refine_probe_dist_kernel<M, Row, Lookup, QT, J>  a workgroup owns an item — a partition of the index and a tile of at most QT of the
//                                                 queries that probe it — and a slice of the partition's rows; a wave takes a row of
//                                                 the partition, finds its key's row in the store, reads it once and forms its distance
//                                                 to every query of the tile; the words that pass the bound are appended
//   refine_probe_select_kernel                    one workgroup per (query, group): the buffer's first R DISTINCT words, the bound lowered
//                                                 to the R-th
//   refine_probe_final_kernel<M>                  one workgroup per query: the groups' lists merged, equal words kept once, the outputs
// The arithmetic, the fold and the sort are refine_knn_dist_kernel's (csrc/qadc_refine_dev.h), and so is the metric policy M (MetricL2,
// MetricIP): what that kernel's comment says of the components that do not exist, and of -0 under MetricIP,
// holds here word for word.
#include "qadc_refine_dev.h"

#include <type_traits>

namespace qadc {
namespace refine {

namespace {

// What a wave knows of a row of the partition before it reads the store: nothing to do (a filter dropped the key), an entry the
// store does not hold, or the store's row.
enum { kRowSkip = 0, kRowMissing = 1, kRowHeld = 2 };

template <typename Lookup>
__device__ inline int probe_fetch(const ProbePart& part, uint64_t r, const adc::ScanFilter& index_filter, const adc::ScanFilter& filter,
                                  const Lookup& look, uint32_t* key, uint64_t* srow) {
    // (the row, its key, the filters' verdicts and the store's row are the same in every lane of the wave)
    const uint32_t k = __builtin_amdgcn_readfirstlane(part.labels ? part.labels[r] : part.key_base + (uint32_t)r);
    *key = k;
    if (index_filter.bitmap && !knn_passes(index_filter, k)) return kRowSkip;
    if (filter.bitmap && !knn_passes(filter, k)) return kRowSkip;
    return look.row_of(k, srow) ? kRowHeld : kRowMissing;
}

// grid (items of the launch, slices).  The tile, the partial sums and the fold are refine_knn_dist_kernel's; what differs is where
// the operands come from: the tile's queries are gathered by the item's slots (query = slot / groups), the row's key is read from the
// partition and the row's address is a lookup in the store.  The key, the lookup and with them the address of the row after this
// one are fetched before the current row is summed, so that the gather's latency lies under the arithmetic.
template <typename M, typename Row, typename Lookup, int QT, int J>
__global__ __launch_bounds__(kKnnWaves * 64) void refine_probe_dist_kernel(const Row* __restrict__ rows, Lookup look, const ProbePart* __restrict__ parts,
                                                                           adc::ScanFilter index_filter, adc::ScanFilter filter, int dim,
                                                                           const float* __restrict__ sq_vmin, const float* __restrict__ sq_step,
                                                                           const float* __restrict__ queries, const ProbeItem* __restrict__ items,
                                                                           const uint32_t* __restrict__ slots, int groups, uint64_t launch_rows,
                                                                           int slice_rows, uint64_t launch, uint64_t buf_cap,
                                                                           uint64_t* __restrict__ buf, uint32_t* __restrict__ cnt,
                                                                           const uint64_t* __restrict__ bound, unsigned long long* __restrict__ missing) {
    extern __shared__ float s_tile[];   // LDS tile (J == 0): [QT][dim]
    constexpr int kShift = 6 - knn_log2(QT), JR = J > 0 ? J : 1;
    constexpr bool kSq = std::is_same<Row, sq8_t>::value;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const ProbeItem it = items[blockIdx.x];
    uint64_t first, last;
    probe_slice(it.rows, launch_rows, slice_rows, launch, blockIdx.y, &first, &last);
    if (first >= last) return;          // (the whole workgroup: a short partition's slices behind its end)
    const ProbePart part = parts[it.part];
    const int count = (int)it.count;

    float qr[QT][JR], vr[JR], sr[JR];
#pragma unroll
    for (int j = 0; j < JR; ++j) {
        const int i = 64 * j + lane;
        vr[j] = (kSq && J > 0 && i < dim) ? sq_vmin[i] : 0.0f;
        sr[j] = (kSq && J > 0 && i < dim) ? sq_step[i] : 0.0f;
    }
    if (J > 0) {
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            const uint32_t query = q < count ? slots[it.first + q] / (uint32_t)groups : 0u;
#pragma unroll
            for (int j = 0; j < JR; ++j) {
                const int i = 64 * j + lane;
                qr[q][j] = (q < count && i < dim) ? queries[(size_t)query * dim + i] : 0.0f;
            }
        }
    } else {
        for (int e = tid; e < QT * dim; e += kKnnWaves * 64) {
            const int q = e / dim, i = e - q * dim;
            s_tile[e] = q < count ? queries[(size_t)(slots[it.first + q] / (uint32_t)groups) * dim + i] : 0.0f;
        }
        __syncthreads();
    }

    const int myq = lane >> kShift;
    const bool emitter = (lane & ((1 << kShift) - 1)) == 0 && myq < count;
    const size_t slot = emitter ? slots[it.first + myq] : 0;
    const uint64_t my_bound = emitter ? bound[slot] : 0ull;

    uint32_t misses = 0;                // entries of this wave's rows the store does not hold: one per query of the tile
    uint64_t r = first + wave, srow = 0;
    uint32_t key = 0;
    int state = r < last ? probe_fetch(part, r, index_filter, filter, look, &key, &srow) : kRowSkip;
    while (r < last) {
        const uint64_t rn = r + kKnnWaves;
        uint64_t nsrow = 0;
        uint32_t nkey = 0;
        const int nstate = rn < last ? probe_fetch(part, rn, index_filter, filter, look, &nkey, &nsrow) : kRowSkip;
        if (state == kRowMissing) {
            misses += (uint32_t)count;
        } else if (state == kRowHeld) {
            const Row* x = rows + srow * (uint64_t)dim;
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
        r = rn;
        state = nstate;
        key = nkey;
        srow = nsrow;
    }
    if (lane == 0 && misses) atomicAdd(missing, (unsigned long long)misses);
}

// s[0 .. N) is sorted ascending, N a power of two >= 64.  A word survives where it is not ~0 and differs from the word before it;
// emit(rank, word) is called for every survivor with its rank among them, and the number of survivors is returned to every thread.
// Thread t owns the N / T consecutive words from t * (N / T) (one word where N < T; at most kProbeSeg words: sort_n <= 8 T in every
// plan).  It takes them into registers, so that the words' own LDS can hold the scan of the threads' counts.
constexpr int kProbeSeg = 8;
template <typename Emit>
__device__ inline uint32_t probe_distinct(uint64_t* s, int N, int tid, int T, Emit emit) {
    const int S = N > T ? N / T : 1, first = tid * S;
    uint64_t w[kProbeSeg];
    uint32_t keep = 0;
#pragma unroll
    for (int i = 0; i < kProbeSeg; ++i) {
        w[i] = kNoWord;
        if (i < S && first + i < N) {
            w[i] = s[first + i];
            if (w[i] != kNoWord && (first + i == 0 || w[i] != s[first + i - 1])) keep |= 1u << i;
        }
    }
    const uint32_t mine = __popc(keep);
    __syncthreads();
    uint32_t* scan = reinterpret_cast<uint32_t*>(s);   // [T] uint32 <= [64] words: T <= sort_n / 2 in every plan, and N >= 64 = T's floor
    scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < T; d <<= 1) {                  // inclusive scan over the threads' counts
        const uint32_t add = tid >= d ? scan[tid - d] : 0u;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    const uint32_t total = scan[T - 1];
    uint32_t rank = scan[tid] - mine;
#pragma unroll
    for (int i = 0; i < kProbeSeg; ++i)
        if (keep & (1u << i)) emit(rank++, w[i]);
    return total;
}

// grid (nq, groups).  A buffer with fewer than R words, or with the R words the last select left, stays as it is.  The same key can
// reach a buffer through two rows — labels may repeat within and across partitions — so equal words are dropped before the count to
// R: the bound is the R-th DISTINCT word, and a buffer whose distinct words are fewer than R keeps them all and its bound.
__global__ __launch_bounds__(1024) void refine_probe_select_kernel(int R, int groups, uint64_t buf_cap, uint64_t* __restrict__ buf,
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
    uint64_t* bound_at = bound + slot;
    const uint32_t distinct = probe_distinct(s_words, N, tid, T, [=](uint32_t rank, uint64_t w) {
        if (rank < (uint32_t)R) list[rank] = w;
        if (rank == (uint32_t)R - 1u) *bound_at = w;
    });
    if (tid == 0) cnt[slot] = min(distinct, (uint32_t)R);
}

// grid nq.  Every group's buffer holds at most R words here (the select ran behind every distance launch); a buffer the select left
// alone may hold a word twice, and two groups may hold the same word.
template <typename M>
__global__ __launch_bounds__(1024) void refine_probe_final_kernel(int R, int groups, uint64_t buf_cap, const uint64_t* __restrict__ buf,
                                                                  const uint32_t* __restrict__ cnt, uint32_t* __restrict__ out_keys,
                                                                  float* __restrict__ out_dist, int32_t* __restrict__ out_sizes) {
    extern __shared__ uint64_t s_words[];
    const int tid = threadIdx.x, T = blockDim.x, q = blockIdx.x;
    uint32_t total = 0;
    for (int g = 0; g < groups; ++g) {
        const size_t slot = (size_t)q * groups + g;
        const uint32_t n = min(cnt[slot], (uint32_t)R);
        for (uint32_t i = tid; i < n; i += T) s_words[total + i] = buf[slot * buf_cap + i];
        total += n;
    }
    const int N = knn_sort_size(total);
    for (int i = total + tid; i < N; i += T) s_words[i] = kNoWord;
    knn_sort(s_words, N, tid, T);
    uint32_t* ok = out_keys + (size_t)q * R;
    float* od = out_dist + (size_t)q * R;
    const uint32_t distinct = probe_distinct(s_words, N, tid, T, [=](uint32_t rank, uint64_t w) {
        if (rank < (uint32_t)R) {
            ok[rank] = (uint32_t)w;
            od[rank] = M::value((uint32_t)(w >> 32));
        }
    });
    const uint32_t size = min(distinct, (uint32_t)R);
    for (uint32_t i = size + tid; i < (uint32_t)R; i += T) {
        ok[i] = 0xFFFFFFFFu;
        od[i] = __uint_as_float(M::kFillerBits);
    }
    if (tid == 0) out_sizes[q] = (int32_t)size;
}

template <typename M, typename Row, typename Lookup, int QT, int J>
hipError_t launch_dist(const ProbePass& p, const ProbePlan& plan, const Lookup& look, const ProbeLaunch& l, hipStream_t stream) {
    const dim3 grid(l.items, l.slices), block(kKnnWaves * 64);
    hipLaunchKernelGGL((refine_probe_dist_kernel<M, Row, Lookup, QT, J>), grid, block, plan.dist_lds_bytes, stream, static_cast<const Row*>(p.rows), look,
                       p.parts, p.index_filter, p.filter, p.dim, p.sq.vmin, p.sq.step, p.queries, p.items, p.slots, plan.groups, plan.launch_rows,
                       l.slice_rows, l.launch, plan.buf_cap, p.buf, p.cnt, p.bound, p.missing);
    return hipGetLastError();
}

template <typename M, typename Row, typename Lookup>
hipError_t dispatch_dist(const ProbePass& p, const ProbePlan& plan, const Lookup& look, const ProbeLaunch& l, hipStream_t stream) {
#define QADC_PROBE(QT, J) \
    if (plan.qt == QT && plan.jregs == J) return launch_dist<M, Row, Lookup, QT, J>(p, plan, look, l, stream)
    QADC_PROBE(32, 1); QADC_PROBE(32, 2); QADC_PROBE(16, 3); QADC_PROBE(16, 4);
    QADC_PROBE(4, 1); QADC_PROBE(4, 2); QADC_PROBE(4, 3); QADC_PROBE(4, 4);
    QADC_PROBE(32, 0); QADC_PROBE(16, 0); QADC_PROBE(8, 0); QADC_PROBE(4, 0);
#undef QADC_PROBE
    return hipErrorInvalidValue;   // (a tile the plan does not make)
}

template <typename M, typename Lookup>
hipError_t dispatch_rows(const ProbePass& p, const ProbePlan& plan, const Lookup& look, const ProbeLaunch& l, hipStream_t stream) {
    if (p.elem == Elem::kSQ8) return dispatch_dist<M, sq8_t, Lookup>(p, plan, look, l, stream);
    return p.elem == Elem::kF16 ? dispatch_dist<M, __half, Lookup>(p, plan, look, l, stream) : dispatch_dist<M, float, Lookup>(p, plan, look, l, stream);
}

template <typename M>
hipError_t dispatch_lookup(const ProbePass& p, const ProbePlan& plan, const ProbeLaunch& l, hipStream_t stream) {
    if (p.tkey) return dispatch_rows<M>(p, plan, KeyedLookup{p.tkey, p.trow, p.tbits}, l, stream);
    return dispatch_rows<M>(p, plan, DenseLookup{p.lo, p.nrows}, l, stream);
}

template <typename M>
hipError_t launch_final(const ProbePass& p, const ProbePlan& plan, hipStream_t stream) {
    hipLaunchKernelGGL(refine_probe_final_kernel<M>, dim3((unsigned)p.nq), dim3(plan.select_threads), plan.select_lds_bytes, stream, p.R,
                       plan.groups, plan.buf_cap, p.buf, p.cnt, p.out_keys, p.out_dist, p.out_sizes);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_probe_dist(const ProbePass& p, const ProbePlan& plan, const ProbeLaunch& l, hipStream_t stream) {
    if (l.items == 0 || l.slices == 0) return hipSuccess;
    if (l.slices > 65535u) return hipErrorInvalidValue;
    return p.metric == kMetricIP ? dispatch_lookup<MetricIP>(p, plan, l, stream) : dispatch_lookup<MetricL2>(p, plan, l, stream);
}

hipError_t launch_probe_select(const ProbePass& p, const ProbePlan& plan, hipStream_t stream) {
    if (p.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(refine_probe_select_kernel, dim3((unsigned)p.nq, (unsigned)plan.groups), dim3(plan.select_threads), plan.select_lds_bytes,
                       stream, p.R, plan.groups, plan.buf_cap, p.buf, p.cnt, p.bound);
    return hipGetLastError();
}

hipError_t launch_probe_final(const ProbePass& p, const ProbePlan& plan, hipStream_t stream) {
    if (p.nq == 0) return hipSuccess;
    return p.metric == kMetricIP ? launch_final<MetricIP>(p, plan, stream) : launch_final<MetricL2>(p, plan, stream);
}

}  // namespace refine
}  // namespace qadc
