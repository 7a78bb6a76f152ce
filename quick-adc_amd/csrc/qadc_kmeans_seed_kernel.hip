// k-means++ seeding in every sub-space at once (include/qadc.h "k-means++ seeding").
//
// A round is two launches.  seed_update_kernel reads every row of the learning set once, for all sub-spaces together: a workgroup
// owns one level-2 node of the sum tree (4096 rows), a wave walks level-1 nodes of it (64 rows).  The rows' components are loaded with
// the lanes along the components (two rows of kSeedCols columns per load) into the wave's LDS window and read back with lane <-> row,
// so that a lane owns the whole distance chain of its row — the contract's one float chain over ascending components — and the
// 64-lane xor-butterfly over the weights is the contract's balanced sum of a level-1 node.  The columns of a row pass a lane in
// ascending order, so one chain is live at a time: it is closed, mind updated and the node's sum written where a sub-space ends.
// seed_pick_kernel, one workgroup per sub-space, sums the levels above 2 the same way and descends with wave 0; without a tree it is
// round 0's pick.  Nothing here depends on the grid: the tree is indexed by the row alone.  Geometry: host/kmeans_seed_plan.hpp.
// Built with -ffp-contract=off; the fused operation is explicit.
#include "qadc_kmeans_seed.h"

namespace qadc {
namespace {

// the balanced binary sum over the wave's 64 values, in every lane (double addition commutes: both partners get the same bits)
__device__ __forceinline__ double seed_wave_sum(double v) {
#pragma unroll
    for (int o = 1; o < kSeedRadix; o <<= 1) v = v + __shfl_xor(v, o);
    return v;
}

// lane j's value in every lane; j is uniform
__device__ __forceinline__ double seed_lane_get(double v, int j) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double seed_uniform(unsigned long long seed, uint32_t m, uint32_t t) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * ((((unsigned long long)m << 32) | (unsigned long long)t) + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ double seed_weight(float mind) { return mind < __builtin_inff() ? (double)mind : 0.0; }

}  // namespace

__global__ __launch_bounds__(kSeedWG) void seed_update_kernel(KmeansSeedState st, int dim, int dsub, int sq_count, uint64_t n1, uint64_t n2,
                                                              uint64_t t, int first) {
    extern __shared__ __attribute__((aligned(16))) float seed_lds[];
    const int tid = threadIdx.x, wave = tid / kSeedRadix, lane = tid % kSeedRadix;
    float* win = seed_lds + (size_t)wave * kSeedRadix * kSeedColStride;             // [64 rows][kSeedColStride]
    float* cs = seed_lds + (size_t)kSeedWaves * kSeedRadix * kSeedColStride;        // [dim]: round t - 1's centres, sub-space by sub-space
    const uint64_t n = st.n;
    for (int c = tid; c < dim; c += kSeedWG) {
        const int m = c / dsub;
        cs[c] = st.centres[((uint64_t)m * st.k + (t - 1)) * (uint64_t)dsub + (uint64_t)(c - m * dsub)];
    }
    const int lcol = kmeans_seed_load_col(lane);
    for (int node = 0; node < kSeedNodesPerWave; ++node) {                           // the same trips in every wave: the barriers are uniform
        const uint64_t node1 = (uint64_t)blockIdx.x * kSeedRadix + (uint64_t)(node * kSeedWaves + wave);
        const uint64_t row = kmeans_seed_row(blockIdx.x, wave, node, lane);
        const bool live = node1 < n1;                                                // wave-uniform: the node has a row
        float acc = 0.0f;
        int m = 0, left = dsub;
        for (int c0 = 0; c0 < dim; c0 += kSeedCols) {
            __syncthreads();                                                         // the previous window is read (first trip: cs is staged)
            if (live) {
                // a column past the row or a row past the set: an existing element is loaded and never used
                const uint64_t col = (uint64_t)min(c0 + lcol, dim - 1);
                float v[kSeedLoadSteps];
#pragma unroll
                for (int s = 0; s < kSeedLoadSteps; ++s) {
                    const uint64_t r = min(node1 * kSeedRadix + (uint64_t)kmeans_seed_load_row(s, lane), n - 1);
                    v[s] = __builtin_nontemporal_load(st.x + r * (uint64_t)dim + col);
                }
#pragma unroll
                for (int s = 0; s < kSeedLoadSteps; ++s) win[kmeans_seed_load_row(s, lane) * kSeedColStride + lcol] = v[s];
            }
            __syncthreads();
            const int cols = min(kSeedCols, dim - c0);
            for (int cc = 0; cc < cols; ++cc) {                                      // ascending component: the pinned order
                const float diff = win[lane * kSeedColStride + cc] - cs[c0 + cc];
                acc = __fmaf_rn(diff, diff, acc);
                if (--left == 0) {                                                   // the sub-space ends here (uniform)
                    double w = 0.0;
                    if (live && row < n) {
                        float* p = st.mind + (uint64_t)m * n + row;
                        const float old = first ? __builtin_inff() : *p;
                        const float now = acc < old ? acc : old;                     // a NaN never replaces
                        *p = now;
                        w = seed_weight(now);
                    }
                    const double sum = seed_wave_sum(w);
                    if (live && lane == 0) st.level1[(uint64_t)m * n1 + node1] = sum;
                    ++m;
                    left = dsub;
                    acc = 0.0f;
                }
            }
        }
    }
    __syncthreads();                                                                 // the workgroup's level-1 sums are written
    for (int m = wave; m < sq_count; m += kSeedWaves) {
        const uint64_t child = (uint64_t)blockIdx.x * kSeedRadix + (uint64_t)lane;
        const double sum = seed_wave_sum(child < n1 ? st.level1[(uint64_t)m * n1 + child] : 0.0);
        if (lane == 0) st.level2[(uint64_t)m * n2 + blockIdx.x] = sum;               // blockIdx.x < n2: the grid is n2
    }
}

__global__ __launch_bounds__(kSeedWG) void seed_pick_kernel(KmeansSeedState st, KmeansSeedPlan p, uint64_t t) {
    __shared__ uint32_t s_row;
    const int tid = threadIdx.x, wave = tid / kSeedRadix, lane = tid % kSeedRadix;
    const uint32_t m = blockIdx.x;
    const uint64_t n = st.n;
    double* const l1 = st.level1 + (uint64_t)m * p.nodes[1];
    double* const l2 = st.level2 + (uint64_t)m * p.nodes[2];
    double* const up = st.upper + (uint64_t)m * p.upper_nodes;
#define SEED_LEVEL(L) ((L) == 1 ? l1 : (L) == 2 ? l2 : up + p.upper_offset[L])
    if (t > 0) {
        for (int L = 3; L <= p.root_level; ++L) {                                    // the levels above 2, each from the one below
            const double* src = SEED_LEVEL(L - 1);
            double* dst = SEED_LEVEL(L);
            const uint64_t have = p.nodes[L - 1], count = p.nodes[L];
            for (uint64_t j = (uint64_t)wave; j < count; j += kSeedWaves) {
                const uint64_t child = j * kSeedRadix + (uint64_t)lane;
                const double sum = seed_wave_sum(child < have ? src[child] : 0.0);
                if (lane == 0) dst[j] = sum;
            }
            __syncthreads();
        }
    }
    if (wave == 0) {                                                                 // uniform within the wave from here on
        const double u = seed_uniform(st.seed, m, (uint32_t)t);
        uint64_t row = 0;
        bool fallback = false;
        if (t == 0) {
            row = (uint64_t)(u * (double)n);
        } else {
            const double root = SEED_LEVEL(p.root_level)[0];
            if (root == 0.0) {                                                       // no weight left: the smallest unpicked row
                fallback = true;
                uint32_t cur = 0;
                if (lane == 0) {
                    const uint32_t* bits = st.picked + (uint64_t)m * p.bitmap_words;
                    cur = st.cursor[m];
                    while ((uint64_t)cur + 1 < n && ((bits[cur >> 5] >> (cur & 31)) & 1u)) ++cur;   // k <= n: it stops on a clear bit
                    st.cursor[m] = cur;
                }
                row = (uint64_t)__shfl(cur, 0);
            } else {
                double target = u * root;
                uint64_t node = 0;
                for (int L = p.root_level; L >= 1; --L) {
                    const uint64_t idx = node * kSeedRadix + (uint64_t)lane;
                    double child = 0.0;
                    if (L == 1) {
                        if (idx < n) child = seed_weight(st.mind[(uint64_t)m * n + idx]);
                    } else if (idx < p.nodes[L - 1]) {
                        child = SEED_LEVEL(L - 1)[idx];
                    }
                    double c = 0.0, sel_c = 0.0, last_c = 0.0;
                    int sel = -1, last = -1;
#pragma unroll
                    for (int j = 0; j < kSeedRadix; ++j) {                           // ascending children under a sequential prefix
                        const double v = seed_lane_get(child, j);
                        if (sel < 0) {
                            if (v > 0.0) { last = j; last_c = c; }
                            if (target < c + v) { sel = j; sel_c = c; }
                            else c = c + v;
                        }
                    }
                    if (sel < 0) { sel = last; sel_c = last_c; }                     // rounding: the last positive child, its own prefix
                    if (sel < 0) sel = 0;                                            // (an entered node has a positive child)
                    target = target - sel_c;
                    node = node * kSeedRadix + (uint64_t)sel;
                }
                row = node;
            }
        }
        if (row > n - 1) row = n - 1;
        if (lane == 0) {
            st.picked[(uint64_t)m * p.bitmap_words + (row >> 5)] |= 1u << (row & 31);
            st.rows[(uint64_t)m * st.k + t] = (uint32_t)row;
            if (fallback) st.fallbacks[m] += 1ull;
            s_row = (uint32_t)row;
        }
    }
#undef SEED_LEVEL
    __syncthreads();
    const uint32_t* src = reinterpret_cast<const uint32_t*>(st.x) + (uint64_t)s_row * (uint64_t)p.dim + (uint64_t)m * (uint64_t)p.dsub;
    uint32_t* dst = reinterpret_cast<uint32_t*>(st.centres) + ((uint64_t)m * st.k + t) * (uint64_t)p.dsub;
    for (int d = tid; d < p.dsub; d += kSeedWG) dst[d] = src[d];                     // the picked sub-vector, bit for bit
}

hipError_t launch_kmeans_seed_update(const KmeansSeedState& st, const KmeansSeedPlan& plan, uint64_t t, hipStream_t stream) {
    if (t < 1 || t >= st.k) return hipErrorInvalidValue;
    hipLaunchKernelGGL(seed_update_kernel, dim3(plan.update_grid), dim3(kSeedWG), plan.lds_bytes, stream, st, plan.dim, plan.dsub,
                       plan.sq_count, plan.nodes[1], plan.nodes[2], t, t == 1 ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_kmeans_seed_pick(const KmeansSeedState& st, const KmeansSeedPlan& plan, uint64_t t, hipStream_t stream) {
    if (t >= st.k) return hipErrorInvalidValue;
    hipLaunchKernelGGL(seed_pick_kernel, dim3(plan.pick_grid), dim3(kSeedWG), 0, stream, st, plan, t);
    return hipGetLastError();
}

}  // namespace qadc
