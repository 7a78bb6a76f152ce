// Float ADC over whole-byte PQ codes on gfx950: the GPU form of the reference's scan_standard<uint8_t, NSQ>
// (query_common.hpp:92-118) as scanner_simple::query_scan drives it (db_query.cpp:26-45).  Host side: csrc/qadc_adc.cpp.
//
//   adc_scan_kernel    one workgroup per run of codes of one probed partition: the (query, slot) float table [NSQ][256]
//                      goes to LDS, each lane sums the NSQ looked-up entries of its codes in the reference's grouping and
//                      emits (candidate, key, scan index) when candidate < bound[query];
//   adc_select_kernel  one workgroup per query: bound = the R-th smallest value the query emitted so far (radix select on
//                      the order-preserving integer image of the floats), the bound of the next level's runs;
//   adc_pack_kernel    the per-query regions packed densely for one device-to-host copy.
// The bound rule and why it is exact: DESIGN.md section 11.  Built with -ffp-contract=off and without fast-math (Makefile):
// every sum rounds like the reference's.
#include <cfloat>

#include "qadc_adc_kernels.h"
#include "qadc_float_sum.h"

namespace qadc {
namespace adc {
namespace {

template <int NSQ>
struct CodeWords;   // one code = one dword, dwordx2 or dwordx4 load
template <>
struct CodeWords<4> { uint32_t w[1]; };
template <>
struct CodeWords<8> { uint32_t w[2]; };
template <>
struct CodeWords<16> { uint32_t w[4]; };

template <int NSQ>
__device__ __forceinline__ CodeWords<NSQ> load_code(const uint8_t* p) {
    CodeWords<NSQ> c;
    if constexpr (NSQ == 4) {
        c.w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else if constexpr (NSQ == 8) {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        c.w[0] = v.x; c.w[1] = v.y;
    } else {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        c.w[0] = v.x; c.w[1] = v.y; c.w[2] = v.z; c.w[3] = v.w;
    }
    return c;
}

template <int NSQ, int SUM>
__device__ __forceinline__ float candidate(const float* lds, const CodeWords<NSQ>& c) {
    float t[NSQ];
#pragma unroll
    for (int m = 0; m < NSQ; ++m) t[m] = lds[m * 256 + ((c.w[m / 4] >> (8 * (m % 4))) & 0xffu)];
    if constexpr (SUM == 0) {                                     // source order, from 0 like the reference's loop
        float s = 0.0f;
#pragma unroll
        for (int m = 0; m < NSQ; ++m) s += t[m];
        return s;
    } else if constexpr (NSQ == 4) {
        return adc_sum4_standard_compiled(t);
    } else if constexpr (NSQ == 8) {
        return adc_sum8_standard_compiled(t);
    } else {
        return adc_sum8_compiled_first(t);
    }
}

constexpr int kUnroll = 4;   // codes per lane in flight

template <int NSQ, int SUM>
__global__ __launch_bounds__(kWG) void adc_scan_kernel(const Item* __restrict__ items, uint32_t first, Db db,
                                                       const int32_t* __restrict__ assign, int ma,
                                                       const float* __restrict__ tables, const float* __restrict__ bound,
                                                       Emit emit) {
    __shared__ float lds[NSQ * 256];
    const Item it = items[first + blockIdx.x];
    const int part = assign[(size_t)it.query * ma + it.slot];
    const float4* tab = reinterpret_cast<const float4*>(tables + ((size_t)it.query * ma + it.slot) * (NSQ * 256));
    for (int i = threadIdx.x; i < NSQ * 64; i += kWG) reinterpret_cast<float4*>(lds)[i] = tab[i];
    const float b = bound[it.query];
    const uint64_t region = emit.base[it.query];
    const uint32_t cap = emit.cap[it.query];
    const uint8_t* codes = db.codes + db.off[part];
    const uint32_t* labels = db.labels ? db.labels + db.lab_off[part] : nullptr;
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    for (uint32_t base = 0; base < it.count; base += kWG * kUnroll) {
        CodeWords<NSQ> c[kUnroll];
        bool valid[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const uint32_t r = base + u * kWG + threadIdx.x;
            valid[u] = r < it.count;
            if (valid[u]) c[u] = load_code<NSQ>(codes + (size_t)(it.start + r) * NSQ);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const float v = valid[u] ? candidate<NSQ, SUM>(lds, c[u]) : 0.0f;
            const bool keep = valid[u] && v < b;                  // NaN, +inf and FLT_MAX never pass (b <= FLT_MAX)
            const unsigned long long m = __ballot(keep);
            if (m == 0) continue;
            const int leader = __builtin_ctzll(m);
            uint32_t o = 0;
            if (lane == leader) o = atomicAdd(emit.count + it.query, (uint32_t)__popcll(m));
            o = __shfl(o, leader) + (uint32_t)__popcll(m & below);
            if (keep && o < cap) {
                const uint32_t r = base + u * kWG + threadIdx.x;
                const size_t at = region + o;
                emit.vals[at] = v;
                emit.keys[at] = labels ? labels[it.start + r] : it.start + r;
                emit.sidx[at] = it.sbase + r;
            }
        }
    }
}

// order-preserving image of a float (never NaN here): -x < -y < -0 < +0 < y < x
__device__ __forceinline__ uint32_t order_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float order_val(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(kWG) void adc_select_kernel(int R, Emit emit, float* __restrict__ bound) {
    const uint32_t q = blockIdx.x;
    const uint32_t n = min(emit.count[q], emit.cap[q]);
    if (n < (uint32_t)R) return;                                 // fewer than R: the FLT_MAX padding is the R-th smallest
    const float* v = emit.vals + emit.base[q];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_k;
    uint32_t prefix = 0, k = (uint32_t)R;                        // k = rank (1-based) still to find under the prefix
    for (int shift = 24; shift >= 0; shift -= 8) {
        const uint32_t mask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += kWG) {
            const uint32_t u = order_key(v[i]);
            if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 64) {                                  // wave 0: lane l holds bins 4l .. 4l+3; prefix sums by shuffles
            const uint32_t l = threadIdx.x;
            const uint32_t h0 = hist[4 * l], h1 = hist[4 * l + 1], h2 = hist[4 * l + 2], h3 = hist[4 * l + 3];
            uint32_t incl = h0 + h1 + h2 + h3;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d);
                if (l >= (uint32_t)d) incl += o;
            }
            const uint32_t excl = incl - (h0 + h1 + h2 + h3);
            if (excl < k && k <= incl) {                         // exactly one lane: the k-th value is in its bins
                uint32_t cum = excl, bin = 4 * l;
                if (cum + h0 < k) { cum += h0; ++bin;
                    if (cum + h1 < k) { cum += h1; ++bin;
                        if (cum + h2 < k) { cum += h2; ++bin; } } }
                s_prefix = prefix | (bin << shift);
                s_k = k - cum;
            }
        }
        __syncthreads();
        prefix = s_prefix;
        k = s_k;
    }
    if (threadIdx.x == 0) bound[q] = fminf(bound[q], order_val(prefix));
}

__global__ __launch_bounds__(kWG) void adc_pack_kernel(Emit emit, uint32_t* __restrict__ out) {
    const uint32_t q = blockIdx.x;
    __shared__ unsigned long long s_off;
    if (threadIdx.x == 0) s_off = 0;
    __syncthreads();
    unsigned long long part = 0;
    for (uint32_t j = threadIdx.x; j < q; j += kWG) part += min(emit.count[j], emit.cap[j]);
    if (part) atomicAdd(&s_off, part);
    __syncthreads();
    const size_t off = s_off;
    const uint32_t n = min(emit.count[q], emit.cap[q]);
    const size_t src = emit.base[q];
    for (uint32_t i = threadIdx.x; i < n; i += kWG) {
        uint32_t* r = out + 3 * (off + i);
        r[0] = __float_as_uint(emit.vals[src + i]);
        r[1] = emit.keys[src + i];
        r[2] = emit.sidx[src + i];
    }
}

template <int NSQ, int SUM>
hipError_t launch_scan_t(const Item* items, uint32_t first, uint32_t n_items, Db db, const int32_t* assign, int ma,
                         const float* tables, const float* bound, Emit emit, hipStream_t s) {
    hipLaunchKernelGGL((adc_scan_kernel<NSQ, SUM>), dim3(n_items), dim3(kWG), 0, s, items, first, db, assign, ma, tables, bound,
                       emit);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_adc_scan(int nsq, int sum_mode, const Item* items, uint32_t first, uint32_t n_items, Db db, const int32_t* assign,
                           int ma, const float* tables, const float* bound, Emit emit, hipStream_t s) {
    if (n_items == 0) return hipSuccess;
    const bool src = sum_mode == 0;
    switch (nsq) {
        case 4: return src ? launch_scan_t<4, 0>(items, first, n_items, db, assign, ma, tables, bound, emit, s)
                           : launch_scan_t<4, 1>(items, first, n_items, db, assign, ma, tables, bound, emit, s);
        case 8: return src ? launch_scan_t<8, 0>(items, first, n_items, db, assign, ma, tables, bound, emit, s)
                           : launch_scan_t<8, 1>(items, first, n_items, db, assign, ma, tables, bound, emit, s);
        case 16: return src ? launch_scan_t<16, 0>(items, first, n_items, db, assign, ma, tables, bound, emit, s)
                            : launch_scan_t<16, 1>(items, first, n_items, db, assign, ma, tables, bound, emit, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_adc_select(int nq, int R, Emit emit, float* bound, hipStream_t s) {
    hipLaunchKernelGGL(adc_select_kernel, dim3(nq), dim3(kWG), 0, s, R, emit, bound);
    return hipGetLastError();
}

hipError_t launch_adc_pack(int nq, Emit emit, uint32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(adc_pack_kernel, dim3(nq), dim3(kWG), 0, s, emit, out);
    return hipGetLastError();
}

}  // namespace adc
}  // namespace qadc
