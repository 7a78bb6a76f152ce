// Device code the refine kernels share (private to csrc/qadc_refine_kernel.hip, csrc/qadc_refine_knn_kernel.hip and
// csrc/qadc_refine_probe_kernel.hip; the range kernels keep their own restatement): the metric policies, a row's components, the lookups from a key to a
// row, the key filter, the transposed fold of a tile's partial sums and the bitonic sort of the selects.  Every unit that includes it
// is built with -ffp-contract=off; the definition all of it is held to is host/refine.hpp.
#pragma once
#include "qadc_refine.h"

#include <hip/hip_fp16.h>

namespace qadc {
namespace refine {

constexpr uint32_t kNanImage = 0x7FC00000u;
constexpr uint32_t kInfImage = 0x7F800000u;
constexpr uint64_t kNoWord = ~0ull;

// The metric of a store (qadc_refine_set_metric) as a compile-time policy of the distance, select and final
// kernels: the term a component adds to a lane's partial sum (the product and the sum it enters are rounded one by one: the units
// are built with -ffp-contract=off), the image of a folded value — the high half of a word, so that ascending words are the
// metric's order, best first — its inverse, and the bit pattern out_dist holds in the slots behind out_sizes[q].
struct MetricL2 {                                     // D: smaller first.  D is +0, positive or NaN, so its bits are its order
    static constexpr uint32_t kFillerBits = kInfImage;
    __device__ static inline float term(float q, float x) {
        const float t = q - x;
        return t * t;
    }
    __device__ static inline uint32_t image(float v) {
        uint32_t img = __float_as_uint(v);
        if (v != v) img = kNanImage;
        return img;
    }
    __device__ static inline float value(uint32_t img) { return __uint_as_float(img); }
};

struct MetricIP {                                     // S: larger first.  +inf 0x007FFFFF .. +0 0x7FFFFFFF, -0 0x80000000 .. -inf
    static constexpr uint32_t kNanImageIP = 0xFFC00000u;   // 0xFF800000, every NaN behind it; all below kNoWord's high half
    static constexpr uint32_t kFillerBits = 0xFF800000u;   // -inf
    __device__ static inline float term(float q, float x) { return q * x; }
    __device__ static inline uint32_t image(float v) {
        const uint32_t b = __float_as_uint(v);
        uint32_t img = (b & 0x80000000u) ? b : (~b & 0x7FFFFFFFu);
        if (v != v) img = kNanImageIP;
        return img;
    }
    __device__ static inline float value(uint32_t img) {
        const uint32_t b = (img & 0x80000000u) ? img : (~img & 0x7FFFFFFFu);
        return __uint_as_float(img > 0xFF800000u ? kNanImage : b);   // (a NaN comes out as 0x7FC00000)
    }
};

struct sq8_t {                                        // a component of an SQ8 row
    uint8_t b;
};

// component i of a row; vmin and step are component i's parameters of an SQ8 store (unused by the other types)
__device__ inline float row_value(const float* x, int i, float, float) { return x[i]; }
__device__ inline float row_value(const __half* x, int i, float, float) { return __half2float(x[i]); }
__device__ inline float row_value(const sq8_t* x, int i, float vmin, float step) {
    const float m = (float)x[i].b * step;
    return vmin + m;
}

// The wide-load form of an SQ8 row: lane l takes the four bytes of the components b .. b + 3 with one load (the row's end is never
// passed: a dword that would reach over it is put together from the bytes that exist), and sq_lane_byte hands component
// 64 s + lane of the 256 the wave holds to its lane: it lies in the dword of lane 16 s + lane / 4, at byte lane % 4.  Every lane
// of the wave calls both, whatever its own component.
__device__ inline uint32_t sq_load4(const sq8_t* x, int b, int dim) {
    uint32_t w = 0;
    if (b + 4 <= dim) {
        __builtin_memcpy(&w, x + b, 4);               // (no alignment is promised: dim may be odd)
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (b + k < dim) w |= (uint32_t)x[b + k].b << (8 * k);
    }
    return w;
}

__device__ inline float sq_lane_value(uint32_t w, int s, int lane, float vmin, float step) {
    const uint32_t v = (uint32_t)__builtin_amdgcn_ds_bpermute((16 * s + (lane >> 2)) << 2, (int)w);
    const float m = (float)((v >> (8 * (lane & 3))) & 0xFFu) * step;
    return vmin + m;
}

// Where a candidate's row lies.  The key is uniform over the wave, so both are uniform code with no per-lane state.
struct DenseLookup {                                  // the keys [lo, lo + nrows), row = key - lo
    uint32_t lo;
    uint64_t nrows;
    __device__ inline bool row_of(uint32_t key, uint64_t* row) const {
        *row = (uint64_t)key - lo;
        return key >= lo && *row < nrows;
    }
};

struct KeyedLookup {                                  // linear probing from the key's home slot; the table is at most half used
    const uint32_t* __restrict__ tkey;
    const uint32_t* __restrict__ trow;
    int bits;
    __device__ inline bool row_of(uint32_t key, uint64_t* row) const {
        if (key == kKeyedEmpty) return false;         // (rerank's filler key: never held)
        const uint32_t mask = (1u << bits) - 1u;
        for (uint32_t s = keyed_slot(key, bits);; s = (s + 1u) & mask) {
            const uint32_t k = tkey[s];
            if (k == key) {                           // live, or dead: a removed key is missing
                const uint32_t r = trow[s];
                *row = r;
                return r != kKeyedNoRow;
            }
            if (k == kKeyedEmpty) return false;
        }
    }
};

// ScanFilter's rule (csrc/qadc_adc_kernels.h): a key is marked where it lies in [lo, lo + last] and its bit is set; EXCLUDE drops
// the marked keys, ALLOW keeps only them.  The bitmap has one word at least and a key outside the span reads none.
__device__ inline bool knn_passes(const adc::ScanFilter& f, uint32_t key) {
    const uint32_t d = key - f.lo;
    const bool marked = d <= f.last && ((f.bitmap[d >> 5] >> (d & 31u)) & 1u);
    return marked == (f.mode == adc::kFilterAllow);
}

constexpr int knn_log2(int n) { return n <= 1 ? 0 : 1 + knn_log2(n / 2); }

// The fold of a tile's partial sums (the comment of refine_knn_dist_kernel explains it): p[q] is lane l's partial sum p[l] of the
// definition for query q of a tile of QT; the value returned is D of query lane >> (6 - log2(QT)) in the lanes whose low
// 6 - log2(QT) bits are zero.  p is consumed.
template <int QT>
__device__ inline float knn_fold(float (&p)[QT], int lane) {
    constexpr int kLog = knn_log2(QT), kShift = 6 - kLog;
    // (constant trip counts: every index of p below is a compile-time constant once unrolled, so p stays in registers)
#pragma unroll
    for (int k = 0; k < kLog; ++k) {
        const int h = QT >> (k + 1), s = 32 >> k;
        const bool up = (lane & s) != 0;
#pragma unroll
        for (int i = 0; i < QT / 2; ++i)
            if (i < h) {
                const float a = p[i], b = p[i + h];   // (values first: a conditional over the two elements would be an lvalue,
                const float send = up ? a : b;        // and p an array indexed per lane)
                const float keep = up ? b : a;
                p[i] = keep + __shfl_xor(send, s, 64);
            }
    }
    float v = p[0];
#pragma unroll
    for (int s = (1 << kShift) >> 1; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
    return v;
}

// s[0 .. n) sorted ascending, n a power of two, by the T threads of the workgroup: refine_select_kernel's bitonic network
__device__ inline void knn_sort(uint64_t* s, int n, int tid, int T) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = tid; t < n / 2; t += T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const uint64_t a = s[i], b = s[l];
                if ((a > b) == ((i & k) == 0)) {
                    s[i] = b;
                    s[l] = a;
                }
            }
        }
    __syncthreads();
}

__device__ inline int knn_sort_size(uint32_t n) {
    int p = 64;
    while ((uint32_t)p < n) p <<= 1;
    return p;
}

}  // namespace refine
}  // namespace qadc
