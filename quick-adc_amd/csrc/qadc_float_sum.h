// Float ADC sum of one 4-bit code in the association of the reference's scan_4<NSQ> (query_common.hpp:59-90).
//
// The source adds the 2*CS looked-up entries sequentially from 0 (72-80), but the reference is built with
// -ffast-math (CMakeLists.txt:7), which lets g++ re-associate the sum — and it does.  The float pre-scan decides
// qmax = the R-th smallest sum of the starts (db_query_4.cpp:259), and qmax scales every int8 table, so the
// grouping is part of the result.  Two groupings are provided:
//
//   sum_mode 1 (default) — AS COMPILED: the grouping g++ 11.4 emits for the stand-alone scan_4<16> / scan_4<32>
//     instances at -O3 -ffast-math (identical with -march=native and with an explicit AVX2/FMA ISA list), read off
//     that build's disassembly and pinned to the binary by the oracle's tests.  With L_b / H_b the entries looked
//     up by the low / high nibble of code byte b:
//         A = (H2+L3)+(H3+L4)   B = (H0+L1)+(H1+L2)   C = (H5+L6)+(H4+L5)   D = (H6+L7)+(H7+L0)
//         s = ((A+B)+C)+D                                      bytes 0..7  (all of NSQ = 16)
//         s = s + ((L_{b+1}+H_{b+1}) + (L_b+H_b))              b = 8, 10, 12, 14  (NSQ = 32 only)
//     (IEEE addition is commutative: only the grouping matters.)  It is also the cheaper one here: the longest
//     dependent chain is 5 adds (NSQ 16) / 9 adds (NSQ 32) instead of 16 / 32.
//   sum_mode 0 — SOURCE ORDER: ((((0 + L0) + H0) + L1) + H1) ...
//
// T is float, or a float vector (one component per query of a multi-query pass: the component-wise adds round like
// the scalar ones).  v[2k] = L_{h+k}, v[2k+1] = H_{h+k} for the eight code bytes h .. h+7 of one call.
#pragma once

template <typename T>
__device__ __forceinline__ T adc_sum8_source(T s, const T* v) {
#pragma unroll
    for (int j = 0; j < 16; ++j) s += v[j];
    return s;
}

#define QADC_L(b) v[2 * (b)]
#define QADC_H(b) v[2 * (b) + 1]

// bytes 0..7: the result does not take an incoming sum (the compiled code has no "0 +")
template <typename T>
__device__ __forceinline__ T adc_sum8_compiled_first(const T* v) {
    const T a = (QADC_H(2) + QADC_L(3)) + (QADC_H(3) + QADC_L(4));
    const T b = (QADC_H(0) + QADC_L(1)) + (QADC_H(1) + QADC_L(2));
    const T c = (QADC_H(5) + QADC_L(6)) + (QADC_H(4) + QADC_L(5));
    const T d = (QADC_H(6) + QADC_L(7)) + (QADC_H(7) + QADC_L(0));
    return ((a + b) + c) + d;
}

// bytes 8..15 (NSQ = 32)
template <typename T>
__device__ __forceinline__ T adc_sum8_compiled_next(T s, const T* v) {
#pragma unroll
    for (int b = 0; b < 8; b += 2) s = s + ((QADC_L(b + 1) + QADC_H(b + 1)) + (QADC_L(b) + QADC_H(b)));
    return s;
}

#undef QADC_L
#undef QADC_H

// scan_standard<uint8_t, NSQ> (query_common.hpp:92-118) as compiled, t[m] = the entry looked up for sub-quantizer m
// (host twin: adc_sum<N> in host/float_sum.hpp; NSQ 16 is adc_sum8_compiled_first with v[m] = t[m])
template <typename T>
__device__ __forceinline__ T adc_sum4_standard_compiled(const T* t) {
    return (t[1] + t[2]) + (t[3] + t[0]);
}

template <typename T>
__device__ __forceinline__ T adc_sum8_standard_compiled(const T* t) {
    return ((t[1] + t[2]) + (t[3] + t[4])) + ((t[5] + t[6]) + (t[7] + t[0]));
}

// all CS = M/2 bytes: v[2b] = L_b, v[2b+1] = H_b
template <int M, typename T>
__device__ __forceinline__ T adc_sum_code(const T* v, int sum_mode, T zero) {
    if (sum_mode == 0) {
        T s = zero;
#pragma unroll
        for (int h = 0; h < M / 2; h += 8) s = adc_sum8_source(s, v + 2 * h);
        return s;
    }
    T s = adc_sum8_compiled_first(v);
    if constexpr (M == 32) s = adc_sum8_compiled_next(s, v + 16);
    return s;
}

// ---- float distance sums shared by the feeders of both engines (csrc/qadc_kernels.hip, csrc/qadc_adc_kernel.hip) ----

// ||x - c||^2 over ds components as the reference's direct table form adds it: fmanorm<ds/8, ds%8> called by
// compute_dists_single_simd_cg (distances.hpp:60-76, 294-311) AS COMPILED with the reference's flags (pinned to that
// build through the oracle's orc_tables_direct; host twin: host/float_sum.hpp sqdist):
//   per AVX lane j: acc[j] = fma(d, d, acc[j]) over the ds/8 blocks, d = x - c;  reduceadd's tree acc[j] + acc[j+4],
//   then (r0 + r2) + (r1 + r3);  the scalar remainder is paired p_k = fma(d_2k, d_2k, r(d_2k+1^2)), d = c - x:
//   REM 4 -> (p0 + p1) + vec,  REM 6 -> (vec + p2) + (p0 + p1).
// sum_mode 0, or a remainder the reference has no instance of (sq_dim 3 of BASELINE configs[4]; its dispatch is
// distances.cpp:50-84): one sequential sum in ascending d.  X / C: anything indexable by int (pointer or register array).
template <typename X, typename C>
__device__ __forceinline__ float direct_sqdist(const X& x, const C& c, int ds, int sum_mode) {
    const int blocks = ds >> 3, rem = ds & 7;
    if (sum_mode == 0 || !(rem == 0 || rem == 4 || rem == 6)) {
        float s = 0.0f;
        for (int d = 0; d < ds; ++d) {
            const float t = x[d] - c[d];
            s += t * t;
        }
        return s;
    }
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int b = 0; b < blocks; ++b) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float d = x[b * 8 + j] - c[b * 8 + j];
            acc[j] = __fmaf_rn(d, d, acc[j]);
        }
    }
    const float r0 = acc[0] + acc[4], r1 = acc[1] + acc[5], r2 = acc[2] + acc[6], r3 = acc[3] + acc[7];
    const float vec = (r0 + r2) + (r1 + r3);
    if (rem == 0) return vec;
    float p[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (2 * k < rem) {
            const float d0 = c[blocks * 8 + 2 * k] - x[blocks * 8 + 2 * k];
            const float d1 = c[blocks * 8 + 2 * k + 1] - x[blocks * 8 + 2 * k + 1];
            p[k] = __fmaf_rn(d0, d0, d1 * d1);
        }
    }
    if (rem == 4) return (p[0] + p[1]) + vec;
    return (vec + p[2]) + (p[0] + p[1]);
}

// The BLAS-expansion distance compute_cross_dists_blas<DSQ> (distances.hpp:151-215) leaves in dists[v][c]:
//   ||v||^2 + ||c||^2 (153-176), then cblas_sgemm(alpha = -2, beta = 1) adds -2 v.c (178-182).
// expansion_sqnorm = fmanorm<DSQ/8, DSQ%8>(vec) / norm_4(vec) AS COMPILED with the reference's flags (sum_mode 1): the
// grouping of direct_sqdist with c = 0 — pinned to the reference's own text compiled up to the sgemm call (oracle/_ref
// qadc_reff_cross_norms, the 14 dimensions of its dispatch, 16 centroids) through the oracle's orc_sqnorm; host twin:
// host/float_sum.hpp sqnorm.  sum_mode 0, or a remainder the reference has no instance of: one sequential sum.
// The product is OpenBLAS's in the reference (not in this image: restated, unpinned): one sequential dot in ascending d,
// then base + (-2 dot) — -2 dot is exact, so this is the single rounding of a gemm kernel's C += alpha * acc.
struct zero_vec {
    __device__ __forceinline__ float operator[](int) const { return 0.0f; }
};
template <typename X>
__device__ __forceinline__ float expansion_sqnorm(const X& x, int ds, int sum_mode) {
    return direct_sqdist(x, zero_vec{}, ds, sum_mode);
}
template <typename X, typename C>
__device__ __forceinline__ float expansion_dist(const X& x, const C& c, int ds, float vn, float cn) {
    float dot = 0.0f;
    for (int d = 0; d < ds; ++d) dot += x[d] * c[d];
    return (vn + cn) + (-2.0f * dot);
}
