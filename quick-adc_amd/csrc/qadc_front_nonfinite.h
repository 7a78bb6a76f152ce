// NaN and infinite values in the float front of the 4-bit engine: what the reference BUILD does with them, restated
// for the three fronts (select_kth_kernel's quantize_query, the query kernel's front, lone_front_kernel).
//
// The reference is compiled with -ffast-math, so on a NaN its behaviour is that of the instructions g++ chose, not of
// the source's operators.  oracle/qadc_oracle.c states the rules and how they were read off the disassembly
// (orc_quantize_tables, orc_min_element_compiled); tests/test_oracle_float_ref.py pins them to the build.
//
//  * pre-scan (scan_4 + kv_binheap<unsigned, float>, db_query_4.cpp:230-242): a candidate is pushed iff
//    cand < top, and the top is the FLT_MAX sentinel until R - 1 values went in: NaN sums of either sign, +inf and
//    FLT_MAX itself are never pushed, and they do not help to fill the heap.  qmax = the R-th smallest of the values
//    BELOW FLT_MAX, or FLT_MAX when there are fewer than R.  The radix selects rank order-preserving u32 keys;
//    qadc_prescan_rank_value maps every value that is not below FLT_MAX to FLT_MAX before its key is taken, which
//    gives exactly that result (and keeps a negative NaN, whose raw key lies below -inf's, out of the R smallest).
//  * qmin (*std::min_element, 258): a reduction of x86 MINPS steps, min(a, b) = a < b ? a : b, that returns its
//    SECOND operand when either is NaN.  Without a NaN it is the minimum, whatever the order; the fronts reduce with
//    qadc_min_keep_nan, which yields a NaN iff there is one, and only then evaluate the build's own order
//    (qadc_min_element_compiled: 8 lanes, tree, 4 lanes, 3 scalars).
//  * QuantizerMAX (37-71, 277-284): !(v < qmax) -> 127 (so a NaN entry gets the worst score), else the LOW BYTE of
//    cvttps2dq((v - qmin) * scale): 0x80000000 for a NaN or out-of-range product.  The negative clamp (262-269) runs
//    only when qmin < 0, which a NaN qmin is not.
#pragma once
#include <cfloat>
#include <cstdint>

__device__ __forceinline__ float qadc_prescan_rank_value(float f) { return f < FLT_MAX ? f : FLT_MAX; }

// fminf, except that a NaN operand comes back (the first one's bits): NaN iff any value of the reduction is NaN
__device__ __forceinline__ float qadc_min_keep_nan(float a, float b) {
    const float r = fminf(a, b);
    return a != a ? a : (b != b ? b : r);
}

__device__ __forceinline__ float qadc_minps(float a, float b) { return a < b ? a : b; }   // x86 MINPS(a, b)

// *std::min_element(t, t + all) as the reference build reduces it (oracle: orc_min_element_compiled).  Called by EVERY
// thread of the workgroup (it holds barriers); s8 = 8 floats of LDS scratch; every thread returns the result.  Only
// run when the tables hold a NaN: eight threads fold the lanes, the rest wait.
__device__ __forceinline__ float qadc_min_element_compiled(const float* t, long all, float* s8, int tid) {
    const float m0 = t[0];
    const float* p = t + 1;
    long left = all - 1, done = 0;
    float m = m0;
    __syncthreads();                                             // (the scratch's earlier readers)
    if (all > 8) {
        const long blocks = left >> 3;
        if (tid < 8) {
            float acc = m0;
            for (long b = 0; b < blocks; ++b) acc = qadc_minps(acc, p[8 * b + tid]);
            s8[tid] = acc;
        }
        __syncthreads();
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = qadc_minps(s8[4 + j], s8[j]);
        m = qadc_minps(qadc_minps(r[3], r[1]), qadc_minps(r[2], r[0]));
        done = blocks * 8;
        left -= done;
        __syncthreads();                                         // (the scratch's next writers)
    }
    if (left > 3) {
        float u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = qadc_minps(m, p[done + j]);
        m = qadc_minps(qadc_minps(u[3], u[1]), qadc_minps(u[2], u[0]));
        done += 4;
        left -= 4;
    }
    for (long i = 0; i < left && i < 3; ++i) m = qadc_minps(m, p[done + i]);
    return m;
}

// vcvttps2dq, then the low byte (the reference build's packs do not saturate: their inputs are masked first)
__device__ __forceinline__ int8_t qadc_cvtt_low8(float q) {
    const int r = (q >= -2147483648.0f && q < 2147483648.0f) ? (int)q : (int)0x80000000u;
    return (int8_t)(uint8_t)((uint32_t)r & 0xffu);
}

// one entry of QuantizerMAX<int8_t>::quantize_tables.  quant_mode 1 = as compiled (scale = 127 / (qmax - qmin)),
// 0 = the source text (delta = (qmax - qmin) / 127)
__device__ __forceinline__ int8_t qadc_quantize_entry(float v, float qmin, float qmax, float scale, float delta, int quant_mode) {
    if (quant_mode == 0) return v >= qmax ? (int8_t)127 : qadc_cvtt_low8((v - qmin) / delta);
    return !(v < qmax) ? (int8_t)127 : qadc_cvtt_low8((v - qmin) * scale);
}
