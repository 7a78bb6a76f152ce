// CPU twin of the PQ decoder (include/qadc.h "Reconstruction") — header-only and HIP-free, driven by
// tests/cpp/pq_decode_host.cpp.  Every float the device writes is defined here:
//   1. gather     y[b] = codebooks[m][code(i, m)][b - m dsub], m = b / dsub: a copy, no arithmetic;
//   2. un-rotate  z[c] = ONE chain acc = fmaf(y[r], rotation[r][c], acc) over ascending r from 0.0f (z = y without a rotation);
//   3. coarse     x[c] = z[c] + coarse[p(i)][c] with K > 0 (x = z with K == 0);
//   4. error      err[i] = ONE chain acc = fmaf(d, d, acc), d = v[c] - x[c], over ascending c from 0.0f.
// A missing row (a partition outside [0, K) with K > 0, or a negative one) is kDecodeNanBits in every float.  Wherever arithmetic
// was done (a rotation, a coarse add, the error chain) a NaN result is written as kDecodeNanBits too: NaN payloads differ between
// processors, the copy of step 1 alone keeps a centroid's bits.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace qadc {

constexpr std::uint32_t kDecodeNanBits = 0x7FC00000u;          // every float of a missing row
constexpr std::uint64_t kReconstructMissing = ~0ull;           // = QADC_RECONSTRUCT_MISSING

// the (sq_count, sq_bits) pairs the encoders take
constexpr bool pq_decode_shape_ok(int sq_count, int sq_bits) {
    return sq_bits == 4    ? (sq_count == 16 || sq_count == 32)
           : sq_bits == 8  ? (sq_count == 4 || sq_count == 8 || sq_count == 16)
           : sq_bits == 16 ? (sq_count == 2 || sq_count == 4 || sq_count == 8)
                           : false;
}

constexpr size_t pq_decode_code_bytes(int sq_count, int sq_bits) {
    return sq_bits == 4 ? (size_t)sq_count / 2 : sq_bits == 8 ? (size_t)sq_count : (size_t)sq_count * 2;
}

// code(i, m) of a row in the encoder's layout: packed nibbles (the even sub-quantizer in the low nibble), bytes, or little-endian words
inline std::uint32_t pq_decode_code(const std::uint8_t* row, int m, int sq_bits) {
    if (sq_bits == 4) return (row[m >> 1] >> (4 * (m & 1))) & 15u;
    if (sq_bits == 8) return row[m];
    return (std::uint32_t)row[2 * m] | ((std::uint32_t)row[2 * m + 1] << 8);
}

inline float pq_decode_nan() {
    float f;
    std::memcpy(&f, &kDecodeNanBits, 4);
    return f;
}

// a row is missing: it has a partition, and that partition is negative or (with a coarse quantizer) not one of its K
inline bool pq_decode_missing(const std::int32_t* assign, size_t i, int K) { return assign && (assign[i] < 0 || (K > 0 && assign[i] >= K)); }

// codes [n][code bytes] -> out [n][dim]; err_out [n] (nullable, needs vectors [n][dim]).  rotation [dim][dim], coarse [K][dim],
// assign [n]: nullable as in qadc_pq_decode_host (assign is required with K > 0; with K == 0 only its negative entries matter).
inline void pq_decode(int sq_count, int sq_bits, int dim, const float* codebooks, const float* rotation, int K, const float* coarse,
                      const std::int32_t* assign, const void* codes, size_t n, const float* vectors, float* out, float* err_out) {
    const int dsub = dim / sq_count;
    const size_t centroids = (size_t)1 << sq_bits, cbytes = pq_decode_code_bytes(sq_count, sq_bits);
    const std::uint8_t* rows = static_cast<const std::uint8_t*>(codes);
    std::vector<float> y((size_t)dim);
    for (size_t i = 0; i < n; ++i) {
        float* x = out + i * (size_t)dim;
        if (pq_decode_missing(assign, i, K)) {
            for (int c = 0; c < dim; ++c) x[c] = pq_decode_nan();
        } else {
            for (int b = 0; b < dim; ++b) {
                const int m = b / dsub;
                y[(size_t)b] = codebooks[((size_t)m * centroids + pq_decode_code(rows + i * cbytes, m, sq_bits)) * (size_t)dsub + (size_t)(b - m * dsub)];
            }
            for (int c = 0; c < dim; ++c) {
                float z = y[(size_t)c];
                if (rotation) {
                    z = 0.0f;
                    for (int r = 0; r < dim; ++r) z = std::fmaf(y[(size_t)r], rotation[(size_t)r * dim + c], z);
                }
                if (K > 0) z = z + coarse[(size_t)assign[i] * dim + c];
                x[c] = (rotation || K > 0) && z != z ? pq_decode_nan() : z;   // a NaN that arithmetic made or passed on: the canonical one
            }
        }
        if (err_out) {
            float acc = 0.0f;
            for (int c = 0; c < dim; ++c) {
                const float d = vectors[i * (size_t)dim + c] - x[c];
                acc = std::fmaf(d, d, acc);
            }
            err_out[i] = acc != acc ? pq_decode_nan() : acc;
        }
    }
}

// The lookup of qadc_adc_index_reconstruct: where_out[i] = (partition << 32 | row) of the row with the smallest (partition, row)
// whose key is keys[i], kReconstructMissing where no row holds it.  labels[p] null: partition p is keyed key_base[p] + position.
inline void reconstruct_where(size_t parts, const std::uint32_t* sizes, const std::uint32_t* const* labels, const std::uint32_t* key_base,
                              const std::uint32_t* keys, size_t count, std::uint64_t* where_out) {
    for (size_t i = 0; i < count; ++i) {
        where_out[i] = kReconstructMissing;
        for (size_t p = 0; p < parts && where_out[i] == kReconstructMissing; ++p)
            for (std::uint32_t r = 0; r < sizes[p]; ++r)
                if ((labels && labels[p] ? labels[p][r] : key_base[p] + r) == keys[i]) {
                    where_out[i] = ((std::uint64_t)p << 32) | r;
                    break;
                }
    }
}

}  // namespace qadc
