// Empty-cluster repair of PQ training (include/qadc.h "Empty-cluster repair") — HIP-free C++14, the CPU twin
// of qadc_pq_repair_host: the definition the device result is tested against bit for bit.
//
// Per sub-space, independently: the clusters without a member are listed in ascending order; every vector gets the distance to the
// centroid it is assigned to (ONE float chain acc = fmaf(t, t, acc), t = x - c, from 0.0f over ascending columns); a vector is
// eligible iff that distance is finite and > 0 and the vector is not the lowest-index member of its cluster; the min(E, eligible)
// eligible vectors with the largest key (distance bits, then the LOWER index) are chosen and, in ascending index, take the empty
// clusters in ascending order.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <vector>

namespace qadc {

// key of include/qadc.h: 0 for a vector that is not eligible (eligible keys are >= 2^32)
inline std::uint64_t pq_repair_key(float d, std::uint32_t i, bool is_first) {
    if (!(d > 0.0f) || !(d < INFINITY) || is_first) return 0;
    std::uint32_t bits;
    std::memcpy(&bits, &d, sizeof bits);
    return ((std::uint64_t)bits << 32) | (std::uint64_t)(0xFFFFFFFFu - i);
}

// One sub-space: x points at its first column of vector 0, rows `stride` floats apart; centroids [K][ds]; assign [n] in [0, K), in
// and out.  Returns the vectors moved.
inline std::uint32_t pq_repair_slice(const float* x, size_t n, size_t stride, int ds, int K, const float* centroids, int* assign) {
    std::vector<std::uint32_t> count((size_t)K, 0u), first((size_t)K, 0xFFFFFFFFu), empties;
    for (size_t i = 0; i < n; ++i) {
        const int k = assign[i];
        if (count[k]++ == 0) first[k] = (std::uint32_t)i;
    }
    for (int k = 0; k < K; ++k)
        if (count[k] == 0) empties.push_back((std::uint32_t)k);
    if (empties.empty()) return 0;
    std::vector<std::uint64_t> keys(n), eligible;
    for (size_t i = 0; i < n; ++i) {
        const float* c = centroids + (size_t)assign[i] * ds;
        float acc = 0.0f;
        for (int d = 0; d < ds; ++d) {
            const volatile float t = x[i * stride + d] - c[d];       // (volatile: the subtraction is rounded to float on its own)
            acc = std::fmaf(t, t, acc);
        }
        keys[i] = pq_repair_key(acc, (std::uint32_t)i, first[assign[i]] == (std::uint32_t)i);
        if (keys[i]) eligible.push_back(keys[i]);
    }
    const size_t take = std::min(empties.size(), eligible.size());
    if (take == 0) return 0;
    std::nth_element(eligible.begin(), eligible.begin() + (take - 1), eligible.end(), std::greater<std::uint64_t>());
    const std::uint64_t threshold = eligible[take - 1];             // the take-th largest key; eligible keys are distinct
    size_t j = 0;
    for (size_t i = 0; i < n; ++i)
        if (keys[i] >= threshold && keys[i] != 0) assign[i] = (int)empties[j++];
    return (std::uint32_t)j;
}

inline int pq_repair_code_get(const void* codes, int sq_count, int sq_bits, size_t i, int m) {
    if (sq_bits == 4) return (static_cast<const std::uint8_t*>(codes)[i * (size_t)(sq_count / 2) + m / 2] >> (4 * (m & 1))) & 15;
    if (sq_bits == 8) return static_cast<const std::uint8_t*>(codes)[i * (size_t)sq_count + m];
    const std::uint8_t* p = static_cast<const std::uint8_t*>(codes) + (i * (size_t)sq_count + m) * 2;   // little-endian uint16
    return p[0] | (p[1] << 8);
}

inline void pq_repair_code_set(void* codes, int sq_count, int sq_bits, size_t i, int m, int k) {
    if (sq_bits == 4) {
        std::uint8_t& b = static_cast<std::uint8_t*>(codes)[i * (size_t)(sq_count / 2) + m / 2];
        b = (std::uint8_t)((b & (m & 1 ? 0x0F : 0xF0)) | (k << (4 * (m & 1))));
    } else if (sq_bits == 8) {
        static_cast<std::uint8_t*>(codes)[i * (size_t)sq_count + m] = (std::uint8_t)k;
    } else {
        std::uint8_t* p = static_cast<std::uint8_t*>(codes) + (i * (size_t)sq_count + m) * 2;
        p[0] = (std::uint8_t)(k & 255);
        p[1] = (std::uint8_t)(k >> 8);
    }
}

// x [n][dim] as the quantizer sees it, cb [sq_count][2^sq_bits][dim / sq_count], codes in the encoder's layout (sq_bits 4: packed
// nibbles [n][sq_count / 2], the even sub-quantizer in the low one; 8: bytes [n][sq_count]; 16: little-endian uint16 [n][sq_count]),
// in and out; moved [sq_count] (nullable).  Returns the vectors moved in all sub-spaces.
inline std::uint64_t pq_repair(const float* x, size_t n, int dim, int sq_count, int sq_bits, const float* cb, void* codes, std::uint32_t* moved) {
    if ((sq_bits != 4 && sq_bits != 8 && sq_bits != 16) || sq_count <= 0 || dim <= 0 || dim % sq_count || (sq_bits == 4 && sq_count % 2) ||
        n >= ((size_t)1 << 32))
        throw std::runtime_error("pq_repair: sq_bits 4, 8 or 16, dim a multiple of sq_count, n < 2^32");
    const int ds = dim / sq_count, K = 1 << sq_bits;
    std::vector<int> assign(n);
    std::uint64_t total = 0;
    for (int m = 0; m < sq_count; ++m) {
        for (size_t i = 0; i < n; ++i) assign[i] = pq_repair_code_get(codes, sq_count, sq_bits, i, m);
        const std::uint32_t mv = pq_repair_slice(x + (size_t)m * ds, n, (size_t)dim, ds, K, cb + (size_t)m * K * ds, assign.data());
        if (mv)
            for (size_t i = 0; i < n; ++i) pq_repair_code_set(codes, sq_count, sq_bits, i, m, assign[i]);
        if (moved) moved[m] = mv;
        total += mv;
    }
    return total;
}

}  // namespace qadc
