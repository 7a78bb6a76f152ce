// Exact re-ranking, the written definition — HIP-free, C++14, header only.  The GPU store behind
// qadc_refine_* (include/qadc.h; csrc/qadc_refine.cpp, csrc/qadc_refine_kernel.hip) is held to this twin bit for bit: keys, the
// distances' bit patterns, sizes and the count of missing keys.  tests/cpp/refine_host.cpp drives it from a file.
//
// Distance.  D(q, x) over dim floats, IEEE binary32, every operation rounded by itself (no fused multiply-add):
//   p[l] = +0 for l in 0..63;  for i = 64 j + l < dim, j ascending:  t = q[i] - x[i];  p[l] = p[l] + t * t
//   for s in 32, 16, 8, 4, 2, 1:  p[l] = p[l] + p[l + s]  for every l < s
//   D = p[0]
// — the order in which a wave of 64 lanes reads a row with coalesced loads and folds its partial sums with a fixed tree.  A row of
// an f16 store is the float value of the stored half, and the stored half is the round-to-nearest-even conversion of the input
// float: subnormal halves are kept, overflow goes to +-inf.
//
// Selection.  Of the entries keys[q][0 .. count_q) an entry is SKIPPED where values are given and values[q][i] == FLT_MAX (the
// float-ADC heap's sentinel), MISSING (dropped and counted) where its key is outside [lo, lo + rows); every other entry gives the
// word (img(D) << 32) | key, img(D) = D's bit pattern (D >= +0: ordered as an unsigned integer), 0x7FC00000 for every NaN.  The
// words are sorted ascending, equal words kept once, and the first min(R, survivors) are the output, ascending by (distance,
// key); the slots behind them hold key 0xFFFFFFFF and distance +inf.
//
// Exhaustive search (knn, at the end): the selection above over every key the store holds that passes a
// key filter — the definition of qadc_refine_knn.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

namespace qadc {
namespace refine {

constexpr int kF32 = 0, kF16 = 1;                    // QADC_REFINE_F32, QADC_REFINE_F16
constexpr int kMaxDim = 4096;
constexpr int kMaxIn = 8192;                         // QADC_REFINE_MAX_IN
constexpr uint32_t kNanImage = 0x7FC00000u;          // every NaN distance: behind +inf (0x7F800000)
constexpr uint32_t kInfImage = 0x7F800000u;
constexpr uint32_t kNoKey = 0xFFFFFFFFu;             // key of the slots behind out_sizes[q]
constexpr uint64_t kNoWord = ~0ull;                  // a skipped or missing entry

inline uint32_t float_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

inline float bits_float(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// binary32 -> binary16, round to nearest even; subnormal results kept, overflow to +-inf, NaN stays NaN (quiet)
inline uint16_t float_to_half(float f) {
    const uint32_t u = float_bits(f);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t a = u & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return (uint16_t)(sign | 0x7E00u | ((a >> 13) & 0x3FFu));   // NaN
    if (a >= 0x47800000u) return (uint16_t)(sign | 0x7C00u);                         // >= 65536 (inf too): inf
    if (a < 0x33000000u) return sign;                                                // below 2^-25: zero (2^-25 itself ties to even, zero, on the path below)
    const int e = (int)(a >> 23);                                                    // biased exponent, >= 102
    uint32_t m = (a & 0x7FFFFFu) | 0x800000u;                                        // 24-bit significand
    // the half's unit in the last place is 2^(max(e, 113) - 127 - 10): drop `shift` bits of m
    const int shift = (e >= 113 ? 13 : 13 + (113 - e));                              // 13 .. 24
    const uint32_t kept = m >> shift, rest = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    uint32_t r = kept + ((rest > half || (rest == half && (kept & 1u))) ? 1u : 0u);
    // normal: r has the hidden bit at 2^10 and the exponent field is e - 112, so adding ((e - 113) << 10) lets a carry out of
    // the significand step the exponent (up to inf at 0x7C00); subnormal: r is the field itself (a carry makes the smallest normal)
    if (e >= 113) r += (uint32_t)(e - 113) << 10;
    return (uint16_t)(sign | r);
}

inline float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const uint32_t e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    if (e == 0x1Fu) return bits_float(sign | 0x7F800000u | (m << 13));
    if (e != 0) return bits_float(sign | ((e + 112u) << 23) | (m << 13));
    if (m == 0) return bits_float(sign);
    const float v = (float)m * 5.9604644775390625e-08f;                              // m * 2^-24, exact
    return sign ? -v : v;
}

// D(q, x): x(i) gives the row's i-th component as a float
#if defined(__GNUC__) && !defined(__clang__)
#define QADC_REFINE_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define QADC_REFINE_NO_CONTRACT
#endif
template <typename RowAt>
QADC_REFINE_NO_CONTRACT inline float distance(const float* q, int dim, RowAt x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float p[64];
    for (int l = 0; l < 64; ++l) p[l] = 0.0f;
    for (int i = 0; i < dim; ++i) {
        const float t = q[i] - x(i);
        const float tt = t * t;
        p[i & 63] = p[i & 63] + tt;
    }
    for (int s = 32; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l) p[l] = p[l] + p[l + s];
    return p[0];
}

inline uint32_t image(float d) { return d != d ? kNanImage : float_bits(d); }

// The store: dense over the keys [lo, lo + rows), row r the vector of key lo + r.
struct store {
    int dim = 0, dtype = kF32;
    uint32_t lo = 0;
    uint64_t rows = 0;
    std::vector<float> f32;
    std::vector<uint16_t> f16;

    store(int dim_, int dtype_) : dim(dim_), dtype(dtype_) {}

    // false: first_key does not continue the store, or lo + rows would pass 2^32 (the store is left as it was)
    bool add(const float* vectors, uint64_t count, uint32_t first_key) {
        if (count == 0) return true;
        if (rows == 0 ? false : (uint64_t)first_key != (uint64_t)lo + rows) return false;
        if ((uint64_t)first_key + count > (1ull << 32)) return false;
        if (rows == 0) lo = first_key;
        const size_t n = (size_t)count * dim;
        if (dtype == kF16) {
            f16.reserve(f16.size() + n);
            for (size_t i = 0; i < n; ++i) f16.push_back(float_to_half(vectors[i]));
        } else {
            f32.insert(f32.end(), vectors, vectors + n);
        }
        rows += count;
        return true;
    }

    bool holds(uint32_t key) const { return key >= lo && (uint64_t)key - lo < rows; }

    // every key held, ascending (what knn ranks)
    std::vector<uint32_t> held_keys() const {
        std::vector<uint32_t> k((size_t)rows);
        for (uint64_t r = 0; r < rows; ++r) k[(size_t)r] = (uint32_t)(lo + r);
        return k;
    }

    float distance_to(const float* q, uint32_t key) const {
        const size_t base = (size_t)(key - lo) * dim;
        if (dtype == kF16) {
            const uint16_t* x = f16.data() + base;
            return distance(q, dim, [x](int i) { return half_to_float(x[i]); });
        }
        const float* x = f32.data() + base;
        return distance(q, dim, [x](int i) { return x[i]; });
    }
};

// The keyed store (qadc_refine_create_keyed): a map from key to vector in place of a dense range.  holds(key)
// = "the map has the key"; the selection above reads nothing else of a store, so a result is a function of the map's contents and
// the call's arguments alone — no slot, row or order of earlier puts can show in it.
struct keyed_store {
    int dim = 0, dtype = kF32;
    std::map<uint32_t, std::vector<float>> f32;      // one of the two is in use, by dtype
    std::map<uint32_t, std::vector<uint16_t>> f16;

    keyed_store(int dim_, int dtype_) : dim(dim_), dtype(dtype_) {}

    uint64_t live() const { return dtype == kF16 ? f16.size() : f32.size(); }

    // For i ascending the vector of key labels[i] becomes vectors[i], converted as store::add converts: a key not held becomes
    // held, the last occurrence of a key wins.  false: a label is 0xFFFFFFFF, the filler key of rerank (the map is left as it was).
    bool put(const float* vectors, const uint32_t* labels, uint64_t count) {
        for (uint64_t i = 0; i < count; ++i)
            if (labels[i] == kNoKey) return false;
        for (uint64_t i = 0; i < count; ++i) {
            const float* v = vectors + (size_t)i * dim;
            if (dtype == kF16) {
                std::vector<uint16_t>& row = f16[labels[i]];
                row.resize(dim);
                for (int j = 0; j < dim; ++j) row[j] = float_to_half(v[j]);
            } else {
                f32[labels[i]].assign(v, v + dim);
            }
        }
        return true;
    }

    // Every listed key that is held leaves; returns how many left (a key listed twice counts once, a key not held is ignored)
    uint64_t remove(const uint32_t* labels, uint64_t count) {
        uint64_t removed = 0;
        for (uint64_t i = 0; i < count; ++i) removed += dtype == kF16 ? f16.erase(labels[i]) : f32.erase(labels[i]);
        return removed;
    }

    bool holds(uint32_t key) const { return dtype == kF16 ? f16.count(key) != 0 : f32.count(key) != 0; }

    // every key held, ascending (what knn ranks)
    std::vector<uint32_t> held_keys() const {
        std::vector<uint32_t> k;
        k.reserve((size_t)live());
        if (dtype == kF16)
            for (const auto& e : f16) k.push_back(e.first);
        else
            for (const auto& e : f32) k.push_back(e.first);
        return k;
    }

    float distance_to(const float* q, uint32_t key) const {
        if (dtype == kF16) {
            const uint16_t* x = f16.find(key)->second.data();
            return distance(q, dim, [x](int i) { return half_to_float(x[i]); });
        }
        const float* x = f32.find(key)->second.data();
        return distance(q, dim, [x](int i) { return x[i]; });
    }
};

// queries [nq][dim], keys [nq][r_in], counts [nq] or null (every count in [0, r_in]), values [nq][r_in] or null ->
// out_keys [nq][R], out_dist [nq][R], out_sizes [nq]; returns the missing entries of all queries.  Store: store or keyed_store —
// the definition reads a store through dim, holds and distance_to alone.
template <typename Store>
inline uint64_t rerank(const Store& s, int nq, const float* queries, int r_in, const uint32_t* keys, const int32_t* counts,
                       const float* values, int R, uint32_t* out_keys, float* out_dist, int32_t* out_sizes) {
    uint64_t missing = 0;
    std::vector<uint64_t> words;
    for (int q = 0; q < nq; ++q) {
        const uint32_t* k = keys + (size_t)q * r_in;
        const int count = counts ? counts[q] : r_in;
        words.clear();
        for (int i = 0; i < count; ++i) {
            if (values && values[(size_t)q * r_in + i] == FLT_MAX) continue;
            if (!s.holds(k[i])) {
                ++missing;
                continue;
            }
            words.push_back(((uint64_t)image(s.distance_to(queries + (size_t)q * s.dim, k[i])) << 32) | k[i]);
        }
        std::sort(words.begin(), words.end());
        words.erase(std::unique(words.begin(), words.end()), words.end());
        const int n = (int)std::min<size_t>((size_t)R, words.size());
        for (int j = 0; j < R; ++j) {
            out_keys[(size_t)q * R + j] = j < n ? (uint32_t)words[j] : kNoKey;
            out_dist[(size_t)q * R + j] = bits_float(j < n ? (uint32_t)(words[j] >> 32) : kInfImage);
        }
        out_sizes[q] = n;
    }
    return missing;
}

// ---- exhaustive search (qadc_refine_knn) ----
// A key filter with qadc_adc_filter's semantics (csrc/qadc_adc_kernels.h, ScanFilter): kFilterExclude drops the listed keys,
// kFilterAllow keeps only the listed keys; an empty allow set keeps nothing.  `keys` is sorted ascending (duplicates are harmless).
constexpr int kFilterExclude = 0, kFilterAllow = 1;   // QADC_ADC_FILTER_EXCLUDE, QADC_ADC_FILTER_ALLOW
struct filter {
    int mode = kFilterExclude;
    std::vector<uint32_t> keys;
    bool passes(uint32_t key) const { return std::binary_search(keys.begin(), keys.end(), key) == (mode == kFilterAllow); }
};

// The R nearest rows of the whole store: rerank with keys[q] = every held key that passes `filter` (null: every held key), with no
// limit on their number (and nothing to skip, miss or dedupe: a store holds a key once).  queries [nq][dim] -> out_keys [nq][R],
// out_dist [nq][R], out_sizes [nq] = min(R, the keys that pass).
template <typename Store>
inline void knn(const Store& s, int nq, const float* queries, int R, const filter* f, uint32_t* out_keys, float* out_dist,
                int32_t* out_sizes) {
    std::vector<uint32_t> keys;
    for (uint32_t k : s.held_keys())
        if (!f || f->passes(k)) keys.push_back(k);
    const int n = (int)keys.size();
    for (int q = 0; q < nq; ++q) {   // one query at a time: every list of the rerank call is `keys`
        if (n == 0) {                // (rerank takes r_in >= 1)
            for (int j = 0; j < R; ++j) {
                out_keys[(size_t)q * R + j] = kNoKey;
                out_dist[(size_t)q * R + j] = bits_float(kInfImage);
            }
            out_sizes[q] = 0;
            continue;
        }
        rerank(s, 1, queries + (size_t)q * s.dim, n, keys.data(), nullptr, nullptr, R, out_keys + (size_t)q * R, out_dist + (size_t)q * R,
               out_sizes + q);
    }
}

}  // namespace refine
}  // namespace qadc
