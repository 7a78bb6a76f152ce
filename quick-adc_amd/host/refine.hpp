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
//
// Probed exact search (knn_probed, behind knn): the selection above over the rows of the partitions of an index
// that a query probes, keyed as the scan keys them — the definition of qadc_refine_knn_probed.
//
// Exact range search (range and rerank_range, at the end): every held key whose distance is below a radius,
// over the whole store or over candidate lists of any length — the definition of qadc_refine_range and qadc_refine_rerank_range.
//
// Inner product (kIP): rerank, knn and knn_probed take a metric, kL2 (the default: everything above) or kIP.
// Score.  S(q, x) over dim floats, IEEE binary32, every operation rounded by itself:
//   p[l] = +0 for l in 0..63;  for i = 64 j + l < dim, j ascending:  m = q[i] * x[i];  p[l] = p[l] + m
//   for s in 32, 16, 8, 4, 2, 1:  p[l] = p[l] + p[l + s]  for every l < s
//   S = p[0]
// — D's strips and D's tree over the products; a row's component is what D reads.  A component that does not exist contributes
// nothing.  A p starts at +0 and IEEE addition gives -0 only from two -0 operands, so no p and no S is ever -0.
// Order.  Larger S first, ties by ascending key: the word is (img_ip(S) << 32) | key, sorted ascending like D's words; img_ip(S) is
// 0xFFC00000 for every NaN, else with b = S's bit pattern b where the sign bit is set and ~b & 0x7FFFFFFF where it is clear:
// +inf 0x007FFFFF, +0 0x7FFFFFFF, -0 0x80000000, -inf 0xFF800000, NaN behind -inf, and every word below kNoWord.  The output holds S
// itself, the inverse of the image (a NaN as 0x7FC00000), descending; the slots behind out_sizes[q] hold key 0xFFFFFFFF and -inf.
// Skips, missing keys, duplicates, filters, the probed entry rule and the limits are the L2 rules word for word.  Range search has
// no inner-product form.
//
// SQ8 rows (kSQ8): one byte per component under a per-dimension affine range, vmin[dim] and step[dim], both
// finite, step >= 0; inv[i] = 1.0f / step[i] where step[i] > 0 (+inf for a subnormal step), else 0, derived once.  sq_encode,
// sq_decode and sq_range below are the definition; a row's i-th component in D(q, x) is sq_decode of its byte, and `clamped` counts
// the written components that fell outside the range.  get() reads rows back as floats, decoded by the store's type.
#pragma once
#include <algorithm>
#include <cfenv>
#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <cmath>
#include <cstring>
#include <map>
#include <stdexcept>
#include <vector>

namespace qadc {
namespace refine {

constexpr int kF32 = 0, kF16 = 1, kSQ8 = 2;          // QADC_REFINE_F32, QADC_REFINE_F16, QADC_REFINE_SQ8
constexpr int kMaxDim = 4096;
constexpr int kMaxIn = 8192;                         // QADC_REFINE_MAX_IN
constexpr uint32_t kNanImage = 0x7FC00000u;          // every NaN distance: behind +inf (0x7F800000)
constexpr uint32_t kInfImage = 0x7F800000u;
constexpr uint32_t kNoKey = 0xFFFFFFFFu;             // key of the slots behind out_sizes[q]
constexpr uint64_t kNoWord = ~0ull;                  // a skipped or missing entry
constexpr int kL2 = 0, kIP = 1;                      // QADC_REFINE_L2, QADC_REFINE_IP
constexpr uint32_t kNanImageIP = 0xFFC00000u;        // every NaN score: behind -inf (0xFF800000)
constexpr uint32_t kNegInfBits = 0xFF800000u;        // the score of the slots behind out_sizes[q] under kIP

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

// S(q, x): x(i) gives the row's i-th component as a float
template <typename RowAt>
QADC_REFINE_NO_CONTRACT inline float score(const float* q, int dim, RowAt x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float p[64];
    for (int l = 0; l < 64; ++l) p[l] = 0.0f;
    for (int i = 0; i < dim; ++i) {
        const float m = q[i] * x(i);
        p[i & 63] = p[i & 63] + m;
    }
    for (int s = 32; s >= 1; s >>= 1)
        for (int l = 0; l < s; ++l) p[l] = p[l] + p[l + s];
    return p[0];
}

// the image of a score: ascending images are descending scores, NaN last
inline uint32_t img_ip(float s) {
    if (s != s) return kNanImageIP;
    const uint32_t b = float_bits(s);
    return (b & 0x80000000u) ? b : (~b & 0x7FFFFFFFu);
}

// the score of an image (the flip is its own inverse); every image behind -inf's is a NaN's and gives 0x7FC00000
inline float img_ip_inverse(uint32_t img) {
    if (img > kNegInfBits) return bits_float(kNanImage);
    return bits_float((img & 0x80000000u) ? img : (~img & 0x7FFFFFFFu));
}

// the high half of a word under a metric, its inverse, and the bits of out_dist behind out_sizes[q]
inline uint32_t image_of(float v, int metric) { return metric == kIP ? img_ip(v) : image(v); }
inline float value_of(uint32_t img, int metric) { return metric == kIP ? img_ip_inverse(img) : bits_float(img); }
inline uint32_t filler_bits(int metric) { return metric == kIP ? kNegInfBits : kInfImage; }

// ---- SQ8 rows: IEEE binary32, every operation rounded by itself ----

inline bool sq_finite(float f) { return (float_bits(f) & 0x7F800000u) != 0x7F800000u; }

// The definition is IEEE arithmetic with subnormals.  A thread may run with subnormals flushed to zero (a library built with
// -ffast-math sets that mode for every thread that loads it); the host-side derivations below — inv, the range's step — run inside
// an ieee_scope, which puts the thread into the default floating-point environment and gives its own back at the end.  The
// arithmetic sits in functions that are not inlined, so that none of it moves across the switch.
struct ieee_scope {
    std::fenv_t saved;
    ieee_scope() {
        std::fegetenv(&saved);
        std::fesetenv(FE_DFL_ENV);
    }
    ~ieee_scope() { std::fesetenv(&saved); }
    ieee_scope(const ieee_scope&) = delete;
    ieee_scope& operator=(const ieee_scope&) = delete;
};
#if defined(__GNUC__) || defined(__clang__)
#define QADC_REFINE_NOINLINE __attribute__((noinline))
#else
#define QADC_REFINE_NOINLINE
#endif

// what a store of this type takes: vmin and step finite, step >= 0 (by their bits: -0 is a zero, a negative subnormal is negative)
inline bool sq_params_ok(const float* vmin, const float* step, int dim) {
    if (!vmin || !step || dim < 1 || dim > kMaxDim) return false;
    for (int i = 0; i < dim; ++i) {
        const uint32_t s = float_bits(step[i]);
        if (!sq_finite(vmin[i]) || !sq_finite(step[i]) || ((s & 0x80000000u) && (s & 0x7FFFFFFFu))) return false;
    }
    return true;
}

inline float sq_inv(float step) { return step > 0.0f ? 1.0f / step : 0.0f; }

// inv[i] = sq_inv(step[i]) under the default floating-point environment
QADC_REFINE_NOINLINE inline void sq_inv_rows(const float* step, int dim, float* inv) {
    for (int i = 0; i < dim; ++i) inv[i] = sq_inv(step[i]);
}
inline void sq_derive_inv(const float* step, int dim, float* inv) {
    ieee_scope ieee;
    sq_inv_rows(step, dim, inv);
}

// The byte of component x under (vmin, step, inv = sq_inv(step)): d = x - vmin, u = d * inv; 0 where !(u > 0) (NaN, below the
// range, a constant dimension), 255 where u >= 255, else u rounded to the nearest integer, ties to even.  *clamped (may be null): the
// component fell outside the range — step > 0: !(d >= 0) or !(u <= 255); step == 0: x differs in value from vmin (a NaN does).
inline uint8_t sq_encode(float x, float vmin, float step, float inv, bool* clamped) {
    const float d = x - vmin;
    const float u = d * inv;
    if (clamped) *clamped = step > 0.0f ? (!(d >= 0.0f) || !(u <= 255.0f)) : !(x == vmin);
    if (!(u > 0.0f)) return 0;
    if (u >= 255.0f) return 255;
    return (uint8_t)std::nearbyintf(u);              // (the default rounding mode: to nearest, ties to even)
}

// vmin + (float)c * step: the product rounded, then the sum
QADC_REFINE_NO_CONTRACT inline float sq_decode(uint8_t c, float vmin, float step) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float m = (float)c * step;
    return vmin + m;
}

// the sign-magnitude order of binary32 as an unsigned integer: -0 below +0
inline uint32_t sq_ordered(float f) {
    const uint32_t u = float_bits(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

inline float sq_unordered(uint32_t o) { return bits_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

// vmin and step of the dimensions whose finite components span [lo[i], hi[i]] as ordered images (lo > hi: none, which gives
// vmin = 0, step = 0)
QADC_REFINE_NOINLINE inline void sq_range_rows(const uint32_t* lo, const uint32_t* hi, int dim, float* vmin, float* step) {
    for (int i = 0; i < dim; ++i) {
        const float a = lo[i] > hi[i] ? 0.0f : sq_unordered(lo[i]), b = lo[i] > hi[i] ? 0.0f : sq_unordered(hi[i]);
        vmin[i] = a;
        step[i] = (b - a) / 255.0f;
    }
}
inline void sq_range_finish(const uint32_t* lo, const uint32_t* hi, int dim, float* vmin, float* step) {
    ieee_scope ieee;
    sq_range_rows(lo, hi, dim, vmin, step);
}

// The range of a learning set [n][dim]: per dimension the minimum and maximum over its finite components in the order of
// sq_ordered; vmin = the minimum, step = (max - min) / 255.0f.  A function of the set alone; step may be +inf where max - min
// overflows, which no store takes.
inline void sq_range(const float* vectors, uint64_t n, int dim, float* vmin, float* step) {
    std::vector<uint32_t> lo((size_t)dim, 0xFFFFFFFFu), hi((size_t)dim, 0u);
    for (uint64_t r = 0; r < n; ++r)
        for (int i = 0; i < dim; ++i) {
            const float x = vectors[(size_t)r * dim + i];
            if (!sq_finite(x)) continue;
            const uint32_t o = sq_ordered(x);
            lo[i] = std::min(lo[i], o);
            hi[i] = std::max(hi[i], o);
        }
    sq_range_finish(lo.data(), hi.data(), dim, vmin, step);
}

// The parameters of an SQ8 store and its clamp counter
struct sq_params {
    std::vector<float> vmin, step, inv;
    uint64_t clamped = 0;
    void set(int dim, const float* vmin_, const float* step_) {
        if (!sq_params_ok(vmin_, step_, dim)) throw std::invalid_argument("SQ8: vmin and step are finite, step >= 0");
        vmin.assign(vmin_, vmin_ + dim);
        step.assign(step_, step_ + dim);
        inv.resize(dim);
        sq_derive_inv(step.data(), dim, inv.data());
    }
    // dst[0 .. dim) = the bytes of v[0 .. dim); counts the clamped components
    void encode_row(const float* v, uint8_t* dst) {
        ieee_scope ieee;
        encode_components(v, dst);
    }
    QADC_REFINE_NOINLINE void encode_components(const float* v, uint8_t* dst) {
        for (size_t i = 0; i < vmin.size(); ++i) {
            bool c;
            dst[i] = sq_encode(v[i], vmin[i], step[i], inv[i], &c);
            clamped += c ? 1 : 0;
        }
    }
};

// The store: dense over the keys [lo, lo + rows), row r the vector of key lo + r.
struct store {
    int dim = 0, dtype = kF32;
    uint32_t lo = 0;
    uint64_t rows = 0;
    std::vector<float> f32;
    std::vector<uint16_t> f16;
    std::vector<uint8_t> sq8;
    sq_params sq;                                    // kSQ8 only

    store(int dim_, int dtype_) : dim(dim_), dtype(dtype_) {
        if (dtype_ == kSQ8) throw std::invalid_argument("an SQ8 store needs vmin and step");
    }
    store(int dim_, const float* vmin, const float* step) : dim(dim_), dtype(kSQ8) { sq.set(dim_, vmin, step); }

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
        } else if (dtype == kSQ8) {
            const size_t at = sq8.size();
            sq8.resize(at + n);
            for (uint64_t r = 0; r < count; ++r) sq.encode_row(vectors + (size_t)r * dim, sq8.data() + at + (size_t)r * dim);
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

    // component i of the row of a held key, as the distance reads it
    float value_at(uint32_t key, int i) const {
        const size_t at = (size_t)(key - lo) * dim + i;
        if (dtype == kF16) return half_to_float(f16[at]);
        if (dtype == kSQ8) return sq_decode(sq8[at], sq.vmin[i], sq.step[i]);
        return f32[at];
    }

    float distance_to(const float* q, uint32_t key) const {
        const size_t base = (size_t)(key - lo) * dim;
        if (dtype == kF16) {
            const uint16_t* x = f16.data() + base;
            return distance(q, dim, [x](int i) { return half_to_float(x[i]); });
        }
        if (dtype == kSQ8) {
            const uint8_t* x = sq8.data() + base;
            const float *vmin = sq.vmin.data(), *step = sq.step.data();
            return distance(q, dim, [x, vmin, step](int i) { return sq_decode(x[i], vmin[i], step[i]); });
        }
        const float* x = f32.data() + base;
        return distance(q, dim, [x](int i) { return x[i]; });
    }

    float score_to(const float* q, uint32_t key) const {
        const size_t base = (size_t)(key - lo) * dim;
        if (dtype == kF16) {
            const uint16_t* x = f16.data() + base;
            return score(q, dim, [x](int i) { return half_to_float(x[i]); });
        }
        if (dtype == kSQ8) {
            const uint8_t* x = sq8.data() + base;
            const float *vmin = sq.vmin.data(), *step = sq.step.data();
            return score(q, dim, [x, vmin, step](int i) { return sq_decode(x[i], vmin[i], step[i]); });
        }
        const float* x = f32.data() + base;
        return score(q, dim, [x](int i) { return x[i]; });
    }
};

// The keyed store (qadc_refine_create_keyed): a map from key to vector in place of a dense range.  holds(key)
// = "the map has the key"; the selection above reads nothing else of a store, so a result is a function of the map's contents and
// the call's arguments alone — no slot, row or order of earlier puts can show in it.
struct keyed_store {
    int dim = 0, dtype = kF32;
    std::map<uint32_t, std::vector<float>> f32;      // one of the three is in use, by dtype
    std::map<uint32_t, std::vector<uint16_t>> f16;
    std::map<uint32_t, std::vector<uint8_t>> sq8;
    sq_params sq;                                    // kSQ8 only

    keyed_store(int dim_, int dtype_) : dim(dim_), dtype(dtype_) {
        if (dtype_ == kSQ8) throw std::invalid_argument("an SQ8 store needs vmin and step");
    }
    keyed_store(int dim_, const float* vmin, const float* step) : dim(dim_), dtype(kSQ8) { sq.set(dim_, vmin, step); }

    uint64_t live() const { return dtype == kF16 ? f16.size() : dtype == kSQ8 ? sq8.size() : f32.size(); }

    // For i ascending the vector of key labels[i] becomes vectors[i], converted as store::add converts: a key not held becomes
    // held, the last occurrence of a key wins.  false: a label is 0xFFFFFFFF, the filler key of rerank (the map is left as it was).
    // An SQ8 store writes the last occurrence of a key only, so that only what reaches a row counts as clamped.
    bool put(const float* vectors, const uint32_t* labels, uint64_t count) {
        for (uint64_t i = 0; i < count; ++i)
            if (labels[i] == kNoKey) return false;
        std::map<uint32_t, uint64_t> last;
        if (dtype == kSQ8)
            for (uint64_t i = 0; i < count; ++i) last[labels[i]] = i;
        for (uint64_t i = 0; i < count; ++i) {
            const float* v = vectors + (size_t)i * dim;
            if (dtype == kSQ8) {
                if (last[labels[i]] != i) continue;
                std::vector<uint8_t>& row = sq8[labels[i]];
                row.resize(dim);
                sq.encode_row(v, row.data());
            } else if (dtype == kF16) {
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
        for (uint64_t i = 0; i < count; ++i)
            removed += dtype == kF16 ? f16.erase(labels[i]) : dtype == kSQ8 ? sq8.erase(labels[i]) : f32.erase(labels[i]);
        return removed;
    }

    bool holds(uint32_t key) const {
        return dtype == kF16 ? f16.count(key) != 0 : dtype == kSQ8 ? sq8.count(key) != 0 : f32.count(key) != 0;
    }

    // every key held, ascending (what knn ranks)
    std::vector<uint32_t> held_keys() const {
        std::vector<uint32_t> k;
        k.reserve((size_t)live());
        if (dtype == kF16)
            for (const auto& e : f16) k.push_back(e.first);
        else if (dtype == kSQ8)
            for (const auto& e : sq8) k.push_back(e.first);
        else
            for (const auto& e : f32) k.push_back(e.first);
        return k;
    }

    // component i of the row of a held key, as the distance reads it
    float value_at(uint32_t key, int i) const {
        if (dtype == kF16) return half_to_float(f16.find(key)->second[i]);
        if (dtype == kSQ8) return sq_decode(sq8.find(key)->second[i], sq.vmin[i], sq.step[i]);
        return f32.find(key)->second[i];
    }

    float distance_to(const float* q, uint32_t key) const {
        if (dtype == kF16) {
            const uint16_t* x = f16.find(key)->second.data();
            return distance(q, dim, [x](int i) { return half_to_float(x[i]); });
        }
        if (dtype == kSQ8) {
            const uint8_t* x = sq8.find(key)->second.data();
            const float *vmin = sq.vmin.data(), *step = sq.step.data();
            return distance(q, dim, [x, vmin, step](int i) { return sq_decode(x[i], vmin[i], step[i]); });
        }
        const float* x = f32.find(key)->second.data();
        return distance(q, dim, [x](int i) { return x[i]; });
    }

    float score_to(const float* q, uint32_t key) const {
        if (dtype == kF16) {
            const uint16_t* x = f16.find(key)->second.data();
            return score(q, dim, [x](int i) { return half_to_float(x[i]); });
        }
        if (dtype == kSQ8) {
            const uint8_t* x = sq8.find(key)->second.data();
            const float *vmin = sq.vmin.data(), *step = sq.step.data();
            return score(q, dim, [x, vmin, step](int i) { return sq_decode(x[i], vmin[i], step[i]); });
        }
        const float* x = f32.find(key)->second.data();
        return score(q, dim, [x](int i) { return x[i]; });
    }
};

// Read-back (qadc_refine_get): out [count][dim] = the rows of the listed keys as floats, decoded by the store's type; a key the
// store does not hold gives a row of 0x7FC00000 and found 0.  found may be null.
template <typename Store>
inline void get(const Store& s, const uint32_t* keys, uint64_t count, float* out, uint8_t* found) {
    for (uint64_t k = 0; k < count; ++k) {
        const bool held = s.holds(keys[k]);
        for (int i = 0; i < s.dim; ++i) out[(size_t)k * s.dim + i] = held ? s.value_at(keys[k], i) : bits_float(kNanImage);
        if (found) found[k] = held ? 1 : 0;
    }
}

// queries [nq][dim], keys [nq][r_in], counts [nq] or null (every count in [0, r_in]), values [nq][r_in] or null ->
// out_keys [nq][R], out_dist [nq][R], out_sizes [nq]; returns the missing entries of all queries.  Store: store or keyed_store —
// the definition reads a store through dim, holds and distance_to (kIP: score_to) alone.  metric: kL2 or kIP.
template <typename Store>
inline uint64_t rerank(const Store& s, int nq, const float* queries, int r_in, const uint32_t* keys, const int32_t* counts,
                       const float* values, int R, uint32_t* out_keys, float* out_dist, int32_t* out_sizes, int metric = kL2) {
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
            const float* qv = queries + (size_t)q * s.dim;
            const float v = metric == kIP ? s.score_to(qv, k[i]) : s.distance_to(qv, k[i]);
            words.push_back(((uint64_t)image_of(v, metric) << 32) | k[i]);
        }
        std::sort(words.begin(), words.end());
        words.erase(std::unique(words.begin(), words.end()), words.end());
        const int n = (int)std::min<size_t>((size_t)R, words.size());
        for (int j = 0; j < R; ++j) {
            out_keys[(size_t)q * R + j] = j < n ? (uint32_t)words[j] : kNoKey;
            out_dist[(size_t)q * R + j] = j < n ? value_of((uint32_t)(words[j] >> 32), metric) : bits_float(filler_bits(metric));
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
                int32_t* out_sizes, int metric = kL2) {
    std::vector<uint32_t> keys;
    for (uint32_t k : s.held_keys())
        if (!f || f->passes(k)) keys.push_back(k);
    const int n = (int)keys.size();
    for (int q = 0; q < nq; ++q) {   // one query at a time: every list of the rerank call is `keys`
        if (n == 0) {                // (rerank takes r_in >= 1)
            for (int j = 0; j < R; ++j) {
                out_keys[(size_t)q * R + j] = kNoKey;
                out_dist[(size_t)q * R + j] = bits_float(filler_bits(metric));
            }
            out_sizes[q] = 0;
            continue;
        }
        rerank(s, 1, queries + (size_t)q * s.dim, n, keys.data(), nullptr, nullptr, R, out_keys + (size_t)q * R, out_dist + (size_t)q * R,
               out_sizes + q, metric);
    }
}

// ---- probed exact search (qadc_refine_knn_probed) ----
// A partition of an index as the search reads it: row i has the key labels[i], or key_base + i where labels is null (the rule of
// adc::Source in the scan).
struct probe_part {
    const uint32_t* labels;
    uint32_t key_base;
    uint64_t rows;
};

// The R nearest rows among the partitions each query probes.  assign [nq][ma]: P_q is the set of distinct partition numbers of
// query q's list that lie in [0, nparts) — a repeat counts once; a number outside is skipped here (the device form's rule; the
// host form of the C-ABI refuses it before this is reached).  Every row of every p in P_q, partitions in the order of their first
// occurrence and rows ascending, contributes one entry, its key, unless the key fails index_filter (the index's set filter) or f
// (the call's); either may be null.  The result is rerank fed q's entries, with no limit on their number: an entry whose key the
// store does not hold is missing and counted in the return value, per entry; a key that occurs several times is kept once.
template <typename Store>
inline uint64_t knn_probed(const Store& s, const probe_part* parts, int nparts, const filter* index_filter, int nq, const float* queries,
                           int ma, const int32_t* assign, int R, const filter* f, uint32_t* out_keys, float* out_dist, int32_t* out_sizes,
                           int metric = kL2) {
    uint64_t missing = 0;
    std::vector<uint32_t> keys;
    std::vector<int32_t> probed;
    for (int q = 0; q < nq; ++q) {
        keys.clear();
        probed.clear();
        for (int j = 0; j < ma; ++j) {
            const int32_t p = assign[(size_t)q * ma + j];
            if (p < 0 || p >= nparts || std::find(probed.begin(), probed.end(), p) != probed.end()) continue;
            probed.push_back(p);
            for (uint64_t i = 0; i < parts[p].rows; ++i) {
                const uint32_t key = parts[p].labels ? parts[p].labels[i] : (uint32_t)(parts[p].key_base + i);
                if ((index_filter && !index_filter->passes(key)) || (f && !f->passes(key))) continue;
                keys.push_back(key);
            }
        }
        if (keys.empty()) {              // (rerank takes r_in >= 1)
            for (int j = 0; j < R; ++j) {
                out_keys[(size_t)q * R + j] = kNoKey;
                out_dist[(size_t)q * R + j] = bits_float(filler_bits(metric));
            }
            out_sizes[q] = 0;
            continue;
        }
        missing += rerank(s, 1, queries + (size_t)q * s.dim, (int)keys.size(), keys.data(), nullptr, nullptr, R, out_keys + (size_t)q * R,
                          out_dist + (size_t)q * R, out_sizes + q, metric);
    }
    return missing;
}

// ---- exact range search (qadc_refine_range, qadc_refine_rerank_range) ----
// A key is KEPT for query q where the store holds it and D(q, x_key) < radius[q] as a binary32 compare: a NaN distance, a NaN
// radius and a radius <= 0 of either sign keep nothing (D is +0, positive or NaN), a distance equal to the radius is not kept, and
// radius +inf keeps every finite distance.  A kept key gives the word (bits(D) << 32) | key; a query's words are sorted ascending
// and equal words kept once.  There is no R and no cap.
//
// rerank_range: the rule over the candidates keys[in_lims[q] .. in_lims[q + 1]), in_lims monotone from 0.  A candidate whose key
// the store does not hold is MISSING: dropped and counted in the return value.  lims gets nq + 1 offsets, out_keys and out_dist the
// lims[nq] kept rows of all queries one behind the other.
template <typename Store>
inline uint64_t rerank_range(const Store& s, int nq, const float* queries, const uint64_t* in_lims, const uint32_t* keys, const float* radius,
                             std::vector<uint64_t>& lims, std::vector<uint32_t>& out_keys, std::vector<float>& out_dist) {
    uint64_t missing = 0;
    std::vector<uint64_t> words;
    lims.assign(1, 0);
    out_keys.clear();
    out_dist.clear();
    for (int q = 0; q < nq; ++q) {
        words.clear();
        for (uint64_t i = in_lims[q]; i < in_lims[q + 1]; ++i) {
            const uint32_t k = keys[(size_t)i];
            if (!s.holds(k)) {
                ++missing;
                continue;
            }
            const float d = s.distance_to(queries + (size_t)q * s.dim, k);
            if (d < radius[q]) words.push_back(((uint64_t)float_bits(d) << 32) | k);
        }
        std::sort(words.begin(), words.end());
        words.erase(std::unique(words.begin(), words.end()), words.end());
        for (uint64_t w : words) {
            out_keys.push_back((uint32_t)w);
            out_dist.push_back(bits_float((uint32_t)(w >> 32)));
        }
        lims.push_back(lims.back() + words.size());
    }
    return missing;
}

// range: the kept rows of the whole store — rerank_range with every query's candidates = every held key that passes `filter`
// (null: every held key).  Nothing is missing and nothing repeats: a store holds a key once.
template <typename Store>
inline void range(const Store& s, int nq, const float* queries, const float* radius, const filter* f, std::vector<uint64_t>& lims,
                  std::vector<uint32_t>& out_keys, std::vector<float>& out_dist) {
    std::vector<uint32_t> keys;
    for (uint32_t k : s.held_keys())
        if (!f || f->passes(k)) keys.push_back(k);
    const uint64_t seg[2] = {0, (uint64_t)keys.size()};
    std::vector<uint64_t> one;
    std::vector<uint32_t> ok;
    std::vector<float> od;
    lims.assign(1, 0);
    out_keys.clear();
    out_dist.clear();
    for (int q = 0; q < nq; ++q) {   // one query at a time: every segment of the rerank_range call is `keys`
        rerank_range(s, 1, queries + (size_t)q * s.dim, seg, keys.data(), radius + q, one, ok, od);
        out_keys.insert(out_keys.end(), ok.begin(), ok.end());
        out_dist.insert(out_dist.end(), od.begin(), od.end());
        lims.push_back(lims.back() + one[1]);
    }
}

}  // namespace refine
}  // namespace qadc
