// Host path of BASELINE configs[0] — the reference's plain ADC scanner (db_query.cpp:17-46) and its scan kernels
// (query_common.hpp:59-146), C++14, header only, NO GPU: this is the CPU plumbing every other path is measured against
// ("Flat DB, PQ 8x8 scalar ADC on CPU, db_query reference path"), kept next to the accelerated scanner so that the
// stand-alone driver (tests/cpp/db_query_simple.cpp) offers both of the reference's query front ends.
//
//   pq_bytes            base_pq / opq with whole-byte codes (sq_bits 8 or 16; quantizers.hpp:96-324): encode, the OPQ rotation,
//                       the two table forms (device twins: adc_tables_kernel, adc_encode_kernel in csrc/qadc_adc_kernel.hip)
//   scan_standard<T,N>  query_common.hpp:92-118: candidate = sum of NSQ table entries in sub-quantizer order
//   scan_4f<N>          query_common.hpp:59-90: the same on row-major 4-bit codes (low nibble = even sub-quantizer)
//   get_scan_func       query_common.hpp:120-146: the (sq_count, sq_bits) dispatch and its error text
//   scanner_simple      db_query.cpp:17-46: R sentinel pushes FLT_MAX - t, then every probed partition in assign[] order
//   key_filter          no reference counterpart: the allow / exclude key set the scan loops skip rows by (set_filter), and a
//                       second one of the query's own chained to it (set_query_filter): a row must pass both
//   range_scan          no reference counterpart: every row below a radius, sorted by (candidate, key) (range_standard, range_4f)
// Float sums take the grouping of the reference AS COMPILED with its -ffast-math (host/float_sum.hpp; float_sum_mode() = 0
// gives the source order); this file itself is built without -ffast-math.  The oracle's orc_scan_standard_u8 /
// orc_candidates_f32 / orc_tables_direct, pinned to the reference build, are the checkers (tests/test_scanner_hip_cpp.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <vector>

#include "float_sum.hpp"
#include "qadc_heap.hpp"

namespace qadc {

typedef kv_heap<unsigned, float> float_heap;

// The key filter of a scan — the written definition of qadc_adc_index_set_filter (include/qadc.h), which the
// reference does not have.  A row's key is what the scan would push for it (its label, else its position); the scan loops below skip a
// row the filter drops before they look at its candidate, which is the reference's loop over the partition without that row, its key kept.
// A filter may be chained to a second one (`also`): the written definition of the *_filtered calls, where a
// row must pass the index's filter and its query's — it is dropped as soon as either drops it.
struct key_filter {
    enum { exclude = 0, allow = 1 };                             // QADC_ADC_FILTER_EXCLUDE, QADC_ADC_FILTER_ALLOW
    int mode;
    std::vector<unsigned> keys;                                  // sorted, unique
    const key_filter* also = nullptr;                            // not owned; null = this filter alone
    key_filter(int mode_, const unsigned* k, std::size_t count) : mode(mode_), keys(k, k + count) {
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    }
    key_filter chained(const key_filter* second) const {         // this set and mode, and `second` behind it
        key_filter both(*this);
        both.also = second;
        return both;
    }
    bool drops(unsigned key) const {
        return std::binary_search(keys.begin(), keys.end(), key) == (mode == exclude) || (also != nullptr && also->drops(key));
    }
};

template <typename T, int NSQ>
void scan_standard(const std::uint8_t* pqcodes_, const unsigned* labels, const unsigned pqcodes_count, const float* dists,
                   float_heap& bh, const key_filter* filter = nullptr) {
    const int NCENT = 1 << (sizeof(T) * 8);
    const T* const pqcodes = reinterpret_cast<const T*>(pqcodes_);
    float min = bh.max();
    for (unsigned i = 0; i < pqcodes_count; ++i) {
        if (filter && filter->drops(labels != nullptr ? labels[i] : i)) continue;
        const T* const code = pqcodes + (std::size_t)i * NSQ;
        float t[NSQ];
        for (int sq = 0; sq < NSQ; ++sq) t[sq] = dists[sq * NCENT + code[sq]];
        const float candidate = adc_sum<NSQ>(t);
        if (candidate < min) {
            bh.push(labels != nullptr ? labels[i] : i, candidate);
            min = bh.max();
        }
    }
}

template <int NSQ>
void scan_4f(const std::uint8_t* pqcodes, const unsigned* labels, const unsigned pqcodes_count, const float* dists,
             float_heap& bh, const key_filter* filter = nullptr) {
    float min = bh.max();
    for (unsigned i = 0; i < pqcodes_count; ++i) {
        if (filter && filter->drops(labels != nullptr ? labels[i] : i)) continue;
        const std::uint8_t* const code = pqcodes + (std::size_t)i * (NSQ / 2);
        float t[NSQ];
        for (int b = 0; b < NSQ / 2; ++b) {                      // byte b: low nibble = sub-quantizer 2b, high nibble = 2b + 1
            t[2 * b] = dists[(2 * b) * 16 + (code[b] & 0xf)];
            t[2 * b + 1] = dists[(2 * b + 1) * 16 + (code[b] >> 4)];
        }
        const float candidate = adc_sum<NSQ>(t);
        if (candidate < min) {
            bh.push(labels != nullptr ? labels[i] : i, candidate);
            min = bh.max();
        }
    }
}

typedef void (*scan_func)(const std::uint8_t*, const unsigned*, unsigned, const float*, float_heap&, const key_filter*);

template <typename Pq>
scan_func get_scan_func(const Pq& pq) {
    if (pq.sq_count == 16 && pq.sq_bits == 4) return scan_4f<16>;
    if (pq.sq_count == 32 && pq.sq_bits == 4) return scan_4f<32>;
    if (pq.sq_count == 4 && pq.sq_bits == 8) return scan_standard<std::uint8_t, 4>;
    if (pq.sq_count == 8 && pq.sq_bits == 8) return scan_standard<std::uint8_t, 8>;
    if (pq.sq_count == 16 && pq.sq_bits == 8) return scan_standard<std::uint8_t, 16>;
    if (pq.sq_count == 2 && pq.sq_bits == 16) return scan_standard<std::uint16_t, 2>;
    if (pq.sq_count == 4 && pq.sq_bits == 16) return scan_standard<std::uint16_t, 4>;
    if (pq.sq_count == 8 && pq.sq_bits == 16) return scan_standard<std::uint16_t, 8>;
    std::cerr << "Unsupported (nsq,nsq_bits) configuration." << std::endl;
    std::cerr << "Supported configurations are: (16,4) (4,8) (8,8) (16,8) (2,16) (4,16) (8,16)." << std::endl;
    std::exit(1);
}

// ---- range search: every row whose candidate lies below a radius (no reference counterpart; the written definition of
// qadc_adc_range_*, include/qadc.h) ----
// order_image: the order-preserving integer image of a float (order_key in csrc/qadc_adc_kernel.hip): -x < -y < -0 < +0 < y < x.
inline std::uint32_t order_image(float v) {
    std::uint32_t u;
    std::memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float order_image_value(std::uint32_t k) {
    const std::uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}
inline std::uint64_t range_word(unsigned key, float candidate) { return ((std::uint64_t)order_image(candidate) << 32) | key; }

// The scan loops of a range query, beside scan_standard / scan_4f: the same candidate (adc_sum grouping, float_sum_mode), kept iff
// candidate < radius as a float compare — a NaN on either side keeps nothing, a candidate equal to the radius is not kept — and
// appended to `kept` as range_word(key, candidate).
template <typename T, int NSQ>
void range_standard(const std::uint8_t* pqcodes_, const unsigned* labels, const unsigned pqcodes_count, const float* dists,
                    float radius, std::vector<std::uint64_t>& kept, const key_filter* filter = nullptr) {
    const int NCENT = 1 << (sizeof(T) * 8);
    const T* const pqcodes = reinterpret_cast<const T*>(pqcodes_);
    for (unsigned i = 0; i < pqcodes_count; ++i) {
        const unsigned key = labels != nullptr ? labels[i] : i;
        if (filter && filter->drops(key)) continue;
        const T* const code = pqcodes + (std::size_t)i * NSQ;
        float t[NSQ];
        for (int sq = 0; sq < NSQ; ++sq) t[sq] = dists[sq * NCENT + code[sq]];
        const float candidate = adc_sum<NSQ>(t);
        if (candidate < radius) kept.push_back(range_word(key, candidate));
    }
}

template <int NSQ>
void range_4f(const std::uint8_t* pqcodes, const unsigned* labels, const unsigned pqcodes_count, const float* dists, float radius,
              std::vector<std::uint64_t>& kept, const key_filter* filter = nullptr) {
    for (unsigned i = 0; i < pqcodes_count; ++i) {
        const unsigned key = labels != nullptr ? labels[i] : i;
        if (filter && filter->drops(key)) continue;
        const std::uint8_t* const code = pqcodes + (std::size_t)i * (NSQ / 2);
        float t[NSQ];
        for (int b = 0; b < NSQ / 2; ++b) {
            t[2 * b] = dists[(2 * b) * 16 + (code[b] & 0xf)];
            t[2 * b + 1] = dists[(2 * b + 1) * 16 + (code[b] >> 4)];
        }
        const float candidate = adc_sum<NSQ>(t);
        if (candidate < radius) kept.push_back(range_word(key, candidate));
    }
}

typedef void (*range_func)(const std::uint8_t*, const unsigned*, unsigned, const float*, float, std::vector<std::uint64_t>&,
                           const key_filter*);

template <typename Pq>
range_func get_range_func(const Pq& pq) {   // the shapes of get_scan_func, which has refused every other one before this is asked
    if (pq.sq_count == 16 && pq.sq_bits == 4) return range_4f<16>;
    if (pq.sq_count == 32 && pq.sq_bits == 4) return range_4f<32>;
    if (pq.sq_count == 4 && pq.sq_bits == 8) return range_standard<std::uint8_t, 4>;
    if (pq.sq_count == 8 && pq.sq_bits == 8) return range_standard<std::uint8_t, 8>;
    if (pq.sq_count == 16 && pq.sq_bits == 8) return range_standard<std::uint8_t, 16>;
    if (pq.sq_count == 2 && pq.sq_bits == 16) return range_standard<std::uint16_t, 2>;
    if (pq.sq_count == 4 && pq.sq_bits == 16) return range_standard<std::uint16_t, 4>;
    if (pq.sq_count == 8 && pq.sq_bits == 16) return range_standard<std::uint16_t, 8>;
    return nullptr;
}

// The result of one range query: the kept (key, candidate) pairs ascending by range_word.
struct range_result {
    std::vector<unsigned> keys;
    std::vector<float> values;
};

// base_pq with whole-byte codes: sq_bits 8 (one byte per sub-quantizer) or 16 (two, little endian).
struct pq_bytes {
    int sq_count, sq_bits, dim;
    std::vector<float> centroids;                                // [sq_count][ncent][sq_dim]
    std::vector<float> rotation;                                 // OPQ: [dim][dim], empty for plain PQ (quantizers.hpp:248-324)
    pq_bytes(int m, int bits, int d) : sq_count(m), sq_bits(bits), dim(d), centroids((std::size_t)m * (1u << bits) * (d / m)) {}
    int ncent() const { return 1 << sq_bits; }
    int sq_dim() const { return dim / sq_count; }
    int code_size() const { return sq_count * sq_bits / 8; }
    int table_dim() const { return sq_count * ncent(); }
    const float* centroid(int m, int c) const { return centroids.data() + ((std::size_t)m * ncent() + c) * sq_dim(); }
    // opq::rotate_multiple_vectors (quantizers.hpp:289-301): rotated[r] = sum_c x[c] * rotation[r][c], one sequential float sum
    // in ascending c (pq4::rotate_multiple_vectors in host/query_driver.hpp; the device feeders add in the same order);
    // plain PQ: no-op (189-195)
    void rotate_multiple_vectors(float* vecs, int count) const {
        if (rotation.empty()) return;
        std::vector<float> out((std::size_t)dim);
        for (int v = 0; v < count; ++v) {
            float* x = vecs + (std::size_t)v * dim;
            for (int r = 0; r < dim; ++r) {
                float acc = 0;
                for (int c = 0; c < dim; ++c) acc += x[c] * rotation[(std::size_t)r * dim + c];
                out[r] = acc;
            }
            for (int r = 0; r < dim; ++r) x[r] = out[r];
        }
    }
    void tables(const float* x, float* out) const {              // ||x_m - c||^2 as fmanorm adds it (float_sum.hpp)
        const int ds = sq_dim(), nc = ncent();
        for (int m = 0; m < sq_count; ++m)
            for (int c = 0; c < nc; ++c) out[m * nc + c] = sqdist(x + m * ds, centroid(m, c), ds);
    }
    void tables_direct(const float* x, float* out) const { tables(x, out); }   // the engine's name for the ma == 1 form
    void tables_blas(const float* vecs, int count, float* out) const {   // (||v||^2 + ||c||^2) - 2 v.c, distances.hpp:151-183
        const int ds = sq_dim(), nc = ncent();                           // (norms as compiled, one sequential dot: float_sum.hpp)
        std::vector<float> cn((std::size_t)sq_count * nc);
        for (int e = 0; e < sq_count * nc; ++e) cn[e] = sqnorm(centroids.data() + (std::size_t)e * ds, ds);
        for (int v = 0; v < count; ++v)
            for (int m = 0; m < sq_count; ++m) {
                const float* x = vecs + (std::size_t)v * dim + m * ds;
                const float vn = sqnorm(x, ds);
                for (int c = 0; c < nc; ++c)
                    out[((std::size_t)v * sq_count + m) * nc + c] = expansion_dist(x, centroid(m, c), ds, vn, cn[m * nc + c]);
            }
    }
    // encode_multiple_vectors (quantizers.hpp:222-245): the rotation (opq), then find_k_neighbors with k = 1 on the expansion
    // distances: a capacity-1 kv_binheap fed in centroid order, whose replace test as compiled is !(s >= kept) — the first
    // strict minimum after the last NaN (the last centroid when its distance is NaN); without NaN the first strict minimum
    void encode(const float* vecs, std::size_t n, std::uint8_t* codes) const {
        const int nc = ncent(), cs = code_size();
        std::vector<float> t((std::size_t)table_dim()), rot;
        for (std::size_t i = 0; i < n; ++i) {
            const float* x = vecs + i * dim;
            if (!rotation.empty()) {
                rot.assign(x, x + dim);
                rotate_multiple_vectors(rot.data(), 1);
                x = rot.data();
            }
            tables_blas(x, 1, t.data());
            for (int m = 0; m < sq_count; ++m) {
                int best = 0;
                for (int c = 1; c < nc; ++c)
                    if (!(t[m * nc + c] >= t[m * nc + best])) best = c;
                if (sq_bits == 8) codes[i * cs + m] = (std::uint8_t)best;
                else { codes[i * cs + 2 * m] = (std::uint8_t)best; codes[i * cs + 2 * m + 1] = (std::uint8_t)(best >> 8); }
            }
        }
    }
};

// db_query.cpp:17-46.  Db offers base_db's get_partition (databases.hpp:50-55) and a `pq` with sq_count / sq_bits.
template <typename Db>
struct scanner_simple {
    typedef float_heap BhType;
    Db* db = nullptr;
    scan_func scan = nullptr;
    range_func range = nullptr;
    const key_filter* filter = nullptr;                          // set_filter: not owned, null = the reference's scan
    void set_filter(const key_filter* f) { filter = f; }
    const key_filter* query_filter = nullptr;                    // set_query_filter: the filter of the query scanned next, on top of `filter`
    void set_query_filter(const key_filter* f) { query_filter = f; }
    void prepare_database(Db& database) {
        db = &database;
        scan = get_scan_func(*database.pq);
        range = get_range_func(*database.pq);
    }
    template <typename Metrics>
    void query_scan(const float*, int* assign, int ma, float* tables, int table_dim, BhType& bh, Metrics&) {
        for (int t = 0; t < bh.capacity(); ++t) bh.push(0, std::numeric_limits<float>::max() - t);   // "Fill binary heap"
        const std::uint8_t* codes;
        unsigned* labels;
        unsigned count;
        const bool two = filter != nullptr && query_filter != nullptr;
        const key_filter both = two ? filter->chained(query_filter) : key_filter(key_filter::exclude, nullptr, 0);
        const key_filter* const pass = two ? &both : filter != nullptr ? filter : query_filter;   // one filter or none: as before
        for (int a = 0; a < ma; ++a) {
            db->get_partition(assign[a], codes, labels, count);
            scan(codes, labels, count, tables, bh, pass);
            tables += table_dim;
        }
    }
    // Range search: every row of the probed partitions, in assign[] order, that passes the chained filter
    // as in query_scan and whose candidate is < radius; `out` = the kept pairs ascending by (order_image(candidate) << 32) | key.
    // Nothing is deduplicated: the result depends only on the multiset of kept (candidate, key) pairs.
    void range_scan(int* assign, int ma, float* tables, int table_dim, float radius, range_result& out) {
        const std::uint8_t* codes;
        unsigned* labels;
        unsigned count;
        const bool two = filter != nullptr && query_filter != nullptr;
        const key_filter both = two ? filter->chained(query_filter) : key_filter(key_filter::exclude, nullptr, 0);
        const key_filter* const pass = two ? &both : filter != nullptr ? filter : query_filter;
        std::vector<std::uint64_t> kept;
        for (int a = 0; a < ma; ++a) {
            db->get_partition(assign[a], codes, labels, count);
            range(codes, labels, count, tables, radius, kept, pass);
            tables += table_dim;
        }
        std::sort(kept.begin(), kept.end());
        out.keys.resize(kept.size());
        out.values.resize(kept.size());
        for (std::size_t i = 0; i < kept.size(); ++i) {
            out.keys[i] = (unsigned)kept[i];
            out.values[i] = order_image_value((std::uint32_t)(kept[i] >> 32));
        }
    }
};

}  // namespace qadc
