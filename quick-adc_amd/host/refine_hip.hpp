// refine_store_hip — C++14 RAII mirror of the refine store (qadc_refine_* in include/qadc.h; DESIGN.md sections 11.11, 11.14 and 11.20): the
// original vectors in device memory, dense over the keys [lo, lo + rows) or, with keyed = true, a map from key to vector filled by
// put() and emptied by remove(); rerank(), which reorders candidate keys by their exact squared L2 distance to them; range() and
// rerank_range(), the exact radius query over the whole store and over a range result (section 11.21); knn_probed() and search_exact(),
// the exact search over the partitions of an index a query probes (section 11.22).  search_refined() composes it with adc_search_engine_hip (host/adc_search_hip.hpp): the engine's search with
// R = the engine's r as r_in, then the re-ranking of the heaps' keys, the FLT_MAX sentinels left out.  The definition both are held
// to is host/refine.hpp.  set_metric(QADC_REFINE_IP) (section 11.23) makes rerank(), knn(), knn_probed() and the compositions rank by the
// inner product, larger first: `dist` then holds the scores, descending, and -inf behind sizes[q]; range() and rerank_range() are L2 only.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "../../include/qadc.h"
#include "adc_search_hip.hpp"

namespace qadc {

struct refine_result {
    int r = 0;                            // slots per query
    std::vector<std::uint32_t> keys;      // [nq][r], ascending by (distance, key) — QADC_REFINE_IP: descending score, then key; behind sizes[q]: 0xFFFFFFFF
    std::vector<float> dist;              // [nq][r]; behind sizes[q]: +inf (QADC_REFINE_IP: the scores, -inf)
    std::vector<std::int32_t> sizes;      // [nq]
    std::uint64_t missing = 0;            // candidates whose key the store does not hold
};

// An exact range result in CSR form (qadc_refine_range*, qadc_refine_rerank_range*)
struct refine_range_result {
    std::vector<std::uint64_t> lims;      // [nq + 1]: query q's rows are [lims[q], lims[q + 1])
    std::vector<std::uint32_t> keys;      // ascending by (distance, key) within a query
    std::vector<float> dist;
    std::uint64_t missing = 0;            // rerank_range: candidates whose key the store does not hold
};

struct refine_store_hip {
    qadc_refine* store = nullptr;
    int dim;

    refine_store_hip(int dim_, int dtype = QADC_REFINE_F32, int device = 0, bool keyed = false) : dim(dim_) {
        if ((keyed ? qadc_refine_create_keyed(&store, dim_, dtype, device) : qadc_refine_create(&store, dim_, dtype, device)) != QADC_OK)
            die("Cannot create the refine store");
    }
    // SQ8 rows (qadc_refine_create_sq8): one byte per component under the range vmin [dim], step [dim]
    refine_store_hip(int dim_, const float* vmin, const float* step, int device = 0, bool keyed = false) : dim(dim_) {
        if (qadc_refine_create_sq8(&store, dim_, vmin, step, keyed ? 1 : 0, device) != QADC_OK) die("Cannot create the SQ8 refine store");
    }
    refine_store_hip(const refine_store_hip&) = delete;
    refine_store_hip& operator=(const refine_store_hip&) = delete;
    ~refine_store_hip() { qadc_refine_destroy(store); }

    static void die(const char* what) {
        std::cerr << what << ": " << qadc_last_error() << std::endl;
        std::exit(1);
    }

    // the metric of every later rerank, knn and knn_probed call (qadc_refine_set_metric): QADC_REFINE_L2 (the
    // default) or QADC_REFINE_IP; host state only
    void set_metric(int metric) {
        if (qadc_refine_set_metric(store, metric) != QADC_OK) die("set_metric");
    }

    int metric() const {
        int m = QADC_REFINE_L2;
        if (qadc_refine_metric(store, &m) != QADC_OK) die("metric");
        return m;
    }

    void reserve(std::uint64_t rows) {
        if (qadc_refine_reserve(store, rows) != QADC_OK) die("reserve");
    }

    // vectors [count][dim] become the rows of the keys first_key .. first_key + count - 1 (the first add fixes lo)
    void add(const float* vectors, std::uint64_t count, std::uint32_t first_key) {
        if (qadc_refine_add(store, vectors, count, first_key) != QADC_OK) die("add");
    }

    // a keyed store: the vector of key labels[i] becomes vectors[i] ([count][dim]); the last occurrence of a key wins
    void put(const float* vectors, const std::uint32_t* labels, std::uint64_t count) {
        if (qadc_refine_put(store, vectors, labels, count) != QADC_OK) die("put");
    }

    // a keyed store: every listed key that is held leaves; returns how many left
    std::uint64_t remove(const std::uint32_t* labels, std::uint64_t count) {
        std::uint64_t removed = 0;
        if (qadc_refine_remove(store, labels, count, &removed) != QADC_OK) die("remove");
        return removed;
    }

    // the rows a dense store holds, the keys a keyed one holds
    std::uint64_t rows() const {
        std::uint64_t n = 0;
        qadc_refine_info(store, nullptr, nullptr, nullptr, &n, nullptr);
        return n;
    }

    // the rows of keys [count] as floats [count][dim], decoded by the store's type; a key not held gives a row of NaN and found 0
    std::vector<float> get(const std::uint32_t* keys, std::uint64_t count, std::vector<std::uint8_t>* found = nullptr) {
        std::vector<float> out((std::size_t)count * dim);
        if (found) found->resize((std::size_t)count);
        if (qadc_refine_get(store, keys, count, out.data(), found ? found->data() : nullptr) != QADC_OK) die("get");
        return out;
    }

    // an SQ8 store: its range (either may be null) and the components written outside it so far
    std::uint64_t sq_info(std::vector<float>* vmin = nullptr, std::vector<float>* step = nullptr) const {
        std::uint64_t clamped = 0;
        if (vmin) vmin->resize(dim);
        if (step) step->resize(dim);
        if (qadc_refine_sq_info(store, vmin ? vmin->data() : nullptr, step ? step->data() : nullptr, &clamped) != QADC_OK) die("sq_info");
        return clamped;
    }

    // queries [nq][dim], keys [nq][r_in], counts [nq] or null, values [nq][r_in] or null -> the first r of every query's candidates
    refine_result rerank(int nq, const float* queries, int r_in, const std::uint32_t* keys, const std::int32_t* counts, const float* values,
                         int r) {
        refine_result out;
        out.r = r;
        out.keys.resize((std::size_t)nq * r);
        out.dist.resize((std::size_t)nq * r);
        out.sizes.resize(nq);
        if (qadc_refine_rerank(store, nq, queries, r_in, keys, counts, values, r, out.keys.data(), out.dist.data(), out.sizes.data(),
                               &out.missing) != QADC_OK)
            die("rerank");
        return out;
    }

    // Exhaustive search (qadc_refine_knn): queries [nq][dim] -> per query the first r of every key the store
    // holds that passes `filter` (null: every key), by (exact distance, key)
    refine_result knn(int nq, const float* queries, int r, const qadc_adc_filter* filter = nullptr) {
        refine_result out;
        out.r = r;
        out.keys.resize((std::size_t)nq * r);
        out.dist.resize((std::size_t)nq * r);
        out.sizes.resize(nq);
        if (qadc_refine_knn(store, nq, queries, r, filter, out.keys.data(), out.dist.data(), out.sizes.data()) != QADC_OK) die("knn");
        return out;
    }

    // the same with every array in device memory of the store's device: d_queries [nq][dim] -> d_keys [nq][r], d_dist [nq][r], d_sizes [nq]
    void knn_device(int nq, const float* d_queries, int r, const qadc_adc_filter* filter, std::uint32_t* d_keys, float* d_dist,
                    std::int32_t* d_sizes) {
        if (qadc_refine_knn_device(store, nq, d_queries, r, filter, d_keys, d_dist, d_sizes) != QADC_OK) die("knn_device");
    }

    // Probed exact search (qadc_refine_knn_probed): queries [nq][dim], assign [nq][ma] -> per query the first
    // r, by (exact distance, key), of the keys of every row of the partitions of `index` its list probes; a key must pass the index's
    // filter and `filter`, a key not held is counted in `missing`, a key reached through several rows is kept once
    refine_result knn_probed(const qadc_adc_index* index, int nq, const float* queries, int ma, const std::int32_t* assign, int r,
                             const qadc_adc_filter* filter = nullptr) {
        refine_result out;
        out.r = r;
        out.keys.resize((std::size_t)nq * r);
        out.dist.resize((std::size_t)nq * r);
        out.sizes.resize(nq);
        if (qadc_refine_knn_probed(store, index, nq, queries, ma, assign, r, filter, out.keys.data(), out.dist.data(), out.sizes.data(),
                                   &out.missing) != QADC_OK)
            die("knn_probed");
        return out;
    }

    // the same with every array in device memory of the store's device; returns the missing count
    std::uint64_t knn_probed_device(const qadc_adc_index* index, int nq, const float* d_queries, int ma, const std::int32_t* d_assign, int r,
                                    const qadc_adc_filter* filter, std::uint32_t* d_keys, float* d_dist, std::int32_t* d_sizes) {
        std::uint64_t missing = 0;
        if (qadc_refine_knn_probed_device(store, index, nq, d_queries, ma, d_assign, r, filter, d_keys, d_dist, d_sizes, &missing) != QADC_OK)
            die("knn_probed_device");
        return missing;
    }

    // a tuning and test knob (qadc_refine_set_knn_plan): 0 = the plan's default; no value changes a result
    void set_knn_plan(std::uint64_t chunk_rows, int pass_nq) {
        if (qadc_refine_set_knn_plan(store, chunk_rows, pass_nq) != QADC_OK) die("set_knn_plan");
    }

    // the range result the store holds, copied out (qadc_refine_range_collect); lims: what the range call returned
    void range_collect(refine_range_result& out) {
        const std::uint64_t n = out.lims.empty() ? 0 : out.lims.back();
        out.keys.resize((std::size_t)n);
        out.dist.resize((std::size_t)n);
        if (qadc_refine_range_collect(store, n, out.keys.data(), out.dist.data()) != QADC_OK) die("range_collect");
    }

    // Exact range search (qadc_refine_range): queries [nq][dim], radius [nq] -> per query every key the store
    // holds that passes `filter` (null: every key) and whose exact distance is < radius[q], by (distance, key)
    refine_range_result range(int nq, const float* queries, const float* radius, const qadc_adc_filter* filter = nullptr) {
        refine_range_result out;
        out.lims.assign((std::size_t)nq + 1, 0);
        if (qadc_refine_range(store, nq, queries, radius, filter, out.lims.data()) != QADC_OK) die("range");
        range_collect(out);
        return out;
    }

    // The same rule over the candidates keys[in_lims[q] .. in_lims[q + 1]) of query q (qadc_refine_rerank_range): no limit on their
    // number, a key listed several times kept once, a key not held counted in `missing`
    refine_range_result rerank_range(int nq, const float* queries, const std::uint64_t* in_lims, const std::uint32_t* keys, const float* radius) {
        refine_range_result out;
        out.lims.assign((std::size_t)nq + 1, 0);
        if (qadc_refine_rerank_range(store, nq, queries, in_lims, keys, radius, out.lims.data(), &out.missing) != QADC_OK) die("rerank_range");
        range_collect(out);
        return out;
    }

    // a tuning and test knob (qadc_refine_set_range_plan): 0 = the plan's default; no value changes a result
    void set_range_plan(std::uint64_t region_rows, std::uint64_t chunk_rows, int pass_nq) {
        if (qadc_refine_set_range_plan(store, region_rows, chunk_rows, pass_nq) != QADC_OK) die("set_range_plan");
    }

    // passes of range() that ran a second time because a query's region overflowed
    std::uint64_t range_reruns() const { return qadc_refine_range_reruns(store); }
};

// The engine's search of nq queries with heaps of e.r entries, then their keys re-ranked against `store`: the first r by (exact
// distance, key).  cand_keys / cand_vals (may be null) receive the heaps' arrays [nq][e.r] the re-ranking consumed.
template <typename Db>
inline refine_result search_refined(adc_search_engine_hip<Db>& e, refine_store_hip& store, int nq, const float* queries, int r,
                                    std::vector<std::uint32_t>* cand_keys = nullptr, std::vector<float>* cand_vals = nullptr) {
    std::vector<std::uint32_t> keys((std::size_t)nq * e.r);
    std::vector<float> vals((std::size_t)nq * e.r);
    std::vector<std::int32_t> sizes(nq), assign((std::size_t)nq * e.ma);
    if (qadc_adc_search(e.index, nq, queries, e.ma, e.r, e.table_form, e.sum_mode, keys.data(), vals.data(), sizes.data(), assign.data()) !=
        QADC_OK)
        adc_search_engine_hip<Db>::die("search");
    refine_result out = store.rerank(nq, queries, e.r, keys.data(), nullptr, vals.data(), r);
    if (cand_keys) cand_keys->swap(keys);
    if (cand_vals) cand_vals->swap(vals);
    return out;
}

// Exact search over the partitions the engine would probe (qadc_adc_search_exact): the engine's coarse step at
// its ma, then store.knn_probed on the probe lists — the ceiling of search_refined at the same ma.  assign (may be null) receives the
// probe lists [nq][e.ma].
template <typename Db>
inline refine_result search_exact(adc_search_engine_hip<Db>& e, refine_store_hip& store, int nq, const float* queries, int r,
                                  const qadc_adc_filter* filter = nullptr, std::vector<std::int32_t>* assign = nullptr) {
    refine_result out;
    out.r = r;
    out.keys.resize((std::size_t)nq * r);
    out.dist.resize((std::size_t)nq * r);
    out.sizes.resize(nq);
    std::vector<std::int32_t> probes((std::size_t)nq * e.ma);
    if (qadc_adc_search_exact(e.index, store.store, nq, queries, e.ma, r, e.sum_mode, filter, out.keys.data(), out.dist.data(), out.sizes.data(),
                              &out.missing, probes.data()) != QADC_OK)
        adc_search_engine_hip<Db>::die("search_exact");
    if (assign) assign->swap(probes);
    return out;
}

// The engine's range search of queries [query_i, query_i + nq) under adc_radius [nq], then its rows re-ranked against `store` under
// the exact radius [nq]: every key of the ADC result whose exact distance is < radius[q], once, by (distance, key).  adc_lims /
// adc_keys (may be null) receive the ADC result the re-ranking consumed.  Host arrays throughout; the device chain — range_search_device,
// range_collect_device, rerank_range_device, nothing but the two lims arrays crossing the bus — is pyqadc's
// AdcIndex.range_search_refined_device.  tests/cpp/refine_range_search_hip_demo.cpp holds this function to the twin.
template <typename Db>
inline refine_range_result range_search_refined(adc_search_engine_hip<Db>& e, refine_store_hip& store, int query_i, const float* queries, int nq,
                                                const float* adc_radius, const float* radius, std::vector<std::uint64_t>* adc_lims = nullptr,
                                                std::vector<std::uint32_t>* adc_keys = nullptr) {
    std::vector<std::uint64_t> lims;
    std::vector<std::uint32_t> keys;
    std::vector<float> values;
    e.range_search(query_i, queries, nq, adc_radius, lims, keys, values);
    refine_range_result out = store.rerank_range(nq, queries + (std::size_t)query_i * store.dim, lims.data(), keys.data(), radius);
    if (adc_lims) adc_lims->swap(lims);
    if (adc_keys) adc_keys->swap(keys);
    return out;
}

}  // namespace qadc
