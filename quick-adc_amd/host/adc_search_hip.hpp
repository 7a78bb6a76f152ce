// adc_search_engine_hip — C++14 host mirror of nns_engine_batch<scanner_simple> on the GPU, queries in.
//
// nns_engine_batch (query_common.hpp:149-243) prepares the tables of `batch` queries on the CPU when the first query of a batch is
// asked for (assign_compute_residuals, rotate_multiple_vectors, the distance tables: 194-213) and scanner_simple then scans every
// query with them.  This engine offers the same contract — prepare_database(), process_query(query_i, queries, count, bh, metrics),
// to be driven by the reference's process_queries<> loop (query_driver.hpp process_queries here) — and hands the query VECTORS to
// qadc_adc_search_candidates (include/qadc.h): coarse assignment, residuals, OPQ rotation and tables are computed in GPU memory and
// scanned there, so no table crosses the bus.  The per-query calls replay the batch's cached candidate stream into the caller's heap
// after its R sentinel pushes (db_query.cpp:31-33), which leaves it in exactly the state the reference's scan would.
//   Db:   int partition_count(); void get_partition(int, const std::uint8_t*&, unsigned*&, unsigned&);
//         int coarse_count(); const float* coarse_centroids();            (0 / nullptr: a flat database)
//         pq->sq_count, pq->sq_bits, pq->dim, pq->centroids, pq->rotation  (host/scanner_simple.hpp pq_bytes; query_driver.hpp pq4)
// 16-bit codes ((2,16) (4,16) (8,16)): the index is qadc_adc_index_create16's, the codebooks [sq_count][65536][dim / sq_count].
// 4-bit codes ((16,4) (32,4)): database and quantizers go into a qadc_index, and the engine searches through a view of it
// (qadc_adc_index_create_view) — the index db_query_4's engine would use, asked the exact float question.
//   Heap: int capacity(); void push(unsigned, float)                       (kv_binheap<unsigned, float>, binheap.hpp)
// table_form: 1 = the BLAS-expansion tables nns_engine_batch builds (default), 0 = direct, 2 = nns_engine's rule.
// set_finish(QADC_ADC_FINISH_DEVICE): the batch's heaps are ordered and replayed on the GPU (qadc_adc_search under
// qadc_adc_index_set_finish) and a query's arrays are pushed into the caller's empty heap in array order, which rebuilds them
// exactly; the default is the host finish, the candidate stream.
// set_filter(f): the scans drop the rows whose key does not pass the qadc_adc_filter f (qadc_adc_index_set_filter).
// set_query_filters(per_query): one filter per query of the caller's query array on top of it (qadc_adc_search_filtered,
// qadc_adc_search_candidates_filtered).
// range_search(...): every row below a radius per query instead of the R best, under the same filters (qadc_adc_range_search;
// DESIGN.md section 11.13).  range_search_refined(engine, store, ...) of host/refine_hip.hpp hands its rows to a refine store's
// rerank_range: the rows of the ADC result within an exact radius (section 11.21).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <vector>

#include "../../include/qadc.h"
#include "qadc_heap.hpp"
#include "query_driver.hpp"

namespace qadc {

template <typename Db>
struct adc_search_engine_hip {
    Db& db;
    int ma, batch, r, device, sum_mode, table_form;
    int finish = QADC_ADC_FINISH_HOST;
    std::vector<std::int32_t> heap_sizes;   // device finish: [batch]; the arrays are in cand_keys / cand_vals [batch][r]
    qadc_adc_index* index;
    qadc_index* source = nullptr;       // 4-bit codes: the index that holds database and quantizers; `index` is a view of it
    std::vector<std::uint32_t> cand_keys;
    std::vector<float> cand_vals;
    std::vector<std::uint64_t> offsets;
    std::vector<std::int32_t> assign;   // [batch][ma] of the last batch, nearest first

    adc_search_engine_hip(Db& d, int ma_, int batch_, int r_, int device_ = 0, int sum_mode_ = 1, int table_form_ = 1)
        : db(d), ma(ma_), batch(batch_), r(r_), device(device_), sum_mode(sum_mode_), table_form(table_form_), index(nullptr),
          cand_keys(1 << 16), cand_vals(1 << 16), offsets((std::size_t)batch_ + 1), assign((std::size_t)batch_ * ma_) {}
    adc_search_engine_hip(const adc_search_engine_hip&) = delete;
    adc_search_engine_hip& operator=(const adc_search_engine_hip&) = delete;
    ~adc_search_engine_hip() {
        qadc_adc_index_destroy(index);   // (the view first: its source refuses to go while it lives)
        qadc_index_destroy(source);
    }

    static void die(const char* what) {
        std::cerr << what << ": " << qadc_last_error() << std::endl;
        std::exit(1);
    }

    // qadc_adc_index_set_finish: before or after prepare_database, between batches
    void set_finish(int mode) {
        if (mode != QADC_ADC_FINISH_HOST && mode != QADC_ADC_FINISH_DEVICE) {
            std::cerr << "set_finish: mode is QADC_ADC_FINISH_HOST or QADC_ADC_FINISH_DEVICE" << std::endl;
            std::exit(1);
        }
        finish = mode;
        if (index && qadc_adc_index_set_finish(index, mode) != QADC_OK) die("set_finish");
    }

    // qadc_adc_index_set_filter: before or after prepare_database, between batches; null clears.  The filter is the caller's
    // (qadc_adc_filter_create) and must outlive the engine or be cleared first.
    const qadc_adc_filter* filter = nullptr;
    void set_filter(const qadc_adc_filter* f) {
        filter = f;
        if (index && qadc_adc_index_set_filter(index, f) != QADC_OK) die("set_filter");
    }

    // One filter per query: per_query[i] is the filter of query i of the `queries` array process_query is given (its query_i), NULL for
    // none; a null array clears.  The array and its filters are the caller's and are read by every process_query that opens a batch: they
    // stay alive until cleared.  A query's rows pass set_filter's filter and its own.
    const qadc_adc_filter* const* query_filters = nullptr;
    void set_query_filters(const qadc_adc_filter* const* per_query) { query_filters = per_query; }

    // scanner_simple::prepare_database (db_query.cpp:21-24) plus the quantizers the feeders need
    void prepare_database() {
        const int m = db.pq->sq_count, bits = db.pq->sq_bits;
        if (bits == 4 && (m == 16 || m == 32)) {
            prepare_nibbles(m);
            return;
        }
        if ((bits == 16 ? qadc_adc_index_create16(&index, m, device) : qadc_adc_index_create(&index, m, bits, device)) != QADC_OK)
            die("Cannot create the GPU index");
        if (qadc_adc_index_set_finish(index, finish) != QADC_OK) die("set_finish");
        if (qadc_adc_index_set_filter(index, filter) != QADC_OK) die("set_filter");
        const int part_count = db.partition_count();
        std::vector<const std::uint8_t*> codes(part_count);
        std::vector<const std::uint32_t*> labels(part_count);
        std::vector<std::uint32_t> sizes(part_count);
        bool labeled = false;
        for (int part_i = 0; part_i < part_count; ++part_i) {
            unsigned* lab;
            unsigned size;
            db.get_partition(part_i, codes[part_i], lab, size);
            labels[part_i] = lab;
            sizes[part_i] = size;
            labeled = labeled || lab != nullptr;
        }
        if (qadc_adc_index_add_partitions(index, part_count, codes.data(), labeled ? labels.data() : nullptr, sizes.data()) != QADC_OK)
            die("Cannot prepare database");
        if (qadc_adc_index_set_pq(index, db.pq->dim, db.pq->centroids.data()) != QADC_OK) die("Cannot set the codebooks");
        if (!db.pq->rotation.empty() && qadc_adc_index_set_rotation(index, db.pq->rotation.data()) != QADC_OK) die("Cannot set the rotation");
        if (db.coarse_count() > 0 && qadc_adc_index_set_coarse(index, db.coarse_count(), db.coarse_centroids()) != QADC_OK)
            die("Cannot set the coarse centroids");
    }

    void prepare_nibbles(int m) {
        if (qadc_index_create(&source, m, device) != QADC_OK) die("Cannot create the GPU index");
        const int part_count = db.partition_count();
        for (int part_i = 0; part_i < part_count; ++part_i) {
            const std::uint8_t* codes;
            unsigned* lab;
            unsigned size;
            db.get_partition(part_i, codes, lab, size);
            const std::uint32_t* labels = lab;
            const std::uint32_t sz = size;
            if (qadc_index_add_partitions(source, 1, &codes, lab ? &labels : nullptr, &sz) != QADC_OK) die("Cannot prepare database");
        }
        if (qadc_index_finalize(source, 0.01f) != QADC_OK) die("Cannot prepare database");
        if (qadc_index_set_pq(source, db.pq->dim, db.pq->centroids.data()) != QADC_OK) die("Cannot set the codebooks");
        if (!db.pq->rotation.empty() && qadc_index_set_rotation(source, db.pq->rotation.data()) != QADC_OK) die("Cannot set the rotation");
        if (db.coarse_count() > 0 && qadc_index_set_coarse(source, db.coarse_count(), db.coarse_centroids()) != QADC_OK)
            die("Cannot set the coarse centroids");
        if (qadc_adc_index_create_view(&index, source) != QADC_OK) die("Cannot create the view");
        if (qadc_adc_index_set_finish(index, finish) != QADC_OK) die("set_finish");
        if (qadc_adc_index_set_filter(index, filter) != QADC_OK) die("set_filter");
    }

    // the filters of the batch that opens at query_i (null: the plain call)
    const qadc_adc_filter* const* batch_filters(int query_i) const { return query_filters ? query_filters + query_i : nullptr; }

    // nns_engine_batch::process_query (query_common.hpp:194-243): the whole batch is searched when its first query is asked for
    template <typename Heap>
    void process_query(int query_i, const float* queries, int count, Heap& bh, query_metrics& metrics) {
        const int b = query_i % batch;
        metrics = query_metrics();
        const std::uint64_t t0 = ustime();
        if (finish == QADC_ADC_FINISH_DEVICE) {   // the heaps' arrays of the batch from the GPU (bh is empty, as the driver hands it over)
            if (b == 0) {
                const int nb = std::min(batch, count - query_i);
                if (cand_keys.size() < (std::size_t)batch * r) {
                    cand_keys.resize((std::size_t)batch * r);
                    cand_vals.resize((std::size_t)batch * r);
                }
                heap_sizes.resize(batch);
                if (qadc_adc_search_filtered(index, nb, queries + (std::size_t)query_i * db.pq->dim, ma, r, table_form, sum_mode, cand_keys.data(),
                                             cand_vals.data(), heap_sizes.data(), assign.data(), batch_filters(query_i)) != QADC_OK)
                    die("search");
            }
            for (std::int32_t i = 0; i < heap_sizes[b]; ++i) bh.push(cand_keys[(std::size_t)b * r + i], cand_vals[(std::size_t)b * r + i]);
            metrics.scan_us = ustime() - t0;
            return;
        }
        if (b == 0) {
            const int nb = std::min(batch, count - query_i);
            const float* q = queries + (std::size_t)query_i * db.pq->dim;
            int rc = qadc_adc_search_candidates_filtered(index, nb, q, ma, r, table_form, sum_mode, cand_keys.size(), cand_keys.data(),
                                                         cand_vals.data(), offsets.data(), assign.data(), batch_filters(query_i));
            if (rc == QADC_E_CAPACITY) {  // offsets[nb] holds the required size: grow and ask again
                cand_keys.resize(offsets[nb]);
                cand_vals.resize(offsets[nb]);
                rc = qadc_adc_search_candidates_filtered(index, nb, q, ma, r, table_form, sum_mode, cand_keys.size(), cand_keys.data(),
                                                         cand_vals.data(), offsets.data(), assign.data(), batch_filters(query_i));
            }
            if (rc != QADC_OK) die("search");
        }
        for (int t = 0; t < bh.capacity(); ++t) bh.push(0, std::numeric_limits<float>::max() - t);   // "Fill binary heap"
        for (std::uint64_t i = offsets[b]; i < offsets[b + 1]; ++i) bh.push(cand_keys[i], cand_vals[i]);
        metrics.scan_us = ustime() - t0;   // (index, rotation and tables are part of the one GPU call)
    }

    // Range search (qadc_adc_range_search): for queries [query_i, query_i + nq) of `queries`, every row of the
    // ma nearest partitions whose candidate is < radius[q] and whose key passes set_filter's filter and the query's own
    // (set_query_filters, indexed by query_i + q), ascending by (candidate, key).  lims [nq + 1]: query q's rows are
    // [lims[q], lims[q + 1]) of keys / values.  The batch size and R of the engine play no part.
    void range_search(int query_i, const float* queries, int nq, const float* radius, std::vector<std::uint64_t>& lims,
                      std::vector<std::uint32_t>& keys, std::vector<float>& values) {
        lims.assign((std::size_t)nq + 1, 0);
        std::vector<std::int32_t> probes((std::size_t)nq * ma);
        if (qadc_adc_range_search(index, nq, queries + (std::size_t)query_i * db.pq->dim, ma, radius, table_form, sum_mode, batch_filters(query_i),
                                  probes.data(), lims.data()) != QADC_OK)
            die("range_search");
        keys.resize(lims[nq]);
        values.resize(lims[nq]);
        if (qadc_adc_range_collect(index, lims[nq], keys.data(), values.data()) != QADC_OK) die("range_search");
    }
};

template <typename Db, typename Heap>
inline void call_engine(adc_search_engine_hip<Db>& e, int q, const float* queries, int count, int, Heap& bh, query_metrics& m) {
    e.process_query(q, queries, count, bh, m);
}

}  // namespace qadc
