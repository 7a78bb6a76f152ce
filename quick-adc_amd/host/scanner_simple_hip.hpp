// scanner_simple_hip — C++14 host mirror of the reference's plain ADC ScannerType on the GPU.
//
// scanner_simple (db_query.cpp:17-46) has three members: `typedef BhType`, `prepare_database(base_db&)` and
// `query_scan(query, assign, ma, tables, table_dim, bh, metrics)`.  This type has the same three, with the same argument
// meaning and error behaviour (get_scan_func's message + std::exit(1) for a configuration it does not take), and forwards to
// the float-ADC engine of include/qadc.h (qadc_adc_*): db_query.cpp drops it in by swapping the scanner type.
// Whole-byte codes ((4,8) (8,8) (16,8), and (2,16) (4,16) (8,16) through qadc_adc_index_create16) go into an ADC index of their
// own; 4-bit codes ((16,4) (32,4), scan_4<M>) go into a
// qadc_index — the database db_query_4's scanner_hip uses — and are scanned through a view of it (qadc_adc_index_create_view).
//   Db:   int partition_count(); void get_partition(int, const std::uint8_t*&, unsigned*&, unsigned&);
//         pq->sq_count, pq->sq_bits                                      (databases.hpp:34-63)
//   Heap: int capacity(); void push(unsigned, float)                     (kv_binheap<unsigned, float>, binheap.hpp)
// Sums are in the reference's grouping as compiled (sum_mode 1) unless the constructor is given 0 (source order).
// set_finish(QADC_ADC_FINISH_DEVICE): the heap is ordered and replayed on the GPU (qadc_adc_query_scan under
// qadc_adc_index_set_finish) and its arrays are pushed into the caller's empty heap in array order, which rebuilds them exactly
// (no entry of a heap's array exceeds its parent, so none moves); the default is the host finish, the candidate stream below.
// set_filter(f): the scans drop the rows whose key does not pass the qadc_adc_filter f (qadc_adc_index_set_filter).
// range_scan(...): every row below a radius instead of the R best (qadc_adc_range_scan).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <vector>

#include "../../include/qadc.h"
#include "qadc_heap.hpp"

namespace qadc {

struct no_simple_metrics {};

template <typename Db, typename Heap = kv_heap<unsigned, float>, typename Metrics = no_simple_metrics>
struct scanner_simple_hip {
    typedef Heap BhType;

    int device, sum_mode;
    int table_floats = 0;   // sq_count * 256, sq_count * 65536 for 16-bit codes, sq_count * 16 for 4-bit codes
    int finish = QADC_ADC_FINISH_HOST;
    qadc_adc_index* index;
    qadc_index* source = nullptr;   // 4-bit codes: the index that holds the database; `index` is a view of it
    std::vector<std::uint32_t> cand_keys;
    std::vector<float> cand_vals;

    explicit scanner_simple_hip(int device_ = 0, int sum_mode_ = 1) : device(device_), sum_mode(sum_mode_), index(nullptr) {}
    scanner_simple_hip(const scanner_simple_hip&) = delete;
    scanner_simple_hip& operator=(const scanner_simple_hip&) = delete;
    ~scanner_simple_hip() {
        qadc_adc_index_destroy(index);   // (the view first: its source refuses to go while it lives)
        qadc_index_destroy(source);
    }

    static void die(const char* what) {
        std::cerr << what << ": " << qadc_last_error() << std::endl;
        std::exit(1);
    }

    // qadc_adc_index_set_finish: before or after prepare_database
    void set_finish(int mode) {
        if (mode != QADC_ADC_FINISH_HOST && mode != QADC_ADC_FINISH_DEVICE) {
            std::cerr << "set_finish: mode is QADC_ADC_FINISH_HOST or QADC_ADC_FINISH_DEVICE" << std::endl;
            std::exit(1);
        }
        finish = mode;
        if (index && qadc_adc_index_set_finish(index, mode) != QADC_OK) die("set_finish");
    }

    // qadc_adc_index_set_filter: before or after prepare_database; null clears.  The filter is the caller's (qadc_adc_filter_create)
    // and must outlive the scanner or be cleared first; host/scanner_simple.hpp's key_filter is the CPU twin of what it does.
    const qadc_adc_filter* filter = nullptr;
    void set_filter(const qadc_adc_filter* f) {
        filter = f;
        if (index && qadc_adc_index_set_filter(index, f) != QADC_OK) die("set_filter");
    }

    // scanner_simple::prepare_database + get_scan_func (db_query.cpp:21-24, query_common.hpp:120-146)
    void prepare_database(Db& db) {
        const int m = db.pq->sq_count, bits = db.pq->sq_bits;
        const bool nibbles = bits == 4 && (m == 16 || m == 32);
        const bool bytes = bits == 8 && (m == 4 || m == 8 || m == 16);
        const bool words = bits == 16 && (m == 2 || m == 4 || m == 8);
        if (!nibbles && !bytes && !words) {   // get_scan_func's message
            std::cerr << "Unsupported (nsq,nsq_bits) configuration." << std::endl;
            std::cerr << "Supported configurations are: (16,4) (4,8) (8,8) (16,8) (2,16) (4,16) (8,16)." << std::endl;
            std::cerr << "This GPU scanner takes those and (32,4)." << std::endl;
            std::exit(1);
        }
        if (nibbles) {
            prepare_nibbles(db, m);
            return;
        }
        if ((words ? qadc_adc_index_create16(&index, m, device) : qadc_adc_index_create(&index, m, bits, device)) != QADC_OK)
            die("Cannot create the GPU index");
        if (qadc_adc_index_set_finish(index, finish) != QADC_OK) die("set_finish");
        if (qadc_adc_index_set_filter(index, filter) != QADC_OK) die("set_filter");
        table_floats = m * (words ? 65536 : 256);
        // every partition in one call (one upload of the partition table, one growth of the device copy)
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
    }

    // (16,4) and (32,4): the partitions go into a qadc_index, finalized (the pre-scan share is scanner_4's business: any keep
    // serves), and the scanner is a view of it
    void prepare_nibbles(Db& db, int m) {
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
        if (qadc_adc_index_create_view(&index, source) != QADC_OK) die("Cannot create the view");
        if (qadc_adc_index_set_finish(index, finish) != QADC_OK) die("set_finish");
        if (qadc_adc_index_set_filter(index, filter) != QADC_OK) die("set_filter");
        table_floats = m * 16;
    }

    // scanner_simple::query_scan (db_query.cpp:26-45).  `query` is unused there too; the tables of the ma probes follow each
    // other table_dim floats apart, which must be sq_count * 256 (sq_count * 65536 for 16-bit, sq_count * 16 for 4-bit codes: what
    // the engine reads).
    void query_scan(const float* /*query*/, int* assign, int ma, float* tables, int table_dim, BhType& bh, Metrics& /*metrics*/) {
        if (table_dim != table_floats) {
            std::cerr << "query_scan: table_dim " << table_dim << " is not " << table_floats << " (sq_count * centroids)" << std::endl;
            std::exit(1);
        }
        if (finish == QADC_ADC_FINISH_DEVICE) {   // the heap's arrays from the GPU (bh is empty, as the engines hand it over)
            const std::size_t r = (std::size_t)bh.capacity();
            if (cand_keys.size() < r) {
                cand_keys.resize(r);
                cand_vals.resize(r);
            }
            std::int32_t size = 0;
            if (qadc_adc_query_scan(index, 1, ma, assign, tables, bh.capacity(), sum_mode, cand_keys.data(), cand_vals.data(), &size) != QADC_OK)
                die("query_scan");
            for (std::int32_t i = 0; i < size; ++i) bh.push(cand_keys[i], cand_vals[i]);
            return;
        }
        std::uint64_t offsets[2] = {0, 0};
        if (cand_keys.empty()) {
            cand_keys.resize(1 << 16);
            cand_vals.resize(1 << 16);
        }
        int rc = qadc_adc_query_scan_candidates(index, 1, ma, assign, tables, bh.capacity(), sum_mode, cand_keys.size(),
                                                cand_keys.data(), cand_vals.data(), offsets);
        if (rc == QADC_E_CAPACITY) {  // offsets[1] holds the required size: grow and ask again
            cand_keys.resize(offsets[1]);
            cand_vals.resize(offsets[1]);
            rc = qadc_adc_query_scan_candidates(index, 1, ma, assign, tables, bh.capacity(), sum_mode, cand_keys.size(),
                                                cand_keys.data(), cand_vals.data(), offsets);
        }
        if (rc != QADC_OK) die("query_scan");
        for (int t = 0; t < bh.capacity(); ++t) bh.push(0, std::numeric_limits<float>::max() - t);   // "Fill binary heap"
        for (std::uint64_t i = offsets[0]; i < offsets[1]; ++i) bh.push(cand_keys[i], cand_vals[i]);
    }

    // scanner_simple::range_scan (host/scanner_simple.hpp) on the GPU: every row of the probed partitions whose
    // candidate is < radius and whose key passes set_filter's filter and `query_filter` (null: none), ascending by (candidate, key),
    // into keys / values (qadc_adc_range_scan, qadc_adc_range_collect).
    void range_scan(int* assign, int ma, float* tables, int table_dim, float radius, std::vector<std::uint32_t>& keys,
                    std::vector<float>& values, const qadc_adc_filter* query_filter = nullptr) {
        if (table_dim != table_floats) {
            std::cerr << "range_scan: table_dim " << table_dim << " is not " << table_floats << " (sq_count * centroids)" << std::endl;
            std::exit(1);
        }
        std::uint64_t lims[2] = {0, 0};
        if (qadc_adc_range_scan(index, 1, ma, assign, tables, &radius, sum_mode, query_filter ? &query_filter : nullptr, lims) != QADC_OK)
            die("range_scan");
        keys.resize(lims[1]);
        values.resize(lims[1]);
        if (qadc_adc_range_collect(index, lims[1], keys.data(), values.data()) != QADC_OK) die("range_scan");
    }
};

}  // namespace qadc
