// Range search through the C++14 mirrors beside the CPU twin: scanner_simple_hip::range_scan
// (quick-adc_amd/host/scanner_simple_hip.hpp; qadc_adc_range_scan) on the tables the host computes, and
// adc_search_engine_hip::range_search (quick-adc_amd/host/adc_search_hip.hpp; qadc_adc_range_search) from the query vectors, against
// scanner_simple::range_scan (host/scanner_simple.hpp), the written definition, on the same seeded database.  C++14.
//   usage: adc_range_hip_demo SQ_COUNT SQ_DIM N K MA NQ R SEED PERCENT
// K = 0: a flat database (keys are positions); K > 0: an IVF database of K partitions with labels.  Query q's radius is the largest
// value of its own R-heap (it keeps fewer than R rows), every third query +inf (every probed row), every fifth -inf (none).  Two
// rounds: no filter; an index-wide EXCLUDE of a seeded PERCENT % of the keys with, for odd queries, an ALLOW of another such set.
// Prints "ok <queries> <rows>" and exits 0 when keys and value bits of every query agree in every round on both mirrors.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <memory>
#include <vector>

#include "../../quick-adc_amd/host/adc_search_hip.hpp"
#include "../../quick-adc_amd/host/query_driver.hpp"
#include "../../quick-adc_amd/host/scanner_simple.hpp"
#include "../../quick-adc_amd/host/scanner_simple_hip.hpp"

using namespace qadc;

static std::uint64_t splitmix64(std::uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
static float unit(std::uint64_t seed, std::uint64_t i) { return (float)(splitmix64(seed ^ splitmix64(i)) >> 40) * (1.0f / 16777216.0f); }

static void add_all(flat_database_t<pq_bytes>& db, const std::vector<float>& v, unsigned n) { db.add_vectors(v.data(), n); }
static void add_all(ivf_database_t<pq_bytes>& db, const std::vector<float>& v, unsigned n) { db.add_vectors(v.data(), n, 0); }

static qadc_adc_filter* gpu_filter(int mode, const std::vector<unsigned>& keys) {
    qadc_adc_filter* f = nullptr;
    if (qadc_adc_filter_create(&f, mode, keys.data(), keys.size(), 0) != QADC_OK) {
        std::cerr << "qadc_adc_filter_create: " << qadc_last_error() << std::endl;
        std::exit(1);
    }
    return f;
}

static std::vector<unsigned> share(std::uint64_t seed, unsigned n, int percent) {
    std::vector<unsigned> keys;
    for (unsigned i = 0; i < n; ++i)
        if (splitmix64(seed + i) % 100 < (std::uint64_t)percent) keys.push_back(i);
    return keys;
}

static bool same(const range_result& want, const std::uint32_t* keys, const float* values, std::uint64_t rows) {
    return want.keys.size() == rows && (rows == 0 || (std::memcmp(want.keys.data(), keys, 4 * rows) == 0 &&
                                                      std::memcmp(want.values.data(), values, 4 * rows) == 0));
}

template <typename Db>
static int compare(Db& db, const std::vector<float>& vectors, unsigned n, const std::vector<float>& queries, int nq, int ma, int r,
                   std::uint64_t seed, int percent, std::uint64_t* rows_out) {
    add_all(db, vectors, n);
    const int dim = db.pq->dim, table_dim = db.pq->table_dim();
    scanner_simple<Db> cpu;
    cpu.prepare_database(db);
    scanner_simple_hip<Db> gpu;
    gpu.prepare_database(db);
    adc_search_engine_hip<Db> egpu(db, ma, nq, r, 0, 1, 2);   // table_form 2: nns_engine's rule, the tables computed below
    egpu.prepare_database();

    // what nns_engine::process_query computes in front of the scan: assign, residuals, rotation, tables
    std::vector<int> assign((std::size_t)nq * ma);
    std::vector<float> tables((std::size_t)nq * ma * table_dim), residuals((std::size_t)ma * dim), radius(nq);
    struct twin_metrics {} tm;
    for (int q = 0; q < nq; ++q) {
        int* a = assign.data() + (std::size_t)q * ma;
        float* t = tables.data() + (std::size_t)q * ma * table_dim;
        db.assign_compute_residuals(queries.data() + (std::size_t)q * dim, ma, a, residuals.data());
        db.pq->rotate_multiple_vectors(residuals.data(), ma);
        if (ma == 1) db.pq->tables_direct(residuals.data(), t);
        else db.pq->tables_blas(residuals.data(), ma, t);
        float_heap bh(r);
        cpu.query_scan(nullptr, a, ma, t, table_dim, bh, tm);
        radius[q] = q % 3 == 2 ? std::numeric_limits<float>::infinity() : q % 5 == 4 ? -std::numeric_limits<float>::infinity() : bh.values()[0];
    }

    std::vector<std::unique_ptr<key_filter>> twins(nq);
    std::vector<const qadc_adc_filter*> filters(nq, nullptr);
    int bad = 0;
    std::uint64_t rows = 0;
    auto round = [&](const char* what, bool per_query) {
        std::vector<range_result> want(nq);
        for (int q = 0; q < nq; ++q) {
            cpu.set_query_filter(per_query ? twins[q].get() : nullptr);
            cpu.range_scan(assign.data() + (std::size_t)q * ma, ma, tables.data() + (std::size_t)q * ma * table_dim, table_dim, radius[q], want[q]);
            rows += want[q].keys.size();
            std::vector<std::uint32_t> keys;
            std::vector<float> values;
            gpu.range_scan(assign.data() + (std::size_t)q * ma, ma, tables.data() + (std::size_t)q * ma * table_dim, table_dim, radius[q], keys,
                           values, per_query ? filters[q] : nullptr);
            if (!same(want[q], keys.data(), values.data(), keys.size())) {
                if (bad < 5) std::cerr << what << ", query " << q << ": scanner_simple_hip::range_scan differs (" << want[q].keys.size() << " / " << keys.size() << " rows)" << std::endl;
                ++bad;
            }
        }
        std::vector<std::uint64_t> lims;
        std::vector<std::uint32_t> keys;
        std::vector<float> values;
        egpu.set_query_filters(per_query ? filters.data() : nullptr);
        egpu.range_search(0, queries.data(), nq, radius.data(), lims, keys, values);
        for (int q = 0; q < nq; ++q)
            if (!same(want[q], keys.data() + lims[q], values.data() + lims[q], lims[q + 1] - lims[q])) {
                if (bad < 5) std::cerr << what << ", query " << q << ": adc_search_engine_hip::range_search differs (" << want[q].keys.size() << " / " << lims[q + 1] - lims[q] << " rows)" << std::endl;
                ++bad;
            }
    };
    round("no filter", false);
    for (int q = 1; q < nq; q += 2) {
        const std::vector<unsigned> keys = share(seed + 100 + 7919ull * q, n, 100 - percent);
        twins[q].reset(new key_filter(key_filter::allow, keys.data(), keys.size()));
        filters[q] = gpu_filter(QADC_ADC_FILTER_ALLOW, keys);
    }
    const std::vector<unsigned> gone = share(seed + 50, n, percent);
    const key_filter twin_gone(key_filter::exclude, gone.data(), gone.size());
    qadc_adc_filter* f_gone = gpu_filter(QADC_ADC_FILTER_EXCLUDE, gone);
    cpu.set_filter(&twin_gone);
    gpu.set_filter(f_gone);
    egpu.set_filter(f_gone);
    round("an index-wide exclude under per-query allows", true);
    gpu.set_filter(nullptr);
    egpu.set_filter(nullptr);
    filters.push_back(f_gone);
    for (const qadc_adc_filter* f : filters)
        if (qadc_adc_filter_destroy(const_cast<qadc_adc_filter*>(f)) != QADC_OK) {
            std::cerr << "qadc_adc_filter_destroy: " << qadc_last_error() << std::endl;
            std::exit(1);
        }
    *rows_out = rows;
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 10) {
        std::cerr << "usage: adc_range_hip_demo SQ_COUNT SQ_DIM N K MA NQ R SEED PERCENT" << std::endl;
        return 2;
    }
    const int M = std::atoi(argv[1]), ds = std::atoi(argv[2]);
    const unsigned n = (unsigned)std::atol(argv[3]);
    const int K = std::atoi(argv[4]), ma = std::atoi(argv[5]), nq = std::atoi(argv[6]), r = std::atoi(argv[7]);
    const std::uint64_t seed = std::strtoull(argv[8], nullptr, 10);
    const int percent = std::atoi(argv[9]);
    const int dim = M * ds;

    std::unique_ptr<pq_bytes> pq(new pq_bytes(M, 8, dim));
    for (std::size_t i = 0; i < pq->centroids.size(); ++i) pq->centroids[i] = unit(seed + 2, i) * 2.0f - 1.0f;
    const int centers = K > 0 ? K : 1;
    std::vector<float> coarse((std::size_t)centers * dim);
    for (std::size_t i = 0; i < coarse.size(); ++i) coarse[i] = K > 0 ? unit(seed + 8, i) * 8.0f - 4.0f : 0.0f;
    // vectors and queries around the centers; the last two centers get no vector (empty partitions)
    std::vector<float> vectors((std::size_t)n * dim), queries((std::size_t)nq * dim);
    for (unsigned i = 0; i < n; ++i) {
        const int c = (int)(splitmix64(seed + 9 + i) % (std::uint64_t)(centers > 2 ? centers - 2 : centers));
        for (int d = 0; d < dim; ++d) vectors[(std::size_t)i * dim + d] = coarse[(std::size_t)c * dim + d] + unit(seed + 1, (std::uint64_t)i * dim + d) * 2.0f - 1.0f;
    }
    for (int q = 0; q < nq; ++q) {
        const int c = (int)(splitmix64(seed + 10 + q) % (std::uint64_t)centers);
        for (int d = 0; d < dim; ++d) queries[(std::size_t)q * dim + d] = coarse[(std::size_t)c * dim + d] + unit(seed + 3, (std::uint64_t)q * dim + d) * 2.0f - 1.0f;
    }

    int bad;
    std::uint64_t rows = 0;
    if (K > 0) {
        ivf_database_t<pq_bytes> db(std::move(pq), K, coarse);
        bad = compare(db, vectors, n, queries, nq, ma, r, seed, percent, &rows);
    } else {
        flat_database_t<pq_bytes> db;
        db.pq = std::move(pq);
        bad = compare(db, vectors, n, queries, nq, ma, r, seed, percent, &rows);
    }
    if (bad) {
        std::cout << "FAIL " << bad << std::endl;
        return 1;
    }
    std::cout << "ok " << nq << " " << rows << std::endl;
    return 0;
}
