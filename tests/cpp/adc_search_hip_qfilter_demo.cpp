// adc_search_engine_hip::set_query_filters (quick-adc_amd/host/adc_search_hip.hpp; qadc_adc_search_filtered)
// heap for heap against the CPU twin — nns_engine over scanner_simple with set_filter and, query by query, set_query_filter
// (host/scanner_simple.hpp), the written definition — on the same seeded database, which the host twin encodes.  The GPU engine is
// handed the query vectors and one filter per query.  C++14.
//   usage: adc_search_hip_qfilter_demo SQ_COUNT SQ_DIM N K MA NQ R BATCH SEED FINISH PERCENT
// K = 0: a flat database (keys are positions); K > 0: an IVF database of K partitions with labels.  Query q's own filter, by q % 4:
// none; EXCLUDE of a seeded PERCENT % of the keys (another set for every query); ALLOW of such a set; EXCLUDE of the keys of the
// query's unfiltered heap (the rows that won must be replaced by the next best).  Four rounds: no filter at all; the per-query
// filters; the same under an index-wide EXCLUDE (set_filter) of a seeded PERCENT %; everything cleared, which must bring the first
// round back.  Prints "ok <queries>" and exits 0 when every heap's arrays are identical in every round.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <vector>

#include "../../quick-adc_amd/host/adc_search_hip.hpp"
#include "../../quick-adc_amd/host/query_driver.hpp"
#include "../../quick-adc_amd/host/scanner_simple.hpp"

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

template <typename Db>
static int compare(Db& db, const std::vector<float>& vectors, unsigned n, const std::vector<float>& queries, int nq, int ma, int r, int batch,
                   std::uint64_t seed, int finish, int percent) {
    add_all(db, vectors, n);
    const int dim = db.pq->dim;
    scanner_simple<Db> cpu;
    nns_engine<Db, scanner_simple<Db>> ecpu(cpu, db, ma);
    adc_search_engine_hip<Db> egpu(db, ma, batch, r, 0, 1, 2);   // table_form 2: nns_engine's rule
    egpu.set_finish(finish);
    egpu.prepare_database();
    ecpu.prepare_database();

    std::vector<std::unique_ptr<key_filter>> twins(nq);         // query q's own filter on both sides; null: none
    std::vector<const qadc_adc_filter*> filters(nq, nullptr);
    std::vector<std::vector<unsigned>> winners(nq);               // the keys of every query's unfiltered heap
    int bad = 0;
    auto round = [&](const char* what, bool per_query, bool collect) {
        for (int q = 0; q < nq; ++q) {
            float_heap hc(r), hg(r);
            query_metrics mc, mg;
            cpu.set_query_filter(per_query ? twins[q].get() : nullptr);
            call_engine(ecpu, q, queries.data(), nq, dim, hc, mc);
            call_engine(egpu, q, queries.data(), nq, dim, hg, mg);
            const bool same = hc.size() == hg.size() && std::memcmp(hc.keys(), hg.keys(), sizeof(unsigned) * hc.size()) == 0 &&
                              std::memcmp(hc.values(), hg.values(), sizeof(float) * hc.size()) == 0;
            if (!same) {
                if (bad < 5) std::cerr << what << ", query " << q << ": heaps differ (sizes " << hc.size() << " / " << hg.size() << ")" << std::endl;
                ++bad;
            }
            if (collect) winners[q].assign(hc.keys(), hc.keys() + hc.size());
        }
    };
    round("no filter", false, true);
    for (int q = 0; q < nq; ++q) {
        if (q % 4 == 0) continue;
        const int mode = q % 4 == 2 ? QADC_ADC_FILTER_ALLOW : QADC_ADC_FILTER_EXCLUDE;
        const std::vector<unsigned> keys = q % 4 == 3 ? winners[q] : share(seed + 100 + 7919ull * q, n, percent);
        twins[q].reset(new key_filter(mode, keys.data(), keys.size()));
        filters[q] = gpu_filter(mode, keys);
    }
    egpu.set_query_filters(filters.data());
    round("per-query filters", true, false);
    const std::vector<unsigned> gone = share(seed + 50, n, percent);
    const key_filter twin_gone(key_filter::exclude, gone.data(), gone.size());
    qadc_adc_filter* f_gone = gpu_filter(QADC_ADC_FILTER_EXCLUDE, gone);
    cpu.set_filter(&twin_gone);
    egpu.set_filter(f_gone);
    round("per-query filters under an index-wide exclude", true, false);
    cpu.set_filter(nullptr);
    egpu.set_filter(nullptr);
    egpu.set_query_filters(nullptr);
    round("everything cleared", false, false);
    filters.push_back(f_gone);
    for (const qadc_adc_filter* f : filters)
        if (qadc_adc_filter_destroy(const_cast<qadc_adc_filter*>(f)) != QADC_OK) {
            std::cerr << "qadc_adc_filter_destroy: " << qadc_last_error() << std::endl;
            std::exit(1);
        }
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 12) {
        std::cerr << "usage: adc_search_hip_qfilter_demo SQ_COUNT SQ_DIM N K MA NQ R BATCH SEED FINISH PERCENT" << std::endl;
        return 2;
    }
    const int M = std::atoi(argv[1]), ds = std::atoi(argv[2]);
    const unsigned n = (unsigned)std::atol(argv[3]);
    const int K = std::atoi(argv[4]), ma = std::atoi(argv[5]), nq = std::atoi(argv[6]), r = std::atoi(argv[7]);
    const int batch = std::atoi(argv[8]);
    const std::uint64_t seed = std::strtoull(argv[9], nullptr, 10);
    const int finish = std::atoi(argv[10]), percent = std::atoi(argv[11]);
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
    if (K > 0) {
        ivf_database_t<pq_bytes> db(std::move(pq), K, coarse);
        bad = compare(db, vectors, n, queries, nq, ma, r, batch, seed, finish, percent);
    } else {
        flat_database_t<pq_bytes> db;
        db.pq = std::move(pq);
        bad = compare(db, vectors, n, queries, nq, ma, r, batch, seed, finish, percent);
    }
    if (bad) {
        std::cout << "FAIL " << bad << std::endl;
        return 1;
    }
    std::cout << "ok " << nq << std::endl;
    return 0;
}
