// scanner_simple_hip::set_filter (quick-adc_amd/host/scanner_simple_hip.hpp; qadc_adc_index_set_filter)
// under the query engine of host/query_driver.hpp, heap for heap against the CPU twin — scanner_simple with a key_filter
// (host/scanner_simple.hpp), the written definition — on the same seeded database, queries and tables.  C++14.
//   usage: scanner_simple_hip_filter_demo SQ_COUNT N K MA NQ R SEED FINISH MODE PERCENT
// K = 1: a flat database (no labels, ma must be 1: keys are positions); K > 1: N codes cut into K labeled partitions of uneven
// sizes, every query probing MA of them (duplicates allowed).  MODE 0 = exclude, 1 = allow.  Three rounds: no filter; a seeded
// PERCENT % of the keys; the keys of every query's unfiltered heap (exclude: the rows that won must be replaced by the next best,
// which a filter behind the bounds has discarded).  After the last round the filter is cleared and the first round must come back.
// Prints "ok <queries>" and exits 0 when every heap's arrays are identical in every round.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <vector>

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

// base_db's partition interface over whole-byte PQ codes; the coarse step is a seeded choice of partitions
struct parts_db {
    std::unique_ptr<pq_bytes> pq;
    std::vector<std::vector<std::uint8_t>> parts;
    std::vector<std::vector<unsigned>> labels;
    std::uint64_t seed = 0;
    int partition_count() const { return (int)parts.size(); }
    void get_partition(int i, const std::uint8_t*& c, unsigned*& l, unsigned& size) {
        c = parts[i].data();
        l = labels[i].empty() ? nullptr : labels[i].data();
        size = (unsigned)(parts[i].size() / pq->sq_count);
    }
    void assign_compute_residuals(const float* x, int ma, int* assign, float* residuals) const {
        std::uint32_t h;
        std::memcpy(&h, x, 4);
        for (int a = 0; a < ma; ++a) {
            assign[a] = (int)(splitmix64(seed + h + (std::uint64_t)a / 2) % parts.size());   // pairs of duplicate probes
            for (int d = 0; d < pq->dim; ++d) residuals[(std::size_t)a * pq->dim + d] = x[d] - 0.01f * (float)a;
        }
    }
};

int main(int argc, char** argv) {
    if (argc != 11) {
        std::cerr << "usage: scanner_simple_hip_filter_demo SQ_COUNT N K MA NQ R SEED FINISH MODE PERCENT" << std::endl;
        return 2;
    }
    const int M = std::atoi(argv[1]);
    const unsigned n = (unsigned)std::atol(argv[2]);
    const int K = std::atoi(argv[3]), ma = std::atoi(argv[4]), nq = std::atoi(argv[5]), r = std::atoi(argv[6]);
    const std::uint64_t seed = std::strtoull(argv[7], nullptr, 10);
    const int finish = std::atoi(argv[8]), mode = std::atoi(argv[9]), percent = std::atoi(argv[10]);
    const int dim = 4 * M;

    parts_db db;
    db.seed = seed;
    db.pq.reset(new pq_bytes(M, 8, dim));
    for (std::size_t i = 0; i < db.pq->centroids.size(); ++i) db.pq->centroids[i] = unit(seed + 2, i) * 4.0f - 2.0f;
    db.parts.resize(K);
    db.labels.resize(K);
    for (unsigned i = 0; i < n; ++i) {
        // uneven partitions: the square of a uniform picks the partition, so low ones are larger; the last one stays empty
        const float u = unit(seed + 3, i);
        const int p = K == 1 ? 0 : (int)(u * u * (float)(K - 1));
        for (int m = 0; m < M; ++m) db.parts[p].push_back((std::uint8_t)(splitmix64(seed + 4 + (std::uint64_t)i * M + m) & 0xff));
        if (K > 1) db.labels[p].push_back(i);
    }
    std::vector<float> queries((std::size_t)nq * dim);
    for (std::size_t i = 0; i < queries.size(); ++i) queries[i] = unit(seed + 1, i) * 4.0f - 2.0f;

    scanner_simple<parts_db> cpu;
    scanner_simple_hip<parts_db, float_heap, query_metrics> gpu;
    nns_engine<parts_db, scanner_simple<parts_db>> ecpu(cpu, db, ma);
    nns_engine<parts_db, scanner_simple_hip<parts_db, float_heap, query_metrics>> egpu(gpu, db, ma);
    gpu.set_finish(finish);
    egpu.prepare_database();
    ecpu.prepare_database();

    std::vector<unsigned> winners;   // the keys of every query's unfiltered heap
    int bad = 0;
    auto round = [&](const char* what, bool collect) {
        for (int q = 0; q < nq; ++q) {
            float_heap hc(r), hg(r);
            query_metrics mc, mg;
            call_engine(ecpu, q, queries.data(), nq, dim, hc, mc);
            call_engine(egpu, q, queries.data(), nq, dim, hg, mg);
            const bool same = hc.size() == hg.size() &&
                              std::memcmp(hc.keys(), hg.keys(), sizeof(unsigned) * hc.size()) == 0 &&
                              std::memcmp(hc.values(), hg.values(), sizeof(float) * hc.size()) == 0;
            if (!same) {
                if (bad < 5) std::cerr << what << ", query " << q << ": heaps differ (sizes " << hc.size() << " / " << hg.size() << ")" << std::endl;
                ++bad;
            }
            if (collect) winners.insert(winners.end(), hc.keys(), hc.keys() + hc.size());
        }
    };
    auto with_filter = [&](const char* what, const std::vector<unsigned>& keys) {
        const key_filter twin(mode, keys.data(), keys.size());
        qadc_adc_filter* f = nullptr;
        if (qadc_adc_filter_create(&f, mode, keys.data(), keys.size(), 0) != QADC_OK) {
            std::cerr << "qadc_adc_filter_create: " << qadc_last_error() << std::endl;
            std::exit(1);
        }
        cpu.set_filter(&twin);
        gpu.set_filter(f);
        round(what, false);
        cpu.set_filter(nullptr);
        gpu.set_filter(nullptr);
        if (qadc_adc_filter_destroy(f) != QADC_OK) {
            std::cerr << "qadc_adc_filter_destroy: " << qadc_last_error() << std::endl;
            std::exit(1);
        }
    };
    round("no filter", true);
    std::vector<unsigned> some;
    for (unsigned i = 0; i < n; ++i)
        if (splitmix64(seed + 9 + i) % 100 < (std::uint64_t)percent) some.push_back(i);
    with_filter("a seeded share of the keys", some);
    with_filter("the keys of the unfiltered heaps", winners);
    round("the filter cleared", false);
    if (bad) {
        std::cout << "FAIL " << bad << std::endl;
        return 1;
    }
    std::cout << "ok " << nq << std::endl;
    return 0;
}
