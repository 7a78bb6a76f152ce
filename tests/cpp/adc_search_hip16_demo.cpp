// adc_search_engine_hip (quick-adc_amd/host/adc_search_hip.hpp) on 16-bit codes — an index of qadc_adc_index_create16 — heap for
// heap against the CPU path it replaces: nns_engine over scanner_simple (scan_standard<uint16_t, NSQ>) with pq_bytes of 65536
// centroids per sub-quantizer (host/query_driver.hpp, host/scanner_simple.hpp) on the same seeded database, which the host twin
// encodes.  The GPU engine is handed the query vectors only.  C++14.
//   usage: adc_search_hip16_demo SQ_COUNT SQ_DIM N K MA NQ R BATCH OPQ FINISH SEED       (SQ_COUNT 2, 4 or 8; FINISH 0 host, 1 device)
// K = 0: a flat database; K > 0: an IVF database of K partitions with labels.  OPQ = 1: a seeded rotation (a product of plane
// rotations, so orthonormal up to rounding).  Prints "ok <queries>" and exits 0 when every heap's arrays are identical.
#include <cmath>
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

template <typename Db>
static int compare(Db& db, const std::vector<float>& vectors, unsigned n, const std::vector<float>& queries, int nq, int ma, int r, int batch,
                   int finish) {
    add_all(db, vectors, n);
    const int dim = db.pq->dim;
    scanner_simple<Db> cpu;
    nns_engine<Db, scanner_simple<Db>> ecpu(cpu, db, ma);
    adc_search_engine_hip<Db> egpu(db, ma, batch, r, 0, 1, 2);   // table_form 2: nns_engine's rule
    egpu.set_finish(finish);
    egpu.prepare_database();
    ecpu.prepare_database();
    int bad = 0;
    for (int q = 0; q < nq; ++q) {
        float_heap hc(r), hg(r);
        query_metrics mc, mg;
        call_engine(ecpu, q, queries.data(), nq, dim, hc, mc);
        call_engine(egpu, q, queries.data(), nq, dim, hg, mg);
        bool same = hc.size() == hg.size() && std::memcmp(hc.keys(), hg.keys(), sizeof(unsigned) * hc.size()) == 0 &&
                    std::memcmp(hc.values(), hg.values(), sizeof(float) * hc.size()) == 0;
        for (int a = 0; a < ma && same; ++a) same = egpu.assign[(std::size_t)(q % batch) * ma + a] == ecpu.assign[a];
        if (!same) {
            if (bad < 5) std::cerr << "query " << q << ": heaps or probes differ (sizes " << hc.size() << " / " << hg.size() << ")" << std::endl;
            ++bad;
        }
    }
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 12) {
        std::cerr << "usage: adc_search_hip16_demo SQ_COUNT SQ_DIM N K MA NQ R BATCH OPQ FINISH SEED" << std::endl;
        return 2;
    }
    const int M = std::atoi(argv[1]), ds = std::atoi(argv[2]);
    const unsigned n = (unsigned)std::atol(argv[3]);
    const int K = std::atoi(argv[4]), ma = std::atoi(argv[5]), nq = std::atoi(argv[6]), r = std::atoi(argv[7]);
    const int batch = std::atoi(argv[8]), opq = std::atoi(argv[9]), finish = std::atoi(argv[10]);
    const std::uint64_t seed = std::strtoull(argv[11], nullptr, 10);
    const int dim = M * ds;

    std::unique_ptr<pq_bytes> pq(new pq_bytes(M, 16, dim));
    for (std::size_t i = 0; i < pq->centroids.size(); ++i) pq->centroids[i] = unit(seed + 2, i) * 2.0f - 1.0f;
    if (opq) {
        pq->rotation.assign((std::size_t)dim * dim, 0.0f);
        for (int d = 0; d < dim; ++d) pq->rotation[(std::size_t)d * dim + d] = 1.0f;
        for (int k = 0; k < 4 * dim; ++k) {   // plane rotations of seeded pairs of rows
            const int i = (int)(splitmix64(seed + 5 + 2 * k) % dim), j = (int)(splitmix64(seed + 6 + 2 * k) % dim);
            if (i == j) continue;
            const float t = unit(seed + 7, k) * 6.2831853f, cs = std::cos(t), sn = std::sin(t);
            for (int c = 0; c < dim; ++c) {
                const float a = pq->rotation[(std::size_t)i * dim + c], b = pq->rotation[(std::size_t)j * dim + c];
                pq->rotation[(std::size_t)i * dim + c] = cs * a - sn * b;
                pq->rotation[(std::size_t)j * dim + c] = sn * a + cs * b;
            }
        }
    }
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
        bad = compare(db, vectors, n, queries, nq, ma, r, batch, finish);
    } else {
        flat_database_t<pq_bytes> db;
        db.pq = std::move(pq);
        bad = compare(db, vectors, n, queries, nq, ma, r, batch, finish);
    }
    if (bad) {
        std::cout << "FAIL " << bad << " of " << nq << std::endl;
        return 1;
    }
    std::cout << "ok " << nq << std::endl;
    return 0;
}
