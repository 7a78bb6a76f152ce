// refine_store_hip and search_refined (quick-adc_amd/host/refine_hip.hpp) beside the host twin (host/refine.hpp) on the same seeded
// IVF database: the engine searches with heaps of R_IN entries, the store re-ranks them, and the twin re-ranks the same heaps on the
// CPU; keys, the distances' bits, sizes and the missing count must be identical, for a float and a half store.  C++14.
//   usage: refine_hip_demo BITS SQ_COUNT SQ_DIM N K MA NQ R R_IN SEED            (BITS 8: pq_bytes;  4: pq4 through a view, SQ_COUNT 16 or 32)
// The database is labelled from 0, so a key is the position of its vector.  The store is filled in three adds, and holds only the
// first N - N / 10 vectors: the candidates behind them are missing.  Prints "ok <queries>" and exits 0 when everything agrees.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <vector>

#include "../../quick-adc_amd/host/adc_search_hip.hpp"
#include "../../quick-adc_amd/host/query_driver.hpp"
#include "../../quick-adc_amd/host/refine.hpp"
#include "../../quick-adc_amd/host/refine_hip.hpp"
#include "../../quick-adc_amd/host/scanner_simple.hpp"

using namespace qadc;

static std::uint64_t splitmix64(std::uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
static float unit(std::uint64_t seed, std::uint64_t i) { return (float)(splitmix64(seed ^ splitmix64(i)) >> 40) * (1.0f / 16777216.0f); }

template <typename Pq>
static int compare(std::unique_ptr<Pq> pq, int K, const std::vector<float>& coarse, const std::vector<float>& vectors, unsigned n,
                   const std::vector<float>& queries, int nq, int ma, int r, int r_in) {
    const int dim = pq->dim;
    ivf_database_t<Pq> db(std::move(pq), K, coarse);
    db.add_vectors(vectors.data(), n, 0);
    adc_search_engine_hip<ivf_database_t<Pq>> engine(db, ma, nq, r_in, 0, 1, 2);
    engine.prepare_database();
    const unsigned held = n - n / 10, cut[4] = {0, held / 3, held / 3 + 1, held};
    int bad = 0;
    for (int dtype = QADC_REFINE_F32; dtype <= QADC_REFINE_F16; ++dtype) {
        refine_store_hip gpu(dim, dtype);
        refine::store cpu(dim, dtype);
        for (int a = 0; a < 3; ++a) {
            gpu.add(vectors.data() + (std::size_t)cut[a] * dim, cut[a + 1] - cut[a], cut[a]);
            if (!cpu.add(vectors.data() + (std::size_t)cut[a] * dim, cut[a + 1] - cut[a], cut[a])) return 1000;
        }
        if (gpu.rows() != held) return 1001;
        std::vector<std::uint32_t> keys;
        std::vector<float> vals;
        const refine_result got = search_refined(engine, gpu, nq, queries.data(), r, &keys, &vals);
        refine_result want;
        want.keys.resize((std::size_t)nq * r);
        want.dist.resize((std::size_t)nq * r);
        want.sizes.resize(nq);
        want.missing = refine::rerank(cpu, nq, queries.data(), r_in, keys.data(), nullptr, vals.data(), r, want.keys.data(), want.dist.data(),
                                      want.sizes.data());
        const bool same = got.missing == want.missing && got.sizes == want.sizes && got.keys == want.keys &&
                          std::memcmp(got.dist.data(), want.dist.data(), sizeof(float) * want.dist.size()) == 0;
        if (!same) {
            std::cerr << "dtype " << dtype << ": the store and the twin differ (missing " << got.missing << " / " << want.missing << ")" << std::endl;
            ++bad;
        }
        std::uint64_t found = 0;
        for (int q = 0; q < nq; ++q) found += (std::uint64_t)want.sizes[q];
        if (found == 0 || want.missing == 0) {
            std::cerr << "the case is vacuous: " << found << " survivors, " << want.missing << " missing" << std::endl;
            ++bad;
        }
    }
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 11) {
        std::cerr << "usage: refine_hip_demo BITS SQ_COUNT SQ_DIM N K MA NQ R R_IN SEED" << std::endl;
        return 2;
    }
    const int bits = std::atoi(argv[1]), M = std::atoi(argv[2]), ds = std::atoi(argv[3]);
    const unsigned n = (unsigned)std::atol(argv[4]);
    const int K = std::atoi(argv[5]), ma = std::atoi(argv[6]), nq = std::atoi(argv[7]), r = std::atoi(argv[8]), r_in = std::atoi(argv[9]);
    const std::uint64_t seed = std::strtoull(argv[10], nullptr, 10);
    const int dim = M * ds;
    if ((bits != 4 && bits != 8) || K < 1) return 2;

    std::vector<float> coarse((std::size_t)K * dim);
    for (std::size_t i = 0; i < coarse.size(); ++i) coarse[i] = unit(seed + 8, i) * 8.0f - 4.0f;
    std::vector<float> vectors((std::size_t)n * dim), queries((std::size_t)nq * dim);
    for (unsigned i = 0; i < n; ++i) {
        const int c = (int)(splitmix64(seed + 9 + i) % (std::uint64_t)K);
        for (int d = 0; d < dim; ++d) vectors[(std::size_t)i * dim + d] = coarse[(std::size_t)c * dim + d] + unit(seed + 1, (std::uint64_t)i * dim + d) * 2.0f - 1.0f;
    }
    for (int q = 0; q < nq; ++q) {
        const int c = (int)(splitmix64(seed + 10 + q) % (std::uint64_t)K);
        for (int d = 0; d < dim; ++d) queries[(std::size_t)q * dim + d] = coarse[(std::size_t)c * dim + d] + unit(seed + 3, (std::uint64_t)q * dim + d) * 2.0f - 1.0f;
    }

    int bad;
    if (bits == 8) {
        std::unique_ptr<pq_bytes> pq(new pq_bytes(M, 8, dim));
        for (std::size_t i = 0; i < pq->centroids.size(); ++i) pq->centroids[i] = unit(seed + 2, i) * 2.0f - 1.0f;
        bad = compare(std::move(pq), K, coarse, vectors, n, queries, nq, ma, r, r_in);
    } else {
        std::unique_ptr<pq4> pq(new pq4(M, dim));
        for (std::size_t i = 0; i < pq->centroids.size(); ++i) pq->centroids[i] = unit(seed + 2, i) * 2.0f - 1.0f;
        bad = compare(std::move(pq), K, coarse, vectors, n, queries, nq, ma, r, r_in);
    }
    if (bad) {
        std::cout << "FAIL " << bad << std::endl;
        return 1;
    }
    std::cout << "ok " << nq << std::endl;
    return 0;
}
