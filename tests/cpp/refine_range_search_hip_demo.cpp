// range_search_refined (quick-adc_amd/host/refine_hip.hpp) — adc_search_engine_hip::range_search, then
// refine_store_hip::rerank_range on its rows — beside the host twin refine::rerank_range (host/refine.hpp) on the same seeded IVF
// database: lims, keys, the distances' bits and the missing count must be identical, for a float and a half store.  C++14.
//   usage: refine_range_search_hip_demo BITS SQ_COUNT SQ_DIM N K MA NQ SEED        (BITS 8: pq_bytes;  4: pq4 through a view, SQ_COUNT 16 or 32)
// The database is labelled from 0, so a key is the position of its vector.  The store holds only the first N - N / 10 vectors: the
// ADC rows behind them are missing.  The ADC radius of query q is the median ADC value of its probed rows (+inf for every third
// query: every probed row); the exact radius is the twin's distance of the row a third of the way into the query's candidates by
// (distance, key), so that a part of them is kept and the row at the radius itself is not.  Prints "ok <queries> <rows>" and exits 0
// when everything agrees.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
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
                   const std::vector<float>& queries, int nq, int ma, std::uint64_t* rows_out) {
    const int dim = pq->dim;
    ivf_database_t<Pq> db(std::move(pq), K, coarse);
    db.add_vectors(vectors.data(), n, 0);
    adc_search_engine_hip<ivf_database_t<Pq>> engine(db, ma, nq, 100, 0, 1, 2);
    engine.prepare_database();

    // the ADC radii: from the engine's own range search under +inf
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> adc_radius(nq, inf);
    {
        std::vector<std::uint64_t> lims;
        std::vector<std::uint32_t> keys;
        std::vector<float> values;
        engine.range_search(0, queries.data(), nq, adc_radius.data(), lims, keys, values);
        for (int q = 0; q < nq; ++q)
            if (q % 3 != 2 && lims[q + 1] > lims[q]) adc_radius[q] = values[(lims[q] + lims[q + 1]) / 2];   // (sorted by value: the median)
    }

    const unsigned held = n - n / 10;
    int bad = 0;
    for (int dtype = QADC_REFINE_F32; dtype <= QADC_REFINE_F16; ++dtype) {
        refine_store_hip gpu(dim, dtype);
        refine::store cpu(dim, dtype);
        gpu.add(vectors.data(), held, 0);
        if (!cpu.add(vectors.data(), held, 0)) return 1000;

        // the exact radii: from the twin under +inf on the rows the engine returns
        std::vector<std::uint64_t> lims, wl;
        std::vector<std::uint32_t> keys, wk;
        std::vector<float> values, wd, radius(nq, inf);
        engine.range_search(0, queries.data(), nq, adc_radius.data(), lims, keys, values);
        refine::rerank_range(cpu, nq, queries.data(), lims.data(), keys.data(), radius.data(), wl, wk, wd);
        for (int q = 0; q < nq; ++q)
            if (wl[q + 1] > wl[q]) radius[q] = wd[wl[q] + (wl[q + 1] - wl[q]) / 3];

        std::vector<std::uint64_t> adc_lims;
        std::vector<std::uint32_t> adc_keys;
        const refine_range_result got = range_search_refined(engine, gpu, 0, queries.data(), nq, adc_radius.data(), radius.data(), &adc_lims, &adc_keys);
        if (adc_lims != lims || adc_keys != keys) {
            std::cerr << "dtype " << dtype << ": the ADC result handed back differs from range_search's" << std::endl;
            ++bad;
        }
        const std::uint64_t missing = refine::rerank_range(cpu, nq, queries.data(), lims.data(), keys.data(), radius.data(), wl, wk, wd);
        const bool same = got.missing == missing && got.lims == wl && got.keys == wk && got.dist.size() == wd.size() &&
                          (wd.empty() || std::memcmp(got.dist.data(), wd.data(), sizeof(float) * wd.size()) == 0);
        if (!same) {
            std::cerr << "dtype " << dtype << ": the composition and the twin differ (missing " << got.missing << " / " << missing << ", rows "
                      << got.keys.size() << " / " << wk.size() << ")" << std::endl;
            ++bad;
        }
        if (wk.empty() || missing == 0 || wk.size() >= keys.size()) {
            std::cerr << "the case is vacuous: " << wk.size() << " rows kept of " << keys.size() << ", " << missing << " missing" << std::endl;
            ++bad;
        }
        *rows_out = wk.size();
    }
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 9) {
        std::cerr << "usage: refine_range_search_hip_demo BITS SQ_COUNT SQ_DIM N K MA NQ SEED" << std::endl;
        return 2;
    }
    const int bits = std::atoi(argv[1]), M = std::atoi(argv[2]), ds = std::atoi(argv[3]);
    const unsigned n = (unsigned)std::atol(argv[4]);
    const int K = std::atoi(argv[5]), ma = std::atoi(argv[6]), nq = std::atoi(argv[7]);
    const std::uint64_t seed = std::strtoull(argv[8], nullptr, 10);
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
    std::uint64_t rows = 0;
    if (bits == 8) {
        std::unique_ptr<pq_bytes> pq(new pq_bytes(M, 8, dim));
        for (std::size_t i = 0; i < pq->centroids.size(); ++i) pq->centroids[i] = unit(seed + 2, i) * 2.0f - 1.0f;
        bad = compare(std::move(pq), K, coarse, vectors, n, queries, nq, ma, &rows);
    } else {
        std::unique_ptr<pq4> pq(new pq4(M, dim));
        for (std::size_t i = 0; i < pq->centroids.size(); ++i) pq->centroids[i] = unit(seed + 2, i) * 2.0f - 1.0f;
        bad = compare(std::move(pq), K, coarse, vectors, n, queries, nq, ma, &rows);
    }
    if (bad) {
        std::cout << "FAIL " << bad << std::endl;
        return 1;
    }
    std::cout << "ok " << nq << " " << rows << std::endl;
    return 0;
}
