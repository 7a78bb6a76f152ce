// An index under the caller's own labels and a keyed refine store (quick-adc_amd/host/refine_hip.hpp, include/qadc.h; DESIGN.md
// sections 11.5 and 11.14) beside the host twins (ivf_database_t::add_vectors with labels, refine::keyed_store) on a seeded IVF
// database with random labels.  C++14.
//   usage: refine_keyed_hip_demo SQ_COUNT SQ_DIM N K MA NQ R R_IN SEED            (8-bit sub-quantizers)
// The life: the first half of the vectors goes through the host twin's labelled add and the engine's upload, the second half through
// qadc_adc_index_add_vectors_labelled on the GPU (and the twin, which must agree: the partitions are read back); put of all labels;
// search_refined; a third of the labels removed from the index, the store and the twin store; search_refined; a put that overwrites
// a tenth of the held labels with other vectors; search_refined.  After every search the store's result and the twin's rerank of the
// same heaps must be identical: keys, the distances' bits, sizes, the missing count.  Prints "ok <queries>" and exits 0.
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

typedef ivf_database_t<pq_bytes> Db;

// one refined search on the GPU and its twin; 0 where they agree.  *found += the survivors, *missing += the missing entries
static int search_both(adc_search_engine_hip<Db>& engine, refine_store_hip& gpu, const refine::keyed_store& cpu, const std::vector<float>& queries,
                       int nq, int r, int r_in, const char* what, std::uint64_t* found, std::uint64_t* missing, std::vector<std::uint32_t>* first) {
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
        std::cerr << what << ": the store and the twin differ (missing " << got.missing << " / " << want.missing << ")" << std::endl;
        return 1;
    }
    for (int q = 0; q < nq; ++q) *found += (std::uint64_t)want.sizes[q];
    *missing += want.missing;
    if (first) {
        first->clear();
        for (int q = 0; q < nq; ++q)
            if (want.sizes[q]) first->push_back(want.keys[(std::size_t)q * r]);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 10) {
        std::cerr << "usage: refine_keyed_hip_demo SQ_COUNT SQ_DIM N K MA NQ R R_IN SEED" << std::endl;
        return 2;
    }
    const int M = std::atoi(argv[1]), ds = std::atoi(argv[2]);
    const unsigned n = (unsigned)std::atol(argv[3]);
    const int K = std::atoi(argv[4]), ma = std::atoi(argv[5]), nq = std::atoi(argv[6]), r = std::atoi(argv[7]), r_in = std::atoi(argv[8]);
    const std::uint64_t seed = std::strtoull(argv[9], nullptr, 10);
    const int dim = M * ds;
    if (K < 1 || n < 20) return 2;

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
    // random labels, injective: an odd multiplier permutes the 32-bit values; never the filler key
    std::vector<std::uint32_t> labels(n);
    const std::uint32_t mul = (std::uint32_t)splitmix64(seed + 20) | 1u, add = (std::uint32_t)splitmix64(seed + 21);
    for (unsigned i = 0; i < n; ++i) {
        labels[i] = i * mul + add;
        if (labels[i] == 0xFFFFFFFFu) return 2;
    }

    std::unique_ptr<pq_bytes> pq(new pq_bytes(M, 8, dim));
    for (std::size_t i = 0; i < pq->centroids.size(); ++i) pq->centroids[i] = unit(seed + 2, i) * 2.0f - 1.0f;
    Db db(std::move(pq), K, coarse);
    const unsigned half = n / 2;
    db.add_vectors(vectors.data(), labels.data(), half);                                   // the twin's labelled add
    adc_search_engine_hip<Db> engine(db, ma, nq, r_in, 0, 1, 2);
    engine.prepare_database();
    if (qadc_adc_index_add_vectors_labelled(engine.index, vectors.data() + (std::size_t)half * dim, labels.data() + half, n - half, 1) != QADC_OK) {
        std::cerr << "qadc_adc_index_add_vectors_labelled: " << qadc_last_error() << std::endl;
        return 1;
    }
    db.add_vectors(vectors.data() + (std::size_t)half * dim, labels.data() + half, n - half);
    int bad = 0;
    for (int p = 0; p < K; ++p) {                                                          // the GPU's partitions are the twin's
        const std::uint32_t size = qadc_adc_index_partition_size(engine.index, p);
        std::vector<std::uint8_t> codes((std::size_t)size * M);
        std::vector<std::uint32_t> lab(size);
        if (size != db.labels[p].size() || qadc_adc_index_read_partition(engine.index, p, 0, size, codes.data(), lab.data()) != QADC_OK ||
            codes != db.partitions[p] || !std::equal(lab.begin(), lab.end(), db.labels[p].begin())) {
            std::cerr << "partition " << p << " differs from the twin's" << std::endl;
            ++bad;
        }
    }

    for (int dtype = QADC_REFINE_F32; dtype <= QADC_REFINE_F16 && !bad; ++dtype) {
        refine_store_hip gpu(dim, dtype, 0, true);
        refine::keyed_store cpu(dim, dtype);
        gpu.put(vectors.data(), labels.data(), n);
        if (!cpu.put(vectors.data(), labels.data(), n) || gpu.rows() != n) return 1000;
        std::uint64_t found = 0, missing = 0, none = 0;
        std::vector<std::uint32_t> best;
        bad += search_both(engine, gpu, cpu, queries, nq, r, r_in, "after the build", &found, &missing, &best);
        if (missing) {
            std::cerr << "dtype " << dtype << ": " << missing << " keys missing while the index and the store hold the same labels" << std::endl;
            ++bad;
        }
        // a tenth of the labels, and every query's best, leave the store (the index keeps them: they are missing afterwards)
        std::vector<std::uint32_t> gone(best);
        for (unsigned i = 0; i < n; i += 10) gone.push_back(labels[i]);
        gone.push_back(labels[0]);                                                         // (listed twice: counts once)
        const std::uint64_t removed = gpu.remove(gone.data(), gone.size());
        if (removed != cpu.remove(gone.data(), gone.size()) || removed == 0 || gpu.rows() != cpu.live()) {
            std::cerr << "dtype " << dtype << ": remove differs from the twin's" << std::endl;
            ++bad;
        }
        bad += search_both(engine, gpu, cpu, queries, nq, r, r_in, "after the removal", &found, &missing, nullptr);
        if (missing == 0) {
            std::cerr << "the case is vacuous: nothing is missing after the removal" << std::endl;
            ++bad;
        }
        // a put that overwrites: every fifth label gets the vector of its neighbour; a fifth of the removed ones come back with it
        std::vector<std::uint32_t> lab2;
        std::vector<float> vec2;
        for (unsigned i = 0; i < n; i += 5) {
            lab2.push_back(labels[i]);
            const float* v = vectors.data() + (std::size_t)((i + 1) % n) * dim;
            vec2.insert(vec2.end(), v, v + dim);
        }
        gpu.put(vec2.data(), lab2.data(), lab2.size());
        if (!cpu.put(vec2.data(), lab2.data(), lab2.size()) || gpu.rows() != cpu.live()) return 1001;
        bad += search_both(engine, gpu, cpu, queries, nq, r, r_in, "after the overwrite", &found, &none, nullptr);
        if (found == 0) {
            std::cerr << "the case is vacuous: no survivors" << std::endl;
            ++bad;
        }
    }
    // the index follows: the removed labels leave it too, and nothing the store lacks is asked for any more
    if (!bad) {
        std::vector<std::uint32_t> gone;
        for (unsigned i = 0; i < n; i += 3) gone.push_back(labels[i]);
        std::uint64_t removed = 0;
        if (qadc_adc_index_remove_labels(engine.index, gone.data(), gone.size(), &removed) != QADC_OK || removed != gone.size()) {
            std::cerr << "qadc_adc_index_remove_labels: " << removed << " of " << gone.size() << " rows: " << qadc_last_error() << std::endl;
            ++bad;
        }
        refine_store_hip gpu(dim, QADC_REFINE_F32, 0, true);
        refine::keyed_store cpu(dim, QADC_REFINE_F32);
        gpu.put(vectors.data(), labels.data(), n);
        cpu.put(vectors.data(), labels.data(), n);
        if (gpu.remove(gone.data(), gone.size()) != cpu.remove(gone.data(), gone.size())) ++bad;
        std::uint64_t found = 0, missing = 0;
        bad += search_both(engine, gpu, cpu, queries, nq, r, r_in, "after remove_labels", &found, &missing, nullptr);
        if (missing || !found) {
            std::cerr << "after remove_labels: " << missing << " missing, " << found << " survivors" << std::endl;
            ++bad;
        }
    }
    if (bad) {
        std::cout << "FAIL " << bad << std::endl;
        return 1;
    }
    std::cout << "ok " << nq << std::endl;
    return 0;
}
