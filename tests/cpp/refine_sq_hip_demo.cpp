// refine_store_hip with SQ8 rows (quick-adc_amd/host/refine_hip.hpp) beside the host twin (host/refine.hpp)
// on seeded vectors: the range found on the GPU, a dense and a keyed store filled through the mirror, the rows read back, the clamp
// counter, a re-ranking and an exhaustive search; everything must equal the twin bit for bit.  C++14.
//   usage: refine_sq_hip_demo DIM N NQ R SEED
// The range is that of the first three quarters of the vectors, so that a few components of the rest are clamped.  Prints
// "ok <queries>" and exits 0 when everything agrees.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include "../../quick-adc_amd/host/refine.hpp"
#include "../../quick-adc_amd/host/refine_hip.hpp"

using namespace qadc;

static std::uint64_t splitmix64(std::uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
static float unit(std::uint64_t seed, std::uint64_t i) { return (float)(splitmix64(seed ^ splitmix64(i)) >> 40) * (1.0f / 16777216.0f); }

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(float) * a.size()) == 0;
}

template <typename Twin>
static int compare(refine_store_hip& gpu, const Twin& cpu, const std::vector<std::uint32_t>& keys, int nq, const std::vector<float>& queries, int r) {
    int bad = 0;
    const int dim = gpu.dim;
    // read-back: every key held, one that is not, and the filler key
    std::vector<std::uint32_t> ask(keys);
    ask.push_back(0xFFFFFFF0u);
    ask.push_back(0xFFFFFFFFu);
    std::vector<std::uint8_t> found, want_found(ask.size());
    const std::vector<float> rows = gpu.get(ask.data(), ask.size(), &found);
    std::vector<float> want_rows(ask.size() * dim);
    refine::get(cpu, ask.data(), ask.size(), want_rows.data(), want_found.data());
    if (!same_bits(rows, want_rows) || found != want_found) {
        std::cerr << "get differs from the twin" << std::endl;
        ++bad;
    }
    if (gpu.sq_info() != cpu.sq.clamped || cpu.sq.clamped == 0) {
        std::cerr << "clamped: " << gpu.sq_info() << " / " << cpu.sq.clamped << std::endl;
        ++bad;
    }
    // every key as every query's candidates, then the exhaustive search: the same words
    const int r_in = (int)ask.size();
    std::vector<std::uint32_t> cand((std::size_t)nq * r_in);
    for (int q = 0; q < nq; ++q) std::memcpy(cand.data() + (std::size_t)q * r_in, ask.data(), sizeof(std::uint32_t) * r_in);
    const refine_result got = gpu.rerank(nq, queries.data(), r_in, cand.data(), nullptr, nullptr, r);
    const refine_result all = gpu.knn(nq, queries.data(), r);
    refine_result want;
    want.keys.resize((std::size_t)nq * r);
    want.dist.resize((std::size_t)nq * r);
    want.sizes.resize(nq);
    want.missing = refine::rerank(cpu, nq, queries.data(), r_in, cand.data(), nullptr, nullptr, r, want.keys.data(), want.dist.data(), want.sizes.data());
    if (got.missing != want.missing || want.missing != 2u * nq || got.sizes != want.sizes || got.keys != want.keys || !same_bits(got.dist, want.dist)) {
        std::cerr << "rerank differs from the twin" << std::endl;
        ++bad;
    }
    if (all.sizes != want.sizes || all.keys != want.keys || !same_bits(all.dist, want.dist)) {
        std::cerr << "knn differs from the twin" << std::endl;
        ++bad;
    }
    return bad;
}

int main(int argc, char** argv) {
    if (argc != 6) {
        std::cerr << "usage: refine_sq_hip_demo DIM N NQ R SEED" << std::endl;
        return 2;
    }
    const int dim = std::atoi(argv[1]), nq = std::atoi(argv[3]), r = std::atoi(argv[4]);
    const unsigned n = (unsigned)std::atol(argv[2]);
    const std::uint64_t seed = std::strtoull(argv[5], nullptr, 10);
    if (dim < 1 || n < 8 || nq < 1 || r < 1) return 2;
    std::vector<float> vectors((std::size_t)n * dim), queries((std::size_t)nq * dim);
    for (std::size_t i = 0; i < vectors.size(); ++i) vectors[i] = unit(seed + 1, i) * unit(seed + 2, i) * 8.0f - 2.0f;
    for (std::size_t i = 0; i < queries.size(); ++i) queries[i] = unit(seed + 3, i) * 6.0f - 2.0f;

    // the range: the GPU's equals the twin's
    const unsigned learn = n - n / 4;
    std::vector<float> vmin(dim), step(dim), vmin_cpu(dim), step_cpu(dim);
    if (qadc_refine_sq_range_host(vectors.data(), learn, dim, 0, vmin.data(), step.data()) != QADC_OK) refine_store_hip::die("sq_range");
    refine::sq_range(vectors.data(), learn, dim, vmin_cpu.data(), step_cpu.data());
    int bad = 0;
    if (!same_bits(vmin, vmin_cpu) || !same_bits(step, step_cpu)) {
        std::cerr << "the range differs from the twin" << std::endl;
        ++bad;
    }

    std::vector<std::uint32_t> dense_keys(n), labels(n);
    for (unsigned i = 0; i < n; ++i) {
        dense_keys[i] = 100 + i;
        labels[i] = 7 + 3 * (std::uint32_t)((i * 2654435761u) % n);   // (a permutation where n is odd or a power of two; else keys repeat: the last wins)
    }
    {
        refine_store_hip gpu(dim, vmin.data(), step.data());
        refine::store cpu(dim, vmin.data(), step.data());
        gpu.add(vectors.data(), n / 2, 100);
        gpu.add(vectors.data() + (std::size_t)(n / 2) * dim, n - n / 2, 100 + n / 2);
        if (!cpu.add(vectors.data(), n, 100)) return 3;
        bad += compare(gpu, cpu, dense_keys, nq, queries, r);
    }
    {
        refine_store_hip gpu(dim, vmin.data(), step.data(), 0, true);
        refine::keyed_store cpu(dim, vmin.data(), step.data());
        gpu.put(vectors.data(), labels.data(), n);
        if (!cpu.put(vectors.data(), labels.data(), n)) return 3;
        const std::uint32_t gone[2] = {labels[1], labels[2]};
        if (gpu.remove(gone, 2) != cpu.remove(gone, 2)) ++bad;
        bad += compare(gpu, cpu, cpu.held_keys(), nq, queries, r);
    }
    if (bad) {
        std::cout << "FAIL " << bad << std::endl;
        return 1;
    }
    std::cout << "ok " << nq << std::endl;
    return 0;
}
