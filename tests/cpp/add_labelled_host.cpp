// TEST DRIVER (CPU only): the labelled add_vectors overload of the host twin (ivf_database_t::add_vectors(vecs, labels, n),
// host/query_driver.hpp) against the plain one with its labels mapped — the definition of qadc_adc_index_add_vectors_labelled and
// qadc_index_add_vectors_labelled.  Over pq_bytes (8-bit codes) and pq4 (4-bit codes), in two calls each, the second with a
// labels_offset on the plain side.  The labels repeat and hold 0 and 0xFFFFFFFF.  Prints "ok", or what differs.  C++14, header only.
//   usage: add_labelled_host
#include <cstdint>
#include <iostream>
#include <memory>
#include <vector>

#include "../../quick-adc_amd/host/query_driver.hpp"
#include "../../quick-adc_amd/host/scanner_simple.hpp"

using namespace qadc;

static std::uint64_t state = 0x9E3779B97F4A7C15ull;
static std::uint32_t next32() {                                  // splitmix64, upper half
    std::uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (std::uint32_t)((z ^ (z >> 31)) >> 32);
}
static float unit() { return (float)(next32() >> 8) / 16777216.0f * 2.0f - 1.0f; }

template <typename Pq>
static int run(std::unique_ptr<Pq> a, std::unique_ptr<Pq> b, const char* what) {
    const int dim = a->dim, K = 5;
    const unsigned n = 500, first = 200;
    for (float& c : a->centroids) c = unit();
    b->centroids = a->centroids;
    std::vector<float> coarse((std::size_t)K * dim), vectors((std::size_t)n * dim);
    for (float& c : coarse) c = 3.0f * unit();
    for (unsigned i = 0; i < n; ++i)
        for (int d = 0; d < dim; ++d) vectors[(std::size_t)i * dim + d] = coarse[(std::size_t)(next32() % K) * dim + d] + unit();
    std::vector<unsigned> lab(n);
    for (unsigned& l : lab) l = next32();
    lab[0] = 0xFFFFFFFFu;
    lab[7] = 0;
    lab[first] = lab[first - 1];                                 // a label on either side of the two calls
    for (unsigned i = 300; i < 320; ++i) lab[i] = lab[i - 300 + 20];

    ivf_database_t<Pq> plain(std::move(a), K, coarse), labelled(std::move(b), K, coarse);
    plain.add_vectors(vectors.data(), first, 0);
    plain.add_vectors(vectors.data() + (std::size_t)first * dim, n - first, first);
    labelled.add_vectors(vectors.data(), lab.data(), first);
    labelled.add_vectors(vectors.data() + (std::size_t)first * dim, lab.data() + first, n - first);

    std::size_t rows = 0;
    for (int p = 0; p < K; ++p) {
        if (plain.partitions[p] != labelled.partitions[p]) {
            std::cout << what << ": the codes of partition " << p << " differ" << std::endl;
            return 1;
        }
        if (plain.labels[p].size() != labelled.labels[p].size()) {
            std::cout << what << ": partition " << p << " holds another number of labels" << std::endl;
            return 1;
        }
        for (std::size_t j = 0; j < plain.labels[p].size(); ++j)
            if (labelled.labels[p][j] != lab[plain.labels[p][j]]) {
                std::cout << what << ": partition " << p << " row " << j << " carries label " << labelled.labels[p][j] << ", expected "
                          << lab[plain.labels[p][j]] << std::endl;
                return 1;
            }
        rows += plain.labels[p].size();
    }
    if (rows != n) {
        std::cout << what << ": " << rows << " rows, expected " << n << std::endl;
        return 1;
    }
    return 0;
}

int main() {
    if (run(std::unique_ptr<pq_bytes>(new pq_bytes(4, 8, 8)), std::unique_ptr<pq_bytes>(new pq_bytes(4, 8, 8)), "pq_bytes 4x8")) return 1;
    if (run(std::unique_ptr<pq4>(new pq4(16, 32)), std::unique_ptr<pq4>(new pq4(16, 32)), "pq4 16x4")) return 1;
    std::cout << "ok" << std::endl;
    return 0;
}
