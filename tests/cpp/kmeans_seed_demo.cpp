// From a learning set to a coarse quantizer and a product quantizer with no caller-made seed, from C++14 (host/db_build.hpp:
// learn_coarse_quantizer_hip and learn_pq_hip with a std::uint64_t seed): reads a learning set (.fvecs / .bvecs), seeds K coarse
// centroids by k-means++ on the GPU and runs the k-means rounds, then seeds and learns the product quantizer of the residuals to them
// and writes the .pq.data file the reference's executables read.  Then reads the file back through pq_from_data_file and writes the
// coarse centroids and the centroids the file holds as raw floats (tests/test_gpu_kmeans_seed_train.py compares them with the
// Python route).
//   kmeans_seed_demo <learn file> <K> <sq_count> <sq_bits> <iters> <seed> <out.pq.data> <readback>
// stdout: "seeded dim=<dim> K=<K> m=<sq_count> b=<sq_bits> n=<vectors> empty=<NaN centroids>".
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "../../quick-adc_amd/host/db_build.hpp"

int main(int argc, char** argv) {
    if (argc != 9) {
        std::fprintf(stderr, "usage: %s <learn file> <K> <sq_count> <sq_bits> <iters> <seed> <out.pq.data> <readback>\n", argv[0]);
        return 2;
    }
    try {
        const qadc::io::vectors_owner<float> learn = qadc::io::load_vectors_by_extension(argv[1]);
        const int dim = learn.dimension, K = std::atoi(argv[2]), sq_count = std::atoi(argv[3]), sq_bits = std::atoi(argv[4]);
        const int iters = std::atoi(argv[5]);
        const std::uint64_t seed = std::strtoull(argv[6], nullptr, 10);
        const size_t n = (size_t)learn.count;
        if (K <= 0 || sq_count <= 0 || dim % sq_count || sq_bits <= 0 || sq_bits > 16 || n < ((size_t)1 << sq_bits) || n < (size_t)K)
            throw std::runtime_error("the learning set does not fit the quantizers' shapes");
        if (qadc::io::data_filename_is_opq(argv[7])) throw std::runtime_error("the output must end with .pq.data");
        const std::vector<float> coarse = qadc::learn_coarse_quantizer_hip(learn.data.data(), n, dim, K, seed);
        std::uint64_t empty = 0;
        const qadc::io::pq_data pq = qadc::learn_pq_hip(learn.data.data(), n, dim, sq_count, sq_bits, seed, iters, K, coarse.data(), nullptr, 0, &empty);
        qadc::io::pq_to_data_file(pq, argv[7]);
        const qadc::io::pq_data back = qadc::io::pq_from_data_file(argv[7]);
        FILE* out = std::fopen(argv[8], "wb");
        if (!out || std::fwrite(coarse.data(), sizeof(float), coarse.size(), out) != coarse.size() ||
            std::fwrite(back.centroids.data(), sizeof(float), back.centroids.size(), out) != back.centroids.size() || std::fclose(out) != 0)
            throw std::runtime_error("cannot write the read-back quantizers");
        std::printf("seeded dim=%d K=%d m=%d b=%d n=%zu empty=%llu\n", back.dim, K, back.sq_count, back.sq_bits, n, (unsigned long long)empty);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
