// Learning a product quantizer from C++14 (host/db_build.hpp: learn_pq_hip): reads a learning set (.fvecs / .bvecs), seeds every
// sub-quantizer with the sub-vectors of the file's first 2^bits vectors, runs `iters` rounds on the GPU and writes the .pq.data file
// the reference's flatdb_create / indexdb_create2 read.  Then reads the file back through pq_from_data_file and writes the
// centroids it holds as raw floats (tests/test_gpu_pq_train_cpp.py compares them with the Python route).
//   pq_train_demo <learn file> <sq_count> <sq_bits> <iters> <out.pq.data> <readback>
// stdout: "pq dim=<dim> m=<sq_count> b=<sq_bits> n=<vectors> empty=<NaN centroids>".
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "../../quick-adc_amd/host/db_build.hpp"

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s <learn file> <sq_count> <sq_bits> <iters> <out.pq.data> <readback>\n", argv[0]);
        return 2;
    }
    try {
        const qadc::io::vectors_owner<float> learn = qadc::io::load_vectors_by_extension(argv[1]);
        const int dim = learn.dimension, sq_count = std::atoi(argv[2]), sq_bits = std::atoi(argv[3]), iters = std::atoi(argv[4]);
        const size_t n = (size_t)learn.count, K = (size_t)1 << sq_bits;
        if (sq_count <= 0 || dim % sq_count || sq_bits <= 0 || sq_bits > 16 || n < K) throw std::runtime_error("the learning set does not fit the quantizer's shape");
        const int ds = dim / sq_count;
        std::vector<float> seed((size_t)dim * K);                    // [sq_count][K][ds] from rows 0 .. K - 1
        for (int m = 0; m < sq_count; ++m)
            for (size_t k = 0; k < K; ++k)
                for (int d = 0; d < ds; ++d) seed[((size_t)m * K + k) * ds + d] = learn.data[k * dim + (size_t)m * ds + d];
        std::uint64_t empty = 0;
        const qadc::io::pq_data pq = qadc::learn_pq_hip(learn.data.data(), n, dim, sq_count, sq_bits, seed.data(), iters, 0, nullptr, nullptr, 0, &empty);
        qadc::io::pq_to_data_file(pq, argv[5]);
        const qadc::io::pq_data back = qadc::io::pq_from_data_file(argv[5]);
        FILE* out = std::fopen(argv[6], "wb");
        if (!out || std::fwrite(back.centroids.data(), sizeof(float), back.centroids.size(), out) != back.centroids.size() || std::fclose(out) != 0)
            throw std::runtime_error("cannot write the read-back centroids");
        std::printf("pq dim=%d m=%d b=%d n=%zu empty=%llu\n", back.dim, back.sq_count, back.sq_bits, n, (unsigned long long)empty);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
