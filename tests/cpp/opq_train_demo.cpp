// Learning an OPQ rotation and its product quantizer from C++14 (host/db_build.hpp: learn_opq_hip): reads a learning set (.fvecs /
// .bvecs), seeds every sub-quantizer with the sub-vectors of the file's first 2^bits vectors, starts from the identity, runs `outer`
// Procrustes rounds of `inner` k-means rounds each on the GPU and writes the .opq.data file the reference's executables read.  Then
// reads the file back through pq_from_data_file and writes the centroids and the rotation it holds as raw floats
// (tests/test_gpu_opq_train_cpp.py compares them with the Python route).
//   opq_train_demo <learn file> <sq_count> <sq_bits> <outer> <inner> <out.opq.data> <readback>
// stdout: "opq dim=<dim> m=<sq_count> b=<sq_bits> n=<vectors> empty=<NaN centroids> rounds=<rotation updates>".
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "../../quick-adc_amd/host/db_build.hpp"

int main(int argc, char** argv) {
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s <learn file> <sq_count> <sq_bits> <outer> <inner> <out.opq.data> <readback>\n", argv[0]);
        return 2;
    }
    try {
        const qadc::io::vectors_owner<float> learn = qadc::io::load_vectors_by_extension(argv[1]);
        const int dim = learn.dimension, sq_count = std::atoi(argv[2]), sq_bits = std::atoi(argv[3]);
        const int outer = std::atoi(argv[4]), inner = std::atoi(argv[5]);
        const size_t n = (size_t)learn.count, K = (size_t)1 << sq_bits;
        if (sq_count <= 0 || dim % sq_count || sq_bits <= 0 || sq_bits > 16 || n < K) throw std::runtime_error("the learning set does not fit the quantizer's shape");
        if (!qadc::io::data_filename_is_opq(argv[6])) throw std::runtime_error("the output must end with .opq.data");
        const int ds = dim / sq_count;
        std::vector<float> seed((size_t)dim * K);                    // [sq_count][K][ds] from rows 0 .. K - 1
        for (int m = 0; m < sq_count; ++m)
            for (size_t k = 0; k < K; ++k)
                for (int d = 0; d < ds; ++d) seed[((size_t)m * K + k) * ds + d] = learn.data[k * dim + (size_t)m * ds + d];
        std::uint64_t empty = 0;
        int rounds = 0;
        const qadc::io::pq_data pq = qadc::learn_opq_hip(learn.data.data(), n, dim, sq_count, sq_bits, seed.data(), outer, inner, 0, nullptr, nullptr, 0,
                                                         &empty, &rounds);
        qadc::io::pq_to_data_file(pq, argv[6]);
        const qadc::io::pq_data back = qadc::io::pq_from_data_file(argv[6]);
        if (!back.is_opq) throw std::runtime_error("the file read back without its rotation");
        FILE* out = std::fopen(argv[7], "wb");
        if (!out || std::fwrite(back.centroids.data(), sizeof(float), back.centroids.size(), out) != back.centroids.size() ||
            std::fwrite(back.rotation.data(), sizeof(float), back.rotation.size(), out) != back.rotation.size() || std::fclose(out) != 0)
            throw std::runtime_error("cannot write the read-back quantizer");
        std::printf("opq dim=%d m=%d b=%d n=%zu empty=%llu rounds=%d\n", back.dim, back.sq_count, back.sq_bits, n, (unsigned long long)empty, rounds);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
