// One CPU thread of the host twin's encoder for 16-bit sub-quantizers, pq_bytes::encode (host/scanner_simple.hpp), timed on a
// few vectors: the figure tools/adc_bench.py --bits 16 --legs encode16 scales to the size of the GPU call.  A port of
// encode_multiple_vectors, not the reference's build (which calls OpenBLAS).  C++14, header only.
//   usage: encode16_host_twin IN OUT
//   IN : int32 nsq, dim, n | float codebooks [nsq][65536][dim/nsq] | float vectors [n][dim]
//   OUT: uint8 codes [n][2*nsq] (little-endian 16-bit words);  stdout: "us <microseconds of the encode call>"
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <vector>

#include "../quick-adc_amd/host/scanner_simple.hpp"

int main(int argc, char** argv) {
    if (argc != 3) {
        std::cerr << "usage: encode16_host_twin IN OUT" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    std::int32_t head[3];
    if (!in || !out || std::fread(head, 4, 3, in) != 3) {
        std::cerr << "cannot read the input" << std::endl;
        return 2;
    }
    const int nsq = head[0], dim = head[1];
    const std::size_t n = (std::size_t)head[2];
    qadc::pq_bytes pq(nsq, 16, dim);
    std::vector<float> vectors(n * dim);
    if (std::fread(pq.centroids.data(), 4, pq.centroids.size(), in) != pq.centroids.size() ||
        std::fread(vectors.data(), 4, vectors.size(), in) != vectors.size()) {
        std::cerr << "short input" << std::endl;
        return 2;
    }
    std::fclose(in);
    std::vector<std::uint8_t> codes(n * pq.code_size());
    const auto t0 = std::chrono::steady_clock::now();
    pq.encode(vectors.data(), n, codes.data());
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (std::fwrite(codes.data(), 1, codes.size(), out) != codes.size()) return 2;
    std::fclose(out);
    std::cout << "us " << us << std::endl;
    return 0;
}
