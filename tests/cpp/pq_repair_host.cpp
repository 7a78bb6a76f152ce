// CPU driver of tests/test_pq_repair_host.py and of the GPU tests' expectations: the host twin of the empty-cluster repair
// (host/pq_repair.hpp) and the `repair` overloads of the training twins (host/db_build.hpp).  Header-only: nothing of the C-ABI
// library is linked.  All files are raw little-endian arrays.
//   pq_repair_host repair IN OUT   IN: int64 {n, dim, sq_count, sq_bits}, vectors [n][dim] float32 as the quantizer sees them,
//                                  codebooks [sq_count][2^sq_bits][dsub] float32, codes in the encoder's layout;
//                                  OUT: the codes repaired, moved [sq_count] uint32
//   pq_repair_host train IN OUT    IN: int64 {n, dim, sq_count, sq_bits, iters, div_mode, repair}, vectors, seed codebooks;
//                                  OUT: codebooks, the last round's codes, uint64 {empty, repaired}
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../quick-adc_amd/host/db_build.hpp"

template <typename T>
static std::vector<T> take(std::ifstream& f, size_t count) {
    std::vector<T> v(count);
    f.read(reinterpret_cast<char*>(v.data()), sizeof(T) * count);
    if (!f) throw std::runtime_error("short input");
    return v;
}

template <typename T>
static void put(std::ofstream& o, const std::vector<T>& v) {
    o.write(reinterpret_cast<const char*>(v.data()), sizeof(T) * v.size());
}

int main(int argc, char** argv) {
    try {
        const std::string mode = argc == 4 ? argv[1] : "";
        if (mode != "repair" && mode != "train") {
            std::fprintf(stderr, "usage: %s repair|train IN OUT\n", argv[0]);
            return 2;
        }
        std::ifstream f(argv[2], std::ios_base::in | std::ios_base::binary);
        if (!f) throw std::runtime_error("cannot open the input");
        std::ofstream o(argv[3], std::ios_base::out | std::ios_base::binary);
        const std::vector<std::int64_t> h = take<std::int64_t>(f, mode == "repair" ? 4 : 7);
        const size_t n = (size_t)h[0];
        const int dim = (int)h[1], sq_count = (int)h[2], sq_bits = (int)h[3];
        if (sq_count <= 0 || dim <= 0 || dim % sq_count || (sq_bits != 4 && sq_bits != 8 && sq_bits != 16)) throw std::runtime_error("bad header");
        const size_t code_bytes = sq_bits == 4 ? (size_t)sq_count / 2 : sq_bits == 8 ? (size_t)sq_count : (size_t)sq_count * 2;
        const std::vector<float> vecs = take<float>(f, n * dim);
        std::vector<float> cb = take<float>(f, ((size_t)1 << sq_bits) * dim);
        if (mode == "repair") {
            std::vector<std::uint8_t> codes = take<std::uint8_t>(f, n * code_bytes);
            std::vector<std::uint32_t> moved((size_t)sq_count);
            qadc::pq_repair(vecs.data(), n, dim, sq_count, sq_bits, cb.data(), codes.data(), moved.data());
            put(o, codes);
            put(o, moved);
        } else {
            const int iters = (int)h[4], div_mode = (int)h[5];
            const bool repair = h[6] != 0;
            std::vector<std::uint64_t> tail(2);
            if (sq_bits == 16) {
                std::vector<std::uint16_t> codes(n * sq_count);
                tail[0] = qadc::pq_train16_iterations(vecs.data(), n, dim, sq_count, 0, nullptr, nullptr, cb.data(), iters, codes.data(), div_mode, repair,
                                                      &tail[1]);
                put(o, cb);
                put(o, codes);
            } else {
                std::vector<std::uint8_t> codes(n * code_bytes);
                tail[0] = qadc::pq_train_iterations(vecs.data(), n, dim, sq_count, sq_bits, 0, nullptr, nullptr, cb.data(), iters, codes.data(), div_mode,
                                                    repair, &tail[1]);
                put(o, cb);
                put(o, codes);
            }
            put(o, tail);
        }
        if (!o) throw std::runtime_error("cannot write the output");
        std::cout << "ok" << std::endl;
        return 0;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
