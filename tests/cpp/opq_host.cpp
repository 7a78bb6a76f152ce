// CPU driver of tests/test_opq_host.py and of the GPU tests' expectations: the host twins of OPQ learning (host/db_build.hpp:
// opq_cross, opq_train_iterations) and a plain restatement of the cross matrix's sums.  Header-only: nothing of the C-ABI library is
// linked.  All files are raw little-endian arrays.
//   opq_host cross IN OUT   IN: int32 {n, dim, sq_count, sq_bits, K_coarse}, vectors [n][dim], codebooks, coarse [K_coarse][dim]
//                           (float32), codes (uint8, the encoder's layout);  OUT: M [dim][dim] float64
//   opq_host chain IN OUT   IN: int32 {n, dim, descending}, x [n][dim], y [n][dim] (float32);  OUT: M [dim][dim] float64, where
//                           per block of QADC_OPQ_BLOCK rows M[a][b] += (double)(the float chain fmaf(x[i][a], y[i][b], acc) over the
//                           block's rows, ascending — or descending on request), the blocks in ascending order
//   opq_host train IN OUT   IN: int32 {n, dim, sq_count, sq_bits, K_coarse, outer, inner, div_mode}, vectors, seed codebooks,
//                           coarse, rotation [dim][dim];  OUT: rotation, codebooks, codes, uint64 empty, int32 rounds_done
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
        if (mode != "cross" && mode != "chain" && mode != "train") {
            std::fprintf(stderr, "usage: %s cross|chain|train IN OUT\n", argv[0]);
            return 2;
        }
        std::ifstream f(argv[2], std::ios_base::in | std::ios_base::binary);
        if (!f) throw std::runtime_error("cannot open the input");
        std::ofstream o(argv[3], std::ios_base::out | std::ios_base::binary);
        if (mode == "chain") {
            const std::vector<std::int32_t> h = take<std::int32_t>(f, 3);
            const size_t n = (size_t)h[0], d = (size_t)h[1];
            const bool descending = h[2] != 0;
            const std::vector<float> x = take<float>(f, n * d), y = take<float>(f, n * d);
            std::vector<double> M(d * d, 0.0);
            for (size_t a = 0; a < d; ++a)
                for (size_t b = 0; b < d; ++b)
                    for (size_t first = 0; first < n; first += QADC_OPQ_BLOCK) {
                        const size_t last = std::min(n, first + (size_t)QADC_OPQ_BLOCK);
                        float acc = 0.0f;
                        for (size_t k = 0; k < last - first; ++k) {
                            const size_t i = descending ? last - 1 - k : first + k;
                            acc = std::fmaf(x[i * d + a], y[i * d + b], acc);
                        }
                        M[a * d + b] += (double)acc;
                    }
            put(o, M);
        } else if (mode == "cross") {
            const std::vector<std::int32_t> h = take<std::int32_t>(f, 5);
            const size_t n = (size_t)h[0];
            const int dim = h[1], sq_count = h[2], sq_bits = h[3], K_coarse = h[4];
            const std::vector<float> vecs = take<float>(f, n * dim);
            const std::vector<float> cb = take<float>(f, ((size_t)dim << sq_bits));
            const std::vector<float> coarse = take<float>(f, (size_t)K_coarse * dim);
            const std::vector<std::uint8_t> codes = take<std::uint8_t>(f, n * (size_t)(sq_bits == 4 ? sq_count / 2 : sq_count));
            std::vector<double> M((size_t)dim * dim);
            qadc::opq_cross(vecs.data(), n, dim, sq_count, sq_bits, K_coarse, K_coarse ? coarse.data() : nullptr, codes.data(), cb.data(), M.data());
            put(o, M);
        } else {
            const std::vector<std::int32_t> h = take<std::int32_t>(f, 8);
            const size_t n = (size_t)h[0];
            const int dim = h[1], sq_count = h[2], sq_bits = h[3], K_coarse = h[4], outer = h[5], inner = h[6], div_mode = h[7];
            const std::vector<float> vecs = take<float>(f, n * dim);
            std::vector<float> cb = take<float>(f, ((size_t)dim << sq_bits));
            const std::vector<float> coarse = take<float>(f, (size_t)K_coarse * dim);
            std::vector<float> rot = take<float>(f, (size_t)dim * dim);
            std::vector<std::uint8_t> codes(n * (size_t)(sq_bits == 4 ? sq_count / 2 : sq_count));
            std::int32_t done = 0;
            const std::uint64_t empty = qadc::opq_train_iterations(vecs.data(), n, dim, sq_count, sq_bits, K_coarse, K_coarse ? coarse.data() : nullptr,
                                                                   rot.data(), cb.data(), outer, inner, codes.data(), div_mode, &done);
            put(o, rot);
            put(o, cb);
            put(o, codes);
            o.write(reinterpret_cast<const char*>(&empty), sizeof(empty));
            o.write(reinterpret_cast<const char*>(&done), sizeof(done));
        }
        if (!o) throw std::runtime_error("cannot write the output");
        std::cout << "ok" << std::endl;
        return 0;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
