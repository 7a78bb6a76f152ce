// CPU driver of tests/test_kmeans_seed_host.py and of the GPU tests' expectations: the host twin of k-means++ seeding
// (host/kmeans_seed.hpp behind host/db_build.hpp's front).  Header-only: nothing of the C-ABI library is linked.  All files are raw
// little-endian arrays.
//   kmeans_seed_host seed IN OUT    IN: int64 {n, dim, sq_count, k, K_coarse, has_rotation, seed, seeds}, vectors [n][dim], coarse
//                                   [K_coarse][dim], rotation [dim][dim] if has_rotation (float32);  OUT: for each of the `seeds`
//                                   seeds seed, seed + 1, ...: centres [sq_count][k][dsub] float32, rows [sq_count][k] uint32,
//                                   fallbacks uint64
//   kmeans_seed_host rows IN OUT    the same input; OUT: only rows, for each seed (the frequency tests)
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
        if (mode != "seed" && mode != "rows") {
            std::fprintf(stderr, "usage: %s seed|rows IN OUT\n", argv[0]);
            return 2;
        }
        std::ifstream f(argv[2], std::ios_base::in | std::ios_base::binary);
        if (!f) throw std::runtime_error("cannot open the input");
        std::ofstream o(argv[3], std::ios_base::out | std::ios_base::binary);
        const std::vector<std::int64_t> h = take<std::int64_t>(f, 8);
        const size_t n = (size_t)h[0], k = (size_t)h[3];
        const int dim = (int)h[1], sq_count = (int)h[2], K_coarse = (int)h[4];
        const bool has_rotation = h[5] != 0;
        const std::uint64_t seed = (std::uint64_t)h[6];
        const std::vector<float> vecs = take<float>(f, n * dim);
        const std::vector<float> coarse = take<float>(f, (size_t)K_coarse * dim);
        const std::vector<float> rot = take<float>(f, has_rotation ? (size_t)dim * dim : 0);
        // the front does not depend on the seed: once
        const std::vector<float> x = qadc::pq_train_front(vecs.data(), n, dim, K_coarse, K_coarse ? coarse.data() : nullptr,
                                                          has_rotation ? rot.data() : nullptr);
        std::vector<float> centres((size_t)k * dim);
        std::vector<std::uint32_t> rows((size_t)sq_count * k);
        for (std::int64_t s = 0; s < h[7]; ++s) {
            const std::uint64_t fallbacks = qadc::kmeans_seed(x.data(), n, dim, sq_count, k, seed + (std::uint64_t)s, centres.data(), rows.data());
            if (mode == "seed") put(o, centres);
            put(o, rows);
            if (mode == "seed") o.write(reinterpret_cast<const char*>(&fallbacks), sizeof(fallbacks));
        }
        if (!o) throw std::runtime_error("cannot write the output");
        std::cout << "ok" << std::endl;
        return 0;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
