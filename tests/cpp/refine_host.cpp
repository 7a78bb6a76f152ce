// TEST DRIVER (CPU only): the host twin of exact re-ranking (host/refine.hpp) — the written definition of qadc_refine_rerank
// (include/qadc.h) — on cases read from a file.  tests/test_refine_host.py compares the outputs, bit for
// bit, with a numpy restatement of the definition; the GPU tests compare the library with these outputs.  C++14, header only.
//   usage: refine_host IN OUT
//   IN : int32 ncases, then per case
//        int32 dim, dtype (0 f32, 1 f16), nadds, nq, r_in, R, has_counts, has_values
//        per add: uint32 first_key, uint32 count | float vectors [count][dim]
//        float queries [nq][dim] | uint32 keys [nq][r_in] | (has_counts) int32 counts [nq] | (has_values) float values [nq][r_in]
//   OUT: per case int32 refused adds | uint64 missing | uint32 keys [nq][R] | float dist [nq][R] | int32 sizes [nq]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "../../quick-adc_amd/host/refine.hpp"

using namespace qadc;

template <typename T>
static void read_vec(std::FILE* f, std::vector<T>& v, std::size_t n) {
    v.resize(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::cerr << "short input" << std::endl;
        std::exit(2);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::cerr << "usage: refine_host IN OUT" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<std::int32_t> head;
    read_vec(in, head, 1);
    for (int c = 0, ncases = head[0]; c < ncases; ++c) {
        read_vec(in, head, 8);
        const int dim = head[0], dtype = head[1], nadds = head[2], nq = head[3], r_in = head[4], R = head[5];
        const bool has_counts = head[6] != 0, has_values = head[7] != 0;
        refine::store st(dim, dtype);
        std::int32_t refused = 0;
        for (int a = 0; a < nadds; ++a) {
            std::vector<std::uint32_t> hd;
            std::vector<float> vec;
            read_vec(in, hd, 2);
            read_vec(in, vec, (std::size_t)hd[1] * dim);
            if (!st.add(vec.data(), hd[1], hd[0])) ++refused;
        }
        std::vector<float> queries, values;
        std::vector<std::uint32_t> keys;
        std::vector<std::int32_t> counts;
        read_vec(in, queries, (std::size_t)nq * dim);
        read_vec(in, keys, (std::size_t)nq * r_in);
        if (has_counts) read_vec(in, counts, nq);
        if (has_values) read_vec(in, values, (std::size_t)nq * r_in);

        std::vector<std::uint32_t> ok((std::size_t)nq * R);
        std::vector<float> od((std::size_t)nq * R);
        std::vector<std::int32_t> os(nq);
        const std::uint64_t missing = refine::rerank(st, nq, queries.data(), r_in, keys.data(), has_counts ? counts.data() : nullptr,
                                                    has_values ? values.data() : nullptr, R, ok.data(), od.data(), os.data());
        std::fwrite(&refused, 4, 1, out);
        std::fwrite(&missing, 8, 1, out);
        std::fwrite(ok.data(), 4, ok.size(), out);
        std::fwrite(od.data(), 4, od.size(), out);
        std::fwrite(os.data(), 4, os.size(), out);
    }
    std::fclose(in);
    std::fclose(out);
    std::cout << "ok" << std::endl;
    return 0;
}
