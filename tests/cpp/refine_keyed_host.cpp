// TEST DRIVER (CPU only): the host twin of the keyed refine store (refine::keyed_store and refine::rerank of host/refine.hpp) —
// the written definition of qadc_refine_put, _remove and of _rerank over a keyed store (include/qadc.h) —
// on a script of operations read from a file.  tests/test_refine_keyed_host.py compares the outputs, bit for bit, with a numpy
// restatement; the GPU tests compare the library with these outputs.  C++14, header only.
//   usage: refine_keyed_host IN OUT
//   IN : int32 dim, dtype (0 f32, 1 f16), nops, then per operation int32 kind and
//        0 put   : uint64 count | uint32 labels [count] | float vectors [count][dim]
//        1 remove: uint64 count | uint32 labels [count]
//        2 rerank: int32 nq, r_in, R, has_counts, has_values | float queries [nq][dim] | uint32 keys [nq][r_in] |
//                  (has_counts) int32 counts [nq] | (has_values) float values [nq][r_in]
//   OUT: per operation
//        put   : int32 ok (0: refused, the map unchanged) | uint64 keys held
//        remove: uint64 removed | uint64 keys held
//        rerank: uint64 missing | uint32 keys [nq][R] | float dist [nq][R] | int32 sizes [nq]
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
        std::cerr << "usage: refine_keyed_host IN OUT" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<std::int32_t> head;
    read_vec(in, head, 3);
    const int dim = head[0], dtype = head[1], nops = head[2];
    refine::keyed_store st(dim, dtype);
    for (int op = 0; op < nops; ++op) {
        read_vec(in, head, 1);
        const int kind = head[0];
        if (kind == 0 || kind == 1) {
            std::vector<std::uint64_t> n;
            std::vector<std::uint32_t> labels;
            std::vector<float> vec;
            read_vec(in, n, 1);
            read_vec(in, labels, (std::size_t)n[0]);
            std::uint64_t live;
            if (kind == 0) {
                read_vec(in, vec, (std::size_t)n[0] * dim);
                const std::int32_t ok = st.put(vec.data(), labels.data(), n[0]) ? 1 : 0;
                std::fwrite(&ok, 4, 1, out);
            } else {
                const std::uint64_t removed = st.remove(labels.data(), n[0]);
                std::fwrite(&removed, 8, 1, out);
            }
            live = st.live();
            std::fwrite(&live, 8, 1, out);
        } else if (kind == 2) {
            read_vec(in, head, 5);
            const int nq = head[0], r_in = head[1], R = head[2];
            const bool has_counts = head[3] != 0, has_values = head[4] != 0;
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
            std::fwrite(&missing, 8, 1, out);
            std::fwrite(ok.data(), 4, ok.size(), out);
            std::fwrite(od.data(), 4, od.size(), out);
            std::fwrite(os.data(), 4, os.size(), out);
        } else {
            std::cerr << "unknown operation " << kind << std::endl;
            return 2;
        }
    }
    std::fclose(in);
    std::fclose(out);
    std::cout << "ok" << std::endl;
    return 0;
}
