// TEST DRIVER (CPU only): the host twin of the exhaustive search (refine::knn of host/refine.hpp) — the written definition of
// qadc_refine_knn (include/qadc.h) — over a dense or a keyed store whose life is a script read from a file.
// tests/test_refine_knn_host.py compares the outputs, bit for bit, with a numpy restatement; the GPU tests compare the library with
// these outputs.  Beside every knn the driver writes the twin's rerank fed every held key that passes the filter, from a key list it
// keeps itself, in descending order.  C++14, header only.
//   usage: refine_knn_host IN OUT
//   IN : int32 ncases, then per case int32 keyed (0 dense, 1 keyed), dim, dtype (0 f32, 1 f16), nops, then per operation int32 kind and
//        0 add   : uint32 first_key, count | float vectors [count][dim]                      (dense)
//        1 put   : uint64 count | uint32 labels [count] | float vectors [count][dim]         (keyed)
//        2 remove: uint64 count | uint32 labels [count]                                      (keyed)
//        3 knn   : int32 nq, R, fmode (-1 no filter, 0 exclude, 1 allow) | uint64 nf | float queries [nq][dim] | uint32 fkeys [nf]
//   OUT: per knn  uint32 keys [nq][R] | float dist [nq][R] | int32 sizes [nq], then the same three of the rerank
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <set>
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

template <typename Store>
static void knn_op(const Store& st, const std::set<std::uint32_t>& held, std::FILE* in, std::FILE* out) {
    std::vector<std::int32_t> head;
    std::vector<std::uint64_t> nf;
    std::vector<float> queries;
    refine::filter f;
    read_vec(in, head, 3);
    read_vec(in, nf, 1);
    const int nq = head[0], R = head[1], fmode = head[2];
    read_vec(in, queries, (std::size_t)nq * st.dim);
    read_vec(in, f.keys, (std::size_t)nf[0]);
    f.mode = fmode == 1 ? refine::kFilterAllow : refine::kFilterExclude;
    std::sort(f.keys.begin(), f.keys.end());
    std::vector<std::uint32_t> ok((std::size_t)nq * R);
    std::vector<float> od((std::size_t)nq * R);
    std::vector<std::int32_t> os(nq);
    refine::knn(st, nq, queries.data(), R, fmode < 0 ? nullptr : &f, ok.data(), od.data(), os.data());
    std::fwrite(ok.data(), 4, ok.size(), out);
    std::fwrite(od.data(), 4, od.size(), out);
    std::fwrite(os.data(), 4, os.size(), out);

    // rerank, fed the keys this driver counted as held and passing, last key first
    const std::set<std::uint32_t> listed(f.keys.begin(), f.keys.end());
    std::vector<std::uint32_t> pass;
    for (auto it = held.rbegin(); it != held.rend(); ++it)
        if (fmode < 0 || (listed.count(*it) != 0) == (fmode == 1)) pass.push_back(*it);
    const int r_in = std::max<int>(1, (int)pass.size());
    std::vector<std::int32_t> counts(nq, (std::int32_t)pass.size());
    std::vector<std::uint32_t> keys((std::size_t)nq * r_in, 0u);
    for (int q = 0; q < nq; ++q) std::copy(pass.begin(), pass.end(), keys.begin() + (std::size_t)q * r_in);
    refine::rerank(st, nq, queries.data(), r_in, keys.data(), counts.data(), nullptr, R, ok.data(), od.data(), os.data());
    std::fwrite(ok.data(), 4, ok.size(), out);
    std::fwrite(od.data(), 4, od.size(), out);
    std::fwrite(os.data(), 4, os.size(), out);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::cerr << "usage: refine_knn_host IN OUT" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<std::int32_t> head;
    read_vec(in, head, 1);
    for (int c = 0, ncases = head[0]; c < ncases; ++c) {
        read_vec(in, head, 4);
        const bool keyed = head[0] != 0;
        const int dim = head[1], dtype = head[2], nops = head[3];
        refine::store dense(dim, dtype);
        refine::keyed_store map(dim, dtype);
        std::set<std::uint32_t> held;
        for (int op = 0; op < nops; ++op) {
            read_vec(in, head, 1);
            const int kind = head[0];
            std::vector<std::uint32_t> labels;
            std::vector<std::uint64_t> n;
            std::vector<float> vec;
            if (kind == 0 && !keyed) {
                read_vec(in, labels, 2);
                read_vec(in, vec, (std::size_t)labels[1] * dim);
                if (!dense.add(vec.data(), labels[1], labels[0])) return 3;
                for (std::uint32_t i = 0; i < labels[1]; ++i) held.insert(labels[0] + i);
            } else if (kind == 1 && keyed) {
                read_vec(in, n, 1);
                read_vec(in, labels, (std::size_t)n[0]);
                read_vec(in, vec, (std::size_t)n[0] * dim);
                if (!map.put(vec.data(), labels.data(), n[0])) return 3;
                held.insert(labels.begin(), labels.end());
            } else if (kind == 2 && keyed) {
                read_vec(in, n, 1);
                read_vec(in, labels, (std::size_t)n[0]);
                map.remove(labels.data(), n[0]);
                for (std::uint32_t k : labels) held.erase(k);
            } else if (kind == 3) {
                if (keyed)
                    knn_op(map, held, in, out);
                else
                    knn_op(dense, held, in, out);
            } else {
                std::cerr << "unknown operation " << kind << std::endl;
                return 2;
            }
        }
    }
    std::fclose(in);
    std::fclose(out);
    std::cout << "ok" << std::endl;
    return 0;
}
