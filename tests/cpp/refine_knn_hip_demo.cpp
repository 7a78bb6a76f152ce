// refine_store_hip::knn (quick-adc_amd/host/refine_hip.hpp) — the C++14 mirror of qadc_refine_knn — beside
// the host twin refine::knn (host/refine.hpp) on a store read from a file: keys, the distances' bits and sizes must be identical, with
// the plan's default and with chunks of 64 rows and passes of 3 queries.  The mirror's result is written out, so that
// tests/test_gpu_refine_knn_cpp.py can compare it with the Python call on the same data.  C++14.
//   usage: refine_knn_hip_demo IN OUT
//   IN : int32 dim, dtype (0 f32, 1 f16), keyed, n, nq, R, fmode (-1 no filter, 0 exclude, 1 allow), nf |
//        uint32 labels [n] (dense: labels[0] is the first key) | float vectors [n][dim] | float queries [nq][dim] | uint32 fkeys [nf]
//   OUT: uint32 keys [nq][R] | float dist [nq][R] | int32 sizes [nq]
// Prints "ok <queries>" and exits 0 when everything agrees.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <vector>

#include "../../quick-adc_amd/host/refine.hpp"
#include "../../quick-adc_amd/host/refine_hip.hpp"

using namespace qadc;

template <typename T>
static void read_vec(std::FILE* f, std::vector<T>& v, std::size_t n) {
    v.resize(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::cerr << "short input" << std::endl;
        std::exit(2);
    }
}

static bool same(const refine_result& a, const std::vector<std::uint32_t>& k, const std::vector<float>& d, const std::vector<std::int32_t>& s) {
    return a.keys == k && a.sizes == s && std::memcmp(a.dist.data(), d.data(), sizeof(float) * d.size()) == 0;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::cerr << "usage: refine_knn_hip_demo IN OUT" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<std::int32_t> head;
    read_vec(in, head, 8);
    const int dim = head[0], dtype = head[1], n = head[3], nq = head[4], R = head[5], fmode = head[6], nf = head[7];
    const bool keyed = head[2] != 0;
    std::vector<std::uint32_t> labels, fkeys;
    std::vector<float> vectors, queries;
    read_vec(in, labels, n);
    read_vec(in, vectors, (std::size_t)n * dim);
    read_vec(in, queries, (std::size_t)nq * dim);
    read_vec(in, fkeys, nf);
    std::fclose(in);

    refine_store_hip gpu(dim, dtype, 0, keyed);
    refine::store dense(dim, dtype);
    refine::keyed_store map(dim, dtype);
    if (keyed) {
        gpu.put(vectors.data(), labels.data(), n);
        if (!map.put(vectors.data(), labels.data(), n)) return 3;
    } else if (n) {
        gpu.add(vectors.data(), n, labels[0]);
        if (!dense.add(vectors.data(), n, labels[0])) return 3;
    }
    qadc_adc_filter* filter = nullptr;
    refine::filter tf;
    if (fmode >= 0) {
        if (qadc_adc_filter_create(&filter, fmode, fkeys.data(), fkeys.size(), 0) != QADC_OK) refine_store_hip::die("filter");
        tf.mode = fmode;
        tf.keys = fkeys;
        std::sort(tf.keys.begin(), tf.keys.end());
    }
    std::vector<std::uint32_t> wk((std::size_t)nq * R);
    std::vector<float> wd((std::size_t)nq * R);
    std::vector<std::int32_t> ws(nq);
    if (keyed)
        refine::knn(map, nq, queries.data(), R, fmode >= 0 ? &tf : nullptr, wk.data(), wd.data(), ws.data());
    else
        refine::knn(dense, nq, queries.data(), R, fmode >= 0 ? &tf : nullptr, wk.data(), wd.data(), ws.data());

    int bad = 0;
    const refine_result got = gpu.knn(nq, queries.data(), R, filter);
    if (!same(got, wk, wd, ws)) {
        std::cerr << "the mirror and the twin differ" << std::endl;
        ++bad;
    }
    gpu.set_knn_plan(64, 3);
    if (!same(gpu.knn(nq, queries.data(), R, filter), wk, wd, ws)) {
        std::cerr << "the mirror and the twin differ in chunks of 64 rows" << std::endl;
        ++bad;
    }
    if (filter && qadc_adc_filter_destroy(filter) != QADC_OK) ++bad;   // (no use was counted on it)

    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    std::fwrite(got.keys.data(), 4, got.keys.size(), out);
    std::fwrite(got.dist.data(), 4, got.dist.size(), out);
    std::fwrite(got.sizes.data(), 4, got.sizes.size(), out);
    std::fclose(out);
    if (bad) {
        std::cout << "FAIL " << bad << std::endl;
        return 1;
    }
    std::cout << "ok " << nq << std::endl;
    return 0;
}
