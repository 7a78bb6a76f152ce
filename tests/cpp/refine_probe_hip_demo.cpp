// refine_store_hip::knn_probed and search_exact (quick-adc_amd/host/refine_hip.hpp) — the C++14 mirrors of qadc_refine_knn_probed and
// qadc_adc_search_exact — beside the host twin refine::knn_probed (host/refine.hpp) on a store and an index
// read from a file: keys, the distances' bits, sizes and the missing count must be identical, with the plan's default and with chunks
// of 64 rows and passes of 3 queries; search_exact must equal the twin on the probe lists it reports.  The mirrors' results are written
// out, so that tests/test_gpu_refine_probe_device.py can compare them with the Python calls on the same data.  C++14.
//   usage: refine_probe_hip_demo IN OUT
//   IN : int32 dim, dtype (0 f32, 1 f16), keyed, n, K, nq, ma, R | uint32 keys [n] (dense: keys[0] is the first key) |
//        float vectors [n][dim] | uint32 sizes [K] | uint32 labels [sum of sizes] | float codebooks [8][256][dim / 8] |
//        float centroids [K][dim] | float queries [nq][dim] | int32 assign [nq][ma]
//   OUT: knn_probed: uint32 keys [nq][R] | float dist [nq][R] | int32 sizes [nq] | uint64 missing; then the same four of search_exact
//        and its int32 assign [nq][ma]
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

struct twin_result {
    std::vector<std::uint32_t> keys;
    std::vector<float> dist;
    std::vector<std::int32_t> sizes;
    std::uint64_t missing = 0;
};

static bool same(const refine_result& a, const twin_result& w) {
    return a.keys == w.keys && a.sizes == w.sizes && a.missing == w.missing &&
           std::memcmp(a.dist.data(), w.dist.data(), sizeof(float) * w.dist.size()) == 0;
}

static void write_result(std::FILE* out, const refine_result& r) {
    std::fwrite(r.keys.data(), 4, r.keys.size(), out);
    std::fwrite(r.dist.data(), 4, r.dist.size(), out);
    std::fwrite(r.sizes.data(), 4, r.sizes.size(), out);
    std::fwrite(&r.missing, 8, 1, out);
}

struct no_db {};   // (the engine is used for its index, ma and sum_mode alone)

int main(int argc, char** argv) {
    if (argc != 3) {
        std::cerr << "usage: refine_probe_hip_demo IN OUT" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<std::int32_t> head, assign;
    read_vec(in, head, 8);
    const int dim = head[0], dtype = head[1], n = head[3], K = head[4], nq = head[5], ma = head[6], R = head[7];
    const bool keyed = head[2] != 0;
    std::vector<std::uint32_t> keys, sizes, labels;
    std::vector<float> vectors, codebooks, centroids, queries;
    read_vec(in, keys, n);
    read_vec(in, vectors, (std::size_t)n * dim);
    read_vec(in, sizes, K);
    std::size_t rows = 0;
    for (std::uint32_t s : sizes) rows += s;
    read_vec(in, labels, rows);
    read_vec(in, codebooks, (std::size_t)256 * dim);
    read_vec(in, centroids, (std::size_t)K * dim);
    read_vec(in, queries, (std::size_t)nq * dim);
    read_vec(in, assign, (std::size_t)nq * ma);
    std::fclose(in);

    refine_store_hip gpu(dim, dtype, 0, keyed);
    refine::store dense(dim, dtype);
    refine::keyed_store map(dim, dtype);
    if (keyed) {
        gpu.put(vectors.data(), keys.data(), n);
        if (!map.put(vectors.data(), keys.data(), n)) return 3;
    } else if (n) {
        gpu.add(vectors.data(), n, keys[0]);
        if (!dense.add(vectors.data(), n, keys[0])) return 3;
    }

    // the index: K labelled partitions of codes that no call of this demo reads, and the quantizers of the coarse step
    no_db db;
    adc_search_engine_hip<no_db> engine(db, ma, nq, R);
    if (qadc_adc_index_create(&engine.index, 8, 8, 0) != QADC_OK) refine_store_hip::die("index");
    std::vector<std::uint8_t> codes(rows * 8, 0);
    std::vector<const std::uint8_t*> code_of(K);
    std::vector<const std::uint32_t*> label_of(K);
    std::vector<refine::probe_part> parts(K);
    for (std::size_t p = 0, at = 0; p < (std::size_t)K; at += sizes[p], ++p) {
        code_of[p] = codes.data() + at * 8;
        label_of[p] = labels.data() + at;
        parts[p] = refine::probe_part{labels.data() + at, 0, sizes[p]};
    }
    if (qadc_adc_index_add_partitions(engine.index, K, code_of.data(), label_of.data(), sizes.data()) != QADC_OK) refine_store_hip::die("partitions");
    if (qadc_adc_index_set_pq(engine.index, dim, codebooks.data()) != QADC_OK) refine_store_hip::die("set_pq");
    if (qadc_adc_index_set_coarse(engine.index, K, centroids.data()) != QADC_OK) refine_store_hip::die("set_coarse");

    auto twin = [&](const std::int32_t* a) {
        twin_result w;
        w.keys.resize((std::size_t)nq * R);
        w.dist.resize((std::size_t)nq * R);
        w.sizes.resize(nq);
        w.missing = keyed ? refine::knn_probed(map, parts.data(), K, nullptr, nq, queries.data(), ma, a, R, nullptr, w.keys.data(), w.dist.data(),
                                               w.sizes.data())
                          : refine::knn_probed(dense, parts.data(), K, nullptr, nq, queries.data(), ma, a, R, nullptr, w.keys.data(),
                                               w.dist.data(), w.sizes.data());
        return w;
    };

    int bad = 0;
    const twin_result want = twin(assign.data());
    const refine_result got = gpu.knn_probed(engine.index, nq, queries.data(), ma, assign.data(), R);
    if (!same(got, want)) {
        std::cerr << "knn_probed: the mirror and the twin differ" << std::endl;
        ++bad;
    }
    gpu.set_knn_plan(64, 3);
    if (!same(gpu.knn_probed(engine.index, nq, queries.data(), ma, assign.data(), R), want)) {
        std::cerr << "knn_probed: the mirror and the twin differ in chunks of 64 rows" << std::endl;
        ++bad;
    }
    gpu.set_knn_plan(0, 0);
    std::vector<std::int32_t> probes;
    const refine_result exact = search_exact(engine, gpu, nq, queries.data(), R, nullptr, &probes);
    if (probes.size() != (std::size_t)nq * ma || !same(exact, twin(probes.data()))) {
        std::cerr << "search_exact: the mirror and the twin on its probe lists differ" << std::endl;
        ++bad;
    }

    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    write_result(out, got);
    write_result(out, exact);
    std::fwrite(probes.data(), 4, probes.size(), out);
    std::fclose(out);
    if (bad) {
        std::cout << "FAIL " << bad << std::endl;
        return 1;
    }
    std::cout << "ok " << nq << std::endl;
    return 0;
}
