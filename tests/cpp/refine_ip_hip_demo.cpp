// refine_store_hip under the inner-product metric (quick-adc_amd/host/refine_hip.hpp: set_metric): knn,
// rerank and knn_probed of a dense store with QADC_REFINE_IP, beside the host twin (host/refine.hpp with metric kIP) on data read
// from a file: keys, the scores' bits, sizes and the missing counts must be identical.  The mirror's arrays are written out, so that
// tests/test_gpu_refine_ip_cpp.py can compare them with the Python calls on the same data.  The store's metric is then set back to
// QADC_REFINE_L2 and knn must equal the twin's L2 result.  C++14.
//   usage: refine_ip_hip_demo IN OUT
//   IN : int32 dim, dtype (0 f32, 1 f16), n, nq, R, r_in, K, ma | uint32 sizes [K] | uint32 labels [the sum of sizes] (the
//        partitions' labels, one behind the other) | float vectors [n][dim] (the rows of the keys 0 .. n - 1) | float queries [nq][dim] |
//        uint32 cand [nq][r_in] | int32 assign [nq][ma]
//   OUT: knn, rerank, knn_probed, each uint32 keys [nq][R] | float dist [nq][R] | int32 sizes [nq]; then uint64 missing of rerank and
//        of knn_probed
// Prints "ok <queries>" and exits 0 when everything agrees.
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
    twin_result(int nq, int R) : keys((std::size_t)nq * R), dist((std::size_t)nq * R), sizes(nq) {}
};

static int differs(const char* what, const refine_result& a, const twin_result& w) {
    if (a.keys == w.keys && a.sizes == w.sizes && a.missing == w.missing &&
        std::memcmp(a.dist.data(), w.dist.data(), sizeof(float) * w.dist.size()) == 0)
        return 0;
    std::cerr << what << ": the mirror and the twin differ" << std::endl;
    return 1;
}

static void write_result(std::FILE* out, const refine_result& r) {
    std::fwrite(r.keys.data(), 4, r.keys.size(), out);
    std::fwrite(r.dist.data(), 4, r.dist.size(), out);
    std::fwrite(r.sizes.data(), 4, r.sizes.size(), out);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::cerr << "usage: refine_ip_hip_demo IN OUT" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<std::int32_t> head, assign;
    read_vec(in, head, 8);
    const int dim = head[0], dtype = head[1], n = head[2], nq = head[3], R = head[4], r_in = head[5], K = head[6], ma = head[7];
    std::vector<std::uint32_t> sizes, labels, cand;
    std::vector<float> vectors, queries;
    read_vec(in, sizes, K);
    std::size_t part_rows = 0;
    for (std::uint32_t sz : sizes) part_rows += sz;
    read_vec(in, labels, part_rows);
    read_vec(in, vectors, (std::size_t)n * dim);
    read_vec(in, queries, (std::size_t)nq * dim);
    read_vec(in, cand, (std::size_t)nq * r_in);
    read_vec(in, assign, (std::size_t)nq * ma);
    std::fclose(in);

    refine_store_hip gpu(dim, dtype);
    refine::store dense(dim, dtype);
    gpu.add(vectors.data(), n, 0);
    if (!dense.add(vectors.data(), n, 0)) return 3;
    if (gpu.metric() != QADC_REFINE_L2) return 3;      // the default
    gpu.set_metric(QADC_REFINE_IP);
    if (gpu.metric() != QADC_REFINE_IP) return 3;

    // the index: K labelled partitions of codes that no call of this demo reads
    qadc_adc_index* index = nullptr;
    if (qadc_adc_index_create(&index, 8, 8, 0) != QADC_OK) refine_store_hip::die("index");
    std::vector<std::uint8_t> codes(part_rows * 8, 0);
    std::vector<const std::uint8_t*> code_of(K);
    std::vector<const std::uint32_t*> label_of(K);
    std::vector<refine::probe_part> parts(K);
    for (std::size_t p = 0, at = 0; p < (std::size_t)K; at += sizes[p], ++p) {
        code_of[p] = codes.data() + at * 8;
        label_of[p] = labels.data() + at;
        parts[p] = refine::probe_part{labels.data() + at, 0, sizes[p]};
    }
    if (qadc_adc_index_add_partitions(index, K, code_of.data(), label_of.data(), sizes.data()) != QADC_OK) refine_store_hip::die("partitions");

    twin_result wk(nq, R), wr(nq, R), wp(nq, R), wl(nq, R);
    refine::knn(dense, nq, queries.data(), R, nullptr, wk.keys.data(), wk.dist.data(), wk.sizes.data(), refine::kIP);
    wr.missing = refine::rerank(dense, nq, queries.data(), r_in, cand.data(), nullptr, nullptr, R, wr.keys.data(), wr.dist.data(), wr.sizes.data(),
                                refine::kIP);
    wp.missing = refine::knn_probed(dense, parts.data(), K, nullptr, nq, queries.data(), ma, assign.data(), R, nullptr, wp.keys.data(),
                                    wp.dist.data(), wp.sizes.data(), refine::kIP);
    refine::knn(dense, nq, queries.data(), R, nullptr, wl.keys.data(), wl.dist.data(), wl.sizes.data());

    const refine_result gk = gpu.knn(nq, queries.data(), R);
    const refine_result gr = gpu.rerank(nq, queries.data(), r_in, cand.data(), nullptr, nullptr, R);
    const refine_result gp = gpu.knn_probed(index, nq, queries.data(), ma, assign.data(), R);
    int bad = differs("knn", gk, wk) + differs("rerank", gr, wr) + differs("knn_probed", gp, wp);
    gpu.set_metric(QADC_REFINE_L2);
    bad += differs("knn, back under L2", gpu.knn(nq, queries.data(), R), wl);
    if (qadc_adc_index_destroy(index) != QADC_OK) ++bad;

    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    write_result(out, gk);
    write_result(out, gr);
    write_result(out, gp);
    std::fwrite(&gr.missing, 8, 1, out);
    std::fwrite(&gp.missing, 8, 1, out);
    std::fclose(out);
    if (bad) {
        std::cout << "FAIL " << bad << std::endl;
        return 1;
    }
    std::cout << "ok " << nq << std::endl;
    return 0;
}
