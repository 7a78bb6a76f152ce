// refine_store_hip::range and ::rerank_range (quick-adc_amd/host/refine_hip.hpp) — the C++14 mirrors of qadc_refine_range and
// qadc_refine_rerank_range — beside the host twins refine::range and refine::rerank_range (host/refine.hpp)
// on a store read from a file: lims, keys, the distances' bits and the missing count must be identical, with the plan's default and
// with regions of 16 words, chunks of 64 rows and passes of 3 queries.  The candidates of rerank_range are the exhaustive result
// under twice the radius, every third key listed twice and two keys no store holds in front of every segment.  The mirrors' results
// are written out, so that tests/test_gpu_refine_range_cpp.py can compare them with the Python calls on the same data.  C++14.
//   usage: refine_range_hip_demo IN OUT
//   IN : int32 dim, dtype (0 f32, 1 f16), keyed, n, nq, fmode (-1 no filter, 0 exclude, 1 allow), nf |
//        uint32 labels [n] (dense: labels[0] is the first key) | float vectors [n][dim] | float queries [nq][dim] | float radius [nq] |
//        uint32 fkeys [nf]
//   OUT: range: uint64 lims [nq + 1] | uint32 keys | float dist;  rerank_range: uint64 in_lims [nq + 1] | uint32 in_keys |
//        uint64 lims [nq + 1] | uint32 keys | float dist | uint64 missing
// Prints "ok <queries> <rows>" and exits 0 when everything agrees.
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

template <typename T>
static void write_vec(std::FILE* f, const std::vector<T>& v) {
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}

static bool same(const refine_range_result& a, const std::vector<std::uint64_t>& l, const std::vector<std::uint32_t>& k, const std::vector<float>& d,
                 std::uint64_t missing) {
    return a.lims == l && a.keys == k && a.dist.size() == d.size() && a.missing == missing &&
           (d.empty() || std::memcmp(a.dist.data(), d.data(), sizeof(float) * d.size()) == 0);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::cerr << "usage: refine_range_hip_demo IN OUT" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<std::int32_t> head;
    read_vec(in, head, 7);
    const int dim = head[0], dtype = head[1], n = head[3], nq = head[4], fmode = head[5], nf = head[6];
    const bool keyed = head[2] != 0;
    std::vector<std::uint32_t> labels, fkeys;
    std::vector<float> vectors, queries, radius;
    read_vec(in, labels, n);
    read_vec(in, vectors, (std::size_t)n * dim);
    read_vec(in, queries, (std::size_t)nq * dim);
    read_vec(in, radius, nq);
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
    std::vector<std::uint64_t> wl, xl;
    std::vector<std::uint32_t> wk, xk;
    std::vector<float> wd, xd;
    if (keyed)
        refine::range(map, nq, queries.data(), radius.data(), fmode >= 0 ? &tf : nullptr, wl, wk, wd);
    else
        refine::range(dense, nq, queries.data(), radius.data(), fmode >= 0 ? &tf : nullptr, wl, wk, wd);

    int bad = 0;
    const refine_range_result got = gpu.range(nq, queries.data(), radius.data(), filter);
    if (!same(got, wl, wk, wd, 0)) {
        std::cerr << "range: the mirror and the twin differ" << std::endl;
        ++bad;
    }
    gpu.set_range_plan(16, 64, 3);
    const std::uint64_t before = gpu.range_reruns();
    if (!same(gpu.range(nq, queries.data(), radius.data(), filter), wl, wk, wd, 0)) {
        std::cerr << "range: the mirror and the twin differ with regions of 16 words and chunks of 64 rows" << std::endl;
        ++bad;
    }
    bool overflows = false;
    for (int q = 0; q < nq; ++q) overflows = overflows || wl[q + 1] - wl[q] > 16;
    if ((gpu.range_reruns() != before) != overflows) {
        std::cerr << "range: the re-run counter moved without an overflow, or stayed with one" << std::endl;
        ++bad;
    }
    if (filter && qadc_adc_filter_destroy(filter) != QADC_OK) ++bad;   // (no use was counted on it)

    // the candidates: the exhaustive result under twice the radius (no filter), repeats and misses mixed in
    std::vector<float> wide(radius);
    for (float& r : wide) r = r * 2.0f;
    gpu.set_range_plan(0, 0, 0);
    const refine_range_result all = gpu.range(nq, queries.data(), wide.data());
    std::vector<std::uint64_t> in_lims(1, 0);
    std::vector<std::uint32_t> in_keys;
    for (int q = 0; q < nq; ++q) {
        in_keys.push_back(0xFFFFFFFFu);
        in_keys.push_back(0xFFFFFFF0u);
        for (std::uint64_t i = all.lims[q + 1]; i > all.lims[q]; --i) {
            in_keys.push_back(all.keys[i - 1]);
            if (i % 3 == 0) in_keys.push_back(all.keys[i - 1]);
        }
        in_lims.push_back(in_keys.size());
    }
    const std::uint64_t missing = keyed ? refine::rerank_range(map, nq, queries.data(), in_lims.data(), in_keys.data(), radius.data(), xl, xk, xd)
                                        : refine::rerank_range(dense, nq, queries.data(), in_lims.data(), in_keys.data(), radius.data(), xl, xk, xd);
    const refine_range_result rr = gpu.rerank_range(nq, queries.data(), in_lims.data(), in_keys.data(), radius.data());
    if (!same(rr, xl, xk, xd, missing)) {
        std::cerr << "rerank_range: the mirror and the twin differ" << std::endl;
        ++bad;
    }
    gpu.set_range_plan(0, 0, 3);
    if (!same(gpu.rerank_range(nq, queries.data(), in_lims.data(), in_keys.data(), radius.data()), xl, xk, xd, missing)) {
        std::cerr << "rerank_range: the mirror and the twin differ in passes of 3 queries" << std::endl;
        ++bad;
    }

    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    write_vec(out, got.lims);
    write_vec(out, got.keys);
    write_vec(out, got.dist);
    write_vec(out, in_lims);
    write_vec(out, in_keys);
    write_vec(out, rr.lims);
    write_vec(out, rr.keys);
    write_vec(out, rr.dist);
    std::fwrite(&rr.missing, 8, 1, out);
    std::fclose(out);
    if (bad) {
        std::cout << "FAIL " << bad << std::endl;
        return 1;
    }
    std::cout << "ok " << nq << " " << got.keys.size() << std::endl;
    return 0;
}
