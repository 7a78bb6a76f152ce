// Demo of the reconstruction mirrors of host/db_build.hpp — pq_decode_hip and reconstruct_hip — for tests/test_gpu_reconstruct_cpp.py:
// an 8-bit IVF index is built with qadc_adc_index_add_vectors_labelled, its keys are looked up and decoded on the GPU, and the demo
// itself holds the result to the CPU twin (host/pq_decode.hpp: reconstruct_where on the index read back, then pq_decode).
//   reconstruct_demo IN OUT   IN: int32 {dim, sq_count, K, rotated, n, count}, codebooks [sq_count][256][dsub], rotation [dim][dim]
//                             when rotated, coarse [K][dim], vectors [n][dim], labels [n] uint32, keys [count] uint32;
//                             OUT: vectors [count][dim] float32, where [count] uint64, then err [n] float32 of pq_decode_hip on the
//                             index's own rows in partition order against zeros;  prints "ok <count>"
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
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

static void check(int rc, const char* what) {
    if (rc != QADC_OK) throw std::runtime_error(std::string(what) + ": " + qadc_last_error());
}

int main(int argc, char** argv) {
    try {
        if (argc != 3) return 2;
        std::ifstream f(argv[1], std::ios_base::in | std::ios_base::binary);
        if (!f) throw std::runtime_error("cannot open the input");
        const std::vector<std::int32_t> h = take<std::int32_t>(f, 6);
        const int dim = h[0], nsq = h[1], K = h[2];
        const bool rotated = h[3] != 0;
        const size_t n = (size_t)h[4], count = (size_t)h[5];
        const std::vector<float> cb = take<float>(f, (size_t)256 * dim), rot = take<float>(f, rotated ? (size_t)dim * dim : 0);
        const std::vector<float> coarse = take<float>(f, (size_t)K * dim), vecs = take<float>(f, n * dim);
        const std::vector<std::uint32_t> labels = take<std::uint32_t>(f, n), keys = take<std::uint32_t>(f, count);

        qadc_adc_index* idx = nullptr;
        check(qadc_adc_index_create(&idx, nsq, 8, 0), "create");
        check(qadc_adc_index_set_pq(idx, dim, cb.data()), "set_pq");
        if (rotated) check(qadc_adc_index_set_rotation(idx, rot.data()), "set_rotation");
        check(qadc_adc_index_set_coarse(idx, K, coarse.data()), "set_coarse");
        check(qadc_adc_index_add_vectors_labelled(idx, vecs.data(), labels.data(), n, 1), "add_vectors_labelled");

        std::vector<std::uint64_t> where;
        const std::vector<float> got = qadc::reconstruct_hip(idx, dim, keys.data(), count, &where);

        // the twin: the index read back, the lookup, the decode
        std::vector<std::uint32_t> sizes((size_t)K);
        std::vector<std::vector<std::uint8_t>> codes((size_t)K);
        std::vector<std::vector<std::uint32_t>> labs((size_t)K);
        std::vector<const std::uint32_t*> lab_ptr((size_t)K);
        for (int p = 0; p < K; ++p) {
            sizes[p] = qadc_adc_index_partition_size(idx, p);
            codes[p].resize((size_t)sizes[p] * nsq);
            labs[p].resize(sizes[p]);
            check(qadc_adc_index_read_partition(idx, p, 0, sizes[p], codes[p].data(), labs[p].data()), "read_partition");
            lab_ptr[p] = labs[p].data();
        }
        std::vector<std::uint32_t> base((size_t)K, 0);
        std::vector<std::uint64_t> want_where(count);
        qadc::reconstruct_where((size_t)K, sizes.data(), lab_ptr.data(), base.data(), keys.data(), count, want_where.data());
        if (want_where != where) throw std::runtime_error("where differs from the twin");
        std::vector<std::uint8_t> rows(count * nsq, 0);
        std::vector<std::int32_t> assign(count, -1);
        for (size_t i = 0; i < count; ++i)
            if (where[i] != QADC_RECONSTRUCT_MISSING) {
                assign[i] = (std::int32_t)(where[i] >> 32);
                std::memcpy(&rows[i * nsq], &codes[where[i] >> 32][(where[i] & 0xffffffffu) * nsq], nsq);
            }
        std::vector<float> want(count * dim);
        qadc::pq_decode(nsq, 8, dim, cb.data(), rotated ? rot.data() : nullptr, K, coarse.data(), assign.data(), rows.data(), count, nullptr,
                        want.data(), nullptr);
        if (std::memcmp(want.data(), got.data(), want.size() * sizeof(float)) != 0) throw std::runtime_error("vectors differ from the twin");

        // the stateless mirror on the index's own rows, partition by partition, with the error against zeros
        std::vector<float> err_all;
        const std::vector<float> zeros(n * dim, 0.0f);
        for (int p = 0; p < K; ++p) {
            const std::vector<std::int32_t> a(sizes[p], p);
            std::vector<float> err, err_want(sizes[p]), out_want((size_t)sizes[p] * dim);
            const std::vector<float> out = qadc::pq_decode_hip(nsq, 8, dim, cb.data(), rotated ? rot.data() : nullptr, K, coarse.data(), a.data(),
                                                               codes[p].data(), sizes[p], zeros.data(), &err);
            qadc::pq_decode(nsq, 8, dim, cb.data(), rotated ? rot.data() : nullptr, K, coarse.data(), a.data(), codes[p].data(), sizes[p],
                            zeros.data(), out_want.data(), err_want.data());
            if (out.size() != out_want.size() || (out.size() && std::memcmp(out.data(), out_want.data(), out.size() * sizeof(float)) != 0) ||
                (err.size() && std::memcmp(err.data(), err_want.data(), err.size() * sizeof(float)) != 0))
                throw std::runtime_error("pq_decode_hip differs from the twin");
            err_all.insert(err_all.end(), err.begin(), err.end());
        }
        check(qadc_adc_index_destroy(idx), "destroy");

        std::ofstream o(argv[2], std::ios_base::out | std::ios_base::binary);
        put(o, got);
        put(o, where);
        put(o, err_all);
        if (!o) throw std::runtime_error("cannot write the output");
        std::cout << "ok " << count << std::endl;
        return 0;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
