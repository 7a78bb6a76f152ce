// db_add into the 4-bit index (host/db_build.hpp: db_add_hip(qadc_index*, ...)): streams a .fvecs / .bvecs file through
// io::vectors_reader in chunks, every chunk encoded and appended on the GPU by qadc_index_add_vectors, then writes every partition
// out as qadc_index_read_partition returns it (tests/test_gpu_index_add_cpp.py compares with the Python route).
//   db_add4_demo <quantizers> <base file> <chunk_count> <out>
//   quantizers: int32 nsq, bits (4), dim, K, opq | float codebooks[nsq][16][dim / nsq] | float coarse[K][dim] | float rotation[dim][dim] if opq
//   out       : int32 parts, labelled | parts x { uint32 size | codes[size][nsq / 2] | uint32 labels[size] if labelled }
// stdout: "ok <vectors added>".
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "../../quick-adc_amd/host/db_build.hpp"

template <typename T>
static bool get(FILE* f, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T>
static bool put(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

static void check(int rc, const char* what) {
    if (rc != QADC_OK) throw std::runtime_error(std::string(what) + ": " + qadc_last_error());
}

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    qadc_index* idx = nullptr;
    try {
        FILE* in = fopen(argv[1], "rb");
        std::vector<int32_t> head(5);
        if (!in || !get(in, head)) return 3;
        const int nsq = head[0], bits = head[1], dim = head[2], K = head[3], opq = head[4];
        if (bits != 4) return 3;
        std::vector<float> codebooks((size_t)nsq * 16 * (dim / nsq)), coarse((size_t)K * dim), rotation(opq ? (size_t)dim * dim : 0);
        if (!get(in, codebooks) || !get(in, coarse) || !get(in, rotation)) return 3;
        fclose(in);
        check(qadc_index_create(&idx, nsq, 0), "create");
        check(qadc_index_set_pq(idx, dim, codebooks.data()), "set_pq");
        if (opq) check(qadc_index_set_rotation(idx, rotation.data()), "set_rotation");
        if (K) check(qadc_index_set_coarse(idx, K, coarse.data()), "set_coarse");
        const unsigned added = qadc::db_add_hip(idx, dim, argv[2], (unsigned)atoi(argv[3]));
        FILE* out = fopen(argv[4], "wb");
        const int parts = qadc_index_partition_count(idx), labelled = K > 0;
        const size_t cs = (size_t)nsq / 2;
        if (!out || !put(out, std::vector<int32_t>{parts, labelled})) return 4;
        for (int p = 0; p < parts; ++p) {
            const uint32_t size = qadc_index_partition_size(idx, p);
            std::vector<uint8_t> codes(size * cs);
            std::vector<uint32_t> labels(labelled ? size : 0);
            check(qadc_index_read_partition(idx, p, 0, size, codes.data(), labelled ? labels.data() : nullptr), "read_partition");
            if (!put(out, std::vector<uint32_t>{size}) || !put(out, codes) || !put(out, labels)) return 4;
        }
        if (fclose(out) != 0) return 4;
        check(qadc_index_destroy(idx), "destroy");
        printf("ok %u\n", added);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        qadc_index_destroy(idx);
        return 1;
    }
}
