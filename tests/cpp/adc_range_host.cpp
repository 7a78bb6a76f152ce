// TEST DRIVER (CPU only): the host twin's scanner_simple::range_scan (host/scanner_simple.hpp) — the written definition of the
// qadc_adc_range_* calls (include/qadc.h): every row of the probed partitions whose key passes the index's
// filter and the query's and whose candidate is < radius, ascending by (order_image(candidate) << 32) | key.  The test
// (tests/test_adc_range_host.py) compares keys and value bits with a numpy restatement.  C++14, header only.
//   usage: adc_range_host IN OUT
//   IN : int32 ncases, then per case
//        int32 nsq, bits (4, 8 or 16), nparts, labelled, the radius' bits, sum_mode,
//              mode (0 exclude, 1 allow, -1: no filter) and nkeys of the index's filter, mode and nkeys of the query's
//        uint32 sizes [nparts] | per partition: code bytes [size][nsq * bits / 8], then (labelled) uint32 labels [size]
//        float tables [nparts][nsq << bits]                                    (the probes are the partitions in order)
//        uint32 keys [nkeys] of the index's filter | uint32 keys [nkeys] of the query's   (any order, duplicates legal)
//   OUT: per case int32 rows | uint32 keys [rows] | float values [rows]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <vector>

#include "../../quick-adc_amd/host/scanner_simple.hpp"

using namespace qadc;

template <typename T>
static void read_vec(std::FILE* f, std::vector<T>& v, std::size_t n) {
    v.resize(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) {
        std::cerr << "short input" << std::endl;
        std::exit(2);
    }
}

struct parts_db {
    std::unique_ptr<pq_bytes> pq;
    std::vector<std::vector<std::uint8_t>> parts;
    std::vector<std::vector<unsigned>> labels;
    std::vector<unsigned> sizes;
    void get_partition(int i, const std::uint8_t*& c, unsigned*& l, unsigned& size) {
        c = parts[i].data();
        l = labels[i].empty() ? nullptr : labels[i].data();
        size = sizes[i];
    }
};

int main(int argc, char** argv) {
    if (argc != 3) {
        std::cerr << "usage: adc_range_host IN OUT" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<std::int32_t> head;
    read_vec(in, head, 1);
    for (int c = 0, ncases = head[0]; c < ncases; ++c) {
        read_vec(in, head, 10);
        const int nsq = head[0], bits = head[1], nparts = head[2], labelled = head[3];
        const int mode1 = head[6], nkeys1 = head[7], mode2 = head[8], nkeys2 = head[9];
        float radius;
        std::memcpy(&radius, &head[4], 4);
        float_sum_mode() = head[5];
        parts_db db;
        db.pq.reset(new pq_bytes(nsq, bits, nsq));
        read_vec(in, db.sizes, nparts);
        db.parts.resize(nparts);
        db.labels.resize(nparts);
        for (int p = 0; p < nparts; ++p) {
            read_vec(in, db.parts[p], (std::size_t)db.sizes[p] * db.pq->code_size());
            if (labelled) read_vec(in, db.labels[p], db.sizes[p]);
        }
        std::vector<float> tables;
        read_vec(in, tables, (std::size_t)nparts * db.pq->table_dim());
        std::vector<unsigned> keys1, keys2;
        read_vec(in, keys1, nkeys1);
        read_vec(in, keys2, nkeys2);

        scanner_simple<parts_db> sc;
        sc.prepare_database(db);
        const key_filter of_index(mode1 == 1 ? key_filter::allow : key_filter::exclude, keys1.data(), keys1.size());
        const key_filter of_query(mode2 == 1 ? key_filter::allow : key_filter::exclude, keys2.data(), keys2.size());
        if (mode1 >= 0) sc.set_filter(&of_index);
        if (mode2 >= 0) sc.set_query_filter(&of_query);
        std::vector<int> assign(nparts);
        for (int p = 0; p < nparts; ++p) assign[p] = p;
        range_result res;
        sc.range_scan(assign.data(), nparts, tables.data(), db.pq->table_dim(), radius, res);

        const std::int32_t n = (std::int32_t)res.keys.size();
        std::fwrite(&n, 4, 1, out);
        if (n) {
            std::fwrite(res.keys.data(), sizeof(unsigned), n, out);
            std::fwrite(res.values.data(), sizeof(float), n, out);
        }
    }
    std::fclose(in);
    std::fclose(out);
    std::cout << "ok" << std::endl;
    return 0;
}
