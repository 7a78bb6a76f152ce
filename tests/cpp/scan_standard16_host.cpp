// TEST DRIVER (CPU only): the host twin's scanner_simple over scan_standard<uint16_t, NSQ> (host/scanner_simple.hpp) on one case of
// tests/golden/ref_scan_standard_u16_cases.npz; the test (tests/test_adc16_host.py) compares the heap's arrays with the reference's,
// bit for bit.  C++14, header only.
//   usage: scan_standard16_host IN OUT [REPEAT]
// REPEAT (tools/adc_bench.py --bits 16): the scan is run that many times more on fresh heaps, one thread, and the median wall
// time of a query_scan call is printed as "us <microseconds>" after "ok".
//   IN : int32 nsq, nparts, labelled, R, sum_mode | uint32 sizes [nparts] | per partition: uint16 codes [size][nsq], then (labelled)
//        uint32 labels [size] | float tables [nparts][nsq * 65536]                (the probes are the partitions in order)
//   OUT: int32 heap size | uint32 keys [size] | float values [size]
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
    std::vector<std::vector<std::uint16_t>> parts;
    std::vector<std::vector<unsigned>> labels;
    void get_partition(int i, const std::uint8_t*& c, unsigned*& l, unsigned& size) {
        c = reinterpret_cast<const std::uint8_t*>(parts[i].data());
        l = labels[i].empty() ? nullptr : labels[i].data();
        size = (unsigned)(parts[i].size() / pq->sq_count);
    }
};

struct no_metrics {};

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) {
        std::cerr << "usage: scan_standard16_host IN OUT [REPEAT]" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<std::int32_t> head;
    read_vec(in, head, 5);
    const int nsq = head[0], nparts = head[1], labelled = head[2], r = head[3];
    float_sum_mode() = head[4];
    std::vector<std::uint32_t> sizes;
    read_vec(in, sizes, nparts);
    parts_db db;
    db.pq.reset(new pq_bytes(nsq, 16, nsq));
    db.parts.resize(nparts);
    db.labels.resize(nparts);
    for (int p = 0; p < nparts; ++p) {
        read_vec(in, db.parts[p], (std::size_t)sizes[p] * nsq);
        if (labelled) read_vec(in, db.labels[p], sizes[p]);
    }
    std::vector<float> tables;
    read_vec(in, tables, (std::size_t)nparts * db.pq->table_dim());
    std::fclose(in);

    scanner_simple<parts_db> sc;
    sc.prepare_database(db);                           // get_scan_func: scan_standard<uint16_t, nsq>
    std::vector<int> assign(nparts);
    for (int p = 0; p < nparts; ++p) assign[p] = p;
    float_heap bh(r);
    no_metrics m;
    sc.query_scan(nullptr, assign.data(), nparts, tables.data(), db.pq->table_dim(), bh, m);

    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    const std::int32_t n = bh.size();
    std::fwrite(&n, 4, 1, out);
    std::fwrite(bh.keys(), sizeof(unsigned), n, out);
    std::fwrite(bh.values(), sizeof(float), n, out);
    std::fclose(out);
    std::cout << "ok" << std::endl;
    if (argc == 4) {
        std::vector<double> us;
        for (int i = 0; i < std::atoi(argv[3]); ++i) {
            float_heap again(r);
            const auto t0 = std::chrono::steady_clock::now();
            sc.query_scan(nullptr, assign.data(), nparts, tables.data(), db.pq->table_dim(), again, m);
            us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
            if (again.size() != bh.size()) return 3;
        }
        std::sort(us.begin(), us.end());
        if (!us.empty()) std::cout << "us " << us[us.size() / 2] << std::endl;
    }
    return 0;
}
