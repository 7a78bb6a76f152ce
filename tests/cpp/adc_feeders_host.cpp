// TEST DRIVER (CPU only): the host twin of the float-ADC feeders — pq_bytes with the OPQ rotation (host/scanner_simple.hpp) under
// flat_database_t / ivf_database_t and nns_engine (host/query_driver.hpp).  Reads one case, writes what the twin computes; the test
// (tests/test_adc_feeders_host.py) compares every array with the composition of the oracle's functions.  C++14, header only.
//   usage: adc_feeders_host IN OUT
//   IN : int32 nsq, dim, K (0 = flat), opq, nq, ma, n, R | float codebooks [nsq][256][dim/nsq] | rotation [dim][dim] (opq) |
//        coarse [K][dim] (K > 0) | queries [nq][dim] | vectors [n][dim]
//   OUT: int32 partition of every vector [n] | uint8 codes [n][nsq] | int32 assign [nq][ma] | float direct tables [nq][ma][nsq*256] |
//        float expansion tables [nq][ma][nsq*256] | int32 heap sizes [nq] | uint32 heap keys [nq][R] | float heap values [nq][R]
//        (the heaps of nns_engine + scanner_simple: direct tables for ma == 1, expansion tables otherwise)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <vector>

#include "../../quick-adc_amd/host/query_driver.hpp"
#include "../../quick-adc_amd/host/scanner_simple.hpp"

using namespace qadc;

struct Case {
    std::int32_t nsq, dim, K, opq, nq, ma, n, R;
    std::vector<float> queries, vectors;
};

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
    if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
        std::cerr << "short output" << std::endl;
        std::exit(2);
    }
}

// the codes of every vector in input order, from a database that files them by partition
static void collect(flat_database_t<pq_bytes>& db, const Case& c, std::vector<std::int32_t>& part, std::vector<std::uint8_t>& codes) {
    part.assign(c.n, 0);
    codes = db.codes;
}
static void collect(ivf_database_t<pq_bytes>& db, const Case& c, std::vector<std::int32_t>& part, std::vector<std::uint8_t>& codes) {
    part.assign(c.n, -1);
    codes.assign((std::size_t)c.n * c.nsq, 0);
    for (int p = 0; p < db.part_count; ++p)
        for (std::size_t j = 0; j < db.labels[p].size(); ++j) {
            const unsigned i = db.labels[p][j];
            part[i] = p;
            for (int m = 0; m < c.nsq; ++m) codes[(std::size_t)i * c.nsq + m] = db.partitions[p][j * c.nsq + m];
        }
}

static void add_all(flat_database_t<pq_bytes>& db, const Case& c) { db.add_vectors(c.vectors.data(), (unsigned)c.n); }
static void add_all(ivf_database_t<pq_bytes>& db, const Case& c) { db.add_vectors(c.vectors.data(), (unsigned)c.n, 0); }

template <typename Db>
static void run(Db& db, const Case& c, std::FILE* out) {
    add_all(db, c);
    std::vector<std::int32_t> part;
    std::vector<std::uint8_t> codes;
    collect(db, c, part, codes);
    write_vec(out, part);
    write_vec(out, codes);

    const int td = db.pq->table_dim();
    std::vector<std::int32_t> assign((std::size_t)c.nq * c.ma);
    std::vector<float> res((std::size_t)c.ma * c.dim), direct((std::size_t)c.nq * c.ma * td), expansion(direct.size());
    for (int q = 0; q < c.nq; ++q) {
        int* a = assign.data() + (std::size_t)q * c.ma;
        db.assign_compute_residuals(c.queries.data() + (std::size_t)q * c.dim, c.ma, a, res.data());
        db.pq->rotate_multiple_vectors(res.data(), c.ma);
        for (int p = 0; p < c.ma; ++p)
            db.pq->tables_direct(res.data() + (std::size_t)p * c.dim, direct.data() + ((std::size_t)q * c.ma + p) * td);
        db.pq->tables_blas(res.data(), c.ma, expansion.data() + (std::size_t)q * c.ma * td);
    }
    write_vec(out, assign);
    write_vec(out, direct);
    write_vec(out, expansion);

    scanner_simple<Db> scanner;
    nns_engine<Db, scanner_simple<Db>> engine(scanner, db, c.ma);
    engine.prepare_database();
    std::vector<std::int32_t> sizes(c.nq);
    std::vector<std::uint32_t> keys((std::size_t)c.nq * c.R, 0);
    std::vector<float> vals((std::size_t)c.nq * c.R, 0.0f);
    for (int q = 0; q < c.nq; ++q) {
        float_heap bh(c.R);
        query_metrics m;
        engine.process_query(c.queries.data() + (std::size_t)q * c.dim, bh, m);
        sizes[q] = bh.size();
        for (int i = 0; i < bh.size(); ++i) {
            keys[(std::size_t)q * c.R + i] = bh.keys()[i];
            vals[(std::size_t)q * c.R + i] = bh.values()[i];
        }
    }
    write_vec(out, sizes);
    write_vec(out, keys);
    write_vec(out, vals);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::cerr << "usage: adc_feeders_host IN OUT" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) {
        std::cerr << "cannot open the files" << std::endl;
        return 2;
    }
    Case c;
    std::vector<std::int32_t> head;
    read_vec(in, head, 8);
    c.nsq = head[0]; c.dim = head[1]; c.K = head[2]; c.opq = head[3]; c.nq = head[4]; c.ma = head[5]; c.n = head[6]; c.R = head[7];
    std::unique_ptr<pq_bytes> pq(new pq_bytes(c.nsq, 8, c.dim));
    read_vec(in, pq->centroids, (std::size_t)c.nsq * 256 * (c.dim / c.nsq));
    if (c.opq) read_vec(in, pq->rotation, (std::size_t)c.dim * c.dim);
    std::vector<float> coarse;
    read_vec(in, coarse, (std::size_t)c.K * c.dim);
    read_vec(in, c.queries, (std::size_t)c.nq * c.dim);
    read_vec(in, c.vectors, (std::size_t)c.n * c.dim);
    std::fclose(in);
    if (c.K > 0) {
        ivf_database_t<pq_bytes> db(std::move(pq), c.K, coarse);
        run(db, c, out);
    } else {
        flat_database_t<pq_bytes> db;
        db.pq = std::move(pq);
        run(db, c, out);
    }
    std::fclose(out);
    std::cout << "ok" << std::endl;
    return 0;
}
