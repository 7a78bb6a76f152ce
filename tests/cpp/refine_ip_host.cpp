// TEST DRIVER (CPU only): the host twin of the inner-product metric (refine::rerank, ::knn and ::knn_probed of host/refine.hpp with a
// metric argument; include/qadc.h, qadc_refine_set_metric) over a dense or a keyed store of float, half or
// SQ8 rows, read from a file.  tests/test_refine_ip_host.py compares the outputs, bit for bit, with a numpy restatement
// (tests/refine_ip_cases.py); the GPU tests compare the library with these outputs.  Every operation names its metric, so that one
// store answers under both.  C++14, header only.
//   usage: refine_ip_host IN OUT            the cases of IN
//          refine_ip_host --images IN OUT   IN: uint32 bit patterns [n] -> OUT: uint32 img_ip [n], then uint32 bits of img_ip_inverse(img_ip) [n]
//   IN : int32 ncases, then per case int32 keyed (0 dense, 1 keyed), dim, dtype (0 f32, 1 f16, 2 sq8), nops | uint32 lo | uint64 n |
//        float vmin [dim], step [dim] (sq8 only) | uint32 labels [n] (keyed only) | float vectors [n][dim]   (dense: the keys lo ..),
//        then per operation int32 kind, metric (0 L2, 1 IP) and
//        0 rerank: int32 nq, r_in, R, has_counts, has_values | float queries [nq][dim] | uint32 keys [nq][r_in] | int32 counts [nq] |
//                  float values [nq][r_in]
//        1 knn   : int32 nq, R, fmode (-1 no filter, 0 exclude, 1 allow) | uint64 nf | float queries [nq][dim] | uint32 fkeys [nf]
//        2 probed: int32 nq, R, fmode, ma, nparts | uint64 nf | per partition uint64 rows, uint32 labels [rows] | int32 assign [nq][ma] |
//                  float queries [nq][dim] | uint32 fkeys [nf]
//   OUT: per operation uint64 missing (knn: 0) | uint32 keys [nq][R] | float dist [nq][R] | int32 sizes [nq]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
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

static void write_result(std::FILE* out, std::uint64_t missing, const std::vector<std::uint32_t>& ok, const std::vector<float>& od,
                         const std::vector<std::int32_t>& os) {
    std::fwrite(&missing, 8, 1, out);
    std::fwrite(ok.data(), 4, ok.size(), out);
    std::fwrite(od.data(), 4, od.size(), out);
    std::fwrite(os.data(), 4, os.size(), out);
}

static void read_filter(std::FILE* in, int fmode, std::size_t nf, refine::filter& f) {
    read_vec(in, f.keys, nf);
    f.mode = fmode == 1 ? refine::kFilterAllow : refine::kFilterExclude;
    std::sort(f.keys.begin(), f.keys.end());
}

template <typename Store>
static void run_ops(const Store& st, int nops, std::FILE* in, std::FILE* out) {
    for (int o = 0; o < nops; ++o) {
        std::vector<std::int32_t> head;
        read_vec(in, head, 2);
        const int kind = head[0], metric = head[1];
        std::vector<float> queries;
        std::vector<std::uint64_t> nf;
        refine::filter f;
        if (kind == 0) {
            read_vec(in, head, 5);
            const int nq = head[0], r_in = head[1], R = head[2];
            const bool has_counts = head[3] != 0, has_values = head[4] != 0;
            std::vector<std::uint32_t> keys;
            std::vector<std::int32_t> counts;
            std::vector<float> values;
            read_vec(in, queries, (std::size_t)nq * st.dim);
            read_vec(in, keys, (std::size_t)nq * r_in);
            if (has_counts) read_vec(in, counts, (std::size_t)nq);
            if (has_values) read_vec(in, values, (std::size_t)nq * r_in);
            std::vector<std::uint32_t> ok((std::size_t)nq * R);
            std::vector<float> od((std::size_t)nq * R);
            std::vector<std::int32_t> os(nq);
            const std::uint64_t missing = refine::rerank(st, nq, queries.data(), r_in, keys.data(), has_counts ? counts.data() : nullptr,
                                                         has_values ? values.data() : nullptr, R, ok.data(), od.data(), os.data(), metric);
            write_result(out, missing, ok, od, os);
        } else if (kind == 1) {
            read_vec(in, head, 3);
            read_vec(in, nf, 1);
            const int nq = head[0], R = head[1], fmode = head[2];
            read_vec(in, queries, (std::size_t)nq * st.dim);
            read_filter(in, fmode, (std::size_t)nf[0], f);
            std::vector<std::uint32_t> ok((std::size_t)nq * R);
            std::vector<float> od((std::size_t)nq * R);
            std::vector<std::int32_t> os(nq);
            refine::knn(st, nq, queries.data(), R, fmode < 0 ? nullptr : &f, ok.data(), od.data(), os.data(), metric);
            write_result(out, 0, ok, od, os);
        } else if (kind == 2) {
            read_vec(in, head, 5);
            read_vec(in, nf, 1);
            const int nq = head[0], R = head[1], fmode = head[2], ma = head[3], nparts = head[4];
            std::vector<std::vector<std::uint32_t>> labels((std::size_t)nparts);
            std::vector<refine::probe_part> parts((std::size_t)nparts);
            for (int p = 0; p < nparts; ++p) {
                std::vector<std::uint64_t> rows;
                read_vec(in, rows, 1);
                read_vec(in, labels[p], (std::size_t)rows[0]);
                static const std::uint32_t none = 0;   // (a partition without rows still has a label array)
                parts[p] = refine::probe_part{labels[p].empty() ? &none : labels[p].data(), 0u, rows[0]};
            }
            std::vector<std::int32_t> assign;
            read_vec(in, assign, (std::size_t)nq * ma);
            read_vec(in, queries, (std::size_t)nq * st.dim);
            read_filter(in, fmode, (std::size_t)nf[0], f);
            std::vector<std::uint32_t> ok((std::size_t)nq * R);
            std::vector<float> od((std::size_t)nq * R);
            std::vector<std::int32_t> os(nq);
            const std::uint64_t missing = refine::knn_probed(st, parts.data(), nparts, nullptr, nq, queries.data(), ma, assign.data(), R,
                                                             fmode < 0 ? nullptr : &f, ok.data(), od.data(), os.data(), metric);
            write_result(out, missing, ok, od, os);
        } else {
            std::cerr << "unknown operation " << kind << std::endl;
            std::exit(2);
        }
    }
}

static int images(const char* fin, const char* fout) {
    std::FILE* in = std::fopen(fin, "rb");
    std::FILE* out = std::fopen(fout, "wb");
    if (!in || !out) return 2;
    std::vector<std::uint32_t> bits, img, back;
    std::uint32_t b;
    while (std::fread(&b, 4, 1, in) == 1) bits.push_back(b);
    for (std::uint32_t u : bits) {
        img.push_back(refine::img_ip(refine::bits_float(u)));
        back.push_back(refine::float_bits(refine::img_ip_inverse(img.back())));
    }
    std::fwrite(img.data(), 4, img.size(), out);
    std::fwrite(back.data(), 4, back.size(), out);
    std::fclose(in);
    std::fclose(out);
    std::cout << "ok" << std::endl;
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[1], "--images") == 0) return images(argv[2], argv[3]);
    if (argc != 3) {
        std::cerr << "usage: refine_ip_host IN OUT | refine_ip_host --images IN OUT" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<std::int32_t> head;
    read_vec(in, head, 1);
    for (int c = 0, ncases = head[0]; c < ncases; ++c) {
        read_vec(in, head, 4);
        const int keyed = head[0], dim = head[1], dtype = head[2], nops = head[3];
        std::vector<std::uint32_t> lo, labels;
        std::vector<std::uint64_t> n;
        std::vector<float> vmin, step, vectors;
        read_vec(in, lo, 1);
        read_vec(in, n, 1);
        if (dtype == refine::kSQ8) {
            read_vec(in, vmin, (std::size_t)dim);
            read_vec(in, step, (std::size_t)dim);
        }
        if (keyed) read_vec(in, labels, (std::size_t)n[0]);
        read_vec(in, vectors, (std::size_t)n[0] * dim);
        if (keyed) {
            std::unique_ptr<refine::keyed_store> st(dtype == refine::kSQ8 ? new refine::keyed_store(dim, vmin.data(), step.data())
                                                                          : new refine::keyed_store(dim, dtype));
            if (!st->put(vectors.data(), labels.data(), n[0])) return 3;
            run_ops(*st, nops, in, out);
        } else {
            std::unique_ptr<refine::store> st(dtype == refine::kSQ8 ? new refine::store(dim, vmin.data(), step.data()) : new refine::store(dim, dtype));
            if (!st->add(vectors.data(), n[0], lo[0])) return 3;
            run_ops(*st, nops, in, out);
        }
    }
    std::fclose(in);
    std::fclose(out);
    std::cout << "ok" << std::endl;
    return 0;
}
