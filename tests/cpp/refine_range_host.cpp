// TEST DRIVER (CPU only): the host twin of the exact range search (refine::range and refine::rerank_range of host/refine.hpp) — the
// written definition of qadc_refine_range and qadc_refine_rerank_range (include/qadc.h) — over a dense or a
// keyed store of floats, halves or SQ8 bytes whose life is a script read from a file.  tests/test_refine_range_host.py compares the
// outputs, bit for bit, with a numpy restatement; the GPU tests compare the library with these outputs.  Beside every range the
// driver writes the twin's rerank_range fed every held key that passes the filter (from a key list it keeps itself, last key first)
// and the twin's knn at R = max(1, keys held); beside every rerank_range the twin's rerank of the same candidates, padded to the
// longest segment, at R = that length.  C++14, header only.
//   usage: refine_range_host IN OUT
//   IN : int32 ncases, then per case int32 keyed (0 dense, 1 keyed), dim, dtype (0 f32, 1 f16, 2 sq8), nops | sq8: float vmin [dim],
//        step [dim]; then per operation int32 kind and
//        0 add         : uint32 first_key, count | float vectors [count][dim]                      (dense)
//        1 put         : uint64 count | uint32 labels [count] | float vectors [count][dim]         (keyed)
//        2 remove      : uint64 count | uint32 labels [count]                                      (keyed)
//        3 range       : int32 nq, fmode (-1 no filter, 0 exclude, 1 allow) | uint64 nf | float queries [nq][dim] | float radius [nq]
//                        | uint32 fkeys [nf]
//        4 rerank_range: int32 nq | uint64 in_lims [nq + 1] | float queries [nq][dim] | float radius [nq] | uint32 keys [in_lims[nq]]
//   OUT: per range         uint64 lims [nq + 1] | uint32 keys | float dist;  the same three of the rerank_range | uint64 missing;
//                          int32 R | uint32 keys [nq][R] | float dist [nq][R] | int32 sizes [nq] of the knn
//        per rerank_range  uint64 lims [nq + 1] | uint32 keys | float dist | uint64 missing;
//                          int32 R | uint32 keys [nq][R] | float dist [nq][R] | int32 sizes [nq] | uint64 missing of the rerank
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <set>
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

template <typename T>
static void write_vec(std::FILE* f, const std::vector<T>& v) {
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}

static void write_csr(std::FILE* out, const std::vector<std::uint64_t>& lims, const std::vector<std::uint32_t>& keys, const std::vector<float>& dist) {
    write_vec(out, lims);
    write_vec(out, keys);
    write_vec(out, dist);
}

template <typename Store>
static void range_op(const Store& st, const std::set<std::uint32_t>& held, std::FILE* in, std::FILE* out) {
    std::vector<std::int32_t> head;
    std::vector<std::uint64_t> nf;
    std::vector<float> queries, radius;
    refine::filter f;
    read_vec(in, head, 2);
    read_vec(in, nf, 1);
    const int nq = head[0], fmode = head[1];
    read_vec(in, queries, (std::size_t)nq * st.dim);
    read_vec(in, radius, (std::size_t)nq);
    read_vec(in, f.keys, (std::size_t)nf[0]);
    f.mode = fmode == 1 ? refine::kFilterAllow : refine::kFilterExclude;
    std::sort(f.keys.begin(), f.keys.end());
    std::vector<std::uint64_t> lims;
    std::vector<std::uint32_t> ok;
    std::vector<float> od;
    refine::range(st, nq, queries.data(), radius.data(), fmode < 0 ? nullptr : &f, lims, ok, od);
    write_csr(out, lims, ok, od);

    // rerank_range, fed the keys this driver counted as held and passing, last key first
    const std::set<std::uint32_t> listed(f.keys.begin(), f.keys.end());
    std::vector<std::uint32_t> pass;
    for (auto it = held.rbegin(); it != held.rend(); ++it)
        if (fmode < 0 || (listed.count(*it) != 0) == (fmode == 1)) pass.push_back(*it);
    std::vector<std::uint64_t> in_lims((std::size_t)nq + 1);
    std::vector<std::uint32_t> keys;
    for (int q = 0; q < nq; ++q) {
        in_lims[q + 1] = in_lims[q] + pass.size();
        keys.insert(keys.end(), pass.begin(), pass.end());
    }
    in_lims[0] = 0;
    const std::uint64_t missing = refine::rerank_range(st, nq, queries.data(), in_lims.data(), keys.data(), radius.data(), lims, ok, od);
    write_csr(out, lims, ok, od);
    std::fwrite(&missing, 8, 1, out);

    const std::int32_t R = (std::int32_t)std::max<std::size_t>(1, held.size());
    std::vector<std::uint32_t> kk((std::size_t)nq * R);
    std::vector<float> kd((std::size_t)nq * R);
    std::vector<std::int32_t> ks(nq);
    refine::knn(st, nq, queries.data(), R, fmode < 0 ? nullptr : &f, kk.data(), kd.data(), ks.data());
    std::fwrite(&R, 4, 1, out);
    write_vec(out, kk);
    write_vec(out, kd);
    write_vec(out, ks);
}

template <typename Store>
static void rerank_range_op(const Store& st, std::FILE* in, std::FILE* out) {
    std::vector<std::int32_t> head;
    std::vector<std::uint64_t> in_lims;
    std::vector<float> queries, radius;
    std::vector<std::uint32_t> keys;
    read_vec(in, head, 1);
    const int nq = head[0];
    read_vec(in, in_lims, (std::size_t)nq + 1);
    read_vec(in, queries, (std::size_t)nq * st.dim);
    read_vec(in, radius, (std::size_t)nq);
    read_vec(in, keys, (std::size_t)in_lims[nq]);
    std::vector<std::uint64_t> lims;
    std::vector<std::uint32_t> ok;
    std::vector<float> od;
    std::uint64_t missing = refine::rerank_range(st, nq, queries.data(), in_lims.data(), keys.data(), radius.data(), lims, ok, od);
    write_csr(out, lims, ok, od);
    std::fwrite(&missing, 8, 1, out);

    std::uint64_t longest = 1;
    for (int q = 0; q < nq; ++q) longest = std::max(longest, in_lims[q + 1] - in_lims[q]);
    const std::int32_t R = (std::int32_t)longest;
    std::vector<std::uint32_t> padded((std::size_t)nq * R, 0u), rk((std::size_t)nq * R);
    std::vector<std::int32_t> counts(nq), rs(nq);
    std::vector<float> rd((std::size_t)nq * R);
    for (int q = 0; q < nq; ++q) {
        counts[q] = (std::int32_t)(in_lims[q + 1] - in_lims[q]);
        std::copy(keys.begin() + in_lims[q], keys.begin() + in_lims[q + 1], padded.begin() + (std::size_t)q * R);
    }
    missing = refine::rerank(st, nq, queries.data(), R, padded.data(), counts.data(), nullptr, R, rk.data(), rd.data(), rs.data());
    std::fwrite(&R, 4, 1, out);
    write_vec(out, rk);
    write_vec(out, rd);
    write_vec(out, rs);
    std::fwrite(&missing, 8, 1, out);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::cerr << "usage: refine_range_host IN OUT" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<std::int32_t> head;
    read_vec(in, head, 1);
    for (int c = 0, ncases = head[0]; c < ncases; ++c) {
        read_vec(in, head, 4);
        const bool keyed = head[0] != 0;
        const int dim = head[1], dtype = head[2], nops = head[3];
        std::unique_ptr<refine::store> dense;
        std::unique_ptr<refine::keyed_store> map;
        if (dtype == refine::kSQ8) {
            std::vector<float> vmin, step;
            read_vec(in, vmin, (std::size_t)dim);
            read_vec(in, step, (std::size_t)dim);
            dense.reset(new refine::store(dim, vmin.data(), step.data()));
            map.reset(new refine::keyed_store(dim, vmin.data(), step.data()));
        } else {
            dense.reset(new refine::store(dim, dtype));
            map.reset(new refine::keyed_store(dim, dtype));
        }
        std::set<std::uint32_t> held;
        for (int op = 0; op < nops; ++op) {
            read_vec(in, head, 1);
            const int kind = head[0];
            std::vector<std::uint32_t> labels;
            std::vector<std::uint64_t> n;
            std::vector<float> vec;
            if (kind == 0 && !keyed) {
                read_vec(in, labels, 2);
                read_vec(in, vec, (std::size_t)labels[1] * dim);
                if (!dense->add(vec.data(), labels[1], labels[0])) return 3;
                for (std::uint32_t i = 0; i < labels[1]; ++i) held.insert(labels[0] + i);
            } else if (kind == 1 && keyed) {
                read_vec(in, n, 1);
                read_vec(in, labels, (std::size_t)n[0]);
                read_vec(in, vec, (std::size_t)n[0] * dim);
                if (!map->put(vec.data(), labels.data(), n[0])) return 3;
                held.insert(labels.begin(), labels.end());
            } else if (kind == 2 && keyed) {
                read_vec(in, n, 1);
                read_vec(in, labels, (std::size_t)n[0]);
                map->remove(labels.data(), n[0]);
                for (std::uint32_t k : labels) held.erase(k);
            } else if (kind == 3) {
                if (keyed)
                    range_op(*map, held, in, out);
                else
                    range_op(*dense, held, in, out);
            } else if (kind == 4) {
                if (keyed)
                    rerank_range_op(*map, in, out);
                else
                    rerank_range_op(*dense, in, out);
            } else {
                std::cerr << "unknown operation " << kind << std::endl;
                return 2;
            }
        }
    }
    std::fclose(in);
    std::fclose(out);
    std::cout << "ok" << std::endl;
    return 0;
}
