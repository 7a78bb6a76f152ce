// TEST DRIVER (CPU only): the host twin of the probed exact search (refine::knn_probed of host/refine.hpp) — the written definition of
// qadc_refine_knn_probed (include/qadc.h) — over a dense or a keyed store whose life is a script read from a
// file, and the partitions of an index given as key lists.  tests/test_refine_probe_host.py compares the outputs, bit for bit, with a
// numpy restatement; the GPU tests compare the library with these outputs.  Beside every call whose queries have at most 8192 entries
// each the driver writes the twin's rerank fed the entries, which it lists itself, last partition and last row first.  C++14, header only.
//   usage: refine_probe_host IN OUT
//   IN : int32 ncases, then per case int32 keyed (0 dense, 1 keyed), dim, dtype (0 f32, 1 f16, 2 sq8), nops, nparts, ncalls
//        | float vmin [dim], step [dim] (sq8), then
//        per operation int32 kind and
//          0 add   : uint32 first_key, count | float vectors [count][dim]                      (dense)
//          1 put   : uint64 count | uint32 labels [count] | float vectors [count][dim]         (keyed)
//          2 remove: uint64 count | uint32 labels [count]                                      (keyed)
//        per partition int32 labelled | uint32 key_base | uint64 rows | uint32 labels [rows] (labelled)
//        the index's filter: int32 mode (-1 none, 0 exclude, 1 allow) | uint64 n | uint32 keys [n]
//        per call int32 nq, ma, R, fmode | uint64 nf | float queries [nq][dim] | int32 assign [nq][ma] | uint32 fkeys [nf]
//   OUT: per call uint32 keys [nq][R] | float dist [nq][R] | int32 sizes [nq] | uint64 missing | int32 has_rerank, and with it the
//        same four of the rerank
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

static void read_filter(std::FILE* in, int mode, std::size_t n, refine::filter& f) {
    read_vec(in, f.keys, n);
    f.mode = mode == 1 ? refine::kFilterAllow : refine::kFilterExclude;
    std::sort(f.keys.begin(), f.keys.end());
}

static void write_result(std::FILE* out, const std::vector<std::uint32_t>& ok, const std::vector<float>& od, const std::vector<std::int32_t>& os,
                         std::uint64_t missing) {
    std::fwrite(ok.data(), 4, ok.size(), out);
    std::fwrite(od.data(), 4, od.size(), out);
    std::fwrite(os.data(), 4, os.size(), out);
    std::fwrite(&missing, 8, 1, out);
}

template <typename Store>
static void call_op(const Store& st, const std::vector<refine::probe_part>& parts, const refine::filter* ifilter, std::FILE* in, std::FILE* out) {
    std::vector<std::int32_t> head, assign;
    std::vector<std::uint64_t> nf;
    std::vector<float> queries;
    refine::filter f;
    read_vec(in, head, 4);
    read_vec(in, nf, 1);
    const int nq = head[0], ma = head[1], R = head[2], fmode = head[3], nparts = (int)parts.size();
    read_vec(in, queries, (std::size_t)nq * st.dim);
    read_vec(in, assign, (std::size_t)nq * ma);
    read_filter(in, fmode, (std::size_t)nf[0], f);
    std::vector<std::uint32_t> ok((std::size_t)nq * R);
    std::vector<float> od((std::size_t)nq * R);
    std::vector<std::int32_t> os(nq);
    const std::uint64_t missing = refine::knn_probed(st, parts.data(), nparts, ifilter, nq, queries.data(), ma, assign.data(), R,
                                                     fmode < 0 ? nullptr : &f, ok.data(), od.data(), os.data());
    write_result(out, ok, od, os, missing);

    // rerank, fed the entries this driver lists: the probed partitions as a set, descending, rows descending
    std::vector<std::vector<std::uint32_t>> entries(nq);
    std::size_t r_in = 1;
    for (int q = 0; q < nq; ++q) {
        std::set<std::int32_t> probed;
        for (int j = 0; j < ma; ++j) {
            const std::int32_t p = assign[(std::size_t)q * ma + j];
            if (p >= 0 && p < nparts) probed.insert(p);
        }
        for (auto it = probed.rbegin(); it != probed.rend(); ++it)
            for (std::uint64_t i = parts[*it].rows; i-- > 0;) {
                const std::uint32_t key = parts[*it].labels ? parts[*it].labels[i] : (std::uint32_t)(parts[*it].key_base + i);
                if (ifilter && !ifilter->passes(key)) continue;
                if (fmode >= 0 && !f.passes(key)) continue;
                entries[q].push_back(key);
            }
        r_in = std::max(r_in, entries[q].size());
    }
    const std::int32_t has = r_in <= (std::size_t)refine::kMaxIn ? 1 : 0;
    std::fwrite(&has, 4, 1, out);
    if (!has) return;
    std::vector<std::int32_t> counts(nq);
    std::vector<std::uint32_t> keys((std::size_t)nq * r_in, 0u);
    for (int q = 0; q < nq; ++q) {
        counts[q] = (std::int32_t)entries[q].size();
        std::copy(entries[q].begin(), entries[q].end(), keys.begin() + (std::size_t)q * r_in);
    }
    const std::uint64_t rr_missing =
        refine::rerank(st, nq, queries.data(), (int)r_in, keys.data(), counts.data(), nullptr, R, ok.data(), od.data(), os.data());
    write_result(out, ok, od, os, rr_missing);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::cerr << "usage: refine_probe_host IN OUT" << std::endl;
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<std::int32_t> head;
    read_vec(in, head, 1);
    for (int c = 0, ncases = head[0]; c < ncases; ++c) {
        read_vec(in, head, 6);
        const bool keyed = head[0] != 0;
        const int dim = head[1], dtype = head[2], nops = head[3], nparts = head[4], ncalls = head[5];
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
            } else if (kind == 1 && keyed) {
                read_vec(in, n, 1);
                read_vec(in, labels, (std::size_t)n[0]);
                read_vec(in, vec, (std::size_t)n[0] * dim);
                if (!map->put(vec.data(), labels.data(), n[0])) return 3;
            } else if (kind == 2 && keyed) {
                read_vec(in, n, 1);
                read_vec(in, labels, (std::size_t)n[0]);
                map->remove(labels.data(), n[0]);
            } else {
                std::cerr << "unknown operation " << kind << std::endl;
                return 2;
            }
        }
        std::vector<std::vector<std::uint32_t>> labels((std::size_t)nparts);
        std::vector<refine::probe_part> parts((std::size_t)nparts);
        for (int p = 0; p < nparts; ++p) {
            std::vector<std::uint32_t> base;
            std::vector<std::uint64_t> rows;
            read_vec(in, head, 1);
            read_vec(in, base, 1);
            read_vec(in, rows, 1);
            if (head[0]) read_vec(in, labels[p], (std::size_t)rows[0]);
            parts[p] = refine::probe_part{head[0] ? labels[p].data() : nullptr, base[0], rows[0]};
        }
        std::vector<std::uint64_t> nif;
        refine::filter ifilter;
        read_vec(in, head, 1);
        read_vec(in, nif, 1);
        const int ifmode = head[0];
        read_filter(in, ifmode, (std::size_t)nif[0], ifilter);
        for (int call = 0; call < ncalls; ++call) {
            if (keyed)
                call_op(*map, parts, ifmode < 0 ? nullptr : &ifilter, in, out);
            else
                call_op(*dense, parts, ifmode < 0 ? nullptr : &ifilter, in, out);
        }
    }
    std::fclose(in);
    std::fclose(out);
    std::cout << "ok" << std::endl;
    return 0;
}
