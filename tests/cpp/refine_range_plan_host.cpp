// CPU driver of the exact range search's launch geometry (host/refine_range_plan.hpp; tests/test_refine_range_plan_host.py): runs
// the header as the library compiles it and writes what it plans out for the test to check.  No HIP, no library.
//   refine_range_plan_host plans IN OUT
//       in : int64 rows of 6: nq, rows, dim, region_rows, chunk_rows, pass_nq
//       out: int64 rows of 14: accepted | qt, jregs, dist_lds_bytes, pass_nq, passes, region_rows, chunk_rows, groups, slice_rows,
//            slices, launches | the fewest and the most visits of a row in a walk of the launches, groups, slices and waves
//   refine_range_plan_host chunks IN OUT
//       in : int64 nq, pass_nq, max_entries, in_lims [nq + 1]
//       out: int64 accepted, passes, then per pass q0, q1, cands_per_wg, chunks and per chunk q, first, count
//   refine_range_plan_host regions IN OUT
//       in : int64 n, max_entries, cap [n], count [n]
//       out: int64 accepted, entries, base [n] | rerun, cap [n] after range_rerun | accepted, entries of the second run
//   refine_range_plan_host sizes IN OUT
//       in : int64 rows of 5: entries, longest, held, kept, max_entries
//       out: int64 rows of 2: range_scratch_entries(entries, longest), range_held_fits(held, kept, max_entries)
//   refine_range_plan_host limits IN OUT
//       in : float radius [...]      out: uint64 range_limit_word of each
//   refine_range_plan_host refusals IN OUT
//       in : int64 rows of 10: call (0 range, 1 rerank_range, 2 set_range_plan), store, nq, queries, radius, lims, in_lims (0 null,
//            1 monotone from 0, 2 starts above 0, 3 decreases, 4 all zero), keys, chunk_rows, pass_nq      out: int64 refused each
// stdout: "ok".
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../quick-adc_amd/host/refine_range_plan.hpp"

using namespace qadc::refine;

template <typename T>
static std::vector<T> read_all(const char* path) {
    std::vector<T> v;
    FILE* in = fopen(path, "rb");
    if (!in) return v;
    T x;
    while (fread(&x, sizeof(T), 1, in) == 1) v.push_back(x);
    fclose(in);
    return v;
}

template <typename T>
static bool write_all(const char* path, const std::vector<T>& v) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

static int plans(const std::vector<int64_t>& in, std::vector<int64_t>& out) {
    for (size_t i = 0; i + 6 <= in.size(); i += 6) {
        const int64_t* a = in.data() + i;
        RangePlan p{};
        int64_t o[14] = {0};
        o[0] = range_plan((int)a[0], (uint64_t)a[1], (int)a[2], (uint64_t)a[3], (uint64_t)a[4], (int)a[5], &p);
        if (o[0]) {
            const int64_t v[11] = {p.qt, p.jregs, (int64_t)p.dist_lds_bytes, p.pass_nq, p.passes, (int64_t)p.region_rows, (int64_t)p.chunk_rows,
                                   p.groups, p.slice_rows, p.slices, (int64_t)p.launches};
            std::copy(v, v + 11, o + 1);
            const uint64_t nrows = (uint64_t)a[1];
            std::vector<uint8_t> seen((size_t)nrows, 0);
            for (uint64_t l = 0; l < p.launches; ++l) {
                const int live = knn_launch_groups(nrows, p.chunk_rows, p.groups, l);
                for (int g = 0; g < live; ++g)
                    for (int s = 0; s < p.slices; ++s) {
                        uint64_t first, last;
                        knn_slice(nrows, p.chunk_rows, p.groups, p.slice_rows, l, g, s, &first, &last);
                        for (int w = 0; w < kKnnWaves; ++w)
                            for (uint64_t r = first + w; r < last; r += kKnnWaves) {
                                if (r >= nrows) return 5;   // (the kernel would read past the store)
                                if (seen[(size_t)r] < 255) ++seen[(size_t)r];
                            }
                    }
            }
            o[12] = nrows ? *std::min_element(seen.begin(), seen.end()) : 1;
            o[13] = nrows ? *std::max_element(seen.begin(), seen.end()) : 1;
        }
        out.insert(out.end(), o, o + 14);
    }
    return 0;
}

static int chunks(const std::vector<int64_t>& in, std::vector<int64_t>& out) {
    const int nq = (int)in[0], pass_nq = (int)in[1];
    const uint64_t max_entries = (uint64_t)in[2];
    std::vector<uint64_t> lims(in.begin() + 3, in.end());
    if ((int)lims.size() != nq + 1) return 6;
    std::vector<RangeCandPass> passes;
    const bool ok = range_cand_passes(lims.data(), nq, pass_nq, max_entries, &passes);
    out.push_back(ok);
    out.push_back(ok ? (int64_t)passes.size() : 0);
    if (!ok) return 0;
    std::vector<RangeChunk> table;
    for (const RangeCandPass& p : passes) {
        const int cpw = range_cands_per_wg(lims.data(), p.q0, p.q1);
        range_cand_chunks(lims.data(), p.q0, p.q1, cpw, &table);
        const int64_t head[4] = {p.q0, p.q1, cpw, (int64_t)table.size()};
        out.insert(out.end(), head, head + 4);
        for (const RangeChunk& c : table) {
            out.push_back(c.q);
            out.push_back(c.first);
            out.push_back(c.count);
        }
    }
    return 0;
}

static int regions(const std::vector<int64_t>& in, std::vector<int64_t>& out) {
    const int n = (int)in[0];
    const uint64_t max_entries = (uint64_t)in[1];
    if ((int64_t)in.size() != 2 + 2 * (int64_t)n) return 6;
    std::vector<uint64_t> cap(in.begin() + 2, in.begin() + 2 + n), count(in.begin() + 2 + n, in.end()), base((size_t)n, 0);
    uint64_t entries = 0;
    bool ok = range_regions(cap.data(), n, max_entries, base.data(), &entries);
    out.push_back(ok);
    out.push_back(ok ? (int64_t)entries : 0);
    out.insert(out.end(), base.begin(), base.end());
    out.push_back(range_rerun(cap.data(), count.data(), n));
    out.insert(out.end(), cap.begin(), cap.end());
    entries = 0;
    ok = range_regions(cap.data(), n, max_entries, base.data(), &entries);
    out.push_back(ok);
    out.push_back(ok ? (int64_t)entries : 0);
    return 0;
}

static int sizes(const std::vector<int64_t>& in, std::vector<int64_t>& out) {
    for (size_t i = 0; i + 5 <= in.size(); i += 5) {
        const int64_t* a = in.data() + i;
        out.push_back((int64_t)range_scratch_entries((uint64_t)a[0], (uint64_t)a[1]));
        out.push_back(range_held_fits((uint64_t)a[2], (uint64_t)a[3], (uint64_t)a[4]));
    }
    return 0;
}

static int refusals(const std::vector<int64_t>& in, std::vector<int64_t>& out) {
    for (size_t i = 0; i + 10 <= in.size(); i += 10) {
        const int64_t* a = in.data() + i;
        const int nq = (int)a[2];
        std::vector<uint64_t> lims((size_t)std::max(nq, 0) + 1, 0);
        for (int q = 0; q < nq; ++q) lims[q + 1] = a[6] == 4 ? 0 : lims[q] + 3;
        if (a[6] == 2) lims[0] = 1;
        if (a[6] == 3 && nq >= 2) lims[nq] = lims[nq - 1] - 1;   // (the test asks for this with two queries at least)
        const uint64_t* il = a[6] == 0 ? nullptr : lims.data();
        const char* why = a[0] == 0   ? range_refusal(a[1] != 0, nq, a[3] != 0, a[4] != 0, a[5] != 0)
                          : a[0] == 1 ? rerank_range_refusal(a[1] != 0, nq, a[3] != 0, il, a[7] != 0, a[4] != 0, a[5] != 0)
                                      : range_plan_refusal(a[1] != 0, (uint64_t)a[8], (int)a[9]);
        out.push_back(why != nullptr);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    int rc = 0;
    if (!strcmp(argv[1], "limits")) {
        std::vector<uint64_t> out;
        for (float r : read_all<float>(argv[2])) out.push_back(range_limit_word(r));
        if (!write_all(argv[3], out)) return 4;
    } else {
        const std::vector<int64_t> in = read_all<int64_t>(argv[2]);
        std::vector<int64_t> out;
        if (!strcmp(argv[1], "plans")) rc = plans(in, out);
        else if (!strcmp(argv[1], "chunks")) rc = chunks(in, out);
        else if (!strcmp(argv[1], "regions")) rc = regions(in, out);
        else if (!strcmp(argv[1], "sizes")) rc = sizes(in, out);
        else if (!strcmp(argv[1], "refusals")) rc = refusals(in, out);
        else return 2;
        if (rc) return rc;
        if (!write_all(argv[3], out)) return 4;
    }
    printf("ok\n");
    return 0;
}
