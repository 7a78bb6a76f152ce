// TEST INFRASTRUCTURE — not product code.  Compiled by tools/gen_golden_adc16.py only, where the reference tree exists.
//
// A C entry around the reference's OWN scanner_simple::query_scan (db_query.cpp:26-45) and get_scan_func (query_common.hpp:120-143)
// for the 16-bit code shapes (2,16) (4,16) (8,16), i.e. scan_standard<uint16_t, NSQ> as g++ compiles it with the reference's
// flags (oracle/Makefile REF_FLAGS).  The x_*.inc names are the line ranges oracle/ref_extract.sh cuts out of the reference's
// files into a temporary directory that is on the include path of this compile only (oracle/ref_float_harness.cpp includes them
// the same way); no reference text and nothing compiled from it is kept.  What this file adds is an in-memory base_db and
// the entry point.
#include <immintrin.h>
#include <x86intrin.h>
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <memory>
#include <string>
#include <vector>
#define _mm256_set_m128i qadc_ref_mm256_set_m128i      // simd_scan.hpp:120 vs GCC >= 8's own intrinsic (see oracle/ref_harness.cpp)
#include "config.h"
#include "binheap.hpp"
#include "neighbors.hpp"
#include "simd_layout.hpp"
#include "simd_scan.hpp"
#include "vector_io.hpp"
#undef _mm256_set_m128i
#include "x_quantizers_a.inc"
#include "x_quantizers_b.inc"
#include "x_base_db.inc"
#include "x_query_metrics.inc"
#include "x_scan_funcs.inc"
#include "x_scanner_simple.inc"

namespace {

// In-memory base_db over 16-bit codes: partitions are owned copies, handed out row-major as flat_db / index_db do.
struct mem_db16 : base_db {
    std::vector<std::vector<std::uint8_t>> codes;
    std::vector<std::vector<unsigned>> labels;
    std::vector<unsigned> sizes;

    mem_db16(int nsq, int nparts, const std::uint8_t* const* parts, const std::uint32_t* const* labs, const std::uint32_t* szs)
        : base_db(std::unique_ptr<base_pq>(new base_pq(nsq, 16, nsq))) {
        const int cs = pq->code_size();
        codes.resize(nparts);
        labels.resize(nparts);
        sizes.assign(szs, szs + nparts);
        for (int p = 0; p < nparts; ++p) {
            codes[p].assign(parts[p], parts[p] + static_cast<long>(szs[p]) * cs);
            if (labs && labs[p]) labels[p].assign(labs[p], labs[p] + szs[p]);
        }
    }
    void assign_compute_residuals(const float*, int, int*, float*) override {}
    void assign_compute_residuals_mutiple(const float*, const int, const int, int*, float*) override {}
    int partition_count() const override { return static_cast<int>(sizes.size()); }
    void get_partition(int part_i, const std::uint8_t*& c, unsigned*& l, unsigned& size) const override {
        c = codes[part_i].data();
        l = labels[part_i].empty() ? nullptr : const_cast<unsigned*>(labels[part_i].data());
        size = sizes[part_i];
    }
    void free_partition(int) override {}
    void add_vectors(float*, unsigned, unsigned, int) override {}
    void print(std::ostream&) const override {}
};

}  // namespace

extern "C" {

// tables [nparts][nsq * 65536]: the probes are the partitions in order.  Heap arrays out (R entries: the sentinels fill it).
int adc16_ref_query_scan(int nsq, int nparts, const std::uint8_t* const* parts, const std::uint32_t* const* labels,
                         const std::uint32_t* sizes, float* tables, int R, std::uint32_t* out_keys, float* out_vals, int* out_size) {
    if (nsq != 2 && nsq != 4 && nsq != 8) return -1;
    mem_db16 db(nsq, nparts, parts, labels, sizes);
    if (db.pq->code_size() != 2 * nsq) return -2;
    scanner_simple sc;
    sc.prepare_database(db);                           // get_scan_func: scan_standard<uint16_t, nsq>
    std::vector<int> assign(nparts);
    for (int p = 0; p < nparts; ++p) assign[p] = p;
    kv_binheap<unsigned, float> bh(R);
    query_metrics m;
    sc.query_scan(nullptr, assign.data(), nparts, tables, nsq * 65536, bh, m);
    *out_size = bh.size();
    std::memcpy(out_keys, bh.keys(), sizeof(unsigned) * bh.size());
    std::memcpy(out_vals, bh.values(), sizeof(float) * bh.size());
    return 0;
}

const char* adc16_ref_compiler() { return "g++ " __VERSION__; }

}  // extern "C"
