// CPU driver of tests/test_pq_train16_host.py: the host twins of qadc_pq_train16_host / qadc_pq_update16_host (host/db_build.hpp:
// pq_train16_iterations, pq_update16) and the geometry of the sorted update (host/pq_train16_plan.hpp).  Header-only: nothing of the
// C-ABI library is linked.
//   pq_train16_host run IN OUT       IN: int32 {n, dim, sq_count, K_coarse, has_rotation, iters, div_mode}, vectors [n][dim], seed
//                                    codebooks, coarse [K_coarse][dim], rotation [dim][dim] (float32);  OUT: codebooks, codes uint16
//                                    [n][sq_count] (absent when iters == 0), uint64 empty
//   pq_train16_host update IN OUT    IN: int32 {n, dim, sq_count, div_mode}, vectors, codes uint16;  OUT: codebooks, counts uint32
//   pq_train16_host plans SQ_COUNT DSUB_MAX   one line per dim = SQ_COUNT * dsub, dsub = 1 .. DSUB_MAX: the plan and, for clusters 0,
//                                    1, 32767 and 65535, owned = how often the walk's lanes own each of the cluster's components
//                                    (min and max over the components) and stray = lanes owning a component outside [0, dsub)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../quick-adc_amd/host/db_build.hpp"
#include "../../quick-adc_amd/host/pq_train16_plan.hpp"

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

static void plans(int sq_count, int last) {
    for (int ds = 1; ds <= last; ++ds) {
        qadc::PqTrain16Plan p;
        if (!qadc::pq_train16_plan(sq_count, sq_count * ds, &p)) {
            std::cout << "refused" << std::endl;
            continue;
        }
        int lo = 1 << 30, hi = 0, stray = 0;
        const std::uint32_t ks[4] = {0u, 1u, 32767u, 65535u};
        for (std::uint32_t k : ks) {
            std::vector<int> owned((size_t)ds, 0);
            // the workgroups that hold a unit of cluster k, and one on either side
            const std::uint32_t b0 = (std::uint32_t)((std::uint64_t)k * p.dblocks / p.wg_groups);
            const std::uint32_t b1 = (std::uint32_t)(((std::uint64_t)(k + 1) * p.dblocks - 1) / p.wg_groups);
            for (std::uint32_t b = b0 ? b0 - 1 : 0; b <= b1 + 1 && b < p.walk_grid; ++b)
                for (int tid = 0; tid < qadc::kPqTrain16WG; ++tid) {
                    const qadc::PqTrain16Owner o = qadc::pq_train16_owner(p.dsub, p.width, p.dblocks, p.wave_groups, b, tid);
                    if (!o.owns) continue;
                    if (o.d < 0 || o.d >= ds || o.k >= 65536u) ++stray;
                    else if (o.k == k) ++owned[(size_t)o.d];
                }
            for (int c : owned) {
                lo = c < lo ? c : lo;
                hi = c > hi ? c : hi;
            }
        }
        std::cout << "wg=" << qadc::kPqTrain16WG << " dsub=" << p.dsub << " width=" << p.width << " dblocks=" << p.dblocks
                  << " wave_groups=" << p.wave_groups << " wg_groups=" << p.wg_groups << " units=" << p.units << " grid=" << p.walk_grid
                  << " lds=" << p.lds_bytes << " owned_min=" << lo << " owned_max=" << hi << " stray=" << stray << std::endl;
    }
}

int main(int argc, char** argv) {
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if (argc == 4 && mode == "plans") {
            plans(std::atoi(argv[2]), std::atoi(argv[3]));
            return 0;
        }
        if (argc != 4 || (mode != "run" && mode != "update")) {
            std::fprintf(stderr, "usage: %s run IN OUT | update IN OUT | plans SQ_COUNT DSUB_MAX\n", argv[0]);
            return 2;
        }
        std::ifstream f(argv[2], std::ios_base::in | std::ios_base::binary);
        if (!f) throw std::runtime_error("cannot open the input");
        std::ofstream o(argv[3], std::ios_base::out | std::ios_base::binary);
        if (mode == "update") {
            const std::vector<std::int32_t> h = take<std::int32_t>(f, 4);
            const size_t n = (size_t)h[0];
            const int dim = h[1], sq_count = h[2], div_mode = h[3];
            const std::vector<float> vecs = take<float>(f, n * dim);
            const std::vector<std::uint16_t> codes = take<std::uint16_t>(f, n * sq_count);
            std::vector<float> cb((size_t)dim * 65536);
            std::vector<std::uint32_t> counts((size_t)sq_count * 65536);
            qadc::pq_update16(vecs.data(), n, dim, sq_count, codes.data(), cb.data(), counts.data(), div_mode);
            put(o, cb);
            put(o, counts);
        } else {
            const std::vector<std::int32_t> h = take<std::int32_t>(f, 7);
            const size_t n = (size_t)h[0];
            const int dim = h[1], sq_count = h[2], K_coarse = h[3], has_rot = h[4], iters = h[5], div_mode = h[6];
            const std::vector<float> vecs = take<float>(f, n * dim);
            std::vector<float> cb = take<float>(f, (size_t)dim * 65536);
            const std::vector<float> coarse = take<float>(f, (size_t)K_coarse * dim);
            const std::vector<float> rot = take<float>(f, has_rot ? (size_t)dim * dim : 0);
            std::vector<std::uint16_t> codes(iters > 0 ? n * (size_t)sq_count : 0);
            const std::uint64_t empty = qadc::pq_train16_iterations(vecs.data(), n, dim, sq_count, K_coarse, K_coarse ? coarse.data() : nullptr,
                                                                    has_rot ? rot.data() : nullptr, cb.data(), iters,
                                                                    iters > 0 ? codes.data() : nullptr, div_mode);
            put(o, cb);
            put(o, codes);
            o.write(reinterpret_cast<const char*>(&empty), sizeof(empty));
        }
        if (!o) throw std::runtime_error("cannot write the output");
        std::cout << "ok" << std::endl;
        return 0;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
