// CPU driver of tests/test_pq_train_host.py: the host twin of qadc_pq_train_host (host/db_build.hpp: pq_train_iterations) and the
// geometry of the update kernel (host/pq_train_plan.hpp).  Header-only: nothing of the C-ABI library is linked.
//   pq_train_host run IN OUT    IN: int32 {n, dim, sq_count, sq_bits, K_coarse, has_rotation, iters, div_mode}, vectors [n][dim], seed
//                               codebooks, coarse [K_coarse][dim], rotation [dim][dim] (float32);  OUT: codebooks, codes, uint64 empty
//   pq_train_host plan SQ_COUNT SQ_BITS DIM    prints the plan, or "refused"
//   pq_train_host plans SQ_COUNT SQ_BITS DSUB_MAX    one such line for every dim = SQ_COUNT * dsub, dsub = 1 .. DSUB_MAX
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../quick-adc_amd/host/db_build.hpp"
#include "../../quick-adc_amd/host/pq_train_plan.hpp"

template <typename T>
static std::vector<T> take(std::ifstream& f, size_t count) {
    std::vector<T> v(count);
    f.read(reinterpret_cast<char*>(v.data()), sizeof(T) * count);
    if (!f) throw std::runtime_error("short input");
    return v;
}

int main(int argc, char** argv) {
    try {
        if (argc == 5 && (std::string(argv[1]) == "plan" || std::string(argv[1]) == "plans")) {
            const bool many = std::string(argv[1]) == "plans";
            const int sq_count = std::atoi(argv[2]), last = many ? std::atoi(argv[4]) : 1;
            for (int ds = 1; ds <= last; ++ds) {
                qadc::PqTrainPlan p;
                if (!qadc::pq_train_plan(sq_count, std::atoi(argv[3]), many ? sq_count * ds : std::atoi(argv[4]), &p)) {
                    std::cout << "refused" << std::endl;
                    continue;
                }
                std::cout << "wg=" << qadc::kPqTrainWG << " stage=" << qadc::kPqTrainStage << " code_stage=" << qadc::kPqTrainCodeStage
                          << " K=" << p.K << " dsub=" << p.dsub << " width=" << p.width << " dblocks=" << p.dblocks << " kper=" << p.kper
                          << " kblocks=" << p.kblocks << " mper=" << p.mper << " mblocks=" << p.mblocks << " cols=" << p.cols
                          << " chunk=" << p.chunk << " grid=" << p.grid << " lds=" << p.lds_bytes << std::endl;
            }
            return 0;
        }
        if (argc != 4 || std::string(argv[1]) != "run") {
            std::fprintf(stderr, "usage: %s run IN OUT | plan SQ_COUNT SQ_BITS DIM | plans SQ_COUNT SQ_BITS DSUB_MAX\n", argv[0]);
            return 2;
        }
        std::ifstream f(argv[2], std::ios_base::in | std::ios_base::binary);
        if (!f) throw std::runtime_error("cannot open the input");
        const std::vector<std::int32_t> h = take<std::int32_t>(f, 8);
        const size_t n = (size_t)h[0];
        const int dim = h[1], sq_count = h[2], sq_bits = h[3], K_coarse = h[4], has_rot = h[5], iters = h[6], div_mode = h[7];
        const std::vector<float> vecs = take<float>(f, n * dim);
        std::vector<float> cb = take<float>(f, ((size_t)dim << sq_bits));
        const std::vector<float> coarse = take<float>(f, (size_t)K_coarse * dim);
        const std::vector<float> rot = take<float>(f, has_rot ? (size_t)dim * dim : 0);
        std::vector<std::uint8_t> codes(n * (size_t)(sq_bits == 4 ? sq_count / 2 : sq_count));
        const std::uint64_t empty = qadc::pq_train_iterations(vecs.data(), n, dim, sq_count, sq_bits, K_coarse, K_coarse ? coarse.data() : nullptr,
                                                              has_rot ? rot.data() : nullptr, cb.data(), iters, codes.data(), div_mode);
        std::ofstream o(argv[3], std::ios_base::out | std::ios_base::binary);
        o.write(reinterpret_cast<const char*>(cb.data()), sizeof(float) * cb.size());
        o.write(reinterpret_cast<const char*>(codes.data()), codes.size());
        o.write(reinterpret_cast<const char*>(&empty), sizeof(empty));
        if (!o) throw std::runtime_error("cannot write the output");
        std::cout << "ok" << std::endl;
        return 0;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
