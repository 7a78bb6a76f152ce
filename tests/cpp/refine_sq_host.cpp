// TEST DRIVER (CPU only): the host twin of the refine store with SQ8 rows and read-back (host/refine.hpp; include/qadc.h;
// DESIGN.md section 11.20) on scripts of operations read from a file.  tests/test_refine_sq_host.py compares the outputs, bit for
// bit, with a numpy restatement; the GPU tests compare the library with these outputs.  C++14, header only.
//   usage: refine_sq_host IN OUT [flush]
// flush: the driver's thread flushes subnormals to zero (x86: the FTZ and DAZ bits of MXCSR), as it does in a process that loaded a
// library built with -ffast-math.  The parameters' check, inv, the encode, the clamp count and the range must not change (they run in
// the default environment: refine::ieee_scope); decoded rows and distances are the caller's arithmetic and may.
//   IN : int32 ncases, then per case int32 dim, dtype (0 f32, 1 f16, 2 sq8), keyed, nops | (sq8) float vmin [dim], step [dim]
//        then per operation int32 op and
//        1 add    uint32 first_key, count | float vectors [count][dim]
//        2 put    uint32 count | uint32 labels [count] | float vectors [count][dim]
//        3 remove uint32 count | uint32 labels [count]
//        4 get    uint32 count | uint32 keys [count]
//        5 rerank int32 nq, r_in, R, has_counts, has_values | float queries [nq][dim] | uint32 keys [nq][r_in] | counts | values
//        6 knn    int32 nq, R, mode (-1: no filter), nf | uint32 filter keys [nf] (sorted) | float queries [nq][dim]
//        7 info
//        8 bytes  uint32 count | uint32 keys [count]   (sq8, every key held)
//        9 range  uint32 n | float vectors [n][dim]
//   OUT: per case int32 refused (1: the constructor refused the parameters; no operation runs), then per operation
//        1, 2 int32 ok | 3 uint64 removed | 4 float rows [count][dim], uint8 found [count] | 5 uint64 missing, uint32 keys [nq][R],
//        float dist [nq][R], int32 sizes [nq] | 6 keys, dist, sizes | 7 uint64 clamped, uint64 keys held | 8 uint8 [count][dim] |
//        9 float vmin [dim], step [dim]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <cstring>
#include <vector>
#if defined(__SSE__)
#include <xmmintrin.h>
#endif

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
static void put(std::FILE* f, const std::vector<T>& v) {
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}

template <typename T>
static void put1(std::FILE* f, T v) {
    std::fwrite(&v, sizeof(T), 1, f);
}

// the operations that read a store, on either kind
template <typename Store>
static void read_op(const Store& st, int op, std::FILE* in, std::FILE* out) {
    const int dim = st.dim;
    std::vector<std::int32_t> hd;
    std::vector<std::uint32_t> cnt, keys;
    std::vector<float> queries, values;
    if (op == 4 || op == 8) {
        read_vec(in, cnt, 1);
        read_vec(in, keys, cnt[0]);
        if (op == 4) {
            std::vector<float> rows((std::size_t)cnt[0] * dim);
            std::vector<std::uint8_t> found(cnt[0]);
            refine::get(st, keys.data(), cnt[0], rows.data(), found.data());
            put(out, rows);
            put(out, found);
        }
    } else if (op == 5) {
        read_vec(in, hd, 5);
        const int nq = hd[0], r_in = hd[1], R = hd[2];
        std::vector<std::int32_t> counts;
        read_vec(in, queries, (std::size_t)nq * dim);
        read_vec(in, keys, (std::size_t)nq * r_in);
        if (hd[3]) read_vec(in, counts, nq);
        if (hd[4]) read_vec(in, values, (std::size_t)nq * r_in);
        std::vector<std::uint32_t> ok((std::size_t)nq * R);
        std::vector<float> od((std::size_t)nq * R);
        std::vector<std::int32_t> os(nq);
        const std::uint64_t missing = refine::rerank(st, nq, queries.data(), r_in, keys.data(), hd[3] ? counts.data() : nullptr,
                                                    hd[4] ? values.data() : nullptr, R, ok.data(), od.data(), os.data());
        put1(out, missing);
        put(out, ok);
        put(out, od);
        put(out, os);
    } else if (op == 6) {
        read_vec(in, hd, 4);
        const int nq = hd[0], R = hd[1];
        refine::filter f;
        f.mode = hd[2];
        read_vec(in, f.keys, hd[3]);
        read_vec(in, queries, (std::size_t)nq * dim);
        std::vector<std::uint32_t> ok((std::size_t)nq * R);
        std::vector<float> od((std::size_t)nq * R);
        std::vector<std::int32_t> os(nq);
        refine::knn(st, nq, queries.data(), R, hd[2] < 0 ? nullptr : &f, ok.data(), od.data(), os.data());
        put(out, ok);
        put(out, od);
        put(out, os);
    }
}

int main(int argc, char** argv) {
    if (argc != 3 && !(argc == 4 && std::strcmp(argv[3], "flush") == 0)) {
        std::cerr << "usage: refine_sq_host IN OUT [flush]" << std::endl;
        return 2;
    }
    if (argc == 4) {
#if defined(__SSE__)
        _mm_setcsr(_mm_getcsr() | 0x8040u);   // FTZ | DAZ
        volatile float tiny = 1e-40f, two = 2.0f;
        if (tiny * two != 0.0f) {
            std::cerr << "the thread does not flush subnormals" << std::endl;
            return 2;
        }
#else
        std::cerr << "flush needs SSE" << std::endl;
        return 3;
#endif
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    std::vector<std::int32_t> head;
    read_vec(in, head, 1);
    for (int c = 0, ncases = head[0]; c < ncases; ++c) {
        read_vec(in, head, 4);
        const int dim = head[0], dtype = head[1], keyed = head[2], nops = head[3];
        std::vector<float> vmin, step;
        std::unique_ptr<refine::store> dense;
        std::unique_ptr<refine::keyed_store> map;
        std::int32_t refused = 0;
        if (dtype == refine::kSQ8) {
            read_vec(in, vmin, dim);
            read_vec(in, step, dim);
        }
        try {
            if (dtype == refine::kSQ8) {
                if (keyed) map.reset(new refine::keyed_store(dim, vmin.data(), step.data()));
                else dense.reset(new refine::store(dim, vmin.data(), step.data()));
            } else {
                if (keyed) map.reset(new refine::keyed_store(dim, dtype));
                else dense.reset(new refine::store(dim, dtype));
            }
        } catch (const std::invalid_argument&) {
            refused = 1;
        }
        put1(out, refused);
        if (refused && nops) {
            std::cerr << "a refused store takes no operations" << std::endl;
            return 2;
        }
        for (int o = 0; o < nops; ++o) {
            read_vec(in, head, 1);
            const int op = head[0];
            std::vector<std::uint32_t> hd, labels;
            std::vector<float> vec;
            if (op == 1) {
                read_vec(in, hd, 2);
                read_vec(in, vec, (std::size_t)hd[1] * dim);
                put1<std::int32_t>(out, dense && dense->add(vec.data(), hd[1], hd[0]) ? 1 : 0);
            } else if (op == 2) {
                read_vec(in, hd, 1);
                read_vec(in, labels, hd[0]);
                read_vec(in, vec, (std::size_t)hd[0] * dim);
                put1<std::int32_t>(out, map && map->put(vec.data(), labels.data(), hd[0]) ? 1 : 0);
            } else if (op == 3) {
                read_vec(in, hd, 1);
                read_vec(in, labels, hd[0]);
                put1<std::uint64_t>(out, map ? map->remove(labels.data(), hd[0]) : 0);
            } else if (op == 7) {
                put1<std::uint64_t>(out, keyed ? map->sq.clamped : dense->sq.clamped);
                put1<std::uint64_t>(out, keyed ? map->live() : dense->rows);
            } else if (op == 9) {
                read_vec(in, hd, 1);
                read_vec(in, vec, (std::size_t)hd[0] * dim);
                std::vector<float> a(dim), b(dim);
                refine::sq_range(vec.data(), hd[0], dim, a.data(), b.data());
                put(out, a);
                put(out, b);
            } else {
                std::fflush(out);
                const long at = std::ftell(in);
                if (keyed) read_op(*map, op, in, out);
                else read_op(*dense, op, in, out);
                if (op == 8) {   // the stored bytes themselves (read_op consumed the keys; read them again)
                    std::fseek(in, at, SEEK_SET);
                    read_vec(in, hd, 1);
                    read_vec(in, labels, hd[0]);
                    for (std::uint32_t k : labels) {
                        const std::uint8_t* row = keyed ? map->sq8.find(k)->second.data() : dense->sq8.data() + (std::size_t)(k - dense->lo) * dim;
                        std::fwrite(row, 1, dim, out);
                    }
                }
            }
        }
    }
    std::fclose(in);
    std::fclose(out);
    std::cout << "ok" << std::endl;
    return 0;
}
