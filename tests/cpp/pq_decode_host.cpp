// CPU driver of tests/test_pq_decode_host.py and of the GPU tests' expectations: the host twin of the PQ decoder and of the key
// lookup (host/pq_decode.hpp).  Header-only: nothing of the C-ABI library is linked.  All files are raw little-endian arrays.
//   pq_decode_host decode IN OUT   IN: int64 {n, dim, sq_count, sq_bits, K, has_rotation, has_assign, has_vectors}, codebooks
//                                  [sq_count][2^sq_bits][dsub] float32, then as flagged rotation [dim][dim], coarse [K][dim], assign [n]
//                                  int32; codes in the encoder's layout; vectors [n][dim] as flagged;
//                                  OUT: out [n][dim] float32, then err [n] float32 when vectors were given
//   pq_decode_host where IN OUT    IN: int64 {parts, labelled, count}, sizes [parts] uint32, key_base [parts] uint32, the labels of all
//                                  partitions back to back when labelled, keys [count] uint32;  OUT: where [count] uint64
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../quick-adc_amd/host/pq_decode.hpp"

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

int main(int argc, char** argv) {
    try {
        const std::string mode = argc == 4 ? argv[1] : "";
        if (mode != "decode" && mode != "where") {
            std::fprintf(stderr, "usage: %s decode|where IN OUT\n", argv[0]);
            return 2;
        }
        std::ifstream f(argv[2], std::ios_base::in | std::ios_base::binary);
        if (!f) throw std::runtime_error("cannot open the input");
        std::ofstream o(argv[3], std::ios_base::out | std::ios_base::binary);
        if (mode == "decode") {
            const std::vector<std::int64_t> h = take<std::int64_t>(f, 8);
            const size_t n = (size_t)h[0];
            const int dim = (int)h[1], sq_count = (int)h[2], sq_bits = (int)h[3], K = (int)h[4];
            if (!qadc::pq_decode_shape_ok(sq_count, sq_bits) || dim <= 0 || dim % sq_count || K < 0) throw std::runtime_error("bad header");
            const std::vector<float> cb = take<float>(f, ((size_t)1 << sq_bits) * dim);
            const std::vector<float> rot = take<float>(f, h[5] ? (size_t)dim * dim : 0);
            const std::vector<float> coarse = take<float>(f, (size_t)K * dim);
            const std::vector<std::int32_t> assign = take<std::int32_t>(f, h[6] ? n : 0);
            const std::vector<std::uint8_t> codes = take<std::uint8_t>(f, n * qadc::pq_decode_code_bytes(sq_count, sq_bits));
            const std::vector<float> vecs = take<float>(f, h[7] ? n * dim : 0);
            if (K > 0 && !h[6]) throw std::runtime_error("K > 0 needs assign");
            std::vector<float> out(n * dim), err(h[7] ? n : 0);
            qadc::pq_decode(sq_count, sq_bits, dim, cb.data(), h[5] ? rot.data() : nullptr, K, K ? coarse.data() : nullptr,
                            h[6] ? assign.data() : nullptr, codes.data(), n, h[7] ? vecs.data() : nullptr, out.data(), h[7] ? err.data() : nullptr);
            put(o, out);
            put(o, err);
        } else {
            const std::vector<std::int64_t> h = take<std::int64_t>(f, 3);
            const size_t parts = (size_t)h[0], count = (size_t)h[2];
            const std::vector<std::uint32_t> sizes = take<std::uint32_t>(f, parts), base = take<std::uint32_t>(f, parts);
            size_t rows = 0;
            for (std::uint32_t s : sizes) rows += s;
            const std::vector<std::uint32_t> labels = take<std::uint32_t>(f, h[1] ? rows : 0);
            const std::vector<std::uint32_t> keys = take<std::uint32_t>(f, count);
            std::vector<const std::uint32_t*> lab(parts, nullptr);
            size_t at = 0;
            for (size_t p = 0; p < parts; ++p) {
                if (h[1]) lab[p] = labels.data() + at;
                at += sizes[p];
            }
            std::vector<std::uint64_t> where(count);
            qadc::reconstruct_where(parts, sizes.data(), h[1] ? lab.data() : nullptr, base.data(), keys.data(), count, where.data());
            put(o, where);
        }
        if (!o) throw std::runtime_error("cannot write the output");
        std::cout << "ok" << std::endl;
        return 0;
    } catch (const std::exception& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
