// Database build on the GPU — C++14, header only, calls the C-ABI (include/qadc.h).
//
//   add_vectors_hip(flat_database&, ...)   flat_db::add_vectors  (databases.hpp:136-156)
//   add_vectors_hip(ivf_database&, ...)    index_db::add_vectors (databases.hpp:270-298): the device does the compute
//                                          (nearest centroid, residual, OPQ rotation, PQ encode: qadc_ivf_encode_host),
//                                          the host dispatches codes and labels to the partitions in vector order
//                                          exactly like lines 291-297
//   kmeans_fast_iterations(...)            CPU restatement of kmeans_fast_iterations_thread (databases.cpp:50-90), the
//                                          definition the device version is tested against bit for bit
//   learn_coarse_quantizer_hip(...)        learn_coarse_quantizer (databases.cpp:94-118) from a caller-provided seed:
//                                          the reference seeds with two OpenCV k-means++ iterations (third-party, absent
//                                          here), then runs kmeans_iter_max - 2 = 48 fast iterations — those run on the GPU.
//                                          With a std::uint64_t seed instead of a seed array: seeded by seed_kmeanspp_hip
//   kmeans_seed(..., K_coarse, coarse, rotation, ...)  CPU twin of qadc_kmeans_seed_host: host/kmeans_seed.hpp behind pq_train_front
//   seed_kmeanspp_hip(...)                 k-means++ seeding on the GPU (qadc_kmeans_seed_host): [sq_count][k][dim / sq_count]
//   pq_train_iterations(...)               CPU twin of qadc_pq_train_host: kmeans_fast_iterations on a copy of every sub-space's
//                                          columns, behind the same residual / rotation front
//   pq_train16_iterations(...), pq_update16(...)  the same for 16-bit sub-quantizers (qadc_pq_train16_host, qadc_pq_update16_host)
//   pq_train_iterations(..., repair, repaired), pq_train16_iterations(..., repair, repaired), opq_train_iterations(..., repair,
//                                          repaired)  CPU twins of the qadc_*_train_repair_host calls: every round is assign,
//                                          pq_repair_slice (host/pq_repair.hpp), update
//   learn_pq_hip(...)                      the product quantizer learned on the GPU from a caller-provided seed, as an io::pq_data
//                                          ready for pq_to_data_file (the reference's flatdb_create / indexdb_create2 read it);
//                                          with a std::uint64_t seed: seeded by seed_kmeanspp_hip (learn_opq_hip likewise)
//   opq_cross(...), opq_train_iterations(...)  CPU twins of qadc_opq_cross_host and qadc_opq_train_host: the cross matrix between
//                                          the learning set and its reconstruction, and the Procrustes rounds (host/procrustes.hpp)
//                                          around pq_train_iterations
//   learn_opq_hip(...)                     the OPQ rotation and its product quantizer learned on the GPU, as an io::pq_data with
//                                          is_opq set, ready for pq_to_data_file (.opq.data)
//   db_add_hip(db, base_file, chunk_count) db_add's add_vectors (db_add.cpp:52-82): a reader thread (io::vectors_reader,
//                                          vector_io.hpp:231-288) fills a two-chunk queue from the .fvecs/.bvecs file while
//                                          this thread encodes the previous chunk on the GPU; labels = index in chunk + the
//                                          chunk's offset, as there.
//   db_add_hip(qadc_adc_index*, dim, base_file, chunk_count)  the same into a float-ADC index: encode and append on the GPU
//   db_add_hip(qadc_index*, dim, base_file, chunk_count)      ... and into the 4-bit index (qadc_index_add_vectors)
//   pq_decode_hip(...)                     PQ codes back to vectors on the GPU (qadc_pq_decode_host; CPU twin: host/pq_decode.hpp pq_decode)
//   reconstruct_hip(qadc_adc_index*, ...)  the vectors behind keys of a float-ADC index or a view (qadc_adc_index_reconstruct)
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include <thread>

#include "../../include/qadc.h"
#include <cmath>

#include "kmeans_seed.hpp"
#include "pq_decode.hpp"
#include "pq_repair.hpp"
#include "procrustes.hpp"
#include "qadc_io.hpp"
#include "query_driver.hpp"

namespace qadc {

inline void add_vectors_hip(flat_database& db, const float* vecs, unsigned n, int device = 0) {
    const pq4& pq = *db.pq;
    db.codes.resize((size_t)(db.count + n) * pq.code_size());
    if (qadc_ivf_encode_host(pq.sq_count, pq.dim, pq.centroids.data(), pq.rotation.empty() ? nullptr : pq.rotation.data(), 0,
                             nullptr, vecs, n, nullptr, db.codes.data() + (size_t)db.count * pq.code_size(), device) != QADC_OK)
        throw std::runtime_error(std::string("qadc_ivf_encode_host: ") + qadc_last_error());
    db.count += n;
}

inline void add_vectors_hip(ivf_database& db, const float* vecs, unsigned n, unsigned labels_offset, int device = 0) {
    const pq4& pq = *db.pq;
    const size_t cs = (size_t)pq.code_size();
    std::vector<std::int32_t> assign(n);
    std::vector<std::uint8_t> codes((size_t)n * cs);
    if (qadc_ivf_encode_host(pq.sq_count, pq.dim, pq.centroids.data(), pq.rotation.empty() ? nullptr : pq.rotation.data(),
                             db.part_count, db.coarse.data(), vecs, n, assign.data(), codes.data(), device) != QADC_OK)
        throw std::runtime_error(std::string("qadc_ivf_encode_host: ") + qadc_last_error());
    for (unsigned i = 0; i < n; ++i) {                         // databases.hpp:291-297
        const int p = assign[i];
        db.partitions[p].insert(db.partitions[p].end(), codes.begin() + (size_t)i * cs, codes.begin() + (size_t)(i + 1) * cs);
        db.labels[p].push_back(i + labels_offset);
    }
}

inline void add_chunk_hip(flat_database& db, const io::vectors_chunk& c, int device) { add_vectors_hip(db, c.data.data(), c.count, device); }
inline void add_chunk_hip(ivf_database& db, const io::vectors_chunk& c, int device) {
    add_vectors_hip(db, c.data.data(), c.count, c.offset, device);
}
inline void add_chunk_cpu(flat_database& db, const io::vectors_chunk& c) { db.add_vectors(c.data.data(), c.count); }
inline void add_chunk_cpu(ivf_database& db, const io::vectors_chunk& c) { db.add_vectors(c.data.data(), c.count, c.offset); }

// db_add.cpp:52-82: `add` takes every chunk of the file in turn.  Returns the vectors added; throws with the reference's message
// if the reader fails (wrong dimension, unknown extension), or with the first error of `add` — after the file has been drained.
template <typename AddChunk>
unsigned db_add_chunks(const char* base_filename, unsigned chunk_count, int dim, AddChunk add) {
    io::vectors_reader reader(base_filename, chunk_count);
    if (reader.dim() != dim) throw std::runtime_error("base vectors and quantizer disagree on the dimension");
    std::thread read_thread([&reader] { reader.run(); });
    unsigned added = 0;
    std::string error;
    while (!reader.done()) {
        io::vectors_chunk chunk = reader.get_chunk();
        if (chunk.failed) {
            error = chunk.error;
            break;
        }
        if (error.empty()) {
            try {
                add(chunk);
                added += chunk.count;
            } catch (const std::exception& e) {
                error = e.what();                                // keep draining: the reader must not stay blocked on a full queue
            }
        }
    }
    read_thread.join();
    if (!error.empty()) throw std::runtime_error(error);
    return added;
}

// on_gpu = false runs the host loops instead (the definition the GPU build is compared with).
template <typename Db>
unsigned db_add_hip(Db& db, const char* base_filename, unsigned chunk_count = 1000000, int device = 0, bool on_gpu = true) {
    return db_add_chunks(base_filename, chunk_count, db.pq->dim, [&](const io::vectors_chunk& chunk) {
        if (on_gpu) add_chunk_hip(db, chunk, device);
        else add_chunk_cpu(db, chunk);
    });
}

// The same into a float-ADC index (qadc_adc_index_add_vectors): every chunk is encoded and appended in device memory with the
// quantizers the index holds (`dim` = the dimension given to qadc_adc_index_set_pq), labels = index in chunk + the chunk's offset;
// a flat index writes the chunk at that offset.  No code comes back to the host.
inline unsigned db_add_hip(qadc_adc_index* idx, int dim, const char* base_filename, unsigned chunk_count = 1000000, int sum_mode = 1) {
    return db_add_chunks(base_filename, chunk_count, dim, [&](const io::vectors_chunk& chunk) {
        if (qadc_adc_index_add_vectors(idx, chunk.data.data(), chunk.count, chunk.offset, sum_mode) != QADC_OK)
            throw std::runtime_error(std::string("qadc_adc_index_add_vectors: ") + qadc_last_error());
    });
}

// The same into the 4-bit index (qadc_index_add_vectors): every chunk is encoded and appended in device memory with the quantizers
// the index holds (`dim` = the dimension given to qadc_index_set_pq), labels = index in chunk + the chunk's offset; a flat index
// writes the chunk at that offset.  No code comes back to the host; call qadc_index_finalize before querying.
inline unsigned db_add_hip(qadc_index* idx, int dim, const char* base_filename, unsigned chunk_count = 1000000, int sum_mode = 1) {
    return db_add_chunks(base_filename, chunk_count, dim, [&](const io::vectors_chunk& chunk) {
        if (qadc_index_add_vectors(idx, chunk.data.data(), chunk.count, chunk.offset, sum_mode) != QADC_OK)
            throw std::runtime_error(std::string("qadc_index_add_vectors: ") + qadc_last_error());
    });
}

// Both with the caller's labels (qadc_adc_index_add_vectors_labelled, qadc_index_add_vectors_labelled): labels [vectors of the
// file], vector i of the file gets labels[i] — ids from a database, sparse, permuted or repeated.  An index with a coarse quantizer
// only: a flat one keys its vectors by position and refuses.
inline unsigned db_add_hip(qadc_adc_index* idx, int dim, const char* base_filename, const std::uint32_t* labels, unsigned chunk_count = 1000000,
                           int sum_mode = 1) {
    return db_add_chunks(base_filename, chunk_count, dim, [&](const io::vectors_chunk& chunk) {
        if (qadc_adc_index_add_vectors_labelled(idx, chunk.data.data(), labels + chunk.offset, chunk.count, sum_mode) != QADC_OK)
            throw std::runtime_error(std::string("qadc_adc_index_add_vectors_labelled: ") + qadc_last_error());
    });
}
inline unsigned db_add_hip(qadc_index* idx, int dim, const char* base_filename, const std::uint32_t* labels, unsigned chunk_count = 1000000,
                           int sum_mode = 1) {
    return db_add_chunks(base_filename, chunk_count, dim, [&](const io::vectors_chunk& chunk) {
        if (qadc_index_add_vectors_labelled(idx, chunk.data.data(), labels + chunk.offset, chunk.count, sum_mode) != QADC_OK)
            throw std::runtime_error(std::string("qadc_index_add_vectors_labelled: ") + qadc_last_error());
    });
}

// databases.cpp:50-90 on the host: assign every vector to its closest centroid (find_k_neighbors with k = 1: the expansion
// distances, the compiled replace test !(s >= kept) — the first strict minimum after the last NaN), then centroid = (sum of its members in vector order) times the reciprocal of the count — what the reference
// binary does under -ffast-math (div_mode 1, pinned to its loops as compiled: oracle/_ref) — or divided by it as the source
// reads (div_mode 0).  An empty cluster becomes NaN either way.  repair: the empty-cluster repair of include/qadc.h between the
// assignment and the update of every round; *repaired (nullable) grows by the vectors it moved.
inline void kmeans_fast_iterations(const float* vecs, size_t n, int dim, int K, float* centroids, int iters, int* assign,
                                   int div_mode = 1, bool repair = false, std::uint64_t* repaired = nullptr) {
    std::vector<int> cnt((size_t)K);
    std::vector<float> cn((size_t)K);
    for (int it = 0; it < iters; ++it) {
        // find_k_neighbors with k = 1 (databases.cpp:60-66 -> neighbors.cpp:30-76): expansion distances (float_sum.hpp) pushed in
        // centroid order into a capacity-1 kv_binheap whose replace test the reference's -ffast-math build compiles to
        // !(s >= kept) (vcomiss + jae; oracle/qadc_oracle.c): a NaN replaces the kept centroid, and any later value replaces a NaN
        for (int k = 0; k < K; ++k) cn[k] = sqnorm(centroids + (size_t)k * dim, dim);
        for (size_t i = 0; i < n; ++i) {
            const float* x = vecs + i * dim;
            const float xn = sqnorm(x, dim);
            int best = 0;
            float bestd = expansion_dist(x, centroids, dim, xn, cn[0]);
            for (int k = 1; k < K; ++k) {
                const float s = expansion_dist(x, centroids + (size_t)k * dim, dim, xn, cn[k]);
                if (!(s >= bestd)) { bestd = s; best = k; }
            }
            assign[i] = best;
        }
        if (repair) {
            const std::uint32_t moved = pq_repair_slice(vecs, n, (size_t)dim, dim, K, centroids, assign);
            if (repaired) *repaired += moved;
        }
        std::fill(centroids, centroids + (size_t)K * dim, 0.0f);
        std::fill(cnt.begin(), cnt.end(), 0);
        for (size_t i = 0; i < n; ++i) {
            cnt[assign[i]]++;
            float* c = centroids + (size_t)assign[i] * dim;
            for (int d = 0; d < dim; ++d) c[d] += vecs[i * dim + d];
        }
        for (int k = 0; k < K; ++k) {
            const volatile float r = 1.0f / (float)cnt[k];          // (volatile: the host compiler must not fold the two forms)
            for (int d = 0; d < dim; ++d) {
                float& c = centroids[(size_t)k * dim + d];
                c = div_mode ? c * r : c / (float)cnt[k];
            }
        }
    }
}

// What the quantizer of an index sees of a learning set (index_db::add_vectors, databases.hpp:270-298): with K_coarse > 0 the
// residual to the nearest coarse centroid (find_k_neighbors with k = 1: the loop of kmeans_fast_iterations above), with a rotation
// rotated[r] = sum_c x[c] * rotation[r][c] in one sequential sum (pq4::rotate_multiple_vectors).  Either may be absent.
inline std::vector<float> pq_train_front(const float* vecs, size_t n, int dim, int K_coarse, const float* coarse, const float* rotation) {
    std::vector<float> out(vecs, vecs + n * (size_t)dim);
    std::vector<float> cn((size_t)std::max(K_coarse, 0)), tmp((size_t)dim);
    for (int k = 0; k < K_coarse; ++k) cn[k] = sqnorm(coarse + (size_t)k * dim, dim);
    for (size_t i = 0; i < n; ++i) {
        float* x = out.data() + i * dim;
        if (K_coarse > 0) {
            const float xn = sqnorm(x, dim);
            int best = 0;
            float bestd = expansion_dist(x, coarse, dim, xn, cn[0]);
            for (int k = 1; k < K_coarse; ++k) {
                const float s = expansion_dist(x, coarse + (size_t)k * dim, dim, xn, cn[k]);
                if (!(s >= bestd)) { bestd = s; best = k; }
            }
            for (int d = 0; d < dim; ++d) x[d] = x[d] - coarse[(size_t)best * dim + d];
        }
        if (rotation) {
            for (int r = 0; r < dim; ++r) {
                float acc = 0;
                for (int c = 0; c < dim; ++c) acc += x[c] * rotation[(size_t)r * dim + c];
                tmp[r] = acc;
            }
            std::copy(tmp.begin(), tmp.end(), x);
        }
    }
    return out;
}

// CPU twin of qadc_pq_train_host (the definition it is tested against bit for bit): sub-quantizer m = kmeans_fast_iterations on a
// copy of columns [m dsub, (m + 1) dsub) of the front's output, started from codebooks[m].  codebooks [sq_count][2^sq_bits][dsub]
// in and out; codes (nullable): the last round's assignment in the encoder's layout — sq_bits 4: [n][sq_count / 2], the even
// sub-quantizer in the low nibble; 8: [n][sq_count].  Returns the centroids that hold a NaN.  iters == 0 changes nothing.
// repair: every round is a repaired round (include/qadc.h "Empty-cluster repair"); *repaired (nullable) = the vectors moved in all
// rounds and sub-spaces.
inline std::uint64_t pq_train_iterations(const float* vecs, size_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                                         const float* rotation, float* codebooks, int iters, std::uint8_t* codes, int div_mode, bool repair,
                                         std::uint64_t* repaired) {
    if (repaired) *repaired = 0;
    if ((sq_bits != 4 && sq_bits != 8) || sq_count <= 0 || dim <= 0 || dim % sq_count || (sq_bits == 4 && sq_count % 2))
        throw std::runtime_error("pq_train_iterations: sq_bits 4 or 8, dim a multiple of sq_count");
    const int ds = dim / sq_count, K = 1 << sq_bits;
    const size_t cs = sq_bits == 4 ? (size_t)sq_count / 2 : (size_t)sq_count;
    if (iters > 0) {
        const std::vector<float> x = pq_train_front(vecs, n, dim, K_coarse, coarse, rotation);
        std::vector<float> slice(n * (size_t)ds);
        std::vector<int> assign(n);
        if (codes) std::fill(codes, codes + n * cs, (std::uint8_t)0);
        for (int m = 0; m < sq_count; ++m) {
            for (size_t i = 0; i < n; ++i) std::copy(x.begin() + i * dim + (size_t)m * ds, x.begin() + i * dim + (size_t)(m + 1) * ds, slice.begin() + i * ds);
            kmeans_fast_iterations(slice.data(), n, ds, K, codebooks + (size_t)m * K * ds, iters, assign.data(), div_mode, repair, repaired);
            if (!codes) continue;
            for (size_t i = 0; i < n; ++i) {
                if (sq_bits == 8) codes[i * cs + m] = (std::uint8_t)assign[i];
                else codes[i * cs + m / 2] |= (std::uint8_t)(assign[i] << (4 * (m & 1)));
            }
        }
    }
    std::uint64_t empty = 0;
    for (size_t r = 0; r < (size_t)sq_count * K; ++r) {
        bool nan = false;
        for (int d = 0; d < ds; ++d) nan = nan || codebooks[r * ds + d] != codebooks[r * ds + d];
        empty += nan;
    }
    return empty;
}

inline std::uint64_t pq_train_iterations(const float* vecs, size_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                                         const float* rotation, float* codebooks, int iters, std::uint8_t* codes, int div_mode = 1) {
    return pq_train_iterations(vecs, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, codebooks, iters, codes, div_mode, false, nullptr);
}

// CPU twin of qadc_pq_update16_host: the centroid update for 16-bit sub-quantizers alone, from given codes.  vecs [n][dim] as the
// quantizer sees them, codes [n][sq_count] -> codebooks [sq_count][65536][dsub], every centroid written (NaN where empty), and
// counts [sq_count][65536] (nullable).  One pass in vector order: every running sum takes its members in ascending index.
inline void pq_update16(const float* vecs, size_t n, int dim, int sq_count, const std::uint16_t* codes, float* codebooks,
                        std::uint32_t* counts, int div_mode = 1) {
    if (sq_count <= 0 || dim <= 0 || dim % sq_count) throw std::runtime_error("pq_update16: dim a positive multiple of sq_count");
    const int ds = dim / sq_count;
    const size_t K = 65536;
    std::vector<std::uint32_t> cnt((size_t)sq_count * K, 0u);
    std::fill(codebooks, codebooks + (size_t)sq_count * K * ds, 0.0f);
    for (size_t i = 0; i < n; ++i)
        for (int m = 0; m < sq_count; ++m) {
            const size_t r = (size_t)m * K + codes[i * sq_count + m];
            cnt[r]++;
            for (int d = 0; d < ds; ++d) codebooks[r * ds + d] += vecs[i * dim + (size_t)m * ds + d];
        }
    for (size_t r = 0; r < (size_t)sq_count * K; ++r) {
        const volatile float rcp = 1.0f / (float)(int)cnt[r];     // (volatile: the host compiler must not fold the two forms)
        for (int d = 0; d < ds; ++d) {
            float& c = codebooks[r * ds + d];
            c = div_mode ? c * rcp : c / (float)(int)cnt[r];
        }
    }
    if (counts) std::copy(cnt.begin(), cnt.end(), counts);
}

// CPU twin of qadc_pq_train16_host: pq_train_iterations for 65536 centroids per sub-quantizer (sq_count 2, 4 or 8), codes (nullable)
// uint16 [n][sq_count].  Returns the centroids that hold a NaN.  iters == 0 changes nothing and writes no code.
// repair, repaired: as for pq_train_iterations.
inline std::uint64_t pq_train16_iterations(const float* vecs, size_t n, int dim, int sq_count, int K_coarse, const float* coarse,
                                           const float* rotation, float* codebooks, int iters, std::uint16_t* codes, int div_mode, bool repair,
                                           std::uint64_t* repaired) {
    if (repaired) *repaired = 0;
    if ((sq_count != 2 && sq_count != 4 && sq_count != 8) || dim <= 0 || dim % sq_count)
        throw std::runtime_error("pq_train16_iterations: sq_count 2, 4 or 8, dim a multiple of it");
    const int ds = dim / sq_count, K = 65536;
    if (iters > 0) {
        const std::vector<float> x = pq_train_front(vecs, n, dim, K_coarse, coarse, rotation);
        std::vector<float> slice(n * (size_t)ds);
        std::vector<int> assign(n);
        for (int m = 0; m < sq_count; ++m) {
            for (size_t i = 0; i < n; ++i) std::copy(x.begin() + i * dim + (size_t)m * ds, x.begin() + i * dim + (size_t)(m + 1) * ds, slice.begin() + i * ds);
            kmeans_fast_iterations(slice.data(), n, ds, K, codebooks + (size_t)m * K * ds, iters, assign.data(), div_mode, repair, repaired);
            if (codes)
                for (size_t i = 0; i < n; ++i) codes[i * sq_count + m] = (std::uint16_t)assign[i];
        }
    }
    std::uint64_t empty = 0;
    for (size_t r = 0; r < (size_t)sq_count * K; ++r) {
        bool nan = false;
        for (int d = 0; d < ds; ++d) nan = nan || codebooks[r * ds + d] != codebooks[r * ds + d];
        empty += nan;
    }
    return empty;
}

inline std::uint64_t pq_train16_iterations(const float* vecs, size_t n, int dim, int sq_count, int K_coarse, const float* coarse,
                                           const float* rotation, float* codebooks, int iters, std::uint16_t* codes, int div_mode = 1) {
    return pq_train16_iterations(vecs, n, dim, sq_count, K_coarse, coarse, rotation, codebooks, iters, codes, div_mode, false, nullptr);
}

// The product quantizer learned on the GPU: `iters` rounds from `seed` [sq_count][2^sq_bits][dim / sq_count] on the learning set
// (made residuals to `coarse` and rotated where given: what indexdb_create1 / indexdb_create2 put before the quantizer).  The
// result carries the rotation, so that pq_to_data_file writes a .pq.data or .opq.data the reference's executables read.
inline io::pq_data learn_pq_hip(const float* vecs, size_t n, int dim, int sq_count, int sq_bits, const float* seed, int iters,
                                int K_coarse = 0, const float* coarse = nullptr, const float* rotation = nullptr, int device = 0,
                                std::uint64_t* empty_out = nullptr, bool repair = false, std::uint64_t* repaired_out = nullptr) {
    io::pq_data pq;
    pq.dim = dim;
    pq.sq_count = sq_count;
    pq.sq_bits = sq_bits;
    if (sq_count <= 0 || dim <= 0 || sq_bits <= 0 || sq_bits > 16 || !seed) throw std::runtime_error("learn_pq_hip: bad arguments");
    pq.centroids.assign(seed, seed + pq.all_centroids_dim());
    if (rotation) {
        pq.is_opq = true;
        pq.rotation.assign(rotation, rotation + (size_t)dim * dim);
    }
    if (sq_bits == 16) {                                        // 65536 centroids per sub-quantizer: the sorted update
        if (qadc_pq_train16_repair_host(vecs, n, dim, sq_count, K_coarse, coarse, rotation, pq.centroids.data(), iters, nullptr, empty_out, 1, 1,
                                        repair ? 1 : 0, repaired_out, device) != QADC_OK)
            throw std::runtime_error(std::string("qadc_pq_train16_host: ") + qadc_last_error());
        return pq;
    }
    if (qadc_pq_train_repair_host(vecs, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, pq.centroids.data(), iters, nullptr, empty_out, 1,
                                  1, repair ? 1 : 0, repaired_out, device) != QADC_OK)
        throw std::runtime_error(std::string("qadc_pq_train_host: ") + qadc_last_error());
    return pq;
}

// CPU twin of qadc_opq_cross_host (the definition it is tested against bit for bit): M [dim][dim] doubles = X0^T Y.  X0 = the front's
// output without a rotation; Y[i][b] = codebooks[m][code(i, m)][b - m dsub], m = b / dsub, the codes in the encoder's layout.  Per
// block of QADC_OPQ_BLOCK vectors one float chain acc = fmaf(X0[i][a], Y[i][b], acc) in ascending i from 0.0f; the blocks' partials
// are added in ascending order in double.
inline void opq_cross(const float* vecs, size_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                      const std::uint8_t* codes, const float* codebooks, double* M) {
    if ((sq_bits != 4 && sq_bits != 8) || sq_count <= 0 || dim <= 0 || dim % sq_count || (sq_bits == 4 && sq_count % 2))
        throw std::runtime_error("opq_cross: sq_bits 4 or 8, dim a multiple of sq_count");
    const int ds = dim / sq_count, K = 1 << sq_bits;
    const size_t cs = sq_bits == 4 ? (size_t)sq_count / 2 : (size_t)sq_count, d = (size_t)dim;
    const std::vector<float> x0 = pq_train_front(vecs, n, dim, K_coarse, coarse, nullptr);
    std::vector<float> partial(d * d), y(d);
    std::fill(M, M + d * d, 0.0);
    for (size_t first = 0; first < n; first += QADC_OPQ_BLOCK) {
        std::fill(partial.begin(), partial.end(), 0.0f);
        for (size_t i = first; i < std::min(n, first + (size_t)QADC_OPQ_BLOCK); ++i) {
            for (int m = 0; m < sq_count; ++m) {
                const int code = sq_bits == 8 ? codes[i * cs + m] : (codes[i * cs + m / 2] >> (4 * (m & 1))) & 15;
                std::copy(codebooks + ((size_t)m * K + code) * ds, codebooks + ((size_t)m * K + code + 1) * ds, y.begin() + (size_t)m * ds);
            }
            for (size_t a = 0; a < d; ++a)
                for (size_t b = 0; b < d; ++b) partial[a * d + b] = std::fmaf(x0[i * d + a], y[b], partial[a * d + b]);
        }
        for (size_t e = 0; e < d * d; ++e) M[e] += (double)partial[e];
    }
}

// CPU twin of qadc_opq_train_host: the loop of include/qadc.h written with pq_train_iterations, opq_cross and procrustes.
// rotation [dim][dim] in and out (the identity for none), codebooks in and out, codes (nullable) of the closing rounds.  Returns the
// centroids that hold a NaN; *rounds_done (nullable): rotation updates completed.  Throws where a Procrustes solve does not converge.
// repair: the loop of the repaired calls; *repaired (nullable) = the vectors moved in all rounds and sub-spaces.
inline std::uint64_t opq_train_iterations(const float* vecs, size_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                                          float* rotation, float* codebooks, int outer, int inner, std::uint8_t* codes, int div_mode,
                                          int* rounds_done, bool repair, std::uint64_t* repaired) {
    std::uint64_t moved = 0, total = 0;
    if (repaired) *repaired = 0;
    if (!rotation || outer < 0 || inner < 1) throw std::runtime_error("opq_train_iterations: a rotation, outer >= 0, inner >= 1");
    const size_t cs = sq_bits == 4 ? (size_t)sq_count / 2 : (size_t)sq_count;
    std::vector<std::uint8_t> round_codes(n * cs);
    std::vector<double> M((size_t)dim * dim);
    int done = 0;
    for (int t = 0; t < outer; ++t) {
        pq_train_iterations(vecs, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, codebooks, inner, round_codes.data(), div_mode, repair, &moved);
        total += moved;
        opq_cross(vecs, n, dim, sq_count, sq_bits, K_coarse, coarse, round_codes.data(), codebooks, M.data());
        const int rc = procrustes(M.data(), dim, rotation);
        if (rc == kProcrustesNotFinite) break;                      // the rotation stays as it is
        if (rc != kProcrustesOk) throw std::runtime_error("opq_train_iterations: the Procrustes solve did not converge");
        ++done;
    }
    if (rounds_done) *rounds_done = done;
    const std::uint64_t empty = pq_train_iterations(vecs, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, codebooks, inner, codes, div_mode, repair, &moved);
    if (repaired) *repaired = total + moved;
    return empty;
}

inline std::uint64_t opq_train_iterations(const float* vecs, size_t n, int dim, int sq_count, int sq_bits, int K_coarse, const float* coarse,
                                          float* rotation, float* codebooks, int outer, int inner, std::uint8_t* codes, int div_mode = 1,
                                          int* rounds_done = nullptr) {
    return opq_train_iterations(vecs, n, dim, sq_count, sq_bits, K_coarse, coarse, rotation, codebooks, outer, inner, codes, div_mode, rounds_done, false,
                                nullptr);
}

// The OPQ rotation and its product quantizer learned on the GPU (qadc_opq_train_host) from `seed` and a start rotation (NULL: the
// identity): an io::pq_data with is_opq set, so that pq_to_data_file writes the .opq.data the reference's executables read.
inline io::pq_data learn_opq_hip(const float* vecs, size_t n, int dim, int sq_count, int sq_bits, const float* seed, int outer, int inner = 1,
                                 int K_coarse = 0, const float* coarse = nullptr, const float* rotation = nullptr, int device = 0,
                                 std::uint64_t* empty_out = nullptr, int* rounds_done_out = nullptr, bool repair = false,
                                 std::uint64_t* repaired_out = nullptr) {
    io::pq_data pq;
    pq.dim = dim;
    pq.sq_count = sq_count;
    pq.sq_bits = sq_bits;
    if (sq_count <= 0 || dim <= 0 || sq_bits <= 0 || sq_bits > 16 || !seed) throw std::runtime_error("learn_opq_hip: bad arguments");
    pq.centroids.assign(seed, seed + pq.all_centroids_dim());
    pq.is_opq = true;
    pq.rotation.assign((size_t)dim * dim, 0.0f);
    for (int r = 0; r < dim; ++r) pq.rotation[(size_t)r * dim + r] = 1.0f;
    if (rotation) pq.rotation.assign(rotation, rotation + (size_t)dim * dim);
    if (qadc_opq_train_repair_host(vecs, n, dim, sq_count, sq_bits, K_coarse, coarse, pq.rotation.data(), pq.centroids.data(), outer, inner, nullptr,
                                   empty_out, rounds_done_out, 1, 1, repair ? 1 : 0, repaired_out, device) != QADC_OK)
        throw std::runtime_error(std::string("qadc_opq_train_host: ") + qadc_last_error());
    return pq;
}

// CPU twin of qadc_kmeans_seed_host (the definition it is tested against bit for bit): kmeans_seed of host/kmeans_seed.hpp on the
// front's output.  centres [sq_count][k][dim / sq_count], rows [sq_count][k] (nullable); returns the fallback picks.
inline std::uint64_t kmeans_seed(const float* vecs, size_t n, int dim, int sq_count, size_t k, int K_coarse, const float* coarse,
                                 const float* rotation, std::uint64_t seed, float* centres, std::uint32_t* rows) {
    if (!vecs || n == 0 || dim <= 0) throw std::runtime_error("kmeans_seed: vectors [n][dim], n > 0");
    const std::vector<float> x = pq_train_front(vecs, n, dim, K_coarse, coarse, rotation);
    return kmeans_seed(x.data(), n, dim, sq_count, k, seed, centres, rows);
}

// k-means++ seeding on the GPU (qadc_kmeans_seed_host): k D^2 picks in every sub-space at once -> [sq_count][k][dim / sq_count], the
// sub-vectors of the picked rows of the learning set as the quantizer sees it (residuals to `coarse`, rotated, where given).
// rows_out [sq_count][k] and fallbacks_out: nullable.
inline std::vector<float> seed_kmeanspp_hip(const float* vecs, size_t n, int dim, int sq_count, size_t k, std::uint64_t seed, int K_coarse = 0,
                                            const float* coarse = nullptr, const float* rotation = nullptr, int device = 0,
                                            std::uint32_t* rows_out = nullptr, std::uint64_t* fallbacks_out = nullptr) {
    if (sq_count <= 0 || dim <= 0 || dim % sq_count) throw std::runtime_error("seed_kmeanspp_hip: dim a positive multiple of sq_count");
    std::vector<float> centres(k * (size_t)dim);
    if (qadc_kmeans_seed_host(vecs, n, dim, sq_count, (std::int64_t)k, K_coarse, coarse, rotation, seed, centres.data(), rows_out, fallbacks_out,
                              device) != QADC_OK)
        throw std::runtime_error(std::string("qadc_kmeans_seed_host: ") + qadc_last_error());
    return centres;
}

// learn_pq_hip / learn_opq_hip without a caller-made seed: the codebooks start from seed_kmeanspp_hip(k = 2^sq_bits) on the same front
inline io::pq_data learn_pq_hip(const float* vecs, size_t n, int dim, int sq_count, int sq_bits, std::uint64_t seed, int iters, int K_coarse = 0,
                                const float* coarse = nullptr, const float* rotation = nullptr, int device = 0,
                                std::uint64_t* empty_out = nullptr, bool repair = false, std::uint64_t* repaired_out = nullptr) {
    if (sq_bits <= 0 || sq_bits > 16) throw std::runtime_error("learn_pq_hip: bad arguments");
    const std::vector<float> start = seed_kmeanspp_hip(vecs, n, dim, sq_count, (size_t)1 << sq_bits, seed, K_coarse, coarse, rotation, device);
    return learn_pq_hip(vecs, n, dim, sq_count, sq_bits, start.data(), iters, K_coarse, coarse, rotation, device, empty_out, repair, repaired_out);
}

// (seeded under the start rotation, NULL: the identity)
inline io::pq_data learn_opq_hip(const float* vecs, size_t n, int dim, int sq_count, int sq_bits, std::uint64_t seed, int outer, int inner = 1,
                                 int K_coarse = 0, const float* coarse = nullptr, const float* rotation = nullptr, int device = 0,
                                 std::uint64_t* empty_out = nullptr, int* rounds_done_out = nullptr, bool repair = false,
                                 std::uint64_t* repaired_out = nullptr) {
    if (sq_bits <= 0 || sq_bits > 16) throw std::runtime_error("learn_opq_hip: bad arguments");
    const std::vector<float> start = seed_kmeanspp_hip(vecs, n, dim, sq_count, (size_t)1 << sq_bits, seed, K_coarse, coarse, rotation, device);
    return learn_opq_hip(vecs, n, dim, sq_count, sq_bits, start.data(), outer, inner, K_coarse, coarse, rotation, device, empty_out,
                         rounds_done_out, repair, repaired_out);
}

constexpr int kmeans_iter_max = 50;                            // databases.cpp:92

// `seed` [K][dim]: what the reference gets from cv::kmeans(KMEANS_PP_CENTERS, 2 iterations)
inline std::vector<float> learn_coarse_quantizer_hip(const float* vecs, size_t n, int dim, int K, const float* seed,
                                                     int device = 0) {
    std::vector<float> centroids(seed, seed + (size_t)K * dim);
    if (qadc_kmeans_iterations_host(vecs, n, dim, K, centroids.data(), kmeans_iter_max - 2, nullptr, device) != QADC_OK)
        throw std::runtime_error(std::string("qadc_kmeans_iterations_host: ") + qadc_last_error());
    return centroids;
}

// The same without a caller-made seed: K k-means++ picks on the whole vectors (seed_kmeanspp_hip with one sub-space) stand in for the
// reference's two OpenCV iterations, then the kmeans_iter_max - 2 fast iterations.
inline std::vector<float> learn_coarse_quantizer_hip(const float* vecs, size_t n, int dim, int K, std::uint64_t seed, int device = 0) {
    if (K <= 0) throw std::runtime_error("learn_coarse_quantizer_hip: K > 0");
    const std::vector<float> start = seed_kmeanspp_hip(vecs, n, dim, 1, (size_t)K, seed, 0, nullptr, nullptr, device);
    return learn_coarse_quantizer_hip(vecs, n, dim, K, start.data(), device);
}

// PQ codes back to vectors on the GPU: out [n][dim]; err (nullable) [n] against vectors.  The CPU twin is pq_decode (host/pq_decode.hpp).
inline std::vector<float> pq_decode_hip(int sq_count, int sq_bits, int dim, const float* codebooks, const float* rotation, int K,
                                        const float* coarse, const std::int32_t* assign, const void* codes, size_t n,
                                        const float* vectors = nullptr, std::vector<float>* err = nullptr, int device = 0) {
    std::vector<float> out(n * (size_t)dim);
    if (err) err->assign(n, 0.0f);
    if (qadc_pq_decode_host(sq_count, sq_bits, dim, codebooks, rotation, K, coarse, assign, codes, n, vectors, out.data(),
                            err ? err->data() : nullptr, device) != QADC_OK)
        throw std::runtime_error(std::string("qadc_pq_decode_host: ") + qadc_last_error());
    return out;
}

// The vectors behind `keys` of a float-ADC index (or a view of a 4-bit index) under the quantizers it holds: [count][dim];
// where (nullable): (partition << 32 | row) of each key's row, QADC_RECONSTRUCT_MISSING where no row holds it.
inline std::vector<float> reconstruct_hip(qadc_adc_index* idx, int dim, const std::uint32_t* keys, size_t count,
                                          std::vector<std::uint64_t>* where = nullptr) {
    std::vector<float> out(count * (size_t)dim);
    if (where) where->assign(count, 0);
    if (qadc_adc_index_reconstruct(idx, keys, count, out.data(), where ? where->data() : nullptr) != QADC_OK)
        throw std::runtime_error(std::string("qadc_adc_index_reconstruct: ") + qadc_last_error());
    return out;
}

}  // namespace qadc
