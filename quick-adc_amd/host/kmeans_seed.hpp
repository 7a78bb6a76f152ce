// CPU twin of qadc_kmeans_seed_host (include/qadc.h "k-means++ seeding"): the definition the device result
// is tested against bit for bit, written plainly.  HIP-free and free of the C-ABI: it works on the learning set as the quantizer
// sees it (host/db_build.hpp puts pq_train_front before it).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <vector>

namespace qadc {

constexpr int kKmeansSeedRadix = 64;

// u(m, t): splitmix64's finaliser on seed + golden * (((m << 32) | t) + 1), the top 53 bits as a double in [0, 1)
inline double kmeans_seed_uniform(std::uint64_t seed, std::uint32_t m, std::uint32_t t) {
    std::uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((((std::uint64_t)m << 32) | (std::uint64_t)t) + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// the balanced binary tree sum of v[first .. first + len), len a power of two; entries at or past `have` count as 0.0
inline double kmeans_seed_balanced(const double* v, std::size_t have, std::size_t first, std::size_t len) {
    if (len == 1) return first < have ? v[first] : 0.0;
    return kmeans_seed_balanced(v, have, first, len / 2) + kmeans_seed_balanced(v, have, first + len / 2, len / 2);
}

// the child of a node that `target` names: children [first, first + 64) of `v` in ascending order under a sequential prefix;
// *target becomes the remainder below the entered child.  -1: no child is positive (the caller never enters such a node).
inline int kmeans_seed_child(const double* v, std::size_t have, std::size_t first, double* target) {
    double c = 0.0, last_c = 0.0;
    int last = -1;
    for (int j = 0; j < kKmeansSeedRadix; ++j) {
        const double child = first + (std::size_t)j < have ? v[first + j] : 0.0;
        if (child > 0.0) { last = j; last_c = c; }
        if (*target < c + child) { *target = *target - c; return j; }
        c = c + child;
    }
    if (last >= 0) *target = *target - last_c;
    return last;
}

// vectors [n][dim] -> centres [sq_count][k][dim / sq_count], rows [sq_count][k] (nullable); returns the fallback picks.
inline std::uint64_t kmeans_seed(const float* x, std::size_t n, int dim, int sq_count, std::size_t k, std::uint64_t seed, float* centres,
                                 std::uint32_t* rows) {
    if (!x || !centres || n == 0 || n >= (1ull << 32) || k < 1 || k > n || sq_count < 1 || dim <= 0 || dim % sq_count)
        throw std::runtime_error("kmeans_seed: 0 < n < 2^32, 1 <= k <= n, dim a positive multiple of sq_count");
    const int ds = dim / sq_count;
    const float inf = std::numeric_limits<float>::infinity();
    std::uint64_t fallbacks = 0;
    std::vector<float> mind(n);
    std::vector<char> picked(n);
    std::vector<std::vector<double>> level;
    for (int m = 0; m < sq_count; ++m) {
        std::fill(mind.begin(), mind.end(), inf);
        std::fill(picked.begin(), picked.end(), (char)0);
        std::size_t cursor = 0;
        for (std::size_t t = 0; t < k; ++t) {
            const double u = kmeans_seed_uniform(seed, (std::uint32_t)m, (std::uint32_t)t);
            std::size_t row = 0;
            bool fallback = false;
            if (t == 0) {
                const std::uint64_t r = (std::uint64_t)(u * (double)n);
                row = r < n - 1 ? (std::size_t)r : n - 1;
            } else {
                // the distances to the centre picked last, the weights and the tree: levels 1 and 2 always, then up to one node
                const float* c = centres + ((std::size_t)m * k + (t - 1)) * ds;
                level.assign(1, std::vector<double>(n));
                for (std::size_t i = 0; i < n; ++i) {
                    float acc = 0.0f;
                    for (int d = 0; d < ds; ++d) {
                        const float diff = x[i * dim + (std::size_t)m * ds + d] - c[d];
                        acc = std::fmaf(diff, diff, acc);
                    }
                    mind[i] = acc < mind[i] ? acc : mind[i];
                    level[0][i] = mind[i] < inf ? (double)mind[i] : 0.0;
                }
                while (level.size() < 3 || level.back().size() > 1) {
                    const std::vector<double>& below = level.back();
                    std::vector<double> up((below.size() + kKmeansSeedRadix - 1) / kKmeansSeedRadix);
                    for (std::size_t j = 0; j < up.size(); ++j)
                        up[j] = kmeans_seed_balanced(below.data(), below.size(), j * kKmeansSeedRadix, kKmeansSeedRadix);
                    level.push_back(up);
                }
                const double root = level.back()[0];
                if (root == 0.0) {
                    while (picked[cursor]) ++cursor;                 // k <= n: an unpicked row exists
                    row = cursor;
                    fallback = true;
                } else {
                    double target = u * root;
                    std::size_t node = 0;
                    for (std::size_t l = level.size() - 1; l >= 1; --l)
                        node = node * kKmeansSeedRadix +
                               (std::size_t)kmeans_seed_child(level[l - 1].data(), level[l - 1].size(), node * kKmeansSeedRadix, &target);
                    row = node;
                }
            }
            fallbacks += fallback;
            picked[row] = 1;
            std::memcpy(centres + ((std::size_t)m * k + t) * ds, x + row * dim + (std::size_t)m * ds, sizeof(float) * ds);
            if (rows) rows[(std::size_t)m * k + t] = (std::uint32_t)row;
        }
    }
    return fallbacks;
}

}  // namespace qadc
