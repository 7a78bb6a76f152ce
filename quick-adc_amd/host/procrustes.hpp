// Orthogonal Procrustes for OPQ learning — HIP-free, C++14, header only.  The library
// (qadc_procrustes_host, the loop of qadc_opq_train_*) and the CPU twin (host/db_build.hpp: opq_train_iterations) both include
// this file, so the two agree bit for bit.
//
//   procrustes(M, dim, R, sweeps): the orthogonal R [dim][dim] that maximises tr(R M).  With M = U S V^T that is R = V U^T.  In the
//   project's convention rotated[r] = sum_c x[c] R[r][c]; with M = X^T Y (row a = component of X, column b = component of Y) the
//   result is the rotation that brings X closest to Y: X R^T ~ Y.
//
// The SVD is a one-sided (Hestenes) Jacobi in double: plane rotations of column pairs (p, q), p < q in cyclic order, applied to
// A = M and accumulated in V, until a whole sweep rotates nothing — every pair then has |a_p . a_q| <= kProcrustesTol |a_p| |a_q|.
// The columns of A V are then U S.  No step depends on anything but the entries of M: the same M gives the same R everywhere.
// A column whose norm is at most dim * 2^-52 times the largest has no direction of its own (rank-deficient M, the zero matrix
// included): its left vector is completed by Gram-Schmidt (two passes) against the unit vectors e_0, e_1, ... in index order, so
// that R stays orthogonal.  The result is rounded to float.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace qadc {

constexpr int kProcrustesMaxDim = 1024;       // O(dim^3) per sweep on the host
constexpr int kProcrustesMaxSweeps = 64;      // cyclic Jacobi converges quadratically; a well-posed M takes about ten
constexpr double kProcrustesTol = 1e-14;      // a pair is rotated while |a_p . a_q| > tol * |a_p| |a_q|

enum { kProcrustesOk = 0, kProcrustesBadArg = 1, kProcrustesNotFinite = 2, kProcrustesNoConvergence = 3 };

// M [dim][dim] row-major -> R [dim][dim] row-major (float); *sweeps (nullable): Jacobi sweeps run, the last one rotating nothing.
// Returns kProcrustesOk, or an error with R untouched: a non-finite entry of M, dim outside [1, kProcrustesMaxDim], or the sweep
// cap reached (never a non-orthogonal matrix).
inline int procrustes(const double* M, int dim, float* R, int* sweeps = nullptr) {
    if (!M || !R || dim <= 0 || dim > kProcrustesMaxDim) return kProcrustesBadArg;
    const size_t d = (size_t)dim;
    for (size_t i = 0; i < d * d; ++i)
        if (!std::isfinite(M[i])) return kProcrustesNotFinite;
    // column-major copies: a[p * d + i] = A[i][p], v[p * d + i] = V[i][p]
    std::vector<double> a(d * d), v(d * d, 0.0);
    for (size_t i = 0; i < d; ++i)
        for (size_t p = 0; p < d; ++p) a[p * d + i] = M[i * d + p];
    for (size_t p = 0; p < d; ++p) v[p * d + p] = 1.0;
    int sweep = 0;
    bool converged = false;
    while (!converged && sweep < kProcrustesMaxSweeps) {
        ++sweep;
        converged = true;
        for (size_t p = 0; p + 1 < d; ++p)
            for (size_t q = p + 1; q < d; ++q) {
                double* ap = &a[p * d];
                double* aq = &a[q * d];
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (size_t i = 0; i < d; ++i) {
                    alpha += ap[i] * ap[i];
                    beta += aq[i] * aq[i];
                    gamma += ap[i] * aq[i];
                }
                if (alpha == 0.0 || beta == 0.0) continue;
                if (!(std::fabs(gamma) > kProcrustesTol * std::sqrt(alpha * beta))) continue;
                converged = false;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta < 0.0 ? -1.0 : 1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                double* vp = &v[p * d];
                double* vq = &v[q * d];
                for (size_t i = 0; i < d; ++i) {
                    const double x = ap[i], y = aq[i];
                    ap[i] = c * x - s * y;
                    aq[i] = s * x + c * y;
                    const double vx = vp[i], vy = vq[i];
                    vp[i] = c * vx - s * vy;
                    vq[i] = s * vx + c * vy;
                }
            }
    }
    if (!converged) return kProcrustesNoConvergence;
    // U: the columns of A V normalised; the columns without a direction are completed afterwards
    std::vector<double> norm(d);
    double largest = 0.0;
    for (size_t p = 0; p < d; ++p) {
        double s2 = 0.0;
        for (size_t i = 0; i < d; ++i) s2 += a[p * d + i] * a[p * d + i];
        norm[p] = std::sqrt(s2);
        if (norm[p] > largest) largest = norm[p];
    }
    const double floor_ = largest * (double)dim * 2.220446049250313e-16;
    std::vector<char> have(d, 0);
    for (size_t p = 0; p < d; ++p) {
        if (!(norm[p] > floor_)) continue;
        have[p] = 1;
        for (size_t i = 0; i < d; ++i) a[p * d + i] /= norm[p];
    }
    size_t next_unit = 0;
    std::vector<double> w(d);
    for (size_t p = 0; p < d; ++p) {
        if (have[p]) continue;
        bool done = false;
        while (!done && next_unit < d) {
            std::fill(w.begin(), w.end(), 0.0);
            w[next_unit++] = 1.0;
            for (int pass = 0; pass < 2; ++pass)
                for (size_t k = 0; k < d; ++k) {
                    if (!have[k]) continue;
                    double dot = 0.0;
                    for (size_t i = 0; i < d; ++i) dot += w[i] * a[k * d + i];
                    for (size_t i = 0; i < d; ++i) w[i] -= dot * a[k * d + i];
                }
            double s2 = 0.0;
            for (size_t i = 0; i < d; ++i) s2 += w[i] * w[i];
            // The squared residuals of all unit vectors sum to dim - (vectors held) >= 1; the rejected ones hold at most 1/4 of that
            // together, so one not yet tried keeps more than 1 / (4 dim): the walk in index order always finds enough.
            if (s2 * (double)dim * 4.0 > 1.0) {
                const double nw = std::sqrt(s2);
                for (size_t i = 0; i < d; ++i) a[p * d + i] = w[i] / nw;
                have[p] = 1;
                done = true;
            }
        }
        if (!done) return kProcrustesNoConvergence;              // (unreachable for an orthonormal set: kept as a refusal, not a guess)
    }
    // R = V U^T: R[r][c] = sum_k V[r][k] U[c][k]
    std::vector<double> row(d);
    for (size_t r = 0; r < d; ++r) {
        std::fill(row.begin(), row.end(), 0.0);
        for (size_t k = 0; k < d; ++k) {
            const double vrk = v[k * d + r];
            const double* uk = &a[k * d];
            for (size_t c = 0; c < d; ++c) row[c] += vrk * uk[c];
        }
        for (size_t c = 0; c < d; ++c) R[r * d + c] = (float)row[c];
    }
    if (sweeps) *sweeps = sweep;
    return kProcrustesOk;
}

}  // namespace qadc
