// pca_host.cpp — the host-only part of the PCA fit (include/dgn.h): merging dgn_pca_moments and
// solving the 35 x 35 eigenproblem (reference pca.cpp:15-34: the right singular vectors and
// s^2 / (N - 1) of the centred matrix are the eigenpairs of its covariance). No HIP, no context:
// this file builds with a plain C++ compiler and is part of the `make sanitize` program.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../include/dgn.h"

namespace {

constexpr int kD = DGN_BETTI_DIM;

// symmetric eigen-decomposition A = V diag(w) V^T by cyclic Jacobi, A (d x d, row-major, destroyed)
// converged to machine precision; the rotation PCA::fit uses (cpp/src/pca.cpp)
void jacobi_eigen(std::vector<double>& a, int d, std::vector<double>& w, std::vector<double>& v) {
    v.assign(static_cast<size_t>(d * d), 0.0);
    for (int i = 0; i < d; ++i) v[static_cast<size_t>(i * d + i)] = 1.0;
    auto A = [&](int i, int j) -> double& { return a[static_cast<size_t>(i * d + j)]; };
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < d; ++i) {
            diag += A(i, i) * A(i, i);
            for (int j = i + 1; j < d; ++j) off += A(i, j) * A(i, j);
        }
        if (off <= 1e-30 * diag || off == 0.0) break;
        for (int p = 0; p < d; ++p)
            for (int q = p + 1; q < d; ++q) {
                const double apq = A(p, q);
                if (apq == 0.0) continue;
                const double theta = (A(q, q) - A(p, p)) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < d; ++k) {  // A <- A J (columns p, q)
                    const double akp = A(k, p), akq = A(k, q);
                    A(k, p) = c * akp - s * akq;
                    A(k, q) = s * akp + c * akq;
                }
                for (int k = 0; k < d; ++k) {  // A <- J^T A (rows p, q)
                    const double apk = A(p, k), aqk = A(q, k);
                    A(p, k) = c * apk - s * aqk;
                    A(q, k) = s * apk + c * aqk;
                }
                for (int k = 0; k < d; ++k) {
                    double& vkp = v[static_cast<size_t>(k * d + p)];
                    double& vkq = v[static_cast<size_t>(k * d + q)];
                    const double x = vkp, y = vkq;
                    vkp = c * x - s * y;
                    vkq = s * x + c * y;
                }
            }
    }
    w.resize(static_cast<size_t>(d));
    for (int i = 0; i < d; ++i) w[static_cast<size_t>(i)] = A(i, i);
}

}  // namespace

extern "C" {

void dgn_pca_moments_init(dgn_pca_moments* m) {
    if (m) std::memset(m, 0, sizeof *m);
}

int dgn_pca_moments_merge(dgn_pca_moments* into, const dgn_pca_moments* other) {
    if (!into || !other || into->n < 0 || other->n < 0 || into->skipped < 0 || other->skipped < 0) return DGN_ERR_ARG;
    if (into == other) return DGN_ERR_ARG;
    into->skipped += other->skipped;
    if (other->n == 0) return DGN_OK;
    if (into->n == 0) {
        into->n = other->n;
        std::memcpy(into->mean, other->mean, sizeof into->mean);
        std::memcpy(into->m2, other->m2, sizeof into->m2);
        return DGN_OK;
    }
    const double na = static_cast<double>(into->n), nb = static_cast<double>(other->n), n = na + nb;
    double delta[kD];
    for (int a = 0; a < kD; ++a) delta[a] = other->mean[a] - into->mean[a];
    const double wgt = na * nb / n;
    for (int a = 0; a < kD; ++a)
        for (int b = a; b < kD; ++b) {
            const double v = into->m2[a * kD + b] + other->m2[a * kD + b] + delta[a] * delta[b] * wgt;
            into->m2[a * kD + b] = into->m2[b * kD + a] = v;
        }
    for (int a = 0; a < kD; ++a) into->mean[a] += delta[a] * (nb / n);
    into->n += other->n;
    return DGN_OK;
}

int dgn_pca_solve(const dgn_pca_moments* m, int32_t k, double* mean, double* components, double* explained_ratio) {
    if (!m || !mean || k < 0 || k > kD || m->n < 2 || (k > 0 && (!components || !explained_ratio))) return DGN_ERR_ARG;
    const double denom = static_cast<double>(m->n - 1);
    std::vector<double> cov(static_cast<size_t>(kD * kD));
    for (int a = 0; a < kD; ++a)
        for (int b = a; b < kD; ++b)  // the upper triangle is the matrix: exactly symmetric input
            cov[static_cast<size_t>(a * kD + b)] = cov[static_cast<size_t>(b * kD + a)] = m->m2[a * kD + b] / denom;
    std::vector<double> w, v;
    jacobi_eigen(cov, kD, w, v);
    std::vector<int> order(static_cast<size_t>(kD));
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return w[static_cast<size_t>(a)] > w[static_cast<size_t>(b)]; });
    double total = 0.0;
    for (double e : w) total += std::max(e, 0.0);
    for (int a = 0; a < kD; ++a) mean[a] = m->mean[a];
    for (int c = 0; c < k; ++c) {
        const int src = order[static_cast<size_t>(c)];
        int big = 0;
        for (int a = 1; a < kD; ++a)
            if (std::fabs(v[static_cast<size_t>(a * kD + src)]) > std::fabs(v[static_cast<size_t>(big * kD + src)])) big = a;
        const double sign = v[static_cast<size_t>(big * kD + src)] < 0 ? -1.0 : 1.0;
        for (int a = 0; a < kD; ++a) components[a * k + c] = sign * v[static_cast<size_t>(a * kD + src)];
        explained_ratio[c] = total > 0 ? std::max(w[static_cast<size_t>(src)], 0.0) / total : 0.0;
    }
    return DGN_OK;
}

}  // extern "C"
