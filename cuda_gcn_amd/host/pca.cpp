// pca.cpp — gcn_sym_eigen and gcn_pca_from_scatter (pca.h has the definitions).  Host only, float64.
#include "pca.h"
#include <algorithm>
#include <cmath>
#include <numeric>

static int pca_fail(std::string *err, const char *what, const std::string &why) {
    if (err) *err = std::string(what) + ": " + why;
    return -1;
}

int gcn_sym_eigen(const double *S, int h, double *lambda, double *V, std::string *err) {
    const char *what = "sym_eigen";
    if (!S || !lambda || !V) return pca_fail(err, what, "invalid argument");
    if (h < 1 || h > PCA_MAX_DIM) return pca_fail(err, what, "the width must be in 1..256, got " + std::to_string(h));
    const size_t n = (size_t)h;
    for (size_t a = 0; a < n; a++)
        for (size_t b = 0; b < n; b++) {
            if (!std::isfinite(S[a * n + b])) return pca_fail(err, what, "entry (" + std::to_string(a) + ", " + std::to_string(b) + ") is not finite");
            if (S[a * n + b] != S[b * n + a])
                return pca_fail(err, what, "the matrix is not symmetric at (" + std::to_string(a) + ", " + std::to_string(b) + ")");
        }
    std::vector<double> A(S, S + n * n);                        // the upper triangle is worked on
    std::vector<double> Vt(n * n, 0.0);                         // row j = vector j: a rotation touches two contiguous rows
    std::vector<double> d(n), base(n), z(n, 0.0);
    for (size_t i = 0; i < n; i++) {
        Vt[i * n + i] = 1.0;
        d[i] = base[i] = A[i * n + i];
    }
    const int max_sweeps = 100;
    int sweep = 1;
    for (; sweep <= max_sweeps; sweep++) {
        double off = 0.0;
        for (size_t p = 0; p + 1 < n; p++)
            for (size_t q = p + 1; q < n; q++) off += std::fabs(A[p * n + q]);
        if (off == 0.0) break;
        const double thresh = sweep < 4 ? 0.2 * off / ((double)n * (double)n) : 0.0;
        for (size_t p = 0; p + 1 < n; p++)
            for (size_t q = p + 1; q < n; q++) {
                const double apq = A[p * n + q];
                const double g = 100.0 * std::fabs(apq);
                if (sweep > 4 && std::fabs(d[p]) + g == std::fabs(d[p]) && std::fabs(d[q]) + g == std::fabs(d[q])) {
                    A[p * n + q] = 0.0;                         // below the last bit of both diagonal entries
                    continue;
                }
                if (!(std::fabs(apq) > thresh)) continue;
                const double diff = d[q] - d[p];
                double t;
                if (std::fabs(diff) + g == std::fabs(diff)) t = apq / diff;
                else {
                    const double theta = 0.5 * diff / apq;
                    t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                    if (theta < 0.0) t = -t;
                }
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
                const double shift = t * apq;
                z[p] -= shift; z[q] += shift;
                d[p] -= shift; d[q] += shift;
                A[p * n + q] = 0.0;
                auto rot = [&](double &x, double &y) {
                    const double gx = x, hy = y;
                    x = gx - s * (hy + gx * tau);
                    y = hy + s * (gx - hy * tau);
                };
                for (size_t j = 0; j < p; j++) rot(A[j * n + p], A[j * n + q]);
                for (size_t j = p + 1; j < q; j++) rot(A[p * n + j], A[j * n + q]);
                for (size_t j = q + 1; j < n; j++) rot(A[p * n + j], A[q * n + j]);
                double *vp = &Vt[p * n], *vq = &Vt[q * n];
                for (size_t j = 0; j < n; j++) rot(vp[j], vq[j]);
            }
        for (size_t i = 0; i < n; i++) {
            base[i] += z[i];
            d[i] = base[i];
            z[i] = 0.0;
        }
    }
    if (sweep > max_sweeps) return pca_fail(err, what, "no convergence in " + std::to_string(max_sweeps) + " sweeps");
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return d[x] > d[y]; });
    for (size_t j = 0; j < n; j++) {
        const double *v = &Vt[(size_t)order[j] * n];
        size_t top = 0;
        for (size_t a = 1; a < n; a++)
            if (std::fabs(v[a]) > std::fabs(v[top])) top = a;
        const double sign = v[top] < 0.0 ? -1.0 : 1.0;
        lambda[j] = d[order[j]];
        for (size_t a = 0; a < n; a++) V[a * n + j] = sign * v[a];
    }
    return 0;
}

int gcn_pca_from_scatter(const double *S, const double *mean, int64_t rows, int h, int k, bool whiten, PcaFit *fit, std::string *err) {
    const char *what = "pca_from_scatter";
    if (!S || !fit) return pca_fail(err, what, "invalid argument");
    if (h < 1 || h > PCA_MAX_DIM) return pca_fail(err, what, "the width must be in 1..256, got " + std::to_string(h));
    if (k < 1 || k > h) return pca_fail(err, what, "k must be in 1.." + std::to_string(h) + ", got " + std::to_string(k));
    if (rows < 2) return pca_fail(err, what, "at least 2 rows, got " + std::to_string(rows));
    if (mean)
        for (int a = 0; a < h; a++)
            if (!std::isfinite(mean[a])) return pca_fail(err, what, "the mean is not finite");
    PcaFit f;
    f.h = h; f.k = k; f.rows = rows;
    const size_t n = (size_t)h;
    f.eigenvalues.resize(n);
    f.components.resize(n * n);
    std::string why;
    if (gcn_sym_eigen(S, h, f.eigenvalues.data(), f.components.data(), &why) != 0) {
        if (err) *err = std::string(what) + ": " + why;
        return -1;
    }
    double total = 0.0;
    for (double &l : f.eigenvalues) {
        if (l < 0.0) l = 0.0;
        total += l;
    }
    const double floor_ = (double)h * 0x1p-52 * f.eigenvalues[0], dof = (double)(rows - 1);
    f.explained_variance.resize(n);
    f.explained_variance_ratio.resize(n);
    f.singular_values.resize(n);
    for (size_t j = 0; j < n; j++) {
        const double l = f.eigenvalues[j];
        if (l > floor_) f.rank++;
        f.explained_variance[j] = l / dof;
        f.explained_variance_ratio[j] = total > 0.0 ? l / total : 0.0;
        f.singular_values[j] = std::sqrt(l);
    }
    if (whiten) {
        f.scale.assign((size_t)k, 0.0);
        for (int j = 0; j < k && j < f.rank; j++) {
            const double sc = 1.0 / std::sqrt(f.eigenvalues[j] / dof);
            f.scale[j] = std::isfinite(sc) ? sc : 0.0;
        }
    }
    *fit = std::move(f);
    return 0;
}
