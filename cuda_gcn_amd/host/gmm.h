// gmm.h — the information criteria of a fitted Gaussian mixture (csrc/gmm.hip, ModelQueries::gmm): the one place the number of free
// parameters, BIC and AIC are derived.  Host only, no GPU.  scikit-learn's definitions (GaussianMixture.bic / .aic / _n_parameters).
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

struct GmmInformation {
    int64_t n_parameters = 0;
    double bic = 0, aic = 0;
};

// lower_bound: the mean of log p(x_i) over `points` rows.  Parameters: k dim means, k - 1 weights, and k dim (diagonal) or k
// (spherical) variances.  bic = -2 n lb + p log n, aic = -2 n lb + 2 p.  -1 with *err: points < 1, k < 1, dim < 1, a lower bound
// that is NaN.
inline int gcn_gmm_information(double lower_bound, int64_t points, int k, int dim, bool spherical, GmmInformation *out, std::string *err) {
    if (!out || points < 1 || k < 1 || dim < 1 || lower_bound != lower_bound) {
        if (err) *err = "gmm_information: invalid argument (points >= 1, k >= 1, dim >= 1, a lower bound that is a number)";
        return -1;
    }
    GmmInformation r;
    r.n_parameters = (int64_t)k * dim + (spherical ? (int64_t)k : (int64_t)k * dim) + k - 1;
    const double n = (double)points, p = (double)r.n_parameters;
    r.bic = -2.0 * n * lower_bound + p * std::log(n);
    r.aic = -2.0 * n * lower_bound + 2.0 * p;
    *out = r;
    return 0;
}
