// pca.h — the symmetric eigenproblem of a scatter matrix and everything a principal component analysis derives from it (beyond
// the reference).  Host only: no GPU, float64 throughout.  The ONE place where a scatter matrix becomes a fit:
// ModelQueries::pca_fit's callers (the Python binding, gcn-hip's GCN_PCA) hand it what gcnhip_pca_scatter summed.
//
// gcn_sym_eigen(S, h, lambda, V): S [h x h] row-major, 1 <= h <= 256, every entry finite and S[a][b] == S[b][a] bit for bit
//   (anything else is refused with a message).  Cyclic Jacobi (Jacobi, 1846; the threshold sweeps and the rotation formulas of
//   Rutishauser, 1966): rotations in row order until every off-diagonal entry is exactly zero; the angle comes from
//   t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), the diagonal is carried as d + the sum of its sweep's corrections.  No
//   absolute threshold anywhere: S and c . S take the same rotations for a power of two c.  lambda [h] descending (equal values
//   in the order of their column); V [h x h], V[a * h + j] = entry a of the unit vector of lambda[j], each vector's entry of
//   largest magnitude positive, the lowest index on equal magnitude.
// gcn_pca_from_scatter(S, mean, rows, h, k, whiten, fit): rows >= 2 valid positions went into S, 1 <= k <= h.
//   eigenvalues [h] = max(lambda, 0) descending; components = V; rank = the number of lambda_j > h . 2^-52 . lambda_1;
//   explained_variance = lambda / (rows - 1); explained_variance_ratio = lambda_j / sum(lambda), 0 when the sum is 0 — never NaN;
//   singular_values = sqrt(lambda); scale [k] = 1 / sqrt(lambda_j / (rows - 1)) for j < rank and 0 past it — never inf — with
//   `whiten`, else empty.  mean [h] (may be NULL) is only checked to be finite.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

constexpr int PCA_MAX_DIM = 256;

struct PcaFit {
    int h = 0, k = 0, rank = 0;
    int64_t rows = 0;
    std::vector<double> eigenvalues, components;               // [h], [h x h] (column j = component j)
    std::vector<double> explained_variance, explained_variance_ratio, singular_values;   // [h]
    std::vector<double> scale;                                 // [k] with whiten, else empty
};

// 0, or -1 with the reason in *err
int gcn_sym_eigen(const double *S, int h, double *lambda, double *V, std::string *err);
int gcn_pca_from_scatter(const double *S, const double *mean, int64_t rows, int h, int k, bool whiten, PcaFit *fit, std::string *err);
