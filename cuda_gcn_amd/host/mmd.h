// mmd.h — the kernel two-sample statistics from the sums csrc/mmd.hip leaves (ModelQueries::mmd): the one place MMD^2 and the
// permutation p-value are derived.  Host only, no GPU.  Gretton et al., "A Kernel Two-Sample Test", JMLR 2012 (eq. 3 and 5).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>

// Per column b = 0 .. cols - 1 (0: the observed groups, 1..: the permuted ones) the sums over ordered pairs, self pairs included and
// each worth exactly 1: aa inside group A (m points), bb inside group B (rest points), ab across.
//   biased[b]   = aa / m^2 + bb / rest^2 - 2 ab / (m rest)
//   unbiased[b] = (aa - m) / (m (m - 1)) + (bb - rest) / (rest (rest - 1)) - 2 ab / (m rest): the self pairs removed analytically.
//                 With m == 1 or rest == 1 a group has no pair of distinct points and the term is undefined: NaN.
//   *p_value    = (1 + #{b >= 1 : biased[b] >= biased[0]}) / cols, the permutation test on the biased statistic (1 with cols == 1).
// -1 with *err: cols < 1, m < 1 or rest < 1, a NULL array.
inline int gcn_mmd_stats(const double *aa, const double *ab, const double *bb, int cols, int64_t m, int64_t rest, double *biased, double *unbiased,
                         double *p_value, std::string *err) {
    if (!aa || !ab || !bb || !biased || !unbiased || !p_value || cols < 1 || m < 1 || rest < 1) {
        if (err) *err = "mmd_stats: invalid argument (at least one column, two groups that are not empty)";
        return -1;
    }
    const double M = (double)m, N = (double)rest, nan = std::numeric_limits<double>::quiet_NaN();
    int64_t at_least = 0;
    for (int b = 0; b < cols; b++) {
        biased[b] = aa[b] / (M * M) + bb[b] / (N * N) - 2.0 * ab[b] / (M * N);
        unbiased[b] = m > 1 && rest > 1 ? (aa[b] - M) / (M * (M - 1.0)) + (bb[b] - N) / (N * (N - 1.0)) - 2.0 * ab[b] / (M * N) : nan;
        if (b >= 1 && biased[b] >= biased[0]) at_least++;
    }
    *p_value = (double)(1 + at_least) / (double)cols;
    return 0;
}
