// louvain.h — what of the Louvain communities is formed on the host, without a GPU: the modularity from the exact integer sums
// (csrc/louvain.hip has the definitions).  Q = num / M2^2 in float64, 0 when M2 = 0.
#pragma once
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

inline double gcn_modularity_from_sums(int64_t numerator, int64_t m2) {
    return m2 > 0 ? (double)numerator / ((double)m2 * (double)m2) : 0.0;
}

// one level of a run: its vertices, the sweeps it ran, the numerator it ended on
struct LouvainLevel {
    int64_t vertices = 0, sweeps = 0, numerator = 0;
};
struct LouvainRun {
    std::vector<LouvainLevel> levels;
    int64_t communities = 0, numerator = 0, m2 = 0, contingency_rows = 0, skipped = 0;
};

// The report gcn-hip writes for GCN_COMMUNITIES (model.read_communities reads it back): a header with the counts, a line with Q
// (17 significant digits: the float64 itself) and the integers it comes from, then `node community` per node in id order.
inline int gcn_communities_write(const char *path, const LouvainRun &run, const std::vector<int32_t> &labels, std::string *err) {
    FILE *f = path ? fopen(path, "w") : nullptr;
    if (!f) {
        if (err) *err = std::string("communities_write: cannot open ") + (path ? path : "(null)");
        return -1;
    }
    bool ok = fprintf(f, "gcn-communities 1 nodes %zu communities %" PRId64 " levels %zu\n", labels.size(), run.communities, run.levels.size()) > 0;
    ok = ok && fprintf(f, "# Q %.17g numerator %" PRId64 " m2 %" PRId64 "\n# node community\n", gcn_modularity_from_sums(run.numerator, run.m2), run.numerator,
                       run.m2) > 0;
    for (size_t i = 0; ok && i < labels.size(); i++) ok = fprintf(f, "%zu %d\n", i, labels[i]) > 0;
    if (fclose(f) != 0) ok = false;
    if (!ok && err) *err = std::string("communities_write: could not write ") + path;
    return ok ? 0 : -1;
}
