// overlap.h — triangles, clustering coefficients and common-neighbour link scores from integer counts (beyond the reference).
// Host only: no GPU, no HIP header; a stand-alone program can include this file alone.  The ONE place where what
// gcnhip_overlap_rows / _pairs counted (csrc/overlap.hip has the definitions) becomes a measure: ModelQueries::clustering's and
// ::link_overlap's callers (the Python binding, gcn-hip's GCN_TRIANGLES) hand it the tables.
//
// totals [8] = {listed rows in range, rows with d >= 2, sum d, sum D, sum t2, max t2, max d, ratio_sum}, D = d (d - 1), ratio_sum =
// the sum over the rows with d >= 2 of floor(t2 . 2^32 / D).
//   triangles = sum t2 / 6 (a symmetric graph's triangles when every row is listed), transitivity = sum t2 / sum D,
//   avg_clustering = ratio_sum / 2^32 / listed rows (rows with d < 2 count as 0), per node c = t2 / D, 0 when d < 2.
// A pair's scores from cn, un and the two set lengths: jaccard = cn / un, preferential attachment = d(a) d(b); a weighted score is
// wsum / 2^32 with the fixed-point table round(2^32 / ln d) (Adamic-Adar, d >= 2) or round(2^32 / d) (resource allocation,
// d >= 1), 0 otherwise: within cn . 2^-33 of the float64 sum.  A zero denominator gives 0, never NaN; a negative count is an error.
#pragma once
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

constexpr int OVERLAP_ADAMIC_ADAR = 1, OVERLAP_RESOURCE_ALLOCATION = 2;   // bits of a weight mask

struct OverlapMetrics {
    int64_t triangles = 0;
    double transitivity = 0, avg_clustering = 0;
};
// the integers of one report, as gcn-hip writes them and reads them back
struct TriangleReport {
    int64_t totals[8] = {};
    std::vector<int32_t> node, deg;
    std::vector<int64_t> t2;
};

inline int overlap_fail(std::string *err, const char *what, const std::string &why) {
    if (err) *err = std::string(what) + ": " + why;
    return -1;
}

// floor(t2 . 2^32 / D) for t2 <= D < 2^48: two 16-bit long-division steps in 64-bit integers (the kernel's own steps)
inline uint64_t gcn_overlap_ratio(uint64_t t2, uint64_t D) {
    uint64_t q = t2 / D, r = t2 % D;
    for (int step = 0; step < 2; step++) {
        r <<= 16;
        q = (q << 16) | (r / D);
        r %= D;
    }
    return q;
}

inline double gcn_overlap_coefficient(int64_t t2, int64_t d) { return d >= 2 ? (double)t2 / ((double)d * (double)(d - 1)) : 0.0; }

inline int gcn_overlap_metrics(const int64_t *totals, OverlapMetrics *out, std::string *err) {
    const char *what = "overlap_metrics";
    if (!totals || !out) return overlap_fail(err, what, "invalid argument");
    for (int k = 0; k < 7; k++)
        if (totals[k] < 0) return overlap_fail(err, what, "a negative count in totals");
    if (totals[1] > totals[0] || totals[4] > totals[3]) return overlap_fail(err, what, "a count in totals above the one it is part of");
    OverlapMetrics m;
    m.triangles = totals[4] / 6;
    m.transitivity = totals[3] > 0 ? (double)totals[4] / (double)totals[3] : 0.0;
    m.avg_clustering = totals[0] > 0 ? (double)(uint64_t)totals[7] / 4294967296.0 / (double)totals[0] : 0.0;
    *out = m;
    return 0;
}

inline double gcn_overlap_jaccard(int64_t cn, int64_t un) { return un > 0 ? (double)cn / (double)un : 0.0; }

// the fixed-point weight of a node with a set of d entries
inline int64_t gcn_overlap_weight(int kind, int64_t d) {
    if (kind == OVERLAP_ADAMIC_ADAR) return d >= 2 ? (int64_t)std::llround(4294967296.0 / std::log((double)d)) : 0;
    return d >= 1 ? (int64_t)std::llround(4294967296.0 / (double)d) : 0;
}

// The text report: a header line, the totals, then `node deg t2 clustering` per listed node; the reader takes the integers alone.
inline int gcn_triangles_write(const char *path, const TriangleReport &r, std::string *err) {
    const char *what = "triangles_write";
    if (!path || r.deg.size() != r.node.size() || r.t2.size() != r.node.size()) return overlap_fail(err, what, "invalid argument");
    OverlapMetrics m;
    if (gcn_overlap_metrics(r.totals, &m, err) != 0) return -1;
    FILE *f = fopen(path, "w");
    if (!f) return overlap_fail(err, what, std::string("cannot open ") + path);
    bool ok = fprintf(f, "gcn-triangles 1 rows %zu\n", r.node.size()) > 0;
    ok = ok && fprintf(f, "# triangles %" PRId64 " transitivity %.9f avg_clustering %.9f\n", m.triangles, m.transitivity, m.avg_clustering) > 0;
    ok = ok && fprintf(f, "totals") > 0;
    for (int k = 0; ok && k < 8; k++) ok = fprintf(f, " %" PRId64, r.totals[k]) > 0;
    ok = ok && fprintf(f, "\n# node deg t2 clustering\n") > 0;
    for (size_t i = 0; ok && i < r.node.size(); i++)
        ok = fprintf(f, "%d %d %" PRId64 " %.9f\n", r.node[i], r.deg[i], r.t2[i], gcn_overlap_coefficient(r.t2[i], r.deg[i])) > 0;
    if (fclose(f) != 0) ok = false;
    return ok ? 0 : overlap_fail(err, what, std::string("could not write ") + path);
}

inline int gcn_triangles_read(const char *path, TriangleReport *out, std::string *err) {
    const char *what = "triangles_read";
    if (!path || !out) return overlap_fail(err, what, "invalid argument");
    FILE *f = fopen(path, "r");
    if (!f) return overlap_fail(err, what, std::string("cannot open ") + path);
    TriangleReport r;
    int version = 0;
    unsigned long long rows = 0;
    char line[256];
    bool ok = fgets(line, sizeof line, f) && sscanf(line, "gcn-triangles %d rows %llu", &version, &rows) == 2 && version == 1;
    if (!ok) {
        fclose(f);
        return overlap_fail(err, what, std::string(path) + " does not start with a gcn-triangles 1 header");
    }
    bool have_totals = false;
    while (ok && fgets(line, sizeof line, f)) {                // row by row: a short file must not size an array
        if (line[0] == '#' || line[0] == '\n') continue;
        if (!have_totals) {
            int64_t *t = r.totals;
            ok = sscanf(line, "totals %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64, t, t + 1, t + 2, t + 3,
                        t + 4, t + 5, t + 6, t + 7) == 8;
            have_totals = true;
            continue;
        }
        int node = 0, deg = 0;
        int64_t t2 = 0;
        ok = sscanf(line, "%d %d %" SCNd64, &node, &deg, &t2) == 3 && deg >= 0 && t2 >= 0;
        if (ok) { r.node.push_back(node); r.deg.push_back(deg); r.t2.push_back(t2); }
    }
    fclose(f);
    if (!ok || !have_totals || r.node.size() != rows) return overlap_fail(err, what, std::string(path) + " is not a complete triangle report");
    *out = r;
    return 0;
}
