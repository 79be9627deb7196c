// structure.cpp — host/structure.h's bodies: the homophily measures and the strata tables from integer counts, and the text report.
// No GPU, no HIP header: a stand-alone program can link this file alone.
#include "structure.h"
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>

namespace {
int fail(std::string *err, const char *what, const std::string &why) {
    if (err) *err = std::string(what) + ": " + why;
    return -1;
}
double ratio(double a, double b) { return b > 0 ? a / b : 0.0; }
}  // namespace

int gcn_structure_metrics(int C, const int64_t *mix, const int64_t *class_rows, const int64_t *totals, StructureMetrics *out, std::string *err) {
    const char *what = "structure_metrics";
    if (C < 1 || C > STRUCTURE_MAX_CLASSES || !mix || !class_rows || !out) return fail(err, what, "invalid argument (a C x C table and C class rows, 1 <= C <= 64)");
    for (size_t e = 0; e < (size_t)C * C; e++)
        if (mix[e] < 0) return fail(err, what, "a negative count in mix");
    for (int k = 0; k < C; k++)
        if (class_rows[k] < 0) return fail(err, what, "a negative count in class_rows");
    if (totals)
        for (int k = 0; k < 7; k++)                            // totals[7] is an unsigned sum
            if (totals[k] < 0) return fail(err, what, "a negative count in totals");
    StructureMetrics r;
    r.num_classes = C;
    r.class_homophily.assign((size_t)C, 0.0);
    r.compatibility.assign((size_t)C * C, 0.0);
    std::vector<double> row((size_t)C, 0.0);
    double E = 0, trace = 0, R = 0;
    for (int a = 0; a < C; a++) {
        for (int b = 0; b < C; b++) row[a] += (double)mix[(size_t)a * C + b];
        E += row[a];
        trace += (double)mix[(size_t)a * C + a];
        R += (double)class_rows[a];
    }
    for (int a = 0; a < C; a++)
        for (int b = 0; b < C; b++) {
            r.edges += mix[(size_t)a * C + b];
            r.compatibility[(size_t)a * C + b] = ratio((double)mix[(size_t)a * C + b], row[a]);
        }
    r.edge_homophily = ratio(trace, E);
    double excess = 0, p2 = 0;
    for (int k = 0; k < C; k++) {
        r.class_homophily[k] = ratio((double)mix[(size_t)k * C + k], row[k]);
        excess += std::max(0.0, r.class_homophily[k] - ratio((double)class_rows[k], R));
        const double p = ratio(row[k], E);
        p2 += p * p;
        r.labelled_rows += class_rows[k];
    }
    r.class_insensitive_homophily = C > 1 ? excess / (double)(C - 1) : 0.0;
    r.adjusted_homophily = E > 0 && 1.0 - p2 > 0 ? (r.edge_homophily - p2) / (1.0 - p2) : 0.0;
    if (totals) {
        r.rows_with_known = totals[2];
        r.node_homophily = totals[2] > 0 ? (double)(uint64_t)totals[7] / 4294967296.0 / (double)totals[2] : 0.0;
    }
    *out = r;
    return 0;
}

int gcn_strata_tables(int bins, const int64_t *strata, StrataTables *out, std::string *err) {
    const char *what = "structure_metrics";
    if (bins < 1 || bins > STRUCTURE_MAX_BINS || !strata || !out) return fail(err, what, "invalid argument (strata of 32 x (bins + 1) x 2 cells, 1 <= bins <= 32)");
    const int D = STRUCTURE_DEGREE_BUCKETS, A = bins + 1;
    for (int e = 0; e < D * A; e++)
        if (strata[2 * e] < 0 || strata[2 * e + 1] < 0 || strata[2 * e + 1] > strata[2 * e]) return fail(err, what, "a negative count in strata, or more correct rows than rows");
    StrataTables t;
    t.bins = bins;
    t.by_degree.assign((size_t)D, StrataRow());
    t.by_agreement.assign((size_t)A, StrataRow());
    for (int d = 0; d < D; d++) {
        StrataRow &r = t.by_degree[d];
        r.lo = d ? (double)((int64_t)1 << (d - 1)) : 0.0;
        r.hi = d ? (double)(((int64_t)1 << d) - 1) : 0.0;
    }
    for (int a = 0; a < A; a++) {
        StrataRow &r = t.by_agreement[a];
        r.lo = a < bins ? (double)a / bins : -1.0;
        r.hi = a < bins ? (double)(a + 1) / bins : -1.0;
    }
    for (int d = 0; d < D; d++)
        for (int a = 0; a < A; a++) {
            const int64_t rows = strata[(size_t)(d * A + a) * 2], ok = strata[(size_t)(d * A + a) * 2 + 1];
            t.by_degree[d].rows += rows; t.by_degree[d].correct += ok;
            t.by_agreement[a].rows += rows; t.by_agreement[a].correct += ok;
            t.rows += rows; t.correct += ok;
        }
    for (StrataRow &r : t.by_degree) r.accuracy = ratio((double)r.correct, (double)r.rows);
    for (StrataRow &r : t.by_agreement) r.accuracy = ratio((double)r.correct, (double)r.rows);
    *out = t;
    return 0;
}

// ---- the text report ---------------------------------------------------------------------------------------------------------

static bool counts_shaped(const StructureCounts &c) {
    const size_t C = (size_t)c.num_classes;
    return c.num_classes >= 1 && c.num_classes <= STRUCTURE_MAX_CLASSES && c.bins >= 1 && c.bins <= STRUCTURE_MAX_BINS && c.class_rows_truth.size() == C &&
           c.class_rows_pred.size() == C && c.mix_truth.size() == C * C && c.mix_pred.size() == C * C &&
           c.strata.size() == (size_t)STRUCTURE_DEGREE_BUCKETS * (c.bins + 1) * 2;
}

int gcn_structure_write(const char *path, const StructureCounts &c, std::string *err) {
    const char *what = "structure_write";
    if (!path || !counts_shaped(c)) return fail(err, what, "invalid argument (the tables do not have the shapes of num_classes and bins)");
    StructureMetrics mt, mp;
    StrataTables st;
    if (gcn_structure_metrics(c.num_classes, c.mix_truth.data(), c.class_rows_truth.data(), c.totals_truth, &mt, err) != 0) return -1;
    if (gcn_structure_metrics(c.num_classes, c.mix_pred.data(), c.class_rows_pred.data(), c.totals_pred, &mp, err) != 0) return -1;
    if (gcn_strata_tables(c.bins, c.strata.data(), &st, err) != 0) return -1;
    FILE *f = fopen(path, "w");
    if (!f) return fail(err, what, std::string("cannot open ") + path);
    const int C = c.num_classes, A = c.bins + 1;
    bool ok = fprintf(f, "gcn-structure 1 classes %d bins %d\n", C, c.bins) > 0;
    auto line = [&](const char *name, const int64_t *v, size_t n) {
        ok = ok && fprintf(f, "%s", name) > 0;
        for (size_t i = 0; ok && i < n; i++) ok = fprintf(f, " %" PRId64, v[i]) > 0;
        ok = ok && fprintf(f, "\n") > 0;
    };
    auto metrics = [&](const char *name, const StructureMetrics &m) {
        ok = ok && fprintf(f, "# %s edge_homophily=%.9f node_homophily=%.9f adjusted_homophily=%.9f class_insensitive_homophily=%.9f edges=%" PRId64 "\n", name,
                           m.edge_homophily, m.node_homophily, m.adjusted_homophily, m.class_insensitive_homophily, m.edges) > 0;
    };
    auto table = [&](const char *name, const std::vector<StrataRow> &rows) {
        ok = ok && fprintf(f, "# %s: bucket lo hi rows correct accuracy\n", name) > 0;
        for (size_t b = 0; ok && b < rows.size(); b++)
            ok = fprintf(f, "# %zu %.9g %.9g %" PRId64 " %" PRId64 " %.9f\n", b, rows[b].lo, rows[b].hi, rows[b].rows, rows[b].correct, rows[b].accuracy) > 0;
    };
    metrics("truth", mt);
    metrics("pred", mp);
    table("by_degree", st.by_degree);
    table("by_agreement", st.by_agreement);
    line("totals_truth", c.totals_truth, 8);
    line("totals_pred", c.totals_pred, 8);
    line("class_rows_truth", c.class_rows_truth.data(), (size_t)C);
    line("class_rows_pred", c.class_rows_pred.data(), (size_t)C);
    for (int a = 0; a < C; a++) line("mix_truth", c.mix_truth.data() + (size_t)a * C, (size_t)C);
    for (int a = 0; a < C; a++) line("mix_pred", c.mix_pred.data() + (size_t)a * C, (size_t)C);
    for (int d = 0; d < STRUCTURE_DEGREE_BUCKETS; d++) line("strata", c.strata.data() + (size_t)d * A * 2, (size_t)A * 2);
    if (fclose(f) != 0) ok = false;
    return ok ? 0 : fail(err, what, std::string("could not write ") + path);
}

int gcn_structure_read(const char *path, StructureCounts *out, std::string *err) {
    const char *what = "structure_read";
    if (!path || !out) return fail(err, what, "invalid argument");
    FILE *f = fopen(path, "r");
    if (!f) return fail(err, what, std::string("cannot open ") + path);
    StructureCounts c;
    int version = 0;
    if (fscanf(f, "gcn-structure %d classes %d bins %d", &version, &c.num_classes, &c.bins) != 3 || version != 1 || c.num_classes < 1 ||
        c.num_classes > STRUCTURE_MAX_CLASSES || c.bins < 1 || c.bins > STRUCTURE_MAX_BINS) {
        fclose(f);
        return fail(err, what, std::string(path) + " does not start with a gcn-structure 1 header");
    }
    const size_t C = (size_t)c.num_classes, A = (size_t)c.bins + 1;
    // the named lines in the writer's order: every line of one name holds `per_line` integers
    struct Block { const char *name; int64_t *at; size_t lines, per_line; };
    c.class_rows_truth.assign(C, 0); c.class_rows_pred.assign(C, 0);
    c.mix_truth.assign(C * C, 0); c.mix_pred.assign(C * C, 0);
    c.strata.assign((size_t)STRUCTURE_DEGREE_BUCKETS * A * 2, 0);
    const Block blocks[7] = {{"totals_truth", c.totals_truth, 1, 8}, {"totals_pred", c.totals_pred, 1, 8},
                             {"class_rows_truth", c.class_rows_truth.data(), 1, C}, {"class_rows_pred", c.class_rows_pred.data(), 1, C},
                             {"mix_truth", c.mix_truth.data(), C, C}, {"mix_pred", c.mix_pred.data(), C, C},
                             {"strata", c.strata.data(), (size_t)STRUCTURE_DEGREE_BUCKETS, A * 2}};
    bool ok = true;
    char word[64];
    for (const Block &b : blocks)
        for (size_t l = 0; ok && l < b.lines; l++) {
            for (;;) {                                         // the next word that does not open a derived line
                if (fscanf(f, "%63s", word) != 1) { ok = false; break; }
                if (word[0] != '#') break;
                int ch;
                while ((ch = fgetc(f)) != EOF && ch != '\n') {}
            }
            ok = ok && strcmp(word, b.name) == 0;
            for (size_t i = 0; ok && i < b.per_line; i++) ok = fscanf(f, "%" SCNd64, &b.at[l * b.per_line + i]) == 1;
        }
    fclose(f);
    if (!ok) return fail(err, what, std::string(path) + " is not a complete structure report");
    *out = c;
    return 0;
}
