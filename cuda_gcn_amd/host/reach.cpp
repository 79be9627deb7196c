// reach.cpp — host/reach.h's bodies: accuracy by distance from the labels out of integer counts, and the text report.
// No GPU, no HIP header: a stand-alone program can link this file alone.
#include "reach.h"
#include <cinttypes>
#include <cstdio>
#include <cstring>

namespace {
int fail(std::string *err, const char *what, const std::string &why) {
    if (err) *err = std::string(what) + ": " + why;
    return -1;
}
double ratio(double a, double b) { return b > 0 ? a / b : 0.0; }
void add(ReachRow &r, const int64_t *cell) {
    r.rows += cell[0]; r.labelled += cell[1]; r.correct += cell[2]; r.nearest_correct += cell[3];
}
void finish(ReachRow &r) {
    r.accuracy = ratio((double)r.correct, (double)r.labelled);
    r.nearest_accuracy = ratio((double)r.nearest_correct, (double)r.labelled);
}
constexpr size_t MAX_LEVELS = (size_t)1 << 31;
}  // namespace

int gcn_reach_metrics(const int64_t *strata, int hops, int layers, ReachMetrics *out, std::string *err) {
    const char *what = "reach_metrics";
    if (!strata || !out || hops < 1 || hops > REACH_MAX_HOPS) return fail(err, what, "invalid argument (strata of (hops + 2) x 4 cells, 1 <= hops <= 32)");
    if (layers < 0 || layers >= hops)
        return fail(err, what, "layers must be in 0..hops - 1 (the buckets 0 .. layers are exact distances only then), got " + std::to_string(layers) +
                                   " with hops = " + std::to_string(hops));
    for (int b = 0; b < hops + 2; b++) {
        const int64_t *c = strata + (size_t)b * 4;
        if (c[0] < 0 || c[1] < 0 || c[2] < 0 || c[3] < 0 || c[1] > c[0] || c[2] > c[1] || c[3] > c[1])
            return fail(err, what, "a negative count in strata, or a count above the one it is part of");
    }
    ReachMetrics m;
    m.hops = hops; m.layers = layers;
    m.by_distance.assign((size_t)hops + 2, ReachRow());
    for (int b = 0; b < hops + 2; b++) {
        const int64_t *c = strata + (size_t)b * 4;
        add(m.by_distance[b], c);
        add(b <= layers ? m.inside : m.outside, c);
        add(m.all, c);
        finish(m.by_distance[b]);
    }
    finish(m.inside); finish(m.outside); finish(m.all);
    m.unreachable = strata[(size_t)(hops + 1) * 4];
    m.unreachable_share = ratio((double)m.unreachable, (double)m.all.rows);
    *out = m;
    return 0;
}

// ---- the text report ---------------------------------------------------------------------------------------------------------

int gcn_reach_write(const char *path, const ReachCounts &c, std::string *err) {
    const char *what = "reach_write";
    if (!path || c.hops < 1 || c.hops > REACH_MAX_HOPS || c.strata.size() != (size_t)(c.hops + 2) * 4 || c.level_counts.empty())
        return fail(err, what, "invalid argument (the tables do not have the shapes of hops, or no level count)");
    ReachMetrics m;
    if (gcn_reach_metrics(c.strata.data(), c.hops, c.layers, &m, err) != 0) return -1;
    FILE *f = fopen(path, "w");
    if (!f) return fail(err, what, std::string("cannot open ") + path);
    bool ok = fprintf(f, "gcn-reach 1 hops %d layers %d levels %zu\n", c.hops, c.layers, c.level_counts.size() - 1) > 0;
    auto line = [&](const char *name, const int64_t *v, size_t n) {
        ok = ok && fprintf(f, "%s", name) > 0;
        for (size_t i = 0; ok && i < n; i++) ok = fprintf(f, " %" PRId64, v[i]) > 0;
        ok = ok && fprintf(f, "\n") > 0;
    };
    auto derived = [&](const char *name, const ReachRow &r) {
        ok = ok && fprintf(f, "# %s %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %.9f %.9f\n", name, r.rows, r.labelled, r.correct, r.nearest_correct,
                           r.accuracy, r.nearest_accuracy) > 0;
    };
    ok = ok && fprintf(f, "# by_distance: bucket rows labelled correct nearest_correct accuracy nearest_label_accuracy (bucket %d: %d hops or more; %d: unreachable)\n",
                       c.hops, c.hops, c.hops + 1) > 0;
    for (int b = 0; ok && b < c.hops + 2; b++) derived(std::to_string(b).c_str(), m.by_distance[b]);
    ok = ok && fprintf(f, "# groups (inside: at most %d hops from a source; outside: the rest): name rows labelled correct nearest_correct accuracy nearest_label_accuracy\n",
                       c.layers) > 0;
    derived("inside", m.inside);
    derived("outside", m.outside);
    derived("all", m.all);
    ok = ok && fprintf(f, "# unreachable %" PRId64 " share %.9f\n", m.unreachable, m.unreachable_share) > 0;
    ok = ok && fprintf(f, "# totals: rows components largest_component unseeded_components unseeded_nodes seeded_rows\n") > 0;
    const int64_t info[3] = {c.sources, c.unlabelled, c.rounds};
    line("info", info, 3);
    line("totals", c.totals, 6);
    line("level_counts", c.level_counts.data(), c.level_counts.size());
    for (int b = 0; b < c.hops + 2; b++) line("strata", c.strata.data() + (size_t)b * 4, 4);
    if (fclose(f) != 0) ok = false;
    return ok ? 0 : fail(err, what, std::string("could not write ") + path);
}

int gcn_reach_read(const char *path, ReachCounts *out, std::string *err) {
    const char *what = "reach_read";
    if (!path || !out) return fail(err, what, "invalid argument");
    FILE *f = fopen(path, "r");
    if (!f) return fail(err, what, std::string("cannot open ") + path);
    ReachCounts c;
    int version = 0;
    unsigned long long levels = 0;
    if (fscanf(f, "gcn-reach %d hops %d layers %d levels %llu", &version, &c.hops, &c.layers, &levels) != 4 || version != 1 || c.hops < 1 ||
        c.hops > REACH_MAX_HOPS || c.layers < 0 || c.layers >= c.hops || levels >= MAX_LEVELS) {
        fclose(f);
        return fail(err, what, std::string(path) + " does not start with a gcn-reach 1 header");
    }
    int64_t info[3] = {};
    c.strata.assign((size_t)(c.hops + 2) * 4, 0);
    // the named lines in the writer's order: every line of one name holds `per_line` integers
    struct Block { const char *name; int64_t *at; size_t lines, per_line; };
    const Block head[2] = {{"info", info, 1, 3}, {"totals", c.totals, 1, 6}};
    bool ok = true;
    char word[64];
    auto read_block = [&](const Block &b) {
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
    };
    for (const Block &b : head) read_block(b);
    if (ok) {                                                  // the level counts one by one: a short file must not size an array
        Block one = {"level_counts", nullptr, 1, 0};
        read_block(one);
        for (unsigned long long i = 0; ok && i <= levels; i++) {
            int64_t x = 0;
            ok = fscanf(f, "%" SCNd64, &x) == 1;
            if (ok) c.level_counts.push_back(x);
        }
    }
    read_block(Block{"strata", c.strata.data(), (size_t)c.hops + 2, 4});
    fclose(f);
    if (!ok) return fail(err, what, std::string(path) + " is not a complete reach report");
    c.sources = info[0]; c.unlabelled = info[1]; c.rounds = info[2];
    *out = c;
    return 0;
}
