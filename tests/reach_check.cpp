// reach_check.cpp — host/reach.h exercised by a program of its own, so that test_reach_cpu.py can build it with g++ and
// -fsanitize=address,undefined (nothing loaded into Python is instrumented).  usage: reach_check <directory for its files>
// Exit status 0 when every check held; the first failed check is named on stderr.
#include "../cuda_gcn_amd/host/reach.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "reach_check: line %d: %s\n", __LINE__, #cond);    \
            return 1;                                                          \
        }                                                                      \
    } while (0)

static bool finite_row(const ReachRow &r) { return std::isfinite(r.accuracy) && std::isfinite(r.nearest_accuracy); }

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const std::string dir = argv[1];
    std::string err;
    ReachMetrics m;
    for (int hops = 1; hops <= REACH_MAX_HOPS; hops++) {       // every table size, all zero and filled, every allowed depth
        std::vector<int64_t> zero((size_t)(hops + 2) * 4, 0), full(zero.size());
        for (int b = 0; b < hops + 2; b++) {
            full[b * 4] = 10 + b; full[b * 4 + 1] = 8 + b; full[b * 4 + 2] = b; full[b * 4 + 3] = 8;
        }
        for (int layers = 0; layers < hops; layers++) {
            CHECK(gcn_reach_metrics(zero.data(), hops, layers, &m, &err) == 0);
            CHECK((int)m.by_distance.size() == hops + 2 && m.all.rows == 0 && m.all.accuracy == 0.0 && m.unreachable_share == 0.0);
            CHECK(gcn_reach_metrics(full.data(), hops, layers, &m, &err) == 0);
            CHECK(m.inside.rows + m.outside.rows == m.all.rows && m.unreachable == 10 + hops + 1);
            for (const ReachRow &r : m.by_distance) CHECK(finite_row(r));
            CHECK(finite_row(m.inside) && finite_row(m.outside) && finite_row(m.all));
        }
        CHECK(gcn_reach_metrics(full.data(), hops, hops, &m, &err) == -1 && err.find("layers must be") != std::string::npos);
        CHECK(gcn_reach_metrics(full.data(), hops, -1, &m, &err) == -1);
        full[2] = full[1] + 1;                                 // more correct rows than labelled ones
        CHECK(gcn_reach_metrics(full.data(), hops, 0, &m, &err) == -1);
        ReachCounts c, back;
        c.hops = hops; c.layers = gcn_reach_layers(hops);
        c.sources = 5; c.unlabelled = 2; c.rounds = 3;
        for (int k = 0; k < 6; k++) c.totals[k] = 100 + k;
        c.level_counts.assign((size_t)hops, 7);
        c.strata = zero;
        c.strata[0] = 4; c.strata[1] = 3; c.strata[2] = 2; c.strata[3] = 1;
        const std::string path = dir + "/r" + std::to_string(hops) + ".txt";
        CHECK(gcn_reach_write(path.c_str(), c, &err) == 0);
        CHECK(gcn_reach_read(path.c_str(), &back, &err) == 0);
        CHECK(back.hops == c.hops && back.layers == c.layers && back.sources == 5 && back.unlabelled == 2 && back.rounds == 3);
        CHECK(back.level_counts == c.level_counts && back.strata == c.strata);
        for (int k = 0; k < 6; k++) CHECK(back.totals[k] == c.totals[k]);
    }
    CHECK(gcn_reach_metrics(nullptr, 3, 2, &m, &err) == -1 && gcn_reach_metrics(nullptr, 0, 0, &m, &err) == -1);
    ReachCounts bad;
    CHECK(gcn_reach_write((dir + "/bad.txt").c_str(), bad, &err) == -1);
    CHECK(gcn_reach_read((dir + "/missing.txt").c_str(), &bad, &err) == -1 && err.find("cannot open") != std::string::npos);
    FILE *f = fopen((dir + "/cut.txt").c_str(), "w");
    CHECK(f != nullptr);
    fprintf(f, "gcn-reach 1 hops 3 layers 2 levels 2000000000\ninfo 1 2 3\ntotals 1 2 3 4 5 6\nlevel_counts 1 2\n");
    fclose(f);
    CHECK(gcn_reach_read((dir + "/cut.txt").c_str(), &bad, &err) == -1 && err.find("not a complete reach report") != std::string::npos);
    printf("reach_check ok\n");
    return 0;
}
