// overlap_check.cpp — host/overlap.h exercised by a program of its own, so that test_overlap_cpu.py can build it with g++ and
// -fsanitize=address,undefined (nothing loaded into Python is instrumented).  usage: overlap_check <directory for its files>
// Exit status 0 when every check held; the first failed check is named on stderr.
#include "../cuda_gcn_amd/host/overlap.h"
#include <cstdlib>

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "overlap_check: line %d: %s\n", __LINE__, #cond);  \
            return 1;                                                          \
        }                                                                      \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const std::string dir = argv[1];
    std::string err;
    OverlapMetrics m;
    const int64_t zero[8] = {};
    CHECK(gcn_overlap_metrics(zero, &m, &err) == 0 && m.triangles == 0 && m.transitivity == 0.0 && m.avg_clustering == 0.0);
    const int64_t full[8] = {4, 3, 10, 18, 12, 6, 3, (int64_t)((uint64_t)5 << 31)};
    CHECK(gcn_overlap_metrics(full, &m, &err) == 0 && m.triangles == 2 && m.transitivity == 12.0 / 18.0 && m.avg_clustering == 2.5 / 4);
    const int64_t neg[8] = {4, 3, -1, 18, 12, 6, 3, 0}, above[8] = {4, 5, 10, 18, 12, 6, 3, 0};
    CHECK(gcn_overlap_metrics(neg, &m, &err) == -1 && gcn_overlap_metrics(above, &m, &err) == -1 && gcn_overlap_metrics(nullptr, &m, &err) == -1);
    CHECK(gcn_overlap_coefficient(5, 1) == 0.0 && gcn_overlap_coefficient(0, 0) == 0.0 && gcn_overlap_coefficient(3, 3) == 0.5);
    CHECK(gcn_overlap_jaccard(0, 0) == 0.0 && gcn_overlap_jaccard(1, 4) == 0.25);
    CHECK(gcn_overlap_weight(OVERLAP_ADAMIC_ADAR, 1) == 0 && gcn_overlap_weight(OVERLAP_RESOURCE_ALLOCATION, 0) == 0);
    CHECK(gcn_overlap_weight(OVERLAP_RESOURCE_ALLOCATION, 2) == (int64_t)1 << 31 && gcn_overlap_weight(OVERLAP_ADAMIC_ADAR, 2) == 6196328019LL);
    const uint64_t D = ((uint64_t)1 << 24) * (((uint64_t)1 << 24) - 1) - 2;   // near 2^48
    CHECK(gcn_overlap_ratio(D, D) == (uint64_t)1 << 32 && gcn_overlap_ratio(0, D) == 0 && gcn_overlap_ratio(D - 1, D) == ((uint64_t)1 << 32) - 1);
    CHECK(gcn_overlap_ratio(1, 2) == (uint64_t)1 << 31 && gcn_overlap_ratio(1, 3) == 1431655765u);
    TriangleReport r, back;
    for (int k = 0; k < 8; k++) r.totals[k] = full[k];
    r.node = {3, 5, 5, 9}; r.deg = {0, 1, 3, 3}; r.t2 = {0, 0, 6, 6};
    const std::string path = dir + "/t.txt";
    CHECK(gcn_triangles_write(path.c_str(), r, &err) == 0 && gcn_triangles_read(path.c_str(), &back, &err) == 0);
    CHECK(back.node == r.node && back.deg == r.deg && back.t2 == r.t2);
    for (int k = 0; k < 8; k++) CHECK(back.totals[k] == r.totals[k]);
    TriangleReport none;
    CHECK(gcn_triangles_write((dir + "/e.txt").c_str(), none, &err) == 0 && gcn_triangles_read((dir + "/e.txt").c_str(), &back, &err) == 0 && back.node.empty());
    r.deg.pop_back();
    CHECK(gcn_triangles_write(path.c_str(), r, &err) == -1);
    CHECK(gcn_triangles_read((dir + "/missing.txt").c_str(), &back, &err) == -1 && err.find("cannot open") != std::string::npos);
    FILE *f = fopen((dir + "/cut.txt").c_str(), "w");
    CHECK(f != nullptr);
    fprintf(f, "gcn-triangles 1 rows 2000000000\ntotals 1 0 0 0 0 0 0 0\n3 0 0 0.0\n");
    fclose(f);
    CHECK(gcn_triangles_read((dir + "/cut.txt").c_str(), &back, &err) == -1 && err.find("not a complete triangle report") != std::string::npos);
    printf("overlap_check ok\n");
    return 0;
}
