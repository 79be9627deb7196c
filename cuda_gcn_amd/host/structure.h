// structure.h — the label structure of a graph from integer counts (beyond the reference).  Host only: no GPU.  The ONE place where
// what gcnhip_nbr_agreement and gcnhip_strata_counts counted (csrc/structure.hip has the definitions) becomes a report:
// ModelQueries::structure's callers (the Python binding, gcn-hip's GCN_STRUCTURE) hand it the tables.
//
// mix [C x C], mix[a * C + b] = non-loop entries from a row labelled a to a column labelled b; r_a = its row sums, E = their total;
// class_rows [C] = labelled rows per class, R = their total; totals [8] as the kernel file lists them.  A zero denominator gives 0.
//   edge_homophily               = trace(mix) / E
//   class_homophily[k]           = mix[k, k] / r_k
//   compatibility [C x C]        = mix[a, b] / r_a (a zero row stays zero)
//   node_homophily               = totals[7] / 2^32 / totals[2]: the mean over rows with a labelled neighbour of same / known
//                                  (0 without totals)
//   class_insensitive_homophily  = 1 / (C - 1) . sum_k max(0, class_homophily[k] - class_rows[k] / R)     (Lim et al., 2021); 0 at C = 1
//   adjusted_homophily           = (edge_homophily - sum_k p_k^2) / (1 - sum_k p_k^2), p_k = r_k / E     (Platonov et al., 2023)
// strata [32 x (bins + 1) x 2] = (rows, correct) per degree bucket and agreement bucket: the two marginal tables.
//   degree bucket 0 holds degree 0, bucket b >= 1 the degrees 2^(b-1) .. 2^b - 1; agreement bucket a < bins the rows with
//   a / bins <= same / known < (a + 1) / bins (the last one closed at 1), bucket `bins` the rows without a labelled neighbour
//   (bounds -1, -1).  accuracy = correct / rows.
// Everything is float64 arithmetic on the integers; a negative count is an error; nothing is ever NaN.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

constexpr int STRUCTURE_MAX_CLASSES = 64, STRUCTURE_MAX_BINS = 32, STRUCTURE_DEGREE_BUCKETS = 32;

struct StructureMetrics {
    int num_classes = 0;
    double edge_homophily = 0, node_homophily = 0, adjusted_homophily = 0, class_insensitive_homophily = 0;
    int64_t edges = 0, rows_with_known = 0, labelled_rows = 0;
    std::vector<double> class_homophily;                       // [C]
    std::vector<double> compatibility;                         // [C x C]
};
struct StrataRow {
    double lo = 0, hi = 0;
    int64_t rows = 0, correct = 0;
    double accuracy = 0;
};
struct StrataTables {
    int bins = 0;
    int64_t rows = 0, correct = 0;
    std::vector<StrataRow> by_degree;                          // [32]
    std::vector<StrataRow> by_agreement;                       // [bins + 1]
};
// the integers of one report, as gcn-hip writes them and reads them back
struct StructureCounts {
    int num_classes = 0, bins = 0;
    int64_t totals_truth[8] = {}, totals_pred[8] = {};
    std::vector<int64_t> class_rows_truth, class_rows_pred;    // [C]
    std::vector<int64_t> mix_truth, mix_pred;                  // [C x C]
    std::vector<int64_t> strata;                               // [32 x (bins + 1) x 2]
};

// each: 0, or -1 with the reason in *err
int gcn_structure_metrics(int num_classes, const int64_t *mix, const int64_t *class_rows, const int64_t *totals, StructureMetrics *out, std::string *err);
int gcn_strata_tables(int bins, const int64_t *strata, StrataTables *out, std::string *err);
// The text report: a header line, the integers by name (totals, class rows, both mixing matrices, the strata cells) and, derived
// from them, one line of metrics per labelling and the two marginal tables; the derived lines start with '#', and the reader,
// which takes the integers alone, passes over them.
int gcn_structure_write(const char *path, const StructureCounts &c, std::string *err);
int gcn_structure_read(const char *path, StructureCounts *out, std::string *err);
