// structure_query.cpp — ModelQueries::neighbor_agreement / structure: the label structure of the model's graph, counted where the
// adjacency lies (queries.h has the contract, csrc/structure.hip the definitions and the kernels, host/structure.h the measures).
// Off the epoch path: no training module is touched; the one forward of structure() is predict()'s.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include "structure.h"
#include <algorithm>

int64_t ModelQueries::structure_rows(const char *what, int num_classes, int bins, bool predicted, int split, const int *nodes, int n) {
    const std::string w = std::string(what) + ": ";
    require(what, ONE_RANK | (predicted ? SINGLE_LABEL | CLASS_AGGREGATION : 0));
    if (num_classes < 1 || num_classes > STRUCTURE_MAX_CLASSES)
        throw GcnHipFailure(-1, w + "1 to 64 classes (the mixing counts of a workgroup sit in LDS), got " + std::to_string(num_classes));
    if (bins < 1 || bins > STRUCTURE_MAX_BINS) throw GcnHipFailure(-1, w + "bins must be in 1..32, got " + std::to_string(bins));
    if (split < 0 || split > 3) throw GcnHipFailure(-1, w + "invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    if (n < 0) throw GcnHipFailure(-1, w + "invalid argument");
    int listed = n;
    kmeans_list(what, split, nodes, listed);                   // a node id outside the graph is refused here
    return listed;
}

int64_t ModelQueries::agreement_launch(const int32_t *d_lab, int C, const int32_t *d_rows, int n, int32_t *d_per, const AgreementOut &out) {
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nn = (size_t)n, cc = (size_t)C * C;
    int64_t *d_counts = d_st_counts.need(cc + C + 8 + 1);
    int64_t *d_mix = d_counts, *d_class = d_counts + cc, *d_totals = d_class + C, *d_skipped = d_totals + 8;
    GCNHIP_CHECK(gcnhip_nbr_agreement(ctx, m.graph, d_lab, C, d_rows, n, d_per, d_per + nn, d_per + 2 * nn, out.mix ? d_mix : nullptr, d_class, d_totals,
                                      d_skipped));
    std::vector<int64_t> h(cc + C + 8 + 1);
    if (out.mix) GCNHIP_CHECK(gcnhip_d2h(ctx, h.data(), d_mix, cc * sizeof(int64_t)));
    GCNHIP_CHECK(gcnhip_d2h(ctx, h.data() + cc, d_class, ((size_t)C + 8 + 1) * sizeof(int64_t)));
    if (out.mix) std::copy(h.begin(), h.begin() + cc, out.mix);
    if (out.class_rows) std::copy(h.begin() + cc, h.begin() + cc + C, out.class_rows);
    if (out.totals) std::copy(h.begin() + cc + C, h.begin() + cc + C + 8, out.totals);
    if (n > 0) {
        if (out.deg) GCNHIP_CHECK(gcnhip_d2h(ctx, out.deg, d_per, nn * sizeof(int32_t)));
        if (out.same) GCNHIP_CHECK(gcnhip_d2h(ctx, out.same, d_per + nn, nn * sizeof(int32_t)));
        if (out.known) GCNHIP_CHECK(gcnhip_d2h(ctx, out.known, d_per + 2 * nn, nn * sizeof(int32_t)));
    }
    return h[cc + C + 8];
}

ModelQueries::Structure ModelQueries::neighbor_agreement(const int32_t *labels, int64_t n_labels, int num_classes, int split, const int *nodes, int n,
                                                         int32_t *deg, int32_t *same, int32_t *known, int64_t *mix, int64_t *class_rows, int64_t *totals) {
    const char *what = "neighbor_agreement";
    Structure res;
    res.rows = structure_rows(what, num_classes, 1, false, split, nodes, n);       // every refusal, before any launch
    if (!labels || n_labels != m.params.num_nodes)
        throw GcnHipFailure(-1, std::string(what) + ": " + std::to_string(labels ? n_labels : 0) + " labels for " + std::to_string(m.params.num_nodes) +
                                    " nodes (one label per node of the dataset)");
    const std::vector<int> rows = kmeans_list(what, split, nodes, n);
    std::vector<int32_t> local((size_t)std::max(m.n_local, 1), -1);
    for (int r = 0; r < m.n_local; r++) local[r] = labels[m.node_id(r)];
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    const size_t nn = (size_t)n;
    int32_t *d_rows = d_st_rows.need(nn), *d_lab = d_st_lab.need(local.size()), *d_per = d_st_per.need(3 * nn);
    if (n > 0) GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_rows, rows.data(), nn * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_h2d(m.env.ctx, d_lab, local.data(), local.size() * sizeof(int32_t)));
    res.skipped = agreement_launch(d_lab, num_classes, d_rows, n, d_per, AgreementOut{deg, same, known, mix, class_rows, totals});
    m.sync();
    return res;
}

ModelQueries::Structure ModelQueries::structure(int split, const int *nodes, int n, int bins, bool predicted, int32_t *deg, int32_t *same, int32_t *known,
                                                int64_t *mix_truth, int64_t *class_rows_truth, int64_t *totals_truth, int64_t *mix_pred,
                                                int64_t *class_rows_pred, int64_t *totals_pred, int64_t *strata) {
    const char *what = "structure";
    const int C = m.params.output_dim;
    Structure res;
    res.rows = structure_rows(what, C, bins, predicted, split, nodes, n);           // every refusal, before any launch
    if (m.data->label.size() < (size_t)(m.row_start() + m.n_local))
        throw GcnHipFailure(-1, std::string(what) + ": the dataset holds no label per node");
    const std::vector<int> rows = kmeans_list(what, split, nodes, n);
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nn = (size_t)n;
    int32_t *d_rows = d_st_rows.need(nn), *d_per = d_st_per.need(3 * nn);
    if (n > 0) GCNHIP_CHECK(gcnhip_h2d(ctx, d_rows, rows.data(), nn * sizeof(int32_t)));
    if (!d_label_all) d_label_all = arena.upload(m.data->label.data() + m.row_start(), (size_t)m.n_local);
    res.skipped = agreement_launch(d_label_all, C, d_rows, n, d_per, AgreementOut{deg, same, known, mix_truth, class_rows_truth, totals_truth});
    if (predicted) {
        forward_predict(nullptr, false);                       // d_pred of every local row; the logits are not stored
        int32_t *d_per2 = d_st_per2.need(3 * nn);
        agreement_launch(d_pred.p, C, d_rows, n, d_per2, AgreementOut{nullptr, nullptr, nullptr, mix_pred, class_rows_pred, totals_pred});
        const size_t cells = (size_t)STRUCTURE_DEGREE_BUCKETS * (bins + 1) * 2;
        int64_t *d_strata = d_st_strata.need(cells + 1);
        GCNHIP_CHECK(gcnhip_strata_counts(ctx, d_per, d_per + nn, d_per + 2 * nn, d_pred.p, d_label_all, m.n_local, d_rows, n, C, bins, d_strata,
                                          d_strata + cells));
        std::vector<int64_t> h(cells + 1);
        GCNHIP_CHECK(gcnhip_d2h(ctx, h.data(), d_strata, h.size() * sizeof(int64_t)));
        if (strata) std::copy(h.begin(), h.begin() + cells, strata);
        res.unlabelled = h[cells];
    }
    m.sync();
    return res;
}
