// silhouette_query.cpp — ModelQueries::silhouette: the silhouette widths of a labelling of the hidden layer of a trained model,
// where it lies (queries.h has the contract, csrc/silhouette.hip the definitions and the kernels).  Off the epoch path: the hidden
// layer comes from embed_forward and no training module is touched.
#include "queries.h"
#include "gcn.h"
#include "hip_check.h"
#include <algorithm>

int64_t ModelQueries::silhouette_rows(int k, int split, const int *nodes, int n, const int32_t *labels, int64_t n_labels, std::vector<int> *rows) {
    const char *what = "silhouette";
    const std::string w = std::string(what) + ": ";
    require(what, ONE_RANK);
    if (m.flags & HIPGCN_BF16_TABLES) throw GcnHipFailure(-1, w + "not with bf16 tables (the kernels read the f32 rows of the hidden layer)");
    if (m.params.hidden_dim < 1 || m.params.hidden_dim > 256)
        throw GcnHipFailure(-1, w + "a hidden width of at most 256 (the sums keep a tile of rows and one of members in LDS)");
    if (split < 0 || split > 3) throw GcnHipFailure(-1, w + "invalid argument (split is 0 with a node query, or 1 train, 2 validation, 3 test)");
    if (n < 0 || n_labels < 0) throw GcnHipFailure(-1, w + "invalid argument");
    if (k < 1 || k > 256) throw GcnHipFailure(-1, w + "k must be in 1..256, got " + std::to_string(k));
    int listed = n;
    std::vector<int> list = kmeans_list(what, split, nodes, listed);   // a node id outside the graph is refused here
    if (n_labels != listed)
        throw GcnHipFailure(-1, w + "the query lists " + std::to_string(listed) + " rows, the labels are " + std::to_string(n_labels));
    if (listed > 0 && !labels) throw GcnHipFailure(-1, w + "invalid argument (the labels are missing)");
    if (rows) *rows = std::move(list);
    return listed;
}

ModelQueries::Silhouette ModelQueries::silhouette(int split, const int *nodes, int n, const int32_t *labels, int64_t n_labels, int k, bool normalize,
                                                  size_t scratch_bytes, double *s, double *a, double *b, int32_t *neighbor, double *cluster_mean,
                                                  int32_t *sizes) {
    Silhouette res;
    std::vector<int> rows;
    res.rows = silhouette_rows(k, split, nodes, n, labels, n_labels, &rows);   // every refusal, before any launch; the list is made once
    n = (int)rows.size();
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    const EmbedTable t = embed_forward(normalize);
    gcnhip_ctx *ctx = m.env.ctx;
    const size_t nn = (size_t)n, kk = (size_t)k;
    size_t full = 0, least = 0;
    if (gcnhip_silhouette_plan(n, k, t.dim, &full, &least) != 0) throw GcnHipFailure(-1, std::string("silhouette: ") + gcnhip_last_error());
    const size_t bytes = std::max(std::min(full, scratch_bytes ? scratch_bytes : SILHOUETTE_SCRATCH_DEFAULT), least);
    unsigned char *d_scr = d_sil_scratch.need(bytes);
    int32_t *d_rows = d_sil_int.need(3 * nn + kk + 3), *d_lab = d_rows + nn, *d_nb = d_lab + nn, *d_sizes = d_nb + nn, *d_counts = d_sizes + kk;
    double *d_sums = d_sil_sums.need(nn * kk);
    double *d_s = d_sil_out.need(3 * nn + kk + 1), *d_a = d_s + nn, *d_b = d_a + nn, *d_csum = d_b + nn, *d_total = d_csum + kk;
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_rows, rows.data(), nn * sizeof(int32_t)));
    if (n > 0) GCNHIP_CHECK(gcnhip_h2d(ctx, d_lab, labels, nn * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_silhouette_sums(ctx, t.data, t.ld, t.rows, t.dim, t.inv_norm, d_rows, n, d_lab, k, d_sums, d_sizes, d_scr, bytes));
    GCNHIP_CHECK(gcnhip_silhouette_rows(ctx, d_sums, d_lab, d_sizes, d_rows, t.rows, n, k, d_s, d_a, d_b, d_nb, d_csum, d_total, d_counts));
    std::vector<int32_t> small(kk + 3);                        // {sizes | counts}
    std::vector<double> tot(kk + 1);                           // {cluster_sum | total}
    GCNHIP_CHECK(gcnhip_d2h(ctx, small.data(), d_sizes, small.size() * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_d2h(ctx, tot.data(), d_csum, tot.size() * sizeof(double)));
    if (n > 0) {
        if (s) GCNHIP_CHECK(gcnhip_d2h(ctx, s, d_s, nn * sizeof(double)));
        if (a) GCNHIP_CHECK(gcnhip_d2h(ctx, a, d_a, nn * sizeof(double)));
        if (b) GCNHIP_CHECK(gcnhip_d2h(ctx, b, d_b, nn * sizeof(double)));
        if (neighbor) GCNHIP_CHECK(gcnhip_d2h(ctx, neighbor, d_nb, nn * sizeof(int32_t)));
    }
    m.sync();
    res.points = small[kk];
    res.excluded = small[kk + 1];
    res.nonempty = small[kk + 2];
    res.defined = res.nonempty >= 2;
    res.score = res.points > 0 ? tot[kk] / (double)res.points : 0.0;
    for (int c = 0; c < k; c++) {
        if (sizes) sizes[c] = small[c];
        if (cluster_mean) cluster_mean[c] = small[c] > 0 ? tot[c] / (double)small[c] : 0.0;
    }
    return res;
}
