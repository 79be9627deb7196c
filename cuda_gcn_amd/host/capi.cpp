// capi.cpp — extern "C" surface of the host library (include/gcnhost.h).
#include "gcnhost.h"
#include <algorithm>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>
#include "gcn.h"
#include "queries.h"
#include "attach.h"
#include "cluster.h"
#include "hip_check.h"
#include "parser.h"
#include "class_weights.h"
#include "labels.h"
#include "report.h"
#include "calibration.h"
#include "kmeans.h"
#include "pca.h"
#include "structure.h"
#include "reach.h"
#include "conformal.h"
#include "ranking.h"
#include "thresholds.h"
#include "weights.h"

static thread_local std::string g_err;

struct gcnhost_model {
    GCNData data;
    HipGCN *gcn = nullptr;
};
struct gcnhost_dataset {
    GCNData data;
};

#define API_TRY(...)                                    \
    try {                                               \
        __VA_ARGS__;                                    \
        return 0;                                       \
    } catch (const GcnHipFailure &e) {                  \
        g_err = e.what();                               \
        return e.code ? e.code : -1;                    \
    } catch (const std::exception &e) {                 \
        g_err = e.what();                               \
        return -1;                                      \
    }

extern "C" {

const char *gcnhost_last_error(void) { return g_err.c_str(); }

gcnhost_params gcnhost_params_default(void) {
    GCNParams d = GCNParams::get_default();
    gcnhost_params p;
    memcpy(&p, &d, sizeof p);
    return p;
}

int gcnhost_nccl_unique_id(char id[GCNHOST_NCCL_ID_BYTES]) { return rccl_get_unique_id(id); }

static int model_create(gcnhost_model **out, const gcnhost_params *p,
                        const int *g_indptr, const int *g_indices,
                        const int *f_indptr, const int *f_indices, const float *f_val,
                        const int *split, const int *label, const uint32_t *multihot,
                        long seed, int device, int flags, int rank, int world, const char *nccl_id,
                        gcnhost_allgather_fn host_ag, gcnhost_allreduce_fn host_ar, void *host_user,
                        const float *class_weights = nullptr) {
    API_TRY({
        gcnhost_model *m = new gcnhost_model();
        const int N = p->num_nodes;
        m->data.graph.indptr.assign(g_indptr, g_indptr + N + 1);
        m->data.graph.indices.assign(g_indices, g_indices + g_indptr[N]);
        m->data.feature_index.indptr.assign(f_indptr, f_indptr + N + 1);
        if (f_indices) m->data.feature_index.indices.assign(f_indices, f_indices + f_indptr[N]);
        m->data.feature_value.assign(f_val, f_val + f_indptr[N]);
        m->data.split.assign(split, split + N);
        if (label) m->data.label.assign(label, label + N);
        else m->data.label.assign(N, -1);
        if (multihot) m->data.multihot.assign(multihot, multihot + (size_t)N * ((p->output_dim + 31) / 32));
        GCNParams gp;
        static_assert(sizeof(GCNParams) == sizeof(gcnhost_params), "params layout");
        memcpy(&gp, p, sizeof gp);
        HipGCNOptions o;
        o.device = device; o.seed = seed; o.flags = flags; o.rank = rank; o.world = world; o.nccl_id = nccl_id;
        o.host_allgather = host_ag; o.host_allreduce = host_ar; o.host_user = host_user;
        o = HipGCNOptions::from_environment(o);                 // every HIPGCN_* variable, read once (host/options.cpp)
        o.multilabel = multihot != nullptr;
        if (class_weights) o.class_weights.assign(class_weights, class_weights + std::max(p->output_dim, 0));
        try {
            m->gcn = new HipGCN(gp, &m->data, o);
        } catch (...) {
            delete m;
            throw;
        }
        *out = m;
    })
}

int gcnhost_model_create(gcnhost_model **out, const gcnhost_params *p,
                         const int *g_indptr, const int *g_indices,
                         const int *f_indptr, const int *f_indices, const float *f_val,
                         const int *split, const int *label,
                         long seed, int device, int flags, int rank, int world, const char *nccl_id,
                         gcnhost_allgather_fn host_ag, gcnhost_allreduce_fn host_ar, void *host_user) {
    if (!out || !p || !g_indptr || !g_indices || !f_indptr || !f_val || !split || !label) { g_err = "null argument"; return -1; }
    return model_create(out, p, g_indptr, g_indices, f_indptr, f_indices, f_val, split, label, nullptr, seed, device, flags, rank, world,
                        nccl_id, host_ag, host_ar, host_user);
}

int gcnhost_model_create_multilabel(gcnhost_model **out, const gcnhost_params *p,
                                    const int *g_indptr, const int *g_indices,
                                    const int *f_indptr, const int *f_indices, const float *f_val,
                                    const int *split, const int *label, const uint32_t *multihot,
                                    long seed, int device, int flags, int rank, int world, const char *nccl_id,
                                    gcnhost_allgather_fn host_ag, gcnhost_allreduce_fn host_ar, void *host_user) {
    if (!out || !p || !g_indptr || !g_indices || !f_indptr || !f_val || !split || !multihot) { g_err = "null argument"; return -1; }
    if (p->output_dim < 1 || p->output_dim > 256) { g_err = "multi-label mode takes 1 to 256 classes"; return -1; }
    return model_create(out, p, g_indptr, g_indices, f_indptr, f_indices, f_val, split, label, multihot, seed, device, flags, rank, world,
                        nccl_id, host_ag, host_ar, host_user);
}

int gcnhost_model_create_weighted(gcnhost_model **out, const gcnhost_params *p,
                                  const int *g_indptr, const int *g_indices,
                                  const int *f_indptr, const int *f_indices, const float *f_val,
                                  const int *split, const int *label, const uint32_t *multihot, const float *class_weights,
                                  long seed, int device, int flags, int rank, int world, const char *nccl_id,
                                  gcnhost_allgather_fn host_ag, gcnhost_allreduce_fn host_ar, void *host_user) {
    if (!out || !p || !g_indptr || !g_indices || !f_indptr || !f_val || !split || (!multihot && !label)) { g_err = "null argument"; return -1; }
    if (multihot && (p->output_dim < 1 || p->output_dim > 256)) { g_err = "multi-label mode takes 1 to 256 classes"; return -1; }
    if (class_weights && (p->output_dim < 1 || p->output_dim > 256)) { g_err = "class weights take 1 to 256 classes"; return -1; }
    return model_create(out, p, g_indptr, g_indices, f_indptr, f_indices, f_val, split, label, multihot, seed, device, flags, rank, world,
                        nccl_id, host_ag, host_ar, host_user, class_weights);
}

int gcnhost_balanced_class_weights(int num_nodes, int num_classes, const int *split, const int *label, const uint32_t *multihot,
                                   int which_split, float *weights) {
    return gcn_balanced_class_weights(num_nodes, num_classes, split, label, multihot, which_split, weights, &g_err);
}
int gcnhost_class_weights_read(const char *path, int *num_classes, float *weights) {
    if (!path || !num_classes) { g_err = "gcnhost_class_weights_read: invalid argument"; return -1; }
    std::vector<float> w;
    if (gcn_class_weights_read(path, *num_classes, w, &g_err) != 0) return -1;
    *num_classes = (int)w.size();
    if (weights) memcpy(weights, w.data(), w.size() * sizeof(float));
    return 0;
}

int gcnhost_model_destroy(gcnhost_model *m) {
    if (!m) return 0;
    API_TRY({ delete m->gcn; delete m; })
}
int gcnhost_model_train_epoch(gcnhost_model *m, float *loss, float *acc) {
    API_TRY({ auto r = m->gcn->train_epoch(); *loss = r.first; *acc = r.second; })
}
int gcnhost_model_eval(gcnhost_model *m, int split, float *loss, float *acc) {
    API_TRY({ auto r = m->gcn->eval(split); *loss = r.first; *acc = r.second; })
}
int gcnhost_model_run_epochs(gcnhost_model *m, int n, float *trace) { API_TRY({ m->gcn->run_epochs(n, trace); }) }
int gcnhost_model_run(gcnhost_model *m) { API_TRY({ m->gcn->run(); }) }
int gcnhost_model_sync(gcnhost_model *m) { API_TRY({ m->gcn->sync(); }) }

int gcnhost_model_exchange(gcnhost_model *m, int *halo, int64_t *recv_rows, int64_t *send_rows, int *table_rows, double *halo_share) {
    API_TRY({
        const ExchangePlan &x = m->gcn->exchange_plan();
        if (halo) *halo = x.halo ? 1 : 0;
        if (recv_rows) *recv_rows = x.world > 1 ? x.recv_total() : 0;
        if (send_rows) *send_rows = x.world > 1 ? x.send_total() : 0;
        if (table_rows) *table_rows = x.table_rows;
        if (halo_share) *halo_share = x.halo_share;
    })
}
int gcnhost_model_info(gcnhost_model *m, int *rank, int *world, int *row_start, int *local_rows, int64_t *local_edges) {
    API_TRY({
        if (rank) *rank = m->gcn->rank();
        if (world) *world = m->gcn->world();
        if (row_start) *row_start = m->gcn->row_start();
        if (local_rows) *local_rows = m->gcn->local_rows();
        if (local_edges) *local_edges = m->gcn->n_edges_local();
    })
}
int gcnhost_model_row_ids(gcnhost_model *m, int *ids, int *renumbered) {
    API_TRY({
        if (renumbered) *renumbered = !m->gcn->node_order().empty();
        if (ids)
            for (int r = 0; r < m->gcn->local_rows(); r++) ids[r] = m->gcn->node_id(r);
    })
}
int gcnhost_model_row_scale(gcnhost_model *m, float *dinv, int *factored) {
    API_TRY({
        if (factored) *factored = m->gcn->factored() ? 1 : 0;
        if (dinv) {
            std::vector<float> v;
            m->gcn->row_scale(v);
            if (!v.empty()) memcpy(dinv, v.data(), v.size() * sizeof(float));
        }
    })
}
int gcnhost_model_schedule(gcnhost_model *m, int *mode, int *n_groups) {
    API_TRY({
        if (mode) *mode = m->gcn->schedule_mode();
        if (n_groups) *n_groups = m->gcn->schedule_groups();
    })
}
int gcnhost_model_transport(gcnhost_model *m, int *ranks, char name[32]) {
    API_TRY({
        if (ranks) *ranks = m->gcn->transport_ranks();
        if (name) { strncpy(name, m->gcn->transport(), 31); name[31] = 0; }
    })
}
int gcnhost_model_slice_floats(gcnhost_model *m, int *floats) {
    API_TRY({ if (floats) *floats = m->gcn->schedule_slice_floats(); })
}
int gcnhost_model_get_var(gcnhost_model *m, int k, int grad, float *out, int *rows, int *cols) {
    API_TRY({
        std::vector<float> v;
        int r, c;
        m->gcn->get_var(k, grad != 0, v, &r, &c);
        if (rows) *rows = r;
        if (cols) *cols = c;
        if (out) memcpy(out, v.data(), v.size() * sizeof(float));
    })
}
int gcnhost_model_set_weights(gcnhost_model *m, const float *w1, const float *w2) { API_TRY({ m->gcn->set_weights(w1, w2); }) }
int gcnhost_model_predict(gcnhost_model *m, const int *nodes, int n, int32_t *pred, float *prob, float *logp) {
    API_TRY({ m->gcn->queries().predict(nodes, n, pred, prob, logp); })
}
int gcnhost_model_predict_multilabel(gcnhost_model *m, const int *nodes, int n, uint32_t *bits, float *prob) {
    API_TRY({ m->gcn->queries().predict_multilabel(nodes, n, bits, prob); })
}
int gcnhost_attach_rows(int num_nodes, const int *g_indptr, int n_new, const int64_t *nbr_ptr, const int *nbr_ids, int mode, int32_t *out_ptr,
                        int32_t *out_col, float *out_coef, int32_t *out_len) {
    if (num_nodes < 0 || !g_indptr || !nbr_ptr || !out_ptr) { g_err = "new_node_rows: invalid argument"; return -1; }
    std::vector<int> len((size_t)num_nodes);
    for (int r = 0; r < num_nodes; r++) len[r] = g_indptr[r + 1] - g_indptr[r];
    AttachRows rows;
    if (gcn_attach_rows(num_nodes, len.data(), nullptr, n_new, nbr_ptr, nbr_ids, mode, &rows, &g_err) != 0) return -1;
    std::copy(rows.ptr.begin(), rows.ptr.end(), out_ptr);
    if (out_col) std::copy(rows.col.begin(), rows.col.end(), out_col);
    if (out_coef) std::copy(rows.coef.begin(), rows.coef.end(), out_coef);
    if (out_len) std::copy(rows.len.begin(), rows.len.end(), out_len);
    return 0;
}
int gcnhost_model_predict_new(gcnhost_model *m, const int *x_indptr, const int *x_indices, const float *x_values, int n_new, const int64_t *nbr_ptr,
                              const int *nbr_ids, const float *thr, int n_thr, int32_t *pred, float *prob, float *logp, uint32_t *bits) {
    if (!m) { g_err = "gcnhost_model_predict_new: invalid argument"; return -1; }
    API_TRY({ m->gcn->queries().predict_new(x_indptr, x_indices, x_values, n_new, nbr_ptr, nbr_ids, thr, n_thr, pred, prob, logp, bits); })
}
int gcnhost_model_mc_dropout(gcnhost_model *m, int split, const int *nodes, int n, int samples, const float *p, const uint64_t *seed, uint64_t first_sample,
                             int64_t capacity, int32_t *pred, float *confidence, float *entropy, float *expected_entropy, float *mutual_information,
                             float *variation_ratio, float *mean_prob, int32_t *votes, float *samples_logp, uint64_t *seed_used, float *p_used,
                             int64_t *rows) {
    if (!m) { g_err = "gcnhost_model_mc_dropout: invalid argument"; return -1; }
    API_TRY({
        ModelQueries &q = m->gcn->queries();
        const int64_t listed = q.mc_dropout_rows(split, nodes, n, samples, p, first_sample);
        if (rows) *rows = listed;
        const bool any = pred || confidence || entropy || expected_entropy || mutual_information || variation_ratio || mean_prob || votes || samples_logp;
        if (!any) return 0;                                    // the arguments are fine and *rows is known: a caller sizes its arrays
        if (listed != capacity && !(listed == 0 && capacity >= 0))
            throw GcnHipFailure(-1, "mc_dropout: the query lists " + std::to_string(listed) + " rows, the arrays are laid out for " + std::to_string(capacity));
        const ModelQueries::McDropout r = q.mc_dropout(split, nodes, n, samples, p, seed, first_sample, pred, confidence, entropy, expected_entropy,
                                                       mutual_information, variation_ratio, mean_prob, votes, samples_logp);
        if (seed_used) *seed_used = r.seed;
        if (p_used) *p_used = r.p;
    })
}
int gcnhost_model_evaluate(gcnhost_model *m, int split, const int *nodes, int n, int64_t *counts, int64_t *rows_counted, int64_t *unlabelled) {
    if (!m || !counts) { g_err = "gcnhost_model_evaluate: invalid argument"; return -1; }
    API_TRY({ m->gcn->queries().evaluate(split, nodes, n, counts, rows_counted, unlabelled); })
}
int gcnhost_model_propagate(gcnhost_model *m, const float *y0, int dim, float alpha, int iters, float lo, float hi, float *out, int32_t *pred) {
    if (!m || !y0 || !out) { g_err = "gcnhost_model_propagate: invalid argument"; return -1; }
    API_TRY({ m->gcn->queries().propagate(y0, dim, alpha, iters, lo, hi, out, pred); })
}
int gcnhost_model_label_propagation(gcnhost_model *m, float alpha, int iters, int splits_mask, int32_t *pred, float *y) {
    if (!m || !pred) { g_err = "gcnhost_model_label_propagation: invalid argument"; return -1; }
    API_TRY({ m->gcn->queries().label_propagation(alpha, iters, splits_mask, pred, y); })
}
int gcnhost_model_correct_and_smooth(gcnhost_model *m, float alpha_correct, int iters_correct, float alpha_smooth, int iters_smooth,
                                     int splits_mask, int32_t *pred, float *g) {
    if (!m || !pred) { g_err = "gcnhost_model_correct_and_smooth: invalid argument"; return -1; }
    API_TRY({ m->gcn->queries().correct_and_smooth(alpha_correct, iters_correct, alpha_smooth, iters_smooth, splits_mask, pred, g); })
}
int gcnhost_model_calibration(gcnhost_model *m, int split, const int *nodes, int n, float temperature, int bins, double *sums, int64_t *count,
                              int64_t *correct, double *conf_sum) {
    if (!m || !sums || !count || !correct || !conf_sum) { g_err = "gcnhost_model_calibration: invalid argument"; return -1; }
    API_TRY({ m->gcn->queries().calibration(split, nodes, n, temperature, bins, sums, count, correct, conf_sum); })
}
int gcnhost_model_calibrate(gcnhost_model *m, int split, int bins, double *out, int64_t *count, int64_t *correct, double *conf_sum) {
    if (!m || !out) { g_err = "gcnhost_model_calibrate: invalid argument"; return -1; }
    API_TRY({
        const ModelQueries::Calibrated c = m->gcn->queries().calibrate(split, bins, count, correct, conf_sum);
        out[0] = c.temperature; out[1] = c.nll_before; out[2] = c.nll_after; out[3] = c.steps; out[4] = c.at_bound ? 1.0 : 0.0;
        out[5] = (double)c.rows;
    })
}
int gcnhost_model_set_temperature(gcnhost_model *m, float temperature) {
    if (!m) { g_err = "gcnhost_model_set_temperature: invalid argument"; return -1; }
    API_TRY({ m->gcn->queries().set_temperature(temperature); })
}
int gcnhost_model_temperature(gcnhost_model *m, float *temperature) {
    if (!m || !temperature) { g_err = "gcnhost_model_temperature: invalid argument"; return -1; }
    API_TRY({ *temperature = m->gcn->queries().temperature(); })
}
int gcnhost_model_embed(gcnhost_model *m, const int *nodes, int n, float *out, int normalize) {
    if (!m) { g_err = "gcnhost_model_embed: invalid argument"; return -1; }
    API_TRY({ m->gcn->queries().embed(nodes, n, out, normalize != 0); })
}
int gcnhost_model_similar(gcnhost_model *m, const int *nodes, int n, int k, int metric, int exclude_self, int32_t *out_id, float *out_score) {
    if (!m) { g_err = "gcnhost_model_similar: invalid argument"; return -1; }
    API_TRY({ m->gcn->queries().similar(nodes, n, k, metric, exclude_self != 0, out_id, out_score); })
}
int gcnhost_model_score_pairs(gcnhost_model *m, const int *src, const int *dst, int n_pairs, int metric, float *out) {
    if (!m) { g_err = "gcnhost_model_score_pairs: invalid argument"; return -1; }
    API_TRY({ m->gcn->queries().score_pairs(src, dst, n_pairs, metric, out); })
}
int gcnhost_model_explain(gcnhost_model *m, const int *nodes, const int *classes, int n, size_t feat_scratch_bytes, int32_t *out_class, float *logit,
                          float *hidden, float *feat, int64_t *nbr_ptr, int32_t *nbr_ids, float *nbr_values, int64_t *nbr_total) {
    if (!m) { g_err = "gcnhost_model_explain: invalid argument"; return -1; }
    API_TRY({
        if (!nbr_ids) {                                        // the first call: the length of the neighbour lists
            if (!nbr_total) throw GcnHipFailure(-1, "explain: invalid argument");
            *nbr_total = m->gcn->queries().explain_size(nodes, n);
        } else {
            m->gcn->queries().explain(nodes, classes, n, feat_scratch_bytes, out_class, logit, hidden, feat, nbr_ptr, nbr_ids, nbr_values);
            if (nbr_total && nbr_ptr) *nbr_total = nbr_ptr[nodes ? n : m->gcn->params.num_nodes];
        }
    })
}
int gcnhost_model_feature_importance(gcnhost_model *m, int split, const int *nodes, int n, size_t feat_scratch_bytes, double *mean_abs, int64_t *count) {
    if (!m) { g_err = "gcnhost_model_feature_importance: invalid argument"; return -1; }
    API_TRY({ m->gcn->queries().feature_importance(split, nodes, n, feat_scratch_bytes, mean_abs, count); })
}
int gcnhost_model_kmeans(gcnhost_model *m, int k, int split, const int *nodes, int n, int iters, int normalize, int init, const int *init_pos,
                         const float *init_centers, const uint64_t *seed, size_t scratch_bytes, int64_t capacity, int32_t *assign, float *dist2,
                         float *centers, int32_t *sizes, int32_t *seed_pos, double *history, int64_t *contingency, int64_t *info, double *inertia,
                         uint64_t *seed_used) {
    if (!m) { g_err = "gcnhost_model_kmeans: invalid argument"; return -1; }
    API_TRY({
        ModelQueries &q = m->gcn->queries();
        const int64_t listed = q.kmeans_rows(k, split, nodes, n, iters, init, init_pos, init_centers);
        if ((assign || dist2) && listed > capacity)
            throw GcnHipFailure(-1, "kmeans: the query lists " + std::to_string(listed) + " rows, the arrays are laid out for " + std::to_string(capacity));
        const ModelQueries::KMeans r = q.kmeans(k, split, nodes, n, iters, normalize != 0, init, init_pos, init_centers, seed, scratch_bytes, assign, dist2,
                                                centers, sizes, seed_pos, history, contingency);
        if (info) { info[0] = r.rows; info[1] = r.iters_run; info[2] = r.converged ? 1 : 0; info[3] = r.skipped; }
        if (inertia) *inertia = r.inertia;
        if (seed_used) *seed_used = r.seed;
    })
}
int gcnhost_cluster_report(int k, int num_classes, const int64_t *counts, double *summary) {
    ClusterReport r;
    if (gcn_cluster_report(k, num_classes, counts, &r, &g_err) != 0) return -1;
    if (summary) {
        const double v[9] = {r.purity, r.homogeneity, r.completeness, r.v_measure, r.nmi, r.ari, r.entropy_classes, r.entropy_clusters, (double)r.rows};
        std::copy(v, v + 9, summary);
    }
    return 0;
}
int gcnhost_model_silhouette(gcnhost_model *m, int split, const int *nodes, int n, const int32_t *labels, int k, int normalize, size_t scratch_bytes,
                             int64_t capacity, double *s, double *a, double *b, int32_t *neighbor, double *cluster_mean, int32_t *sizes,
                             int64_t *info, double *score) {
    if (!m) { g_err = "gcnhost_model_silhouette: invalid argument"; return -1; }
    API_TRY({
        const ModelQueries::Silhouette r =
            m->gcn->queries().silhouette(split, nodes, n, labels, capacity, k, normalize != 0, scratch_bytes, s, a, b, neighbor, cluster_mean, sizes);
        if (info) { info[0] = r.rows; info[1] = r.points; info[2] = r.excluded; info[3] = r.nonempty; info[4] = r.defined ? 1 : 0; }
        if (score) *score = r.score;
    })
}
int gcnhost_sym_eigen(const double *S, int h, double *lambda, double *V) { return gcn_sym_eigen(S, h, lambda, V, &g_err); }
int gcnhost_pca_from_scatter(const double *S, const double *mean, int64_t rows, int h, int k, int whiten, double *eigenvalues, double *components,
                             double *explained, double *scale, int *rank) {
    PcaFit f;
    if (gcn_pca_from_scatter(S, mean, rows, h, k, whiten != 0, &f, &g_err) != 0) return -1;
    const size_t n = (size_t)h;
    if (eigenvalues) std::copy(f.eigenvalues.begin(), f.eigenvalues.end(), eigenvalues);
    if (components)
        for (size_t j = 0; j < n; j++)
            for (size_t a = 0; a < n; a++) components[j * n + a] = f.components[a * n + j];
    if (explained) {
        std::copy(f.explained_variance.begin(), f.explained_variance.end(), explained);
        std::copy(f.explained_variance_ratio.begin(), f.explained_variance_ratio.end(), explained + n);
        std::copy(f.singular_values.begin(), f.singular_values.end(), explained + 2 * n);
    }
    if (scale && whiten) std::copy(f.scale.begin(), f.scale.end(), scale);
    if (rank) *rank = f.rank;
    return 0;
}
int gcnhost_model_pca_fit(gcnhost_model *m, int k, int split, const int *nodes, int n, int normalize, int center, int whiten, size_t scratch_bytes,
                          int64_t capacity, double *mean, double *scatter, double *eigenvalues, double *components, double *explained, double *scale,
                          float *coords, int64_t *info) {
    if (!m) { g_err = "gcnhost_model_pca_fit: invalid argument"; return -1; }
    API_TRY({
        ModelQueries &q = m->gcn->queries();
        const int64_t listed = q.pca_rows(k, split, nodes, n);
        if (coords && listed > capacity)
            throw GcnHipFailure(-1, "pca: the query lists " + std::to_string(listed) + " rows, the arrays are laid out for " + std::to_string(capacity));
        const ModelQueries::Pca r = q.pca_fit(k, split, nodes, n, normalize != 0, center != 0, whiten != 0, scratch_bytes, mean, scatter, eigenvalues,
                                              components, explained, scale, coords);
        if (info) { info[0] = r.rows; info[1] = r.rank; info[2] = r.k; }
    })
}
int gcnhost_model_pca_project(gcnhost_model *m, int width, int k, const double *mean, const double *components, const double *scale, int normalize,
                              const int *nodes, int n, float *out) {
    if (!m) { g_err = "gcnhost_model_pca_project: invalid argument"; return -1; }
    API_TRY({ m->gcn->queries().pca_project(width, k, mean, components, scale, normalize != 0, nodes, n, out); })
}
int gcnhost_model_neighbor_agreement(gcnhost_model *m, const int32_t *labels, int64_t n_labels, int num_classes, int split, const int *nodes, int n,
                                     int64_t capacity, int32_t *deg, int32_t *same, int32_t *known, int64_t *mix, int64_t *class_rows, int64_t *totals,
                                     int64_t *info) {
    if (!m) { g_err = "gcnhost_model_neighbor_agreement: invalid argument"; return -1; }
    API_TRY({
        ModelQueries &q = m->gcn->queries();
        const int64_t listed = q.structure_rows("neighbor_agreement", num_classes, 1, false, split, nodes, n);
        if ((deg || same || known) && listed > capacity)
            throw GcnHipFailure(-1, "neighbor_agreement: the query lists " + std::to_string(listed) + " rows, the arrays are laid out for " + std::to_string(capacity));
        const ModelQueries::Structure r = q.neighbor_agreement(labels, n_labels, num_classes, split, nodes, n, deg, same, known, mix, class_rows, totals);
        if (info) { info[0] = r.rows; info[1] = r.skipped; }
    })
}
int gcnhost_model_structure(gcnhost_model *m, int split, const int *nodes, int n, int bins, int predicted, int64_t capacity, int32_t *deg, int32_t *same,
                            int32_t *known, int64_t *mix_truth, int64_t *class_rows_truth, int64_t *totals_truth, int64_t *mix_pred,
                            int64_t *class_rows_pred, int64_t *totals_pred, int64_t *strata, int64_t *info) {
    if (!m) { g_err = "gcnhost_model_structure: invalid argument"; return -1; }
    API_TRY({
        ModelQueries &q = m->gcn->queries();
        const int64_t listed = q.structure_rows("structure", m->gcn->params.output_dim, bins, predicted != 0, split, nodes, n);
        if ((deg || same || known) && listed > capacity)
            throw GcnHipFailure(-1, "structure: the query lists " + std::to_string(listed) + " rows, the arrays are laid out for " + std::to_string(capacity));
        const ModelQueries::Structure r = q.structure(split, nodes, n, bins, predicted != 0, deg, same, known, mix_truth, class_rows_truth, totals_truth,
                                                      mix_pred, class_rows_pred, totals_pred, strata);
        if (info) { info[0] = r.rows; info[1] = r.skipped; info[2] = r.unlabelled; }
    })
}
int gcnhost_structure_metrics(int num_classes, const int64_t *mix, const int64_t *class_rows, const int64_t *totals, int bins, const int64_t *strata,
                              double *summary, double *class_homophily, double *compatibility, double *by_degree, double *by_agreement) {
    StructureMetrics r;
    StrataTables t;
    if (gcn_structure_metrics(num_classes, mix, class_rows, totals, &r, &g_err) != 0) return -1;
    if (strata && gcn_strata_tables(bins, strata, &t, &g_err) != 0) return -1;
    if (summary) {
        const double v[8] = {r.edge_homophily, r.node_homophily, r.adjusted_homophily, r.class_insensitive_homophily,
                             (double)r.edges, (double)r.rows_with_known, (double)r.labelled_rows, (double)t.rows};
        std::copy(v, v + 8, summary);
    }
    if (class_homophily) std::copy(r.class_homophily.begin(), r.class_homophily.end(), class_homophily);
    if (compatibility) std::copy(r.compatibility.begin(), r.compatibility.end(), compatibility);
    auto rows_out = [](const std::vector<StrataRow> &rows, double *out) {
        for (size_t b = 0; out && b < rows.size(); b++) {
            const double v[5] = {rows[b].lo, rows[b].hi, (double)rows[b].rows, (double)rows[b].correct, rows[b].accuracy};
            std::copy(v, v + 5, out + 5 * b);
        }
    };
    if (strata) { rows_out(t.by_degree, by_degree); rows_out(t.by_agreement, by_agreement); }
    return 0;
}
int gcnhost_structure_write(const char *path, int num_classes, int bins, const int64_t *totals_truth, const int64_t *totals_pred,
                            const int64_t *class_rows_truth, const int64_t *class_rows_pred, const int64_t *mix_truth, const int64_t *mix_pred,
                            const int64_t *strata) {
    if (!path || !totals_truth || !totals_pred || !class_rows_truth || !class_rows_pred || !mix_truth || !mix_pred || !strata || num_classes < 1 ||
        num_classes > STRUCTURE_MAX_CLASSES || bins < 1 || bins > STRUCTURE_MAX_BINS) {
        g_err = "structure_write: invalid argument (1..64 classes, 1..32 bins, every table)";
        return -1;
    }
    StructureCounts c;
    const size_t C = (size_t)num_classes, cells = (size_t)STRUCTURE_DEGREE_BUCKETS * (bins + 1) * 2;
    c.num_classes = num_classes; c.bins = bins;
    std::copy(totals_truth, totals_truth + 8, c.totals_truth);
    std::copy(totals_pred, totals_pred + 8, c.totals_pred);
    c.class_rows_truth.assign(class_rows_truth, class_rows_truth + C);
    c.class_rows_pred.assign(class_rows_pred, class_rows_pred + C);
    c.mix_truth.assign(mix_truth, mix_truth + C * C);
    c.mix_pred.assign(mix_pred, mix_pred + C * C);
    c.strata.assign(strata, strata + cells);
    return gcn_structure_write(path, c, &g_err);
}
int gcnhost_structure_read(const char *path, int *num_classes, int *bins, int64_t *totals_truth, int64_t *totals_pred, int64_t *class_rows_truth,
                           int64_t *class_rows_pred, int64_t *mix_truth, int64_t *mix_pred, int64_t *strata) {
    if (!path || !num_classes || !bins || !totals_truth || !totals_pred || !class_rows_truth || !class_rows_pred || !mix_truth || !mix_pred || !strata) {
        g_err = "structure_read: invalid argument";
        return -1;
    }
    StructureCounts c;
    if (gcn_structure_read(path, &c, &g_err) != 0) return -1;
    *num_classes = c.num_classes; *bins = c.bins;
    std::copy(c.totals_truth, c.totals_truth + 8, totals_truth);
    std::copy(c.totals_pred, c.totals_pred + 8, totals_pred);
    std::copy(c.class_rows_truth.begin(), c.class_rows_truth.end(), class_rows_truth);
    std::copy(c.class_rows_pred.begin(), c.class_rows_pred.end(), class_rows_pred);
    std::copy(c.mix_truth.begin(), c.mix_truth.end(), mix_truth);
    std::copy(c.mix_pred.begin(), c.mix_pred.end(), mix_pred);
    std::copy(c.strata.begin(), c.strata.end(), strata);
    return 0;
}
int gcnhost_model_label_distance(gcnhost_model *m, int source_mask, const int *source_nodes, int n_sources, int split, const int *nodes, int n,
                                 int max_hops, int64_t capacity, int32_t *dist, int32_t *nearest, int64_t *level_counts, int level_capacity,
                                 int64_t *info) {
    if (!m) { g_err = "gcnhost_model_label_distance: invalid argument"; return -1; }
    API_TRY({
        ModelQueries &q = m->gcn->queries();
        const int64_t listed = q.reach_rows("label_distance", split, nodes, n, source_mask, source_nodes, n_sources, max_hops, 1, false);
        if ((dist || nearest) && listed > capacity)
            throw GcnHipFailure(-1, "label_distance: the query lists " + std::to_string(listed) + " rows, the arrays are laid out for " + std::to_string(capacity));
        const ModelQueries::Reach r = q.label_distance(source_mask, source_nodes, n_sources, split, nodes, n, max_hops, dist, nearest, level_counts, level_capacity);
        if (info) { info[0] = r.rows; info[1] = r.sources; info[2] = r.skipped; info[3] = r.unreachable; info[4] = r.levels; }
    })
}
int gcnhost_model_components(gcnhost_model *m, int split, const int *nodes, int n, int source_mask, const int *source_nodes, int n_sources,
                             int64_t capacity, int32_t *component, int32_t *size, int64_t *totals, int64_t *info) {
    if (!m) { g_err = "gcnhost_model_components: invalid argument"; return -1; }
    API_TRY({
        ModelQueries &q = m->gcn->queries();
        const int64_t listed = q.reach_rows("components", split, nodes, n, source_mask, source_nodes, n_sources, 0, 1, false);
        if ((component || size) && listed > capacity)
            throw GcnHipFailure(-1, "components: the query lists " + std::to_string(listed) + " rows, the arrays are laid out for " + std::to_string(capacity));
        const ModelQueries::Reach r = q.components(split, nodes, n, source_mask, source_nodes, n_sources, component, size, totals);
        if (info) { info[0] = r.rows; info[1] = r.rounds; }
    })
}
int gcnhost_model_reach(gcnhost_model *m, int split, const int *nodes, int n, int source_mask, const int *source_nodes, int n_sources, int hops,
                        int predicted, int64_t capacity, int32_t *dist, int32_t *nearest, int32_t *component, int64_t *strata, int64_t *totals,
                        int64_t *level_counts, int level_capacity, int64_t *info) {
    if (!m) { g_err = "gcnhost_model_reach: invalid argument"; return -1; }
    API_TRY({
        ModelQueries &q = m->gcn->queries();
        const int64_t listed = q.reach_rows("reach", split, nodes, n, source_mask, source_nodes, n_sources, 0, hops, predicted != 0);
        if ((dist || nearest || component) && listed > capacity)
            throw GcnHipFailure(-1, "reach: the query lists " + std::to_string(listed) + " rows, the arrays are laid out for " + std::to_string(capacity));
        const ModelQueries::Reach r = q.reach(split, nodes, n, source_mask, source_nodes, n_sources, hops, predicted != 0, dist, nearest, component, strata,
                                              totals, level_counts, level_capacity);
        if (info) {
            info[0] = r.rows; info[1] = r.sources; info[2] = r.skipped; info[3] = r.unlabelled; info[4] = r.unreachable; info[5] = r.levels;
            info[6] = r.rounds;
        }
    })
}
int gcnhost_reach_metrics(const int64_t *strata, int hops, int layers, double *by_distance, double *groups, double *summary) {
    ReachMetrics r;
    if (gcn_reach_metrics(strata, hops, layers, &r, &g_err) != 0) return -1;
    auto row_out = [](const ReachRow &x, double *out) {
        const double v[6] = {(double)x.rows, (double)x.labelled, (double)x.correct, (double)x.nearest_correct, x.accuracy, x.nearest_accuracy};
        std::copy(v, v + 6, out);
    };
    for (size_t b = 0; by_distance && b < r.by_distance.size(); b++) row_out(r.by_distance[b], by_distance + 6 * b);
    if (groups) { row_out(r.inside, groups); row_out(r.outside, groups + 6); row_out(r.all, groups + 12); }
    if (summary) { summary[0] = (double)r.unreachable; summary[1] = r.unreachable_share; }
    return 0;
}
int gcnhost_reach_write(const char *path, int hops, int layers, const int64_t *info, const int64_t *totals, const int64_t *level_counts, int64_t n_levels,
                        const int64_t *strata) {
    if (!path || !info || !totals || !level_counts || !strata || hops < 1 || hops > REACH_MAX_HOPS || n_levels < 1 || n_levels > ((int64_t)1 << 31)) {
        g_err = "reach_write: invalid argument (1..32 hops, every table, at least the count of level 0)";
        return -1;
    }
    ReachCounts c;
    c.hops = hops; c.layers = layers;
    c.sources = info[0]; c.unlabelled = info[1]; c.rounds = info[2];
    std::copy(totals, totals + 6, c.totals);
    c.level_counts.assign(level_counts, level_counts + n_levels);
    c.strata.assign(strata, strata + (size_t)(hops + 2) * 4);
    return gcn_reach_write(path, c, &g_err);
}
int gcnhost_reach_read(const char *path, int *hops, int *layers, int64_t *info, int64_t *totals, int64_t *level_counts, int64_t level_capacity,
                       int64_t *n_levels, int64_t *strata) {
    if (!path || !hops || !layers || !info || !totals || !n_levels || !strata || level_capacity < 0 || (level_capacity > 0 && !level_counts)) {
        g_err = "reach_read: invalid argument";
        return -1;
    }
    ReachCounts c;
    if (gcn_reach_read(path, &c, &g_err) != 0) return -1;
    *hops = c.hops; *layers = c.layers;
    info[0] = c.sources; info[1] = c.unlabelled; info[2] = c.rounds;
    std::copy(c.totals, c.totals + 6, totals);
    *n_levels = (int64_t)c.level_counts.size();
    for (size_t i = 0; i < c.level_counts.size() && (int64_t)i < level_capacity; i++) level_counts[i] = c.level_counts[i];
    std::copy(c.strata.begin(), c.strata.end(), strata);
    return 0;
}
int gcnhost_calibration_report(int bins, const int64_t *count, const int64_t *correct, const double *conf_sum, double *accuracy,
                               double *confidence, double *summary) {
    CalibrationReport r;
    if (gcn_calibration_report(bins, count, correct, conf_sum, &r, &g_err) != 0) return -1;
    if (accuracy) std::copy(r.accuracy.begin(), r.accuracy.end(), accuracy);
    if (confidence) std::copy(r.confidence.begin(), r.confidence.end(), confidence);
    if (summary) { summary[0] = r.ece; summary[1] = r.mce; summary[2] = (double)r.rows; }
    return 0;
}
int gcnhost_model_conformal_fit(gcnhost_model *m, int split, const int *nodes, int n, double alpha, int method, float lam, int k_reg,
                                float diffusion, int per_class, gcnhost_conformal *fit, float *scores, int64_t scores_cap, int64_t *n_scores) {
    if (!m || !fit) { g_err = "gcnhost_model_conformal_fit: invalid argument"; return -1; }
    API_TRY({
        std::vector<float> s;
        const ModelQueries::Conformal f = m->gcn->queries().conformal_fit(split, nodes, n, alpha, method, lam, k_reg, diffusion, per_class != 0,
                                                                           scores || n_scores ? &s : nullptr);
        if (scores && (int64_t)s.size() > scores_cap) throw GcnHipFailure(-1, "conformal_fit: the scores need room for " + std::to_string(s.size()) + " floats");
        fit->method = f.method; fit->lam = f.lam; fit->k_reg = f.k_reg; fit->diffusion = f.diffusion; fit->temperature = f.temperature;
        fit->alpha = f.alpha; fit->per_class = f.per_class ? 1 : 0;
        std::copy(f.thresh, f.thresh + 64, fit->thresh);
        std::copy(f.n_cal, f.n_cal + 64, fit->n_cal);
        if (scores) std::copy(s.begin(), s.end(), scores);
        if (n_scores) *n_scores = (int64_t)s.size();
    })
}
int gcnhost_model_conformal_sets(gcnhost_model *m, const gcnhost_conformal *fit, int split, const int *nodes, int n, uint32_t *bits,
                                 int32_t *size, int64_t *counts) {
    if (!m || !fit) { g_err = "gcnhost_model_conformal_sets: invalid argument"; return -1; }
    API_TRY({
        ModelQueries::Conformal f;
        f.method = fit->method; f.lam = fit->lam; f.k_reg = fit->k_reg; f.diffusion = fit->diffusion; f.temperature = fit->temperature;
        f.alpha = fit->alpha; f.per_class = fit->per_class != 0;
        std::copy(fit->thresh, fit->thresh + 64, f.thresh);
        std::copy(fit->n_cal, fit->n_cal + 64, f.n_cal);
        m->gcn->queries().conformal_sets(f, split, nodes, n, bits, size, counts);
    })
}
int gcnhost_conformal_quantile(const float *scores, int64_t n, double alpha, const int32_t *labels, int num_classes, float *thresh,
                               int64_t *n_cal, int64_t *k) {
    return gcn_conformal_quantile(scores, n, alpha, labels, num_classes, thresh, n_cal, k, &g_err);
}
int gcnhost_model_ranking(gcnhost_model *m, int split, const int *nodes, int n, size_t scratch_bytes, int64_t *u2, double *ap_sum, int64_t *pos,
                          int64_t *neg, int64_t *invalid, int64_t *unlabelled, int64_t *rows, float *scores, int64_t scores_cap) {
    if (!m || !u2 || !ap_sum || !pos || !neg || !invalid) { g_err = "gcnhost_model_ranking: invalid argument"; return -1; }
    API_TRY({
        std::vector<float> s;
        const int64_t listed = m->gcn->queries().ranking(split, nodes, n, scratch_bytes, u2, ap_sum, pos, neg, invalid, unlabelled, scores ? &s : nullptr);
        if (scores && (int64_t)s.size() > scores_cap) throw GcnHipFailure(-1, "ranking: the scores need room for " + std::to_string(s.size()) + " floats");
        if (scores) std::copy(s.begin(), s.end(), scores);
        if (rows) *rows = listed;
    })
}
int gcnhost_ranking_report(int num_classes, const int64_t *u2, const double *ap_sum, const int64_t *pos, const int64_t *neg, double *auc, double *ap,
                           int32_t *auc_defined, int32_t *ap_defined, double *summary) {
    RankingReport r;
    if (gcn_ranking_report(num_classes, u2, ap_sum, pos, neg, &r, &g_err) != 0) return -1;
    if (auc) std::copy(r.auc.begin(), r.auc.end(), auc);
    if (ap) std::copy(r.ap.begin(), r.ap.end(), ap);
    if (auc_defined) std::copy(r.auc_defined.begin(), r.auc_defined.end(), auc_defined);
    if (ap_defined) std::copy(r.ap_defined.begin(), r.ap_defined.end(), ap_defined);
    if (summary) { summary[0] = r.macro_auc; summary[1] = r.macro_ap; summary[2] = r.weighted_auc; summary[3] = r.weighted_ap; summary[4] = (double)r.classes_defined; }
    return 0;
}
int gcnhost_model_tune_thresholds(gcnhost_model *m, int split, const int *nodes, int n, double beta, size_t scratch_bytes, float *thr, int64_t *tp,
                                  int64_t *fp, int64_t *fn, double *f, int64_t *pos, int64_t *neg, int64_t *invalid, int32_t *defined, int64_t *rows) {
    if (!m || !thr || !tp || !fp || !fn || !f || !pos || !neg || !invalid || !defined) { g_err = "gcnhost_model_tune_thresholds: invalid argument"; return -1; }
    API_TRY({
        const int64_t listed = m->gcn->queries().tune_thresholds(split, nodes, n, beta, scratch_bytes, thr, tp, fp, fn, f, pos, neg, invalid, defined);
        if (rows) *rows = listed;
    })
}
int gcnhost_model_predict_multilabel_thr(gcnhost_model *m, const int *nodes, int n, const float *thr, int n_thr, uint32_t *bits, float *prob) {
    if (!m || !thr) { g_err = "gcnhost_model_predict_multilabel_thr: invalid argument"; return -1; }
    API_TRY({ m->gcn->queries().predict_multilabel(nodes, n, thr, n_thr, bits, prob); })
}
int gcnhost_model_evaluate_thr(gcnhost_model *m, int split, const int *nodes, int n, const float *thr, int n_thr, int64_t *counts, int64_t *rows_counted) {
    if (!m || !thr || !counts) { g_err = "gcnhost_model_evaluate_thr: invalid argument"; return -1; }
    API_TRY({ m->gcn->queries().evaluate(split, nodes, n, thr, n_thr, counts, rows_counted); })
}
int gcnhost_thresholds_read(const char *path, int *num_classes, float *thr) {
    if (!path || !num_classes) { g_err = "gcnhost_thresholds_read: invalid argument"; return -1; }
    std::vector<float> t;
    if (gcn_thresholds_read(path, *num_classes, t, &g_err) != 0) return -1;
    *num_classes = (int)t.size();
    if (thr) memcpy(thr, t.data(), t.size() * sizeof(float));
    return 0;
}
int gcnhost_thresholds_write(const char *path, int num_classes, const float *thr, const int64_t *pos, const int64_t *neg, const int64_t *tp,
                             const int64_t *fp, const int64_t *fn, const double *f) {
    const bool any = pos || neg || tp || fp || fn || f, all = pos && neg && tp && fp && fn && f;
    if (any != all) { g_err = "gcnhost_thresholds_write: pos, neg, tp, fp, fn and f go together"; return -1; }
    ThresholdFit fit;
    fit.pos = pos; fit.neg = neg; fit.tp = tp; fit.fp = fp; fit.fn = fn; fit.f = f;
    return gcn_thresholds_write(path, num_classes, thr, all ? &fit : nullptr, &g_err);
}
int gcnhost_class_report(int num_classes, const int64_t *confusion, const int64_t *tp, const int64_t *fp, const int64_t *fn,
                         int64_t *tp_fp_fn, double *support, double *precision, double *recall, double *f1, double *summary) {
    ClassReport r;
    if (gcn_class_report(num_classes, confusion, tp, fp, fn, &r, &g_err) != 0) return -1;
    const size_t C = (size_t)num_classes;
    if (tp_fp_fn) {
        std::copy(r.tp.begin(), r.tp.end(), tp_fp_fn);
        std::copy(r.fp.begin(), r.fp.end(), tp_fp_fn + C);
        std::copy(r.fn.begin(), r.fn.end(), tp_fp_fn + 2 * C);
    }
    if (support) std::copy(r.support.begin(), r.support.end(), support);
    if (precision) std::copy(r.precision.begin(), r.precision.end(), precision);
    if (recall) std::copy(r.recall.begin(), r.recall.end(), recall);
    if (f1) std::copy(r.f1.begin(), r.f1.end(), f1);
    if (summary) { summary[0] = r.macro_f1; summary[1] = r.micro_f1; summary[2] = r.accuracy; }
    return 0;
}
int gcnhost_labels_read(const char *path, int *num_nodes, int *num_classes, uint32_t *bits) {
    if (!path || !num_nodes || !num_classes) { g_err = "gcnhost_labels_read: invalid argument"; return -1; }
    std::vector<uint32_t> b;
    int n = *num_nodes, c = *num_classes;
    if (gcn_labels_read(path, &n, &c, b, &g_err) != 0) return -1;
    *num_nodes = n;
    *num_classes = c;
    if (bits) memcpy(bits, b.data(), b.size() * sizeof(uint32_t));
    return 0;
}
int gcnhost_model_save_weights(gcnhost_model *m, const char *path) {
    if (!m || !path) { g_err = "gcnhost_model_save_weights: invalid argument"; return -1; }
    API_TRY({ m->gcn->save_weights(path); })
}
int gcnhost_model_load_weights(gcnhost_model *m, const char *path) {
    if (!m || !path) { g_err = "gcnhost_model_load_weights: invalid argument"; return -1; }
    API_TRY({ m->gcn->load_weights(path); })
}
int gcnhost_weights_write(const char *path, int input_dim, int hidden_dim, int output_dim, const float *w1, const float *w2) {
    return gcn_weights_write(path, input_dim, hidden_dim, output_dim, w1, w2, &g_err);
}
int gcnhost_weights_read(const char *path, int *input_dim, int *hidden_dim, int *output_dim, float *w1, float *w2) {
    return gcn_weights_read(path, input_dim, hidden_dim, output_dim, w1, w2, &g_err);
}
int gcnhost_model_timer(gcnhost_model *m, int id, double *seconds, long *count) {
    if (id < 0 || id >= __NUM_TMR) { g_err = "bad timer id"; return -1; }
    API_TRY({ *seconds = m->gcn->timer_total((timer_instance)id, count); })
}
int gcnhost_model_timers_reset(gcnhost_model *m) { API_TRY({ m->gcn->timers_reset(); }) }
int gcnhost_model_set_timers(gcnhost_model *m, int on) { API_TRY({ m->gcn->set_timers(on != 0); }) }

int gcnhost_dataset_load(gcnhost_dataset **out, const char *root, const char *name, gcnhost_params *p) {
    API_TRY({
        gcnhost_dataset *d = new gcnhost_dataset();
        GCNParams gp;
        memcpy(&gp, p, sizeof gp);
        Parser parser(&gp, &d->data, name, root ? root : "");
        if (!parser.parse()) { delete d; throw std::runtime_error(std::string("Cannot read input: ") + name); }
        memcpy(p, &gp, sizeof gp);
        *out = d;
    })
}
int gcnhost_dataset_arrays(gcnhost_dataset *d, const int **g_indptr, const int **g_indices, int64_t *g_nnz,
                           const int **f_indptr, const int **f_indices, const float **f_val, int64_t *f_nnz,
                           const int **split, int64_t *n_split, const int **label, int64_t *n_label) {
    if (!d) return -1;
    *g_indptr = d->data.graph.indptr.data(); *g_indices = d->data.graph.indices.data(); *g_nnz = (int64_t)d->data.graph.indices.size();
    *f_indptr = d->data.feature_index.indptr.data(); *f_indices = d->data.feature_index.indices.data();
    *f_val = d->data.feature_value.data(); *f_nnz = (int64_t)d->data.feature_value.size();
    *split = d->data.split.data(); *n_split = (int64_t)d->data.split.size();
    *label = d->data.label.data(); *n_label = (int64_t)d->data.label.size();
    return 0;
}
int gcnhost_dataset_save_binary(gcnhost_dataset *d, const gcnhost_params *p, const char *path) {
    GCNParams gp;
    memcpy(&gp, p, sizeof gp);
    return Parser::save_binary(path, gp, d->data) ? 0 : -1;
}
int gcnhost_dataset_free(gcnhost_dataset *d) { delete d; return 0; }

// The HALO exchange (RCCL: grouped ncclSend/ncclRecv straight into the table segments) on a small synthetic graph:
// node i points at i+1, i+3, i-1 and i + N/2 (mod N), so every rank needs rows of its neighbour ranks and of the rank
// half-way round; every table row must come back holding its global id.  Any transport.
static void halo_round_trip(gcnhip_ctx *ctx, Comm *comm, int rank, int world) {
    const int N = world * 96, ld = 8;
    std::vector<int> gp(N + 1), gi;
    for (int i = 0; i < N; i++) {
        gp[i] = (int)gi.size();
        gi.push_back(i);
        for (int off : {1, 3, N / 2, N - 1}) gi.push_back((i + off) % N);
    }
    gp[N] = (int)gi.size();
    const RowPartition part = make_partition(gp.data(), N, world);
    const ExchangePlan plan = make_exchange_plan(gp.data(), gi.data(), N, part, rank, /*HALO*/ 2);
    ExchangeBuffers xb;
    exchange_buffers_create(ctx, plan, ld, &xb);
    std::vector<float> tab((size_t)plan.table_rows * ld, -1.f);
    for (int r = 0; r < plan.n_local; r++)
        for (int k = 0; k < ld; k++) tab[(size_t)r * ld + k] = (float)(part.start[rank] + r) + 0.125f * k;
    void *dt = nullptr;
    try {
        GCNHIP_CHECK(gcnhip_malloc(ctx, &dt, tab.size() * sizeof(float)));
        GCNHIP_CHECK(gcnhip_h2d(ctx, dt, tab.data(), tab.size() * sizeof(float)));
        for (int it = 0; it < 3; it++) comm->exchange_rows(plan, xb, (float *)dt, ld);
        GCNHIP_CHECK(gcnhip_d2h(ctx, tab.data(), dt, tab.size() * sizeof(float)));
    } catch (...) {
        gcnhip_free(ctx, dt);
        exchange_buffers_destroy(&xb);
        throw;
    }
    gcnhip_free(ctx, dt);
    exchange_buffers_destroy(&xb);
    for (int t = 0; t < plan.table_rows; t++)
        for (int k = 0; k < ld; k++)
            if (tab[(size_t)t * ld + k] != (float)plan.table_global[t] + 0.125f * k)
                throw GcnHipFailure(-1, "halo exchange self-test: a table row came back with the wrong content");
}

// RCCL round trip with `world` ranks (one per process; world == 1: a single-rank communicator): communicator
// init from the shared unique id, in-place all-gather of distinct blocks, all-reduce, the halo exchange (grouped
// ncclSend/ncclRecv through an ExchangePlan's send lists, world > 1), the validation lane's split communicator on a
// second stream, and collectives alternating between the two (turnstile order).
int gcnhost_rccl_selftest_world(int device, int rank, int world, const char *nccl_id) {
    if (world < 1 || rank < 0 || rank >= world || !nccl_id) { g_err = "bad rank/world/id"; return -1; }
    API_TRY({
        gcnhip_ctx *ctx = nullptr;
        GCNHIP_CHECK(gcnhip_ctx_create(&ctx, device, nullptr));
        {
            std::unique_ptr<Comm> comm(make_rccl_comm(ctx, rank, world, nccl_id));
            const size_t B = 1024;
            std::vector<float> h(B * world, -1.f);
            for (size_t i = 0; i < B; i++) h[rank * B + i] = (float)(rank * 1000) + (float)i * 0.5f;
            void *d;
            GCNHIP_CHECK(gcnhip_malloc(ctx, &d, h.size() * sizeof(float)));
            GCNHIP_CHECK(gcnhip_h2d(ctx, d, h.data(), h.size() * sizeof(float)));
            comm->allgather_rows((float *)d, B);
            std::vector<float> back(h.size());
            GCNHIP_CHECK(gcnhip_d2h(ctx, back.data(), d, back.size() * sizeof(float)));
            for (int q = 0; q < world; q++)
                for (size_t i = 0; i < B; i++)
                    if (back[q * B + i] != (float)(q * 1000) + (float)i * 0.5f)
                        throw GcnHipFailure(-1, "RCCL self-test: all-gather block mismatch");
            comm->allreduce_sum((float *)d, B);        // block 0 of every rank is now identical: sum = world * value
            GCNHIP_CHECK(gcnhip_d2h(ctx, back.data(), d, B * sizeof(float)));
            for (size_t i = 0; i < B; i++)
                if (back[i] != (float)world * ((float)i * 0.5f)) throw GcnHipFailure(-1, "RCCL self-test: all-reduce mismatch");
            gcnhip_free(ctx, d);
            if (world > 1) halo_round_trip(ctx, comm.get(), rank, world);
            void *sa;
            GCNHIP_CHECK(gcnhip_malloc(ctx, &sa, 256 * world * sizeof(float)));
            GCNHIP_CHECK(gcnhip_memset_async(ctx, sa, 0, 256 * world * sizeof(float)));
            float *scratch_a = (float *)sa;
            double v[2] = {3.0, 4.0 + rank};
            comm->allreduce_sum_host(v, 2);
            if (v[0] != 3.0 * world || v[1] != 4.0 * world + world * (world - 1) / 2.0)
                throw GcnHipFailure(-1, "RCCL self-test: host reduction");
            // the validation lane's communicator (ncclCommSplit) on a second stream
            gcnhip_ctx *ctx2 = nullptr;
            GCNHIP_CHECK(gcnhip_ctx_create(&ctx2, device, nullptr));
            {
                std::unique_ptr<Comm> comm2(comm->clone_for(ctx2));
                double w2[1] = {5.0};
                comm2->allreduce_sum_host(w2, 1);
                if (w2[0] != 5.0 * world) throw GcnHipFailure(-1, "RCCL self-test: split communicator");
                // collectives alternating between the two lanes (serialised by the turnstile event)
                void *d2;
                GCNHIP_CHECK(gcnhip_malloc(ctx2, &d2, 256 * world * sizeof(float)));
                GCNHIP_CHECK(gcnhip_memset_async(ctx2, d2, 0, 256 * world * sizeof(float)));
                for (int it = 0; it < 4; it++) {
                    comm->allreduce_sum(scratch_a, 256);
                    comm2->allgather_rows((float *)d2, 256);
                    comm2->allreduce_sum((float *)d2, 256);
                    comm->allgather_rows(scratch_a, 256);
                }
                GCNHIP_CHECK(gcnhip_ctx_sync(ctx));
                GCNHIP_CHECK(gcnhip_ctx_sync(ctx2));
                gcnhip_free(ctx2, d2);
            }
            gcnhip_ctx_destroy(ctx2);
            gcnhip_free(ctx, sa);
        }
        gcnhip_ctx_destroy(ctx);
    })
}

// the same halo round trip through the host-staged transport (tests: ranks as threads or gloo processes sharing a GPU)
int gcnhost_halo_selftest_host(int device, int rank, int world, gcnhost_allgather_fn ag, gcnhost_allreduce_fn ar, void *user) {
    if (world < 2 || rank < 0 || rank >= world || !ag || !ar) { g_err = "bad rank/world/callbacks"; return -1; }
    API_TRY({
        gcnhip_ctx *ctx = nullptr;
        GCNHIP_CHECK(gcnhip_ctx_create(&ctx, device, nullptr));
        try {
            std::unique_ptr<Comm> comm(make_host_comm(ctx, rank, world, ag, ar, user));
            halo_round_trip(ctx, comm.get(), rank, world);
        } catch (...) {
            gcnhip_ctx_destroy(ctx);
            throw;
        }
        gcnhip_ctx_destroy(ctx);
    })
}

// Device time per collective on the stream, HIP events around `iters` back-to-back calls (after two warm-up calls): the
// in-place all-gather of `block_floats` floats per rank and the all-reduce of `reduce_floats` floats, as the epoch issues
// them.  With one rank (what a single-GPU box can run) this is the launch + kernel floor of a collective — a LOWER bound on
// what a peer adds; tools/comm_model.py takes it instead of an assumed latency.
int gcnhost_rccl_collective_us(int device, int rank, int world, const char *nccl_id, long block_floats, long reduce_floats, int iters,
                               double *us_allgather, double *us_allreduce) {
    if (world < 1 || rank < 0 || rank >= world || !nccl_id || block_floats < 1 || reduce_floats < 1 || iters < 1) { g_err = "bad arguments"; return -1; }
    API_TRY({
        gcnhip_ctx *ctx = nullptr;
        GCNHIP_CHECK(gcnhip_ctx_create(&ctx, device, nullptr));
        {
            std::unique_ptr<Comm> comm(make_rccl_comm(ctx, rank, world, nccl_id));
            void *d = nullptr, *e0 = nullptr, *e1 = nullptr;
            const size_t n = std::max((size_t)block_floats * world, (size_t)reduce_floats);
            GCNHIP_CHECK(gcnhip_malloc(ctx, &d, n * sizeof(float)));
            GCNHIP_CHECK(gcnhip_memset_async(ctx, d, 0, n * sizeof(float)));
            GCNHIP_CHECK(gcnhip_event_create(&e0));
            GCNHIP_CHECK(gcnhip_event_create(&e1));
            float ms = 0.f;
            for (int which = 0; which < 2; which++) {
                for (int i = 0; i < 2 + iters; i++) {
                    if (i == 2) GCNHIP_CHECK(gcnhip_event_record(ctx, e0));
                    if (which == 0) comm->allgather_rows((float *)d, (size_t)block_floats);
                    else comm->allreduce_sum((float *)d, (size_t)reduce_floats);
                }
                GCNHIP_CHECK(gcnhip_event_record(ctx, e1));
                GCNHIP_CHECK(gcnhip_event_elapsed_ms(e0, e1, &ms));
                if (which == 0 && us_allgather) *us_allgather = 1e3 * ms / iters;
                if (which == 1 && us_allreduce) *us_allreduce = 1e3 * ms / iters;
            }
            gcnhip_event_destroy(e0);
            gcnhip_event_destroy(e1);
            gcnhip_free(ctx, d);
        }
        gcnhip_ctx_destroy(ctx);
    })
}

int gcnhost_rccl_selftest(int device) {
    char id[GCN_NCCL_ID_BYTES];
    const int rc = rccl_get_unique_id(id);
    if (rc) { g_err = "ncclGetUniqueId failed"; return rc; }
    return gcnhost_rccl_selftest_world(device, 0, 1, id);
}

int gcnhost_partition(const int *g_indptr, int n_rows, int world, int *start, int *rows_max) {
    if (!g_indptr || !start || world < 1) return -1;
    RowPartition p = make_partition(g_indptr, n_rows, world);
    for (int q = 0; q <= world; q++) start[q] = p.start[q];
    if (rows_max) *rows_max = p.rows_max;
    return 0;
}
int gcnhost_local_graph(const int *g_indptr, const int *g_indices, int n_rows, int world, int rank,
                        int *indptr, int *indices, int *col_deg, int *n_local, int *n_cols, int64_t *nnz_local) {
    if (!g_indptr || !g_indices || world < 1 || rank < 0 || rank >= world) return -1;
    const RowPartition part = make_partition(g_indptr, n_rows, world);
    const LocalGraph lg = build_local_graph(g_indptr, g_indices, n_rows, part, rank);
    if (n_local) *n_local = lg.n_rows;
    if (n_cols) *n_cols = lg.n_cols;
    if (nnz_local) *nnz_local = (int64_t)lg.indices.size();
    if (indptr) memcpy(indptr, lg.indptr.data(), lg.indptr.size() * sizeof(int));
    if (indices && !lg.indices.empty()) memcpy(indices, lg.indices.data(), lg.indices.size() * sizeof(int));
    if (col_deg) memcpy(col_deg, lg.col_deg.data(), lg.col_deg.size() * sizeof(int));
    return 0;
}
struct gcnhost_plan {
    RowPartition part;
    ExchangePlan plan;
    LocalGraph graph;
};
int gcnhost_plan_create(gcnhost_plan **out, const int *g_indptr, const int *g_indices, int n_rows, int world, int rank, int mode) {
    if (!out || !g_indptr || !g_indices || world < 1 || rank < 0 || rank >= world || mode < 0 || mode > 2) return -1;
    API_TRY({
        gcnhost_plan *p = new gcnhost_plan();
        p->part = make_partition(g_indptr, n_rows, world);
        p->plan = make_exchange_plan(g_indptr, g_indices, n_rows, p->part, rank, mode);
        p->graph = build_table_graph(g_indptr, g_indices, n_rows, p->part, p->plan);
        *out = p;
    })
}
int gcnhost_plan_info(const gcnhost_plan *p, int *halo, int *n_local, int *table_rows, int *own_offset, int *rows_max,
                      double *halo_share, int64_t *nnz_local, int64_t *n_recv, int64_t *n_send) {
    if (!p) return -1;
    if (halo) *halo = p->plan.halo ? 1 : 0;
    if (n_local) *n_local = p->plan.n_local;
    if (table_rows) *table_rows = p->plan.table_rows;
    if (own_offset) *own_offset = p->plan.own_offset;
    if (rows_max) *rows_max = p->plan.rows_max;
    if (halo_share) *halo_share = p->plan.halo_share;
    if (nnz_local) *nnz_local = (int64_t)p->graph.indices.size();
    if (n_recv) *n_recv = (int64_t)p->plan.recv_rows.size();
    if (n_send) *n_send = (int64_t)p->plan.send_rows.size();
    return 0;
}
int gcnhost_plan_arrays(const gcnhost_plan *p, const int **recv_off, const int **recv_rows, const int **send_off, const int **send_rows,
                        const int **table_global, const int **indptr, const int **indices, const int **col_deg) {
    if (!p) return -1;
    if (recv_off) *recv_off = p->plan.recv_off.data();
    if (recv_rows) *recv_rows = p->plan.recv_rows.data();
    if (send_off) *send_off = p->plan.send_off.data();
    if (send_rows) *send_rows = p->plan.send_rows.data();
    if (table_global) *table_global = p->plan.table_global.data();
    if (indptr) *indptr = p->graph.indptr.data();
    if (indices) *indices = p->graph.indices.data();
    if (col_deg) *col_deg = p->graph.col_deg.data();
    return 0;
}
int gcnhost_plan_free(gcnhost_plan *p) { delete p; return 0; }

int gcnhost_choose_node_order(const int *g_indptr, const int *g_indices, int n_rows, int world, int force, int *order, int *renumbered,
                              double *ids_share, int64_t *ids_recv_rows, double *new_share, int64_t *new_recv_rows, int64_t *allgather_rows) {
    if (!g_indptr || !g_indices || n_rows < 0 || world < 1) return -1;
    API_TRY({
        StructureGroups sg;
        const OrderCost ids = exchange_cost(g_indptr, g_indices, n_rows, world);
        if ((force || ids.halo_share > 0.75) && n_rows >= 4096) sg = structure_groups(g_indptr, g_indices, n_rows);
        const NodeOrderChoice ch = choose_node_order(g_indptr, g_indices, n_rows, world, sg.useful ? sg.group.data() : nullptr, force != 0);
        if (renumbered) *renumbered = !ch.order.empty();
        if (order) {                                            // the identity, under the chosen order when there is one
            std::iota(order, order + n_rows, 0);
            std::copy(ch.order.begin(), ch.order.end(), order);
        }
        if (ids_share) *ids_share = ch.ids.halo_share;
        if (ids_recv_rows) *ids_recv_rows = ch.ids.recv_rows_max;
        if (new_share) *new_share = ch.chosen.halo_share;
        if (new_recv_rows) *new_recv_rows = ch.chosen.recv_rows_max;
        if (allgather_rows) *allgather_rows = (int64_t)(world - 1) * ch.ids.rows_max;
    })
}

int gcnhost_structure_groups(const int *g_indptr, const int *g_indices, int n_rows, int *group, int *n_groups, int *sweeps,
                             double *largest_share, int *useful) {
    if (!g_indptr || !g_indices || n_rows < 0 || !group) return -1;
    API_TRY({
        const StructureGroups sg = structure_groups(g_indptr, g_indices, n_rows);
        if (n_rows) memcpy(group, sg.group.data(), (size_t)n_rows * sizeof(int));
        if (n_groups) *n_groups = sg.n_groups;
        if (sweeps) *sweeps = sg.sweeps;
        if (largest_share) *largest_share = sg.largest_share;
        if (useful) *useful = sg.useful ? 1 : 0;
    })
}

int gcnhost_glorot(float *w, int size, int in_size, int out_size, long seed, int skip_draws) {
    HostRng rng;
    rng.seed_time((unsigned)seed);
    for (int i = 0; i < skip_draws; i++) rng.next();
    Variable v(size, false);
    v.glorot(in_size, out_size, rng);
    memcpy(w, v.data.data(), (size_t)size * sizeof(float));
    return 0;
}
int gcnhost_host_masks(uint8_t *keep, int64_t n, float p, long seed, int64_t skip_draws) {
    HostRng rng;
    rng.seed_time((unsigned)seed);
    for (int64_t i = 0; i < skip_draws; i++) rng.next();
    const int thr = (int)(p * MY_RAND_MAX);
    for (int64_t i = 0; i < n; i++) keep[i] = (int)rng.next() >= thr;
    return 0;
}

}  // extern "C"
