// predict_new.cpp — ModelQueries::predict_new: nodes the dataset did not hold, attached to the trained graph (queries.h has the
// definition and the contract, attach.h the stored rows, csrc/attach.hip the gather).  Off the epoch path.
#include "queries.h"
#include "attach.h"
#include "gcn.h"
#include "hip_check.h"
#include <cmath>

void ModelQueries::predict_new(const int *x_indptr, const int *x_indices, const float *x_values, int n_new, const int64_t *nbr_ptr, const int *nbr_ids,
                               const float *thr, int n_thr, int32_t *pred, float *prob, float *logp, uint32_t *bits) {
    const char *what = "predict_new";
    const std::string w = std::string(what) + ": ";
    const bool ml = m.opt_.multilabel;
    const int N = m.params.num_nodes, F = m.params.input_dim, H = m.params.hidden_dim, C = m.params.output_dim;
    require(what, ONE_RANK | (ml ? AT_MOST_256 : AT_MOST_64) | (thr ? MULTI_LABEL : 0));
    if (thr) thresholds_check(what, thr, n_thr);
    if (m.flags & HIPGCN_BF16_TABLES) throw GcnHipFailure(-1, w + "not with bf16 tables (the new rows gather the f32 rows a forward stores)");
    if (H < 1 || H > 256) throw GcnHipFailure(-1, w + "a hidden width of at most 256 (the gather of a new row takes at most 256 columns)");
    if (n_new < 0) throw GcnHipFailure(-1, w + "m = " + std::to_string(n_new) + " is negative");
    if (!x_indptr || !nbr_ptr || (n_new > 0 && (!x_values || (ml ? !bits : (!pred || !prob))))) throw GcnHipFailure(-1, w + "invalid argument");
    // X_new, as the dataset's own feature arrays are laid out
    if (x_indptr[0] != 0) throw GcnHipFailure(-1, w + "the feature row pointers do not start at 0");
    for (int i = 0; i < n_new; i++) {
        if (x_indptr[i + 1] < x_indptr[i]) throw GcnHipFailure(-1, w + "the feature row pointers decrease at new node " + std::to_string(i));
        if (!x_indices && x_indptr[i + 1] - x_indptr[i] != F)
            throw GcnHipFailure(-1, w + "dense feature rows have " + std::to_string(x_indptr[i + 1] - x_indptr[i]) + " values, the model takes " + std::to_string(F));
    }
    if (x_indices)
        for (int64_t e = 0; e < x_indptr[n_new]; e++)
            if (x_indices[e] < 0 || x_indices[e] >= F)
                throw GcnHipFailure(-1, w + "feature column " + std::to_string(x_indices[e]) + " is outside the model's input width " + std::to_string(F));
    m.sync();                                                  // run()'s epochs in flight, the validation lane's pass
    // the stored rows: lengths by table row from the adjacency's own row pointers, dataset ids mapped as query_rows maps them
    const std::vector<int> &ip = explain_indptr();
    std::vector<int> row_len((size_t)m.n_local), row_of_id;
    for (int r = 0; r < m.n_local; r++) row_len[r] = ip[r + 1] - ip[r];
    if (!m.node_order_.empty()) {
        row_of_id.assign((size_t)N, 0);
        for (int p = 0; p < N; p++) row_of_id[m.node_order_[p]] = p;
    }
    AttachRows rows;
    std::string err;
    if (gcn_attach_rows(N, row_len.data(), row_of_id.empty() ? nullptr : row_of_id.data(), n_new, nbr_ptr, nbr_ids,
                        m.factored_ ? ATTACH_COEF_FACTORED : ATTACH_COEF_EDGE, &rows, &err) != 0)
        throw GcnHipFailure(-1, w + err);
    if (n_new == 0) return;
    const size_t nn = (size_t)n_new, nnz = rows.col.size();
    // factored model: the gathered tables carry dinv of their own row, the new rows' product too (the factor rides in X_new's
    // values, as apply_factored_scales puts it into X); the hidden gather leaves dinv(v) . h_v, as variable 3 holds it
    std::vector<float> xv, coef_hidden;
    if (m.factored_) {
        xv.assign(x_values, x_values + x_indptr[n_new]);
        for (int i = 0; i < n_new; i++)
            for (int e = x_indptr[i]; e < x_indptr[i + 1]; e++) xv[e] *= rows.coef[rows.ptr[i]];
        x_values = xv.data();
        coef_hidden.resize(nnz);
        for (size_t e = 0; e < nnz; e++) coef_hidden[e] = rows.coef[e] * rows.coef[e];
    }
    const HipVariable &T = *m.variables[1], &W1 = *m.variables[2], &H1 = *m.variables[3], &P = *m.variables[4], &W2 = *m.variables[5];
    gcnhip_ctx *ctx = m.env.ctx;
    const uint64_t seed = m.env.seed ^ KEY_INPUT_DROPOUT;       // no dropout (p = 0): the arguments of the model's own evaluation product
    float *d_tb = d_nn_tb.need(nn * T.ld), *d_hb = d_nn_hb.need(nn * H1.ld), *d_pb = d_nn_pb.need(nn * P.ld);
    int32_t *d_ptr = d_nn_ptr.need(nn + 1), *d_col = d_nn_col.need(nnz);
    float *d_coef = d_nn_coef.need(2 * nnz), *d_coef_hidden = m.factored_ ? d_coef + nnz : d_coef;
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_ptr, rows.ptr.data(), (nn + 1) * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_col, rows.col.data(), nnz * sizeof(int32_t)));
    GCNHIP_CHECK(gcnhip_h2d(ctx, d_coef, rows.coef.data(), nnz * sizeof(float)));
    if (m.factored_) GCNHIP_CHECK(gcnhip_h2d(ctx, d_coef_hidden, coef_hidden.data(), nnz * sizeof(float)));
    // the dataset nodes: H1.W2 in variable 4, and X.W1 — variable 1 where the forward ran that product, else the product itself
    m.forward_class_products();
    const float *d_ta = T.data;
    if (!m.eval_modules.empty()) {
        float *t = d_nn_ta.need((size_t)m.n_local * T.ld);
        GCNHIP_CHECK(gcnhip_spmm_fwd(ctx, m.feat, gcnhip_feat_values(m.feat), W1.data, W1.ld, t, T.ld, H, 0.f, seed, m.env.d_epoch, 0, nullptr));
        d_ta = t;
    }
    // the new nodes: X_new . W1, the hidden gather, h . W2, the class gather
    gcnhip_feat *x_new = nullptr;
    GCNHIP_CHECK(gcnhip_feat_create(ctx, &x_new, x_indptr, x_indices, x_values, n_new, F));
    struct Destroy {                                           // also when a launch throws
        gcnhip_ctx *ctx; gcnhip_feat *f;
        ~Destroy() { gcnhip_feat_destroy(ctx, f); }
    } destroy{ctx, x_new};
    GCNHIP_CHECK(gcnhip_spmm_fwd(ctx, x_new, gcnhip_feat_values(x_new), W1.data, W1.ld, d_tb, T.ld, H, 0.f, seed, m.env.d_epoch, 0, nullptr));
    GCNHIP_CHECK(gcnhip_attach_gather(ctx, d_ptr, d_col, d_coef_hidden, n_new, d_ta, T.ld, m.n_local, d_tb, T.ld, H, 1, d_hb, H1.ld, nullptr, nullptr, nullptr, 0, 1.f));
    GCNHIP_CHECK(gcnhip_matmul_fwd(ctx, d_hb, H1.ld, W2.data, W2.ld, d_pb, P.ld, n_new, H, C));
    if (ml) {
        const int wpr = m.ml_wpr;
        float *d_z = d_nn_z.need(nn * P.ld), *d_q = prob ? d_nn_prob.need(nn * C) : nullptr;
        uint32_t *d_bits = d_nn_bits.need(nn * wpr);
        GCNHIP_CHECK(gcnhip_attach_gather(ctx, d_ptr, d_col, d_coef, n_new, P.data, P.ld, m.n_local, d_pb, P.ld, C, 0, d_z, P.ld, nullptr, nullptr, nullptr, 0, 1.f));
        if (thr) GCNHIP_CHECK(gcnhip_bce_predict_rows_thr(ctx, d_z, P.ld, nullptr, n_new, C, upload_cuts(thr), d_bits, wpr, d_q, C));
        else GCNHIP_CHECK(gcnhip_bce_predict_rows(ctx, d_z, P.ld, nullptr, n_new, C, d_bits, wpr, d_q, C));
        GCNHIP_CHECK(gcnhip_d2h(ctx, bits, d_bits, nn * wpr * sizeof(uint32_t)));
        if (prob) GCNHIP_CHECK(gcnhip_d2h(ctx, prob, d_q, nn * C * sizeof(float)));
    } else {
        int32_t *d_p = d_nn_pred.need(nn);
        float *d_q = d_nn_prob.need(nn), *d_l = logp ? d_nn_logp.need(nn * C) : nullptr;
        GCNHIP_CHECK(gcnhip_attach_gather(ctx, d_ptr, d_col, d_coef, n_new, P.data, P.ld, m.n_local, d_pb, P.ld, C, 2, nullptr, 0, d_p, d_q, d_l, C,
                                          1.f / temperature_));
        GCNHIP_CHECK(gcnhip_d2h(ctx, pred, d_p, nn * sizeof(int32_t)));
        GCNHIP_CHECK(gcnhip_d2h(ctx, prob, d_q, nn * sizeof(float)));
        if (logp) GCNHIP_CHECK(gcnhip_d2h(ctx, logp, d_l, nn * C * sizeof(float)));
    }
    m.sync();
}
