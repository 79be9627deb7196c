// gcn_access.cpp — a built HipGCN read and written from outside the epoch loop: variables, weights and the weights file, and
// the hooked evaluation forward that the queries (host/queries.cpp) run.
#include "gcn.h"
#include "weights.h"
#include "hip_check.h"

void HipGCN::row_scale(std::vector<float> &dinv) {
    dinv.assign((size_t)n_local, 1.f);
    const float *d = nullptr;
    GCNHIP_CHECK(gcnhip_graph_scales(graph, &d, nullptr, nullptr, nullptr));
    if (n_local) GCNHIP_CHECK(gcnhip_d2h(env.ctx, dinv.data(), d, dinv.size() * sizeof(float)));
}

void HipGCN::get_var(int k, bool grad, std::vector<float> &out, int *rows, int *cols) {
    if (k < 1 || k > 6) throw GcnHipFailure(-1, "get_var: k must be 1..6");
    HipVariable *v = variables[k].get();
    if (k == 3 && !grad && h1_from_fused_eval && !eval_modules.empty()) {
        // the last forward on this stream was an evaluation whose hidden matrix stayed in registers: run it as its own launch
        static_cast<HipSparseMatmul *>(eval_modules[0])->forward_stored();
        h1_from_fused_eval = false;
        sync();
    }
    out.resize((size_t)v->rows * v->cols);
    v->download(out.data(), grad);
    if (rows) *rows = v->rows;
    if (cols) *cols = v->cols;
}

void HipGCN::set_weights(const float *w1, const float *w2) {
    variables[2]->upload(w1);
    variables[5]->upload(w2);
    GCNHIP_CHECK(gcnhip_sumsq(env.ctx, variables[2]->data, (int64_t)variables[2]->elems(), optimizer->d_sumsq));
    sync();
}

// An evaluation forward (eval_async's module list without the loss) on the main stream with one hook set on the logit
// aggregation: the prediction epilogue, or the logits redirected to a scratch table.  Training state stays as it was.
void HipGCN::forward_hooked(const HipGraphSum::Prediction *prediction, const HipGraphSum::Redirect *redirect) {
    refresh_input();
    const std::vector<Module *> &list = eval_modules.empty() ? modules : eval_modules;
    struct Unhook {                                            // also when a forward throws
        HipGraphSum *gs;
        ~Unhook() { gs->predict = nullptr; gs->redirect = nullptr; }
    } unhook{logits_gs};
    logits_gs->predict = prediction;
    logits_gs->redirect = redirect;
    for (size_t i = 0; i + 1 < list.size(); i++) list[i]->forward(false);           // the last module is the loss
    // variable 3: a fused evaluation keeps H1 in registers (what it held stays); otherwise the forward stored it
    if (eval_modules.empty() || !static_cast<HipSparseMatmul *>(eval_modules[0])->hidden_not_stored) h1_from_fused_eval = false;
}

// The evaluation forward up to the class-layer product: variable 4 = H1.W2 of every row of this rank (dinv . H1.W2 on a factored
// model), neither the logit aggregation nor the loss — what a query needs that aggregates those rows itself (predict_new).
// Variable 1 = X.W1 is written on the way unless the model evaluates aggregate-first.  Training state stays as it was.
void HipGCN::forward_class_products() {
    refresh_input();
    const std::vector<Module *> &list = eval_modules.empty() ? modules : eval_modules;
    for (size_t i = 0; i + 2 < list.size(); i++) list[i]->forward(false);           // the last two: the logit aggregation, the loss
    if (eval_modules.empty() || !static_cast<HipSparseMatmul *>(eval_modules[0])->hidden_not_stored) h1_from_fused_eval = false;
}

// The hidden matrix of an evaluation forward in variable 3 at the price of its own product: an aggregate-first model computes
// ReLU((A^.X).W1) in one launch (what get_var(3) runs after a fused evaluation, so the bits are get_var's).  Other models have
// no such form: the caller runs a whole hooked forward, whose hidden-width aggregation stores the matrix.
bool HipGCN::forward_hidden_only() {
    if (eval_modules.empty()) return false;
    refresh_input();
    static_cast<HipSparseMatmul *>(eval_modules[0])->forward_stored();
    h1_from_fused_eval = false;
    return true;
}

void HipGCN::save_weights(const char *path) {
    std::vector<float> w1, w2;
    get_var(2, false, w1, nullptr, nullptr);
    get_var(5, false, w2, nullptr, nullptr);
    std::string err;
    if (gcn_weights_write(path, params.input_dim, params.hidden_dim, params.output_dim, w1.data(), w2.data(), &err) != 0) throw GcnHipFailure(-1, err);
}

void HipGCN::load_weights(const char *path) {
    int F = params.input_dim, h = params.hidden_dim, C = params.output_dim;
    std::vector<float> w1((size_t)F * h), w2((size_t)h * C);
    std::string err;
    if (gcn_weights_read(path, &F, &h, &C, w1.data(), w2.data(), &err) != 0) throw GcnHipFailure(-1, err);
    set_weights(w1.data(), w2.data());
}
