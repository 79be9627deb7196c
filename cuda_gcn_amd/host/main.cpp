// main.cpp — `gcn-hip <graph_name> [...]`: the reference's command line
// (src/main.cpp:15-48) for the MI355X backend.  It prints the same lines as
// gcn-seq ("RUNNING ON GPU", per-epoch loss/accuracy, totals) and implements
// the positional hyper-parameters the reference's usage string advertises but
// never reads (src/main.cpp:24-25):
//
//   gcn-hip graph_name [num_nodes input_dim hidden_dim output_dim dropout
//                       learning_rate weight_decay epochs early_stopping]
//
// "-" keeps a default; num_nodes/input_dim/output_dim always come from the
// data.  Environment: GCN_SEED (plays time(NULL) of rand.cpp:7), GCN_DATA_ROOT,
// GCN_GPUS=N (row-partition over N GPUs of this node, one host thread per GPU,
// RCCL over xGMI), GCN_MODULAR=1, GCN_HOST_MASKS=1, GCN_TIMERS=1,
// GCN_BF16_TABLES=1 (opt-in storage format of the aggregation inputs, beyond the reference),
// GCN_OVERLAP=1 (row-partitioned runs: exchanges on their own stream beside the aggregation of the
// locally owned columns).
//
// Schedule defaults follow from ONE question: does a printed number feed back into the run?
//  * early_stopping == 0 (the reference's default, gcn.cpp:9-11): no.  The run takes the library's fastest tested
//    schedule — epochs enqueued ahead of the line being printed (HipGCN::run_pipelined), evaluation forwards as
//    ReLU((A^.X).W1) with A^.X built once (validation loss within 2e-5 of the reference's operation order, training
//    bit-identical), and on one GPU either the validation forward on a second stream (graphs above LANE_MIN_NODES
//    nodes: Pubmed, Reddit) or one stream replaying the captured epoch (Cora, Citeseer: 18 launches of ~4 us, where two
//    streams of eager launches are bound by the host; tools/cli_small.py).  Metrics come back in groups of consecutive
//    epochs (1 on Reddit, 16 where an epoch takes ~100 us): the lines of a group are printed together, `time=` is the
//    group's interval / its size; `total training time=` their sum = the wall time of the loop.
//  * early_stopping > 0: yes — gcn.cpp:141-150 compares validation losses between epochs.  The loop is the
//    reference's (one epoch, wait, print, decide) and evaluation keeps its operation order A^.(X.W1), so that a
//    near-tie stops at the epoch gcn-seq stops at.
// GCN_WRITE_CACHE=1: after parsing the text files, write data/<name>.gcnbin for the next run.
// Overrides: GCN_SYNC_EPOCHS=1 (reference loop, `time=` = that epoch's own latency), GCN_EVAL_LANE=0|1,
// GCN_REFERENCE_ORDER=0|1.
// Trained weights and predictions (beyond the reference, whose program keeps nothing; stdout is unchanged, notes go to stderr):
//   GCN_LOAD_WEIGHTS=<file>  after the model is built, before the run, its weights come from the file (host/weights.h; the widths
//                            must match the dataset and hidden_dim).  With epochs = 0 (positional argument 9) the run is
//                            inference only: `total training time=0.00000` and the test line of the loaded weights.
//   GCN_SAVE_WEIGHTS=<file>  after the run, rank 0 writes the final weights.
//   GCN_PREDICT=<file>       after the test line, one line per node of the dataset in id order: `node class probability`
//                            (class = argmax of the node's logits, lowest on a tie; its softmax probability).  With several
//                            GPUs each worker predicts its own rows into an array indexed by node id; the file is written
//                            after the join.
//   GCN_REPORT=<file>        after the test line, the TEST split is evaluated per class (ModelQueries::evaluate: counts formed on the GPU) and
//                            a text report written: `class <c> support <n> precision <p> recall <r> f1 <f>` per class, a line
//                            `macro_f1 <x> micro_f1 <y>`, and for a single-label model a line `confusion` followed by the matrix
//                            (row = truth, column = prediction) as C lines of C integers.  With several GPUs every worker takes
//                            part, all receive the same totals, and the file is written once after the join.
//   GCN_SMOOTH=cs|lp        after the test line, the predictions are post-processed with the graph and the training labels on the GPU
//                            (ModelQueries::correct_and_smooth / label_propagation at their default settings: alpha 0.8 / 50 iterations
//                            each for cs, alpha 0.9 / 50 iterations for lp) and one more line is printed:
//                            `smoothed_test_acc=<share of the test split whose smoothed class is its label>`.  GCN_PREDICT then
//                            writes the smoothed classes, one line `node class` per node.  One GPU, single-label.
//   GCN_CALIBRATE=<file>     directly after the test line (before GCN_REPORT / GCN_SMOOTH / GCN_PREDICT, which then see the temperature):
//                            one scalar temperature T is fitted on the VALIDATION split by minimising the negative log-likelihood of
//                            softmax(z / T) (ModelQueries::calibrate), set on the model, and one line is printed:
//                            `temperature=<T> val_nll_before=<x> val_nll_after=<y> test_ece_before=<a> test_ece_after=<b>` (ECE: expected
//                            calibration error of the TEST split, 15 bins).  The file gets the test split's reliability table at
//                            T = 1 and at the fitted T (host/calibration.h: a summary line, then one line per bin).  Works with
//                            GCN_LOAD_WEIGHTS and 0 epochs.  One GPU, single-label, at most 64 classes.
//   GCN_UNCERTAINTY=<file>   after the test line and after GCN_CALIBRATE's fit (at its temperature), before every other step: Monte Carlo
//                            dropout on the TEST split (ModelQueries::mc_dropout; csrc/mcdropout.hip has the definition) — GCN_MC_SAMPLES
//                            (default 20, 1..1024) forwards with the model's dropout on, seeded by GCN_MC_SEED (a 64-bit integer;
//                            default: the model's seed ^ KEY_MC_DROPOUT).  One line is printed: `mc_samples=<S> mc_test_acc=<share of
//                            the test nodes whose mean-softmax class is their label> mc_mean_entropy=<x> mc_mean_mutual_information=<y>`.
//                            The file gets one line per test node in id order: `node pred confidence entropy mutual_information`
//                            (%.9g).  stdout is otherwise unchanged.  Works with GCN_LOAD_WEIGHTS and 0 epochs.  One GPU, single-label,
//                            at most 64 classes, f32 tables, hidden_dim at most 256.
//   GCN_CONFORMAL=<file>     after the test line (and after GCN_CALIBRATE's fit when both are set, at its temperature): split conformal
//                            prediction sets (ModelQueries::conformal_fit / conformal_sets).  The threshold is fitted on the
//                            VALIDATION split at GCN_CONFORMAL_ALPHA (default 0.1) with GCN_CONFORMAL_METHOD=aps|lac (default aps) and
//                            GCN_CONFORMAL_DIFFUSION=<d in [0, 1]> (default 0: the scores are not blended with their neighbours'), and
//                            one line is printed: `conformal_alpha=<a> threshold=<q> cal_rows=<n> test_coverage=<share of the labelled
//                            test nodes whose set holds their label> test_mean_set_size=<s> test_empty=<n>`.  The file gets one line
//                            per node of the TEST split in id order: `node size c1,c2,...`.  One GPU, single-label, at most 64 classes.
//   GCN_RANKING=<file>       after the test line (and after GCN_CALIBRATE's fit when both are set, at its temperature): per-class ROC-AUC
//                            and average precision of the TEST split without a decision threshold (ModelQueries::ranking: keys, a
//                            segmented sort and binary searches on the GPU; host/ranking.h derives the metrics).  The file gets one line
//                            per class, `class <c> pos <P> neg <N> auc <a> ap <p>` with `undefined` in place of a value the class does
//                            not have (no positive, or no negative), then `macro_auc <x> macro_ap <y> weighted_auc <u> weighted_ap <v>
//                            classes <k>` (the means over the defined classes).  stdout and the GCN_REPORT file are unchanged.  One GPU;
//                            at most 64 classes, or 256 on a multi-label model (scored on its logits).
//   GCN_THRESHOLDS=<file>    after the test line (and GCN_RANKING): one decision threshold per class of a multi-label model, fitted on
//                            the VALIDATION split for the largest F-beta, GCN_THRESHOLDS_BETA (default 1), on the GPU
//                            (ModelQueries::tune_thresholds; csrc/thresholds.hip has the rule), and written to the file (host/thresholds.h:
//                            one line per class, `<threshold> # class c pos P neg N tp .. fp .. fn .. f ..`).  One line is printed:
//                            `thresholds_beta=<b> val_macro_f1_default=<x> val_macro_f1_tuned=<y> test_micro_f1_default=<a>
//                            test_micro_f1_tuned=<b> test_macro_f1_default=<c> test_macro_f1_tuned=<d>` (default: the rule logit > 0).
//                            GCN_PREDICT and GCN_REPORT then decide by the tuned cuts (logit >= threshold).
//   GCN_APPLY_THRESHOLDS=<file>  the cuts are read from such a file (checked before the GPU is touched) instead of fitted — for
//                            GCN_LOAD_WEIGHTS runs with 0 epochs; the line printed is `test_micro_f1_default=.. test_micro_f1_tuned=..
//                            test_macro_f1_default=.. test_macro_f1_tuned=..`.  Both need GCN_MULTILABEL, one GPU and at most 256 classes,
//                            and exclude each other.
// Unseen nodes (beyond the reference; ModelQueries::predict_new, host/attach.h, csrc/attach.hip), after the test line and every
// step above (at GCN_CALIBRATE's temperature, by GCN_THRESHOLDS' cuts); stdout is unchanged.  One GPU, f32 tables, hidden_dim at most 256:
//   GCN_NEW_NODES=<stem>     <stem>.graph and <stem>.svmlight in the dataset's own text format, read with its parser and checked before
//                            the GPU is touched: line i is new node N + i (N = the dataset's nodes), the ids it lists are in
//                            [0, N + lines) — a dataset node, or another new node of the same files — its stored row is itself first,
//                            then those ids, and no existing row changes.  The label column of the .svmlight file is read and ignored.
//   GCN_NEW_PREDICT=<file>   the new nodes' predictions in GCN_PREDICT's line format, node ids N + i.  Works with GCN_LOAD_WEIGHTS
//                            and 0 epochs: the dataset, its adjacency object and schedule are built once, not again per batch of nodes.
// Node embeddings (beyond the reference; ModelQueries::embed / similar, kernels in csrc/embed.hip), after the test line and every
// post-processing step above; stdout is unchanged.  One GPU, hidden_dim at most 256; single- and multi-label models alike:
//   GCN_EMBED=<file>         one line per node of the dataset in id order: `node v1 ... vh`, the node's row of the hidden layer
//                            H1 = ReLU(A^.X.W1) of an evaluation forward with the final (or loaded) weights, %.9g (exact f32).
//   GCN_SIMILAR=<file>       one line per node: `node id:score ...`, its 10 nearest nodes by the cosine of those rows (best
//                            first, equal scores by ascending id, the node itself left out), found on the GPU.
// Clustering (beyond the reference; ModelQueries::kmeans, kernels in csrc/kmeans.hip), after the test line and the steps above.
// One GPU, hidden_dim at most 256, f32 tables, a single-label model:
//   GCN_CLUSTER=<file>       k-means on the unit rows of the hidden layer of EVERY node: GCN_CLUSTER_K clusters (default: the
//                            number of classes, 1..256), at most GCN_CLUSTER_ITERS iterations (default 100), k-means++ seeding
//                            on GCN_CLUSTER_SEED (a 64-bit integer; default: the model's seed).  One line is printed:
//                            `clusters=<k> cluster_iters=<n> cluster_inertia=<x> cluster_nmi=<a> cluster_ari=<b> cluster_purity=<c>`,
//                            the last three of the TEST split's nodes against their labels (host/kmeans.h).  The file gets one
//                            line per node in id order: `node cluster dist2` (%.9g).  Works with GCN_LOAD_WEIGHTS and 0 epochs.
//   GCN_CLUSTER_SILHOUETTE=<file>  with GCN_CLUSTER (refused without it): the silhouette widths of that clustering over every
//                            node (ModelQueries::silhouette, kernels in csrc/silhouette.hip).  One further line is printed:
//                            `silhouette=<score> silhouette_min_cluster=<lowest cluster mean> silhouette_negative=<share of
//                            points with s < 0>`.  The file gets one line per node in id order: `node cluster s neighbor` (%.9g).
// Label structure (beyond the reference; ModelQueries::structure, kernels in csrc/structure.hip, measures in host/structure.h),
// after the test line and the steps above.  One GPU, a single-label model with at most 64 classes:
//   GCN_STRUCTURE=<file>     homophily of the graph and of the model's predictions over the nodes of the TEST split, and the
//                            accuracy by degree and by neighbourhood agreement in GCN_STRUCTURE_BINS agreement buckets (default
//                            10, 1..32).  One line is printed: `edge_homophily=<a> node_homophily=<b> adjusted_homophily=<c>
//                            class_insensitive_homophily=<d> pred_edge_homophily=<e>` (the first four of the labels, the last of
//                            the predicted classes).  The file gets the two strata tables, both mixing matrices and the integers
//                            they come from (host/structure.h).  Works with GCN_LOAD_WEIGHTS and 0 epochs.
// Reach of the labels (beyond the reference; ModelQueries::reach, kernels in csrc/reach.hip, measures in host/reach.h), after the
// test line and the steps above.  One GPU, a single-label model:
//   GCN_REACH=<file>         how far the nodes of the TEST split are from the TRAINING split's labels (hops along the stored rows,
//                            breadth-first on the GPU), the weak components of the graph, and the accuracy by that distance in
//                            GCN_REACH_HOPS exact distances (default 8, 1..32).  One line is printed: `reach_sources=<n>
//                            reach_levels=<n> reach_unreachable=<n> reach_outside_two_hops=<n> acc_inside_two_hops=<a>
//                            acc_outside_two_hops=<b> nearest_label_acc=<c> components=<n> largest_component=<n>
//                            unseeded_components=<n> unseeded_nodes=<n>` ("two hops" is min(2, GCN_REACH_HOPS - 1)).  The file
//                            gets the per-distance table, the totals and the integers they come from (host/reach.h).  Works with
//                            GCN_LOAD_WEIGHTS and 0 epochs.
// Explanations (beyond the reference; ModelQueries::explain / feature_importance, kernels in csrc/explain.hip), after the test line
// and the steps above; stdout is unchanged.  One GPU, hidden_dim at most 256, f32 tables; single- and multi-label models alike:
//   GCN_EXPLAIN=<file>       one line per node of the TEST split in id order: `node class logit | id:share x5 | f:share x5` — the
//                            class with the node's highest logit, that logit, and the five largest shares of it by neighbour (node
//                            ids, the self loop among them) and by input feature column, largest first, ties by ascending id or
//                            column (%.9g); then one line per class, `class c nodes=<n> | f:mean x10`: the ten columns with the
//                            largest mean |share| over the test nodes explained for that class.
// Principal components (beyond the reference; ModelQueries::pca_fit, sums in csrc/pca.hip, the eigenproblem in host/pca.h), after
// the test line and every step above.  One GPU, hidden_dim at most 256, f32 tables; single- and multi-label models alike:
//   GCN_PCA=<file>           principal component analysis of the unit rows of the hidden layer of EVERY node (centred): the
//                            float64 mean and scatter matrix on the GPU, the eigenproblem on the host, the projection onto the
//                            leading GCN_PCA_K components (default 2, 1..hidden_dim) on the GPU.  One line is printed:
//                            `pca_components=<k> pca_rows=<n> pca_rank=<r> pca_explained_variance_ratio=<a>,<b>,...` (k values,
//                            %.6f).  The file gets one line per node in id order: `node y1 ... yk` (%.9g).  Works with
//                            GCN_LOAD_WEIGHTS and 0 epochs.
// Multi-label training (beyond the reference):
//   GCN_MULTILABEL=<file>    the truth is the label file (host/labels.h: one line per node, comma-separated class ids), read and
//                            checked before the GPU is touched; output_dim = its number of classes (largest id + 1).  The loss is
//                            the per-class sigmoid cross-entropy; the lines carry train_f1= / val_f1= / test_f1= (micro-F1) in
//                            place of the _acc fields.  GCN_PREDICT then writes `node c1,c2,...` per node (the classes whose
//                            logit is above 0; the node alone for an empty set).
// Class-weighted loss (beyond the reference; host/class_weights.h):
//   GCN_CLASS_WEIGHTS=balanced|<file>  a weight per class in the loss, read and checked before the GPU is touched.  `balanced`:
//                            from the training split (single-label n / (C n_c); with GCN_MULTILABEL the positive-term weight
//                            (n - pos_c) / pos_c).  <file>: one float per line, one line per class.  The lines keep their
//                            format; the loss columns are the weighted loss.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <iostream>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>
#include "calibration.h"
#include "queries.h"
#include "class_weights.h"
#include "gcn.h"
#include "hip_check.h"
#include "kmeans.h"
#include "labels.h"
#include "parser.h"
#include "ranking.h"
#include "structure.h"
#include "reach.h"
#include "report.h"
#include "thresholds.h"

static int env_int(const char *name, int dflt) {
    const char *s = getenv(name);
    return s ? atoi(s) : dflt;
}

static constexpr size_t LANE_MIN_NODES = 8192;

int main(int argc, char **argv) {
    setbuf(stdout, NULL);
    if (argc < 2) {
        std::cout << "gcn-hip graph_name [num_nodes input_dim hidden_dim "
                     "output_dim dropout learning_rate, weight_decay epochs early_stopping]" << std::endl;
        return EXIT_FAILURE;
    }
    GCNParams params = GCNParams::get_default();
    GCNData data;
    std::string input_name(argv[1]);
    Parser parser(&params, &data, input_name);
    const auto t_load0 = std::chrono::steady_clock::now();
    if (!parser.parse()) {
        std::cerr << "Cannot read input: " << input_name << std::endl;
        exit(EXIT_FAILURE);
    }
    const double load_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_load0).count();
    // GCN_WRITE_CACHE=1: a dataset that was parsed from the three text files leaves data/<name>.gcnbin behind, so the next
    // run loads it in a fraction of the time (Reddit's text form is gigabytes of `k:v` tokens)
    if (env_int("GCN_WRITE_CACHE", 0) && !parser.from_cache()) {
        if (Parser::save_binary(parser.cache_path(), params, data)) std::cerr << "gcn-hip: wrote " << parser.cache_path() << std::endl;
        else std::cerr << "gcn-hip: could not write " << parser.cache_path() << std::endl;
    }
#define ARG(i) (argc > (i) && strcmp(argv[i], "-") != 0)
    if (ARG(4)) params.hidden_dim = atoi(argv[4]);
    if (ARG(6)) params.dropout = (float)atof(argv[6]);
    if (ARG(7)) params.learning_rate = (float)atof(argv[7]);
    if (ARG(8)) params.weight_decay = (float)atof(argv[8]);
    if (ARG(9)) params.epochs = atoi(argv[9]);
    if (ARG(10)) params.early_stopping = atoi(argv[10]);
    const char *multilabel_path = getenv("GCN_MULTILABEL");
    if (multilabel_path && !*multilabel_path) multilabel_path = nullptr;
    if (multilabel_path) {
        int n = params.num_nodes, c = 0;
        std::string err;
        if (gcn_labels_read(multilabel_path, &n, &c, data.multihot, &err) != 0) {
            std::cerr << "gcn-hip: GCN_MULTILABEL: " << err << std::endl;
            return EXIT_FAILURE;
        }
        if (c > 256) {
            std::cerr << "gcn-hip: GCN_MULTILABEL: " << c << " classes; multi-label mode takes at most 256" << std::endl;
            return EXIT_FAILURE;
        }
        params.output_dim = c;
    }

    std::vector<float> class_weights;
    const char *cw_spec = getenv("GCN_CLASS_WEIGHTS");
    if (cw_spec && *cw_spec) {
        std::string err;
        int bad = 0;
        if (strcmp(cw_spec, "balanced") == 0) {
            class_weights.resize(params.output_dim);
            bad = gcn_balanced_class_weights(params.num_nodes, params.output_dim, data.split.data(), data.label.data(),
                                             multilabel_path ? data.multihot.data() : nullptr, 1, class_weights.data(), &err);
        } else {
            bad = gcn_class_weights_read(cw_spec, params.output_dim, class_weights, &err);
        }
        if (bad) {
            std::cerr << "gcn-hip: GCN_CLASS_WEIGHTS: " << err << std::endl;
            return EXIT_FAILURE;
        }
        if (params.output_dim > 256) {
            std::cerr << "gcn-hip: GCN_CLASS_WEIGHTS: " << params.output_dim << " classes; class weights take at most 256" << std::endl;
            return EXIT_FAILURE;
        }
    }

    const char *smooth = getenv("GCN_SMOOTH");
    if (smooth && !*smooth) smooth = nullptr;
    if (smooth) {
        const char *why = strcmp(smooth, "cs") != 0 && strcmp(smooth, "lp") != 0 ? "is cs (Correct & Smooth) or lp (label propagation)"
                          : multilabel_path                                       ? "post-processes a single-label model (GCN_MULTILABEL is set)"
                          : env_int("GCN_GPUS", 1) > 1                            ? "runs on one GPU (GCN_GPUS is above 1)"
                          : params.output_dim > 64                                ? "takes at most 64 classes"
                                                                                  : nullptr;
        if (why) {
            std::cerr << "gcn-hip: GCN_SMOOTH " << why << std::endl;
            return EXIT_FAILURE;
        }
    }

    const char *calibrate_path = getenv("GCN_CALIBRATE");
    if (calibrate_path && !*calibrate_path) calibrate_path = nullptr;
    if (calibrate_path) {
        const char *why = multilabel_path              ? "fits the temperature of a single-label model (GCN_MULTILABEL is set)"
                          : env_int("GCN_GPUS", 1) > 1 ? "runs on one GPU (GCN_GPUS is above 1)"
                          : params.output_dim > 64     ? "takes at most 64 classes"
                                                       : nullptr;
        if (why) {
            std::cerr << "gcn-hip: GCN_CALIBRATE " << why << std::endl;
            return EXIT_FAILURE;
        }
    }

    const char *uncertainty_path = getenv("GCN_UNCERTAINTY");
    if (uncertainty_path && !*uncertainty_path) uncertainty_path = nullptr;
    const int mc_samples = env_int("GCN_MC_SAMPLES", 20);
    uint64_t mc_seed = 0;
    const char *mc_seed_text = getenv("GCN_MC_SEED");
    if (mc_seed_text && !*mc_seed_text) mc_seed_text = nullptr;
    if (uncertainty_path) {
        char *end = nullptr;
        if (mc_seed_text) mc_seed = strtoull(mc_seed_text, &end, 0);
        const char *why = multilabel_path                                  ? "samples the softmax of a single-label model (GCN_MULTILABEL is set)"
                          : env_int("GCN_GPUS", 1) > 1                     ? "runs on one GPU (GCN_GPUS is above 1)"
                          : params.output_dim > 64                         ? "takes at most 64 classes"
                          : params.hidden_dim > 256                        ? "takes a hidden_dim of at most 256"
                          : env_int("GCN_BF16_TABLES", 0)                  ? "needs f32 tables (GCN_BF16_TABLES is set)"
                          : mc_samples < 1 || mc_samples > ModelQueries::MC_SAMPLES_MAX ? "needs GCN_MC_SAMPLES in 1..1024"
                          : mc_seed_text && (end == mc_seed_text || *end)  ? "needs an integer GCN_MC_SEED"
                                                                           : nullptr;
        if (why) {
            std::cerr << "gcn-hip: GCN_UNCERTAINTY " << why << std::endl;
            return EXIT_FAILURE;
        }
    }

    const char *conformal_path = getenv("GCN_CONFORMAL");
    if (conformal_path && !*conformal_path) conformal_path = nullptr;
    double conformal_alpha = 0.1;
    int conformal_method = ModelQueries::CONFORMAL_APS;
    float conformal_diffusion = 0.f;
    if (conformal_path) {
        const char *a = getenv("GCN_CONFORMAL_ALPHA"), *meth = getenv("GCN_CONFORMAL_METHOD"), *d = getenv("GCN_CONFORMAL_DIFFUSION");
        if (a && *a) conformal_alpha = atof(a);
        if (d && *d) conformal_diffusion = (float)atof(d);
        const bool lac = meth && strcmp(meth, "lac") == 0;
        if (lac) conformal_method = ModelQueries::CONFORMAL_LAC;
        const char *why = multilabel_path                                          ? "builds the sets of a single-label model (GCN_MULTILABEL is set)"
                          : env_int("GCN_GPUS", 1) > 1                             ? "runs on one GPU (GCN_GPUS is above 1)"
                          : params.output_dim > 64                                 ? "takes at most 64 classes"
                          : !(conformal_alpha > 0.0 && conformal_alpha < 1.0)      ? "needs GCN_CONFORMAL_ALPHA in (0, 1)"
                          : meth && *meth && !lac && strcmp(meth, "aps") != 0      ? "needs GCN_CONFORMAL_METHOD=aps or lac"
                          : !(conformal_diffusion >= 0.f && conformal_diffusion <= 1.f) ? "needs GCN_CONFORMAL_DIFFUSION in [0, 1]"
                                                                                   : nullptr;
        if (why) {
            std::cerr << "gcn-hip: GCN_CONFORMAL " << why << std::endl;
            return EXIT_FAILURE;
        }
    }

    const char *ranking_path = getenv("GCN_RANKING");
    if (ranking_path && !*ranking_path) ranking_path = nullptr;
    if (ranking_path) {
        const char *why = env_int("GCN_GPUS", 1) > 1                              ? "runs on one GPU (GCN_GPUS is above 1)"
                          : params.output_dim > (multilabel_path ? 256 : 64)      ? "takes at most 64 classes (256 on a multi-label model)"
                                                                                  : nullptr;
        if (why) {
            std::cerr << "gcn-hip: GCN_RANKING " << why << std::endl;
            return EXIT_FAILURE;
        }
    }

    const char *thresholds_path = getenv("GCN_THRESHOLDS"), *apply_thresholds_path = getenv("GCN_APPLY_THRESHOLDS");
    if (thresholds_path && !*thresholds_path) thresholds_path = nullptr;
    if (apply_thresholds_path && !*apply_thresholds_path) apply_thresholds_path = nullptr;
    double thresholds_beta = 1.0;
    std::vector<float> cuts;                                   // one per class once read or fitted; empty: the rule logit > 0
    if (thresholds_path || apply_thresholds_path) {
        const char *b = getenv("GCN_THRESHOLDS_BETA");
        if (b && *b) thresholds_beta = atof(b);
        const char *why = !multilabel_path                                  ? "need GCN_MULTILABEL (a cut per class of a multi-label model)"
                          : env_int("GCN_GPUS", 1) > 1                       ? "run on one GPU (GCN_GPUS is above 1)"
                          : params.output_dim > 256                          ? "take at most 256 classes"
                          : thresholds_path && apply_thresholds_path         ? "exclude each other: fit the cuts or read them"
                          : !(thresholds_beta > 0.0 && thresholds_beta < 1e300) ? "need GCN_THRESHOLDS_BETA finite and > 0"
                                                                             : nullptr;
        if (why) {
            std::cerr << "gcn-hip: GCN_THRESHOLDS / GCN_APPLY_THRESHOLDS " << why << std::endl;
            return EXIT_FAILURE;
        }
        std::string err;
        if (apply_thresholds_path && gcn_thresholds_read(apply_thresholds_path, params.output_dim, cuts, &err) != 0) {
            std::cerr << "gcn-hip: GCN_APPLY_THRESHOLDS: " << err << std::endl;
            return EXIT_FAILURE;
        }
    }

    const char *embed_path = getenv("GCN_EMBED"), *similar_path = getenv("GCN_SIMILAR");
    if (embed_path && !*embed_path) embed_path = nullptr;
    if (similar_path && !*similar_path) similar_path = nullptr;
    if (embed_path || similar_path) {
        const char *why = env_int("GCN_GPUS", 1) > 1 ? "run on one GPU (GCN_GPUS is above 1)"
                          : params.hidden_dim > 256  ? "take a hidden width of at most 256"
                                                     : nullptr;
        if (why) {
            std::cerr << "gcn-hip: GCN_EMBED / GCN_SIMILAR " << why << std::endl;
            return EXIT_FAILURE;
        }
    }

    const char *cluster_path = getenv("GCN_CLUSTER");
    if (cluster_path && !*cluster_path) cluster_path = nullptr;
    const int cluster_k = env_int("GCN_CLUSTER_K", params.output_dim), cluster_iters = env_int("GCN_CLUSTER_ITERS", 100);
    uint64_t cluster_seed = 0;
    const char *cluster_seed_text = getenv("GCN_CLUSTER_SEED");
    if (cluster_seed_text && !*cluster_seed_text) cluster_seed_text = nullptr;
    if (cluster_path) {
        char *end = nullptr;
        if (cluster_seed_text) cluster_seed = strtoull(cluster_seed_text, &end, 0);
        const char *why = multilabel_path                                          ? "scores the clusters against single labels (GCN_MULTILABEL is set)"
                          : env_int("GCN_GPUS", 1) > 1                             ? "runs on one GPU (GCN_GPUS is above 1)"
                          : params.hidden_dim > 256                                ? "takes a hidden width of at most 256"
                          : env_int("GCN_BF16_TABLES", 0)                          ? "needs f32 tables (GCN_BF16_TABLES is set)"
                          : cluster_k < 1 || cluster_k > 256 || cluster_k > params.num_nodes ? "needs GCN_CLUSTER_K in 1..256 and at most the number of nodes"
                          : cluster_iters < 1                                      ? "needs GCN_CLUSTER_ITERS of at least 1"
                          : cluster_seed_text && (end == cluster_seed_text || *end) ? "needs an integer GCN_CLUSTER_SEED"
                                                                                   : nullptr;
        if (why) {
            std::cerr << "gcn-hip: GCN_CLUSTER " << why << std::endl;
            return EXIT_FAILURE;
        }
    }
    const char *silhouette_path = getenv("GCN_CLUSTER_SILHOUETTE");
    if (silhouette_path && !*silhouette_path) silhouette_path = nullptr;
    if (silhouette_path && !cluster_path) {
        std::cerr << "gcn-hip: GCN_CLUSTER_SILHOUETTE needs GCN_CLUSTER (it measures the clustering that makes)" << std::endl;
        return EXIT_FAILURE;
    }

    const char *pca_path = getenv("GCN_PCA");
    if (pca_path && !*pca_path) pca_path = nullptr;
    const int pca_k = env_int("GCN_PCA_K", 2);
    if (pca_path) {
        const char *why = env_int("GCN_GPUS", 1) > 1                 ? "runs on one GPU (GCN_GPUS is above 1)"
                          : params.hidden_dim > 256                  ? "takes a hidden width of at most 256"
                          : env_int("GCN_BF16_TABLES", 0)            ? "needs f32 tables (GCN_BF16_TABLES is set)"
                          : pca_k < 1 || pca_k > params.hidden_dim   ? "needs GCN_PCA_K in 1..hidden_dim"
                          : params.num_nodes < 2                     ? "needs at least 2 nodes"
                                                                     : nullptr;
        if (why) {
            std::cerr << "gcn-hip: GCN_PCA " << why << std::endl;
            return EXIT_FAILURE;
        }
    }

    const char *structure_path = getenv("GCN_STRUCTURE");
    if (structure_path && !*structure_path) structure_path = nullptr;
    const int structure_bins = env_int("GCN_STRUCTURE_BINS", 10);
    if (structure_path) {
        const char *why = multilabel_path                                        ? "compares one predicted class per node (GCN_MULTILABEL is set)"
                          : env_int("GCN_GPUS", 1) > 1                           ? "runs on one GPU (GCN_GPUS is above 1)"
                          : params.output_dim > STRUCTURE_MAX_CLASSES            ? "takes at most 64 classes"
                          : structure_bins < 1 || structure_bins > STRUCTURE_MAX_BINS ? "needs GCN_STRUCTURE_BINS in 1..32"
                                                                                 : nullptr;
        if (why) {
            std::cerr << "gcn-hip: GCN_STRUCTURE " << why << std::endl;
            return EXIT_FAILURE;
        }
    }

    const char *reach_path = getenv("GCN_REACH");
    if (reach_path && !*reach_path) reach_path = nullptr;
    const int reach_hops = env_int("GCN_REACH_HOPS", 8);
    if (reach_path) {
        const char *why = multilabel_path                                  ? "compares one predicted class per node (GCN_MULTILABEL is set)"
                          : env_int("GCN_GPUS", 1) > 1                     ? "runs on one GPU (GCN_GPUS is above 1)"
                          : reach_hops < 1 || reach_hops > REACH_MAX_HOPS  ? "needs GCN_REACH_HOPS in 1..32"
                                                                           : nullptr;
        if (why) {
            std::cerr << "gcn-hip: GCN_REACH " << why << std::endl;
            return EXIT_FAILURE;
        }
    }

    const char *explain_path = getenv("GCN_EXPLAIN");
    if (explain_path && !*explain_path) explain_path = nullptr;
    if (explain_path) {
        const char *why = env_int("GCN_GPUS", 1) > 1      ? "runs on one GPU (GCN_GPUS is above 1)"
                          : params.hidden_dim > 256        ? "takes a hidden width of at most 256"
                          : env_int("GCN_BF16_TABLES", 0) ? "does not go with GCN_BF16_TABLES"
                                                           : nullptr;
        if (why) {
            std::cerr << "gcn-hip: GCN_EXPLAIN " << why << std::endl;
            return EXIT_FAILURE;
        }
    }

    // new nodes: read with the dataset's own text parser and checked before the GPU is touched
    const char *new_nodes_stem = getenv("GCN_NEW_NODES"), *new_predict_path = getenv("GCN_NEW_PREDICT");
    if (new_nodes_stem && !*new_nodes_stem) new_nodes_stem = nullptr;
    if (new_predict_path && !*new_predict_path) new_predict_path = nullptr;
    GCNData new_nodes;
    std::vector<int64_t> new_nbr_ptr;
    std::vector<int> new_nbr_ids;
    int n_new = 0;
    if (new_nodes_stem || new_predict_path) {
        GCNParams np = params;
        std::string why;
        if (!new_nodes_stem || !new_predict_path) why = "GCN_NEW_NODES=<stem> and GCN_NEW_PREDICT=<file> go together";
        else if (env_int("GCN_GPUS", 1) > 1) why = "runs on one GPU (GCN_GPUS is above 1)";
        else if (env_int("GCN_BF16_TABLES", 0)) why = "does not go with GCN_BF16_TABLES";
        else if (params.hidden_dim > 256) why = "takes a hidden width of at most 256";
        else if (!Parser::parse_rows(new_nodes_stem, &np, &new_nodes)) why = std::string("cannot read ") + new_nodes_stem + ".graph and " + new_nodes_stem + ".svmlight (one line per new node in both)";
        else if (new_nodes.feature_index.indptr.back() > 0 && np.input_dim > params.input_dim)
            why = "a feature column " + std::to_string(np.input_dim - 1) + " is outside the dataset's input width " + std::to_string(params.input_dim);
        if (!why.empty()) {
            std::cerr << "gcn-hip: GCN_NEW_NODES " << why << std::endl;
            return EXIT_FAILURE;
        }
        n_new = np.num_nodes;
        // line i of the .graph file lists the ids of new node N + i; the parser's implicit first entry is not one of them
        new_nbr_ptr.assign(1, 0);
        for (int i = 0; i < n_new; i++) {
            const std::vector<int> &gp = new_nodes.graph.indptr, &gi = new_nodes.graph.indices;
            new_nbr_ids.insert(new_nbr_ids.end(), gi.begin() + gp[i] + 1, gi.begin() + gp[i + 1]);
            new_nbr_ptr.push_back((int64_t)new_nbr_ids.size());
        }
    }

    int n_dev = 0;
    if (gcnhip_device_count(&n_dev) != 0 || n_dev < 1) {
        std::cerr << "gcn-hip: no GPU available (this backend has no CPU path; use gcn-seq)" << std::endl;
        return EXIT_FAILURE;
    }
    const int world = env_int("GCN_GPUS", 1);
    if (world > n_dev) {
        std::cerr << "gcn-hip: GCN_GPUS=" << world << " but only " << n_dev << " visible" << std::endl;
        return EXIT_FAILURE;
    }
    HipGCNOptions base;
    const char *seed = getenv("GCN_SEED");
    base.seed = seed ? atol(seed) : (long)time(NULL);
    base.flags = (env_int("GCN_MODULAR", 0) ? HIPGCN_MODULAR : 0) | (env_int("GCN_HOST_MASKS", 0) ? HIPGCN_HOST_MASKS : 0) |
                 (env_int("GCN_TIMERS", 0) ? HIPGCN_TIMERS : 0) | (env_int("GCN_BF16_TABLES", 0) ? HIPGCN_BF16_TABLES : 0) |
                 (env_int("GCN_OVERLAP", 0) ? HIPGCN_OVERLAP_EXCHANGE : 0);
    const bool feedback = params.early_stopping > 0;          // see the header: printed numbers decide the run
    // validation lane: on one GPU unless early stopping serialises the epochs anyway; with several GPUs it brings a second
    // communicator and stays opt-in until measured on such a node
    if (env_int("GCN_EVAL_LANE", (world == 1 && !feedback && data.graph.indptr.size() > LANE_MIN_NODES) ? 1 : 0)) base.flags |= HIPGCN_EVAL_LANE;
    else base.flags |= HIPGCN_NO_EVAL_LANE;
    if (env_int("GCN_REFERENCE_ORDER", feedback ? 1 : 0)) base.flags |= HIPGCN_NO_AGG_FIRST_EVAL;
    if (env_int("GCN_SYNC_EPOCHS", 0)) base.flags |= HIPGCN_SYNC_EPOCHS;
    base = HipGCNOptions::from_environment(base);             // every HIPGCN_* variable, read once (host/options.cpp)
    base.multilabel = multilabel_path != nullptr;
    base.class_weights = class_weights;
    std::cout << "RUNNING ON GPU" << std::endl;

    int rc = EXIT_SUCCESS;
    const char *load_path = getenv("GCN_LOAD_WEIGHTS"), *save_path = getenv("GCN_SAVE_WEIGHTS"), *predict_path = getenv("GCN_PREDICT");
    if (load_path && !*load_path) load_path = nullptr;
    if (save_path && !*save_path) save_path = nullptr;
    if (predict_path && !*predict_path) predict_path = nullptr;
    const char *report_path = getenv("GCN_REPORT");
    if (report_path && !*report_path) report_path = nullptr;
    const int C_out = params.output_dim;
    std::vector<int64_t> report_counts(report_path ? (size_t)(multilabel_path ? 3 * C_out : C_out * C_out) : 0, 0);   // rank 0's copy of the totals
    std::vector<int32_t> all_pred(predict_path ? params.num_nodes : 0, -1);   // by node id, filled by the workers
    std::vector<float> all_prob(predict_path ? params.num_nodes : 0, 0.f);
    const int ml_wpr = gcn_label_words(params.output_dim);
    std::vector<uint32_t> all_bits(predict_path && multilabel_path ? (size_t)params.num_nodes * ml_wpr : 0, 0u);
    auto worker = [&](int rank, const char *id) {
        try {
            HipGCNOptions o = base;
            o.device = rank; o.rank = rank; o.world = world; o.nccl_id = id;
            const auto t_build0 = std::chrono::steady_clock::now();
            HipGCN gcn(params, &data, o);
            if (rank == 0)      // stderr: stdout stays the reference's lines (src/seq/gcn.cpp:133-158)
                fprintf(stderr, "gcn-hip: dataset loaded in %.3f s, model built in %.3f s (host preparation + every H2D copy)\n", load_s,
                        std::chrono::duration<double>(std::chrono::steady_clock::now() - t_build0).count());
            if (load_path) {
                gcn.load_weights(load_path);
                if (rank == 0) fprintf(stderr, "gcn-hip: weights loaded from %s\n", load_path);
            }
            gcn.run();
            if (save_path && rank == 0) {
                gcn.save_weights(save_path);
                fprintf(stderr, "gcn-hip: weights written to %s\n", save_path);
            }
            if (calibrate_path) {                              // one rank (checked above)
                constexpr int BINS = 15;
                const ModelQueries::Calibrated fit = gcn.queries().calibrate(2, 0, nullptr, nullptr, nullptr);
                double sums[2][4], conf[2][BINS];
                int64_t count[2][BINS], correct[2][BINS];
                CalibrationReport rep[2];
                const float T[2] = {1.f, fit.temperature};
                std::string err;
                for (int k = 0; k < 2; k++) {
                    gcn.queries().calibration(3, nullptr, 0, T[k], BINS, sums[k], count[k], correct[k], conf[k]);
                    if (gcn_calibration_report(BINS, count[k], correct[k], conf[k], &rep[k], &err) != 0) throw GcnHipFailure(-1, err);
                }
                gcn.queries().set_temperature(fit.temperature);
                printf("temperature=%.5f val_nll_before=%.5f val_nll_after=%.5f test_ece_before=%.5f test_ece_after=%.5f\n", fit.temperature,
                       fit.nll_before, fit.nll_after, rep[0].ece, rep[1].ece);
                FILE *f = fopen(calibrate_path, "w");
                bool ok = f != nullptr;
                for (int k = 0; ok && k < 2; k++)
                    ok = gcn_calibration_table_write(f, T[k], sums[k][3] > 0 ? sums[k][0] / sums[k][3] : 0.0, BINS, count[k], rep[k]);
                if (f && fclose(f) != 0) ok = false;
                if (!ok) throw GcnHipFailure(-1, std::string("gcn-hip: could not write the reliability tables to ") + calibrate_path);
                fprintf(stderr, "gcn-hip: reliability tables of the test split written to %s%s\n", calibrate_path,
                        fit.at_bound ? " (the fit stopped on an end of its bracket: the validation split is classified perfectly)" : "");
            }
            if (uncertainty_path) {                            // one rank (checked above); after the calibration: at its temperature
                std::vector<int> test;
                test.reserve(1);                               // an empty split is still a query (not "every row")
                for (int i = 0; i < params.num_nodes; i++)
                    if (data.split[i] == 3) test.push_back(i);
                const size_t nt = test.size(), cap = std::max<size_t>(nt, 1);
                std::vector<int32_t> pred(cap);
                std::vector<float> conf(cap), ent(cap), mi(cap);
                const ModelQueries::McDropout r = gcn.queries().mc_dropout(0, test.data(), (int)nt, mc_samples, nullptr, mc_seed_text ? &mc_seed : nullptr, 0,
                                                                           pred.data(), conf.data(), ent.data(), nullptr, mi.data(), nullptr, nullptr, nullptr,
                                                                           nullptr);
                double right = 0, sum_ent = 0, sum_mi = 0;
                for (size_t i = 0; i < nt; i++) {
                    right += pred[i] == data.label[test[i]];
                    sum_ent += ent[i];
                    sum_mi += mi[i];
                }
                const double d = nt ? (double)nt : 1.0;
                printf("mc_samples=%d mc_test_acc=%.5f mc_mean_entropy=%.5f mc_mean_mutual_information=%.5f\n", r.samples, right / d, sum_ent / d, sum_mi / d);
                FILE *f = fopen(uncertainty_path, "w");
                bool ok = f != nullptr;
                for (size_t i = 0; ok && i < nt; i++) ok = fprintf(f, "%d %d %.9g %.9g %.9g\n", test[i], pred[i], conf[i], ent[i], mi[i]) > 0;
                if (f && fclose(f) != 0) ok = false;
                if (!ok) throw GcnHipFailure(-1, std::string("gcn-hip: could not write the uncertainties to ") + uncertainty_path);
                fprintf(stderr, "gcn-hip: Monte Carlo dropout (%d samples, p %g, seed %llu) of the test split written to %s\n", r.samples, r.p,
                        (unsigned long long)r.seed, uncertainty_path);
            }
            if (conformal_path) {                              // one rank (checked above); after the calibration: at its temperature
                const int C = params.output_dim, wpr = (C + 31) / 32;
                const ModelQueries::Conformal fit =
                    gcn.queries().conformal_fit(2, nullptr, 0, conformal_alpha, conformal_method, 0.f, 0, conformal_diffusion, false, nullptr);
                std::vector<int> test;
                test.reserve(1);                               // an empty split is still a query (not "every row")
                for (int i = 0; i < params.num_nodes; i++)
                    if (data.split[i] == 3) test.push_back(i);
                const size_t nt = test.size();
                std::vector<uint32_t> bits(std::max<size_t>(nt, 1) * wpr);
                std::vector<int32_t> size(std::max<size_t>(nt, 1));
                std::vector<int64_t> counts((size_t)(4 + 3 * C + 1));
                gcn.queries().conformal_sets(fit, 0, test.data(), (int)nt, bits.data(), size.data(), counts.data());
                int64_t total = 0;
                for (size_t i = 0; i < nt; i++) total += size[i];
                printf("conformal_alpha=%g threshold=%.6f cal_rows=%lld test_coverage=%.5f test_mean_set_size=%.4f test_empty=%lld\n", conformal_alpha,
                       fit.thresh[0], (long long)fit.n_cal[0], counts[1] ? (double)counts[2] / (double)counts[1] : 0.0,
                       nt ? (double)total / (double)nt : 0.0, (long long)counts[3]);
                FILE *f = fopen(conformal_path, "w");
                bool ok = f != nullptr;
                for (size_t i = 0; ok && i < nt; i++) {
                    ok = fprintf(f, "%d %d", test[i], size[i]) > 0;
                    bool first = true;
                    for (int c = 0; ok && c < C; c++)
                        if ((bits[i * wpr + (c >> 5)] >> (c & 31)) & 1u) {
                            ok = fprintf(f, "%s%d", first ? " " : ",", c) > 0;
                            first = false;
                        }
                    ok = ok && fputc('\n', f) != EOF;
                }
                if (f && fclose(f) != 0) ok = false;
                if (!ok) throw GcnHipFailure(-1, std::string("gcn-hip: could not write the prediction sets to ") + conformal_path);
                fprintf(stderr, "gcn-hip: conformal prediction sets of the test split written to %s\n", conformal_path);
            }
            if (ranking_path) {                                // one rank (checked above); after the calibration: at its temperature
                const int C = params.output_dim;
                std::vector<int64_t> u2(C), pos(C), neg(C), invalid(C);
                std::vector<double> ap_sum(C);
                int64_t unlabelled = 0;
                gcn.queries().ranking(3, nullptr, 0, 0, u2.data(), ap_sum.data(), pos.data(), neg.data(), invalid.data(), &unlabelled, nullptr);
                RankingReport rep;
                std::string err;
                if (gcn_ranking_report(C, u2.data(), ap_sum.data(), pos.data(), neg.data(), &rep, &err) != 0 ||
                    gcn_ranking_report_write(ranking_path, C, rep, pos.data(), neg.data(), &err) != 0)
                    throw GcnHipFailure(-1, "gcn-hip: GCN_RANKING: " + err);
                fprintf(stderr, "gcn-hip: ranking metrics of the test split (macro AUC %.5f, macro AP %.5f over %d classes) written to %s\n", rep.macro_auc,
                        rep.macro_ap, rep.classes_defined, ranking_path);
            }
            if (thresholds_path || apply_thresholds_path) {    // one rank, multi-label (checked above)
                const int C = params.output_dim;
                std::string err;
                // macro- and micro-F1 of a split by the rule logit > 0 (thr == NULL) or by the cuts, derived where every report is
                auto f1 = [&](int split, const float *thr, double *micro) {
                    std::vector<int64_t> cnt(3 * (size_t)C);
                    if (thr) gcn.queries().evaluate(split, nullptr, 0, thr, C, cnt.data(), nullptr);
                    else gcn.queries().evaluate(split, nullptr, 0, cnt.data(), nullptr, nullptr);
                    ClassReport r;
                    if (gcn_class_report(C, nullptr, cnt.data(), cnt.data() + C, cnt.data() + 2 * C, &r, &err) != 0) throw GcnHipFailure(-1, err);
                    if (micro) *micro = r.micro_f1;
                    return r.macro_f1;
                };
                if (thresholds_path) {
                    std::vector<int64_t> tp(C), fp(C), fn(C), pos(C), neg(C), invalid(C);
                    std::vector<double> f(C);
                    std::vector<int32_t> defined(C);
                    cuts.resize(C);
                    gcn.queries().tune_thresholds(2, nullptr, 0, thresholds_beta, 0, cuts.data(), tp.data(), fp.data(), fn.data(), f.data(), pos.data(),
                                                  neg.data(), invalid.data(), defined.data());
                    ThresholdFit fit;
                    fit.pos = pos.data(); fit.neg = neg.data(); fit.tp = tp.data(); fit.fp = fp.data(); fit.fn = fn.data(); fit.f = f.data();
                    if (gcn_thresholds_write(thresholds_path, C, cuts.data(), &fit, &err) != 0) throw GcnHipFailure(-1, "gcn-hip: GCN_THRESHOLDS: " + err);
                    const double val_default = f1(2, nullptr, nullptr), val_tuned = f1(2, cuts.data(), nullptr);
                    printf("thresholds_beta=%g val_macro_f1_default=%.5f val_macro_f1_tuned=%.5f ", thresholds_beta, val_default, val_tuned);
                    fprintf(stderr, "gcn-hip: decision thresholds of %d classes, fitted on the validation split, written to %s\n", C, thresholds_path);
                }
                double micro_default = 0, micro_tuned = 0;
                const double macro_default = f1(3, nullptr, &micro_default), macro_tuned = f1(3, cuts.data(), &micro_tuned);
                printf("test_micro_f1_default=%.5f test_micro_f1_tuned=%.5f test_macro_f1_default=%.5f test_macro_f1_tuned=%.5f\n", micro_default, micro_tuned,
                       macro_default, macro_tuned);
            }
            if (predict_path && multilabel_path) {             // the same, as class sets (by the cuts when there are any)
                const int n = gcn.local_rows();
                std::vector<uint32_t> b((size_t)std::max(n, 1) * ml_wpr);
                if (cuts.empty()) gcn.queries().predict_multilabel(nullptr, n, b.data(), nullptr);
                else gcn.queries().predict_multilabel(nullptr, n, cuts.data(), (int)cuts.size(), b.data(), nullptr);
                for (int r = 0; r < n; r++) {
                    const int id = gcn.node_id(r);
                    std::copy(b.begin() + (size_t)r * ml_wpr, b.begin() + (size_t)(r + 1) * ml_wpr, all_bits.begin() + (size_t)id * ml_wpr);
                }
            } else if (smooth) {                               // one rank (checked above): arrays by node id
                std::vector<int32_t> p(std::max(params.num_nodes, 1));
                if (strcmp(smooth, "cs") == 0) gcn.queries().correct_and_smooth(0.8f, 50, 0.8f, 50, 1 << 1, p.data(), nullptr);
                else gcn.queries().label_propagation(0.9f, 50, 1 << 1, p.data(), nullptr);
                long hit = 0, total = 0;
                for (int i = 0; i < params.num_nodes; i++)
                    if (data.split[i] == 3) { total++; hit += p[i] == data.label[i]; }
                printf("smoothed_test_acc=%.5f\n", total ? (double)hit / (double)total : 0.0);
                if (predict_path) std::copy(p.begin(), p.begin() + params.num_nodes, all_pred.begin());
            } else if (predict_path) {                         // every rank: the logit aggregation exchanges rows
                const int n = gcn.local_rows();
                std::vector<int32_t> p(std::max(n, 1));
                std::vector<float> q(std::max(n, 1));
                gcn.queries().predict(nullptr, n, p.data(), q.data(), nullptr);
                for (int r = 0; r < n; r++) {
                    const int id = gcn.node_id(r);
                    all_pred[id] = p[r];
                    all_prob[id] = q[r];
                }
            }
            if (report_path) {                                 // every rank: a collective; the totals are the same everywhere
                std::vector<int64_t> cnt(report_counts.size());
                if (cuts.empty()) gcn.queries().evaluate(3, nullptr, 0, cnt.data(), nullptr, nullptr);
                else gcn.queries().evaluate(3, nullptr, 0, cuts.data(), (int)cuts.size(), cnt.data(), nullptr);
                if (rank == 0) report_counts = cnt;
            }
            if (embed_path) {                                  // one rank (checked above): rows by node id
                const int N = params.num_nodes, h = params.hidden_dim;
                std::vector<float> e((size_t)std::max(N, 1) * h);
                gcn.queries().embed(nullptr, N, e.data(), false);
                FILE *f = fopen(embed_path, "w");
                bool ok = f != nullptr;
                for (int i = 0; ok && i < N; i++) {
                    ok = fprintf(f, "%d", i) > 0;
                    for (int j = 0; ok && j < h; j++) ok = fprintf(f, " %.9g", e[(size_t)i * h + j]) > 0;
                    ok = ok && fputc('\n', f) != EOF;
                }
                if (f && fclose(f) != 0) ok = false;
                if (!ok) throw GcnHipFailure(-1, std::string("gcn-hip: could not write the embeddings to ") + embed_path);
                fprintf(stderr, "gcn-hip: embeddings of %d nodes (%d wide) written to %s\n", N, h, embed_path);
            }
            if (similar_path) {
                constexpr int K = 10;
                const int N = params.num_nodes;
                std::vector<int32_t> ids((size_t)std::max(N, 1) * K);
                std::vector<float> sc((size_t)std::max(N, 1) * K);
                gcn.queries().similar(nullptr, N, K, ModelQueries::METRIC_COSINE, true, ids.data(), sc.data());
                FILE *f = fopen(similar_path, "w");
                bool ok = f != nullptr;
                for (int i = 0; ok && i < N; i++) {
                    ok = fprintf(f, "%d", i) > 0;
                    for (int j = 0; ok && j < K && ids[(size_t)i * K + j] >= 0; j++)
                        ok = fprintf(f, " %d:%.9g", ids[(size_t)i * K + j], sc[(size_t)i * K + j]) > 0;
                    ok = ok && fputc('\n', f) != EOF;
                }
                if (f && fclose(f) != 0) ok = false;
                if (!ok) throw GcnHipFailure(-1, std::string("gcn-hip: could not write the neighbours to ") + similar_path);
                fprintf(stderr, "gcn-hip: %d cosine neighbours of %d nodes written to %s\n", K, N, similar_path);
            }
            if (cluster_path) {                                // one rank (checked above): every node, rows by node id
                const int N = params.num_nodes, C = params.output_dim, K = cluster_k;
                std::vector<int32_t> assign((size_t)std::max(N, 1));
                std::vector<float> dist2((size_t)std::max(N, 1));
                const ModelQueries::KMeans r =
                    gcn.queries().kmeans(K, 0, nullptr, N, cluster_iters, true, ModelQueries::KMEANS_INIT_PLUSPLUS, nullptr, nullptr,
                                         cluster_seed_text ? &cluster_seed : nullptr, 0, assign.data(), dist2.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
                std::vector<int64_t> table((size_t)K * C, 0);      // the test split's nodes against their labels
                for (int i = 0; i < N; i++)
                    if (data.split[i] == 3 && data.label[i] >= 0 && data.label[i] < C && assign[i] >= 0) table[(size_t)assign[i] * C + data.label[i]]++;
                ClusterReport rep;
                std::string err;
                if (gcn_cluster_report(K, C, table.data(), &rep, &err) != 0) throw GcnHipFailure(-1, err);
                printf("clusters=%d cluster_iters=%d cluster_inertia=%.9g cluster_nmi=%.6f cluster_ari=%.6f cluster_purity=%.6f\n", K, r.iters_run, r.inertia,
                       rep.nmi, rep.ari, rep.purity);
                FILE *f = fopen(cluster_path, "w");
                bool ok = f != nullptr;
                for (int i = 0; ok && i < N; i++) ok = fprintf(f, "%d %d %.9g\n", i, assign[i], dist2[i]) > 0;
                if (f && fclose(f) != 0) ok = false;
                if (!ok) throw GcnHipFailure(-1, std::string("gcn-hip: could not write the clusters to ") + cluster_path);
                fprintf(stderr, "gcn-hip: %d clusters of %d nodes (%d iterations%s, seed %llu) written to %s\n", K, N, r.iters_run,
                        r.converged ? ", converged" : "", (unsigned long long)r.seed, cluster_path);
                if (silhouette_path) {                         // the clustering just made, over every node
                    std::vector<double> s((size_t)std::max(N, 1)), cmean((size_t)K);
                    std::vector<int32_t> nb((size_t)std::max(N, 1)), sizes((size_t)K);
                    const ModelQueries::Silhouette sr = gcn.queries().silhouette(0, nullptr, N, assign.data(), N, K, true, 0, s.data(), nullptr, nullptr,
                                                                                 nb.data(), cmean.data(), sizes.data());
                    double lowest = 0.0;
                    bool any = false;
                    for (int c = 0; c < K; c++)
                        if (sizes[c] > 0 && (!any || cmean[c] < lowest)) { lowest = cmean[c]; any = true; }
                    int64_t negative = 0;
                    for (int i = 0; i < N; i++) negative += s[i] < 0.0;
                    printf("silhouette=%.9g silhouette_min_cluster=%.9g silhouette_negative=%.6f\n", sr.score, lowest,
                           sr.points > 0 ? (double)negative / (double)sr.points : 0.0);
                    FILE *g = fopen(silhouette_path, "w");
                    bool good = g != nullptr;
                    for (int i = 0; good && i < N; i++) good = fprintf(g, "%d %d %.9g %d\n", i, assign[i], s[i], nb[i]) > 0;
                    if (g && fclose(g) != 0) good = false;
                    if (!good) throw GcnHipFailure(-1, std::string("gcn-hip: could not write the silhouette widths to ") + silhouette_path);
                    fprintf(stderr, "gcn-hip: the silhouette widths of %lld points in %d clusters written to %s\n", (long long)sr.points, sr.nonempty,
                            silhouette_path);
                }
            }
            if (structure_path) {                              // one rank (checked above): the test split
                const int C = params.output_dim;
                StructureCounts sc;
                sc.num_classes = C; sc.bins = structure_bins;
                sc.class_rows_truth.assign((size_t)C, 0); sc.class_rows_pred.assign((size_t)C, 0);
                sc.mix_truth.assign((size_t)C * C, 0); sc.mix_pred.assign((size_t)C * C, 0);
                sc.strata.assign((size_t)STRUCTURE_DEGREE_BUCKETS * (structure_bins + 1) * 2, 0);
                const ModelQueries::Structure r =
                    gcn.queries().structure(3, nullptr, 0, structure_bins, true, nullptr, nullptr, nullptr, sc.mix_truth.data(), sc.class_rows_truth.data(),
                                            sc.totals_truth, sc.mix_pred.data(), sc.class_rows_pred.data(), sc.totals_pred, sc.strata.data());
                StructureMetrics mt, mp;
                std::string err;
                if (gcn_structure_metrics(C, sc.mix_truth.data(), sc.class_rows_truth.data(), sc.totals_truth, &mt, &err) != 0 ||
                    gcn_structure_metrics(C, sc.mix_pred.data(), sc.class_rows_pred.data(), sc.totals_pred, &mp, &err) != 0 ||
                    gcn_structure_write(structure_path, sc, &err) != 0)
                    throw GcnHipFailure(-1, "gcn-hip: " + err);
                printf("edge_homophily=%.6f node_homophily=%.6f adjusted_homophily=%.6f class_insensitive_homophily=%.6f pred_edge_homophily=%.6f\n",
                       mt.edge_homophily, mt.node_homophily, mt.adjusted_homophily, mt.class_insensitive_homophily, mp.edge_homophily);
                fprintf(stderr, "gcn-hip: the label structure of %lld test nodes (%d agreement buckets) written to %s\n", (long long)r.rows, structure_bins,
                        structure_path);
            }
            if (reach_path) {                                  // one rank (checked above): the test split from the training split
                ReachCounts rc;
                rc.hops = reach_hops; rc.layers = gcn_reach_layers(reach_hops);
                rc.strata.assign((size_t)(reach_hops + 2) * 4, 0);
                rc.level_counts.assign((size_t)params.num_nodes + 1, 0);
                const ModelQueries::Reach r = gcn.queries().reach(3, nullptr, 0, 1 << 1, nullptr, 0, reach_hops, true, nullptr, nullptr, nullptr,
                                                                  rc.strata.data(), rc.totals, rc.level_counts.data(), (int)rc.level_counts.size());
                rc.level_counts.resize((size_t)r.levels + 1);
                rc.sources = r.sources; rc.unlabelled = r.unlabelled; rc.rounds = r.rounds;
                ReachMetrics rm;
                std::string err;
                if (gcn_reach_metrics(rc.strata.data(), rc.hops, rc.layers, &rm, &err) != 0 || gcn_reach_write(reach_path, rc, &err) != 0)
                    throw GcnHipFailure(-1, "gcn-hip: " + err);
                printf("reach_sources=%lld reach_levels=%d reach_unreachable=%lld reach_outside_two_hops=%lld acc_inside_two_hops=%.6f "
                       "acc_outside_two_hops=%.6f nearest_label_acc=%.6f components=%lld largest_component=%lld unseeded_components=%lld "
                       "unseeded_nodes=%lld\n",
                       (long long)r.sources, r.levels, (long long)rm.unreachable, (long long)rm.outside.rows, rm.inside.accuracy, rm.outside.accuracy,
                       rm.all.nearest_accuracy, (long long)rc.totals[1], (long long)rc.totals[2], (long long)rc.totals[3], (long long)rc.totals[4]);
                fprintf(stderr, "gcn-hip: the reach of %lld test nodes from %lld training nodes (%d distances) written to %s\n", (long long)r.rows,
                        (long long)r.sources, reach_hops, reach_path);
            }
            if (explain_path) {                                // one rank (checked above)
                const int h = params.hidden_dim, F = params.input_dim, C = params.output_dim;
                std::vector<int> nodes;
                for (int i = 0; i < params.num_nodes; i++)
                    if (data.split[i] == 3) nodes.push_back(i);
                const int n = (int)nodes.size();
                const size_t total = (size_t)gcn.queries().explain_size(nodes.data(), n);
                std::vector<int32_t> cls(std::max(n, 1)), ids(std::max<size_t>(total, 1));
                std::vector<float> logit(std::max(n, 1)), hid((size_t)std::max(n, 1) * h), feat((size_t)std::max(n, 1) * F), vals(std::max<size_t>(total, 1));
                std::vector<int64_t> ptr((size_t)n + 1);
                gcn.queries().explain(nodes.data(), nullptr, n, 0, cls.data(), logit.data(), hid.data(), feat.data(), ptr.data(), ids.data(), vals.data());
                std::vector<double> mean((size_t)C * F);
                std::vector<int64_t> cnt((size_t)C);
                if (n) gcn.queries().feature_importance(3, nullptr, 0, 0, mean.data(), cnt.data());
                FILE *f = fopen(explain_path, "w");
                bool ok = f != nullptr;
                // the `top` largest of key[0 .. m), largest first, ties by ascending label
                auto top_of = [](int m, int top, auto value, auto label) {
                    std::vector<int> order(m);
                    for (int j = 0; j < m; j++) order[j] = j;
                    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return value(a) > value(b) || (value(a) == value(b) && label(a) < label(b)); });
                    order.resize(std::min(m, top));
                    return order;
                };
                for (int i = 0; ok && i < n; i++) {
                    ok = fprintf(f, "%d %d %.9g |", nodes[i], cls[i], logit[i]) > 0;
                    const int64_t e0 = ptr[i];
                    for (int j : top_of((int)(ptr[i + 1] - e0), 5, [&](int a) { return vals[e0 + a]; }, [&](int a) { return ids[e0 + a]; }))
                        ok = ok && fprintf(f, " %d:%.9g", ids[e0 + j], vals[e0 + j]) > 0;
                    ok = ok && fputs(" |", f) != EOF;
                    for (int j : top_of(F, 5, [&](int a) { return feat[(size_t)i * F + a]; }, [](int a) { return a; }))
                        ok = ok && fprintf(f, " %d:%.9g", j, feat[(size_t)i * F + j]) > 0;
                    ok = ok && fputc('\n', f) != EOF;
                }
                for (int c = 0; ok && c < C; c++) {
                    ok = fprintf(f, "class %d nodes=%lld |", c, (long long)cnt[c]) > 0;
                    for (int j : top_of(F, 10, [&](int a) { return mean[(size_t)c * F + a]; }, [](int a) { return a; }))
                        ok = ok && fprintf(f, " %d:%.9g", j, mean[(size_t)c * F + j]) > 0;
                    ok = ok && fputc('\n', f) != EOF;
                }
                if (f && fclose(f) != 0) ok = false;
                if (!ok) throw GcnHipFailure(-1, std::string("gcn-hip: could not write the explanations to ") + explain_path);
                fprintf(stderr, "gcn-hip: explanations of %d test nodes written to %s\n", n, explain_path);
            }
            if (new_predict_path) {                            // one rank (checked above); at the temperature and by the cuts of the steps above
                const int C = params.output_dim, N = params.num_nodes;
                std::vector<int32_t> p(std::max(n_new, 1));
                std::vector<float> q(std::max(n_new, 1));
                std::vector<uint32_t> b((size_t)std::max(n_new, 1) * ml_wpr);
                static const int no_column = 0;                // rows without a single feature: still a sparse X_new, not a dense one
                const int *x_cols = new_nodes.feature_index.indices.empty() ? &no_column : new_nodes.feature_index.indices.data();
                static const float no_value = 0.f;
                const float *x_vals = new_nodes.feature_value.empty() ? &no_value : new_nodes.feature_value.data();
                gcn.queries().predict_new(new_nodes.feature_index.indptr.data(), x_cols, x_vals, n_new,
                                          new_nbr_ptr.data(), new_nbr_ids.data(), cuts.empty() ? nullptr : cuts.data(), (int)cuts.size(), p.data(),
                                          multilabel_path ? nullptr : q.data(), nullptr, b.data());
                FILE *f = fopen(new_predict_path, "w");
                bool ok = f != nullptr;
                for (int i = 0; ok && i < n_new; i++) {            // GCN_PREDICT's line format, node ids N + i
                    if (!multilabel_path) {
                        ok = fprintf(f, "%d %d %.6g\n", N + i, p[i], q[i]) > 0;
                        continue;
                    }
                    std::string line = std::to_string(N + i);
                    char sep = ' ';
                    for (int c = 0; c < C; c++)
                        if ((b[(size_t)i * ml_wpr + (c >> 5)] >> (c & 31)) & 1u) { line += sep; line += std::to_string(c); sep = ','; }
                    ok = fprintf(f, "%s\n", line.c_str()) > 0;
                }
                if (f && fclose(f) != 0) ok = false;
                if (!ok) throw GcnHipFailure(-1, std::string("gcn-hip: could not write the new nodes' predictions to ") + new_predict_path);
                fprintf(stderr, "gcn-hip: predictions of %d new nodes (ids %d..%d) written to %s\n", n_new, N, N + n_new - 1, new_predict_path);
            }
            if (pca_path) {                                    // one rank (checked above): every node, rows by node id
                const int N = params.num_nodes, h = params.hidden_dim, K = pca_k;
                std::vector<float> y((size_t)N * K);
                std::vector<double> expl((size_t)3 * h);
                const ModelQueries::Pca r = gcn.queries().pca_fit(K, 0, nullptr, N, true, true, false, 0, nullptr, nullptr, nullptr, nullptr, expl.data(),
                                                                  nullptr, y.data());
                printf("pca_components=%d pca_rows=%lld pca_rank=%d pca_explained_variance_ratio=", K, (long long)r.rows, r.rank);
                for (int j = 0; j < K; j++) printf("%s%.6f", j ? "," : "", expl[(size_t)h + j]);
                printf("\n");
                FILE *f = fopen(pca_path, "w");
                bool ok = f != nullptr;
                for (int i = 0; ok && i < N; i++) {
                    ok = fprintf(f, "%d", i) > 0;
                    for (int j = 0; ok && j < K; j++) ok = fprintf(f, " %.9g", y[(size_t)i * K + j]) > 0;
                    ok = ok && fputc('\n', f) != EOF;
                }
                if (f && fclose(f) != 0) ok = false;
                if (!ok) throw GcnHipFailure(-1, std::string("gcn-hip: could not write the principal coordinates to ") + pca_path);
                fprintf(stderr, "gcn-hip: %d principal coordinates of %d nodes (rank %d of %d) written to %s\n", K, N, r.rank, h, pca_path);
            }
            if ((o.flags & HIPGCN_TIMERS) && rank == 0) {
                static const char *names[] = {"train", "test", "matmul_fw", "matmul_bw", "spmatmul_fw", "spmatmul_bw", "graphsum_fw",
                                              "graphsum_bw", "loss_fw", "relu_fw", "relu_bw", "dropout_fw", "dropout_bw", "adam", "comm", "graphsum_wide"};
                for (int t = 2; t < __NUM_TMR; t++) {
                    long cnt = 0;
                    const double s = gcn.device_timers().total((timer_instance)t, &cnt);
                    if (cnt) printf("timer %-14s total=%.6f s  n=%ld  avg=%.3f ms\n", names[t], s, cnt, 1e3 * s / cnt);
                }
            }
        } catch (const GcnHipFailure &e) {
            // CUDA_CHECK policy: print and exit (cuda_kernel.cuh:11-18).  With one thread per GPU the sibling threads may be
            // inside an RCCL collective that will never complete: _exit ends the process without running static destructors
            // under them (exit() would).
            fprintf(stderr, "%s\n", e.what());
            fflush(stdout);
            fflush(stderr);
            _exit(e.code ? (e.code & 0xFF ? e.code & 0xFF : EXIT_FAILURE) : EXIT_FAILURE);
        }
    };
    // GCN_THREADS=1: one GPU through the worker-thread path of the several-GPU run (thread creation, join, the
    // failure policy above), so that path is executed on boxes that have a single GPU
    if (world == 1 && !env_int("GCN_THREADS", 0)) {
        worker(0, nullptr);
    } else if (world == 1) {
        std::thread t(worker, 0, nullptr);
        t.join();
    } else {
        char id[GCN_NCCL_ID_BYTES];
        if (rccl_get_unique_id(id) != 0) { std::cerr << "gcn-hip: ncclGetUniqueId failed" << std::endl; return EXIT_FAILURE; }
        std::vector<std::thread> th;
        for (int r = 0; r < world; r++) th.emplace_back(worker, r, id);
        for (auto &t : th) t.join();
    }
    if (predict_path) {
        FILE *f = fopen(predict_path, "w");
        bool ok = f != nullptr;
        for (int i = 0; ok && i < params.num_nodes; i++) {
            if (smooth) {                                  // smoothed classes carry no softmax probability
                ok = fprintf(f, "%d %d\n", i, all_pred[i]) > 0;
                continue;
            }
            if (!multilabel_path) {
                ok = fprintf(f, "%d %d %.6g\n", i, all_pred[i], all_prob[i]) > 0;
                continue;
            }
            std::string line = std::to_string(i);
            char sep = ' ';
            for (int c = 0; c < params.output_dim; c++)
                if ((all_bits[(size_t)i * ml_wpr + (c >> 5)] >> (c & 31)) & 1u) { line += sep; line += std::to_string(c); sep = ','; }
            ok = fprintf(f, "%s\n", line.c_str()) > 0;
        }
        if (f && fclose(f) != 0) ok = false;
        if (!ok) {
            fprintf(stderr, "gcn-hip: could not write the predictions to %s\n", predict_path);
            return EXIT_FAILURE;
        }
        fprintf(stderr, "gcn-hip: predictions of %d nodes written to %s\n", params.num_nodes, predict_path);
    }
    if (report_path) {
        ClassReport rep;
        std::string err;
        const int64_t *cm = multilabel_path ? nullptr : report_counts.data();
        int bad = multilabel_path ? gcn_class_report(C_out, nullptr, report_counts.data(), report_counts.data() + C_out, report_counts.data() + 2 * C_out, &rep, &err)
                                  : gcn_class_report(C_out, cm, nullptr, nullptr, nullptr, &rep, &err);
        if (!bad) bad = gcn_class_report_write(report_path, C_out, rep, cm, &err);
        if (bad) {
            fprintf(stderr, "gcn-hip: GCN_REPORT: %s\n", err.c_str());
            return EXIT_FAILURE;
        }
        fprintf(stderr, "gcn-hip: per-class report of the test split (macro-F1 %.5f, micro-F1 %.5f) written to %s\n", rep.macro_f1, rep.micro_f1, report_path);
    }
    return rc;
}
