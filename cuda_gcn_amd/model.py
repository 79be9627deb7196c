"""Python handle on the C++ host driver (libgcnhost.so: HipGCN and its Hip*
modules).  Mirrors the reference's GCN class: construct from params + data,
then train_epoch() / eval(split) / run() (src/seq/gcn.h:24-44).

All compute is in the HIP kernels behind include/gcnhip.h; this file only
marshals numpy arrays.  No GPU or no built library -> an exception.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib

MODULAR, HOST_MASKS, TIMERS, NO_GRAPH, EVAL_LANE, NO_EVAL_LANE, NO_REPLICATE_L1, REPLICATE_L1, GATHER_DH1, NO_ROW_GROUPS, NULL_COMM, BF16_TABLES, ALL_ROWS, NO_AGG_FIRST_EVAL, EXCHANGE_ALLGATHER, EXCHANGE_HALO, MASKED_BWD, NO_LABEL_HINT, OVERLAP_EXCHANGE, STRUCTURE_PARTITION, ID_PARTITION, SYNC_EPOCHS, EDGE_COEF = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 131072, 524288, 1048576, 2097152, 4194304, 8388608, 16777216
# (65536 and 262144 are retired flag bits: not to be reused)
TIMER_NAMES = ["train", "test", "matmul_fw", "matmul_bw", "spmatmul_fw", "spmatmul_bw", "graphsum_fw", "graphsum_bw",
               "loss_fw", "relu_fw", "relu_bw", "dropout_fw", "dropout_bw", "adam", "comm", "graphsum_wide"]
BETA_MAX = np.float32(8e37)           # GCNHIP_BETA_MAX of include/gcnhip_driver.h: the largest beta = 1 / T the kernels accept


class GcnHostError(RuntimeError):
    pass


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _ck(lib, rc, what):
    if rc != 0:
        raise GcnHostError(f"{what}: error {rc}: {lib.gcnhost_last_error().decode()}")


def default_params(**kw):
    lib = _lib.gcnhost()
    p = lib.gcnhost_params_default()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def nccl_unique_id() -> bytes:
    lib = _lib.gcnhost()
    buf = C.create_string_buffer(128)
    _ck(lib, lib.gcnhost_nccl_unique_id(buf), "gcnhost_nccl_unique_id")
    return buf.raw


class HipGCNModel:
    """ds: dict with num_nodes, input_dim, output_dim, g_indptr, g_indices, f_indptr, f_indices (or None
    for a dense X), f_val, split, label (the reference's GCNData).

    multilabel: a bool/uint8 [num_nodes, C] matrix (1 <= C <= 256) switches the model to multi-label mode: output_dim = C,
    the loss is the per-class sigmoid cross-entropy, and train_epoch / eval / run_epochs report micro-F1 where they report
    accuracy otherwise.  ds["label"] may then be absent.

    class_weights: a float [C] array, or "balanced" (balanced_class_weights of the training split).  Single-label: the weight of
    every class in the loss, which becomes the weighted mean sum(w[t] . term) / sum(w[t]) (torch's cross_entropy(weight=));
    accuracy stays unweighted.  With multilabel=Y: the weight of every class's positive term (BCEWithLogitsLoss(pos_weight=)).
    None: the unweighted model, bit for bit."""

    def __init__(self, ds, seed=0, device=0, flags=0, rank=0, world=1, nccl_id: bytes | None = None,
                 host_allgather=None, host_allreduce=None, multilabel=None, class_weights=None, **hyper):
        self.lib = lib = _lib.gcnhost()
        self.seed = int(seed)
        out_dim = ds["output_dim"]
        words = None
        if multilabel is not None:
            from .ops import pack_multihot
            y = np.asarray(multilabel)
            if y.ndim != 2 or y.shape[0] != ds["num_nodes"] or not 1 <= y.shape[1] <= 256:
                raise ValueError(f"multilabel: expected a [num_nodes={ds['num_nodes']}, C] matrix with 1 <= C <= 256, got {y.shape}")
            out_dim = y.shape[1]
            words = pack_multihot(y != 0)
        self.multilabel = words is not None
        cw = None
        if class_weights is not None:
            if isinstance(class_weights, str):
                if class_weights != "balanced":
                    raise ValueError(f"class_weights: an array of {out_dim} floats or 'balanced', got {class_weights!r}")
                cw = balanced_class_weights(np.asarray(multilabel) != 0 if words is not None else ds["label"], ds["split"], out_dim)
            else:
                cw = np.ascontiguousarray(class_weights, np.float32).ravel()
                if cw.size != out_dim:
                    raise ValueError(f"class_weights: {cw.size} weights for {out_dim} classes")
        self.class_weights = cw
        p = default_params(num_nodes=ds["num_nodes"], input_dim=ds["input_dim"], output_dim=out_dim, **hyper)
        self.params = p
        self._keep = [_i32(ds["g_indptr"]), _i32(ds["g_indices"]), _i32(ds["f_indptr"]),
                      _i32(ds["f_indices"]) if ds.get("f_indices") is not None else None,
                      np.ascontiguousarray(ds["f_val"], np.float32), _i32(ds["split"]),
                      _i32(ds["label"]) if ds.get("label") is not None else None, words]
        k = self._keep
        self._ag = _lib.ALLGATHER_FN(host_allgather) if host_allgather else C.cast(None, _lib.ALLGATHER_FN)
        self._ar = _lib.ALLREDUCE_FN(host_allreduce) if host_allreduce else C.cast(None, _lib.ALLREDUCE_FN)
        h = C.c_void_p()
        if cw is not None:
            rc = lib.gcnhost_model_create_weighted(C.byref(h), C.byref(p), k[0].ctypes.data, k[1].ctypes.data, k[2].ctypes.data,
                                                   k[3].ctypes.data if k[3] is not None else None, k[4].ctypes.data,
                                                   k[5].ctypes.data, k[6].ctypes.data if k[6] is not None else None,
                                                   k[7].ctypes.data if k[7] is not None else None, cw.ctypes.data,
                                                   int(seed), int(device), int(flags),
                                                   int(rank), int(world), nccl_id, self._ag, self._ar, None)
            _ck(lib, rc, "gcnhost_model_create_weighted")
        elif words is None:
            rc = lib.gcnhost_model_create(C.byref(h), C.byref(p), k[0].ctypes.data, k[1].ctypes.data, k[2].ctypes.data,
                                          k[3].ctypes.data if k[3] is not None else None, k[4].ctypes.data,
                                          k[5].ctypes.data, k[6].ctypes.data, int(seed), int(device), int(flags),
                                          int(rank), int(world), nccl_id, self._ag, self._ar, None)
            _ck(lib, rc, "gcnhost_model_create")
        else:
            rc = lib.gcnhost_model_create_multilabel(C.byref(h), C.byref(p), k[0].ctypes.data, k[1].ctypes.data, k[2].ctypes.data,
                                                     k[3].ctypes.data if k[3] is not None else None, k[4].ctypes.data,
                                                     k[5].ctypes.data, k[6].ctypes.data if k[6] is not None else None,
                                                     k[7].ctypes.data, int(seed), int(device), int(flags),
                                                     int(rank), int(world), nccl_id, self._ag, self._ar, None)
            _ck(lib, rc, "gcnhost_model_create_multilabel")
        self.h = h
        self._keep = None           # the C++ side copied everything it needs

    def train_epoch(self):
        a, b = C.c_float(), C.c_float()
        _ck(self.lib, self.lib.gcnhost_model_train_epoch(self.h, C.byref(a), C.byref(b)), "train_epoch")
        return a.value, b.value

    def eval(self, split):
        a, b = C.c_float(), C.c_float()
        _ck(self.lib, self.lib.gcnhost_model_eval(self.h, split, C.byref(a), C.byref(b)), "eval")
        return a.value, b.value

    def run_epochs(self, n, want_trace=True):
        tr = np.zeros((n, 4), np.float32) if want_trace else None
        _ck(self.lib, self.lib.gcnhost_model_run_epochs(self.h, n, tr.ctypes.data if tr is not None else None), "run_epochs")
        return tr

    def run(self):
        _ck(self.lib, self.lib.gcnhost_model_run(self.h), "run")

    def sync(self):
        _ck(self.lib, self.lib.gcnhost_model_sync(self.h), "sync")

    def info(self):
        r, w, s, n = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        e = C.c_int64()
        _ck(self.lib, self.lib.gcnhost_model_info(self.h, C.byref(r), C.byref(w), C.byref(s), C.byref(n), C.byref(e)), "info")
        return dict(rank=r.value, world=w.value, row_start=s.value, local_rows=n.value, local_edges=e.value)

    def row_scale(self):
        """(dinv = 1/sqrt(deg) of this rank's rows, factored?) — factored: var(1), var(3), var(4) are stored pre-multiplied by
        dinv of their row and their gradients accordingly (host/gcn.h); EDGE_COEF restores the reference's values"""
        n = self.info()["local_rows"]
        d = np.ones(n, np.float32)
        f = C.c_int()
        _ck(self.lib, self.lib.gcnhost_model_row_scale(self.h, d.ctypes.data, C.byref(f)), "row_scale")
        return d, bool(f.value)

    def var_reference(self, k, grad=False):
        """variable k as the REFERENCE stores it (gcn.cpp:21-54): the factored model's pre-multiplied rows divided back"""
        v = self.var(k, grad)
        d, factored = self.row_scale()
        if not factored or k in (2, 5):
            return v
        d = d[:, None].astype(np.float64)
        if not grad:
            return (v / d).astype(np.float32) if k in (1, 3, 4) else v            # dinv.H0, dinv.H1, dinv.Z0 ; Z as is
        # gradients: dZ' = dinv.dZ (6), dH1' = dinv.dH1 (3) ; T = dZ0/dinv (4), S = dH0/dinv (1)
        return (v / d).astype(np.float32) if k in (6, 3) else (v * d).astype(np.float32)

    def row_ids(self):
        """(node of the caller's dataset for every local row of this rank, whether the model renumbered the nodes)"""
        n = self.info()["local_rows"]
        ids = np.zeros(n, np.int32)
        ren = C.c_int()
        _ck(self.lib, self.lib.gcnhost_model_row_ids(self.h, ids.ctypes.data, C.byref(ren)), "row_ids")
        return ids, bool(ren.value)

    def exchange(self):
        h, t = C.c_int(), C.c_int()
        r, sn = C.c_int64(), C.c_int64()
        sh = C.c_double()
        _ck(self.lib, self.lib.gcnhost_model_exchange(self.h, C.byref(h), C.byref(r), C.byref(sn), C.byref(t), C.byref(sh)), "exchange")
        return dict(mode="halo" if h.value else "allgather", recv_rows=r.value, send_rows=sn.value, table_rows=t.value, halo_share=sh.value)

    def var(self, k, grad=False):
        r, c = C.c_int(), C.c_int()
        _ck(self.lib, self.lib.gcnhost_model_get_var(self.h, k, int(grad), None, C.byref(r), C.byref(c)), "get_var")
        out = np.zeros((r.value, c.value), np.float32)
        _ck(self.lib, self.lib.gcnhost_model_get_var(self.h, k, int(grad), out.ctypes.data, C.byref(r), C.byref(c)), "get_var")
        return out

    def set_weights(self, w1, w2):
        w1, w2 = np.ascontiguousarray(w1, np.float32), np.ascontiguousarray(w2, np.float32)
        _ck(self.lib, self.lib.gcnhost_model_set_weights(self.h, w1.ctypes.data, w2.ctypes.data), "set_weights")

    def predict(self, nodes=None, logp=False):
        """(pred int32[n], prob f32[n]) — the class with the largest logit (the lowest on a tie, numpy.argmax's rule) and its softmax
        probability, from an evaluation forward with the current weights (no dropout) whose logit aggregation carries the
        prediction epilogue.  nodes: dataset node ids, each a row of this rank (repeats allowed); None: every row of this rank in
        local-row order (row_ids() names them).  logp=True: a third array [n, output_dim] with the log-softmax rows.  Several
        ranks: every rank calls it.  Training state is not touched."""
        if nodes is None:
            q, n, qp = None, self.info()["local_rows"], None
        else:
            q = np.ascontiguousarray(nodes, np.int32).ravel()
            n, qp = q.size, q.ctypes.data
        pred = np.zeros(max(n, 1), np.int32)
        prob = np.zeros(max(n, 1), np.float32)
        lp = np.zeros((max(n, 1), self.params.output_dim), np.float32) if logp else None
        _ck(self.lib, self.lib.gcnhost_model_predict(self.h, qp, n, pred.ctypes.data, prob.ctypes.data, lp.ctypes.data if logp else None), "predict")
        return (pred[:n], prob[:n], lp[:n]) if logp else (pred[:n], prob[:n])

    def predict_multilabel(self, nodes=None, prob=False, thresholds=None):
        """bool [n, C] — the classes whose logit is above 0 (the rule micro-F1 counts with), from an evaluation forward with the
        current weights whose logits go to scratch; prob=True: also the sigmoid of every logit, f32 [n, C].  nodes as in
        predict(); only on a model built with multilabel=.  Several ranks: every rank calls it.  Training state is not touched.
        thresholds (f32 [C], tune_thresholds()["threshold"] or read_thresholds()): class c is predicted when its logit is >=
        thresholds[c] instead (one rank; prob stays the sigmoid); a wrong length or a NaN raises ValueError."""
        from .ops import unpack_multihot
        if nodes is None:
            n, qp = self.info()["local_rows"], None
        else:
            q = np.ascontiguousarray(nodes, np.int32).ravel()
            n, qp = q.size, q.ctypes.data
        c = self.params.output_dim
        words = np.zeros((max(n, 1), (c + 31) // 32), np.uint32)
        pr = np.zeros((max(n, 1), c), np.float32) if prob else None
        if thresholds is None:
            _ck(self.lib, self.lib.gcnhost_model_predict_multilabel(self.h, qp, n, words.ctypes.data, pr.ctypes.data if prob else None),
                "predict_multilabel")
        else:
            thr = thresholds_array("predict_multilabel", thresholds, c)
            _ck(self.lib, self.lib.gcnhost_model_predict_multilabel_thr(self.h, qp, n, thr.ctypes.data, thr.size, words.ctypes.data,
                                                                       pr.ctypes.data if prob else None), "predict_multilabel")
        sets = unpack_multihot(words[:n], c)
        return (sets, pr[:n]) if prob else sets

    def predict_new_nodes(self, features, nbr_ptr, nbr_ids, logp=False, prob=False, thresholds=None):
        """Classify m nodes the dataset did not hold, attached to the trained graph: new node i has id num_nodes + i, the
        feature row features[i] and the stored row [num_nodes + i, nbr_ids[nbr_ptr[i]:nbr_ptr[i + 1]]...] (new_node_rows has the
        rule; an id num_nodes + k names new node k of the same call).  No existing row changes and the new rows influence no
        dataset node, so the logits are what an evaluation forward gives those rows on the augmented dataset; the dataset, the
        adjacency object and its schedule are not rebuilt.  features: a float [m, input_dim] array, or an (indptr, indices,
        values) CSR triple.  Single-label model: (pred int32 [m], prob f32 [m]) at the model's temperature, with logp=True a
        third array [m, C] of log-softmax rows, as predict() returns them.  Multi-label model: the bool [m, C] sets (z > 0, or
        z >= thresholds[c]), with prob=True also the sigmoid of every logit.  m = 0 returns empty arrays.  One rank; training
        state is not touched and nothing is cached between calls."""
        c, f = self.params.output_dim, self.params.input_dim
        if isinstance(features, tuple):
            xp, xi, xv = (np.ascontiguousarray(features[0], np.int32).ravel(), np.ascontiguousarray(features[1], np.int32).ravel(),
                          np.ascontiguousarray(features[2], np.float32).ravel())
            m = xp.size - 1
            if m < 0 or xi.size != xv.size or (m >= 0 and xp.size and xi.size != xp[-1]):
                raise ValueError("predict_new_nodes: features is (indptr [m + 1], indices [nnz], values [nnz])")
        else:
            x = np.ascontiguousarray(features, np.float32)
            if x.ndim != 2 or x.shape[1] != f:
                raise ValueError(f"predict_new_nodes: features has shape {x.shape}, the model takes [m, {f}]")
            m = x.shape[0]
            xp, xi, xv = np.arange(m + 1, dtype=np.int32) * f, None, x.ravel()
        p64 = np.ascontiguousarray(nbr_ptr, np.int64).ravel()
        ids = np.ascontiguousarray(nbr_ids, np.int32).ravel()
        if p64.size != m + 1:
            raise ValueError(f"predict_new_nodes: nbr_ptr has {p64.size} entries for {m} new nodes (m + 1 expected)")
        if p64[-1] != ids.size:
            raise ValueError(f"predict_new_nodes: nbr_ptr ends at {p64[-1]}, nbr_ids has {ids.size} entries")
        thr = None
        if thresholds is not None and self.multilabel:
            thr = thresholds_array("predict_new_nodes", thresholds, c)
        elif thresholds is not None:
            thr = np.ascontiguousarray(thresholds, np.float32).ravel()      # refused by the library: a single-label model
        n1 = max(m, 1)
        pred, pr1 = np.zeros(n1, np.int32), np.zeros(n1, np.float32)
        lp = np.zeros((n1, c), np.float32) if logp and not self.multilabel else None
        words = np.zeros((n1, (c + 31) // 32), np.uint32) if self.multilabel else None
        prc = np.zeros((n1, c), np.float32) if prob and self.multilabel else None
        probs = prc if self.multilabel else pr1
        _ck(self.lib, self.lib.gcnhost_model_predict_new(
            self.h, xp.ctypes.data, xi.ctypes.data if xi is not None else None, xv.ctypes.data, m, p64.ctypes.data, ids.ctypes.data,
            thr.ctypes.data if thr is not None else None, thr.size if thr is not None else 0, pred.ctypes.data,
            probs.ctypes.data if probs is not None else None, lp.ctypes.data if lp is not None else None,
            words.ctypes.data if words is not None else None), "predict_new_nodes")
        if self.multilabel:
            from .ops import unpack_multihot
            sets = unpack_multihot(words[:m], c)
            return (sets, prc[:m]) if prob else sets
        return (pred[:m], pr1[:m], lp[:m]) if logp else (pred[:m], pr1[:m])

    def evaluate(self, split=None, nodes=None, thresholds=None):
        """Per-class evaluation: one evaluation forward with the current weights (no dropout) over a set of rows, integer counts
        per class formed on the GPU behind it, and the metrics class_report() derives from them.  Rows: the nodes of `split`
        (1 train, 2 validation, 3 test) on this rank; or, with split=None, the `nodes` query with predict()'s conventions
        (repeats counted as often as listed; None: every row of this rank).  Returns a dict: rows, support, precision, recall, f1
        (float64 [C]), macro_f1, micro_f1; a single-label model adds confusion (int64 [C, C], row = truth, column = prediction),
        accuracy, unlabelled (rows whose label is outside [0, C): in no cell); a multi-label model adds tp, fp, fn (int64 [C]).
        Several ranks: every rank calls it and every rank gets the totals over all ranks.  Training state is not touched.
        thresholds (f32 [C]; a multi-label model on one rank): class c is predicted when its logit is >= thresholds[c] instead
        of > 0; a wrong length or a NaN raises ValueError."""
        if split is not None and nodes is not None:
            raise ValueError("evaluate: give a split or a node query, not both")
        if split is not None and split not in (1, 2, 3):
            raise ValueError(f"evaluate: split is 1 (train), 2 (validation) or 3 (test), got {split!r}")
        if nodes is None:
            n, qp = 0, None
        else:
            q = np.ascontiguousarray(nodes, np.int32).ravel()
            n = q.size
            q = q if n else np.zeros(1, np.int32)              # an empty query is still a query (not "every row")
            qp = q.ctypes.data
        c = self.params.output_dim
        counts = np.zeros((3, c) if self.multilabel else (c, c), np.int64)
        rows, unl = C.c_int64(), C.c_int64()
        if thresholds is None:
            _ck(self.lib, self.lib.gcnhost_model_evaluate(self.h, int(split or 0), qp, n, counts.ctypes.data, C.byref(rows), C.byref(unl)), "evaluate")
        else:
            thr = thresholds_array("evaluate", thresholds, c)
            counts = np.zeros((3, c), np.int64)                # the call refuses a single-label model
            _ck(self.lib, self.lib.gcnhost_model_evaluate_thr(self.h, int(split or 0), qp, n, thr.ctypes.data, thr.size, counts.ctypes.data,
                                                              C.byref(rows)), "evaluate")
        if self.multilabel:
            out = class_report(tp=counts[0], fp=counts[1], fn=counts[2])
            out.pop("accuracy")
        else:
            out = class_report(confusion=counts)
            out["confusion"] = counts
            out["unlabelled"] = unl.value
            for k in ("tp", "fp", "fn"):
                out.pop(k)
        out["rows"] = rows.value
        return out

    def ranking(self, split=3, nodes=None, return_scores=False, scratch_bytes=0):
        """Per-class ROC-AUC and average precision without a decision threshold: one evaluation forward with the current weights
        (no dropout), then keys, a segmented sort and binary searches on the GPU; 5 C + 1 numbers cross to the host.  Rows as in
        evaluate(): the nodes of `split` (3, the test split, by default), or with split=None the `nodes` query (repeats counted
        as often as listed; None: every row).  A multi-label model is scored on its logits; a single-label model one-vs-rest on
        the log-softmax rows at the model's temperature (predict's logp).  Returns a dict: rows, unlabelled (rows with a label
        outside [0, C): in no class), invalid (int64 [C]: labelled rows whose score is NaN), pos, neg, u2 (int64 [C]), ap_sum
        (float64 [C]) and what ranking_report() derives from them: auc, ap, auc_defined, ap_defined, macro_auc, macro_ap,
        weighted_auc, weighted_ap, classes_defined.  return_scores=True adds scores (f32 [rows, C], in list order).
        scratch_bytes caps the key tables and the sort scratch (0: 256 MiB): the classes run in batches, with the same result
        in every batching.  One rank, at most 64 (single-label) or 256 (multi-label) classes.  Training state is not touched."""
        if split is not None and nodes is not None:
            raise ValueError("ranking: give a split or a node query, not both")
        if split is not None and split not in (1, 2, 3):
            raise ValueError(f"ranking: split is 1 (train), 2 (validation) or 3 (test), got {split!r}")
        if int(scratch_bytes) < 0:
            raise ValueError(f"ranking: scratch_bytes must be >= 0, got {scratch_bytes!r}")
        if nodes is None:
            n, qp, listed = 0, None, self.info()["local_rows"]     # (a split lists at most that many rows)
        else:
            q = np.ascontiguousarray(nodes, np.int32).ravel()
            n = listed = q.size
            q = q if n else np.zeros(1, np.int32)              # an empty query is still a query (not "every row")
            qp = q.ctypes.data
        c = self.params.output_dim
        u2, pos, neg, inv = (np.zeros(c, np.int64) for _ in range(4))
        aps = np.zeros(c, np.float64)
        unl, rows = C.c_int64(), C.c_int64()
        sc = np.zeros((max(listed, 1), c), np.float32) if return_scores else None
        _ck(self.lib, self.lib.gcnhost_model_ranking(self.h, int(split or 0), qp, n, int(scratch_bytes), u2.ctypes.data, aps.ctypes.data, pos.ctypes.data,
                                                     neg.ctypes.data, inv.ctypes.data, C.byref(unl), C.byref(rows),
                                                     sc.ctypes.data if return_scores else None, sc.size if return_scores else 0), "ranking")
        out = ranking_report(u2=u2, ap_sum=aps, pos=pos, neg=neg)
        out.update(rows=rows.value, unlabelled=unl.value, invalid=inv, pos=pos, neg=neg, u2=u2, ap_sum=aps)
        if return_scores:
            out["scores"] = sc[:rows.value].copy()
        return out

    def tune_thresholds(self, split=2, nodes=None, beta=1.0, scratch_bytes=0):
        """One decision threshold per class of a multi-label model, fitted on the GPU: the cut on the logit with the largest
        F-beta over the listed rows (the validation split by default), the highest such cut on a tie.  ranking()'s path — one
        evaluation forward, keys, a segmented sort — then one scan per class batch; only O(C) numbers cross to the host.  Rows as
        in evaluate(); scratch_bytes as in ranking() (the same bits in every batching).  Returns a dict: threshold (f32 [C]: class
        c is predicted when its logit is >= threshold[c]), defined (bool [C]; False: no positive among the rows — threshold 0, f 0),
        tp, fp, fn (int64 [C], at the cut), f (float64 [C], the F-beta at the cut), pos, neg (int64 [C]), invalid (int64 [C]: rows
        with a NaN logit, in neither), rows, beta, and the class_report(tp=, fp=, fn=) metrics of the fit rows at the cuts
        (support, precision, recall, f1, macro_f1, micro_f1).  Hand threshold to predict_multilabel / evaluate(thresholds=) or
        write_thresholds().  A multi-label model, one rank, at most 256 classes.  Training state is not touched."""
        if split is not None and nodes is not None:
            raise ValueError("tune_thresholds: give a split or a node query, not both")
        if split is not None and split not in (1, 2, 3):
            raise ValueError(f"tune_thresholds: split is 1 (train), 2 (validation) or 3 (test), got {split!r}")
        if int(scratch_bytes) < 0:
            raise ValueError(f"tune_thresholds: scratch_bytes must be >= 0, got {scratch_bytes!r}")
        beta = check_beta("tune_thresholds", beta)
        if nodes is None:
            n, qp = 0, None
        else:
            q = np.ascontiguousarray(nodes, np.int32).ravel()
            n = q.size
            q = q if n else np.zeros(1, np.int32)              # an empty query is still a query (not "every row")
            qp = q.ctypes.data
        c = self.params.output_dim
        thr, f, defined = np.zeros(c, np.float32), np.zeros(c, np.float64), np.zeros(c, np.int32)
        tp, fp, fn, pos, neg, inv = (np.zeros(c, np.int64) for _ in range(6))
        rows = C.c_int64()
        _ck(self.lib, self.lib.gcnhost_model_tune_thresholds(self.h, int(split or 0), qp, n, beta, int(scratch_bytes), thr.ctypes.data, tp.ctypes.data,
                                                             fp.ctypes.data, fn.ctypes.data, f.ctypes.data, pos.ctypes.data, neg.ctypes.data,
                                                             inv.ctypes.data, defined.ctypes.data, C.byref(rows)), "tune_thresholds")
        out = class_report(tp=tp, fp=fp, fn=fn)
        out.pop("accuracy")
        out.update(threshold=thr, defined=defined.astype(bool), tp=tp, fp=fp, fn=fn, f=f, pos=pos, neg=neg, invalid=inv, rows=rows.value, beta=beta)
        return out

    # ---- label propagation and Correct & Smooth: the graph and the known labels used at inference time
    def _smooth_args(self, what, pairs, splits=None):
        """argument checks that need no GPU; returns the split mask (bit s = the labelled nodes of split s are known)"""
        for name, alpha, iters in pairs:
            if not 0.0 <= float(alpha) <= 1.0:
                raise ValueError(f"{what}: {name} must be in [0, 1], got {alpha!r}")
            if int(iters) != iters or iters < 0:
                raise ValueError(f"{what}: iters must be an integer >= 0, got {iters!r}")
        if splits is None:
            return 0
        if self.multilabel:
            raise ValueError(f"{what}: this is a multi-label model")
        if self.params.output_dim > 64:
            raise ValueError(f"{what}: at most 64 classes, this model has {self.params.output_dim}")
        s = sorted(set(int(x) for x in np.atleast_1d(splits)))
        if not s or any(x not in (1, 2, 3) for x in s):
            raise ValueError(f"{what}: splits are 1 (train), 2 (validation), 3 (test), at least one; got {splits!r}")
        return sum(1 << x for x in s)

    def propagate(self, y0, alpha, iters, clamp=(-np.inf, np.inf), argmax=False):
        """Y_{k+1} = clip(alpha . A^ . Y_k + (1 - alpha) . Y_0, lo, hi) with Y_0 = y0, `iters` times on the GPU (one blend
        aggregation per iteration, ping-ponging two device tables).  y0: float32 [num_nodes, C'] in dataset node order, 1 <= C' <=
        64 (it need not be the model's class count).  Returns Y_iters (y0 itself for iters=0), and with argmax=True also its row
        argmax (int32, the lowest column on a tie).  One rank only.  Training state is not touched."""
        lo, hi = clamp
        self._smooth_args("propagate", [("alpha", alpha, iters)])
        y = np.ascontiguousarray(y0, np.float32)
        n = self.params.num_nodes
        if y.ndim != 2 or y.shape[0] != n or not 1 <= y.shape[1] <= 64:
            raise ValueError(f"propagate: y0 must be [num_nodes={n}, C'] with 1 <= C' <= 64, got {y.shape}")
        if not float(lo) <= float(hi):
            raise ValueError(f"propagate: clamp=(lo, hi) needs lo <= hi, got {clamp!r}")
        out = np.zeros_like(y)
        pred = np.zeros(max(n, 1), np.int32) if argmax else None
        _ck(self.lib, self.lib.gcnhost_model_propagate(self.h, y.ctypes.data, y.shape[1], float(alpha), int(iters), float(lo), float(hi),
                                                       out.ctypes.data, pred.ctypes.data if argmax else None), "propagate")
        return (out, pred[:n]) if argmax else out

    def label_propagation(self, alpha=0.9, iters=50, splits=(1,)):
        """(pred int32 [num_nodes], Y f32 [num_nodes, C]) — label propagation from the labelled nodes of `splits`: propagate() with
        Y_0 = their one-hot rows (zero rows elsewhere) and clamp [0, 1].  Needs no trained weights.  Single-label models, at most
        64 classes, one rank."""
        mask = self._smooth_args("label_propagation", [("alpha", alpha, iters)], splits)
        n, c = self.params.num_nodes, self.params.output_dim
        pred, y = np.zeros(max(n, 1), np.int32), np.zeros((n, c), np.float32)
        _ck(self.lib, self.lib.gcnhost_model_label_propagation(self.h, float(alpha), int(iters), mask, pred.ctypes.data, y.ctypes.data),
            "label_propagation")
        return pred[:n], y

    def correct_and_smooth(self, alpha_correct=0.8, iters_correct=50, alpha_smooth=0.8, iters_smooth=50, splits=(1,), scores=True):
        """(pred int32 [num_nodes], G f32 [num_nodes, C]) — Correct & Smooth (Huang et al., 2020) on the softmax of one evaluation
        forward with the current weights: the residual of the labelled nodes of `splits` is propagated (clamp [-1, 1]), scaled per
        row and added to the softmax, the labelled rows are reset to their one-hot labels, and the result is propagated again
        (clamp [0, 1]); pred is the row argmax of G, written by the last launch.  scores=False: G is not copied back (None).
        Single-label models, at most 64 classes, one rank.  Training state is not touched."""
        mask = self._smooth_args("correct_and_smooth", [("alpha_correct", alpha_correct, iters_correct),
                                                        ("alpha_smooth", alpha_smooth, iters_smooth)], splits)
        n, c = self.params.num_nodes, self.params.output_dim
        pred = np.zeros(max(n, 1), np.int32)
        g = np.zeros((n, c), np.float32) if scores else None
        _ck(self.lib, self.lib.gcnhost_model_correct_and_smooth(self.h, float(alpha_correct), int(iters_correct), float(alpha_smooth),
                                                                int(iters_smooth), mask, pred.ctypes.data, g.ctypes.data if scores else None),
            "correct_and_smooth")
        return pred[:n], g

    # ---- temperature scaling and calibration error: can predict()'s probabilities be trusted, and one scalar that repairs them
    def _calib_args(self, what, bins=None, temperature=None):
        """argument checks that need no GPU"""
        if self.multilabel:
            raise GcnHostError(f"{what}: this is a multi-label model (a temperature scales one softmax per node)")
        if self.params.output_dim > 64:
            raise GcnHostError(f"{what}: at most 64 classes, this model has {self.params.output_dim}")
        if bins is not None and (int(bins) != bins or not 1 <= bins <= 64):
            raise GcnHostError(f"{what}: bins must be an integer in 1..64, got {bins!r}")
        if temperature is not None:
            # the kernels take the f32 beta = 1 / T and accept it up to BETA_MAX (include/gcnhip_driver.h derives the limit)
            with np.errstate(all="ignore"):
                t32 = np.float32(temperature)
                ok = float(temperature) > 0.0 and np.isfinite(t32) and t32 > 0 and np.float32(1.0) / t32 <= BETA_MAX
            if not ok:
                raise GcnHostError(f"{what}: the temperature must be finite and > 0, with 1 / T at most 8e37 (T >= 1.25e-38), got {temperature!r}")

    @property
    def temperature(self):
        """the temperature T of predict()'s softmax(z / T) and of correct_and_smooth's starting point (1 unless set)"""
        t = C.c_float()
        _ck(self.lib, self.lib.gcnhost_model_temperature(self.h, C.byref(t)), "temperature")
        return t.value

    def set_temperature(self, temperature):
        """From now on predict() returns prob (and logp) of softmax(z / T) — pred does not depend on T — and correct_and_smooth()
        starts from that softmax.  At T = 1 both run exactly what they ran before.  Training, eval, evaluate and the weights file
        ignore the temperature."""
        if float(temperature) != 1.0:
            self._calib_args("set_temperature", temperature=temperature)
        _ck(self.lib, self.lib.gcnhost_model_set_temperature(self.h, float(temperature)), "set_temperature")

    def calibrate(self, split=2, bins=15, apply=True):
        """Temperature scaling (Guo et al., 2017): fits T on the labelled rows of `split` (the validation split) by minimising the
        negative log-likelihood of softmax(z / T) — one evaluation forward, then a safeguarded Newton iteration in beta = 1 / T on
        [0.01, 100] whose every step is one small launch.  Returns a dict: temperature, nll_before / nll_after (mean NLL of the
        split at T = 1 and at the fit), steps, at_bound (the fit stopped on an end of the bracket: a split classified perfectly
        has no minimum), rows, and ece_before / ece_after of the same split over `bins` bins.  apply=True then sets the
        temperature.  Single-label models, at most 64 classes, one rank.  Training state is not touched."""
        self._calib_args("calibrate", bins=bins)
        if split not in (1, 2, 3):
            raise GcnHostError(f"calibrate: split is 1 (train), 2 (validation) or 3 (test), got {split!r}")
        out = np.zeros(6, np.float64)
        count, correct, conf = np.zeros((2, bins), np.int64), np.zeros((2, bins), np.int64), np.zeros((2, bins), np.float64)
        _ck(self.lib, self.lib.gcnhost_model_calibrate(self.h, int(split), int(bins), out.ctypes.data, count.ctypes.data, correct.ctypes.data,
                                                       conf.ctypes.data), "calibrate")
        res = dict(temperature=float(out[0]), nll_before=float(out[1]), nll_after=float(out[2]), steps=int(out[3]), at_bound=bool(out[4]),
                   rows=int(out[5]), ece_before=calibration_report(count[0], correct[0], conf[0])["ece"],
                   ece_after=calibration_report(count[1], correct[1], conf[1])["ece"])
        if apply:
            self.set_temperature(res["temperature"])
        return res

    def calibration(self, split=None, nodes=None, temperature=None, bins=15):
        """Reliability of softmax(z / T): one evaluation forward over the labelled rows of `split` (1 train, 2 validation, 3 test) or,
        with split=None, of the `nodes` query with predict()'s conventions (None: every row), then the negative log-likelihood
        and the reliability diagram formed on the GPU.  temperature=None: the model's own.  Returns a dict: nll (mean), ece, mce,
        rows, and per bin (b / bins, (b + 1) / bins] count (int64), accuracy and confidence (float64, 0 for an empty bin).
        Single-label models, at most 64 classes, one rank.  Training state is not touched."""
        self._calib_args("calibration", bins=bins, temperature=temperature)
        if split is not None and nodes is not None:
            raise GcnHostError("calibration: give a split or a node query, not both")
        if split is not None and split not in (1, 2, 3):
            raise GcnHostError(f"calibration: split is 1 (train), 2 (validation) or 3 (test), got {split!r}")
        if nodes is None:
            n, qp = 0, None
        else:
            q = np.ascontiguousarray(nodes, np.int32).ravel()
            n = q.size
            q = q if n else np.zeros(1, np.int32)              # an empty query is still a query (not "every row")
            qp = q.ctypes.data
        t = self.temperature if temperature is None else float(temperature)
        sums = np.zeros(4, np.float64)
        count, correct, conf = np.zeros(bins, np.int64), np.zeros(bins, np.int64), np.zeros(bins, np.float64)
        _ck(self.lib, self.lib.gcnhost_model_calibration(self.h, int(split or 0), qp, n, t, int(bins), sums.ctypes.data, count.ctypes.data,
                                                         correct.ctypes.data, conf.ctypes.data), "calibration")
        out = calibration_report(count, correct, conf)
        out.update(nll=float(sums[0] / sums[3]) if sums[3] else 0.0, temperature=t, sums=sums)
        return out

    # ---- Monte Carlo dropout: how sure the model itself is about one node
    MC_SAMPLES_MAX = 1024

    @property
    def stream_seed(self):
        """the 64-bit seed of the model's dropout streams (host/gcn_build.cpp derives it from the constructor's seed):
        mc_dropout(seed=stream_seed, first_sample=e) draws the masks of training epoch e"""
        return ((self.seed & ((1 << 64) - 1)) * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & ((1 << 64) - 1)

    def _mc_args(self, split, nodes, samples, p, seed, first_sample):
        """argument checks that need no GPU"""
        what = "mc_dropout"
        if self.multilabel:
            raise GcnHostError(f"{what}: this is a multi-label model (the call works on one softmax per node)")
        if self.params.output_dim > 64:
            raise GcnHostError(f"{what}: at most 64 classes, this model has {self.params.output_dim}")
        if self.params.hidden_dim > 256:
            raise GcnHostError(f"{what}: a hidden width of at most 256, this model has {self.params.hidden_dim}")
        if split is not None and nodes is not None:
            raise GcnHostError(f"{what}: give a split or a node query, not both")
        if split is not None and split not in (1, 2, 3):
            raise GcnHostError(f"{what}: split is 1 (train), 2 (validation) or 3 (test), got {split!r}")
        if isinstance(samples, bool) or int(samples) != samples or not 1 <= samples <= self.MC_SAMPLES_MAX:
            raise GcnHostError(f"{what}: samples must be an integer in 1..{self.MC_SAMPLES_MAX}, got {samples!r}")
        if p is not None and not 0.0 <= float(p) < 1.0:
            raise GcnHostError(f"{what}: the dropout rate p must be in [0, 1), got {p!r}")
        if seed is not None and (int(seed) != seed or not 0 <= seed < 1 << 64):
            raise GcnHostError(f"{what}: the seed is an integer in [0, 2^64), got {seed!r}")
        if int(first_sample) != first_sample or first_sample < 0 or first_sample + samples > 1 << 32:
            raise GcnHostError(f"{what}: first_sample >= 0 and first_sample + samples <= 2^32, got {first_sample!r} + {samples!r}")

    def mc_dropout(self, split=None, nodes=None, samples=20, p=None, seed=None, first_sample=0, mean_prob=False, votes=False, return_samples=False):
        """Monte Carlo dropout (Gal & Ghahramani, 2016): `samples` forwards with dropout ON, their softmax rows averaged, and the
        predictive entropy split into its expected part and the mutual information between prediction and weights (BALD) — the
        part of a node's uncertainty that is the model's own.  Sample s in [first_sample, first_sample + samples) is the training
        forward with the epoch word s, the rate p (None: the model's dropout) and the 64-bit `seed` (None: the model's seed ^
        KEY_MC_DROPOUT, so that no sample repeats a training epoch's masks; the model's own seed with first_sample=e draws the
        masks of training epoch e).  Rows as in evaluate(): the nodes of `split`, or the `nodes` query (dataset ids, repeats
        allowed), or with both None every row.  Returns a dict by list position: pred (int32, the argmax of the mean softmax row,
        lowest class on a tie), confidence (its mean probability), entropy, expected_entropy, mutual_information, variation_ratio
        (f32, formed in float64 on the GPU), with mean_prob=True mean_prob f32 [n, C], with votes=True votes int32 [n, C], with
        return_samples=True samples_logp f32 [samples, n, C] (the per-sample log-softmax rows at the model's temperature), and
        seed, p, samples, first_sample as used.  Single-label models, at most 64 classes, hidden width at most 256, f32 tables,
        one rank.  Training state is not touched."""
        self._mc_args(split, nodes, samples, p, seed, first_sample)
        if nodes is None:
            q, n, listed = None, 0, self.info()["local_rows"]     # (a split lists at most that many rows)
        else:
            q = np.ascontiguousarray(nodes, np.int32).ravel()
            n = listed = q.size
            q = q if n else np.zeros(1, np.int32)              # an empty query is still a query (not "every row")
        c, s_count = self.params.output_dim, int(samples)
        rows = C.c_int64()
        pp = C.c_float(float(p)) if p is not None else None
        sp = C.c_uint64(int(seed)) if seed is not None else None
        args = (self.h, int(split or 0), q.ctypes.data if q is not None else None, n, s_count, C.byref(pp) if pp is not None else None,
                C.byref(sp) if sp is not None else None, int(first_sample))
        if split is not None:
            # the rows of a split are known to the model: a call without arrays checks the arguments and counts them, no more
            _ck(self.lib, self.lib.gcnhost_model_mc_dropout(*args, 0, *([None] * 11), C.byref(rows)), "mc_dropout")
            listed = rows.value
        cap = max(listed, 1)
        pred = np.zeros(cap, np.int32)
        f32 = {k: np.zeros(cap, np.float32) for k in ("confidence", "entropy", "expected_entropy", "mutual_information", "variation_ratio")}
        mp = np.zeros((cap, c), np.float32) if mean_prob else None
        vt = np.zeros((cap, c), np.int32) if votes else None
        sl = np.zeros((s_count, cap, c), np.float32) if return_samples else None
        su, pu = C.c_uint64(), C.c_float()
        _ck(self.lib, self.lib.gcnhost_model_mc_dropout(
            *args, cap, pred.ctypes.data, f32["confidence"].ctypes.data, f32["entropy"].ctypes.data, f32["expected_entropy"].ctypes.data,
            f32["mutual_information"].ctypes.data, f32["variation_ratio"].ctypes.data, mp.ctypes.data if mean_prob else None,
            vt.ctypes.data if votes else None, sl.ctypes.data if return_samples else None, C.byref(su), C.byref(pu), C.byref(rows)), "mc_dropout")
        k = rows.value
        out = dict(pred=pred[:k].copy(), seed=su.value, p=pu.value, samples=s_count, first_sample=int(first_sample))
        out.update({name: a[:k].copy() for name, a in f32.items()})
        if mean_prob:
            out["mean_prob"] = mp[:k].copy()
        if votes:
            out["votes"] = vt[:k].copy()
        if return_samples:
            out["samples_logp"] = sl[:, :k].copy()
        return out

    # ---- split conformal prediction: a set of classes per node that holds the true one with probability >= 1 - alpha
    CONFORMAL_METHODS = {"lac": 0, "aps": 1}

    def _conformal_query(self, what, split, nodes):
        if split is not None and nodes is not None:
            raise GcnHostError(f"{what}: give a split or a node query, not both")
        if split is not None and split not in (1, 2, 3):
            raise GcnHostError(f"{what}: split is 1 (train), 2 (validation) or 3 (test), got {split!r}")
        if nodes is None:
            return None, 0, self.info()["local_rows"]          # (a split lists at most that many rows)
        q = np.ascontiguousarray(nodes, np.int32).ravel()
        n = q.size
        return (q if n else np.zeros(1, np.int32)), n, n       # an empty query is still a query (not "every row")

    def _conformal_struct(self, fit):
        """the dict conformal_fit returned -> the C struct"""
        c = self.params.output_dim
        if c > 64:
            raise GcnHostError(f"conformal_sets: at most 64 classes, this model has {c}")
        s = _ConformalFit()
        try:
            s.method = self.CONFORMAL_METHODS[fit["method"]]
            s.lam, s.k_reg, s.diffusion, s.temperature = float(fit["lam"]), int(fit["k_reg"]), float(fit["diffusion"]), float(fit["temperature"])
            s.alpha, s.per_class = float(fit["alpha"]), int(bool(fit["per_class"]))
            th = np.ascontiguousarray(fit["thresh"], np.float32).ravel()
            nc = np.ascontiguousarray(fit["n_cal"], np.int64).ravel()
        except (KeyError, TypeError) as e:
            raise GcnHostError(f"conformal_sets: not a fit as conformal_fit returns it ({e!r})") from None
        if th.size != c or nc.size != c:
            raise GcnHostError(f"conformal_sets: the fit holds {th.size} thresholds, the model has {c} classes")
        for j in range(c):
            s.thresh[j], s.n_cal[j] = float(th[j]), int(nc[j])
        return s

    def conformal_fit(self, alpha=0.1, split=2, nodes=None, method="aps", lam=0.0, k_reg=0, diffusion=0.0, per_class=False, return_scores=False):
        """Split conformal prediction: fits the threshold of the prediction sets on the labelled rows of `split` (the validation
        split; or, with split=None, of the `nodes` query) so that a set holds the true class with probability >= 1 - alpha.
        method "lac": the score of class j is 1 - p_j; "aps": the probability cumulated from the most likely class down to j,
        plus the RAPS penalty lam . max(0, rank_j + 1 - k_reg).  diffusion d in (0, 1]: the scores are blended with their
        neighbourhood mean, d . A^ . S + (1 - d) . S.  per_class: one threshold per label (class-conditional coverage).  One
        evaluation forward, the scores formed on the GPU at the model's temperature, one float per row to the host and the
        quantile rule of conformal_quantile() there.  Returns a dict: method, lam, k_reg, diffusion, temperature, alpha,
        per_class, thresh (f32 [C]; +inf: too few rows for this alpha), n_cal (int64 [C]), threshold (thresh[0] unless per_class),
        and with return_scores=True scores (f32 per listed row, -1 for a row without a label).  Single-label models, at most 64
        classes, one rank.  Training state is not touched."""
        if method not in self.CONFORMAL_METHODS:
            raise GcnHostError(f"conformal_fit: the method is 'aps' or 'lac', got {method!r}")
        q, n, listed = self._conformal_query("conformal_fit", split, nodes)
        s = _ConformalFit()
        sc = np.zeros(max(listed, 1), np.float32)
        ns = C.c_int64()
        _ck(self.lib, self.lib.gcnhost_model_conformal_fit(self.h, int(split or 0), q.ctypes.data if q is not None else None, n, float(alpha),
                                                           self.CONFORMAL_METHODS[method], float(lam), int(k_reg), float(diffusion), int(bool(per_class)),
                                                           C.addressof(s), sc.ctypes.data, sc.size, C.byref(ns)), "conformal_fit")
        c = self.params.output_dim
        out = dict(method=method, lam=float(s.lam), k_reg=int(s.k_reg), diffusion=float(s.diffusion), temperature=float(s.temperature),
                   alpha=float(s.alpha), per_class=bool(s.per_class), thresh=np.array(s.thresh[:c], np.float32), n_cal=np.array(s.n_cal[:c], np.int64))
        if not out["per_class"]:
            out["threshold"] = float(out["thresh"][0])
        if return_scores:
            out["scores"] = sc[:ns.value].copy()
        return out

    def predict_sets(self, fit, nodes=None):
        """(sets bool [n, C], size int32 [n]) — the conformal prediction set of every queried node under `fit` (conformal_fit's
        dict): class j is in the set iff its score is <= the threshold.  nodes as in predict().  Refused when the model's
        temperature is not the one the fit was made at.  Training state is not touched."""
        from .ops import unpack_multihot
        q, n, listed = self._conformal_query("predict_sets", None, nodes)
        c = self.params.output_dim
        words = np.zeros((max(listed, 1), (c + 31) // 32), np.uint32)
        size = np.zeros(max(listed, 1), np.int32)
        s = self._conformal_struct(fit)
        _ck(self.lib, self.lib.gcnhost_model_conformal_sets(self.h, C.addressof(s), 0, q.ctypes.data if q is not None else None, n, words.ctypes.data,
                                                            size.ctypes.data, None), "predict_sets")
        return unpack_multihot(words[:listed], c), size[:listed]

    def coverage(self, fit, split=3, nodes=None):
        """How the sets of `fit` do on the labelled rows of `split` (the test split; or, with split=None, of the `nodes` query):
        counted on the GPU, only 4 + 3 C + 1 integers cross.  Returns a dict: rows, labelled, covered (labelled rows whose set holds
        their label), coverage = covered / labelled, mean_size (over all rows), empty, size_hist (int64 [C + 1]), class_support and
        class_covered (int64 [C])."""
        q, n, _ = self._conformal_query("coverage", split, nodes)
        c = self.params.output_dim
        cnt = np.zeros(4 + 3 * c + 1, np.int64)
        s = self._conformal_struct(fit)
        _ck(self.lib, self.lib.gcnhost_model_conformal_sets(self.h, C.addressof(s), int(split or 0), q.ctypes.data if q is not None else None, n, None,
                                                            None, cnt.ctypes.data), "coverage")
        hist = cnt[4:4 + c + 1].copy()
        rows, labelled, covered = int(cnt[0]), int(cnt[1]), int(cnt[2])
        return dict(rows=rows, labelled=labelled, covered=covered, coverage=covered / labelled if labelled else 0.0,
                    mean_size=float((hist * np.arange(c + 1)).sum() / rows) if rows else 0.0, empty=int(cnt[3]), size_hist=hist,
                    class_support=cnt[4 + c + 1:4 + 2 * c + 1].copy(), class_covered=cnt[4 + 2 * c + 1:].copy())

    # ---- node embeddings: the hidden layer H1 = ReLU(A^.X.W1), queried on the GPU
    METRICS = {"dot": 0, "cosine": 1}

    def _embed_args(self, what, metric="dot", k=1, **node_lists):
        """argument checks that need no GPU; returns the metric's code and the node lists as int32 arrays"""
        if metric not in self.METRICS:
            raise GcnHostError(f"{what}: the metric is 'dot' or 'cosine', got {metric!r}")
        if not (isinstance(k, (int, np.integer)) and not isinstance(k, bool) and 1 <= k <= 64):
            raise GcnHostError(f"{what}: k must be an integer in 1..64, got {k!r}")
        if self.params.hidden_dim > 256:
            raise GcnHostError(f"{what}: a hidden width of at most 256, this model has {self.params.hidden_dim}")
        out = []
        for name, nodes in node_lists.items():
            q = np.ascontiguousarray(nodes, np.int32).ravel()
            if q.size and (q.min() < 0 or q.max() >= self.params.num_nodes):
                raise GcnHostError(f"{what}: {name} holds an id that is not a node of the dataset (0..{self.params.num_nodes - 1})")
            out.append(q)
        return [self.METRICS[metric]] + out

    def embed(self, nodes=None, normalize=False):
        """float32 [n, hidden_dim] — the rows of the hidden layer H1 = ReLU(A^.X.W1) of an evaluation forward with the current
        weights (no dropout) for the listed dataset node ids (repeats allowed; None: every node, in id order), gathered on the
        GPU so that only these rows cross.  The values are var(3)'s: a factored model (row_scale()) keeps 1/sqrt(deg) of the
        node on its row.  normalize=True: each row divided by its Euclidean norm (an all-zero row stays zero).  One rank, hidden
        width at most 256.  Training state is not touched."""
        if nodes is None:
            n, qp = self.params.num_nodes, None
        else:
            _, q = self._embed_args("embed", nodes=nodes)
            n, q = q.size, (q if q.size else np.zeros(1, np.int32))         # an empty query is still a query (not "every node")
            qp = q.ctypes.data
        out = np.zeros((max(n, 1), self.params.hidden_dim), np.float32)
        _ck(self.lib, self.lib.gcnhost_model_embed(self.h, qp, n, out.ctypes.data, int(bool(normalize))), "embed")
        return out[:n]

    def similar(self, nodes, k=10, metric="cosine", exclude_self=True):
        """(ids int32 [n, k], scores float32 [n, k]) — for each listed node (None: every node) the k nodes of the graph whose
        embed() rows score highest against its own: metric "dot" (the f32 dot product) or "cosine"; best first, equal scores by
        ascending node id; without the node itself unless exclude_self=False.  Slots past the last candidate hold -1 / -inf.  The
        n x N x hidden product and the selection run on the GPU; only the answer crosses.  1 <= k <= 64."""
        if nodes is None:
            code, = self._embed_args("similar", metric, k)
            n, qp = self.params.num_nodes, None
        else:
            code, q = self._embed_args("similar", metric, k, nodes=nodes)
            n, q = q.size, (q if q.size else np.zeros(1, np.int32))
            qp = q.ctypes.data
        ids = np.zeros((max(n, 1), k), np.int32)
        scores = np.zeros((max(n, 1), k), np.float32)
        _ck(self.lib, self.lib.gcnhost_model_similar(self.h, qp, n, int(k), code, int(bool(exclude_self)), ids.ctypes.data, scores.ctypes.data), "similar")
        return ids[:n], scores[:n]

    def score_edges(self, src, dst, metric="dot"):
        """float32 [m] — the score of every listed node pair (src[i], dst[i]) under the metric: candidate edges ranked by the
        embeddings of their ends.  src[i] == dst[i] is allowed (cosine: about 1, or 0 for a zero row)."""
        code, s, d = self._embed_args("score_edges", metric, src=src, dst=dst)
        if s.size != d.size:
            raise GcnHostError(f"score_edges: {s.size} sources for {d.size} destinations")
        out = np.zeros(max(s.size, 1), np.float32)
        z = np.zeros(1, np.int32)
        _ck(self.lib, self.lib.gcnhost_model_score_pairs(self.h, (s if s.size else z).ctypes.data, (d if d.size else z).ctypes.data, int(s.size), code,
                                                         out.ctypes.data), "score_edges")
        return out[:s.size]

    # ---- k-means on the hidden layer: groups of nodes, on the GPU
    def _cluster_args(self, k, split, nodes, iters, init, seed):
        """argument checks that need no GPU; returns (k, init code, init positions or None, init centres or None)"""
        what = "cluster"
        if self.params.hidden_dim > 256:
            raise GcnHostError(f"{what}: a hidden width of at most 256, this model has {self.params.hidden_dim}")
        if split is not None and nodes is not None:
            raise GcnHostError(f"{what}: give a split or a node query, not both")
        if split is not None and split not in (1, 2, 3):
            raise GcnHostError(f"{what}: split is 1 (train), 2 (validation) or 3 (test), got {split!r}")
        k = self.params.output_dim if k is None else k
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 256:
            raise GcnHostError(f"{what}: k must be an integer in 1..256, got {k!r}")
        if isinstance(iters, bool) or int(iters) != iters or iters < 1:
            raise GcnHostError(f"{what}: iters must be an integer >= 1, got {iters!r}")
        if seed is not None and (int(seed) != seed or not 0 <= seed < 1 << 64):
            raise GcnHostError(f"{what}: the seed is an integer in [0, 2^64), got {seed!r}")
        if isinstance(init, str):
            if init != "kmeans++":
                raise GcnHostError(f"{what}: init is 'kmeans++', an int array of k row positions or a float [k, hidden] array, got {init!r}")
            return int(k), 0, None, None
        arr = np.asarray(init)
        if arr.dtype.kind in "iu":
            if arr.shape != (k,):
                raise GcnHostError(f"{what}: init positions must have shape ({k},), got {arr.shape}")
            return int(k), 1, np.ascontiguousarray(arr, np.int32), None
        if arr.dtype.kind != "f" or arr.shape != (k, self.params.hidden_dim):
            raise GcnHostError(f"{what}: init centres must be a float array of shape ({k}, {self.params.hidden_dim}), got {arr.dtype} {arr.shape}")
        return int(k), 2, None, np.ascontiguousarray(arr, np.float32)

    def cluster(self, k=None, split=None, nodes=None, iters=100, normalize=True, init="kmeans++", seed=None, report=True, scratch_bytes=0):
        """k-means (Lloyd) on the rows embed() exports, run where they lie: one evaluation forward, k-means++ seeding by an
        exponential race on a Philox stream, then assignment (an n x k x hidden product on the exact-f32 MFMA with the row-wise
        argmin behind it) and update (float64 means in a summation order fixed by the data) until an assignment moves nothing or
        `iters` are made — the same answer, bit for bit, on every run.  Rows: the nodes of `split` in ascending id, or the `nodes`
        query (dataset ids in the order given, repeats allowed), or with both None every node in id order.  k: None = output_dim.
        normalize=True clusters unit rows (cosine geometry); it is the default because a factored model (row_scale()) keeps
        1/sqrt(deg) of the node on its stored row — with normalize=False the clustering is of the STORED rows, as similar()'s
        "dot" is.  init: "kmeans++", an int array of k list positions whose rows start as centres, or a float [k, hidden] array.
        seed: the 64-bit seed of the seeding draws (None: the model's stream_seed).  Returns a dict: assign int32 [n] and dist2
        f32 [n] by list position (squared distance to the centre the row was assigned to), centers f32 [k, hidden] (the means of
        the returned assignment; an empty cluster keeps its centre), sizes int32 [k], seed_pos (list positions, None unless
        seeded), iters_run, converged, history float64 [iters_run, 2] = (moved, inertia) per iteration, inertia, seed.  With
        report=True on a single-label model with at most 64 classes also contingency int64 [k, C] against the dataset's labels,
        counted on the GPU, skipped (rows without a label in [0, C)) and cluster_report()'s scores.  One rank, hidden width at
        most 256, f32 tables, k at most the rows listed.  Training state is not touched."""
        k, code, ipos, icen = self._cluster_args(k, split, nodes, iters, init, seed)
        if nodes is None:
            q, n, cap = None, 0, self.params.num_nodes
        else:
            q = np.ascontiguousarray(nodes, np.int32).ravel()
            n = cap = q.size
            q = q if n else np.zeros(1, np.int32)
        h, c = self.params.hidden_dim, self.params.output_dim
        want_report = bool(report) and not self.multilabel and c <= 64
        assign, dist2 = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float32)
        centers, sizes, pos = np.zeros((k, h), np.float32), np.zeros(k, np.int32), np.zeros(k, np.int32)
        hist = np.zeros((int(iters), 2), np.float64)
        cont = np.zeros((k, c), np.int64) if want_report else None
        info, inertia, su = np.zeros(4, np.int64), C.c_double(), C.c_uint64()
        sp = C.c_uint64(int(seed)) if seed is not None else None
        _ck(self.lib, self.lib.gcnhost_model_kmeans(
            self.h, k, int(split or 0), q.ctypes.data if q is not None else None, n, int(iters), int(bool(normalize)), code,
            ipos.ctypes.data if ipos is not None else None, icen.ctypes.data if icen is not None else None,
            C.byref(sp) if sp is not None else None, int(scratch_bytes), cap, assign.ctypes.data, dist2.ctypes.data, centers.ctypes.data,
            sizes.ctypes.data, pos.ctypes.data if code == 0 else None, hist.ctypes.data, cont.ctypes.data if want_report else None,
            info.ctypes.data, C.byref(inertia), C.byref(su)), "cluster")
        rows, run = int(info[0]), int(info[1])
        out = dict(assign=assign[:rows].copy(), dist2=dist2[:rows].copy(), centers=centers, sizes=sizes, seed_pos=pos if code == 0 else None,
                   iters_run=run, converged=bool(info[2]), history=hist[:run].copy(), inertia=inertia.value, seed=su.value)
        if want_report:
            out.update(contingency=cont, skipped=int(info[3]))
            out.update(cluster_report(cont))
        return out

    # ---- silhouette widths of a clustering of the hidden layer: is this k a good one, which nodes sit badly, on the GPU
    def silhouette(self, labels, k=None, split=None, nodes=None, normalize=True, per_node=True, scratch_bytes=0):
        """Silhouette widths (Rousseeuw, 1987; scikit-learn's silhouette_samples, euclidean) of a labelling of the rows embed()
        exports, computed where they lie: one evaluation forward, then for every listed row its summed distance to the points of
        every label — an n x n x hidden product on the exact-f32 MFMA with a correctly rounded square root behind every entry,
        added in float64 in an order fixed by the data: the same bits on every run and with every scratch size.  Rows: the nodes
        of `split` in ascending id, or the `nodes` query (dataset ids in the order given, a repeat is a point of its own), or
        with both None every node in id order.  labels: int [n] by LIST POSITION, exactly what cluster(split=..., nodes=...)
        ["assign"] is for the same arguments; k: None = labels.max() + 1.  A label outside [0, k) takes its position out of the
        points.  normalize=True measures unit rows, for the reason cluster() does (row_scale()).  Returns a dict: score (the mean
        width over the points), cluster_mean float64 [k] (0 for an empty label), sizes int32 [k], points, excluded, defined (at
        least two non-empty labels; otherwise every width is 0), and with per_node=True s, a, b float64 [n] (the width, the mean
        distance inside the own label, the lowest mean distance to another label) and neighbor int32 [n] (that label, the
        lowest on equal means; -1 when none); NaN / -1 at an excluded position.  scratch_bytes caps the device scratch of the
        sums (0: 256 MiB; less: more launches, the same bits).  One rank, hidden width at most 256, f32 tables.  Training state
        is not touched and nothing is cached."""
        what = "silhouette"
        q, n, cap = self._pca_query(what, split, nodes)
        lab = np.asarray(labels)
        if lab.dtype.kind not in "iu" or lab.ndim != 1:
            raise GcnHostError(f"{what}: labels must be a one-dimensional integer array, got {lab.dtype} {lab.shape}")
        if k is None:
            k = int(lab.max()) + 1 if lab.size else 1
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 256:
            raise GcnHostError(f"{what}: k must be an integer in 1..256, got {k!r}")
        if split is None and lab.size != cap:
            raise GcnHostError(f"{what}: the query lists {cap} rows, the labels are {lab.size}")
        lab = np.ascontiguousarray(np.clip(lab, -1, 256), np.int32)
        m = int(lab.size)
        k = int(k)
        lp = lab if m else np.zeros(1, np.int32)
        s, a, b = (np.zeros(max(m, 1), np.float64) for _ in range(3)) if per_node else (None, None, None)
        nb = np.zeros(max(m, 1), np.int32) if per_node else None
        cmean, sizes, info, score = np.zeros(k, np.float64), np.zeros(k, np.int32), np.zeros(5, np.int64), C.c_double()
        _ck(self.lib, self.lib.gcnhost_model_silhouette(
            self.h, int(split or 0), q.ctypes.data if q is not None else None, n, lp.ctypes.data, k, int(bool(normalize)), int(scratch_bytes), m,
            s.ctypes.data if per_node else None, a.ctypes.data if per_node else None, b.ctypes.data if per_node else None,
            nb.ctypes.data if per_node else None, cmean.ctypes.data, sizes.ctypes.data, info.ctypes.data, C.byref(score)), what)
        out = dict(score=score.value, cluster_mean=cmean, sizes=sizes, points=int(info[1]), excluded=int(info[2]), defined=bool(info[4]))
        if per_node:
            out.update(s=s[:m], a=a[:m], b=b[:m], neighbor=nb[:m])
        return out

    # ---- principal components of the hidden layer: coordinates, spectrum and whitening, on the GPU
    def _pca_query(self, what, split, nodes):
        if self.params.hidden_dim > 256:
            raise GcnHostError(f"{what}: a hidden width of at most 256, this model has {self.params.hidden_dim}")
        if split is not None and nodes is not None:
            raise GcnHostError(f"{what}: give a split or a node query, not both")
        if split is not None and split not in (1, 2, 3):
            raise GcnHostError(f"{what}: split is 1 (train), 2 (validation) or 3 (test), got {split!r}")
        if nodes is None:
            return None, 0, self.params.num_nodes
        q = np.ascontiguousarray(nodes, np.int32).ravel()
        return (q if q.size else np.zeros(1, np.int32)), int(q.size), int(q.size)

    def pca(self, k=2, split=None, nodes=None, normalize=True, center=True, whiten=False, coords=True, return_scatter=False, scratch_bytes=0):
        """Principal component analysis of the rows embed() exports, run where they lie: one evaluation forward, the float64 mean
        and the float64 scatter matrix of the listed rows on the GPU (the f64 MFMA, a summation order fixed by the data: the same
        bits on every run), hidden + hidden^2 doubles to the host, the symmetric eigenproblem there (sym_eigen), and the
        projection of the rows onto the leading k components on the GPU.  Rows: the nodes of `split` in ascending id, or the
        `nodes` query (dataset ids in the order given, repeats counted as often as listed), or with both None every node in id
        order.  normalize=True analyses unit rows (see cluster()); center=False analyses the uncentred Gram matrix; whiten=True
        scales every coordinate to unit sample variance (0 for a component past the rank).  Returns a dict: mean float64 [h],
        components float64 [k, h] (unit rows, the entry of largest magnitude positive), eigenvalues float64 [h] (descending,
        clipped at 0), explained_variance, explained_variance_ratio, singular_values float64 [h], rank, rows, normalize, center,
        whiten, scale (float64 [k] with whiten, else None), coords f32 [rows, k] by list position (None with coords=False) and
        with return_scatter=True scatter float64 [h, h].  pca_transform() applies the fit to other nodes.  One rank, hidden width
        at most 256, f32 tables, at least 2 rows.  Training state is not touched."""
        what = "pca"
        q, n, cap = self._pca_query(what, split, nodes)
        h = self.params.hidden_dim
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= h:
            raise GcnHostError(f"{what}: k must be an integer in 1..{h}, got {k!r}")
        k = int(k)
        mean, ev, comp, expl = np.zeros(h, np.float64), np.zeros(h, np.float64), np.zeros((h, h), np.float64), np.zeros((3, h), np.float64)
        scat = np.zeros((h, h), np.float64) if return_scatter else None
        scale = np.zeros(k, np.float64) if whiten else None
        y = np.zeros(max(cap, 1) * k, np.float32) if coords else None
        info = np.zeros(3, np.int64)
        _ck(self.lib, self.lib.gcnhost_model_pca_fit(
            self.h, k, int(split or 0), q.ctypes.data if q is not None else None, n, int(bool(normalize)), int(bool(center)), int(bool(whiten)),
            int(scratch_bytes), cap, mean.ctypes.data, scat.ctypes.data if return_scatter else None, ev.ctypes.data, comp.ctypes.data,
            expl.ctypes.data, scale.ctypes.data if whiten else None, y.ctypes.data if coords else None, info.ctypes.data), what)
        rows = int(info[0])
        out = dict(mean=mean, components=comp[:k].copy(), eigenvalues=ev, explained_variance=expl[0].copy(), explained_variance_ratio=expl[1].copy(),
                   singular_values=expl[2].copy(), rank=int(info[1]), rows=rows, normalize=bool(normalize), center=bool(center), whiten=bool(whiten),
                   scale=scale, coords=y[:rows * k].reshape(rows, k).copy() if coords else None)
        if return_scatter:
            out["scatter"] = scat
        return out

    def pca_transform(self, fit, nodes=None):
        """f32 [n, k] — the listed nodes (None: every node in id order) projected with a fit pca() returned, at the CURRENT
        weights: one evaluation forward and one projection launch on the GPU; nothing is cached.  A fit on the training split
        places every node.  Refused when the fit has another width than the hidden layer or holds a value that is not finite."""
        what = "pca_transform"
        q, n, cap = self._pca_query(what, None, nodes)
        comp = np.ascontiguousarray(fit["components"], np.float64)
        if comp.ndim != 2:
            raise GcnHostError(f"{what}: components must be a [k, hidden] array, got shape {comp.shape}")
        k, width = comp.shape
        mean = np.ascontiguousarray(fit["mean"], np.float64).ravel() if fit.get("center", True) else None
        if mean is not None and mean.size != width:
            raise GcnHostError(f"{what}: the mean has {mean.size} entries, the components {width}")
        scale = fit.get("scale") if fit.get("whiten", False) else None
        if scale is not None:
            scale = np.ascontiguousarray(scale, np.float64).ravel()
            if scale.size != k:
                raise GcnHostError(f"{what}: the scale has {scale.size} entries for {k} components")
        y = np.zeros((max(cap, 1), max(k, 1)), np.float32)
        _ck(self.lib, self.lib.gcnhost_model_pca_project(
            self.h, int(width), int(k), mean.ctypes.data if mean is not None else None, comp.ctypes.data, scale.ctypes.data if scale is not None else None,
            int(bool(fit.get("normalize", True))), q.ctypes.data if q is not None else None, n, y.ctypes.data), what)
        return y[:cap]

    # ---- label structure of the graph: homophily, class mixing, accuracy by degree and by neighbourhood agreement, on the GPU
    def _structure_query(self, what, split, nodes):
        """argument checks that need no GPU; returns (split code, node ids int32 or None, n, capacity)"""
        if split is not None and nodes is not None:
            raise GcnHostError(f"{what}: give a split or a node query, not both")
        if split is not None and split not in (1, 2, 3):
            raise GcnHostError(f"{what}: split is 1 (train), 2 (validation) or 3 (test), got {split!r}")
        if nodes is None:
            return int(split or 0), None, 0, self.params.num_nodes
        q = np.ascontiguousarray(nodes, np.int32).ravel()
        return 0, (q if q.size else np.zeros(1, np.int32)), int(q.size), int(q.size)

    def neighbor_agreement(self, labels, num_classes=None, split=None, nodes=None, per_node=False):
        """How far a labelling agrees with itself over the model's graph, counted on the GPU in one walk over the adjacency's index
        stream (csrc/structure.hip has the definitions).  labels: ANY int array [num_nodes] in dataset node order — the dataset's
        labels, predict()'s output, cluster()["assign"] — with x known when 0 <= x < num_classes (None: the model's classes; at
        most 64).  Rows: the nodes of `split` in ascending id, or the `nodes` query (dataset ids, repeats counted as often as
        listed), or with both None every node.  Per listed node: deg = its stored neighbours without the self loop, known = those
        with a known label, same = those of them with the node's own label.  Returns structure_metrics() of the counts
        (edge_homophily, node_homophily, adjusted_homophily, class_insensitive_homophily, class_homophily [C], compatibility
        [C, C], ...) plus mix int64 [C, C], class_rows int64 [C], totals int64 [8], rows, and with per_node=True deg / same / known
        int32 [rows] by list position.  Needs neither weights nor a forward; single- and multi-label models alike; one rank.
        Training state is not touched."""
        what = "neighbor_agreement"
        c = self.params.output_dim if num_classes is None else num_classes
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 1 <= c <= 64:
            raise GcnHostError(f"{what}: num_classes must be an integer in 1..64, got {c!r}")
        lab = np.asarray(labels)
        if lab.dtype.kind not in "iu" or lab.ndim != 1 or lab.size != self.params.num_nodes:
            raise GcnHostError(f"{what}: labels must be an int array of shape ({self.params.num_nodes},), got {lab.dtype} {lab.shape}")
        lab = np.ascontiguousarray(np.clip(lab.astype(np.int64), -1, 2**31 - 1), np.int32)
        code, q, n, cap = self._structure_query(what, split, nodes)
        c = int(c)
        per = [np.zeros(max(cap, 1), np.int32) for _ in range(3)] if per_node else [None] * 3
        mix, rows_c, totals, info = np.zeros((c, c), np.int64), np.zeros(c, np.int64), np.zeros(8, np.int64), np.zeros(2, np.int64)
        _ck(self.lib, self.lib.gcnhost_model_neighbor_agreement(
            self.h, lab.ctypes.data, lab.size, c, code, q.ctypes.data if q is not None else None, n, cap,
            *[a.ctypes.data if a is not None else None for a in per], mix.ctypes.data, rows_c.ctypes.data, totals.ctypes.data, info.ctypes.data), what)
        out = structure_metrics(mix, rows_c, totals)
        out.update(mix=mix, class_rows=rows_c, totals=totals, rows=int(info[0]))
        if per_node:
            out.update(deg=per[0][:out["rows"]].copy(), same=per[1][:out["rows"]].copy(), known=per[2][:out["rows"]].copy())
        return out

    def structure_report(self, split=None, nodes=None, bins=10, predicted=True, per_node=False):
        """Where on the graph the model is right: the label structure of the graph it was given, of its own predictions, and its
        accuracy by degree and by neighbourhood agreement — the two stratifications of a GCN's errors.  Rows as
        neighbor_agreement() takes them.  One agreement launch on the dataset's labels; with predicted=True (single-label models)
        one evaluation forward, one agreement launch on the predicted classes and one strata launch with agreement measured on
        the TRUTH.  Returns a dict: truth and pred (None without predicted), each structure_metrics() of that labelling plus
        mix, class_rows, totals; strata int64 [32, bins + 1, 2] = (rows, rows predicted right) per degree bucket (0: degree 0,
        b: 2^(b-1) .. 2^b - 1) and agreement bucket (a < bins: a / bins <= same / known < (a + 1) / bins, the last closed at 1;
        bins: no labelled neighbour); by_degree / by_agreement: lists of dict(lo, hi, rows, correct, accuracy);
        pred_vs_truth_edge_homophily = pred's edge homophily minus the truth's (above 0: the predictions are smoother over the
        edges than the labels are); rows, unlabelled; with per_node=True deg / same / known int32 [rows] of the truth by list
        position.  Only the count tables cross to the host.  One rank, at most 64 classes.  Training state is not touched."""
        what = "structure_report"
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= 32:
            raise GcnHostError(f"{what}: bins must be an integer in 1..32, got {bins!r}")
        if predicted and self.multilabel:
            raise GcnHostError(f"{what}: predicted=True takes a single-label model (one predicted class per node)")
        code, q, n, cap = self._structure_query(what, split, nodes)
        c, bins = self.params.output_dim, int(bins)
        if c > 64:
            raise GcnHostError(f"{what}: at most 64 classes, this model has {c}")
        per = [np.zeros(max(cap, 1), np.int32) for _ in range(3)] if per_node else [None] * 3
        tabs = [(np.zeros((c, c), np.int64), np.zeros(c, np.int64), np.zeros(8, np.int64)) for _ in range(2)]
        strata, info = np.zeros((32, bins + 1, 2), np.int64), np.zeros(3, np.int64)
        _ck(self.lib, self.lib.gcnhost_model_structure(
            self.h, code, q.ctypes.data if q is not None else None, n, bins, int(bool(predicted)), cap,
            *[a.ctypes.data if a is not None else None for a in per], *[a.ctypes.data for a in tabs[0]], *[a.ctypes.data for a in tabs[1]],
            strata.ctypes.data, info.ctypes.data), what)

        def side(t, with_strata):
            d = structure_metrics(t[0], t[1], t[2], strata if with_strata else None, bins if with_strata else None)
            d.update(mix=t[0], class_rows=t[1], totals=t[2])
            return d
        truth = side(tabs[0], bool(predicted))
        out = dict(truth=truth, pred=None, strata=None, by_degree=None, by_agreement=None, pred_vs_truth_edge_homophily=None, bins=bins,
                   rows=int(info[0]), unlabelled=int(info[2]))
        if predicted:
            out.update(by_degree=truth.pop("by_degree"), by_agreement=truth.pop("by_agreement"), strata=strata, pred=side(tabs[1], False))
            truth.pop("strata_rows", None)
            out["pred_vs_truth_edge_homophily"] = out["pred"]["edge_homophily"] - truth["edge_homophily"]
        if per_node:
            out.update(deg=per[0][:out["rows"]].copy(), same=per[1][:out["rows"]].copy(), known=per[2][:out["rows"]].copy())
        return out

    # ---- reach of the labels: hops to the nearest labelled node, weak components, accuracy by that distance, on the GPU
    def _reach_sources(self, what, splits, source_nodes):
        """argument checks that need no GPU; returns (split mask, node ids int32 or None, n)"""
        if source_nodes is not None:
            s = np.ascontiguousarray(source_nodes, np.int32).ravel()
            return 0, (s if s.size else np.zeros(1, np.int32)), int(s.size)
        splits = (splits,) if isinstance(splits, (int, np.integer)) and not isinstance(splits, bool) else tuple(splits)
        if not splits or any(isinstance(s, bool) or not isinstance(s, (int, np.integer)) or s not in (1, 2, 3) for s in splits):
            raise GcnHostError(f"{what}: the source splits are 1 (train), 2 (validation), 3 (test), got {splits!r}")
        return sum({1 << int(s) for s in splits}), None, 0

    def label_distance(self, sources=(1,), source_nodes=None, split=None, nodes=None, max_hops=0, nearest=False):
        """How many hops every listed node is from the nearest source, found on the GPU by a level-synchronous breadth-first
        search over the model's adjacency (csrc/reach.hip has the definitions).  Sources: the nodes of the splits in `sources`
        (default: the training split), or the dataset ids in `source_nodes` (repeats allowed, an empty list: no source).  Rows:
        the nodes of `split` in ascending id, or the `nodes` query (dataset ids, repeats counted as often as listed), or with
        both None every node.  The distance follows an aggregation: a node gathers from the entries its stored row lists, so
        dist = 1 + the smallest dist among them, 0 for a source, -1 when no source reaches the node (or none within max_hops; 0:
        no limit) — the reach of label_propagation(), and for dist <= 2 of the two-layer model itself.  Returns a dict: dist int32
        [rows]; nearest int32 [rows] with nearest=True, else None: the source at distance dist with the lowest row (the node id,
        unless the model was given a node order), -1 when unreachable; levels (the largest distance in the graph), level_counts
        int64 [levels + 1] (nodes of the WHOLE graph per distance), unreachable (listed rows with dist -1), sources, rows.
        Single- and multi-label models alike; one rank.  Training state is not touched."""
        what = "label_distance"
        if isinstance(max_hops, bool) or not isinstance(max_hops, (int, np.integer)) or max_hops < 0:
            raise GcnHostError(f"{what}: max_hops must be an integer >= 0 (0: no limit), got {max_hops!r}")
        mask, s, ns = self._reach_sources(what, sources, source_nodes)
        code, q, n, cap = self._structure_query(what, split, nodes)
        dist = np.zeros(max(cap, 1), np.int32)
        near = np.zeros(max(cap, 1), np.int32) if nearest else None
        lc, info = np.zeros(self.params.num_nodes + 1, np.int64), np.zeros(5, np.int64)
        _ck(self.lib, self.lib.gcnhost_model_label_distance(
            self.h, mask, s.ctypes.data if s is not None else None, ns, code, q.ctypes.data if q is not None else None, n, int(max_hops), cap,
            dist.ctypes.data, near.ctypes.data if nearest else None, lc.ctypes.data, lc.size, info.ctypes.data), what)
        rows, levels = int(info[0]), int(info[4])
        return dict(dist=dist[:rows].copy(), nearest=near[:rows].copy() if nearest else None, levels=levels, level_counts=lc[:levels + 1].copy(),
                    unreachable=int(info[3]), sources=int(info[1]), rows=rows)

    def components(self, split=None, nodes=None, marked=(1,), marked_nodes=None):
        """The weakly connected components of the model's adjacency, labelled on the GPU (min-label hooking and pointer jumping,
        csrc/reach.hip): every stored entry joins its two ends, whichever row stores it.  Rows as label_distance() takes them.
        marked: the splits whose nodes count as marks (default: the training split), or marked_nodes: dataset ids — a component
        without a marked node holds no label to learn from.  Returns a dict: component int32 [rows] (the smallest node of the
        component) and size int32 [rows] per listed node; n_components, largest, unmarked_components, unmarked_nodes, marked_rows
        (of the WHOLE graph), rounds, rows.  Single- and multi-label models alike; one rank.  Training state is not touched."""
        what = "components"
        mask, s, ns = self._reach_sources(what, marked, marked_nodes)
        code, q, n, cap = self._structure_query(what, split, nodes)
        comp, size = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
        totals, info = np.zeros(6, np.int64), np.zeros(2, np.int64)
        _ck(self.lib, self.lib.gcnhost_model_components(
            self.h, code, q.ctypes.data if q is not None else None, n, mask, s.ctypes.data if s is not None else None, ns, cap, comp.ctypes.data,
            size.ctypes.data, totals.ctypes.data, info.ctypes.data), what)
        rows = int(info[0])
        return dict(component=comp[:rows].copy(), size=size[:rows].copy(), n_components=int(totals[1]), largest=int(totals[2]),
                    unmarked_components=int(totals[3]), unmarked_nodes=int(totals[4]), marked_rows=int(totals[5]), totals=totals, rounds=int(info[1]),
                    rows=rows)

    def reach_report(self, split=3, nodes=None, sources=(1,), source_nodes=None, hops=8, predicted=True, per_node=False):
        """How far the listed nodes (default: the test split) are from the labels the model learns from, and how its accuracy
        falls with that distance.  One traversal from the sources (label_distance() with nearest), the components with the sources
        as marks, with predicted=True (single-label models) one evaluation forward, and one strata launch.  Returns
        reach_metrics() of the strata — by_distance: a list of dict(rows, labelled, correct, nearest_correct, accuracy,
        nearest_label_accuracy) per bucket (b < hops: distance b; hops: further away; hops + 1: unreachable);
        inside_receptive_field / outside_receptive_field: the same over the rows within `layers` = min(2, hops - 1) hops and over
        the rest; all; unreachable, unreachable_share; nearest_label_accuracy ("copy the label of the nearest source") — plus the
        integers: strata int64 [hops + 2, 4], totals int64 [6], n_components, largest, unmarked_components, unmarked_nodes, levels,
        level_counts, sources, rounds, rows, unlabelled; with per_node=True dist / nearest / component int32 [rows].  Without
        predicted the `correct` counts are 0.  Only the count tables cross to the host.  One rank.  Training state is not touched."""
        what = "reach_report"
        if isinstance(hops, bool) or not isinstance(hops, (int, np.integer)) or not 1 <= hops <= 32:
            raise GcnHostError(f"{what}: hops must be an integer in 1..32, got {hops!r}")
        if predicted and self.multilabel:
            raise GcnHostError(f"{what}: predicted=True takes a single-label model (one predicted class per node)")
        mask, s, ns = self._reach_sources(what, sources, source_nodes)
        code, q, n, cap = self._structure_query(what, None if nodes is not None else split, nodes)
        hops = int(hops)
        per = [np.zeros(max(cap, 1), np.int32) for _ in range(3)] if per_node else [None] * 3
        strata, totals = np.zeros((hops + 2, 4), np.int64), np.zeros(6, np.int64)
        lc, info = np.zeros(self.params.num_nodes + 1, np.int64), np.zeros(7, np.int64)
        _ck(self.lib, self.lib.gcnhost_model_reach(
            self.h, code, q.ctypes.data if q is not None else None, n, mask, s.ctypes.data if s is not None else None, ns, hops, int(bool(predicted)), cap,
            *[a.ctypes.data if a is not None else None for a in per], strata.ctypes.data, totals.ctypes.data, lc.ctypes.data, lc.size,
            info.ctypes.data), what)
        rows, levels = int(info[0]), int(info[5])
        out = reach_metrics(strata, hops, min(2, hops - 1))
        out.update(strata=strata, totals=totals, n_components=int(totals[1]), largest=int(totals[2]), unmarked_components=int(totals[3]),
                   unmarked_nodes=int(totals[4]), levels=levels, level_counts=lc[:levels + 1].copy(), sources=int(info[1]), rounds=int(info[6]),
                   rows=rows, unlabelled=int(info[3]), predicted=bool(predicted))
        if per_node:
            out.update(dist=per[0][:rows].copy(), nearest=per[1][:rows].copy(), component=per[2][:rows].copy())
        return out

    # ---- explaining a logit: neighbour, hidden-unit and feature shares, on the GPU
    def _explain_args(self, what, nodes, classes=None):
        """argument checks that need no GPU; returns (node ids int32 or None, classes int32 or None)"""
        if self.params.hidden_dim > 256:
            raise GcnHostError(f"{what}: a hidden width of at most 256, this model has {self.params.hidden_dim}")
        q = None
        if nodes is not None:
            q = np.ascontiguousarray(nodes, np.int32).ravel()
            if q.size and (q.min() < 0 or q.max() >= self.params.num_nodes):
                raise GcnHostError(f"{what}: nodes holds an id that is not a node of the dataset (0..{self.params.num_nodes - 1})")
        c = None
        if classes is not None:
            c = np.ascontiguousarray(classes, np.int32).ravel()
            n = self.params.num_nodes if q is None else q.size
            if c.size != n:
                raise GcnHostError(f"{what}: {c.size} classes for {n} nodes")
            if c.size and (c.min() < 0 or c.max() >= self.params.output_dim):
                raise GcnHostError(f"{what}: classes holds a class the model does not have (0..{self.params.output_dim - 1})")
        return q, c

    def explain(self, nodes, classes=None, features=True, scratch_bytes=0):
        """Why the model gives a node its logit.  The network is Z = A^.(ReLU(A^.X.W1).W2) without bias, so with the ReLU gates
        of an evaluation forward fixed the logit of (node, class) is a plain sum, split here exactly three ways; every split adds
        up to the logit (the feature shares up to the first layer's own rounding).  nodes: dataset ids (repeats allowed; None:
        every node); classes: one per node, or None for each node's highest logit (lowest class on a tie; predict()'s class on a
        single-label model).  Returns a dict: logit f32 [n]; classes int32 [n]; hidden f32 [n, hidden_dim], the share of every
        hidden unit; features f32 [n, input_dim], the share of every input column (None when features=False); nbr_ptr int64
        [n + 1], nbr_ids int32, nbr_values f32: entries nbr_ptr[i] .. nbr_ptr[i + 1] - 1 are the shares of the stored edges of
        node i's row (dataset ids; the self loop included, a repeated edge twice).  scratch_bytes: device scratch of the feature
        shares (0: 64 MiB, the most); larger queries run in batches, same bits.  One rank, hidden width at most 256, f32 tables.
        Training state is not touched."""
        q, c = self._explain_args("explain", nodes, classes)
        n = self.params.num_nodes if q is None else int(q.size)
        z = np.zeros(1, np.int32)
        qp = None if q is None else (q if n else z).ctypes.data
        cp = None if c is None else (c if n else z).ctypes.data
        total = C.c_int64(0)
        _ck(self.lib, self.lib.gcnhost_model_explain(self.h, qp, cp, n, 0, None, None, None, None, None, None, None, C.byref(total)), "explain")
        h, nf = self.params.hidden_dim, self.params.input_dim
        out_c, logit = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float32)
        hidden = np.zeros((max(n, 1), h), np.float32)
        feat = np.zeros((max(n, 1), nf), np.float32) if features else None
        ptr = np.zeros(n + 1, np.int64)
        ids, vals = np.zeros(max(total.value, 1), np.int32), np.zeros(max(total.value, 1), np.float32)
        _ck(self.lib, self.lib.gcnhost_model_explain(self.h, qp, cp, n, int(scratch_bytes), out_c.ctypes.data, logit.ctypes.data, hidden.ctypes.data,
                                                     feat.ctypes.data if features else None, ptr.ctypes.data, ids.ctypes.data, vals.ctypes.data,
                                                     C.byref(total)), "explain")
        return dict(logit=logit[:n], classes=out_c[:n], hidden=hidden[:n], features=feat[:n] if features else None, nbr_ptr=ptr,
                    nbr_ids=ids[:total.value], nbr_values=vals[:total.value])

    def feature_importance(self, split=3, nodes=None, scratch_bytes=0):
        """(mean_abs float64 [C, input_dim], count int64 [C]) — the mean of |explain().features| over the nodes of `split` (1 train,
        2 validation, 3 test), or over `nodes` when given, each explained for its default class, grouped by that class: which
        input columns the model leans on for each class.  Formed on the GPU; only C x F numbers cross.  At most 256 classes."""
        q, _ = self._explain_args("feature_importance", nodes)
        if self.params.output_dim > 256:
            raise GcnHostError(f"feature_importance: at most 256 classes, this model has {self.params.output_dim}")
        if q is None and split not in (1, 2, 3):
            raise GcnHostError(f"feature_importance: split is 1 (train), 2 (validation) or 3 (test), got {split!r}")
        n = 0 if q is None else int(q.size)
        qp = None if q is None else (q if n else np.zeros(1, np.int32)).ctypes.data
        nc, nf = self.params.output_dim, self.params.input_dim
        mean_abs, count = np.zeros((nc, nf), np.float64), np.zeros(nc, np.int64)
        _ck(self.lib, self.lib.gcnhost_model_feature_importance(self.h, 0 if q is not None else int(split), qp, n, int(scratch_bytes), mean_abs.ctypes.data,
                                                                count.ctypes.data), "feature_importance")
        return mean_abs, count

    def save_weights(self, path):
        """W1, W2 to a weights file (read_weights; Adam's state is not saved)"""
        _ck(self.lib, self.lib.gcnhost_model_save_weights(self.h, os.fsencode(path)), "save_weights")

    def load_weights(self, path):
        """W1, W2 from a weights file whose widths match this model (else GcnHostError); Adam starts afresh"""
        _ck(self.lib, self.lib.gcnhost_model_load_weights(self.h, os.fsencode(path)), "load_weights")

    def schedule(self):
        """row schedule of the aggregation picked at construction: 'degree', 'label-major', 'dealt-<G>' or
        'structure-major (<G> groups)' — groups found in the graph by modularity local moving"""
        m, g = C.c_int(), C.c_int()
        _ck(self.lib, self.lib.gcnhost_model_schedule(self.h, C.byref(m), C.byref(g)), "schedule")
        return {0: "degree", 1: "label-major", 2: f"dealt-{g.value}", 3: f"structure-major ({g.value} groups)"}[m.value]

    def transport(self):
        """(name of the layer that moves rows between ranks, ranks that layer counts — ncclCommCount under RCCL)"""
        n, buf = C.c_int(), C.create_string_buffer(32)
        _ck(self.lib, self.lib.gcnhost_model_transport(self.h, C.byref(n), buf), "transport")
        return buf.value.decode(), n.value

    def slice_floats(self):
        """column-slice width (floats) of the XCD-sliced hidden-width aggregation, timed at load: 64 or 32"""
        f = C.c_int()
        _ck(self.lib, self.lib.gcnhost_model_slice_floats(self.h, C.byref(f)), "slice_floats")
        return f.value

    def timer(self, name_or_id):
        i = TIMER_NAMES.index(name_or_id) if isinstance(name_or_id, str) else int(name_or_id)
        s, n = C.c_double(), C.c_long()
        _ck(self.lib, self.lib.gcnhost_model_timer(self.h, i, C.byref(s), C.byref(n)), "timer")
        return s.value, n.value

    def timers_reset(self):
        _ck(self.lib, self.lib.gcnhost_model_timers_reset(self.h), "timers_reset")

    def set_timers(self, on):
        _ck(self.lib, self.lib.gcnhost_model_set_timers(self.h, int(bool(on))), "set_timers")

    def close(self):
        if self.h:
            self.lib.gcnhost_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def class_report(confusion=None, tp=None, fp=None, fn=None):
    """Per-class metrics from integer counts — host only, no GPU; the one place they are derived (host/report.h).  Either a
    confusion matrix [C, C] (row = truth, column = prediction) or the vectors tp, fp, fn [C].  Returns a dict: tp, fp, fn (int64
    [C]), support (= tp + fn), precision = tp / (tp + fp), recall = tp / (tp + fn), f1 = 2 tp / (2 tp + fp + fn) (float64 [C], each
    0 when its denominator is 0), macro_f1 (mean of f1 over all C classes, those without support included), micro_f1 =
    2 sum(tp) / (2 sum(tp) + sum(fp) + sum(fn)), accuracy (trace / sum of the matrix; 0.0 from vectors) and rows (sum of the
    matrix; 0 from vectors).  A non-square matrix or vectors of different lengths raise ValueError, a negative count GcnHostError."""
    vectors = [v for v in (tp, fp, fn) if v is not None]
    if (confusion is None) == (not vectors):
        raise ValueError("class_report: give either a confusion matrix or tp, fp and fn")
    if vectors and len(vectors) != 3:
        raise ValueError("class_report: tp, fp and fn go together")
    lib = _lib.gcnhost()
    if confusion is not None:
        m = np.ascontiguousarray(confusion, np.int64)
        if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1:
            raise ValueError(f"class_report: expected a square matrix [C, C] with C >= 1, got {m.shape}")
        c, args, rows = m.shape[0], (m.ctypes.data, None, None, None), int(m.sum()) if (m >= 0).all() else 0
    else:
        v = [np.ascontiguousarray(x, np.int64).ravel() for x in (tp, fp, fn)]
        if not (v[0].size == v[1].size == v[2].size) or v[0].size < 1:
            raise ValueError(f"class_report: tp, fp and fn must have one length C >= 1, got {[x.size for x in v]}")
        c, args, rows = v[0].size, (None, v[0].ctypes.data, v[1].ctypes.data, v[2].ctypes.data), 0
    cnt = np.zeros((3, c), np.int64)
    sup, pre, rec, f1 = (np.zeros(c, np.float64) for _ in range(4))
    summ = np.zeros(3, np.float64)
    _ck(lib, lib.gcnhost_class_report(c, *args, cnt.ctypes.data, sup.ctypes.data, pre.ctypes.data, rec.ctypes.data, f1.ctypes.data,
                                      summ.ctypes.data), "class_report")
    return dict(tp=cnt[0].copy(), fp=cnt[1].copy(), fn=cnt[2].copy(), support=sup, precision=pre, recall=rec, f1=f1,
                macro_f1=float(summ[0]), micro_f1=float(summ[1]), accuracy=float(summ[2]), rows=rows)


def thresholds_array(what, thresholds, num_classes):
    """f32 [C] from what a caller hands in as thresholds (an array, or the dict tune_thresholds() returns); a wrong length or a NaN
    raises ValueError"""
    if isinstance(thresholds, dict):
        thresholds = thresholds["threshold"]
    thr = np.ascontiguousarray(thresholds, np.float32).ravel()
    if thr.size != int(num_classes):
        raise ValueError(f"{what}: {thr.size} thresholds for {int(num_classes)} classes")
    if np.isnan(thr).any():
        raise ValueError(f"{what}: the threshold of class {int(np.flatnonzero(np.isnan(thr))[0])} is NaN")
    return thr


def new_node_rows(g_indptr, nbr_ptr, nbr_ids, m=None, factored=False):
    """The stored rows of m new nodes attached to a dataset's graph, host only (host/attach.h): the dataset has N =
    len(g_indptr) - 1 nodes, new node i has id N + i and the row [N + i, nbr_ids[nbr_ptr[i]:nbr_ptr[i + 1]]...] — the self loop
    first, then its listed ids in listed order, each in [0, N + m); repeats and one-way entries count as the loader counts them
    (degree = stored row length).  Returns dict(ptr int32 [m + 1], col int32, coef f32, len int32 [m]); coef[e] =
    1 / sqrt(len(v) . len(j)) as the adjacency object stores it, or with factored=True 1 / sqrt(len(v)) on every entry of row v
    (the factored model, whose tables carry the factor of their own row).  m: None = len(nbr_ptr) - 1.  Raises GcnHostError with
    a message for m < 0, nbr_ptr[0] != 0, a decreasing nbr_ptr, an id outside [0, N + m), more than 2^31 - 1 stored entries."""
    lib = _lib.gcnhost()
    gp = _i32(g_indptr).ravel()
    p64 = np.ascontiguousarray(nbr_ptr, np.int64).ravel()
    ids = np.ascontiguousarray(nbr_ids, np.int32).ravel()
    m = p64.size - 1 if m is None else int(m)
    if p64.size < max(m, 0) + 1:
        raise ValueError(f"new_node_rows: nbr_ptr has {p64.size} entries for {m} new nodes (m + 1 expected)")
    listed = int(p64[m]) if m >= 0 else 0
    total = max(listed, 0) + max(m, 0)
    if m >= 0 and ids.size < listed and total <= 2**31 - 1 and np.all(np.diff(p64[:m + 1]) >= 0):
        raise ValueError(f"new_node_rows: nbr_ptr ends at {listed}, nbr_ids has {ids.size} entries")
    room = total if total <= 2**31 - 1 else 1                # refused by the library before anything is written
    ptr, ln = np.zeros(max(m, 0) + 1, np.int32), np.zeros(max(m, 1), np.int32)
    col, coef = np.zeros(max(room, 1), np.int32), np.zeros(max(room, 1), np.float32)
    _ck(lib, lib.gcnhost_attach_rows(gp.size - 1, gp.ctypes.data, m, p64.ctypes.data, ids.ctypes.data, 1 if factored else 0, ptr.ctypes.data,
                                     col.ctypes.data, coef.ctypes.data, ln.ctypes.data), "new_node_rows")
    return dict(ptr=ptr, col=col[:total], coef=coef[:total], len=ln[:m])


def check_beta(what, beta):
    beta = float(beta)
    if not (np.isfinite(beta) and beta > 0):
        raise ValueError(f"{what}: beta must be finite and > 0, got {beta!r}")
    return beta


def read_thresholds(path, num_classes=None):
    """f32 [C] from a thresholds text file (write_thresholds, gcn-hip's GCN_THRESHOLDS=<file>; host/thresholds.h): one line per
    class, the first token the threshold, everything from '#' on ignored — host only, no GPU.  num_classes: the count the file
    must hold.  A wrong count, a bad token or a NaN raises GcnHostError naming the line."""
    lib = _lib.gcnhost()
    c = C.c_int(int(num_classes or 0))
    _ck(lib, lib.gcnhost_thresholds_read(os.fsencode(path), C.byref(c), None), "thresholds_read")
    thr = np.zeros(c.value, np.float32)
    _ck(lib, lib.gcnhost_thresholds_read(os.fsencode(path), C.byref(c), thr.ctypes.data), "thresholds_read")
    return thr


def write_thresholds(path, fit_or_array):
    """A thresholds file from the dict tune_thresholds() returns (each line then carries `# class c pos P neg N tp .. fp .. fn ..
    f ..`) or from a plain array of C thresholds — host only, no GPU.  Every float32 is written as %.9g and read back exactly.
    A NaN raises ValueError."""
    fit = fit_or_array if isinstance(fit_or_array, dict) else None
    thr = np.ascontiguousarray(fit["threshold"] if fit else fit_or_array, np.float32).ravel()
    thr = thresholds_array("write_thresholds", thr, max(thr.size, 1))
    notes = [None] * 6
    if fit:
        notes = [np.ascontiguousarray(fit[k], np.int64).ravel() for k in ("pos", "neg", "tp", "fp", "fn")] + [np.ascontiguousarray(fit["f"], np.float64).ravel()]
        if any(a.size != thr.size for a in notes):
            raise ValueError("write_thresholds: the fit's arrays must have one entry per threshold")
    lib = _lib.gcnhost()
    _ck(lib, lib.gcnhost_thresholds_write(os.fsencode(path), thr.size, thr.ctypes.data, *[a.ctypes.data if a is not None else None for a in notes]),
        "thresholds_write")


def ranking_report(u2, ap_sum, pos, neg):
    """Per-class ROC-AUC and average precision from the numbers ranking() forms on the GPU — host only, no GPU; the one place they
    are derived (host/ranking.h).  u2, pos, neg (integers) and ap_sum (float64) [C].  auc = u2 / (2 pos neg), defined when the
    class has a positive and a negative; ap = ap_sum / pos, defined when it has a positive; an undefined value is 0, never NaN.
    Returns a dict: auc, ap (float64 [C]), auc_defined, ap_defined (bool [C]), macro_auc, macro_ap (means over the defined
    classes only), weighted_auc, weighted_ap (weighted by pos over the defined classes), classes_defined.  A negative count, u2
    outside [0, 2 pos neg] or ap_sum outside [0, pos] raise GcnHostError."""
    u2, pos, neg = (np.ascontiguousarray(a, np.int64).ravel() for a in (u2, pos, neg))
    aps = np.ascontiguousarray(ap_sum, np.float64).ravel()
    c = u2.size
    if not (pos.size == c and neg.size == c and aps.size == c):
        raise GcnHostError(f"ranking_report: u2, ap_sum, pos and neg must have one entry per class, got {u2.size}, {aps.size}, {pos.size}, {neg.size}")
    lib = _lib.gcnhost()
    auc, ap = np.zeros(max(c, 1), np.float64), np.zeros(max(c, 1), np.float64)
    ad, pd = np.zeros(max(c, 1), np.int32), np.zeros(max(c, 1), np.int32)
    summ = np.zeros(5, np.float64)
    _ck(lib, lib.gcnhost_ranking_report(c, u2.ctypes.data, aps.ctypes.data, pos.ctypes.data, neg.ctypes.data, auc.ctypes.data, ap.ctypes.data,
                                        ad.ctypes.data, pd.ctypes.data, summ.ctypes.data), "ranking_report")
    return dict(auc=auc[:c], ap=ap[:c], auc_defined=ad[:c].astype(bool), ap_defined=pd[:c].astype(bool), macro_auc=float(summ[0]),
                macro_ap=float(summ[1]), weighted_auc=float(summ[2]), weighted_ap=float(summ[3]), classes_defined=int(summ[4]))


class _ConformalFit(C.Structure):
    """gcnhost_conformal of include/gcnhost.h"""
    _fields_ = [("method", C.c_int), ("lam", C.c_float), ("k_reg", C.c_int), ("diffusion", C.c_float), ("temperature", C.c_float),
                ("alpha", C.c_double), ("per_class", C.c_int), ("thresh", C.c_float * 64), ("n_cal", C.c_int64 * 64)]


def conformal_quantile(scores, alpha, labels=None, num_classes=None):
    """The threshold of split conformal prediction — host only, no GPU; the one place it is derived (host/conformal.h).  Negative
    scores are dropped (a row without a label); with n' left, k = ceil((n' + 1)(1 - alpha)) in float64 and the threshold is the
    k-th smallest score, +inf when k > n'.  Returns a dict: threshold (float), n_cal, k.  With labels (int [n]) and num_classes
    the scores are grouped by label and threshold (f32 [C]), n_cal and k (int64 [C]) hold one entry per class.  alpha outside
    (0, 1) or a NaN score raise GcnHostError."""
    s = np.ascontiguousarray(scores, np.float32).ravel()
    lib = _lib.gcnhost()
    if labels is None:
        c, lp = 1, None
    else:
        lab = _i32(labels).ravel()
        if lab.size != s.size or num_classes is None:
            raise GcnHostError(f"conformal_quantile: {lab.size} labels for {s.size} scores (and num_classes must be given)")
        c, lp = int(num_classes), (lab if lab.size else np.zeros(1, np.int32)).ctypes.data
    th, nc, k = np.zeros(max(c, 1), np.float32), np.zeros(max(c, 1), np.int64), np.zeros(max(c, 1), np.int64)
    sp = (s if s.size else np.zeros(1, np.float32)).ctypes.data
    _ck(lib, lib.gcnhost_conformal_quantile(sp, s.size, float(alpha), lp, c, th.ctypes.data, nc.ctypes.data, k.ctypes.data), "conformal_quantile")
    if labels is None:
        return dict(threshold=float(th[0]), n_cal=int(nc[0]), k=int(k[0]))
    return dict(threshold=th, n_cal=nc, k=k)


KEY_KMEANS = 0xE7037ED1A0B428DB           # host/module.h: the stream of cluster()'s seeding draws is its seed ^ this


def cluster_report(contingency):
    """The scores of a clustering against class labels from the integer table contingency [k, C] (rows: clusters) — host only,
    no GPU; the one place they are derived (host/kmeans.h has the formulas).  Returns a dict of float64: purity, homogeneity,
    completeness, v_measure (Rosenberg & Hirschberg), nmi (arithmetic-mean normalisation), ari (Hubert & Arabie),
    entropy_classes, entropy_clusters (natural logarithm), and rows.  Empty rows and columns are allowed; one cluster or one class
    gives the conventional values (both: a perfect match), never NaN.  A negative entry raises GcnHostError."""
    t = np.ascontiguousarray(contingency, np.int64)
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise GcnHostError(f"cluster_report: a [k, C] table with k, C >= 1, got shape {t.shape}")
    lib = _lib.gcnhost()
    s = np.zeros(9, np.float64)
    _ck(lib, lib.gcnhost_cluster_report(t.shape[0], t.shape[1], t.ctypes.data, s.ctypes.data), "cluster_report")
    names = ("purity", "homogeneity", "completeness", "v_measure", "nmi", "ari", "entropy_classes", "entropy_clusters")
    out = {name: float(v) for name, v in zip(names, s)}
    out["rows"] = int(s[8])
    return out


def read_silhouette(path):
    """The file gcn-hip writes with GCN_CLUSTER_SILHOUETTE, one line `node cluster s neighbor` per node: a dict of node int32 [n],
    cluster int32 [n], s float64 [n] (NaN for a node outside the points), neighbor int32 [n].  Needs no GPU."""
    node, cluster, s, nb = [], [], [], []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            try:
                if len(p) != 4:
                    raise ValueError
                node.append(int(p[0])), cluster.append(int(p[1])), s.append(float(p[2])), nb.append(int(p[3]))
            except ValueError:
                raise GcnHostError(f"read_silhouette: {path}:{no}: expected `node cluster s neighbor`, got {line.strip()!r}") from None
    return dict(node=np.array(node, np.int32), cluster=np.array(cluster, np.int32), s=np.array(s, np.float64), neighbor=np.array(nb, np.int32))


def sym_eigen(S):
    """(eigenvalues float64 [h] descending, vectors float64 [h, h] with COLUMN j the unit vector of eigenvalue j, its entry of
    largest magnitude positive) of a symmetric float64 matrix, 1 <= h <= 256 — host only, no GPU: cyclic Jacobi (host/pca.h).  A
    matrix that is not square, not finite or not symmetric bit for bit raises GcnHostError."""
    a = np.ascontiguousarray(S, np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise GcnHostError(f"sym_eigen: a square matrix, got shape {a.shape}")
    h = a.shape[0]
    lib = _lib.gcnhost()
    lam, v = np.zeros(max(h, 1), np.float64), np.zeros((max(h, 1), max(h, 1)), np.float64)
    _ck(lib, lib.gcnhost_sym_eigen((a if a.size else np.zeros(1)).ctypes.data, h, lam.ctypes.data, v.ctypes.data), "sym_eigen")
    return lam, v


def pca_from_scatter(scatter, mean, rows, k=None, whiten=False):
    """Everything a principal component analysis derives from the scatter matrix [h, h] of `rows` centred rows — host only, no
    GPU; the one place it is derived (host/pca.h has the formulas).  Returns a dict of float64: eigenvalues [h] (descending,
    clipped at 0), components [k, h] (k None: h), explained_variance, explained_variance_ratio (0 when the spectrum is 0),
    singular_values [h], rank, rows, and with whiten=True scale [k] (0 past the rank).  Never NaN or inf."""
    a = np.ascontiguousarray(scatter, np.float64)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise GcnHostError(f"pca_from_scatter: a square matrix, got shape {a.shape}")
    h = a.shape[0]
    k = h if k is None else int(k)
    m = None if mean is None else np.ascontiguousarray(mean, np.float64).ravel()
    if m is not None and m.size != h:
        raise GcnHostError(f"pca_from_scatter: the mean has {m.size} entries, the matrix {h} rows")
    lib = _lib.gcnhost()
    hh = max(h, 1)
    ev, comp, expl, scale = np.zeros(hh, np.float64), np.zeros((hh, hh), np.float64), np.zeros((3, hh), np.float64), np.zeros(max(k, 1), np.float64)
    rank = C.c_int()
    _ck(lib, lib.gcnhost_pca_from_scatter((a if a.size else np.zeros(1)).ctypes.data, m.ctypes.data if m is not None else None, int(rows), h, k,
                                          int(bool(whiten)), ev.ctypes.data, comp.ctypes.data, expl.ctypes.data, scale.ctypes.data, C.byref(rank)),
        "pca_from_scatter")
    return dict(eigenvalues=ev, components=comp[:k].copy(), explained_variance=expl[0].copy(), explained_variance_ratio=expl[1].copy(),
                singular_values=expl[2].copy(), rank=rank.value, rows=int(rows), scale=scale if whiten else None)


def _structure_tables(what, mix, class_rows, totals=None, strata=None, bins=None):
    m = np.ascontiguousarray(mix, np.int64)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or not 1 <= m.shape[0] <= 64:
        raise GcnHostError(f"{what}: mix must be a [C, C] table with 1 <= C <= 64, got shape {m.shape}")
    c = m.shape[0]
    r = np.ascontiguousarray(class_rows, np.int64)
    if r.shape != (c,):
        raise GcnHostError(f"{what}: class_rows must have shape ({c},), got {r.shape}")
    t = None
    if totals is not None:
        t = np.ascontiguousarray(totals, np.int64)
        if t.shape != (8,):
            raise GcnHostError(f"{what}: totals must have shape (8,), got {t.shape}")
    st = None
    if strata is not None:
        st = np.ascontiguousarray(strata, np.int64)
        b = st.shape[1] - 1 if st.ndim == 3 else -1
        bins = b if bins is None else bins
        if st.ndim != 3 or not 1 <= bins <= 32 or st.shape != (32, bins + 1, 2):
            raise GcnHostError(f"{what}: strata must have shape (32, bins + 1, 2) with 1 <= bins <= 32, got {st.shape} with bins = {bins!r}")
    return m, r, t, st, (int(bins) if st is not None else 0)


def structure_metrics(mix, class_rows, totals=None, strata=None, bins=None):
    """The label structure of a graph from integer counts — host only, no GPU; the one place the measures are derived
    (host/structure.h has the formulas).  mix int [C, C] (entries from a row labelled a to a neighbour labelled b), class_rows int
    [C], totals int [8] (None: node_homophily is 0), strata int [32, bins + 1, 2] (None: no tables).  Returns a dict of float64:
    edge_homophily, node_homophily, adjusted_homophily (Platonov et al., 2023), class_insensitive_homophily (Lim et al., 2021),
    class_homophily [C], compatibility [C, C] (the row-normalised mix; a zero row stays zero), and the integers edges,
    rows_with_known, labelled_rows; with strata also strata_rows and by_degree / by_agreement: lists of dict(lo, hi, rows, correct,
    accuracy) (the bucket without a labelled neighbour has lo = hi = -1).  A zero denominator gives 0, never NaN.  A negative
    count or a mismatched shape raises GcnHostError."""
    what = "structure_metrics"
    m, r, t, st, bins = _structure_tables(what, mix, class_rows, totals, strata, bins)
    c = m.shape[0]
    lib = _lib.gcnhost()
    s, ch, comp = np.zeros(8, np.float64), np.zeros(c, np.float64), np.zeros((c, c), np.float64)
    bd, ba = np.zeros((32, 5), np.float64), np.zeros((bins + 1, 5), np.float64)
    _ck(lib, lib.gcnhost_structure_metrics(c, m.ctypes.data, r.ctypes.data, t.ctypes.data if t is not None else None, bins,
                                           st.ctypes.data if st is not None else None, s.ctypes.data, ch.ctypes.data, comp.ctypes.data,
                                           bd.ctypes.data, ba.ctypes.data), what)
    out = dict(edge_homophily=float(s[0]), node_homophily=float(s[1]), adjusted_homophily=float(s[2]), class_insensitive_homophily=float(s[3]),
               class_homophily=ch, compatibility=comp, edges=int(s[4]), rows_with_known=int(s[5]), labelled_rows=int(s[6]))
    if st is not None:
        rows = lambda tab: [dict(lo=float(x[0]), hi=float(x[1]), rows=int(x[2]), correct=int(x[3]), accuracy=float(x[4])) for x in tab]
        out.update(strata_rows=int(s[7]), by_degree=rows(bd), by_agreement=rows(ba))
    return out


def write_structure_report(path, report):
    """structure_report()'s integers (a report made with predicted=True) as the text file gcn-hip writes for GCN_STRUCTURE"""
    what = "write_structure_report"
    if report.get("pred") is None or report.get("strata") is None:
        raise GcnHostError(f"{what}: a report made with predicted=True")
    t, p = report["truth"], report["pred"]
    m, r, tt, st, bins = _structure_tables(what, t["mix"], t["class_rows"], t["totals"], report["strata"], None)
    m2, r2, tp, _, _ = _structure_tables(what, p["mix"], p["class_rows"], p["totals"])
    if m2.shape != m.shape:
        raise GcnHostError(f"{what}: the two mixing tables have shapes {m.shape} and {m2.shape}")
    lib = _lib.gcnhost()
    _ck(lib, lib.gcnhost_structure_write(os.fspath(path).encode(), m.shape[0], bins, tt.ctypes.data, tp.ctypes.data, r.ctypes.data, r2.ctypes.data,
                                         m.ctypes.data, m2.ctypes.data, st.ctypes.data), what)


def read_structure_report(path):
    """the integers of a structure report file: dict(num_classes, bins, truth=dict(mix, class_rows, totals), pred=..., strata)"""
    lib = _lib.gcnhost()
    c, b = C.c_int(), C.c_int()
    tt, tp, rt, rp = np.zeros(8, np.int64), np.zeros(8, np.int64), np.zeros(64, np.int64), np.zeros(64, np.int64)
    mt, mp, st = np.zeros(64 * 64, np.int64), np.zeros(64 * 64, np.int64), np.zeros(32 * 33 * 2, np.int64)
    _ck(lib, lib.gcnhost_structure_read(os.fspath(path).encode(), C.byref(c), C.byref(b), tt.ctypes.data, tp.ctypes.data, rt.ctypes.data, rp.ctypes.data,
                                        mt.ctypes.data, mp.ctypes.data, st.ctypes.data), "read_structure_report")
    c, b = c.value, b.value
    return dict(num_classes=c, bins=b, truth=dict(mix=mt[:c * c].reshape(c, c).copy(), class_rows=rt[:c].copy(), totals=tt),
                pred=dict(mix=mp[:c * c].reshape(c, c).copy(), class_rows=rp[:c].copy(), totals=tp), strata=st[:32 * (b + 1) * 2].reshape(32, b + 1, 2).copy())


def _reach_strata(what, strata, hops):
    st = np.ascontiguousarray(strata, np.int64)
    if hops is None and st.ndim == 2:
        hops = st.shape[0] - 2
    if isinstance(hops, bool) or not isinstance(hops, (int, np.integer)) or not 1 <= hops <= 32 or st.shape != (hops + 2, 4):
        raise GcnHostError(f"{what}: strata must have shape (hops + 2, 4) with 1 <= hops <= 32, got {st.shape} with hops = {hops!r}")
    return st, int(hops)


def reach_metrics(strata, hops=None, layers=2):
    """Accuracy by distance from the labels out of integer counts — host only, no GPU; the one place the measures are derived
    (host/reach.h).  strata int [hops + 2, 4]: per bucket (b < hops: distance b; hops: further away; hops + 1: unreachable) the
    rows listed, those with a label, of those the ones predicted right, of those the ones whose nearest source carries their
    label.  layers: the depth of the model, 0 <= layers < hops: a row within `layers` hops is inside the receptive field.  Returns
    a dict: by_distance (a list of dict(rows, labelled, correct, nearest_correct, accuracy, nearest_label_accuracy)),
    inside_receptive_field, outside_receptive_field, all (the same keys), unreachable, unreachable_share, nearest_label_accuracy
    (over all rows), hops, layers.  A zero denominator gives 0, never NaN.  A negative or inconsistent count, or a mismatched
    shape, raises GcnHostError."""
    what = "reach_metrics"
    st, hops = _reach_strata(what, strata, hops)
    if isinstance(layers, bool) or not isinstance(layers, (int, np.integer)):
        raise GcnHostError(f"{what}: layers must be an integer in 0..hops - 1, got {layers!r}")
    lib = _lib.gcnhost()
    bd, gr, sm = np.zeros((hops + 2, 6), np.float64), np.zeros((3, 6), np.float64), np.zeros(2, np.float64)
    _ck(lib, lib.gcnhost_reach_metrics(st.ctypes.data, hops, int(layers), bd.ctypes.data, gr.ctypes.data, sm.ctypes.data), what)
    row = lambda x: dict(rows=int(x[0]), labelled=int(x[1]), correct=int(x[2]), nearest_correct=int(x[3]), accuracy=float(x[4]),
                         nearest_label_accuracy=float(x[5]))
    return dict(by_distance=[row(x) for x in bd], inside_receptive_field=row(gr[0]), outside_receptive_field=row(gr[1]), all=row(gr[2]),
                unreachable=int(sm[0]), unreachable_share=float(sm[1]), nearest_label_accuracy=float(gr[2][5]), hops=hops, layers=int(layers))


def write_reach_report(path, report):
    """reach_report()'s integers as the text file gcn-hip writes for GCN_REACH"""
    what = "write_reach_report"
    st, hops = _reach_strata(what, report["strata"], report.get("hops"))
    totals, lc = np.ascontiguousarray(report["totals"], np.int64), np.ascontiguousarray(report["level_counts"], np.int64)
    if totals.shape != (6,) or lc.ndim != 1 or lc.size < 1:
        raise GcnHostError(f"{what}: totals must have shape (6,) and level_counts at least one entry, got {totals.shape} and {lc.shape}")
    info = np.array([report.get("sources", 0), report.get("unlabelled", 0), report.get("rounds", 0)], np.int64)
    lib = _lib.gcnhost()
    _ck(lib, lib.gcnhost_reach_write(os.fspath(path).encode(), hops, int(report.get("layers", min(2, hops - 1))), info.ctypes.data, totals.ctypes.data,
                                     lc.ctypes.data, lc.size, st.ctypes.data), what)


def read_reach_report(path):
    """the integers of a reach report file: dict(hops, layers, strata, totals, level_counts, levels, sources, unlabelled, rounds)"""
    lib = _lib.gcnhost()
    h, la, nl = C.c_int(), C.c_int(), C.c_int64()
    info, totals, st = np.zeros(3, np.int64), np.zeros(6, np.int64), np.zeros(34 * 4, np.int64)
    fn = os.fspath(path).encode()
    _ck(lib, lib.gcnhost_reach_read(fn, C.byref(h), C.byref(la), info.ctypes.data, totals.ctypes.data, None, 0, C.byref(nl), st.ctypes.data),
        "read_reach_report")
    lc = np.zeros(nl.value, np.int64)
    _ck(lib, lib.gcnhost_reach_read(fn, C.byref(h), C.byref(la), info.ctypes.data, totals.ctypes.data, lc.ctypes.data, lc.size, C.byref(nl), st.ctypes.data),
        "read_reach_report")
    hops = h.value
    return dict(hops=hops, layers=la.value, strata=st[:(hops + 2) * 4].reshape(hops + 2, 4).copy(), totals=totals, level_counts=lc, levels=int(lc.size) - 1,
                sources=int(info[0]), unlabelled=int(info[1]), rounds=int(info[2]))


def calibration_report(count, correct, conf_sum):
    """The reliability diagram from per-bin counts — host only, no GPU; the one place it is derived (host/calibration.h).  count,
    correct (integers) and conf_sum (float64) [bins]: rows, rows predicted right and the sum of confidences in bin (b / bins,
    (b + 1) / bins].  Returns a dict: count (int64), accuracy = correct / count and confidence = conf_sum / count (float64, 0 for
    an empty bin), ece = sum_b (count_b / rows) |accuracy_b - confidence_b|, mce = the largest gap of a non-empty bin, rows.  Arrays
    of different lengths, correct above count or a negative entry raise GcnHostError."""
    c, k, s = (np.ascontiguousarray(count, np.int64).ravel(), np.ascontiguousarray(correct, np.int64).ravel(),
               np.ascontiguousarray(conf_sum, np.float64).ravel())
    if not (c.size == k.size == s.size) or c.size < 1:
        raise GcnHostError(f"calibration_report: count, correct and conf_sum must have one length >= 1, got {[c.size, k.size, s.size]}")
    lib = _lib.gcnhost()
    acc, conf, summ = np.zeros(c.size, np.float64), np.zeros(c.size, np.float64), np.zeros(3, np.float64)
    _ck(lib, lib.gcnhost_calibration_report(c.size, c.ctypes.data, k.ctypes.data, s.ctypes.data, acc.ctypes.data, conf.ctypes.data,
                                            summ.ctypes.data), "calibration_report")
    return dict(count=c.copy(), accuracy=acc, confidence=conf, ece=float(summ[0]), mce=float(summ[1]), rows=int(summ[2]))


def balanced_class_weights(labels_or_y, split, num_classes, which_split=1):
    """f32 [C] "balanced" class weights from the rows of one split (1 = train) — host only, no GPU (host/class_weights.h).
    labels_or_y 1-D int labels: w_c = n / (C n_c) over the split's rows whose label is in [0, C) (0 for a class without rows;
    scikit-learn's class_weight="balanced").  2-D bool [N, C]: pw_c = (n - pos_c) / pos_c over the split's rows (1 for a class
    without positives; PyTorch's pos_weight rule)."""
    lib = _lib.gcnhost()
    y = np.asarray(labels_or_y)
    sp = _i32(split)
    w = np.zeros(int(num_classes), np.float32)
    if y.ndim == 2:
        from .ops import pack_multihot
        if y.shape != (sp.size, int(num_classes)):
            raise ValueError(f"balanced_class_weights: expected a [{sp.size}, {num_classes}] matrix, got {y.shape}")
        words = pack_multihot(y != 0)
        rc = lib.gcnhost_balanced_class_weights(sp.size, int(num_classes), sp.ctypes.data, None, words.ctypes.data, int(which_split), w.ctypes.data)
    else:
        lab = _i32(y)
        if lab.shape != sp.shape:
            raise ValueError(f"balanced_class_weights: {lab.size} labels for {sp.size} nodes")
        rc = lib.gcnhost_balanced_class_weights(sp.size, int(num_classes), sp.ctypes.data, lab.ctypes.data, None, int(which_split), w.ctypes.data)
    _ck(lib, rc, "balanced_class_weights")
    return w


def read_class_weights(path, num_classes=None):
    """f32 [C] from a class weights text file (one float per line, one line per class; gcn-hip's GCN_CLASS_WEIGHTS=<file>) — host
    only.  num_classes: the line count the file must have.  A wrong count, a bad token, a negative, nan or inf raises
    GcnHostError naming the line."""
    lib = _lib.gcnhost()
    c = C.c_int(int(num_classes or 0))
    _ck(lib, lib.gcnhost_class_weights_read(os.fsencode(path), C.byref(c), None), "class_weights_read")
    w = np.zeros(c.value, np.float32)
    _ck(lib, lib.gcnhost_class_weights_read(os.fsencode(path), C.byref(c), w.ctypes.data), "class_weights_read")
    return w


def read_weights(path):
    """(W1 [F, h], W2 [h, C]) of a weights file (HipGCNModel.save_weights, gcn-hip GCN_SAVE_WEIGHTS) — host only, no GPU"""
    lib = _lib.gcnhost()
    F, h, c = C.c_int(), C.c_int(), C.c_int()
    _ck(lib, lib.gcnhost_weights_read(os.fsencode(path), C.byref(F), C.byref(h), C.byref(c), None, None), "weights_read")
    w1 = np.zeros((F.value, h.value), np.float32)
    w2 = np.zeros((h.value, c.value), np.float32)
    _ck(lib, lib.gcnhost_weights_read(os.fsencode(path), C.byref(F), C.byref(h), C.byref(c), w1.ctypes.data, w2.ctypes.data), "weights_read")
    return w1, w2


def read_labels(path, num_nodes=None, num_classes=None):
    """bool [N, C] from a multi-label truth file (one line per node, comma-separated class ids, empty for none; host/labels.h) —
    host only, no GPU.  num_nodes: the line count the file must have; num_classes: fixes C (else the largest id + 1).  A wrong
    line count, a bad token or a negative id raises GcnHostError with the file's line."""
    from .ops import unpack_multihot
    lib = _lib.gcnhost()
    n, c = C.c_int(int(num_nodes or 0)), C.c_int(int(num_classes or 0))
    _ck(lib, lib.gcnhost_labels_read(os.fsencode(path), C.byref(n), C.byref(c), None), "labels_read")
    words = np.zeros((n.value, (c.value + 31) // 32), np.uint32)
    _ck(lib, lib.gcnhost_labels_read(os.fsencode(path), C.byref(n), C.byref(c), words.ctypes.data), "labels_read")
    return unpack_multihot(words, c.value)


def write_labels(path, y):
    """the inverse of read_labels: one line per row of the bool [N, C] matrix y, its class ids ascending"""
    y = np.asarray(y).astype(bool)
    with open(path, "w") as f:
        for row in y:
            f.write(",".join(str(int(c)) for c in np.flatnonzero(row)) + "\n")


def write_weights(path, w1, w2):
    """a weights file from two arrays W1 [F, h], W2 [h, C] — host only, no GPU"""
    w1, w2 = np.ascontiguousarray(w1, np.float32), np.ascontiguousarray(w2, np.float32)
    if w1.ndim != 2 or w2.ndim != 2 or w1.shape[1] != w2.shape[0]:
        raise ValueError(f"write_weights: shapes {w1.shape} and {w2.shape} do not chain")
    lib = _lib.gcnhost()
    _ck(lib, lib.gcnhost_weights_write(os.fsencode(path), w1.shape[0], w1.shape[1], w2.shape[1], w1.ctypes.data, w2.ctypes.data), "weights_write")


def load_dataset(root, name):
    """the reference's text formats (or a .gcnbin cache) through the C++ Parser"""
    lib = _lib.gcnhost()
    p = lib.gcnhost_params_default()
    h = C.c_void_p()
    if root and not root.endswith("/"):
        root += "/"
    import time
    t0 = time.perf_counter()
    _ck(lib, lib.gcnhost_dataset_load(C.byref(h), root.encode() if root else None, name.encode(), C.byref(p)), "dataset_load")
    load_s = time.perf_counter() - t0      # the C++ Parser alone (the numpy copies below are the Python front end's)
    ptrs = [C.c_void_p() for _ in range(7)]
    ns = [C.c_int64() for _ in range(4)]
    lib.gcnhost_dataset_arrays(h, C.byref(ptrs[0]), C.byref(ptrs[1]), C.byref(ns[0]), C.byref(ptrs[2]), C.byref(ptrs[3]),
                               C.byref(ptrs[4]), C.byref(ns[1]), C.byref(ptrs[5]), C.byref(ns[2]), C.byref(ptrs[6]), C.byref(ns[3]))

    def arr(ptr, n, t):
        if n == 0:
            return np.zeros(0, t)
        ct = C.c_float if t == np.float32 else C.c_int
        return np.frombuffer((ct * n).from_address(ptr.value), dtype=t).copy()
    N = p.num_nodes
    ds = dict(name=name, num_nodes=N, input_dim=p.input_dim, output_dim=p.output_dim,
              g_indptr=arr(ptrs[0], N + 1, np.int32), g_indices=arr(ptrs[1], ns[0].value, np.int32),
              f_indptr=arr(ptrs[2], ns[3].value + 1, np.int32), f_indices=arr(ptrs[3], ns[1].value, np.int32),
              f_val=arr(ptrs[4], ns[1].value, np.float32), split=arr(ptrs[5], ns[2].value, np.int32),
              label=arr(ptrs[6], ns[3].value, np.int32))
    ds["_handle"] = (lib, h, p)
    ds["_load_s"] = load_s
    return ds


def save_binary(ds, path):
    lib, h, p = ds["_handle"]
    if lib.gcnhost_dataset_save_binary(h, C.byref(p), path.encode()) != 0:
        raise GcnHostError("save_binary failed")


def partition(g_indptr, world):
    lib = _lib.gcnhost()
    gp = _i32(g_indptr)
    start = np.zeros(world + 1, np.int32)
    rm = C.c_int()
    rc = lib.gcnhost_partition(gp.ctypes.data, gp.size - 1, world, start.ctypes.data, C.byref(rm))
    if rc != 0:
        raise GcnHostError("partition failed")
    return start, rm.value


def local_graph(g_indptr, g_indices, world, rank):
    """(indptr, padded indices, col_deg, n_cols) of `rank`'s row block — host-only"""
    lib = _lib.gcnhost()
    gp, gi = _i32(g_indptr), _i32(g_indices)
    nl, nc, nnz = C.c_int(), C.c_int(), C.c_int64()
    rc = lib.gcnhost_local_graph(gp.ctypes.data, gi.ctypes.data, gp.size - 1, world, rank, None, None, None,
                                 C.byref(nl), C.byref(nc), C.byref(nnz))
    if rc != 0:
        raise GcnHostError("local_graph failed")
    ip, ix, cd = np.zeros(nl.value + 1, np.int32), np.zeros(nnz.value, np.int32), np.zeros(nc.value, np.int32)
    lib.gcnhost_local_graph(gp.ctypes.data, gi.ctypes.data, gp.size - 1, world, rank, ip.ctypes.data, ix.ctypes.data,
                            cd.ctypes.data, None, None, None)
    return ip, ix, cd, nc.value


def exchange_plan(g_indptr, g_indices, world, rank, mode=0):
    """the host-side plan of `rank` (host/partition.h) as a dict of numpy arrays — host only"""
    lib = _lib.gcnhost()
    gp, gi = _i32(g_indptr), _i32(g_indices)
    h = C.c_void_p()
    if lib.gcnhost_plan_create(C.byref(h), gp.ctypes.data, gi.ctypes.data, gp.size - 1, world, rank, mode) != 0:
        raise GcnHostError("plan_create failed")
    halo, nl, tr, oo, rm = (C.c_int() for _ in range(5))
    sh = C.c_double()
    nnz, nr, ns = C.c_int64(), C.c_int64(), C.c_int64()
    lib.gcnhost_plan_info(h, C.byref(halo), C.byref(nl), C.byref(tr), C.byref(oo), C.byref(rm), C.byref(sh), C.byref(nnz), C.byref(nr), C.byref(ns))
    ptr = [C.c_void_p() for _ in range(8)]
    lib.gcnhost_plan_arrays(h, *[C.byref(q) for q in ptr])

    def arr(q, n):
        return np.frombuffer((C.c_int * n).from_address(q.value), dtype=np.int32).copy() if n and q.value else np.zeros(0, np.int32)
    is_halo = bool(halo.value)
    out = dict(halo=is_halo, n_local=nl.value, table_rows=tr.value, own_offset=oo.value, rows_max=rm.value, halo_share=sh.value,
               recv_off=arr(ptr[0], world + 1 if is_halo else 0), recv_rows=arr(ptr[1], nr.value),
               send_off=arr(ptr[2], world + 1 if is_halo else 0), send_rows=arr(ptr[3], ns.value),
               table_global=arr(ptr[4], tr.value), indptr=arr(ptr[5], nl.value + 1), indices=arr(ptr[6], nnz.value),
               col_deg=arr(ptr[7], max(tr.value, 1)))
    lib.gcnhost_plan_free(h)
    return out


def choose_node_order(g_indptr, g_indices, world, force=False):
    """what a `world`-rank model does with the node ids of this graph (host only): dict(order, renumbered, ids_share, ids_recv_rows,
    new_share, new_recv_rows, allgather_rows)"""
    lib = _lib.gcnhost()
    gp, gi = _i32(g_indptr), _i32(g_indices)
    n = gp.size - 1
    order = np.zeros(n, np.int32)
    ren = C.c_int()
    s0, s1 = C.c_double(), C.c_double()
    r0, r1, ag = C.c_int64(), C.c_int64(), C.c_int64()
    rc = lib.gcnhost_choose_node_order(gp.ctypes.data, gi.ctypes.data, n, world, int(force), order.ctypes.data, C.byref(ren),
                                       C.byref(s0), C.byref(r0), C.byref(s1), C.byref(r1), C.byref(ag))
    if rc != 0:
        raise GcnHostError("choose_node_order failed")
    return dict(order=order, renumbered=bool(ren.value), ids_share=s0.value, ids_recv_rows=r0.value, new_share=s1.value,
                new_recv_rows=r1.value, allgather_rows=ag.value)


def glorot(size, in_size, out_size, seed, skip_draws=0):
    lib = _lib.gcnhost()
    w = np.zeros(size, np.float32)
    lib.gcnhost_glorot(w.ctypes.data, size, in_size, out_size, int(seed), int(skip_draws))
    return w


def host_masks(n, p, seed, skip_draws=0):
    lib = _lib.gcnhost()
    k = np.zeros(n, np.uint8)
    lib.gcnhost_host_masks(k.ctypes.data, n, p, int(seed), int(skip_draws))
    return k
