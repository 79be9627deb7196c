"""References for the class-weighted loss tests (tests/test_class_weights_gpu.py, tests/mr_class_weights_worker.py): numpy
float64 restatements of the two kernels, a torch-CPU float64 two-layer GCN with the model's Glorot weights, replayed host
dropout masks and the reference's Adam (the idea of tests/test_multilabel_gpu.py::torch_trace, with torch's own
cross_entropy(weight=) / binary_cross_entropy_with_logits(pos_weight=) as the loss), and the imbalanced planted dataset.
Nothing here touches the GPU."""
import numpy as np

from cuda_gcn_amd import datagen


def wxent_reference(z, truth, w, rows, weight_sum=None, scale=None):
    """(sum of w . term, sum of w, dZ [n, C] (zero outside rows), correct, total, sum of |w . term|) in float64"""
    z = np.asarray(z, np.float64)
    w = np.asarray(w, np.float64)
    zr, t = z[rows], np.asarray(truth)[rows]
    n, C = zr.shape
    mx = zr.max(1, keepdims=True)
    with np.errstate(over="ignore", under="ignore"):
        ex = np.exp(zr - mx)
    se = ex.sum(1)
    zt = zr[np.arange(n), t]
    terms = np.log(se) - (zt - mx[:, 0])
    wt = w[t]
    ws = wt.sum() if weight_sum is None else weight_sum
    p = ex / se[:, None]
    p[np.arange(n), t] -= 1.0
    gr = wt[:, None] * p / ws
    if scale is not None:
        gr = gr * np.asarray(scale, np.float64)[rows][:, None]
    g = np.zeros_like(z)
    g[rows] = gr
    correct = int(np.sum(~(mx[:, 0] > zt)))
    return float((wt * terms).sum()), float(wt.sum()), g, correct, n, float(np.abs(wt * terms).sum())


def wbce_reference(z, y, pw, rows, count=None, scale=None):
    """(loss, dZ, TP, FP, FN, F1, mean |term|) in float64: pw . y . softplus(-z) + (1 - y) . softplus(z)"""
    z = np.asarray(z, np.float64)
    pw = np.asarray(pw, np.float64)[None, :]
    zr, yr = z[rows], np.asarray(y, bool)[rows]
    n, C = zr.shape
    count = count or n
    with np.errstate(over="ignore"):
        l1p = np.log1p(np.exp(-np.abs(zr)))
        e = np.exp(-np.abs(zr))
    sp_pos, sp_neg = np.maximum(zr, 0) + l1p, np.maximum(-zr, 0) + l1p          # softplus(z), softplus(-z)
    terms = np.where(yr, pw * sp_neg, sp_pos)
    sig = np.where(zr >= 0, 1 / (1 + e), e / (1 + e))                             # sigmoid(z); sigmoid(-z) = 1 - it, formed without cancellation:
    sig_neg = np.where(zr >= 0, e / (1 + e), 1 / (1 + e))
    gr = np.where(yr, -pw * sig_neg, sig) / (count * C)
    if scale is not None:
        gr = gr * np.asarray(scale, np.float64)[rows][:, None]
    g = np.zeros_like(z)
    g[rows] = gr
    pos = zr > 0
    tp, fp, fn = int(np.sum(pos & yr)), int(np.sum(pos & ~yr)), int(np.sum(~pos & yr))
    f1 = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0
    return terms.sum() / (n * C), g, tp, fp, fn, f1, np.abs(terms).sum() / (n * C)


def balanced_reference(labels_or_y, split, C, s=1):
    """the two `balanced` rules restated directly"""
    y = np.asarray(labels_or_y)
    rows = np.asarray(split) == s
    if y.ndim == 2:
        n, pos = rows.sum(), y[rows].astype(bool).sum(0).astype(np.float64)
        return np.where(pos > 0, (n - pos) / np.where(pos > 0, pos, 1), 1.0)
    lab = y[rows]
    lab = lab[(lab >= 0) & (lab < C)]
    cnt = np.bincount(lab, minlength=C).astype(np.float64)
    return np.where(cnt > 0, lab.size / (C * np.where(cnt > 0, cnt, 1)), 0.0)


def macro_recall(pred, truth, C):
    """mean over the C classes of (rows of the class predicted as it) / (rows of the class); every class must have a row"""
    rec = []
    for c in range(C):
        rows = truth == c
        assert rows.any(), f"class {c} has no row"
        rec.append(float(np.mean(pred[rows] == c)))
    return float(np.mean(rec))


def torch_trace(ds, seed, hidden, epochs, weight=None, multilabel=None, dropout=0.5, lr=0.01, wd=5e-4, want_val_pred=False):
    """[(train_loss, train_acc or micro-F1, val_loss, val_acc or micro-F1)] per epoch of the reference's two-layer GCN in torch
    (float64 activations) with the model's glorot weights, host dropout masks and Adam (W1 decayed).  weight: None, or the class
    weights [C] (single-label: cross_entropy(weight=); with multilabel=Y: pos_weight=).  want_val_pred: also the argmax
    predictions of the validation rows after the last epoch (single-label)."""
    import torch
    from cuda_gcn_amd import model as M
    N, F = ds["num_nodes"], ds["input_dim"]
    C = multilabel.shape[1] if multilabel is not None else ds["output_dim"]
    gp, gi = ds["g_indptr"].astype(np.int64), ds["g_indices"].astype(np.int64)
    deg = np.diff(gp).astype(np.float64)
    r = np.repeat(np.arange(N), np.diff(gp))
    A = torch.sparse_coo_tensor(np.vstack([r, gi]), 1 / np.sqrt(deg[r] * deg[gi]), (N, N)).coalesce()
    fp_, fi = ds["f_indptr"].astype(np.int64), ds["f_indices"].astype(np.int64)
    fr = np.repeat(np.arange(N), np.diff(fp_))
    fv = torch.tensor(ds["f_val"], dtype=torch.float64)
    nnz = fv.numel()
    w = [M.glorot(F * hidden, F, hidden, seed).reshape(F, hidden), M.glorot(hidden * C, hidden, C, seed, F * hidden).reshape(hidden, C)]
    mom = [np.zeros_like(x) for x in w]
    vel = [np.zeros_like(x) for x in w]
    Y = torch.tensor(np.asarray(multilabel), dtype=torch.float64) if multilabel is not None else None
    T = torch.tensor(np.asarray(ds["label"]), dtype=torch.int64) if multilabel is None else None
    W = torch.tensor(np.asarray(weight), dtype=torch.float64) if weight is not None else None
    split = ds["split"]
    draws = F * hidden + hidden * C

    def forward(W1, W2, k0=None, k1=None):
        v = fv if k0 is None else fv * torch.tensor(k0, dtype=torch.float64) / (1 - dropout)
        X = torch.sparse_coo_tensor(np.vstack([fr, fi]), v, (N, F))
        H = torch.relu(torch.sparse.mm(A, torch.sparse.mm(X, W1)))
        if k1 is not None:
            H = H * torch.tensor(k1.reshape(N, hidden), dtype=torch.float64) / (1 - dropout)
        return torch.sparse.mm(A, H @ W2)

    def metrics(Z, s):
        rows = np.flatnonzero(split == s)
        zr = Z[rows]
        if Y is not None:
            yr = Y[rows]
            loss = torch.nn.functional.binary_cross_entropy_with_logits(zr, yr, pos_weight=W, reduction="mean")
            pos, yy = (zr > 0).numpy(), yr.numpy() > 0
            tp, fpp, fn = np.sum(pos & yy), np.sum(pos & ~yy), np.sum(~pos & yy)
            return loss, (2 * tp / (2 * tp + fpp + fn) if 2 * tp + fpp + fn else 0.0)
        tr = T[rows]
        loss = torch.nn.functional.cross_entropy(zr, tr, weight=W, reduction="mean")
        zd = zr.detach()
        zt = zd[torch.arange(len(rows)), tr]
        return loss, float((~(zd.max(1).values > zt)).double().mean())

    out = []
    for e in range(epochs):
        if dropout > 0:
            k0 = M.host_masks(nnz, dropout, seed, draws)
            k1 = M.host_masks(N * hidden, dropout, seed, draws + nnz)
            draws += nnz + N * hidden
        else:
            k0 = k1 = None
        W1 = torch.tensor(w[0], dtype=torch.float64, requires_grad=True)
        W2 = torch.tensor(w[1], dtype=torch.float64, requires_grad=True)
        loss, acc = metrics(forward(W1, W2, k0, k1), 1)
        loss.backward()
        tl = float(loss.detach()) + wd * float(np.sum(w[0].astype(np.float64) ** 2)) / 2
        grads = [W1.grad.numpy().astype(np.float32), W2.grad.numpy().astype(np.float32)]
        step = np.float32(lr * np.sqrt(1 - 0.999 ** (e + 1)) / (1 - 0.9 ** (e + 1)))
        for i in range(2):
            g = grads[i] + (np.float32(wd) * w[i] if i == 0 else 0)
            mom[i] = (0.9 * mom[i].astype(np.float64) + 0.1 * g).astype(np.float32)
            vel[i] = (0.999 * vel[i].astype(np.float64) + 0.001 * g.astype(np.float64) ** 2).astype(np.float32)
            w[i] = (w[i] - step * mom[i] / (np.sqrt(vel[i]) + np.float32(1e-8))).astype(np.float32)
        with torch.no_grad():
            Zv = forward(torch.tensor(w[0], dtype=torch.float64), torch.tensor(w[1], dtype=torch.float64))
            vl, va = metrics(Zv, 2)
        out.append((tl, acc, float(vl) + wd * float(np.sum(w[0].astype(np.float64) ** 2)) / 2, va))
    out = np.array(out)
    if want_val_pred:
        rows = np.flatnonzero(split == 2)
        return out, Zv[rows].numpy().argmax(1), np.asarray(ds["label"])[rows]
    return out


# the imbalanced planted graph of the "it does what it is for" test: 8 classes over 16 communities whose edges mostly stay
# inside (p_in 0.8), and the training split of classes 3 .. 7 thinned to a twentieth (the thinned nodes leave every split)
IMBALANCED = dict(n_comm=16, size=128, deg=8, p_in=0.8, feats=16, classes=8, rare=(3, 4, 5, 6, 7), keep=0.05, seed=3,
                  hidden=16, epochs=40, model_seed=5)


def imbalanced_planted(n_comm, size, deg, p_in, feats, classes, rare, keep, seed, **_):
    ds = datagen.planted_communities(n_comm=n_comm, size=size, deg=deg, p_in=p_in, feats=feats, classes=classes,
                                     seed=datagen.DEFAULT_SEED + seed)
    rng = np.random.default_rng(seed)
    split, label = ds["split"].copy(), ds["label"]
    for c in rare:
        rows = np.flatnonzero((split == 1) & (label == c))
        drop = rng.permutation(rows)[max(1, int(round(keep * rows.size))):]
        split[drop] = 0
    ds["split"] = split
    for c in range(classes):                                   # the condition of the test: no empty class in either split
        assert np.any((split == 1) & (label == c)) and np.any((split == 2) & (label == c))
    ds["name"] = "planted-imbalanced"
    return ds
