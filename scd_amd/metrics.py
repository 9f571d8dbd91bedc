"""Clustering scores on the device: ACC, NMI, ARI and purity of a clustering against targets, from the contingency table
(scd_contingency) and its statistics (scd_contingency_stats).

What they restate (paths relative to the reference):
  * `cluster_acc`  gcd/project_utils/cluster_utils.py:39-62: D = max(pred.max(), true.max()) + 1, w[pred, true] counts,
    `linear_assignment(w.max() - w)` (ops.munkres, the same Munkres and tie-breaking), matched cells / N;
  * `purity_score` cluster_utils.py:65-69: sum over clusters of the largest cell / N;
  * `nmi_score`, `ari_score`: scikit-learn 1.7.2's `normalized_mutual_info_score` (arithmetic normaliser; 1.0 when both labellings
    have one class, or none; 0.0 when the mutual information is 0) and `adjusted_rand_score` (pair-confusion integers, as Python
    ints; 1.0 when fn == fp == 0), which the reference calls at gcd/methods/estimate_k/estimate_k.py:87-94.
The label arrays stay on the device; a call reads back S x 6 integers and S x 3 doubles, and `cluster_acc` the one table it solves.
NMI / ARI / purity are pure functions of those statistics (`nmi_from_stats`, `ari_from_stats`, `purity_from_stats`).

Tables are indexed [pred, truth]: a_i (row sums) belong to the predictions, b_j (column sums) to the targets.

`silhouette_samples` / `silhouette_score` need no targets: scikit-learn's functions of those names (metric='euclidean') through
scd_silhouette, one n x n x d MFMA pass; features and labels stay on the device.
"""
import numpy as np
import torch

from . import ops


def _labels(x, device=None):
    """Labels as a device int32 vector; numpy / list input (any integer or float dtype, truncated as `.astype(int)` does) is uploaded."""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(np.int64).reshape(-1)))
    x = x.reshape(-1)
    if not x.is_cuda:
        x = x.to(device if device is not None else "cuda")
    return x.to(torch.int32).contiguous()


def _mask(m, device):
    if not torch.is_tensor(m):
        m = torch.from_numpy(np.ascontiguousarray(np.asarray(m).astype(bool).reshape(-1)))
    return (m.reshape(-1).to(device) != 0).to(torch.uint8).contiguous()


def _sizes(pred, truth):
    """(pred.max() + 1, truth.max() + 1) in one read."""
    if pred.numel() == 0:
        raise ValueError("no rows to score")
    mx = torch.stack([pred.max(), truth.max()]).cpu().numpy()
    return int(mx[0]) + 1, int(mx[1]) + 1


def contingency(pred, truth, subset=None, kp=None, kt=None):
    """Device int32 table [kp, kt] of (pred, truth) pairs - or, with `subset` (a mask), tables [2, kp, kt]: the rows inside the subset,
    then the others.  kp / kt default to pred.max() + 1 / truth.max() + 1.  A label outside its range raises ValueError."""
    pred = _labels(pred)
    truth = _labels(truth, pred.device)
    if kp is None or kt is None:
        dp, dt = _sizes(pred, truth)
        kp, kt = (dp if kp is None else kp), (dt if kt is None else kt)
    sub = None if subset is None else _mask(subset, pred.device)
    table, n_bad = ops.contingency(pred, truth, sub, kp, kt)
    bad = int(n_bad.item())
    if bad:
        raise ValueError("%d rows have a label outside the %d x %d table (negative, or >= kp / kt)" % (bad, kp, kt))
    return table[0] if subset is None else table


def stats(table):
    """Host copies (ints int64 [S, 6], info float64 [S, 3]) of scd_contingency_stats for a device table [kp, kt] or [S, kp, kt]."""
    ints, info = ops.contingency_stats(table if table.dim() == 3 else table.unsqueeze(0))
    return ints.cpu().numpy(), info.cpu().numpy()


# ------------------------------------------------------------------ scores as pure functions of one table's statistics
def nmi_from_stats(ints, info):
    """sklearn 1.7.2 `normalized_mutual_info_score(average_method='arithmetic')` from (n, sum n_ij^2, sum a_i^2, sum b_j^2, purity
    numerator, non-zero cells) and (H(pred), H(truth), MI)."""
    n, nnz = int(ints[0]), int(ints[5])
    if n == 0 or nnz == 1:                  # no class on either side / one class on both: one non-zero cell
        return 1.0
    mi = max(float(info[2]), 0.0)           # mutual_info_score clips at 0
    if mi == 0.0:
        return 0.0
    normalizer = (float(info[1]) + float(info[0])) / 2.0
    return float(mi / normalizer)


def ari_from_stats(ints):
    """sklearn 1.7.2 `adjusted_rand_score`: the pair-confusion matrix as Python ints (no overflow at any n)."""
    n, ss, sa, sb = int(ints[0]), int(ints[1]), int(ints[2]), int(ints[3])
    tp = ss - n
    fp = sb - ss
    fn = sa - ss
    tn = n * n - fp - fn - ss               # pair_confusion_matrix: C[0, 0] = n^2 - C[0, 1] - C[1, 0] - sum n_ij^2 (ordered pairs, no self-pairs)
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


def purity_from_stats(ints):
    """cluster_utils.py:65-69: np.sum(np.amax(contingency, axis=0)) / np.sum(contingency), the maxima taken per cluster."""
    return float(np.int64(ints[4]) / np.int64(ints[0]))


def _acc_from_table(w):
    """cluster_utils.py:57-62 on the host copy of one square table."""
    w = np.asarray(w).astype(int)
    n = int(w.sum())
    ind = ops.munkres(w.max() - w)
    return sum([w[i, j] for i, j in ind]) * 1.0 / n


# ------------------------------------------------------------------ the reference's call surface
def cluster_acc(y_true, y_pred):
    """cluster_utils.py:39-62 with the counting on the device; only the D x D table comes to the host."""
    pred = _labels(y_pred)
    truth = _labels(y_true, pred.device)
    d = max(_sizes(pred, truth))
    return _acc_from_table(contingency(pred, truth, kp=d, kt=d).cpu().numpy())


def _one_table_stats(y_true, y_pred):
    ints, info = stats(contingency(y_pred, y_true))
    return ints[0], info[0]


def nmi_score(y_true, y_pred):
    return nmi_from_stats(*_one_table_stats(y_true, y_pred))


def ari_score(y_true, y_pred):
    return ari_from_stats(_one_table_stats(y_true, y_pred)[0])


def purity_score(y_true, y_pred):
    return purity_from_stats(_one_table_stats(y_true, y_pred)[0])


def score_split(pred, truth, labelled_mask):
    """What one evaluation of the estimator needs (estimate_k.py:87-94): one scd_contingency call with subset = labelled_mask, one
    statistics call -> {'labelled': {acc, nmi, ari, purity}, 'unlabelled': {...}}.  Both tables are D x D with D over all rows; the
    zero rows and columns this adds to a subset's own table change none of its four scores.  A subset without rows scores None."""
    pred = _labels(pred)
    truth = _labels(truth, pred.device)
    d = max(_sizes(pred, truth))
    tables = contingency(pred, truth, subset=labelled_mask, kp=d, kt=d)
    ints, info = stats(tables)
    w = tables.cpu().numpy()
    out = {}
    for s, name in enumerate(("labelled", "unlabelled")):
        if int(ints[s][0]) == 0:
            out[name] = None
            continue
        out[name] = dict(acc=_acc_from_table(w[s]), nmi=nmi_from_stats(ints[s], info[s]), ari=ari_from_stats(ints[s]),
                         purity=purity_from_stats(ints[s]))
    return out


# ------------------------------------------------------------------ silhouette (no targets)
def _silhouette(X, labels, k=None):
    if not torch.is_tensor(X):
        X = torch.from_numpy(np.ascontiguousarray(np.asarray(X)))
        if X.dtype not in (torch.float16, torch.float32):
            X = X.float()
    if X.dim() != 2:
        raise ValueError("X must be [n_samples, n_features]")
    if not X.is_cuda:
        X = X.to(labels.device if torch.is_tensor(labels) and labels.is_cuda else "cuda")
    if X.dtype not in (torch.float16, torch.float32):
        X = X.float()
    labels = _labels(labels, X.device)
    n = X.shape[0]
    if labels.numel() != n:
        raise ValueError("X has %d rows, labels %d" % (n, labels.numel()))
    if n < 2:
        raise ValueError("the silhouette needs at least 2 rows")
    k = int(labels.max().item()) + 1 if k is None else int(k)
    if k > n:                       # an id this large cannot come from a clustering of n rows with ids [0, k): more ids than rows
        raise ValueError("labels reach %d on %d rows: label ids must lie in [0, n_samples)" % (k - 1, n))
    samples, mean, info = ops.silhouette(X, labels, max(k, 2))
    bad, n_labels = (int(v) for v in info.cpu().numpy())
    if bad:
        raise ValueError("%d rows have a label outside [0, %d)" % (bad, max(k, 2)))
    if not 1 < n_labels < n:
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % n_labels)
    return samples, mean


def silhouette_samples(X, labels, k=None):
    """sklearn.metrics.silhouette_samples(X, labels, metric='euclidean') as a device float32 vector [n] in X's row order.  X: device
    fp16 / fp32 tensor or numpy [n, d] (used as fp16: fp32 is rounded to nearest); labels: integers in [0, k), ids without rows
    allowed; k defaults to labels.max() + 1.  ValueError on a label outside [0, k) and unless 1 < non-empty clusters < n
    (scikit-learn's check)."""
    return _silhouette(X, labels, k)[0]


def silhouette_score(X, labels, k=None):
    """sklearn.metrics.silhouette_score(X, labels, metric='euclidean'): the mean of silhouette_samples, summed in float64 on the device."""
    return float(_silhouette(X, labels, k)[1].item())
