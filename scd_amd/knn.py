"""Exact cosine k nearest neighbours and the weighted k-NN classifier of the DINO / DINOv2 evaluation protocol (Caron et al., ICCV 2021,
section 4.1: k = 20, temperature 0.07) on the HIP primitives of scd_amd/csrc/knn.hip.  docs/design/knn.md has the semantics.

The n x n x d passes and the float64 decision (ops.knn), the vote (ops.knn_vote) and the unit rows (ops.segment_mean_unit on singleton
segments: FINCH's rule 1, the norm in float64) are HIP; torch does the index plumbing.  There is no dense N x N matrix at any size.
"""
import numpy as np
import torch

from . import ops

WEIGHTS = {"uniform": ops.KNN_UNIFORM, "softmax": ops.KNN_SOFTMAX}


def _as_device_f32(x):
    if isinstance(x, np.ndarray):
        x = torch.as_tensor(np.ascontiguousarray(x))
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError("k-NN needs a 2-d array of rows")
    if not x.is_cuda:
        x = x.cuda()
    return x.float().contiguous()


def unit_rows(x):
    """x / |x| as fp32 with the norm in float64; a zero row stays zero (FINCH's rule 1, the same kernel)."""
    n = x.shape[0]
    ident = torch.arange(n + 1, device=x.device)
    return ops.segment_mean_unit(x, ident[:n].to(torch.int32), ident)[1]


def knn_graph(x, k, queries=None, normalize=True):
    """The k nearest rows of x for every row of x (queries=None: the k-NN graph, a row is not its own neighbour) or for every row of
    `queries` (nothing excluded), by cosine similarity (normalize=True) or by the inner product of the rows as given.
    Returns (idx int64 [m, k], sim float64 [m, k], info int32 [4] as ops.knn), on the device, neighbours ordered by (sim descending,
    index ascending)."""
    x = _as_device_f32(x)
    u = unit_rows(x) if normalize else x
    if queries is None:
        idx, sim, info = ops.knn(u, u, k, self_base=0)
    else:
        q = _as_device_f32(queries)
        idx, sim, info = ops.knn(unit_rows(q) if normalize else q, u, k, self_base=-1)
    return idx.long(), sim, info


def knn_classify(train_x, train_y, test_x=None, k=20, temperature=0.07, weights='softmax', return_info=False):
    """Weighted k-NN predictions from the labelled rows (train_x, train_y) for test_x, or leave-one-out for the training rows themselves
    (test_x=None).  weights: 'softmax' (exp(cosine / temperature), DINO's) or 'uniform' (scikit-learn's KNeighborsClassifier).  A
    negative training label does not vote.  Returns pred int64 [m] on the device (-1: no neighbour voted)."""
    if weights not in WEIGHTS:
        raise ValueError("weights must be 'softmax' or 'uniform', not %r" % (weights,))
    train_x = _as_device_f32(train_x)
    y = torch.as_tensor(np.asarray(train_y.cpu() if torch.is_tensor(train_y) else train_y)).to(train_x.device).to(torch.int32).contiguous()
    if y.dim() != 1 or y.numel() != train_x.shape[0]:
        raise ValueError("one label per training row")
    idx, sim, info = knn_graph(train_x, k, queries=test_x)
    pred, _ = ops.knn_vote(idx.to(torch.int32), sim, y, mode=WEIGHTS[weights], temperature=temperature)
    return (pred.long(), info) if return_info else pred.long()


def knn_accuracy(train_x, train_y, test_x=None, test_y=None, k=20, temperature=0.07, weights='softmax', return_info=False):
    """The accuracy of knn_classify against test_y (test_x=None: leave-one-out on the training rows against train_y), a Python float."""
    pred, info = knn_classify(train_x, train_y, test_x, k=k, temperature=temperature, weights=weights, return_info=True)
    want = train_y if test_x is None else test_y
    want = torch.as_tensor(np.asarray(want.cpu() if torch.is_tensor(want) else want)).to(pred.device).long()
    if want.numel() != pred.numel():
        raise ValueError("one target per query row")
    acc = int((pred == want).sum().item()) / pred.numel()      # the exact count over the row count
    return (acc, info) if return_info else acc
