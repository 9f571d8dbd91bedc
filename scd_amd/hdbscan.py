"""HDBSCAN on unit rows: scikit-learn 1.7's HDBSCAN(metric='euclidean', algorithm='brute') without the N x N matrix, on the HIP
primitives of scd_amd/csrc/knn.hip and scd_amd/csrc/hdbscan.hip and the host solver scd_amd/csrc/hdbscan_tree.cpp.
docs/design/hdbscan.md has the semantics, the edge order and the bound.

The core dots (ops.knn) and every Boruvka round's n x n x d search (ops.mr_nearest) are HIP; the per-component choice among n proposals,
the merge of components and the final sort are numpy on the host (n-sized, a few times per fit); the condensed tree is a host solver
(ops.hdbscan_tree), as Munkres and the transport solver are.
"""
import math

import numpy as np
import torch

from . import ops

MAX_MIN_SAMPLES = 65            # scikit-learn's min_samples counts the row itself: scd_knn's k = min_samples - 1 <= 64
_UNSUPPORTED = {"cluster_selection_epsilon": 0.0, "max_cluster_size": None, "metric": "euclidean", "metric_params": None, "alpha": 1.0,
                "store_centers": None}


def _check_min_samples(n, min_samples):
    if not 1 <= min_samples <= MAX_MIN_SAMPLES:
        raise ValueError("min_samples = %d outside the limit 1 <= min_samples <= %d" % (min_samples, MAX_MIN_SAMPLES))
    if not 2 <= n < 2 ** 31:
        raise ValueError("n = %d rows outside the limit 2 <= n < 2^31" % n)
    if min_samples > n:
        raise ValueError("min_samples = %d exceeds the limit min_samples <= n = %d" % (min_samples, n))


def core_dots(u, min_samples):
    """(core float64 [n] on the device, ops.knn's info or None): the dot of each row of u with its (min_samples - 1)-th nearest other row
    (scikit-learn's min_samples counts the row itself); +inf, that is core distance 0, at min_samples = 1."""
    n = u.shape[0]
    if min_samples == 1:
        return torch.full((n,), float("inf"), dtype=torch.float64, device=u.device), None
    _, dot, info = ops.knn(u, u, min_samples - 1, self_base=0)
    return dot[:, min_samples - 2].contiguous(), info


def _merge(comp, lo, hi):
    """The components after joining those of the rows lo[e] and hi[e]: labels by the smallest old label (hooking and pointer jumping)."""
    ids, inv = np.unique(comp, return_inverse=True)
    a, b = inv[lo], inv[hi]
    lab = np.arange(len(ids))
    while True:
        new = lab.copy()
        np.minimum.at(new, a, lab[b])
        np.minimum.at(new, b, lab[a])
        new = new[new]
        if np.array_equal(new, lab):
            return lab[inv]
        lab = new


def choose_edges(comp, nn, r):
    """One round's edges from the rows' proposals (nn [n], r [n]; nn = -1: none): per component the best proposal by the edge order
    (r descending, lo ascending, hi ascending), an edge proposed from both sides once -> (lo, hi, r), unordered."""
    rows = np.nonzero(nn >= 0)[0]
    j = nn[rows].astype(np.int64)
    lo, hi, rv, cv = np.minimum(rows, j), np.maximum(rows, j), r[rows], comp[rows]
    order = np.lexsort((hi, lo, -rv, cv))
    first = np.ones(len(order), dtype=bool)
    first[1:] = cv[order][1:] != cv[order][:-1]
    pick = order[first]
    pairs, where = np.unique(np.stack([lo[pick], hi[pick]], 1), axis=0, return_index=True)
    return pairs[:, 0], pairs[:, 1], rv[pick][where]


def mutual_reachability_mst(x, min_samples, normalize=True):
    """x: device fp16 / fp32 tensor or numpy [n, d].  The unique minimum spanning tree of the mutual-reachability graph of the unit rows
    under the strict edge order (r descending, lo ascending, hi ascending), r_ij = min(core_i, core_j, float64 dot), by Boruvka rounds of
    ops.mr_nearest -> (lo int32 [n - 1], hi int32 [n - 1], r float64 [n - 1], weight float64 [n - 1] = sqrt(max(0, 2 - 2 r)), info),
    numpy arrays sorted by the edge order.  info: dict(rounds, round_info = each round's ops.mr_nearest info as a list, components =
    the components before each round, knn = ops.knn's info of the core-dot call or None).  normalize=False takes the rows as given."""
    from .knn import _as_device_f32, unit_rows
    x = _as_device_f32(x)
    n, min_samples = x.shape[0], int(min_samples)
    _check_min_samples(n, min_samples)
    u = unit_rows(x) if normalize else x
    core, kinfo = core_dots(u, min_samples)
    ws = ops.mr_nearest_workspace(u)
    comp = np.arange(n, dtype=np.int64)
    lo_all, hi_all, r_all = [], [], []
    info = dict(rounds=0, round_info=[], components=[], knn=None if kinfo is None else kinfo.cpu().tolist())
    ncomp, max_rounds = n, max(1, math.ceil(math.log2(n)))
    while ncomp > 1:
        if info["rounds"] == max_rounds:
            raise RuntimeError("mutual_reachability_mst: %d components left after ceil(log2 n) = %d rounds" % (ncomp, max_rounds))
        nn, r, rinfo = ops.mr_nearest(u, core, torch.as_tensor(comp.astype(np.int32), device=u.device), ws=ws, prepared=info["rounds"] > 0)
        info["components"].append(ncomp)
        info["rounds"] += 1
        info["round_info"].append(rinfo.cpu().tolist())
        lo, hi, rv = choose_edges(comp, nn.cpu().numpy(), r.cpu().numpy())
        comp = _merge(comp, lo, hi)
        left = len(np.unique(comp))
        if len(lo) != ncomp - left:
            raise RuntimeError("mutual_reachability_mst: %d edges joined %d components into %d" % (len(lo), ncomp, left))
        ncomp = left
        lo_all.append(lo)
        hi_all.append(hi)
        r_all.append(rv)
    lo, hi, rv = np.concatenate(lo_all), np.concatenate(hi_all), np.concatenate(r_all)
    order = np.lexsort((hi, lo, -rv))
    lo, hi, rv = lo[order].astype(np.int32), hi[order].astype(np.int32), rv[order]
    return lo, hi, rv, np.sqrt(np.maximum(0.0, 2.0 - 2.0 * rv)), info


def attach_noise(x, labels):
    """A full partition from HDBSCAN's labels: each noise row (label -1) takes the label of its nearest clustered row by cosine similarity
    (ops.knn with the noise rows as queries, the clustered rows as base, k = 1).  x as for fit; labels numpy int [n] -> numpy int64 [n].
    With no clustered row there is nothing to attach to: the labels come back unchanged."""
    from .knn import _as_device_f32, unit_rows
    labels = np.asarray(labels, dtype=np.int64)
    noise = labels < 0
    if not noise.any() or noise.all():
        return labels.copy()
    u = unit_rows(_as_device_f32(x))
    keep = torch.as_tensor(np.nonzero(~noise)[0], device=u.device)
    idx, _, _ = ops.knn(u[torch.as_tensor(np.nonzero(noise)[0], device=u.device)].contiguous(), u[keep].contiguous(), 1, self_base=-1)
    out = labels.copy()
    out[noise] = labels[~noise][idx[:, 0].cpu().numpy()]
    return out


class HDBSCAN:
    """HDBSCAN(min_cluster_size=5, min_samples=None, cluster_selection_method='eom', allow_single_cluster=False).fit(x): scikit-learn's
    HDBSCAN(metric='euclidean', algorithm='brute') on the unit rows of x.  min_samples=None means min_cluster_size, as in scikit-learn.

    After fit: labels_ (numpy int64 [n], noise = -1), probabilities_ (numpy float64 [n]), n_clusters_, mst_ = (lo, hi, r, weight) and
    info_ (mutual_reachability_mst's)."""

    def __init__(self, min_cluster_size=5, min_samples=None, cluster_selection_method="eom", allow_single_cluster=False, **unsupported):
        for name, value in unsupported.items():
            if name not in _UNSUPPORTED:
                raise ValueError("HDBSCAN: unknown argument %r" % name)
            if value != _UNSUPPORTED[name]:
                raise ValueError("HDBSCAN: %s = %r is not supported (only %r)" % (name, value, _UNSUPPORTED[name]))
        if cluster_selection_method not in ops.HDBSCAN_METHODS:
            raise ValueError("HDBSCAN: cluster_selection_method = %r is not one of %s" % (cluster_selection_method, sorted(ops.HDBSCAN_METHODS)))
        if int(min_cluster_size) < 2:
            raise ValueError("HDBSCAN: min_cluster_size = %d must be at least 2" % min_cluster_size)
        self.min_cluster_size = int(min_cluster_size)
        self.min_samples = None if min_samples is None else int(min_samples)
        self.cluster_selection_method, self.allow_single_cluster = cluster_selection_method, bool(allow_single_cluster)

    def fit(self, x, y=None):
        ms = self.min_cluster_size if self.min_samples is None else self.min_samples
        lo, hi, r, weight, info = mutual_reachability_mst(x, ms)
        self.labels_, self.probabilities_, self.n_clusters_ = ops.hdbscan_tree(lo, hi, weight, self.min_cluster_size,
                                                                              self.cluster_selection_method, self.allow_single_cluster)
        self.mst_, self.info_ = (lo, hi, r, weight), info
        return self

    def fit_predict(self, x, y=None):
        return self.fit(x).labels_
