"""Ward agglomerative clustering on the HIP device: scipy's linkage(x, 'ward') / scikit-learn's AgglomerativeClustering(linkage='ward')
without the n x n matrix.  One fit gives the whole tree; every K from 1 to n is a cut of it.

The contract is a procedure (docs/design/ward.md): rounds of ops.ward_nearest on the stale clusters, the reciprocal nearest pairs of a
round merged at once by ops.ward_merge (Ward linkage is reducible), the lower position kept.  The device decides every neighbour and
computes every centroid; the reciprocal test, the stale set and the linkage bookkeeping here are small numpy work."""
import numpy as np
import torch

from . import ops

_UNSUPPORTED = dict(metric="euclidean", affinity="euclidean", memory=None, connectivity=None, compute_full_tree="auto", linkage="ward",
                    distance_threshold=None, compute_distances=True)


# ---------------------------------------------------------------------------------------------------- the tree from the merges
def linkage_from_merges(n, a, b, height):
    """The merges in creation order (a[t], b[t] = the two nodes, leaves 0 .. n - 1, merge t = node n + t; height[t]) -> (Z float64
    [n - 1, 4] as scipy's linkage, inversions).  Rows are ordered by (key, creation), key = max(own height, the children's keys): a child
    comes before its parent even where rounding inverts two heights by an ulp; the heights are reported as computed."""
    a, b, height = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.asarray(height, dtype=np.float64)
    t = len(a)
    if t != n - 1:
        raise ValueError("linkage_from_merges: %d merges for %d rows" % (t, n))
    key, size, inversions = [0.0] * (n + t), [1] * (n + t), 0   # plain lists: the loop is sequential
    for s, (p, q, h) in enumerate(zip(a.tolist(), b.tolist(), height.tolist())):
        below = max(key[p], key[q])
        inversions += h < below
        key[n + s] = max(h, below)
        size[n + s] = size[p] + size[q]
    key, size = np.array(key), np.array(size, dtype=np.int64)
    order = np.lexsort((np.arange(t), key[n:]))
    new_id = np.arange(n + t)
    new_id[n + order] = n + np.arange(t)
    za, zb = new_id[a[order]], new_id[b[order]]
    z = np.empty((t, 4))
    z[:, 0], z[:, 1], z[:, 2], z[:, 3] = np.minimum(za, zb), np.maximum(za, zb), height[order], size[n + order]
    return z, inversions


def cut_tree(Z, n_clusters):
    """labels int64 [n] of the cut of Z at n_clusters: the first n - n_clusters merges applied; clusters numbered by their lowest row."""
    Z = np.asarray(Z, dtype=np.float64)
    n, k = Z.shape[0] + 1, int(n_clusters)
    if Z.ndim != 2 or Z.shape[1] != 4:
        raise ValueError("cut_tree: Z must be a linkage matrix [n - 1, 4]")
    if not 1 <= k <= n:
        raise ValueError("cut_tree: n_clusters = %d outside [1, %d]" % (k, n))
    za, zb = Z[:, 0].astype(np.int64).tolist(), Z[:, 1].astype(np.int64).tolist()
    low = list(range(2 * n - 1))                                # the lowest row of each node
    for s in range(n - 1):
        low[n + s] = min(low[za[s]], low[zb[s]])
    root = list(range(2 * n - 1))                               # top-down: a node merged before the cut takes its parent's root
    for s in range(n - k - 1, -1, -1):
        root[za[s]] = root[zb[s]] = root[n + s]
    rep = np.array(low)[np.array(root[:n], dtype=np.int64)]
    return np.unique(rep, return_inverse=True)[1].astype(np.int64)


# ---------------------------------------------------------------------------------------------------- the round loop
def reciprocal_pairs(live, nn, cost):
    """The pairs (lo, hi) with nn[lo] == hi and nn[hi] == lo among the live positions, in (cost, lo, hi) order."""
    j = nn[live]
    ok = j > live
    lo, hi = live[ok], j[ok]
    ok = nn[hi] == lo
    lo, hi = lo[ok], hi[ok]
    order = np.lexsort((hi, lo, cost[lo]))
    return lo[order], hi[order]


def ward_tree(x, normalize=False, compact=True, profile=False):
    """x: device fp16 / fp32 tensor or numpy [n, d], 2 <= n < 2^29, d <= 1024 -> (Z float64 [n - 1, 4], info).  Z is scipy's linkage
    matrix: heights sqrt(2 cost).  normalize=True clusters the unit rows.  info: rounds, queries and live (per round), round_info (each
    round's ops.ward_nearest info), full_requeries, compactions, inversions.  compact=False never renumbers the table (the same Z: a
    measurement switch).  profile=True also times every round (nearest_ms by device events with a synchronise, host_ms the rest of the
    round by the host clock)."""
    import time
    from .knn import _as_device_f32, unit_rows
    x = _as_device_f32(x)
    if x.dim() != 2 or x.shape[0] < 2:
        raise ValueError("ward_tree: x must be [n, d] with n >= 2")
    n, d = x.shape
    tab = unit_rows(x) if normalize else x.clone()
    tab = tab.contiguous()
    dev = tab.device
    xcnt = torch.ones(n, dtype=torch.int32, device=dev)
    ws = ops.ward_workspace(n, n, d, dev)
    cnt = np.ones(n, dtype=np.int64)                            # the host's copy of the sizes
    node = np.arange(n, dtype=np.int64)                         # the tree node at each position
    nn = np.full(n, -1, dtype=np.int64)
    cost = np.full(n, np.inf)
    stale = np.arange(n, dtype=np.int64)
    full, prepared, nlive = True, 0, n
    ma, mb, mh = [], [], []
    info = dict(rounds=0, queries=[], live=[], round_info=[], full_requeries=0, compactions=0, inversions=0)
    if profile:
        info.update(nearest_ms=[], host_ms=[])
    while nlive > 1:
        m = tab.shape[0]
        t_round = time.perf_counter()
        if len(stale) == m:
            q, qcnt, qself = tab, xcnt, torch.arange(m, dtype=torch.int32, device=dev)
        else:
            idx = torch.as_tensor(stale, device=dev)
            q, qcnt, qself = tab.index_select(0, idx), xcnt.index_select(0, idx), idx.to(torch.int32)
        if profile:
            ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev[0].record()
        nn_q, cost_q, rinfo = ops.ward_nearest(q, qcnt, qself, tab, xcnt, ws=ws, prepared=prepared)
        if profile:
            ev[1].record()
            ev[1].synchronize()
            info["nearest_ms"].append(ev[0].elapsed_time(ev[1]))
            info["host_ms"].append(-info["nearest_ms"][-1])
        prepared = m
        nn[stale], cost[stale] = nn_q.cpu().numpy(), cost_q.cpu().numpy()
        info["rounds"] += 1
        info["queries"].append(int(len(stale)))
        info["live"].append(int(nlive))
        info["round_info"].append(rinfo.cpu().tolist())
        live = np.nonzero(cnt > 0)[0]
        lo, hi = reciprocal_pairs(live, nn, cost)
        if len(lo) == 0:
            if full:
                raise RuntimeError("ward_tree: no reciprocal pair among %d clusters after a full query" % nlive)
            info["full_requeries"] += 1                         # float32 centroids: a cached neighbour was overtaken
            stale, full = live, True
            if profile:
                info["host_ms"][-1] += 1e3 * (time.perf_counter() - t_round)
            continue
        ops.ward_merge(tab, xcnt, torch.as_tensor(lo.astype(np.int32), device=dev), torch.as_tensor(hi.astype(np.int32), device=dev), ws)
        ma.append(node[lo])
        mb.append(node[hi])
        node[lo] = n + n - nlive + np.arange(len(lo))           # n - nlive merges so far
        mh.append(np.sqrt(2.0 * cost[lo]))
        cnt[lo] += cnt[hi]
        cnt[hi] = 0
        nlive -= len(lo)
        touched = np.zeros(m, dtype=bool)
        touched[lo] = touched[hi] = True
        live = np.nonzero(cnt > 0)[0]
        is_stale = touched[live] | touched[np.maximum(nn[live], 0)] | (nn[live] < 0)
        stale, full = live[is_stale], bool(is_stale.all())
        if compact and 2 * nlive < m and nlive > 1:             # an order-preserving renumbering: no decision depends on it
            new = np.full(m, -1, dtype=np.int64)
            new[live] = np.arange(nlive)
            keep = torch.as_tensor(live, device=dev)
            tab, xcnt = tab.index_select(0, keep).contiguous(), xcnt.index_select(0, keep).contiguous()
            cnt, node, cost = cnt[live], node[live], cost[live]
            nn = np.where(nn[live] >= 0, new[np.maximum(nn[live], 0)], -1)
            stale, prepared = new[stale], 0
            info["compactions"] += 1
        if profile:
            torch.cuda.synchronize()
            info["host_ms"][-1] += 1e3 * (time.perf_counter() - t_round)
    z, info["inversions"] = linkage_from_merges(n, np.concatenate(ma), np.concatenate(mb), np.concatenate(mh))
    return z, info


# ---------------------------------------------------------------------------------------------------- the estimator
def _same(value, only):
    try:
        return value is only or bool(value == only)
    except (TypeError, ValueError):                             # an array, a callable: not the one value taken
        return False


class Ward:
    """Ward(n_clusters=2, normalize=False).fit(x): scikit-learn's AgglomerativeClustering(n_clusters, linkage='ward') on the rows of x
    (normalize=True: on their unit rows).  After fit: labels_ (numpy int64 [n], clusters numbered by their lowest row), linkage_ (scipy's
    Z), children_, distances_, n_leaves_, n_clusters_ and info_ (ward_tree's).  cut(K) gives the labels at any other K without a refit."""

    def __init__(self, n_clusters=2, normalize=False, **unsupported):
        for name, value in unsupported.items():
            if name not in _UNSUPPORTED:
                raise ValueError("Ward: unknown argument %r" % name)
            if not _same(value, _UNSUPPORTED[name]) and not (name == "compute_distances" and value is False) \
                    and not (name == "compute_full_tree" and value is True):
                raise ValueError("Ward: %s = %r is not supported (only %r): Ward linkage on Euclidean distances, the full tree, no "
                                 "connectivity and no distance_threshold" % (name, value, _UNSUPPORTED[name]))
        if n_clusters is None or int(n_clusters) < 1:
            raise ValueError("Ward: n_clusters = %r must be a positive integer (distance_threshold is not supported)" % (n_clusters,))
        self.n_clusters, self.normalize = int(n_clusters), bool(normalize)

    def fit(self, x, y=None):
        z, info = ward_tree(x, normalize=self.normalize)
        self.linkage_, self.info_ = z, info
        self.children_, self.distances_ = z[:, :2].astype(np.int64), z[:, 2].copy()
        self.n_leaves_ = z.shape[0] + 1
        self.n_clusters_ = self.n_clusters
        self.labels_ = cut_tree(z, self.n_clusters)
        return self

    def fit_predict(self, x, y=None):
        return self.fit(x).labels_

    def cut(self, n_clusters):
        return cut_tree(self.linkage_, n_clusters)
