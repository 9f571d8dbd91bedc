"""FINCH first-neighbour clustering (the reference's local_utils/finch.py; Sarfraz et al., "Efficient Parameter-free Clustering Using
First Neighbor Relations", CVPR 2019) with cosine distance, on the HIP primitives of scd_amd/csrc/finch.hip.  No K and no sweep: one
first-neighbour pass over the rows gives a partition, the same pass over its cluster means the next, coarser one, and so on.

The rules, their reference lines and the derivation of the sparse edge rule are in docs/design/finch.md.  The n x n x d pass
(ops.first_neighbor), the pair distances, the components (ops.link_components) and the means (ops.segment_mean_unit) are HIP; torch
does the index plumbing (stable sort, bincount, cumsum, gather, argmin, composing labels).  The path is exact at any N: there is no
dense N x N matrix and no approximate-neighbour branch (the reference switches to flann above 70,000 rows and applies no threshold
there; beyond that size there is no reference result to match).
"""
import numpy as np
import torch

from . import ops

PAIR_CHUNK = 1 << 22            # sibling pairs evaluated per launch: bounds the pair lists' memory (a hub of in-degree g has g (g - 1) / 2 pairs)


def _as_device_f32(x):
    if isinstance(x, np.ndarray):
        x = torch.as_tensor(np.ascontiguousarray(x))
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError("FINCH needs a 2-d array of rows")
    if not x.is_cuda:
        x = x.cuda()
    if x.dtype not in (torch.float16, torch.float32):
        x = x.to(torch.float32)                                 # finch.py:128 casts to float32
    return x.float().contiguous()


def _segments(labels, k):
    """(order int32 [n]: the stable sort of the rows by label, offsets int64 [k + 1])."""
    lab = labels.long()
    order = torch.sort(lab, stable=True).indices.to(torch.int32)
    counts = torch.bincount(lab, minlength=k)
    offsets = torch.zeros(k + 1, dtype=torch.int64, device=labels.device)
    offsets[1:] = torch.cumsum(counts, 0)
    return order, offsets


def _means(data, labels, k):
    """Rule 6 and rule 1 of the next level: (means float32 [k, d] of the ORIGINAL rows, their unit rows)."""
    order, offsets = _segments(labels, k)
    return ops.segment_mean_unit(data, order, offsets)


def _mutual_weight(nn64):
    idx = torch.arange(nn64.numel(), device=nn64.device)
    mutual = nn64[nn64] == idx
    w = torch.where(mutual, 2.0, 1.0).to(torch.float64)
    return idx, mutual, w


def _max_sibling_dist(u, nn64):
    """The largest distance between two rows that share a first neighbour (None without such a pair), in chunks of PAIR_CHUNK pairs."""
    order = torch.sort(nn64, stable=True).indices
    key = nn64[order]
    s = key.numel()
    pos = torch.arange(s, device=key.device)
    last = torch.ones(s, dtype=torch.bool, device=key.device)
    last[:-1] = key[1:] != key[:-1]
    # end[p]: one past the last position of p's group
    ends = pos[last] + 1
    end = ends[torch.searchsorted(ends, pos, right=True)]
    counts = end - pos - 1                                      # partners of position p: the later positions of its group
    cum = torch.cumsum(counts, 0)
    total = int(cum[-1].item())
    best = None
    for t0 in range(0, total, PAIR_CHUNK):
        t = torch.arange(t0, min(t0 + PAIR_CHUNK, total), device=key.device)
        p = torch.searchsorted(cum, t, right=True)
        off = t - (cum[p] - counts[p])
        a, b = order[p].to(torch.int32), order[p + 1 + off].to(torch.int32)
        m = float(ops.pair_dist_f64(u, a, b).max().item())
        best = m if best is None else max(best, m)
    return best


def _min_sim(u, nn, d1):
    """Rule 4: max(dist * A) over the non-zero entries of A (finch.py:138-139)."""
    nn64 = nn.long()
    _, _, w = _mutual_weight(nn64)
    m = float((w * d1).max().item())
    sib = _max_sibling_dist(u, nn64)
    return m if sib is None else max(m, sib)


def _level_edges(u, nn, d1, min_sim):
    """Rule 3: the undirected edges whose components are those of the reference's thresholded A (finch.py:39-52)."""
    nn64 = nn.long()
    idx, mutual, w = _mutual_weight(nn64)
    if min_sim is None:
        return idx.to(torch.int32), nn.to(torch.int32)
    keep = ~(w * d1 > min_sim)
    ea, eb = idx[keep], nn64[keep]
    # the exception: (i, k) a cut mutual pair and nn[j] = k, j != i: the sibling edge j - i survives iff d(i, j) <= min_sim
    k = nn64
    i = nn64[k]
    j = idx[(i != idx) & mutual[k] & ~keep[k]]
    if j.numel():
        ok = ops.pair_dist_f64(u, i[j].to(torch.int32), j.to(torch.int32)) <= min_sim
        ea, eb = torch.cat([ea, j[ok]]), torch.cat([eb, i[j][ok]])
    return ea.to(torch.int32), eb.to(torch.int32)


def _level_labels(u, nn, d1, min_sim):
    ea, eb = _level_edges(u, nn, d1, min_sim)
    return ops.link_components(nn.numel(), ea, eb)


class Finch:
    """Finch(req_clust=None, distance='cosine').fit(x, initial_rank=None); x: device fp16 / fp32 tensor or numpy [N, D].

    After fit:  partitions_device_ int32 [N, P], num_clust_ (list of P counts), req_labels_device_ (int32 [N] or None), min_sim_
    (float or None), exact_rows_ (per level: the rows that took the exact full-row pass of scd_first_neighbor) and, with
    keep_levels=True, levels_: per level a dict U, nn, d1, labels (the level's component labels), means, exact_rows."""

    def __init__(self, req_clust=None, distance='cosine', keep_levels=False):
        if distance != 'cosine':
            raise ValueError("FINCH: only distance='cosine' is implemented (got %r)" % (distance,))
        self.req_clust = None if req_clust is None else int(req_clust)
        self.distance = distance
        self.keep_levels = keep_levels

    def _neighbours(self, u):
        nn, d1, info = ops.first_neighbor(u)
        return nn, d1, int(info[0].item())

    def fit(self, x, initial_rank=None):
        data = _as_device_f32(x)
        n = data.shape[0]
        if n < 2:
            raise ValueError("FINCH needs at least 2 rows")
        dev = data.device
        self.levels_ = [] if self.keep_levels else None
        self.exact_rows_ = []
        # level 0: unit rows through the kernel of the later levels (singleton segments), the norm in float64
        ident = torch.arange(n + 1, device=dev)
        means, u = ops.segment_mean_unit(data, ident[:n].to(torch.int32), ident)
        if initial_rank is None:
            nn, d1, exact = self._neighbours(u)
            min_sim = _min_sim(u, nn, d1)
        else:                                                   # rule 9: no distances, hence no min_sim (finch.py:22-23)
            nn = torch.as_tensor(np.asarray(initial_rank.cpu() if torch.is_tensor(initial_rank) else initial_rank)).to(dev).to(torch.int32)
            if nn.numel() != n or int(nn.min()) < 0 or int(nn.max()) >= n:
                raise ValueError("initial_rank must hold one row index in [0, N) per row")
            d1, exact, min_sim = None, 0, None
        labels, k = _level_labels(u, nn, d1, None)
        self._note(u, nn, d1, labels, means, exact)
        cols, num = [labels], [k]
        while num[-1] > 1:
            means, u = _means(data, cols[-1], num[-1])
            nn, d1, exact = self._neighbours(u)
            labels, k = _level_labels(u, nn, d1, min_sim)
            if k == 1 or num[-1] - k < 1:                       # finch.py:155-158: the partition is dropped
                break
            self._note(u, nn, d1, labels, means, exact)
            cols.append(labels[cols[-1].long()])
            num.append(k)
        self.partitions_device_ = torch.stack(cols, 1).contiguous()
        self.num_clust_ = num
        self.min_sim_ = min_sim
        self.req_labels_device_ = None if self.req_clust is None else self._required(data, self.req_clust)
        return self

    def _note(self, u, nn, d1, labels, means, exact):
        self.exact_rows_.append(exact)
        if self.keep_levels:
            self.levels_.append(dict(U=u, nn=nn, d1=d1, labels=labels, means=means, exact_rows=exact))

    def _required(self, data, req):
        """Rule 8 (finch.py:95-103, :164-171): one merge of the closest pair of means per step.  (The reference's argsort(...)[:2] merges
        two pairs in one step when two different pairs tie exactly; that is not restated.)"""
        num = self.num_clust_
        if req in num:
            return self.partitions_device_[:, num.index(req)].contiguous()
        ind = [i for i, v in enumerate(num) if v >= req]
        if not ind or req < 1:
            raise ValueError("req_clust = %d is outside [1, %d], the first partition's cluster count" % (req, num[0]))
        cur, k = self.partitions_device_[:, ind[-1]].long(), num[ind[-1]]
        while k > req:
            _, u = _means(data, cur, k)
            nn, d1, _ = ops.first_neighbor(u)
            i = int(torch.argmin(d1).item())                    # the first minimum: lowest i on ties
            j = int(nn[i].item())
            a, b = min(i, j), max(i, j)
            remap = torch.arange(k, device=cur.device)          # rank of the lowest member: b joins a, the labels above b move down
            remap[b] = a
            remap[b + 1:] -= 1
            cur = remap[cur]
            k -= 1
        return cur.to(torch.int32).contiguous()


def FINCH(data, initial_rank=None, req_clust=None, distance='cosine', verbose=True):
    """The reference's FINCH(data, initial_rank, req_clust, distance, verbose) -> (c [N, P], num_clust list, req_c [N] or None), numpy.
    Only distance='cosine'; a req_clust above the first partition's count raises ValueError (the reference: IndexError)."""
    f = Finch(req_clust=req_clust, distance=distance).fit(data, initial_rank=initial_rank)
    if verbose:
        for p, k in enumerate(f.num_clust_):
            print('Partition {}: {} clusters'.format(p, k))
    req_c = None if f.req_labels_device_ is None else f.req_labels_device_.cpu().numpy()
    return f.partitions_device_.cpu().numpy(), list(f.num_clust_), req_c
