"""The FINCH cases of tests/golden/finch.npz (tools/gen_finch_golden.py), regenerated from seeds, and a float64 numpy restatement of
the reference's local_utils/finch.py with cosine distance (docs/design/finch.md has the rules and their reference lines), with optional
planted mistakes.  Two forms of one level's graph: the sparse edge rule the device code uses (`level_edges`) and the dense matrix
A = (P + I)(P + I)^T the reference forms (`level_labels_dense`, CPU tests only).

The golden file holds only what cannot be regenerated without the reference: its partitions, cluster counts and req_clust labels."""
import numpy as np

from oracle import synth

# name -> (N, D, K, noise, seed, rows cast to fp16 first, req_clust values)
CASES = {
    "b600": (600, 32, 12, 0.6, 40, False, (13, 50)),
    "b1500": (1500, 48, 37, 0.9, 40, False, (37, 100, 33)),
    "h1200": (1200, 64, 20, 0.6, 42, True, ()),
    "h900": (900, 768, 30, 0.8, 41, True, ()),
    "s600": (600, 32, 12, 0.9, 0, False, ()),                  # the sibling term of min_sim decides its last partition
}
# the cluster counts the reference finds (checked by the generator)
NUM_CLUST = {"b600": [96, 14, 12], "b1500": [251, 38, 30], "h1200": [154, 20], "h900": [132, 30], "s600": [99, 14, 6]}
# the smallest margins the generator demands: top-2 first-neighbour margin over all levels, threshold margin
MIN_NEIGHBOUR_MARGIN, MIN_THRESHOLD_MARGIN = 1e-5, 1e-4
MISTAKES = ("self", "tie_high", "mutual1", "no_sibling", "root", "prev_means")


def case_input(name):
    """float32 [N, D]; the fp16 cases hold fp16-representable values, so `.astype(np.float16)` of them is exact."""
    n, d, k, noise, seed, half, _ = CASES[name]
    x, _, _ = synth.clustered_features(n, d, k, seed=seed, center_seed=seed + 100, noise=noise)
    if half:
        x = x.astype(np.float16)
    return np.ascontiguousarray(x.astype(np.float32))


def tie_case():
    """Small integer-valued rows with exact ties between columns of different components: the case that catches `tie_high`
    (tests/test_finch_host.py; no blob case has an exact tie)."""
    return grid_rows(np.random.RandomState(TIE_SEED), 14, 4, 3)


TIE_SEED = 2


def grid_rows(r, s, d, amp, step=1.0):
    """s rows of d integers in [-amp, amp] times step: float64 dots of such rows are exact."""
    return (r.randint(-amp, amp + 1, size=(s, d)) * step).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the rules
def unit_rows(m):
    """Rule 1: U = M / |M| as fp32, the norm in float64; zero rows stay zero."""
    m64 = np.asarray(m, dtype=np.float32).astype(np.float64)
    nrm = np.sqrt((m64 * m64).sum(axis=1, keepdims=True))
    return np.where(nrm > 0, m64 / np.where(nrm > 0, nrm, 1.0), 0.0).astype(np.float32)


def gram(u):
    u64 = np.asarray(u, dtype=np.float32).astype(np.float64)
    return u64 @ u64.T


def first_neighbor(u, mistake=None, g=None):
    """Rule 2 on rows u (any rows: the dot is not normalised here).  Returns (nn int64 [s], d1 float64 [s])."""
    g = gram(u) if g is None else g.copy()
    s = g.shape[0]
    if mistake != "self":
        g[np.arange(s), np.arange(s)] = -np.inf
    if mistake == "tie_high":
        nn = s - 1 - np.argmax(g[:, ::-1], axis=1)
    else:
        nn = np.argmax(g, axis=1)
    return nn.astype(np.int64), 1.0 - g[np.arange(s), nn]


def sibling_pairs(nn):
    """All pairs a < b with nn[a] = nn[b]."""
    order = np.argsort(nn, kind="stable")
    a, b = [], []
    start = 0
    s = len(nn)
    while start < s:
        end = start
        while end < s and nn[order[end]] == nn[order[start]]:
            end += 1
        grp = order[start:end]
        for p in range(len(grp)):
            for q in range(p + 1, len(grp)):
                a.append(grp[p])
                b.append(grp[q])
        start = end
    return np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)


def pair_dist(u, a, b):
    u64 = np.asarray(u, dtype=np.float32).astype(np.float64)
    return 1.0 - np.einsum("ij,ij->i", u64[a], u64[b]) if len(a) else np.zeros(0)


def mutual_weight(nn, mistake=None):
    nn = np.asarray(nn)
    mutual = nn[nn] == np.arange(len(nn))
    return mutual, np.where(mutual & (mistake != "mutual1"), 2.0, 1.0)


def min_sim_of(u, nn, d1, mistake=None):
    """Rule 4: max(dist * A) over the non-zero entries of A at level 0."""
    _, w = mutual_weight(nn, mistake)
    m = float((w * d1).max())
    if mistake != "no_sibling":
        a, b = sibling_pairs(nn)
        if len(a):
            m = max(m, float(pair_dist(u, a, b).max()))
    return m


def level_edges(u, nn, d1, min_sim, mistake=None):
    """Rule 3, sparse: the undirected edges whose components are those of the thresholded A.  Returns (ea, eb)."""
    nn = np.asarray(nn, dtype=np.int64)
    s = len(nn)
    idx = np.arange(s)
    if min_sim is None:
        return idx, nn
    mutual, w = mutual_weight(nn, mistake)
    keep = ~(w * d1 > min_sim)
    ea, eb = list(idx[keep]), list(nn[keep])
    # the exception: (i, k) a cut mutual pair, nn[j] = k, j != i: the sibling edge j - i survives iff d(i, j) <= min_sim
    k = nn
    i = nn[k]
    cand = (i != idx) & mutual[k] & ~keep[k]
    j = idx[cand]
    if len(j):
        ok = pair_dist(u, i[j], j) <= min_sim
        ea += list(j[ok])
        eb += list(i[j][ok])
    return np.asarray(ea, dtype=np.int64), np.asarray(eb, dtype=np.int64)


def components(s, ea, eb, mistake=None):
    """Rule 5: union-find; labels numbered by the rank of each component's lowest member (`root`: of its highest).  (labels, count)."""
    parent = np.arange(s)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b in zip(ea, eb):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            lo, hi = (ra, rb) if ra < rb else (rb, ra)
            if mistake == "root":
                parent[lo] = hi
            else:
                parent[hi] = lo
    roots = np.array([find(x) for x in range(s)])
    uniq, labels = np.unique(roots, return_inverse=True)
    return labels.astype(np.int64), len(uniq)


def level_labels(u, nn, d1, min_sim, mistake=None):
    ea, eb = level_edges(u, nn, d1, min_sim, mistake)
    return components(len(nn), ea, eb, mistake)


def level_labels_dense(u, nn, min_sim):
    """The reference's form (finch.py:39-52): A = (P + I)(P + I)^T with the diagonal cleared, entries with dist * A > min_sim deleted."""
    s = len(nn)
    p = np.zeros((s, s))
    p[np.arange(s), nn] = 1.0
    p += np.eye(s)
    a = p @ p.T
    a[np.arange(s), np.arange(s)] = 0.0
    if min_sim is not None:
        dist = 1.0 - gram(u)
        dist[np.arange(s), np.arange(s)] = 1000.0
        a[dist * a > min_sim] = 0.0
    ea, eb = np.nonzero(a)
    return components(s, ea, eb)


def segment_means(x, labels, k):
    """Rule 6: the float64 sum of the member rows in row order, divided by the count, rounded to fp32."""
    sums = np.zeros((k, x.shape[1]))
    np.add.at(sums, labels, np.asarray(x, dtype=np.float32).astype(np.float64))
    cnt = np.bincount(labels, minlength=k).astype(np.float64)
    return (sums / cnt[:, None]).astype(np.float32)


def finch_f64(data, initial_rank=None, req_clust=None, mistake=None, return_levels=False):
    """Rules 7-9.  Returns (c int64 [N, P], num_clust list, req_c or None[, levels])."""
    data = np.ascontiguousarray(np.asarray(data).astype(np.float32))
    levels = []
    u = unit_rows(data)
    if initial_rank is None:
        nn, d1 = first_neighbor(u, mistake)
        min_sim = min_sim_of(u, nn, d1, mistake)
    else:
        nn, d1, min_sim = np.asarray(initial_rank, dtype=np.int64), None, None
    lab, k = level_labels(u, nn, d1, None, mistake)
    levels.append(dict(u=u, nn=nn, d1=d1, labels=lab))
    cols, num = [lab], [k]
    means = segment_means(data, lab, k)
    while num[-1] > 1:
        u = unit_rows(means)
        nn, d1 = first_neighbor(u, mistake)
        lab, k = level_labels(u, nn, d1, min_sim, mistake)
        if k == 1 or num[-1] - k < 1:
            break
        levels.append(dict(u=u, nn=nn, d1=d1, labels=lab))
        cols.append(lab[cols[-1]])
        num.append(k)
        means = segment_means(means, lab, k) if mistake == "prev_means" else segment_means(data, cols[-1], k)
    c = np.column_stack(cols)
    req_c = None
    if req_clust is not None:
        req_c = req_labels(data, c, num, int(req_clust), mistake)
    out = (c, num, req_c)
    return out + (levels, min_sim) if return_levels else out


def req_labels(data, c, num, req_clust, mistake=None):
    """Rule 8."""
    if req_clust in num:
        return c[:, num.index(req_clust)]
    ind = [i for i, v in enumerate(num) if v >= req_clust]
    if not ind:
        raise ValueError("req_clust = %d exceeds the first partition's %d clusters" % (req_clust, num[0]))
    cur, k = c[:, ind[-1]], num[ind[-1]]
    means = segment_means(data, cur, k)
    while k > req_clust:
        nn, d1 = first_neighbor(unit_rows(means), mistake)
        i = int(np.argmin(d1))
        u, k = components(k, [i], [int(nn[i])])
        cur = u[cur]
        means = segment_means(data, cur, k)
    return cur


def margins(data):
    """(smallest top-2 first-neighbour margin over all levels, smallest threshold margin): what the generator asserts."""
    _, _, _, levels, min_sim = finch_f64(data, return_levels=True)
    nb, th = np.inf, np.inf
    for li, lv in enumerate(levels):
        g = gram(lv["u"])
        s = g.shape[0]
        g[np.arange(s), np.arange(s)] = -np.inf
        if s > 2:
            top = np.sort(g, axis=1)[:, -2:]
            nb = min(nb, float((top[:, 1] - top[:, 0]).min()))
        if li > 0:
            _, w = mutual_weight(lv["nn"])
            th = min(th, float(np.abs(w * lv["d1"] - min_sim).min()))
    return nb, th
