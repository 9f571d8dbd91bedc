"""A numpy float64 restatement of scd_mr_nearest and of the fit loop on top of it (include/scd_hip.h, docs/design/hdbscan.md), the named
cases of the HDBSCAN tests, planted mistakes, and a CPU simulation of the fp16 filter that says how many candidates each row gets in a
round (on exact-grid rows: exactly).

The value of a pair is fn_dot64's (knn_cases.dot64 returns the device's bits); r_ij = min(c_i, c_j, v_ij); the edge order is
(r descending, lo ascending, hi ascending), strict and total, so the minimum spanning tree is unique: Prim's algorithm under that order
finds it here, Boruvka rounds find it on the device."""
import numpy as np

import finch_cases as fc
import knn_cases as kc

MISTAKES = ("core_off_by_one", "no_cj_clamp", "tie_high", "no_mask", "component_best_by_r", "threshold_without_ci")
SLOTS = 512


# ---------------------------------------------------------------------------------------------------- values
def values(x):
    """v [n, n] float64: fn_dot64 of every pair of rows, the device's bits (symmetric: the products commute)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    x64 = x.astype(np.float64)
    n, d = x64.shape
    s = np.zeros((4, n, n))
    for c in range(d):
        s[c & 3] += x64[:, c, None] * x64[None, :, c]
    return (s[0] + s[1]) + (s[2] + s[3])


def core_dots(v, min_samples, mistake=None):
    """c [n]: the dot with the (min_samples - 1)-th nearest OTHER row (scikit-learn's min_samples counts the row itself), +inf at 1."""
    n = v.shape[0]
    k = min_samples - 1 + (1 if mistake == "core_off_by_one" else 0)
    if k == 0:
        return np.full(n, np.inf)
    w = v.copy()
    np.fill_diagonal(w, -np.inf)
    return -np.partition(-w, k - 1, axis=1)[:, k - 1]


def reach(v, c, mistake=None):
    """r [n, n] = min(c_i, c_j, v_ij); the planted clamp mistake leaves c_j out (the matrix is then not symmetric)."""
    r = np.minimum(c[:, None], v)
    return r if mistake == "no_cj_clamp" else np.minimum(r, c[None, :])


def nearest_round(r, comp, mistake=None):
    """(nn int64 [n], r_out float64 [n]) of scd_mr_nearest: per row the foreign column of the largest r, ties to the lowest column; -1 and
    -inf for a row without a foreign column."""
    n = r.shape[0]
    comp = np.asarray(comp)
    foreign = comp[:, None] != comp[None, :]
    if mistake == "no_mask":
        foreign = ~np.eye(n, dtype=bool)
    m = np.where(foreign, r, -np.inf)
    best = m.max(axis=1)
    hit = foreign & (m == best[:, None])
    nn = (n - 1 - np.argmax(hit[:, ::-1], axis=1)) if mistake == "tie_high" else np.argmax(hit, axis=1)
    none = ~foreign.any(axis=1)
    return np.where(none, -1, nn).astype(np.int64), np.where(none, -np.inf, best)


# ---------------------------------------------------------------------------------------------------- the tree, two ways
def sort_edges(lo, hi, r):
    order = np.lexsort((hi, lo, -r))
    lo, hi, r = lo[order], hi[order], r[order]
    return lo.astype(np.int32), hi.astype(np.int32), r, np.sqrt(np.maximum(0.0, 2.0 - 2.0 * r))


def mst_prim(r):
    """The unique MST under (r descending, lo ascending, hi ascending) by Prim's algorithm from row 0 -> (lo, hi, r, weight) sorted by
    that order."""
    n = r.shape[0]
    ids = np.arange(n)
    in_tree = np.zeros(n, dtype=bool)
    br, blo, bhi = np.full(n, -np.inf), np.full(n, n), np.full(n, n)
    lo_out, hi_out, r_out = [], [], []
    u = 0
    for _ in range(n - 1):
        in_tree[u] = True
        lo, hi = np.minimum(ids, u), np.maximum(ids, u)
        better = ~in_tree & ((r[u] > br) | ((r[u] == br) & ((lo < blo) | ((lo == blo) & (hi < bhi)))))
        br[better], blo[better], bhi[better] = r[u][better], lo[better], hi[better]
        cand = np.nonzero(~in_tree)[0]
        top = cand[br[cand] == br[cand].max()]
        w = top[np.lexsort((bhi[top], blo[top]))[0]]
        lo_out.append(blo[w])
        hi_out.append(bhi[w])
        r_out.append(br[w])
        u = w
    return sort_edges(np.array(lo_out), np.array(hi_out), np.array(r_out))


def merge(comp, lo, hi):
    """Union-find over the edges: new labels = the smallest old label of each merged set."""
    ids, inv = np.unique(comp, return_inverse=True)
    par = np.arange(len(ids))

    def find(a):
        while par[a] != a:
            par[a] = par[par[a]]
            a = par[a]
        return a
    for a, b in zip(inv[lo], inv[hi]):
        a, b = find(a), find(b)
        if a != b:
            par[max(a, b)] = min(a, b)
    return np.array([find(a) for a in range(len(ids))])[inv]


def boruvka(r, mistake=None, max_rounds=64, on_round=None):
    """The fit loop restated: rounds of nearest_round, per component the best proposal by the edge order, both-sided proposals once,
    merge -> (lo, hi, r, weight sorted, the component labels before each round).  on_round(comp, nn, r_out) sees each round."""
    n = r.shape[0]
    comp = np.arange(n)
    comps, edges = [], {}
    while len(np.unique(comp)) > 1 and len(comps) < max_rounds:
        comps.append(comp.copy())
        nn, best = nearest_round(r, comp, mistake)
        if on_round is not None:
            on_round(comp, nn, best)
        rows = np.nonzero(nn >= 0)[0]
        lo, hi = np.minimum(rows, nn[rows]), np.maximum(rows, nn[rows])
        if mistake == "component_best_by_r":                    # the first row of the largest r, whatever its (lo, hi)
            order = np.lexsort((rows, -best[rows], comp[rows]))
        else:
            order = np.lexsort((hi, lo, -best[rows], comp[rows]))
        first = np.ones(len(rows), dtype=bool)
        first[1:] = comp[rows][order][1:] != comp[rows][order][:-1]
        new = {}
        for q in order[first]:
            new[(int(lo[q]), int(hi[q]))] = best[rows[q]]
        edges.update(new)
        e = np.array(sorted(new), dtype=np.int64).reshape(-1, 2)
        comp = merge(comp, e[:, 0], e[:, 1])
    e = np.array(sorted(edges), dtype=np.int64).reshape(-1, 2)
    return sort_edges(e[:, 0], e[:, 1], np.array([edges[k] for k in sorted(edges)])) + (comps,)


def sklearn_labels(lo, hi, weight, min_cluster_size, method="eom", allow_single_cluster=False):
    """scikit-learn's own make_single_linkage + tree_to_labels on the sorted edges (current_node = lo, next_node = hi)."""
    from sklearn.cluster._hdbscan._linkage import MST_edge_dtype, make_single_linkage
    from sklearn.cluster._hdbscan._tree import tree_to_labels
    mst = np.empty(len(lo), dtype=MST_edge_dtype)
    mst["current_node"], mst["next_node"], mst["distance"] = lo, hi, weight
    labels, prob = tree_to_labels(make_single_linkage(mst), int(min_cluster_size), cluster_selection_method=method,
                                  allow_single_cluster=bool(allow_single_cluster))
    return np.asarray(labels, dtype=np.int64), np.asarray(prob, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------- the filter, simulated
def _round_dn(a64):
    f = a64.astype(np.float32)
    up = f.astype(np.float64) > a64
    f[up] = np.nextafter(f[up], np.float32(-np.inf))
    return f


def _round_up(a64):
    f = a64.astype(np.float32)
    dn = f.astype(np.float64) < a64
    f[dn] = np.nextafter(f[dn], np.float32(np.inf))
    return f


def simulate_filter(x, c, comp, v=None, scale=1.0, mistake=None):
    """One round of scd_mr_nearest's two passes -> (counts int64 [n], bounded bool [n], covered bool [n]).  Float32 dots of the flushed
    fp16 rows (numpy's summation order, not the MFMA's: a simulation), a_ij = min(c_j rounded down to fp32, s_ij) on foreign columns,
    g_i their maximum, theta_i = min(c_i, g_i - B_i) - B_i rounded down to fp32, every foreign column with min(c_j rounded up, s_ij) >=
    theta_i counts.  A row without a foreign column has no bound.  covered (needs v): the row's true answer is among its candidates.
    On exact-grid rows this is no simulation but the device's count; `scale` multiplies B_i to show that its rounding cannot move it."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, d = x.shape
    comp = np.asarray(comp)
    h = kc.f16_flushed(x)
    s = h @ h.T
    e_r = np.sqrt(((x.astype(np.float64) - h) ** 2).sum(1))
    h_r = np.sqrt((h.astype(np.float64) ** 2).sum(1))
    dp = -(-d // 32) * 32
    b = (e_r * (h_r.max() + e_r.max()) + h_r * e_r.max() + 2.0 ** -22 * (dp // 32 + 1) * h_r * h_r.max()) * 1.001 * scale
    foreign = comp[:, None] != comp[None, :]
    bounded = foreign.any(axis=1)
    a_dn = np.where(foreign, np.minimum(_round_dn(c)[None, :], s), np.float32(-np.inf))
    g = a_dn.max(axis=1).astype(np.float64)
    want = (g - b) - b if mistake == "threshold_without_ci" else np.minimum(c, g - b) - b
    theta = _round_dn(np.where(bounded, want, 0.0))
    cand = foreign & (np.minimum(_round_up(c)[None, :], s) >= theta[:, None])
    counts = cand.sum(axis=1)
    covered = np.ones(n, dtype=bool)
    if v is not None:
        nn, _ = nearest_round(reach(v, c), comp)
        covered = ~bounded | cand[np.arange(n), np.maximum(nn, 0)]
    return counts, bounded, covered


def ranges(n, cu=256):
    """(ny, tiles_per_y) of scd_mr_nearest on a device of cu compute units: ny_max from 1024 blocks, then ny from 4 cu."""
    tiles = -(-n // kc.TILE)
    ny = max(1, min(32, tiles, -(-1024 // tiles), -(-4 * cu // tiles)))
    per = -(-tiles // ny)
    return -(-tiles // per), per


def filter_info(counts, bounded):
    """(info[0], info[2], info[3]) of scd_mr_nearest as simulate_filter predicts them."""
    over = bounded & (counts > SLOTS)
    return int((~bounded).sum() + over.sum()), int(over.sum()), int(counts[bounded].max()) if bounded.any() else 0


# ---------------------------------------------------------------------------------------------------- cases
def _blobs(n, d, classes, noise, n_out, seed=0):
    """n blob rows around `classes` unit centres plus n_out Gaussian rows, float32, not yet unit; the truth with -1 for the Gaussian rows."""
    r = np.random.default_rng(seed)
    cen = r.standard_normal((classes, d))
    cen /= np.linalg.norm(cen, axis=1, keepdims=True)
    y = r.integers(0, classes, n)
    x = cen[y] + noise / np.sqrt(d) * r.standard_normal((n, d))
    x = np.concatenate([x, r.standard_normal((n_out, d))]).astype(np.float32)
    return x, np.concatenate([y, -np.ones(n_out, dtype=np.int64)])


def _case(raw, min_samples, min_cluster_size, unit=True, truth=None):
    """unit: the fit's input is `raw` and its rows are finch_cases.unit_rows(raw), the device's rule; otherwise the rows are taken as given
    (mutual_reachability_mst(..., normalize=False)) and the estimator is not run on the case."""
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    return dict(raw=raw, x=fc.unit_rows(raw) if unit else raw, min_samples=min_samples, min_cluster_size=min_cluster_size, unit=unit,
                truth=truth)


def half_rows(seed, n, d=16):
    """Rows with four entries of +-0.5: exactly unit in any precision, dots are multiples of 0.25, unit_rows leaves them as they are."""
    r = np.random.RandomState(seed)
    x = np.zeros((n, d), dtype=np.float32)
    for i in range(n):
        x[i, r.choice(d, 4, replace=False)] = r.choice([-0.5, 0.5], 4)
    return x


BLOBS = ("blobs660", "blobs1650", "blobs900")
# what scikit-learn's HDBSCAN(algorithm='brute') finds on the blob cases: (clusters, noise rows)
SKLEARN_FINDS = {"blobs660": (5, 58), "blobs1650": (10, 148), "blobs900": (4, 6)}


def make_case(name):
    if name == "blobs660":
        x, y = _blobs(600, 16, 6, 0.5, 60)
        return _case(x, 15, 15, truth=y)
    if name == "blobs1650":
        x, y = _blobs(1500, 64, 10, 0.6, 150)
        return _case(x, 5, 20, truth=y)
    if name in ("blobs900", "plain900"):
        x, y = _blobs(900, 32, 5, 0.8, 0)
        return _case(x, 10 if name == "blobs900" else 1, 25, truth=y)
    if name == "t34_4300":                                      # 34 tiles: two per range; the last tile holds 76 valid columns
        x = np.random.RandomState(120).randn(4300, 40).astype(np.float32)
        # plant the last column as a row's answer: a row whose best r is attained by one column alone (BLAS values suffice to pick it;
        # the host test asserts the fact from the float64 answer), and that column's row changes places with the last row
        u = fc.unit_rows(x).astype(np.float64)
        g = u @ u.T
        np.fill_diagonal(g, -np.inf)
        c = -np.partition(-g, 6, axis=1)[:, 6]
        r = np.minimum(np.minimum(c[:, None], c[None, :]), g)
        alone = np.nonzero((r >= r.max(axis=1, keepdims=True) - 1e-6).sum(axis=1) == 1)[0]
        j = int(np.argmax(r[alone[0]]))
        x[[j, 4299]] = x[[4299, j]]
        case = _case(x, 8, 20)
        case["twin"] = int(alone[0]) if alone[0] != 4299 else j
        return case
    if name == "grid1000":                                      # exact in fp16, dots exact in fp32 in any order, hundreds of ties
        return _case(fc.grid_rows(np.random.RandomState(122), 1000, 16, 4, 2.0 ** -3), 4, 10, unit=False)
    if name == "dups900":                                       # every row three times: weight-0 edges, lambda = inf
        return _case(np.tile(half_rows(123, 300), (3, 1)), 3, 5)
    if name == "hub4200":                                       # one row 3,000 times, the others around it: 3,000 tied candidates
        r = np.random.RandomState(124)
        hub = half_rows(125, 1)
        others = hub + 0.2 / np.sqrt(16) * r.randn(1200, 16)
        return _case(np.concatenate([np.tile(hub, (3000, 1)), others]), 10, 20)
    if name in ("flagged449", "flagged1345"):
        n = int(name[7:])
        x = np.random.RandomState(126 + n).randn(n, 24).astype(np.float32)
        x[n // 3, 3] = 131072.0                                 # does not fit fp16: the flag, every row walks all columns
        return _case(x, 4, 5, unit=False)
    if name == "n2":
        return _case(np.random.RandomState(127).randn(2, 8), 2, 2)
    if name == "n129":                                          # one row in the second panel
        return _case(np.random.RandomState(128).randn(129, 8), 5, 5)
    raise KeyError(name)


CASES = ("blobs660", "blobs1650", "blobs900", "plain900", "t34_4300", "grid1000", "dups900", "hub4200", "flagged449", "flagged1345", "n2",
         "n129")
FILTER_CAP_CASES = ("blobs660", "blobs1650", "t34_4300")
_cache = {}


def solved(name):
    """The case with its float64 answer, computed once per process and never changed: v, core, r, the MST by Prim (lo, hi, r_mst, weight),
    the Boruvka restatement's component labels before each round (comps)."""
    if name not in _cache:
        case = make_case(name)
        v = values(case["x"])
        core = core_dots(v, case["min_samples"])
        r = reach(v, core)
        lo, hi, rm, w = mst_prim(r)
        blo, bhi, brm, bw, comps = boruvka(r)
        assert np.array_equal(lo, blo) and np.array_equal(hi, bhi) and np.array_equal(rm, brm), "Boruvka and Prim disagree on " + name
        case.update(v=v, core=core, r=r, lo=lo, hi=hi, r_mst=rm, weight=w, comps=comps)
        for a in (v, core, r, lo, hi, rm, w):
            a.setflags(write=False)
        _cache[name] = case
    return _cache[name]


def masks(n):
    """The component labellings of the mask test: name -> comp int32 [n]."""
    i = np.arange(n)
    panel = np.where((i >= 128) & (i < 256), 1, 2 + i)          # one component = exactly rows 128..255: a whole panel x tile block masked
    wild = np.where(i % 3 == 0, -7 - (i % 5), 2 ** 31 - 1 - (i % 4))
    return {"sevens": (i // 7).astype(np.int32), "halves": (i >= n // 2).astype(np.int32), "all_equal": np.full(n, 3, dtype=np.int32),
            "panel_block": panel.astype(np.int32), "negative_and_huge": wild.astype(np.int32)}
