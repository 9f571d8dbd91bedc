"""A numpy float64 restatement of scd_ward_nearest, scd_ward_merge and the fit on top of them (include/scd_hip.h, docs/design/ward.md),
the named cases of the Ward tests, planted mistakes, and a CPU simulation of the fp16 filter that says how many candidates each query
gets (on exact-grid rows: exactly).

The value of a pair is the contract's: q = fn_dot64(row, row), v = fn_dot64(Q_p, X_j) (knn_cases.dot64's order: the device's bits),
D = max(0, (q_p + q_j) - 2 v), w = (a b) / (a + b), cost = w D, every operation rounded once in float64."""
import numpy as np

import finch_cases as fc
import hdbscan_cases as hc
import knn_cases as kc

MISTAKES = ("no_weight", "sum_as_product", "tie_high", "no_dead_mask", "self", "unweighted_centroid", "merge_at_hi", "stale_kept",
            "threshold_without_2wb")
SLOTS = 512
T_SLACK, K_UP, K_DN, TH_ABS = np.float32(2.0 ** -19), np.float32(1.0 + 2.0 ** -18), np.float32(1.0 - 2.0 ** -18), np.float32(1e-25)
_CHUNK = 512


# ---------------------------------------------------------------------------------------------------- values
def norms(x):
    return kc.dot64(x, x)


def values(q, x):
    """v [nq, m] float64: fn_dot64 of every query with every row, the device's bits."""
    q64, x64 = np.asarray(q, dtype=np.float32).astype(np.float64), np.asarray(x, dtype=np.float32).astype(np.float64)
    s = np.zeros((4, q64.shape[0], x64.shape[0]))
    for c in range(q64.shape[1]):
        s[c & 3] += q64[:, c, None] * x64[None, :, c]
    return (s[0] + s[1]) + (s[2] + s[3])


def pair_costs(q, qcnt, x, xcnt, mistake=None):
    """cost [nq, m] float64 of the contract (a dead column gets w = 0: the caller masks it)."""
    qq, qx, v = norms(q), norms(x), values(q, x)
    dist = np.maximum(0.0, (qq[:, None] + qx[None, :]) - 2.0 * v)
    a, b = np.asarray(qcnt, dtype=np.int64)[:, None], np.asarray(xcnt, dtype=np.int64)[None, :]
    prod = a.astype(np.float64) * b.astype(np.float64)
    den = prod if mistake == "sum_as_product" else (a + b).astype(np.float64)
    w = np.ones_like(dist) if mistake == "no_weight" else prod / np.where(den > 0, den, 1.0)
    return w * dist


def nearest(q, qcnt, qself, x, xcnt, mistake=None):
    """(nn int64 [nq], cost float64 [nq]) of scd_ward_nearest: per query the live column j != qself of the least cost, ties to the lowest
    column; -1 and +inf for a query without one."""
    q, x = np.asarray(q, dtype=np.float32), np.asarray(x, dtype=np.float32)
    qcnt, qself, xcnt = np.asarray(qcnt), np.asarray(qself), np.asarray(xcnt)
    m = x.shape[0]
    nn, best = np.empty(len(q), dtype=np.int64), np.empty(len(q))
    for s in range(0, len(q), _CHUNK):
        e = min(len(q), s + _CHUNK)
        c = pair_costs(q[s:e], qcnt[s:e], x, xcnt, mistake)
        ok = np.ones(c.shape, dtype=bool) if mistake == "no_dead_mask" else np.broadcast_to(xcnt[None, :] > 0, c.shape).copy()
        if mistake != "self":
            ok &= np.arange(m)[None, :] != qself[s:e, None]
        cm = np.where(ok, c, np.inf)
        b = cm.min(axis=1)
        hit = ok & (cm == b[:, None])
        j = (m - 1 - np.argmax(hit[:, ::-1], axis=1)) if mistake == "tie_high" else np.argmax(hit, axis=1)
        none = ~ok.any(axis=1)
        nn[s:e], best[s:e] = np.where(none, -1, j), np.where(none, np.inf, b)
    return nn, best


def merge(x, cnt, lo, hi, mistake=None):
    """scd_ward_merge on copies -> (x float32 [m, d], cnt int64 [m])."""
    x, cnt = np.array(x, dtype=np.float32), np.array(cnt, dtype=np.int64)
    for a, b in zip(lo, hi):
        ca, cb = float(cnt[a]), float(cnt[b])
        xa, xb = x[a].astype(np.float64), x[b].astype(np.float64)
        new = ((xa + xb) / 2.0) if mistake == "unweighted_centroid" else (ca * xa + cb * xb) / float(cnt[a] + cnt[b])
        keep, die = (b, a) if mistake == "merge_at_hi" else (a, b)
        x[keep] = new.astype(np.float32)
        cnt[keep] = cnt[a] + cnt[b]
        cnt[die] = 0
    return x, cnt


def linkage(n, a, b, height):
    """Z of the merges in creation order (nodes: leaves 0 .. n - 1, merge t = n + t), rows by (key, creation), key = max(own height,
    children's keys) -> (Z, inversions)."""
    t = len(a)
    key, size, inv = np.zeros(n + t), np.ones(n + t), 0
    for s in range(t):
        inv += int(height[s] < max(key[a[s]], key[b[s]]))
        key[n + s] = max(height[s], key[a[s]], key[b[s]])
        size[n + s] = size[a[s]] + size[b[s]]
    order = sorted(range(t), key=lambda s: (key[n + s], s))
    new = {n + s: n + r for r, s in enumerate(order)}
    z = np.array([[min(new.get(a[s], a[s]), new.get(b[s], b[s])), max(new.get(a[s], a[s]), new.get(b[s], b[s])), height[s], size[n + s]]
                  for s in order], dtype=np.float64).reshape(-1, 4)
    return z, inv


def fit(x, mistake=None, max_rounds=None):
    """The fit restated, without compaction -> dict(Z, inversions, full_requeries, rounds = a list per round of dict(x, cnt: the table
    before the search; stale, nn, cost: the search; lo, hi: the pairs merged (empty: a full requery follows); x_after, cnt_after)).
    With max_rounds the fit stops early and Z is None."""
    x = np.array(x, dtype=np.float32)
    n = x.shape[0]
    cnt = np.ones(n, dtype=np.int64)
    node = np.arange(n)
    nn, cost = np.full(n, -1, dtype=np.int64), np.full(n, np.inf)
    stale, full = np.arange(n), True
    ma, mb, mh, rounds, requeries = [], [], [], [], 0
    while (cnt > 0).sum() > 1 and (max_rounds is None or len(rounds) < max_rounds):
        nn_q, cost_q = nearest(x[stale], cnt[stale], stale, x, cnt, mistake)
        nn[stale], cost[stale] = nn_q, cost_q
        live = np.nonzero(cnt > 0)[0]
        pairs = [(cost[i], i, nn[i]) for i in live if nn[i] > i and cnt[nn[i]] > 0 and nn[nn[i]] == i]
        pairs.sort()
        lo, hi = np.array([p[1] for p in pairs], dtype=np.int64), np.array([p[2] for p in pairs], dtype=np.int64)
        rec = dict(x=x.copy(), cnt=cnt.copy(), stale=stale.copy(), nn=nn_q, cost=cost_q, lo=lo, hi=hi)
        rounds.append(rec)
        if len(lo) == 0:
            assert not full, "no reciprocal pair after a full query"
            requeries += 1
            stale, full = live, True
            rec.update(x_after=x.copy(), cnt_after=cnt.copy())
            continue
        for c, a, b in pairs:
            ma.append(node[a])
            mb.append(node[b])
            mh.append(np.sqrt(2.0 * c))
            node[a] = node[b] = n + len(ma) - 1
        x, cnt = merge(x, cnt, lo, hi, mistake)
        rec.update(x_after=x.copy(), cnt_after=cnt.copy())
        touched = np.zeros(n, dtype=bool)
        touched[lo] = touched[hi] = True
        live = np.nonzero(cnt > 0)[0]
        if mistake == "stale_kept":
            is_stale = touched[live]
        else:
            is_stale = touched[live] | (nn[live] < 0) | touched[np.maximum(nn[live], 0)]
        stale, full = live[is_stale], bool(is_stale.all())
    z, inv = linkage(n, ma, mb, mh) if (cnt > 0).sum() == 1 else (None, 0)
    return dict(Z=z, inversions=inv, full_requeries=requeries, rounds=rounds)


def partition_of(labels):
    """Canonical labels: clusters numbered by their lowest row."""
    labels = np.asarray(labels)
    first = {}
    for i, l in enumerate(labels):
        first.setdefault(l, i)
    return np.unique(np.array([first[l] for l in labels]), return_inverse=True)[1]


# ---------------------------------------------------------------------------------------------------- the filter, simulated
def simulate_filter(q, qcnt, qself, x, xcnt, scale=1.0, mistake=None, with_answer=False):
    """scd_ward_nearest's two passes -> (counts int64 [nq], bounded bool [nq], covered bool [nq]).  Float32 dots of the flushed fp16 rows
    (numpy's summation order, not the MFMA's: a simulation) and the epilogue's float32 operations one by one: T = q_p + q_j, Dh = T - 2 s,
    sl = T 2^-19 + c_p, U = (max(0, Dh + sl) / (1/a + 1/b)) (1 + 2^-18) on live foreign columns, theta_p their minimum; a column counts
    when max(0, Dh - sl) (1 - 2^-18) <= (theta_p + 1e-25) (1/a + 1/b).  A query without a live foreign column, and every query when a value
    does not fit fp16, has no bound.  covered: the true answer is among the candidates.  On exact-grid rows this is no simulation but the
    device's count; `scale` multiplies B_p to show that its rounding cannot move it."""
    q, x = np.ascontiguousarray(q, dtype=np.float32), np.ascontiguousarray(x, dtype=np.float32)
    qcnt, qself, xcnt = np.asarray(qcnt), np.asarray(qself), np.asarray(xcnt)
    m, d = x.shape
    live = xcnt > 0
    with np.errstate(over="ignore", invalid="ignore"):
        flag = not (np.isfinite(q.astype(np.float16)).all() and np.isfinite(x[live].astype(np.float16)).all())
        hq, hx = kc.f16_flushed(q), kc.f16_flushed(x)
    if flag:
        hq, hx = np.zeros_like(hq), np.zeros_like(hx)
    s = hq @ hx.T
    e_q = np.sqrt(((q.astype(np.float64) - hq) ** 2).sum(1))
    e_x = np.sqrt(((x.astype(np.float64) - hx) ** 2).sum(1))[live]
    h_q, h_x = np.sqrt((hq.astype(np.float64) ** 2).sum(1)), np.sqrt((hx.astype(np.float64) ** 2).sum(1))[live]
    dp = -(-d // 32) * 32
    hmax, emax = (h_x.max(), e_x.max()) if live.any() else (0.0, 0.0)
    b = (e_q * (hmax + emax) + h_q * emax + 2.0 ** -22 * (dp // 32 + 1) * h_q * hmax) * 1.001 * scale
    c = np.zeros(len(q), dtype=np.float32) if mistake == "threshold_without_2wb" else hc._round_up(2.0 * b)
    qf_q, qf_x = norms(q).astype(np.float32), norms(x).astype(np.float32)
    ra = (1.0 / qcnt.astype(np.float64)).astype(np.float32)
    rb = (1.0 / np.where(live, xcnt, 1).astype(np.float64)).astype(np.float32)
    t = qf_q[:, None] + qf_x[None, :]
    dh = t - np.float32(2.0) * s
    sl = t * T_SLACK + c[:, None]
    rs = ra[:, None] + rb[None, :]
    ok = live[None, :] & (np.arange(m)[None, :] != qself[:, None])
    u = np.where(ok, (np.float32(1.0) / rs * np.maximum(dh + sl, np.float32(0.0))) * K_UP, np.float32(np.inf))
    theta = u.min(axis=1)
    bounded = ok.any(axis=1) & np.isfinite(theta) & (not flag)
    cand = ok & (np.maximum(dh - sl, np.float32(0.0)) * K_DN <= (theta + TH_ABS)[:, None] * rs)
    counts = np.where(bounded, cand.sum(axis=1), 0)
    covered = np.ones(len(q), dtype=bool)
    if with_answer:
        nn, _ = nearest(q, qcnt, qself, x, xcnt)
        covered = ~bounded | cand[np.arange(len(q)), np.maximum(nn, 0)]
    return counts, bounded, covered


def filter_info(counts, bounded, flag=False):
    """(info[0], info[1], info[2], info[3]) of scd_ward_nearest as simulate_filter predicts them."""
    over = bounded & (counts > SLOTS)
    return [int((~bounded).sum() + over.sum()), int(flag), int(over.sum()), int(counts[bounded].max()) if bounded.any() else 0]


# ---------------------------------------------------------------------------------------------------- cases
def _blobs(n, d, classes, noise, seed=0):
    x, y = hc._blobs(n, d, classes, noise, 0, seed)
    return fc.unit_rows(x), y


FIT_CASES = ("n2", "n129", "blobs600", "blobs1500", "blobs900", "grid1000", "dups900", "flagged449")
PARTIAL_CASES = {"t34_4300": 2, "hub4200": 2}                  # the restated fit's first rounds only: the searches and the merges
BLOBS = {"blobs600": 6, "blobs1500": 10, "blobs900": 5}


def make_case(name):
    """The rows of a fit case, float32 [n, d]."""
    if name == "n2":
        return np.random.RandomState(227).randn(2, 8).astype(np.float32)
    if name == "n129":                                          # one row in the second panel
        return np.random.RandomState(228).randn(129, 8).astype(np.float32)
    if name == "blobs600":                                      # the last panel holds 88 rows
        return _blobs(600, 16, 6, 0.5)[0]
    if name == "blobs1500":
        return _blobs(1500, 64, 10, 0.6)[0]
    if name == "blobs900":
        return _blobs(900, 32, 5, 0.8)[0]
    if name == "t34_4300":                                      # 34 tiles: two per range; the last column is row `twin`'s answer
        x = fc.unit_rows(np.random.RandomState(220).randn(4300, 40).astype(np.float32))
        g = x.astype(np.float64) @ x.astype(np.float64).T
        np.fill_diagonal(g, -np.inf)
        alone = np.nonzero((g >= g.max(axis=1, keepdims=True) - 1e-6).sum(axis=1) == 1)[0]
        i = int(alone[alone < 4000][0])
        j = int(np.argmax(g[i]))
        x[[j, 4299]] = x[[4299, j]]
        TWIN["t34_4300"] = i
        return x
    if name == "grid1000":                                      # exact in fp16, dots exact in fp32 in any order, hundreds of cost ties
        return fc.grid_rows(np.random.RandomState(222), 1000, 8, 2, 2.0 ** -3)
    if name == "dups900":                                       # 300 rows three times over: cost 0, ties by index
        return np.tile(hc.half_rows(223, 300), (3, 1))
    if name == "hub4200":                                       # one row 3,000 times, the others around it: the slots overflow
        r = np.random.RandomState(224)
        hub = hc.half_rows(225, 1)
        return np.concatenate([np.tile(hub, (3000, 1)), hub + 0.2 / np.sqrt(16) * r.randn(1200, 16)]).astype(np.float32)
    if name == "flagged449":
        x = np.random.RandomState(226).randn(449, 24).astype(np.float32)
        x[149, 3] = 131072.0                                    # does not fit fp16: the flag, every query walks all columns
        return x
    raise KeyError(name)


TWIN = {}                                                       # t34_4300: the row whose first-round answer is the last column
_cache = {}


def solved(name):
    """The case with its restated fit, computed once per process and never changed."""
    if name not in _cache:
        x = make_case(name)
        f = fit(x, max_rounds=PARTIAL_CASES.get(name))
        f["x"] = x
        x.setflags(write=False)
        _cache[name] = f
    return _cache[name]


def search_cases():
    """Single searches: name -> dict(q, qcnt, qself, x, xcnt)."""
    out = {}
    r = np.random.RandomState(230)
    x = r.randn(1000, 24).astype(np.float32)
    ones = np.ones(1000, dtype=np.int32)

    def case(q, qcnt, qself, x, xcnt):
        return dict(q=np.ascontiguousarray(q, dtype=np.float32), qcnt=np.asarray(qcnt, dtype=np.int32), qself=np.asarray(qself, dtype=np.int32),
                    x=np.ascontiguousarray(x, dtype=np.float32), xcnt=np.asarray(xcnt, dtype=np.int32))
    # rectangular: one query and 130 (a second panel of two rows) against 1000 columns, as rows of the table and as foreign rows
    out["rect_q1_self"] = case(x[999:], [1], [999], x, ones)
    out["rect_q1_free"] = case(x[999:], [1], [-1], x, ones)
    idx = np.arange(860, 990)
    out["rect_q130_self"] = case(x[idx], ones[idx], idx, x, ones)
    out["rect_q130_free"] = case(x[idx] + 0.05 * r.randn(130, 24), ones[idx] * 3, -np.ones(130), x, ones)
    # dead positions
    y = r.randn(600, 16).astype(np.float32)
    i = np.arange(600)
    every_other = (i % 2 == 0).astype(np.int32)
    live = np.nonzero(every_other)[0]
    out["dead_every_other"] = case(y[live], every_other[live], live, y, every_other)
    # the dead rows of this table are copies of live ones, shifted a little: unmasked, each would be its original's answer
    y2 = y.copy()
    y2[1::2] = y[0::2] + np.float32(1e-3)
    out["dead_every_other_near"] = case(y2[live], every_other[live], live, y2, every_other)
    panel = np.where((i >= 128) & (i < 256), 0, 1).astype(np.int32)   # a whole tile of columns masked
    live = np.nonzero(panel)[0]
    out["dead_panel"] = case(y[live], panel[live], live, y, panel)
    two = np.zeros(600, dtype=np.int32)
    two[[77, 599]] = (5, 2)
    out["dead_all_but_two"] = case(y[[77, 599]], [5, 2], [77, 599], y, two)
    one = np.zeros(600, dtype=np.int32)
    one[300] = 4
    out["dead_all_but_self"] = case(y[300:301], [4], [300], y, one)         # answers -1 / inf
    # sizes up to 2^20: the weight decides against the distance
    z = r.randn(500, 32).astype(np.float32)
    sizes = np.ones(500, dtype=np.int32)
    sizes[r.choice(500, 12, replace=False)] = 2 ** 20
    sizes[r.choice(500, 40, replace=False)] = r.randint(2, 5000, 40)
    out["sizes"] = case(z, sizes, np.arange(500), z, sizes)
    return out
