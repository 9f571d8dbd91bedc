"""A numpy float64 restatement of scd_knn / scd_knn_vote (include/scd_hip.h, docs/design/knn.md), the named cases of the k-NN tests,
planted mistakes, and a CPU simulation of the fp16 filter that says how many candidates each row gets (on exact-grid rows: exactly).

The value of a pair is fn_dot64's: element c goes into partial sum c mod 4 in increasing c, then (s0 + s1) + (s2 + s3).  The product of two
float32 values is exact in float64, so `s += a * b` in float64 IS the kernel's fma, and `dot64` returns the device's bits."""
import numpy as np

import finch_cases as fc
from oracle import synth

MISTAKES = ("self", "tie_high", "k_minus_1", "unsorted", "vote_tie_high", "no_temperature", "shard_base")
KNN_MISTAKES = ("self", "tie_high", "k_minus_1", "unsorted", "shard_base")
VOTE_MISTAKES = ("vote_tie_high", "no_temperature")
# mistakes of one code path each, shown on the cases named for that path (tests/test_knn_host.py): only the first tile of a range is seen,
# the exact pass keeps the best of its first chunk, the padding columns of the last tile are admitted with dot 0, the self column is
# admitted with value 0 (the exact pass's placeholder entry)
PATH_MISTAKES = ("first_tile_only", "first_chunk_only", "pad_cols", "self_zero")
TILE = 128              # KNN_BN: columns per tile of the two MFMA passes
CHUNK = 448             # KNN_SLOTS - KNN_KMAX: columns per step of the exact pass


# ---------------------------------------------------------------------------------------------------- the value of a pair
def dot64(a, b):
    """Row-wise fn_dot64 of a [p, d] and b [p, d] (float32) -> float64 [p]."""
    a64, b64 = np.asarray(a, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
    s = np.zeros((4, a64.shape[0]))
    for c in range(a64.shape[1]):
        s[c & 3] += a64[:, c] * b64[:, c]
    return (s[0] + s[1]) + (s[2] + s[3])


def knn_f64(q, x, k, self_base=-1, mistake=None):
    """(idx int64 [m, k], dot float64 [m, k]): per query the k admissible columns with the largest dot64, ordered by (value descending,
    column ascending).  A BLAS float64 product only shortlists: every column within 1e-11 |q_i| max|x_j| of the k-th largest BLAS value -
    a hundred times the error of any summation order - gets its dot64, and those decide."""
    q, x = np.ascontiguousarray(q, dtype=np.float32), np.ascontiguousarray(x, dtype=np.float32)
    if mistake == "pad_cols":                                   # the zero rows that fill the last tile count as columns
        x = np.concatenate([x, np.zeros((-x.shape[0] % TILE, x.shape[1]), dtype=np.float32)])
    m, n = q.shape[0], x.shape[0]
    q64, x64 = q.astype(np.float64), x.astype(np.float64)
    g = q64 @ x64.T
    tol = 1e-11 * np.sqrt((q64 * q64).sum(1)) * np.sqrt((x64 * x64).sum(1)).max() + 1e-300
    if self_base >= 0 and mistake == "self_zero":
        g[np.arange(m), self_base + np.arange(m)] = 0.0
    elif self_base >= 0 and mistake != "self":
        base = 0 if mistake == "shard_base" else self_base
        g[np.arange(m), base + np.arange(m)] = -np.inf
    if mistake == "first_tile_only":
        g[:, (np.arange(n) // TILE) % ranges(m, n, k)[1] != 0] = -np.inf
    if mistake == "first_chunk_only":
        g[:, CHUNK:] = -np.inf
    need = k + 1 if mistake == "k_minus_1" else k
    idx, dot = np.zeros((m, k), dtype=np.int64), np.zeros((m, k))
    cands, wants = [], []
    for i in range(m):
        row = g[i]
        adm = np.nonzero(row > -np.inf)[0]
        assert len(adm) >= k, "k exceeds the admissible columns"
        want = min(need, len(adm))
        kth = np.partition(row[adm], len(adm) - want)[len(adm) - want]
        cands.append(adm[row[adm] >= kth - tol[i]])
        wants.append(want)
    rows, cols = np.repeat(np.arange(m), [len(c) for c in cands]), np.concatenate(cands)
    vals = np.concatenate([dot64(q[rows[s:s + 16384]], x[cols[s:s + 16384]]) for s in range(0, len(rows), 16384)])
    if self_base >= 0 and mistake == "self_zero":
        vals[cols == self_base + rows] = 0.0
    ends = np.cumsum([len(c) for c in cands])
    for i in range(m):
        cand, v, want = cands[i], vals[ends[i] - len(cands[i]):ends[i]], wants[i]
        order = np.lexsort((-cand if mistake == "tie_high" else cand, -v))
        pick = order[:want]
        if mistake == "k_minus_1" and want == k + 1:             # the bound taken from k - 1 columns can lose the k-th: the next one shows
            pick = np.concatenate([pick[:k - 1], pick[k:k + 1]])
        pick = pick[:k]
        if mistake == "unsorted":
            pick = pick[np.argsort(cand[pick], kind="stable")]
        idx[i], dot[i] = cand[pick], v[pick]
    return idx, dot


def vote_f64(idx, dot, labels, k_use=None, mode="softmax", temperature=0.07, mistake=None, return_gap=False):
    """(pred int64 [m], score float64 [m]) of scd_knn_vote; with return_gap also the relative gap between the two best class scores
    (inf with fewer than two classes voting)."""
    idx, dot, labels = np.asarray(idx), np.asarray(dot, dtype=np.float64), np.asarray(labels)
    m, k = idx.shape
    k_use = k if k_use is None else k_use
    t = 1.0 if mistake == "no_temperature" else temperature
    pred, score, gap = np.full(m, -1, dtype=np.int64), np.zeros(m), np.full(m, np.inf)
    for i in range(m):
        sums = {}
        for b in range(k_use):
            j = idx[i, b]
            if j < 0 or j >= len(labels) or labels[j] < 0:
                continue
            w = np.exp((dot[i, b] - dot[i, 0]) / t) if mode == "softmax" else 1.0
            sums[int(labels[j])] = sums.get(int(labels[j]), 0.0) + w
        if not sums:
            continue
        sign = -1 if mistake == "vote_tie_high" else 1
        ranked = sorted(sums.items(), key=lambda cv: (-cv[1], sign * cv[0]))
        pred[i], score[i] = ranked[0]
        if len(ranked) > 1:
            gap[i] = (ranked[0][1] - ranked[1][1]) / ranked[0][1]
    return (pred, score, gap) if return_gap else (pred, score)


# ---------------------------------------------------------------------------------------------------- cases
def _rand(seed, n, d):
    return np.random.RandomState(seed).randn(n, d).astype(np.float32)


def _grid(seed, n, d, amp=4, step=2.0 ** -3):
    return fc.grid_rows(np.random.RandomState(seed), n, d, amp, step)


def _case(x, k, self_base=-1, q=None, m=None, labels=None):
    """q=None, m=None: Q is X; m: Q is X[:m] (self_base 0 or -1); q: other queries."""
    if q is None:
        q = x if m is None else x[:m]
    return dict(q=np.ascontiguousarray(q), x=np.ascontiguousarray(x), k=k, self_base=self_base, labels=labels)


# the shapes of the issue: n in {2, 130, 257, 1000}, m in {1, 129, n}, d in {4, 33, 64, 768, 1024}, k in {1, 16, 17, 64}, k = n - 1 with self
# excluded and k = n without, and (n = 130, k = 64), (n = 257, k = 64): rows that keep fewer than k columns and take the exact pass
def shape_cases():
    out = {}
    out["n2_graph_k1"] = _case(_grid(1, 2, 4), 1, 0)                                       # k = n - 1, self excluded
    out["n2_m1_k2"] = _case(_grid(2, 2, 4), 2, -1, m=1)                                    # k = n, nothing excluded
    out["n17_graph_k16"] = _case(_rand(3, 17, 33), 16, 0)                                  # k = n - 1, self excluded
    out["n64_q129_k64"] = _case(_rand(4, 64, 33), 64, -1, q=_rand(5, 129, 33))             # k = n, nothing excluded
    out["n130_graph_k64"] = _case(_rand(6, 130, 33), 64, 0)                                # 16-lane border: 18 kept columns < k
    out["n257_graph_k64"] = _case(_grid(7, 257, 64), 64, 0)                                # one-tile border, exact ties
    out["n130_m1_d768_k16"] = _case(_rand(8, 130, 768), 16, -1, q=_rand(9, 1, 768))
    out["n257_q129_d1024_k17"] = _case(_rand(10, 257, 1024), 17, -1, q=_rand(11, 129, 1024))
    out["n1000_graph_d64_k17"] = _case(_rand(12, 1000, 64), 17, 0)
    out["n1000_q129_d768_k16"] = _case(_rand(13, 1000, 768), 16, -1, q=_rand(14, 129, 768))
    out["n1000_graph_d33_k1"] = _case(_grid(15, 1000, 33), 1, 0)
    out["n1000_graph_d1024_k64"] = _case(_rand(16, 1000, 1024), 64, 0)
    out["n1000_m129_d4_k16"] = _case(_grid(17, 1000, 4), 16, 0, m=129)                     # a shard at row 0, heavy ties
    return out


def tie_case():
    """Small-integer grid rows with duplicated rows: every dot is exact in any order, and ties reach across tiles and lanes."""
    x = _grid(20, 400, 64, amp=3, step=0.25)
    x[11] = x[12] = x[13] = x[10]
    x[390] = x[5]
    x[200] = x[140] = x[7]
    return _case(x, 5, 0)


SHARD = (200, 460)                                             # starts inside a 128-row panel and spans three


def shard_case():
    """Q = X[a:b] with self_base = a: rows a:b of the k-NN graph of X."""
    x = _rand(21, 1000, 64)
    return _case(x, 12, SHARD[0], q=x[SHARD[0]:SHARD[1]])


def overflow_case(slots):
    """2 * slots + 3 identical rows: every candidate ties, the slots overflow, the answer is the k lowest admissible columns."""
    x = np.tile(np.array([[1.0, 0.5, -0.25, 2.0, 0.0, 1.5, -1.0, 0.75]], dtype=np.float32), (2 * slots + 3, 1))
    return _case(x, 5, 0)


def degenerate_cases():
    out = {}
    x = _rand(30, 300, 40)
    x[0] = 0
    x[150] = 0
    out["zero_rows"] = _case(x, 7, 0)
    out["tiny_2m20"] = _case(_grid(31, 200, 16, amp=5, step=2.0 ** -20), 6, 0)             # every half is subnormal: flushed, e_i carries it
    x = _rand(32, 150, 24)
    x[40, 3] = 131072.0
    out["fp16_overflow"] = _case(x, 9, 0)
    return out


# name -> (N, D, classes, noise, seed, rows cast to fp16 first, k): the two cases that must go through the filter
BLOBS = {"b3000": (3000, 64, 30, 0.6, 50, False, 20), "h2000": (2000, 768, 25, 0.6, 51, True, 10)}
# small blob cases for the scikit-learn comparisons, seeds chosen so that every row has a gap of 1e-5 between its k-th and (k + 1)-th value
# (tests/test_knn_host.py asserts it); v500 has two classes and an odd k, so that no uniform vote ties
SMALL_BLOBS = {"s600": (600, 32, 12, 0.6, 78, False, 20), "v500": (500, 16, 2, 1.5, 60, False, 7), "s300": (300, 48, 5, 1.0, 61, False, 5)}
MIN_VALUE_GAP, MIN_SCORE_GAP = 1e-5, 1e-9


def blob_case(name):
    """The k-NN graph of unit blob rows (finch_cases.unit_rows: the rule the Python layer applies on the device) with their classes."""
    n, d, classes, noise, seed, half, k = {**BLOBS, **SMALL_BLOBS}[name]
    x, y, _ = synth.clustered_features(n, d, classes, seed=seed, center_seed=seed + 100, noise=noise)
    if half:
        x = x.astype(np.float16)
    raw = np.ascontiguousarray(x.astype(np.float32))
    case = _case(fc.unit_rows(raw), k, 0, labels=y.astype(np.int64))
    case["raw"] = raw
    return case


# ---------------------------------------------------------------------------------------------------- the paths that need n > 4096
# More than 32 tiles, so that a range of the two MFMA passes holds several tiles on a device of any size (ranges(), asserted for 64, 256
# and 304 compute units in tests/test_knn_host.py).  The seeds are chosen so that the facts the host test asserts of each case hold.
BORDER = (4000, 4260)                                          # self columns in tiles 31, 32 and 33; tile 33 is the second of its range


def tile_cases():
    out = {}
    x, q = _rand(100, 4097, 33), _rand(101, 129, 33)           # 33 tiles, 17 ranges of 2; the last range: one tile with ONE valid column
    x[4096], x[4095] = 2 * q[5], 2 * q[77]                     # column 4096 is query 5's first neighbour
    out["t33_q129"] = _case(x, 17, -1, q=q)
    out["t65_q129"] = _case(_rand(102, 8200, 64), 16, -1, q=_rand(103, 129, 64))           # 65 tiles, 22 ranges of 3, the last clipped to 2
    out["t34_k64"] = _case(_rand(104, 4225, 40), 64, -1, q=_rand(105, 260, 40))            # k / 4 = 16 ranges wanted, 17 of 2 tiles given
    x = _grid(106, 4300, 64, amp=4, step=2.0 ** -3)            # dots are multiples of 2^-6 below 16: exact in fp32 in any order, many ties
    out["border_shard"] = _case(x, 12, BORDER[0], q=x[BORDER[0]:BORDER[1]])
    out["graph_4225"] = _case(_rand(107, 4225, 32), 20, 0)     # Q is X: 34 panels x 17 ranges of 2, one preparation for both sides
    return out


def _flagged(seed, n):
    x = _rand(seed, n, 24)
    x[n // 3, 3] = 131072.0                                     # does not fit fp16: the flag, every row through the exact pass
    return _case(x, 64, 0)


# name -> seed of the flagged cases: n = 3 chunks + ONE column, an exact multiple of the chunk, one past a chunk
FLAGGED = {"flagged_1345_k64": (110, 1345), "flagged_896": (111, 896), "flagged_449": (112, 449)}


def chunk_cases():
    """The exact pass over several chunks of CHUNK columns with distinct values: a later chunk changes the best so far."""
    out = {}
    x = _rand(108, 4200, 64)
    x[4150] *= 3000.0                                           # max |x| of some thousands fits fp16, but h_max makes every bound huge
    out["hub"] = _case(x, 10, 0, m=200)
    x = (8.0 + 2.0 ** -6 * np.random.RandomState(146).randn(4200, 64)).astype(np.float32)  # same-sign rows, near-ties far below fp16 resolution
    out["offset"] = _case(x, 10, 0, m=200)
    for name, (seed, n) in FLAGGED.items():
        out[name] = _flagged(seed, n)
    return out


def chunks_of(case):
    return -(-case["x"].shape[0] // CHUNK)


def simplex_rows(n=120, d=128):
    """Rows e_i - 1 / d: every pair's dot is exactly -1 / d (d a power of two), every value fits fp16."""
    x = np.full((n, d), -1.0 / d, dtype=np.float32)
    x[np.arange(n), np.arange(n)] += 1.0
    return x


def negative_cases():
    """Every admissible dot is negative: a padding column (approximate dot 0) or the exact pass's self entry (value 0) would win."""
    out = {}
    x = np.abs(_rand(113, 4200, 40)) + 0.25                     # 4200 = 32 * 128 + 104: 24 padding columns
    out["neg_q130"] = _case(x, 9, -1, q=-(np.abs(_rand(114, 130, 40)) + 0.25))
    x = np.abs(_rand(115, 1000, 40)) + 0.25
    x[40, 3] = 131072.0
    out["neg_flagged"] = _case(x, 9, 300, q=-x[300:430])       # the exact pass with a self entry
    out["simplex120"] = _case(simplex_rows(), 5, 0)             # 8 padding columns, all values tie at -1 / 128
    return out


def same_no_self_case():
    """Q is X with nothing excluded: every row's first neighbour is itself, or its lowest-index duplicate."""
    x = _rand(116, 1000, 64)
    x[11] = x[12] = x[13] = x[10]
    return _case(x, 5, -1)


def vote_case():
    """(idx [300, 8], dot, labels in {-1, 0 .. 3}): uniform ties, negative labels, and row 0 with no valid neighbour."""
    x = _rand(40, 300, 8)
    idx, dot = knn_f64(x, x, 8, 0)
    labels = np.random.RandomState(41).randint(-1, 4, size=300).astype(np.int64)
    labels[idx[0]] = -1
    return idx, dot, labels


def margins(case, temperature=0.07):
    """(the smallest gap between the k-th and the (k + 1)-th value over the rows, the smallest relative gap between the two best class
    scores over the rows and both vote modes - inf without labels): what a comparison with another implementation needs."""
    k = case["k"]
    idx, dot = knn_f64(case["q"], case["x"], k + 1, case["self_base"])
    gap = float((dot[:, k - 1] - dot[:, k]).min())
    vote = np.inf
    if case.get("labels") is not None:
        for mode in ("uniform", "softmax"):
            vote = min(vote, float(vote_f64(idx[:, :k], dot[:, :k], case["labels"], mode=mode, temperature=temperature, return_gap=True)[2].min()))
    return gap, vote


# ---------------------------------------------------------------------------------------------------- the filter, simulated
def f16_flushed(a):
    """The filter's operand: fp16 rounding with subnormal halfs flushed to zero, as float32."""
    h = np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)
    h[np.abs(h) < 2.0 ** -14] = 0.0
    return h


def ranges(m, n, k, cu=256):
    """(ny, tiles_per_y) of scd_knn on a device of cu compute units, by the host code's two steps: ny_max (what the workspace is sized
    for) from 1024 blocks, then ny from 4 cu."""
    panels, tiles = -(-m // TILE), -(-n // TILE)
    ny_max = min(32, tiles, max(-(-1024 // panels), -(-k // 4)))
    ny = max(1, min(ny_max, max(-(-4 * cu // panels), -(-k // 4))))
    per = -(-tiles // ny)
    return -(-tiles // per), per


def simulate_filter(case, slots, cu=256, scale=1.0, with_bound=False):
    """The candidate count of every row as scd_knn's two passes form it - float32 dots of the flushed fp16 rows (numpy's summation order,
    not the MFMA's: a simulation), t_i = the k-th largest of the per-range, per-residue-class maxima, every admissible column with
    approximate dot >= t_i - 2 B_i (rounded down to fp32, as the device rounds it) counts.  A row that keeps fewer than k columns has no
    bound: it gets 2 * slots + 1.  On exact-grid rows (every fp16 copy exact, every dot exact in fp32 in any order) this is no simulation
    but the device's count, as long as the float32 rounding of h_i cannot move it: `scale` multiplies B_i to show that it cannot.
    with_bound: also the mask of the rows that have a bound."""
    q, x, k, self_base = case["q"], case["x"], case["k"], case["self_base"]
    m, n, d = q.shape[0], x.shape[0], x.shape[1]
    hq, hx = f16_flushed(q), f16_flushed(x)
    s = hq @ hx.T
    if self_base >= 0:
        s[np.arange(m), self_base + np.arange(m)] = -np.inf
    e_q = np.sqrt(((q.astype(np.float64) - hq) ** 2).sum(1))
    e_x = np.sqrt(((x.astype(np.float64) - hx) ** 2).sum(1))
    h_q, h_x = np.sqrt((hq.astype(np.float64) ** 2).sum(1)), np.sqrt((hx.astype(np.float64) ** 2).sum(1))
    dp = -(-d // 32) * 32
    b = (e_q * (h_x.max() + e_x.max()) + h_q * e_x.max() + 2.0 ** -22 * (dp // 32 + 1) * h_q * h_x.max()) * 1.001 * scale
    ny, per = ranges(m, n, k, cu)
    col = np.arange(n)
    bins = (col // (TILE * per)) * 16 + col % 16
    kept = np.full((m, ny * 16), -np.inf, dtype=np.float32)
    for bn in np.unique(bins):
        kept[:, bn] = s[:, bins == bn].max(1)
    counts, bounded = np.full(m, 2 * slots + 1, dtype=np.int64), np.zeros(m, dtype=bool)
    for i in range(m):
        row = kept[i][kept[i] > -np.inf]
        if len(row) >= k:
            t = np.partition(row, len(row) - k)[len(row) - k]
            want = float(t) - 2.0 * b[i]
            theta = np.float32(want)
            if float(theta) > want:                             # to nearest went up: one down is the value rounded down
                theta = np.nextafter(theta, np.float32(-np.inf))
            counts[i], bounded[i] = int((s[i] >= theta).sum()), True
    return (counts, bounded) if with_bound else counts


def filter_info(case, slots, cu=256):
    """(info[0], info[2], info[3]) of scd_knn as simulate_filter predicts them: rows through the exact pass (no bound, or more candidates
    than slots), rows whose slots overflowed, the largest candidate count of a row (a row without a bound emits nothing)."""
    counts, bounded = simulate_filter(case, slots, cu, with_bound=True)
    over = bounded & (counts > slots)
    return int((~bounded).sum() + over.sum()), int(over.sum()), int(counts[bounded].max()) if bounded.any() else 0
