"""The silhouette cases of tests/golden/silhouette.npz (tools/gen_silhouette_golden.py), regenerated from seeds, a float64 numpy
restatement of sklearn.metrics.silhouette_samples with optional planted mistakes, and the per-case error bounds of the GPU test.

Rows are oracle/synth.clustered_features output cast to fp16, so rounding them to fp16 again is the identity.  The golden file holds
only what cannot be regenerated without scikit-learn: the expected float64 samples, the scikit-learn KMeans partitions of the blobs
and their silhouette table.

Below those: two EXACT families at the shapes real runs use (docs/design/estimate_k.md, "Measured error"), numpy only, from seeds.

Lattice family (bit for bit).  Row i is t_i * u: t_i a small non-negative integer drawn per row, u a fixed vector of small signed
integers whose squared sum is a perfect square g^2.  Then every fp16 value t_i u_c is an integer of magnitude <= 2048 (exact), every
product of a dot is t_i t_j u_c^2 >= 0, so every MFMA partial sum is a non-negative integer <= g^2 t_i t_j, and every fp32 norm is
the integer g^2 t_i^2; with 2 g^2 max(t)^2 < 2^24 all of them and |x_i|^2 + |x_j|^2 are exact, dist^2 = g^2 (t_i - t_j)^2 exactly,
and a correctly rounded sqrtf returns the integer g |t_i - t_j|.  A row's sum over a cluster is then an integer; if
g max(t) cnt < 2^24 for the largest cluster, every partial sum in ANY order is an integer below 2^24, so the sum is the same
whatever the lanes, tiles and butterflies.  lattice_case() asserts each of these conditions for the case it builds.  What is left is
three IEEE fp32 divisions, a subtraction, comparisons and minima, which lattice_reference() performs in numpy float32 on the exact
integer sums taken from the cluster x t count table, O(n + k max(t)^2): the device's samples must EQUAL it.

General grid family (derived bound).  Rows have independent coordinates j / 8, j an integer in [-4, 4] (a per-cluster centre in
[-2, 2] plus noise in [-2, 2]), so they are in general position and distances are irrational.  Products are multiples of 2^-6 below
1/4 and d <= 1024, so dots, norms and dist^2 = |x_i|^2 + |x_j|^2 - 2 dot are exact in fp32 (integers below 2^24 in units of 2^-6)
and in the float64 GEMM form of the reference.  With u = 2^-24 the device's errors are:
  * sqrtf, correctly rounded: one factor (1 + d), |d| <= u, per term;
  * the sum: a lane adds its T_c = 8 * ceil(cnt_c / 128) terms (8 sub-tile columns per 128-column tile) one after the other, then four
    butterfly additions join the 16 lanes: every term passes through at most T_c + 4 additions.  All terms are >= 0, so the sum is
    within (1 + u)^(1 + T_c + 4) - 1 relative;
  * the division by cnt_c (or cnt - 1 for the own cluster): one more factor.
So a cluster's mean is within eps_c = (T_c + 6) u relative, up to second order.  a carries eps_own; b, a minimum of positive means
each within eps_c of its own value, is within max_c eps_c of the exact minimum.  With r = (1 + e_a) / (1 + e_b) or its inverse,
the exact quotient of the perturbed a and b moves s = 1 - a / b (a <= b; b / a - 1 otherwise; if the perturbation swaps their
order both values lie within r - 1 of 0) by at most r - 1 <= (eps_own + max_c eps_c)(1 + O(eps)).  The finish then rounds b - a and
the division once each on a value of magnitude <= 1: 2 u (the plan for these tests allowed 3 u there; the derivation gives 2 u, which is
what grid_bound() uses):
    |s_dev - s_64| <= (eps_own + max_c eps_c + 2 u) (1 + 1e-3),
the last factor for the second-order terms ((T + 6) u <= 1.6e-5 at 32 tiles) and the float64 reference's own rounding.

kernel_sums() restates which sorted slots sl_main_kernel adds for which cluster, on count tables (slots grouped into classes: the t
values of the lattice, or single slots on the grid), with the seven planted mistakes of tests/test_silhouette_host.py."""
import numpy as np

from oracle import synth

# K visited by estimate_k.grid_search on [2, 64] when the maximum is at 20 (tests/test_silhouette_host.py checks the rounds)
GRID_KS = [2, 10, 12, 14, 16, 18, 19, 20, 21, 23, 25, 33, 41, 49, 56, 64]

# Largest |s_device - s_golden| over a case's rows, measured on an MI355X (docs/design/estimate_k.md, "Measured error"), and the test
# bound = 4 x that.  The summation order is fixed by the labels, so the margin is for compiler changes only.
MEASURED = {
    "ragged": 1.82e-7, "long_segment": 2.05e-7, "pad_d": 1.31e-7, "odd_d": 1.41e-7, "many_tiny": 2.16e-7, "blobs_true": 1.51e-7,
    "blobs_fit": 1.51e-7, "shuffled": 1.55e-7,
}


def bound(name):
    return 4.0 * MEASURED[name]


def blobs(n):
    """tests/test_gpu_cluster_scores.py::blobs: D = 64, 20 true classes, noise 0.6 / sqrt(D), labelled rows first."""
    x, y, _ = synth.clustered_features(n, 64, 20, noise=0.6)
    perm, mask_lab = synth.labelled_split(y, 20, prop=0.5)
    return x[perm], y[perm], mask_lab


def _f16(x):
    return np.ascontiguousarray(x.astype(np.float16))


def _ragged():
    x, y, _ = synth.clustered_features(257, 64, 5, seed=21, center_seed=22)
    labels = np.where(y == 4, 5, y)                                 # id 4 stays empty
    for c, keep in ((0, 1), (1, 2), (2, 3), (3, 5)):                # sizes 1, 2, 3, 5; the other members join the big cluster
        idx = np.nonzero(y == c)[0]
        labels[idx[keep:]] = 5
    return _f16(x), labels.astype(np.int64)


def cases(gold=None):
    """name -> (x fp16 [n, d], labels int64 [n], k).  `blobs_fit` (labels of scikit-learn's K = 20 fit) needs the golden file."""
    out = {}
    x, labels = _ragged()
    out["ragged"] = (x, labels, 6)
    xs, ys, _ = synth.clustered_features(1100, 64, 11, seed=23, center_seed=24)
    out["long_segment"] = (_f16(xs), np.where(ys < 7, 0, np.where(ys < 10, 1, 2)).astype(np.int64), 3)
    xs, ys, _ = synth.clustered_features(300, 40, 7, seed=25, center_seed=26)
    out["pad_d"] = (_f16(xs), ys, 7)
    xs, ys, _ = synth.clustered_features(1000, 96, 37, seed=27, center_seed=28)
    out["odd_d"] = (_f16(xs), ys, 37)
    xs, ys, _ = synth.clustered_features(640, 768, 130, seed=29, center_seed=30)
    out["many_tiny"] = (_f16(xs), ys, 130)
    xb, yb, _ = blobs(3000)
    out["blobs_true"] = (_f16(xb), yb, 20)
    if gold is not None:
        out["blobs_fit"] = (_f16(xb), gold["blobs_part"][GRID_KS.index(20)].astype(np.int64), 20)
    xs, ys, _ = synth.clustered_features(64, 64, 4, seed=31, center_seed=32)
    xs = _f16(xs)
    c0 = np.nonzero(ys == 0)[0]
    xs[c0[1:4]] = xs[c0[0]]                                         # four identical rows inside cluster 0
    xs[np.nonzero(ys == 2)[0][0]] = xs[np.nonzero(ys == 1)[0][0]]   # two identical rows in different clusters
    out["duplicates"] = (xs, ys, 4)
    r = np.random.RandomState(33)
    out["shuffled"] = (x, np.array([3, 5, 0, 1, 4, 2])[labels[r.permutation(labels.size)]], 6)
    return out


def distances_f64(x):
    """Euclidean distances from coordinate differences in float64: identical rows are at exactly 0."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    out = np.empty((n, n))
    for i0 in range(0, n, 64):
        diff = x[i0:i0 + 64, None, :] - x[None, :, :]
        out[i0:i0 + 64] = np.sqrt(np.einsum("ijk,ijk->ij", diff, diff))
    return out


def silhouette_f64(x, labels, k, mistake=None, dist=None, return_ab=False):
    """sklearn.metrics.silhouette_samples in float64 numpy.  `mistake` plants one error a kernel could make:
    'cnt' (a divided by cnt, not cnt - 1), 'singleton_one' (a singleton scores 1), 'empty_id' (an id without rows counts as a cluster
    at mean distance 0), 'sorted_order' (output left in label-sorted order), 'centroid' (the nearest cluster chosen by centroid
    distance).  Returns float64 [n], with return_ab also the a and b it was formed from."""
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels)
    n = x.shape[0]
    d = distances_f64(x) if dist is None else dist
    cnt = np.bincount(labels, minlength=k)
    sums = np.zeros((n, k))
    for c in range(k):
        if cnt[c]:
            sums[:, c] = d[:, labels == c].sum(1)
    own = sums[np.arange(n), labels]
    a = own / np.maximum(cnt[labels] - (0 if mistake == "cnt" else 1), 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        means = sums / cnt[None, :]
    present = cnt > 0
    if mistake == "empty_id":
        means[:, ~present] = 0.0
        present = np.ones(k, dtype=bool)
    means[:, ~present] = np.inf
    means[np.arange(n), labels] = np.inf
    if mistake == "centroid":
        cent = np.stack([x[labels == c].mean(0) if cnt[c] else np.full(x.shape[1], np.inf) for c in range(k)])
        dc = np.linalg.norm(x[:, None, :] - cent[None, :, :], axis=2)
        dc[~np.isfinite(dc)] = np.inf
        dc[np.arange(n), labels] = np.inf
        b = means[np.arange(n), dc.argmin(1)]
    else:
        b = means.min(1)
    m = np.maximum(a, b)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(m > 0, (b - a) / m, 0.0)
    s[cnt[labels] == 1] = 1.0 if mistake == "singleton_one" else 0.0
    if mistake == "sorted_order":
        s = s[np.argsort(labels, kind="stable")]
    return (s, a, b) if return_ab else s


# ------------------------------------------------------------------------------------------------ the exact families
U24 = 2.0 ** -24
# planted mistakes of kernel_sums / lattice_reference / grid_model (tests/test_silhouette_host.py, (i) ... (vii))
MISTAKES = ("border_both", "border_neither", "drop_partial_subtile", "unmasked_tail", "pad_slots_in_last", "scan_restart",
            "skip_second_kstep")


def _cdiv(a, b):
    return -(-a // b)


def ranges(n, k, n_cu):
    """grid.y of sl_main_kernel as silhouette.hip's sl_ranges computes it.  Restated here for BUILDING cases without a device only; the GPU
    tests ask scd_silhouette_ranges, and nothing asserts this against itself."""
    return max(1, min(k, 32, _cdiv(4 * n_cu, _cdiv(n, 128))))


def smallest_n(want, ranges_fn):
    """The smallest n >= 32 for which ranges_fn(n, 32) == want; ranges_fn(n, k) does not increase with n."""
    lo, hi = 32, 1 << 24
    assert ranges_fn(hi, 32) <= want
    while lo < hi:
        mid = (lo + hi) // 2
        if ranges_fn(mid, 32) <= want:
            hi = mid
        else:
            lo = mid + 1
    assert ranges_fn(lo, 32) == want, (want, lo, ranges_fn(lo, 32))
    return lo


def lattice_u(d):
    """(u int64 [d], g): magnitudes 1, 2, 3 (the larger ones last), signs alternating, sum u^2 = g^2 the smallest square reachable:
    d = 32 -> 28 ones, 3 twos and a three (g = 7), d = 64 -> ones (g = 8), d = 1000 -> 992 ones and 8 twos (g = 32)."""
    g = int(np.ceil(np.sqrt(d)))
    while True:
        rest = g * g - d                                            # a two adds 3 to the squared sum, a three 8
        for threes in range(min(d, rest // 8) + 1):
            twos, rem = divmod(rest - 8 * threes, 3)
            if rem == 0 and twos + threes <= d:
                u = np.array([1] * (d - twos - threes) + [2] * twos + [3] * threes, dtype=np.int64)
                u[1::2] *= -1
                return u, g
        g += 1


def _sizes_to_labels(sizes, n_bad, rs):
    """Labels with sizes[c] rows of id c and n_bad rows labelled -1 / k in turn, in random row order."""
    k = len(sizes)
    lab = np.concatenate([np.repeat(np.arange(k), sizes), np.where(np.arange(n_bad) % 2 == 0, -1, k)]).astype(np.int64)
    return lab[rs.permutation(lab.size)]


def _random_sizes(n, k, n_empty, n_single, rs):
    """k sizes that add up to n: n_empty zeros, n_single ones, the others >= 2 with gamma-distributed weights, ids shuffled."""
    m = k - n_empty - n_single
    rest = n - n_single - 2 * m
    assert m > 0 and rest >= 0
    w = rs.gamma(1.0, size=m)
    big = 2 + rs.multinomial(rest, w / w.sum())
    sizes = np.concatenate([np.zeros(n_empty, dtype=np.int64), np.ones(n_single, dtype=np.int64), big])
    return sizes[rs.permutation(k)]


D_SWEEP = (1, 31, 32, 33, 64, 65, 96, 1000, 1024)
N_VALID = (127, 128, 129, 400)
LATTICE_NAMES = (["scan_piece2", "scan_piece3", "two_ranges_99_1", "two_ranges_tiny_first", "two_ranges_border_m1", "two_ranges_border_0",
                  "two_ranges_border_p1", "two_ranges_bad_rows", "one_range_k2", "one_range_k1000", "ranges32"]
                 + ["valid_%d" % v for v in N_VALID] + ["d_%d" % d for d in D_SWEEP] + ["d_65_fp32"])


def _lattice_spec(name, ranges_fn):
    """-> (sizes, n_bad, d, tmax (t < tmax), ny the case is for or None, seed)"""
    seed = 1000 + LATTICE_NAMES.index(name)
    rs = np.random.RandomState(seed)
    if name == "scan_piece2":                                       # 3 chunks x 400 ids = 1,200 entries: threads 600 ... 1023 hold empty pieces
        return _random_sizes(2100, 400, 40, 30, rs), 0, 64, 16, None, seed
    if name == "scan_piece3":                                       # 4 chunks x 700 ids = 2,800 entries: pieces of 3, the last one of 1
        return _random_sizes(3100, 700, 60, 50, rs), 0, 64, 16, None, seed
    if name.startswith("two_ranges"):
        n = smallest_n(2, ranges_fn) + 37
        if name == "two_ranges_99_1":
            sizes = [n - n // 100, n // 100]
        elif name == "two_ranges_tiny_first":                       # both clusters start in range 0; range 1 holds nothing
            sizes = [5, n - 5]
        elif name == "two_ranges_bad_rows":                         # n_valid != n moves the border
            sizes = [(n - 300) - (n - 300) // 100, (n - 300) // 100]
        else:                                                       # cluster 1 starts one before, on and one after the border
            off1 = _cdiv(n, 2) + {"m1": -1, "0": 0, "p1": 1}[name.rsplit("_", 1)[1]]
            third = (n - off1) // 3
            sizes = [off1, third, n - off1 - third]
        return np.array(sizes), n - int(np.sum(sizes)), 64, 8, 2, seed
    if name == "one_range_k2":
        n = smallest_n(1, ranges_fn) + 37
        return np.array([n // 2, n - n // 2]), 0, 32, 8, 1, seed
    if name == "one_range_k1000":
        n = smallest_n(1, ranges_fn) + 37
        return _random_sizes(n, 1000, 25, 40, rs), 0, 32, 8, 1, seed
    if name == "ranges32":                                          # most ranges start no multi-row cluster; every singleton scores 0
        sizes = np.ones(257, dtype=np.int64)
        sizes[100] = 259
        return sizes, 0, 64, 16, 32, seed
    if name.startswith("valid_"):                                   # whole panels past the last valid row
        v = int(name[6:])
        first = v // 3
        return np.array([first, 0, v // 4, 1, v - first - v // 4 - 1]), 1000 - v, 64, 16, None, seed
    d = int(name.split("_")[1])
    return _random_sizes(300, 5, 0, 0, rs), 0, d, 16, None, seed


def lattice_case(name, ranges_fn):
    """One case of the lattice family as a dict: x [n, d] (fp16; fp32 for *_fp32), labels int64 [n] (-1 and k mark rows to be dropped),
    k, t int64 [n], u, g, d, ny (the range count the case is built for, or None).  Sizes that depend on the device come from
    ranges_fn(n, k) -> grid.y.  Asserts the conditions under which the device arithmetic is exact (module docstring)."""
    sizes, n_bad, d, tmax, ny, seed = _lattice_spec(name, ranges_fn)
    rs = np.random.RandomState(seed + 500)
    labels = _sizes_to_labels(sizes, n_bad, rs)
    n, k = labels.size, len(sizes)
    t = rs.randint(0, tmax, size=n).astype(np.int64)
    u, g = lattice_u(d)
    x = (t[:, None] * u[None, :]).astype(np.float32 if name.endswith("fp32") else np.float16)
    case = dict(name=name, x=np.ascontiguousarray(x), labels=labels, k=k, t=t, u=u, g=g, d=d, n=n, ny=ny)
    # exactness
    assert int((u * u).sum()) == g * g and (d == 1 or (u.min() < 0 < u.max()))
    assert int(t.max()) * int(np.abs(u).max()) <= 2048 and np.array_equal(x.astype(np.int64), t[:, None] * u[None, :])
    assert 2 * g * g * int(t.max()) ** 2 < 2 ** 24                  # norms, their sum and 2 dot; MFMA partial sums are <= g^2 t_i t_j
    tt = np.arange(int(t.max()) + 1)
    d2 = (g * g * (tt[:, None] ** 2 + tt[None, :] ** 2) - 2 * g * g * tt[:, None] * tt[None, :]).astype(np.float32)
    assert np.array_equal(np.sqrt(d2), (g * np.abs(tt[:, None] - tt[None, :])).astype(np.float32))
    valid = (labels >= 0) & (labels < k)
    table = np.zeros((k, tt.size), dtype=np.int64)
    np.add.at(table, (labels[valid], t[valid]), 1)
    sums = g * np.abs(tt[:, None] - tt[None, :]) @ table.T          # [t, k]: a row's sum over a cluster, exact in int64
    assert int(sums.max()) < 2 ** 24                                # every partial sum of non-negative integers, in any order
    return case


def sorted_slots(labels, k):
    """The stable counting sort: (the original row of every sorted slot [n_valid], off int64 [k + 1])."""
    idx = np.nonzero((labels >= 0) & (labels < k))[0]
    order = idx[np.argsort(labels[idx], kind="stable")]
    off = np.concatenate([[0], np.cumsum(np.bincount(labels[idx], minlength=k))]).astype(np.int64)
    return order, off


def scan_offsets(labels, k, restart=False):
    """off [k + 1] as sl_rank_kernel / sl_scan_kernel / sl_offsets_kernel form it: the exclusive scan of the [k][chunks] counts in pieces
    of ceil(k chunks / 1024) entries.  restart = mistake (vi): every thread's piece starts from 0 again."""
    n = labels.size
    chunks = _cdiv(n, 1024)
    idx = np.nonzero((labels >= 0) & (labels < k))[0]
    hist = np.zeros((k, chunks), dtype=np.int64)
    np.add.at(hist, (labels[idx], idx // 1024), 1)
    flat = hist.ravel()
    excl = np.cumsum(flat) - flat
    if restart:
        piece = _cdiv(flat.size, 1024)
        excl = excl - excl[np.arange(flat.size) // piece * piece]
    return np.concatenate([excl[::chunks], [flat.sum()]]).astype(np.int64)


def kernel_sums(slot_cls, dist, off, n_valid, ny, mistake=None):
    """Which slots sl_main_kernel adds for which cluster, on count tables.  slot_cls [n_alloc]: the class of every sorted slot (slots
    past n_valid hold zero rows); dist [classes, classes]: the distance between two classes; off [k + 1]; ny: grid.y.  Returns
    (S [classes, k]: the sum a row of a class gets against cluster c, seen bool [k]: some range walks cluster c).  A cluster
    belongs to the range its first slot falls in, ranges being ceil(n_valid / ny) slots wide; that every non-empty cluster is
    walked once is taken as given, and the mistakes break it:
      border_both / border_neither (i, ii): a cluster whose first slot is a range's first slot is added by both neighbours / by none;
      drop_partial_subtile (iii): the last partial 16-column sub-tile of a cluster is not added;
      unmasked_tail (iv): the columns of that sub-tile past the segment's end are added too;
      pad_slots_in_last (v): the zero slots up to the end of the last panel count as columns of the last non-empty cluster.
    (vi) and (vii) change `off` and `dist`, so they are planted by the callers."""
    k = off.size - 1
    ncls = dist.shape[0]
    per = _cdiv(int(n_valid), ny)
    borders = set(y * per for y in range(1, ny) if y * per < n_valid)
    cnt = np.diff(off)
    last = int(np.nonzero(cnt > 0)[0].max())
    cols = np.zeros((k, ncls), dtype=np.int64)
    seen = cnt > 0
    for c in np.nonzero(cnt > 0)[0]:
        lo, hi, times = int(off[c]), int(off[c + 1]), 1
        if mistake == "drop_partial_subtile":
            hi = lo + (hi - lo) // 16 * 16
        elif mistake == "unmasked_tail":
            hi = lo + _cdiv(hi - lo, 16) * 16
        elif mistake == "pad_slots_in_last" and c == last:
            hi = max(hi, _cdiv(int(n_valid), 128) * 128)
        elif mistake == "border_both" and lo in borders:
            times = 2
        elif mistake == "border_neither" and lo in borders:
            times, seen[c] = 0, False
        cols[c] = times * np.bincount(slot_cls[lo:hi], minlength=ncls)
    return dist @ cols.T, seen


def finish(S, seen, cnt, rows, row_cls, row_lab, n, dtype):
    """sl_finish_kernel in numpy `dtype`: a = own sum / (cnt - 1), b = the smallest sum_c / cnt_c over the other walked clusters,
    s = (b - a) / max(a, b), 0 for cnt <= 1, for max = 0, for the rows outside `rows` and with fewer than two non-empty clusters."""
    f = np.dtype(dtype).type
    out = np.zeros(n, dtype=dtype)
    if (cnt > 0).sum() < 2:
        return out
    with np.errstate(all="ignore"):
        means = np.where((seen & (cnt > 0))[None, :], S.astype(dtype) / np.maximum(cnt, 1).astype(dtype)[None, :], f(np.inf))
        two = np.argsort(means, axis=1, kind="stable")[:, :2]
        r = np.arange(means.shape[0])
        first, m1, m2 = two[:, 0], means[r, two[:, 0]], means[r, two[:, 1]]
        own = np.where(seen[row_lab], S[row_cls, row_lab], 0).astype(dtype)
        c1 = cnt[row_lab]
        a = own / np.maximum(c1 - 1, 1).astype(dtype)
        b = np.where(first[row_cls] == row_lab, m2[row_cls], m1[row_cls])
        m = np.maximum(a, b)
        s = np.where(m > 0, (b - a) / m, f(0))
        s[c1 <= 1] = 0
    assert s.dtype == np.dtype(dtype)
    out[rows] = s
    return out


def _kstep_mask(d):
    """Columns whose products survive mistake (vii): the second 32-wide k-step of every 64-chunk is skipped when dp is a multiple of 64."""
    dp = _cdiv(d, 32) * 32
    return np.ones(d, dtype=bool) if dp % 64 else (np.arange(d) % 64) < 32


def lattice_reference(case, ny=1, mistake=None, dtype=np.float32):
    """(samples float32 [n], mean float64) of a lattice case: exact integer sums from the cluster x t count table, finished in numpy
    float32 as sl_main_kernel / sl_finish_kernel finish them (dtype = np.float64: the same finish in float64).  O(n + k max(t)^2).
    Without a mistake the result does not depend on ny."""
    labels, k, t, g, u, n = case["labels"], case["k"], case["t"], case["g"], case["u"], case["n"]
    order, off = sorted_slots(labels, k)
    assert np.array_equal(off, scan_offsets(labels, k))
    n_valid = int(off[-1])
    if mistake == "scan_restart":
        off = scan_offsets(labels, k, restart=True)
    slot_cls = np.zeros(_cdiv(n, 128) * 128 + 128, dtype=np.int64)  # n_alloc slots; a zero row is the lattice's t = 0
    slot_cls[:n_valid] = t[order]
    tt = np.arange(int(t.max()) + 1)
    dist = g * np.abs(tt[:, None] - tt[None, :])
    if mistake == "skip_second_kstep":
        g2 = int((u[_kstep_mask(u.size)] ** 2).sum())
        dist = np.sqrt(np.maximum(0, g * g * (tt[:, None] ** 2 + tt[None, :] ** 2) - 2 * g2 * tt[:, None] * tt[None, :]).astype(np.float64))
        dist[tt, tt] = 0.0                                          # the pair i = j is excluded by index
    S, seen = kernel_sums(slot_cls, dist, off, n_valid, ny, mistake)
    s = finish(S, seen, np.diff(off), order, t[order], labels[order], n, dtype)
    return s, float(s.astype(np.float64).mean())


GRID_SHAPES = {"grid_big_of_3": (1500, 40, 3), "grid_37": (2000, 96, 37), "grid_130": (1200, 768, 130), "grid_32_tiles": (4500, 64, 2)}


def grid_case(name):
    """One case of the general grid family: x fp16 [n, d] = (a centre in [-2, 2]^d per cluster + noise in [-2, 2]^d) / 8, labels, k."""
    n, d, k = GRID_SHAPES[name]
    seed = 2000 + sorted(GRID_SHAPES).index(name)
    rs = np.random.RandomState(seed)
    if name == "grid_big_of_3":
        sizes = np.array([150, 1100, 250])
    elif name == "grid_32_tiles":
        sizes = np.array([4000, 500])
    elif name == "grid_37":                                         # cluster 1 starts at slot 63 = ceil(2000 / 32): a range border at ny = 32
        sizes = np.concatenate([[63], _random_sizes(n - 63, k - 1, 0, 2, rs)])
    else:
        sizes = _random_sizes(n, k, 3, 9, rs)
    labels = _sizes_to_labels(sizes, 0, rs)
    x = (rs.randint(-2, 3, size=(k, d))[labels] + rs.randint(-2, 3, size=(n, d))) / 8.0
    x16 = np.ascontiguousarray(x.astype(np.float16))
    assert np.array_equal(x16.astype(np.float64), x) and np.abs(x).max() <= 0.5 and d * 0.25 * 64 < 2 ** 24
    return dict(name=name, x=x16, labels=labels, k=k, n=n, d=d)


def grid_distances(x, mask=None):
    """Float64 distances in the GEMM form, exact up to the square root on the grid (zero diagonal).  mask: the columns the dots use."""
    x = np.asarray(x, dtype=np.float64)
    nrm = (x * x).sum(1)
    xm = x if mask is None else x[:, mask]
    dist = np.sqrt(np.maximum(0.0, nrm[:, None] + nrm[None, :] - 2.0 * (xm @ xm.T)))
    np.fill_diagonal(dist, 0.0)
    return dist


def grid_bound(labels, k):
    """Per-row bound on |s_device - s_float64| of a general grid case (module docstring): (eps_own + max_c eps_c + 2 u)(1 + 1e-3) with
    eps_c = (8 ceil(cnt_c / 128) + 6) u."""
    cnt = np.bincount(labels, minlength=k)
    eps = (8 * _cdiv(cnt, 128) + 6) * U24
    return (eps[labels] + eps[cnt > 0].max() + 2 * U24) * (1 + 1e-3)


def grid_model(case, ny, mistake=None, dist=None):
    """Float64 samples of a general grid case through kernel_sums (every sorted slot a class of its own, one more for the zero rows past
    the last valid one).  `dist`: grid_distances of the sorted rows plus that zero row, if the caller has it."""
    x, labels, k, n = case["x"], case["labels"], case["k"], case["n"]
    order, off = sorted_slots(labels, k)
    if mistake == "scan_restart":
        off = scan_offsets(labels, k, restart=True)
    if dist is None or mistake == "skip_second_kstep":
        xs = np.concatenate([x[order].astype(np.float64), np.zeros((1, x.shape[1]))])
        dist = grid_distances(xs, _kstep_mask(x.shape[1]) if mistake == "skip_second_kstep" else None)
    slot_cls = np.full(_cdiv(n, 128) * 128 + 128, n, dtype=np.int64)
    slot_cls[:n] = np.arange(n)
    S, seen = kernel_sums(slot_cls, dist, off, n, ny, mistake)
    return finish(S, seen, np.diff(off), order, np.arange(n), labels[order], n, np.float64)
