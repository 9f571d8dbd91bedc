"""The silhouette cases of tests/golden/silhouette.npz (tools/gen_silhouette_golden.py), regenerated from seeds, a float64 numpy
restatement of sklearn.metrics.silhouette_samples with optional planted mistakes, and the per-case error bounds of the GPU test.

Rows are oracle/synth.clustered_features output cast to fp16, so rounding them to fp16 again is the identity.  The golden file holds
only what cannot be regenerated without scikit-learn: the expected float64 samples, the scikit-learn KMeans partitions of the blobs
and their silhouette table."""
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
