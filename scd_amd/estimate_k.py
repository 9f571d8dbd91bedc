"""GCD's estimator of the number of categories (the reference's gcd/methods/estimate_k/estimate_k.py) on the HIP k-means and
the on-device scores: fit `KMeans(n_clusters=K, random_state=0)` on all L2-normalised features, labelled and unlabelled, for a
sequence of K, and keep the K whose clustering accuracy on the LABELLED rows is highest.

  * `evaluate_k`    restates `test_kmeans` / `test_kmeans_for_scipy` (estimate_k.py:41-105, :109-169);
  * `binary_search` restates estimate_k.py:172-218 decision for decision;
  * `brent`         restates `scipy_optimise`, estimate_k.py:221-242 (scipy's bounded Brent on -ACC).

Without labelled rows (main_unsup.py's setting) there is nothing to take an accuracy on:

  * `evaluate_k_unlabelled` scores a fit by its mean silhouette coefficient (metrics.silhouette_score: scd_silhouette on the device);
  * `grid_search`           is an integer search for it - bounded Brent on an integer-truncated K is fragile for this criterion
                            (docs/design/estimate_k.md, "Without labels").

  * `evaluate_cut`          scores the cut at K of a Ward tree fitted once (scd_amd.ward; docs/design/ward.md): no fit per K;
  * `finch_search`          scores only the cluster counts FINCH's partitions propose (scd_amd.finch; docs/design/finch.md): a
                            handful of fits instead of a sweep.

All searches memoise their evaluations by int(K).  The fit is deterministic for a fixed K (random_state=0, deterministic kernels), so
an evaluation repeated at the same K would return the same accuracy: memoising changes no decision of either search, it only saves
the repeated fits (bounded Brent on an integer-truncated K revisits the same int(K) several times near its end).
"""
import numpy as np

from . import metrics
from .cluster import KMeans


def evaluate_k(K, feats, targets, mask_lab, verbose=False, **kmeans_kw):
    """estimate_k.py:41-105 for one K.  feats: device float32 [n, d], L2-normalised once by the caller (ops.l2norm_rows; :61) and reused
    for every K; targets, mask_lab: device tensors or numpy.  Returns (labelled ACC, {'labelled': {acc, nmi, ari, purity},
    'unlabelled': {...}}): the labels never leave the device, metrics.score_split scores them there."""
    K = int(K)
    kw = dict(random_state=0)
    kw.update(kmeans_kw)
    km = KMeans(n_clusters=K, **kw).fit(feats)
    scores = metrics.score_split(km.labels_device_, targets, mask_lab)
    if scores["labelled"] is None:
        raise ValueError("mask_lab selects no row: the estimator scores K on the labelled rows")
    if verbose:                                     # the reference's per-K lines (:163-167)
        print(f'K = {K}')
        for name, key in (('Labelled', 'labelled'), ('Unlabelled', 'unlabelled')):
            s = scores[key]
            if s is not None:
                print('{} Instances acc {:.4f}, nmi {:.4f}, ari {:.4f}'.format(name, s['acc'], s['nmi'], s['ari']))
    return scores["labelled"]["acc"], scores


def evaluate_k_unlabelled(K, feats, verbose=False, **kmeans_kw):
    """One K of the label-free search: fit `KMeans(n_clusters=K, random_state=0)` on feats (device float32 / float16 [n, d]) and score
    `labels_device_` by the mean silhouette coefficient on the device.  Returns (silhouette, {'silhouette': s}); neither the labels nor
    the features leave the device."""
    K = int(K)
    kw = dict(random_state=0)
    kw.update(kmeans_kw)
    km = KMeans(n_clusters=K, **kw).fit(feats)
    s = metrics.silhouette_score(feats, km.labels_device_)
    if verbose:
        print('K = {}: silhouette {:.4f}'.format(K, s))
    return s, {'silhouette': s}


def evaluate_k_bic(K, feats, covariance_type="diag", verbose=False, **gmm_kw):
    """One K of the mixture search: fit `GaussianMixture(n_components=K, covariance_type, random_state=0)` (scd_amd.gmm; scd_amd.gmm_full's
    FullGaussianMixture for 'full' and 'tied') on feats (device
    float32 [n, d]) and take its BIC on the same rows: one n x K x d pass per EM step, no n x n pass.  The searches maximise, so the
    value returned is -BIC: (-bic, {'bic', 'lower_bound', 'n_iter', 'converged'})."""
    if covariance_type in ("full", "tied"):                     # docs/design/gmm_full.md: rows of at most 64 dimensions
        from .gmm_full import FullGaussianMixture as GaussianMixture
    else:
        from .gmm import GaussianMixture
    K = int(K)
    kw = dict(random_state=0)
    kw.update(gmm_kw)
    gm = GaussianMixture(n_components=K, covariance_type=covariance_type, **kw).fit(feats)
    bic = float(gm.bic(feats))
    if verbose:
        print('K = {}: BIC {:.1f}, lower bound {:.6f} ({} iterations)'.format(K, bic, gm.lower_bound_, gm.n_iter_))
    return -bic, {'bic': bic, 'lower_bound': float(gm.lower_bound_), 'n_iter': int(gm.n_iter_), 'converged': bool(gm.converged_)}


def evaluate_cut(K, feats, Z, targets=None, mask_lab=None, verbose=False):
    """One K of the search on a Ward tree fitted once (scd_amd.ward.ward_tree's Z on all rows of feats): the labels are the tree's cut at
    K, no fit.  With targets and mask_lab the score is evaluate_k's (labelled ACC, the score dict); without them evaluate_k_unlabelled's
    (silhouette, {'silhouette': s})."""
    import torch
    from .ward import cut_tree
    K = int(K)
    labels = torch.as_tensor(cut_tree(Z, K).astype(np.int32), device=feats.device)
    if targets is None:
        s = metrics.silhouette_score(feats, labels)
        if verbose:
            print('K = {}: silhouette {:.4f}'.format(K, s))
        return s, {'silhouette': s}
    scores = metrics.score_split(labels, targets, mask_lab)
    if scores["labelled"] is None:
        raise ValueError("mask_lab selects no row: the estimator scores K on the labelled rows")
    if verbose:
        print('K = {}: labelled acc {:.4f}'.format(K, scores["labelled"]["acc"]))
    return scores["labelled"]["acc"], scores


class _Memo:
    """evaluate(int K) -> float, each distinct K evaluated once."""

    def __init__(self, evaluate):
        self.evaluate = evaluate
        self.seen = {}

    def __call__(self, K):
        K = int(K)
        if K not in self.seen:
            self.seen[K] = float(self.evaluate(K))
        return self.seen[K]


def binary_search(evaluate, small_k, big_k, log=None):
    """estimate_k.py:172-218.  evaluate(K) -> labelled ACC.  The reference's decisions are kept as they are, quirks included: the
    number of iterations is int(log2(big_k - small_k)) of the FIRST interval, the interval moves up whenever ACC(big) > ACC(small),
    and "best so far" looks only at the current (small, middle, big) triple - an earlier, better K that left the triple is forgotten.
    Returns (best_acc_at_k of the last iteration, trace) with trace[i] = (small_k, middle_k, big_k, (acc_small, acc_middle, acc_big));
    `log` (print, for the driver) receives the reference's two lines per iteration."""
    small_k, big_k = int(small_k), int(big_k)
    if big_k <= small_k:
        raise ValueError("binary_search needs small_k < big_k (got %d, %d)" % (small_k, big_k))
    ev = _Memo(evaluate)
    log = log or (lambda s: None)
    trace = []

    # Iter 0
    diff = big_k - small_k
    middle_k = int(0.5 * diff + small_k)
    acc_big = ev(big_k)
    acc_small = ev(small_k)
    acc_middle = ev(middle_k)

    def note(i):
        log(f'Iter {i}: BigK {big_k}, Acc {acc_big:.4f} | MiddleK {middle_k}, Acc {acc_middle:.4f} | SmallK {small_k}, Acc {acc_small:.4f} ')
        all_accs = [acc_small, acc_middle, acc_big]
        best = int(np.array([small_k, middle_k, big_k])[np.argmax(all_accs)])
        log(f'Best Acc so far {np.max(all_accs):.4f} at K {best}')
        trace.append((small_k, middle_k, big_k, (acc_small, acc_middle, acc_big)))
        return best

    best_acc_at_k = note(0)
    for i in range(1, int(np.log2(diff)) + 1):
        if acc_big > acc_small:
            small_k = middle_k
            acc_small = acc_middle
            diff = big_k - small_k
            middle_k = int(0.5 * diff + small_k)
        else:
            big_k = middle_k
            diff = big_k - small_k
            middle_k = int(0.5 * diff + small_k)
            acc_big = acc_middle
        acc_middle = ev(middle_k)
        best_acc_at_k = note(i)
    return best_acc_at_k, trace


def brent(evaluate, small_k, big_k):
    """estimate_k.py:221-242: scipy's bounded Brent on K -> -ACC(int(K)).  Returns (res.x, int(res.x), trace) with
    trace[i] = (K as scipy asked for it, int(K), ACC)."""
    from scipy.optimize import minimize_scalar          # lazily: only this search needs scipy
    ev = _Memo(evaluate)
    trace = []

    def neg_acc(K):
        acc = ev(int(K))
        trace.append((float(K), int(K), acc))
        return -acc

    res = minimize_scalar(neg_acc, bounds=(small_k, big_k), method='bounded')
    return float(res.x), int(res.x), trace


def grid_search(evaluate, small_k, big_k, points=9, log=None):
    """Integer search for the K in [small_k, big_k] that maximises evaluate(K).  Each round lays `m = min(points, hi - lo + 1)` integers
    evenly over [lo, hi] (ends included, rounded to nearest), evaluates them all (memoised) and takes the FIRST maximum, so the lowest K
    wins a tie.  If the round's K are consecutive integers that K is the answer; otherwise the interval shrinks to the grid neighbours
    below and above the best (clamped at the ends) and the search repeats.  (With three points and the best in the middle those
    neighbours are the interval's own ends; the interval then shrinks to the midpoints between the best and its neighbours.)
    Deterministic.  Returns (best_k, trace) with trace[r] = (ks, scores, best)."""
    small_k, big_k, points = int(small_k), int(big_k), int(points)
    if big_k <= small_k:
        raise ValueError("grid_search needs small_k < big_k (got %d, %d)" % (small_k, big_k))
    if points < 3:
        raise ValueError("grid_search needs points >= 3 (got %d)" % points)
    ev = _Memo(evaluate)
    log = log or (lambda s: None)
    trace = []
    lo, hi = small_k, big_k
    while True:
        m = min(points, hi - lo + 1)
        ks = sorted({lo + ((hi - lo) * i + (m - 1) // 2) // (m - 1) for i in range(m)})
        scores = [ev(K) for K in ks]
        b = max(range(len(ks)), key=lambda i: (scores[i], -i))
        best = ks[b]
        trace.append((ks, scores, best))
        log('Round %d: K %s -> best %d (%.4f)' % (len(trace) - 1, ks, best, scores[b]))
        if ks[-1] - ks[0] == len(ks) - 1:
            return best, trace
        below, above = ks[max(b - 1, 0)], ks[min(b + 1, len(ks) - 1)]
        if (below, above) == (lo, hi):
            below, above = (below + best + 1) // 2, (best + above) // 2
        lo, hi = below, above


def finch_search(evaluate, candidates, small_k, big_k, log=None):
    """The K among FINCH's cluster counts that maximises evaluate(K).  `candidates` (FINCH's num_clust) are clipped to
    [small_k, big_k]; the distinct values are evaluated in increasing order (memoised) and the FIRST maximum wins, so the lowest K wins
    a tie - grid_search's rule.  Returns (best_k, trace) with trace[0] = (ks, scores, best).  No candidate: ValueError."""
    small_k, big_k = int(small_k), int(big_k)
    if big_k < small_k:
        raise ValueError("finch_search needs small_k <= big_k (got %d, %d)" % (small_k, big_k))
    ks = sorted({min(max(int(k), small_k), big_k) for k in candidates})
    if not ks:
        raise ValueError("finch_search: FINCH proposed no cluster count")
    ev = _Memo(evaluate)
    log = log or (lambda s: None)
    scores = [ev(K) for K in ks]
    b = max(range(len(ks)), key=lambda i: (scores[i], -i))
    log('FINCH candidates: K %s -> best %d (%.4f)' % (ks, ks[b], scores[b]))
    return ks[b], [(ks, scores, ks[b])]
