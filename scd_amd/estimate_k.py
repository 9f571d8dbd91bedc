"""GCD's estimator of the number of categories (the reference's gcd/methods/estimate_k/estimate_k.py) on the HIP k-means and
the on-device scores: fit `KMeans(n_clusters=K, random_state=0)` on all L2-normalised features, labelled and unlabelled, for a
sequence of K, and keep the K whose clustering accuracy on the LABELLED rows is highest.

  * `evaluate_k`    restates `test_kmeans` / `test_kmeans_for_scipy` (estimate_k.py:41-105, :109-169);
  * `binary_search` restates estimate_k.py:172-218 decision for decision;
  * `brent`         restates `scipy_optimise`, estimate_k.py:221-242 (scipy's bounded Brent on -ACC).

Both searches memoise their evaluations by int(K).  The fit is deterministic for a fixed K (random_state=0, deterministic kernels), so
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
