#!/usr/bin/env python
"""Writes tests/golden/cluster_scores.npz: label pairs with the scores the reference computes for them, and the reference's two
searches for the number of categories on a fixed accuracy curve.  `python tools/gen_cluster_scores_golden.py --reference DIR`
(DIR: a checkout of the reference; needs scikit-learn 1.7.2 and scipy; runs on the CPU).

Used at generation time only, nothing of it is stored: the reference's `cluster_acc`, `linear_assignment` and `purity_score`
(gcd/project_utils/cluster_utils.py), scikit-learn's `normalized_mutual_info_score`, `adjusted_rand_score`, `mutual_info_score` and
`entropy`, the reference's `binary_search` (gcd/methods/estimate_k/estimate_k.py:172-218, run from its source with `test_kmeans`
replaced by a lookup into the curve - the device its own DUMMY_ACCS is) and scipy's bounded `minimize_scalar`.

Keys (numeric arrays only; tests/cluster_score_cases.py unpacks them): rows int32 [C] and dims int32 [C] (rows and table side D of
each of the C cases), pred, truth int16 and mask bool (the cases' rows back to back), tables int32 (the D x D w of cluster_acc of
every case, flattened, back to back), scores float64 [C, 4] (ACC, NMI, ARI, purity), ints int64 [C, 6] and info float64 [C, 3]
(what scd_contingency_stats returns for the case's table).  curve float64 [201] (ACC at K, K in [10, 200]); bs_range [2]; bs_calls (the Ks in evaluation order);
bs_trace int16 [iters, 3] (small, middle, big); bs_best int16 [iters]; brent_ks int16 (int(K) per evaluation); brent_x float64 [1]."""
import argparse
import ast
import contextlib
import io
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_K, BIG_K = 10, 200


def cases():
    r = np.random.RandomState(20)
    out = []

    def add(pred, truth, p_lab=0.4):
        pred, truth = np.asarray(pred, dtype=np.int64), np.asarray(truth, dtype=np.int64)
        out.append((pred, truth, r.rand(pred.size) < p_lab))

    add(r.randint(0, 3, 200), r.randint(0, 7, 200))                     # 3 clusters against 7 classes, independent
    add(r.randint(0, 7, 200), r.randint(0, 3, 200))                     # 7 against 3
    t = r.randint(0, 9, 500)
    add(r.permutation(9)[t], t)                                         # a perfect clustering under a permutation: all scores 1
    add(np.zeros(50), np.zeros(50))                                     # one class on both sides: NMI 1, ARI 1
    add(np.zeros(120), r.randint(0, 5, 120))                            # one cluster, several classes: MI = 0 -> NMI 0
    t = r.randint(0, 30, 1200)
    add(np.where(r.rand(1200) < 0.7, t, r.randint(0, 36, 1200)), t)     # 36 clusters, 30 classes, 70 % agreement
    add([4], [2])                                                       # one row
    add(r.choice([0, 3, 11], 300), r.choice([1, 2, 8, 9], 300))         # label ids with gaps
    add(np.arange(64), r.randint(0, 4, 64))                             # every row its own cluster: purity 1
    t = (r.rand(1000) ** 3 * 12).astype(int)
    add(np.where(r.rand(1000) < 0.5, t, (t + 1) % 12), t)               # very unequal class sizes
    return out


def curve():
    """A seeded skewed bump over K in [10, 200], strictly unimodal; zeros outside."""
    r = np.random.RandomState(3)
    peak, left, right = r.randint(50, 120), r.uniform(20, 40), r.uniform(50, 90)
    k = np.arange(BIG_K + 1, dtype=np.float64)
    acc = 0.35 + 0.6 * np.exp(-((k - peak) / np.where(k < peak, left, right)) ** 2)
    acc[:SMALL_K] = 0.0
    return acc


def reference_binary_search(ref, acc):
    """The reference's own `binary_search`, compiled from its source (importing the module would run its data set set-up)."""
    path = os.path.join(ref, "gcd", "methods", "estimate_k", "estimate_k.py")
    tree = ast.parse(open(path).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "binary_search"]
    calls = []

    def test_kmeans(K, loader, args=None, verbose=False):
        calls.append(int(K))
        return float(acc[int(K)])

    ns = {"np": np, "test_kmeans": test_kmeans}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), ns)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ns["binary_search"](None, argparse.Namespace(num_labeled_classes=SMALL_K, max_classes=BIG_K))
    trace, best = [], []
    for line in buf.getvalue().splitlines():
        m = re.match(r"Iter \d+: BigK (\d+), .* MiddleK (\d+), .* SmallK (\d+),", line)
        if m:
            trace.append((int(m.group(3)), int(m.group(2)), int(m.group(1))))
        m = re.match(r"Best Acc so far .* at K (\d+)", line)
        if m:
            best.append(int(m.group(1)))
    assert len(trace) == len(best) == int(np.log2(BIG_K - SMALL_K)) + 1
    return np.array(calls), np.array(trace), np.array(best)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (holds gcd/project_utils/cluster_utils.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cluster_scores.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.reference, "gcd"))
    import sklearn
    from scipy.optimize import minimize_scalar
    from sklearn.metrics import adjusted_rand_score, mutual_info_score, normalized_mutual_info_score
    from sklearn.metrics.cluster import entropy
    from project_utils.cluster_utils import cluster_acc, purity_score
    assert sklearn.__version__ == "1.7.2", sklearn.__version__

    blob, rows = {}, []
    cs = cases()
    for c, (pred, truth, mask) in enumerate(cs):
        acc, _, w = cluster_acc(truth, pred, return_ind=True)
        w = np.asarray(w, dtype=np.int64)
        a, b = w.sum(1), w.sum(0)
        ints = np.array([w.sum(), (w ** 2).sum(), (a ** 2).sum(), (b ** 2).sum(), w.max(1).sum(), (w > 0).sum()], dtype=np.int64)
        info = np.array([entropy(pred), entropy(truth), mutual_info_score(truth, pred)], dtype=np.float64)
        scores = np.array([acc, normalized_mutual_info_score(truth, pred), adjusted_rand_score(truth, pred), purity_score(truth, pred)],
                          dtype=np.float64)
        rows.append((pred, truth, mask, w, scores, ints, info))
    # few, packed arrays: every member of an .npz costs some hundred bytes of its own
    blob["rows"] = np.array([r[0].size for r in rows], dtype=np.int32)
    blob["dims"] = np.array([r[3].shape[0] for r in rows], dtype=np.int32)
    blob["pred"] = np.concatenate([r[0] for r in rows]).astype(np.int16)
    blob["truth"] = np.concatenate([r[1] for r in rows]).astype(np.int16)
    blob["mask"] = np.concatenate([r[2] for r in rows])
    blob["tables"] = np.concatenate([r[3].reshape(-1) for r in rows]).astype(np.int32)
    blob["scores"], blob["ints"], blob["info"] = np.stack([r[4] for r in rows]), np.stack([r[5] for r in rows]), np.stack([r[6] for r in rows])

    acc = curve()
    blob["curve"] = acc
    blob["bs_range"] = np.array([SMALL_K, BIG_K])
    calls, trace, best = reference_binary_search(args.reference, acc)
    blob["bs_calls"], blob["bs_trace"], blob["bs_best"] = calls.astype(np.int16), trace.astype(np.int16), best.astype(np.int16)
    ks = []

    def f(K):
        ks.append(int(K))
        return -acc[int(K)]

    res = minimize_scalar(f, bounds=(SMALL_K, BIG_K), method="bounded")
    blob["brent_ks"] = np.array(ks, dtype=np.int16)
    blob["brent_x"] = np.array([res.x], dtype=np.float64)
    np.savez_compressed(args.out, **blob)
    print("wrote", args.out, os.path.getsize(args.out), "bytes;", "binary search ->", blob["bs_best"][-1], "brent ->", res.x)


if __name__ == "__main__":
    main()
