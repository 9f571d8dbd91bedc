"""Writes tests/golden/tsne_blobs.npz, the end-to-end case of tests/test_gpu_tsne.py: 1,500 unit blob rows (D = 32, ten classes), their
labels, and what scikit-learn's TSNE(perplexity=20, method='barnes_hut') reaches on them for random_state 0 .. 4: kl_divergence_ and
sklearn.manifold.trustworthiness.  At perplexity 20 scikit-learn takes 60 neighbours, so its P is the one scd_amd.tsne builds.  CPU only.

  python tools/gen_tsne_golden.py            write the fixture
  python tools/gen_tsne_golden.py --tail     the conditional mass beyond the 64th / 91st neighbour at perplexity 30 on the same rows
                                             (tests/tsne_cases.py: TAIL_BEYOND_64, TAIL_BEYOND_91)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import finch_cases as fc                                        # noqa: E402
import tsne_cases as tc                                         # noqa: E402

N, D, CLASSES, SEED, PERPLEXITY = 1500, 32, 10, 90, 20.0


def rows():
    x, y = tc.blob_rows(N, D, CLASSES, SEED)
    return fc.unit_rows(x), y


def tail():
    u, _ = rows()
    g = u.astype(np.float64) @ u.astype(np.float64).T
    np.fill_diagonal(g, -np.inf)
    d = np.sort(np.maximum(0.0, 2.0 - 2.0 * g), axis=1)[:, :N - 1]               # every other row, nearest first
    p, _, unreached = tc.calibrate_f64(d, 30.0)
    assert not unreached.any()
    for kk in (64, 91):
        beyond = p[:, kk:].sum(1)
        print("perplexity 30, dense float64 calibration: mass beyond neighbour %d: mean %.4f max %.4f" % (kk, beyond.mean(), beyond.max()))


def main():
    from sklearn.manifold import TSNE, trustworthiness
    u, y = rows()
    kl, trust = [], []
    for seed in range(5):
        t0 = time.time()
        ts = TSNE(n_components=2, perplexity=PERPLEXITY, method='barnes_hut', random_state=seed)
        emb = ts.fit_transform(u)
        kl.append(float(ts.kl_divergence_))
        trust.append(float(trustworthiness(u, emb, n_neighbors=5)))
        print("seed %d: KL %.4f trustworthiness %.4f, %d iterations, %.1f s" % (seed, kl[-1], trust[-1], ts.n_iter_, time.time() - t0))
    out = os.path.join(ROOT, "tests", "golden", "tsne_blobs.npz")
    np.savez_compressed(out, rows=u, labels=y.astype(np.int64), sklearn_kl=np.array(kl), sklearn_trust=np.array(trust),
                        perplexity=np.array(PERPLEXITY))
    print("written", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    tail() if "--tail" in sys.argv else main()
