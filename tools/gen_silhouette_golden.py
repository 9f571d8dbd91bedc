"""Writes tests/golden/silhouette.npz with scikit-learn 1.7.2 on the CPU (the test suite itself never imports scikit-learn).

  s_<case>      float64 [n]      sklearn.metrics.silhouette_samples of the fp16-rounded rows of every case of tests/silhouette_cases.py,
                                 on float64 distances taken from coordinate differences (metric='precomputed'), so that identical rows
                                 are at exactly 0 and the expected values carry no cancellation noise of their own
  blobs_ks      int32 [16]       the K estimate_k.grid_search visits on [2, 64] on the blobs (silhouette_cases.GRID_KS)
  blobs_part    int8 [16, 3000]  labels of sklearn.cluster.KMeans(n_clusters=K, random_state=0, n_init=10) on the blobs (float32 rows)
  blobs_sil     float64 [16]     the mean silhouette of those partitions (fp16-rounded rows)

  python tools/gen_silhouette_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import silhouette_cases as sc                                   # noqa: E402


def main():
    from sklearn.cluster import KMeans
    from sklearn.metrics import silhouette_samples
    out = {}
    xb, yb, _ = sc.blobs(3000)
    db = sc.distances_f64(xb.astype(np.float16))
    parts, sils = [], []
    for K in sc.GRID_KS:
        lab = KMeans(n_clusters=K, random_state=0, n_init=10).fit(xb).labels_
        parts.append(lab.astype(np.int8))
        sils.append(float(silhouette_samples(db, lab, metric="precomputed").mean()))
        print("blobs K = %2d: silhouette %.4f" % (K, sils[-1]))
    out["blobs_ks"] = np.asarray(sc.GRID_KS, dtype=np.int32)
    out["blobs_part"] = np.stack(parts)
    out["blobs_sil"] = np.asarray(sils)
    for name, (x, labels, k) in sc.cases(out).items():
        d = db if name.startswith("blobs") else sc.distances_f64(x)
        out["s_" + name] = silhouette_samples(d, labels, metric="precomputed")
        sizes = np.bincount(labels, minlength=k)
        print("%-13s n %4d d %3d k %3d sizes %d..%d (%d empty): mean %.6f" % (name, x.shape[0], x.shape[1], k, sizes[sizes > 0].min(),
                                                                            sizes.max(), int((sizes == 0).sum()), out["s_" + name].mean()))
    path = os.path.join(ROOT, "tests", "golden", "silhouette.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
