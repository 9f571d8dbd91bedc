#!/usr/bin/env python
"""Times Ward clustering on the device (scd_amd/ward.py, scd_amd/csrc/ward.hip) on the synthetic blobs of tools/hdbscan_bench.py (100
true classes, D = 768, noise 0.6, 5 % unstructured Gaussian rows), taken as unit rows as the mains pass them: one JSON line per
measurement, no assertions - there is no earlier number for a feature that did not exist.  docs/design/ward.md reports the lines.

  fit         N = 50,000 and N = 126,976 at D = 768, and N = 126,976 at D = 32 (a --pca_dim-like shape: blobs drawn at 32 dimensions):
              one profiled fit (HIP events around every ops.ward_nearest call, each round once: the rounds differ, so there is no
              median; the host clock for the rest of each round), after one unprofiled fit as the warm-up; the whole fit (host clock
              around a synchronise, median of 3) with and without compaction; rounds, queries and live columns per round, each round's
              kernel info, the ARI against the truth at the planted K (all rows, and the blob rows alone)
  compare     N = 20,000 of the D = 768 rows: sklearn.cluster.AgglomerativeClustering(linkage='ward') on the host's CPUs (the thread
              count given caps the BLAS / OpenMP pools; scipy's linkage is one thread) against scd_amd.ward.Ward
  flagship    one default `bench.py --gpus 1` line from a fresh child process, to show the flagship path beside these numbers

  python tools/ward_bench.py [--parts fit compare flagship] [--threads 16] [--out profiles/ward_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import synth                                            # noqa: E402
from scd_amd import ops, ward                                       # noqa: E402
from scd_amd.knn import unit_rows                                   # noqa: E402
import hdbscan_bench as hb                                          # noqa: E402

SHAPES = ((50000, 768), (126976, 768), (126976, 32))


def rows_and_truth(n, d):
    if d == hb.D:
        return hb.rows_and_truth(n)
    x, y, _ = synth.clustered_features(n, d, hb.CLASSES, noise=hb.NOISE)
    return np.ascontiguousarray(x, dtype=np.float32), np.asarray(y, dtype=np.int64)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def emit(rows, **row):
    row = dict(tool="ward_bench", device=torch.cuda.get_device_name(0), **row)
    print(json.dumps(row), flush=True)
    rows.append(row)


def fit_part(rows, n, d):
    from sklearn.metrics import adjusted_rand_score as ari
    x, y = rows_and_truth(n, d)
    u = unit_rows(torch.as_tensor(x).cuda())
    ward.ward_tree(u)                                           # warm-up: code objects, allocator
    z, prof = ward.ward_tree(u, profile=True)
    fits = [wall(lambda: ward.ward_tree(u))[1] for _ in range(3)]
    plain = [wall(lambda: ward.ward_tree(u, compact=False))]
    t = time.perf_counter()
    labels = ward.cut_tree(z, hb.CLASSES)
    cut_s = time.perf_counter() - t
    blob = y >= 0
    emit(rows, part="fit", n=n, d=d, classes=hb.CLASSES, rounds=prof["rounds"], queries=prof["queries"], live=prof["live"],
         work_n2=float(sum(q * m for q, m in zip(prof["queries"], prof["live"])) / n / n), round_info=prof["round_info"],
         nearest_ms=prof["nearest_ms"], host_ms=prof["host_ms"], nearest_ms_sum=float(sum(prof["nearest_ms"])),
         host_ms_sum=float(sum(prof["host_ms"])), compactions=prof["compactions"], full_requeries=prof["full_requeries"],
         inversions=prof["inversions"], fit_s=float(np.median(fits)), fit_s_all=fits,
         fit_s_no_compaction=float(min(p[1] for p in plain)), no_compaction_same_tree=bool(np.array_equal(plain[0][0][0], z)),
         cut_tree_s=cut_s, ari_truth=float(ari(y, labels)), ari_truth_blob_rows=float(ari(y[blob], labels[blob])),
         ws_bytes=int(ops._L().scd_ward_nearest_ws_bytes(n, n, d)))


def compare(rows, threads):
    from sklearn.cluster import AgglomerativeClustering
    from sklearn.metrics import adjusted_rand_score as ari
    n = 20000
    x, y = rows_and_truth(n, hb.D)
    u = unit_rows(torch.as_tensor(x).cuda())
    model = ward.Ward(n_clusters=hb.CLASSES)
    model.fit(u)                                                # warm-up
    _, dev_s = wall(lambda: model.fit(u))
    u64 = u.cpu().numpy().astype(np.float64)
    t = time.perf_counter()
    sk = AgglomerativeClustering(n_clusters=hb.CLASSES, linkage="ward").fit(u64)
    sk_s = time.perf_counter() - t
    emit(rows, part="compare", n=n, d=hb.D, n_clusters=hb.CLASSES, device_s=dev_s, device_rounds=model.info_["rounds"], sklearn_s=sk_s,
         sklearn_threads=threads, ari_device_truth=float(ari(y, model.labels_)), ari_sklearn_truth=float(ari(y, sk.labels_)),
         ari_device_sklearn=float(ari(sk.labels_, model.labels_)))


def flagship(rows):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    emit(rows, part="flagship", returncode=r.returncode, bench_line=json.loads(lines[-1]) if lines else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["fit", "compare", "flagship"], choices=["fit", "compare", "flagship"])
    ap.add_argument("--threads", type=int, default=16, help="CPU threads scikit-learn may use in the comparison")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ward_bench.py needs a HIP device"
    rows = []
    try:
        if "fit" in args.parts:
            for n, d in SHAPES:
                fit_part(rows, n, d)
        if "compare" in args.parts:
            compare(rows, args.threads)
        if "flagship" in args.parts:
            flagship(rows)
    finally:
        if args.out and rows:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                for r in rows:
                    fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
