#!/usr/bin/env python
"""Times HDBSCAN on the device (scd_amd/hdbscan.py, scd_amd/csrc/hdbscan.hip, scd_amd/csrc/hdbscan_tree.cpp) on synthetic blobs (100
true classes, D = 768, noise 0.6, tools/knn_bench.py's rows) plus 5 % unstructured Gaussian rows: one JSON line per measurement, no
assertions - there is no earlier number for a feature that did not exist.  docs/design/hdbscan.md reports the lines.

  fit         N = 50,000 and N = 126,976, min_cluster_size 50, min_samples 10: the core-distance call (unit rows + ops.knn; HIP events,
              median of 5 after 1 warm-up call), every Boruvka round of one fit (HIP events around ops.mr_nearest, each round once: the
              rounds differ, so there is no median; the first round is run once beforehand as the warm-up, and its fp16 copy is remade
              inside the timed first round as in a fit) with its info and component count, the host's share per round (choice, merge),
              the tree's host time (median of 3), the whole fit (host clock around a synchronise, median of 3), clusters found, noise
              share and the ARI against the truth (the unstructured rows as a class of their own)
  compare     N = 20,000 of those rows: sklearn.cluster.HDBSCAN(algorithm='brute', n_jobs = the thread count given) on the host's CPUs
              against scd_amd.hdbscan.HDBSCAN: wall time each, the ARI of each against the truth and of one against the other
  flagship    one default `bench.py --gpus 1` line from a fresh child process, to show the flagship path beside these numbers

  python tools/hdbscan_bench.py [--parts fit compare flagship] [--sizes 50000 126976] [--threads 16] [--out profiles/hdbscan_bench.json]
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

from oracle import synth                                            # noqa: E402
from scd_amd import hdbscan, ops                                    # noqa: E402
from scd_amd.knn import unit_rows                                   # noqa: E402

D, CLASSES, NOISE, OUTLIERS = 768, 100, 0.6, 0.05
MIN_CLUSTER_SIZE, MIN_SAMPLES = 50, 10


def rows_and_truth(n):
    """n rows: (1 - OUTLIERS) n blob rows and OUTLIERS n Gaussian rows, shuffled; the truth has -1 for the Gaussian rows."""
    n_out = int(round(n * OUTLIERS))
    x, y, _ = synth.clustered_features(n - n_out, D, CLASSES, noise=NOISE)
    r = np.random.RandomState(7)
    x = np.concatenate([x.astype(np.float32), r.randn(n_out, D).astype(np.float32)])
    y = np.concatenate([np.asarray(y, dtype=np.int64), -np.ones(n_out, dtype=np.int64)])
    p = r.permutation(n)
    return np.ascontiguousarray(x[p]), y[p]


def ev_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def ev_ms(fn, reps=5, warm=1):
    for _ in range(warm):
        fn()
    return float(np.median([ev_once(fn)[1] for _ in range(reps)]))


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def emit(rows, **row):
    row = dict(tool="hdbscan_bench", device=torch.cuda.get_device_name(0), **row)
    print(json.dumps(row), flush=True)
    rows.append(row)


def fit_part(rows, n):
    from sklearn.metrics import adjusted_rand_score as ari
    x, y = rows_and_truth(n)
    xd = torch.as_tensor(x).cuda()
    core_ms = ev_ms(lambda: hdbscan.core_dots(unit_rows(xd), MIN_SAMPLES))
    u = unit_rows(xd)
    core, kinfo = hdbscan.core_dots(u, MIN_SAMPLES)
    ws = ops.mr_nearest_workspace(u)
    comp = np.arange(n, dtype=np.int64)
    ops.mr_nearest(u, core, torch.as_tensor(comp.astype(np.int32)).cuda(), ws=ws)                  # warm-up: code objects
    per_round, ncomp = [], n
    while ncomp > 1:
        cd = torch.as_tensor(comp.astype(np.int32)).cuda()
        (nn, r, info), ms = ev_once(lambda: ops.mr_nearest(u, core, cd, ws=ws, prepared=len(per_round) > 0))
        t = time.perf_counter()
        lo, hi, _ = hdbscan.choose_edges(comp, nn.cpu().numpy(), r.cpu().numpy())
        comp = hdbscan._merge(comp, lo, hi)
        host_s = time.perf_counter() - t
        per_round.append(dict(components=ncomp, device_ms=ms, host_choice_and_merge_ms=1e3 * host_s, info=info.cpu().tolist()))
        ncomp = len(np.unique(comp))
    del ws
    model = hdbscan.HDBSCAN(min_cluster_size=MIN_CLUSTER_SIZE, min_samples=MIN_SAMPLES)
    fits = [wall(lambda: model.fit(xd))[1] for _ in range(3)]
    lo, hi, _, w = model.mst_
    trees = []
    for _ in range(3):
        t = time.perf_counter()
        ops.hdbscan_tree(lo, hi, w, MIN_CLUSTER_SIZE)
        trees.append(time.perf_counter() - t)
    emit(rows, part="fit", n=n, d=D, classes=CLASSES, unstructured_share=OUTLIERS, min_cluster_size=MIN_CLUSTER_SIZE, min_samples=MIN_SAMPLES,
         unit_rows_and_core_dots_ms=core_ms, knn_info=kinfo.cpu().tolist(), rounds=len(per_round), per_round=per_round,
         rounds_device_ms=sum(p["device_ms"] for p in per_round), tree_host_ms=1e3 * float(np.median(trees)), fit_s=float(np.median(fits)),
         fit_s_all=fits, clusters=int(model.n_clusters_), noise_share=float((model.labels_ < 0).mean()),
         ari_truth=float(ari(y, model.labels_)), ws_bytes=int(ops._L().scd_mr_nearest_ws_bytes(n, D)))


def compare(rows, threads):
    from sklearn.cluster import HDBSCAN as SkHDBSCAN
    from sklearn.metrics import adjusted_rand_score as ari
    n = 20000
    x, y = rows_and_truth(n)
    xd = torch.as_tensor(x).cuda()
    model = hdbscan.HDBSCAN(min_cluster_size=MIN_CLUSTER_SIZE, min_samples=MIN_SAMPLES)
    model.fit(xd)                                               # warm-up: code objects, allocator
    _, dev_s = wall(lambda: model.fit(xd))
    u = unit_rows(xd).cpu().numpy().astype(np.float64)
    t = time.perf_counter()
    sk = SkHDBSCAN(min_cluster_size=MIN_CLUSTER_SIZE, min_samples=MIN_SAMPLES, algorithm="brute", metric="euclidean", n_jobs=threads, copy=True).fit(u)
    sk_s = time.perf_counter() - t
    emit(rows, part="compare", n=n, d=D, min_cluster_size=MIN_CLUSTER_SIZE, min_samples=MIN_SAMPLES, device_s=dev_s, device_rounds=model.info_["rounds"],
         sklearn_s=sk_s, sklearn_threads=threads, sklearn_algorithm="brute", clusters_device=int(model.n_clusters_), clusters_sklearn=int(sk.labels_.max()) + 1,
         noise_device=int((model.labels_ < 0).sum()), noise_sklearn=int((sk.labels_ < 0).sum()), ari_device_truth=float(ari(y, model.labels_)),
         ari_sklearn_truth=float(ari(y, sk.labels_)), ari_device_sklearn=float(ari(sk.labels_, model.labels_)),
         labels_equal=bool(np.array_equal(sk.labels_, model.labels_)))


def flagship(rows):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    emit(rows, part="flagship", returncode=r.returncode, bench_line=json.loads(lines[-1]) if lines else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["fit", "compare", "flagship"], choices=["fit", "compare", "flagship"])
    ap.add_argument("--sizes", nargs="+", type=int, default=[50000, 126976])
    ap.add_argument("--threads", type=int, default=16, help="CPU threads scikit-learn may use in the comparison")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hdbscan_bench.py needs a HIP device"
    rows = []
    try:
        if "fit" in args.parts:
            for n in args.sizes:
                fit_part(rows, n)
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
