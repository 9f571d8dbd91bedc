#!/usr/bin/env python
"""Times scd_silhouette by itself on synthetic blobs (100 true classes, D = 768): one JSON line per (shape, K), no assertions.

Shapes as tools/estimate_k_bench.py: n50k (N = 50,000, K = 100) and imagenet100 (N = 126,976, K = 100 and K = 1000).  The labels are
those of `KMeans(n_clusters=K, random_state=0)` on the same rows, whose fit is timed beside it (ONE un-warmed fit, perf_counter wall
time between synchronisations - estimate_k_bench's convention).  `silhouette_ms`: HIP events around ops.silhouette (workspace
allocation included), median of 10 after 2 warm-up calls; TFLOP/s counts 2 n^2 dp (dp = d rounded up to 32).  `sim_topk_ms`: the
similarity top-k kernel (ops.sim_topk, raw, k = 5) on an n x n x d problem of the same rows against themselves - the same MFMA work
without the square-root epilogue - timed the same way.

  python tools/silhouette_bench.py [--shape n50k|imagenet100|both] [--out profiles/silhouette_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import synth                                            # noqa: E402
from scd_amd import ops                                             # noqa: E402
from scd_amd.cluster import KMeans                                  # noqa: E402


def ev_ms(fn, reps=10, warm=2):
    """Median HIP-event time of fn() in ms."""
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def shape(name, n, d, classes, ks):
    x, _, _ = synth.clustered_features(n, d, classes, noise=0.6)
    feats = ops.l2norm_rows(torch.as_tensor(x).cuda())
    f16 = feats.half()
    dp = (d + 31) // 32 * 32
    flop = 2.0 * n * n * dp
    rows = []
    try:
        sim_ms = ev_ms(lambda: ops.sim_topk(f16, f16, 5, "raw"))
        sim = dict(sim_topk_ms=sim_ms, sim_topk_tflops=2.0 * n * n * d / sim_ms / 1e9)
    except Exception as e:                                          # reported, not hidden: the line then carries the reason
        sim = dict(sim_topk_error=str(e)[:200])
    for K in ks:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        km = KMeans(n_clusters=K, random_state=0).fit(feats)
        torch.cuda.synchronize()
        fit_ms = (time.perf_counter() - t0) * 1e3
        lab = km.labels_device_.to(torch.int32)
        sizes = torch.bincount(lab.long(), minlength=K)
        ms = ev_ms(lambda: ops.silhouette(f16, lab, K))
        _, mean, info = ops.silhouette(f16, lab, K)
        row = dict(tool="silhouette_bench", device=torch.cuda.get_device_name(0), shape=name, n=n, d=d, dp=dp, K=K,
                   cluster_rows_min=int(sizes.min()), cluster_rows_max=int(sizes.max()), silhouette=float(mean.item()),
                   non_empty=int(info[1]), silhouette_ms=ms, silhouette_tflops=flop / ms / 1e9, fit_ms=fit_ms, n_iter=int(km.n_iter_),
                   ws_bytes=int(ops._L().scd_silhouette_ws_bytes(n, d, K)))
        row.update(sim)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["both", "n50k", "imagenet100"], default="both")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    rows = []
    if args.shape in ("both", "n50k"):
        rows += shape("n50k", 50000, 768, 100, [100])
    if args.shape in ("both", "imagenet100"):
        rows += shape("imagenet100", 126976, 768, 100, [100, 1000])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
