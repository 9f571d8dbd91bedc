#!/usr/bin/env python
"""Times the number-of-categories search (scd_amd.estimate_k) on synthetic blobs: one JSON line, no assertions.

Two sweeps (bounded Brent, as the driver's default): N = 50,000, D = 768, K in [80, 400]; and the ImageNet-100 shape N = 126,976,
D = 768, K in [50, 1000].  Per evaluated K: the fit, the scoring through metrics.score_split (contingency + statistics on the
device, two D x D tables to the host, Munkres twice), the scoring the host path needs for the same four-by-two scores (labels_ to the
host, np.add.at tables, sklearn-free integer statistics, Munkres twice), and - Munkres being common to both - the table-building parts
alone: scd_contingency + scd_contingency_stats against the device-to-host copy of the labels + np.add.at.  Device times are HIP-event
times on the stream after a warm-up, medians of `--reps` repetitions; the host path is timed with perf_counter around synchronised
calls; the fit is ONE un-warmed fit per K, perf_counter wall time between synchronisations.  `estep_multipass` is the rule K > 128
(where scd_kmeans_estep leaves its single-pass streaming kernel at D = 768), stated here, not read from the library.  `--shape`
picks one of the two sweeps; `--quick` runs the end-to-end test's small shape."""
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
from scd_amd import estimate_k as ek, metrics, ops                  # noqa: E402
from scd_amd.cluster import KMeans                                  # noqa: E402


ESTEP_SINGLE_PASS_MAX_K = 128     # scd_kmeans_estep's streaming kernel serves K <= 128 (docs/design/estep.md); an assumption of this tool


def ev_ms(fn, reps, warm=2):
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


def wall_ms(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out))


def host_tables(pred, truth, mask, d):
    w = np.zeros((2, d, d), dtype=int)
    np.add.at(w, (np.where(mask, 0, 1), pred, truth), 1)
    return w


def host_scores(w):
    out = []
    for t in w:
        ind = ops.munkres(t.max() - t)
        out.append(sum([t[i, j] for i, j in ind]) * 1.0 / max(1, t.sum()))
    return out


def sweep(n, d, classes, small_k, big_k, reps):
    x, y, _ = synth.clustered_features(n, d, classes, noise=0.6)
    perm, mask_lab = synth.labelled_split(y, classes, prop=0.5)
    x, y = x[perm], y[perm].astype(int)
    feats = ops.l2norm_rows(torch.as_tensor(x).cuda())
    targets, mask = torch.as_tensor(y).cuda(), torch.as_tensor(mask_lab).cuda()
    sub = mask.to(torch.uint8)
    t32 = targets.to(torch.int32)
    per_k = []

    def evaluate(K):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        km = KMeans(n_clusters=int(K), random_state=0).fit(feats)
        torch.cuda.synchronize()
        fit_ms = (time.perf_counter() - t0) * 1e3
        lab = km.labels_device_
        dd = max(int(K), int(y.max()) + 1)
        scores = metrics.score_split(lab, targets, mask)
        row = dict(K=int(K), n_iter=int(km.n_iter_), fit_ms=fit_ms, labelled_acc=scores["labelled"]["acc"],
                   estep_multipass=bool(int(K) > ESTEP_SINGLE_PASS_MAX_K),
                   score_split_ms=wall_ms(lambda: metrics.score_split(lab, targets, mask), reps),
                   host_score_ms=wall_ms(lambda: host_scores(host_tables(lab.cpu().numpy(), y, mask_lab, dd)), reps),
                   device_tables_stats_ms=ev_ms(lambda: ops.contingency_stats(ops.contingency(lab, t32, sub, dd, dd)[0]), max(reps, 10)),
                   host_labels_copy_add_at_ms=wall_ms(lambda: host_tables(lab.cpu().numpy(), y, mask_lab, dd), reps),
                   contingency_path=ops.contingency_last_path())
        per_k.append(row)
        return row["labelled_acc"]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x_opt, k_opt, trace = ek.brent(evaluate, small_k, big_k)
    torch.cuda.synchronize()
    total = (time.perf_counter() - t0) * 1e3
    fit = sum(r["fit_ms"] for r in per_k)
    timing = sum(r["score_split_ms"] + r["host_score_ms"] + r["host_labels_copy_add_at_ms"] for r in per_k) * 1.0
    return dict(n=n, d=d, true_classes=classes, k_range=[small_k, big_k], estimated_k=k_opt, brent_x=x_opt,
                visited=[t[1] for t in trace], distinct_k=len(per_k), fit_ms_total=fit,
                fit_ms_multipass_estep=sum(r["fit_ms"] for r in per_k if r["estep_multipass"]),
                multipass_share_of_fits=(sum(r["fit_ms"] for r in per_k if r["estep_multipass"]) / fit) if fit else 0.0,
                score_split_ms_total=sum(r["score_split_ms"] for r in per_k), host_score_ms_total=sum(r["host_score_ms"] for r in per_k),
                sweep_wall_ms_including_repeated_timing=total, timing_overhead_ms_approx=timing, per_k=per_k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--shape", choices=["both", "n50k", "imagenet100"], default="both")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    out = dict(tool="estimate_k_bench", device=torch.cuda.get_device_name(0), reps=args.reps, sweeps=[])
    if args.quick:
        out["sweeps"].append(sweep(3000, 64, 20, 10, 64, args.reps))
    else:
        if args.shape in ("both", "n50k"):
            out["sweeps"].append(sweep(50000, 768, 100, 80, 400, args.reps))
        if args.shape in ("both", "imagenet100"):
            out["sweeps"].append(sweep(126976, 768, 100, 50, 1000, args.reps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
