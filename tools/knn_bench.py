#!/usr/bin/env python
"""Times the exact k-NN graph (ops.knn, scd_amd/csrc/knn.hip) on synthetic blobs (100 true classes, D = 768, noise 0.6): one JSON line
per shape, no assertions - there is no earlier number for a feature that did not exist.

Shapes as tools/finch_bench.py: n50k (N = 50,000) and imagenet100 (N = 126,976).  HIP events, median of 10 after 2 warm-up calls
(workspace allocation included):
  knn_ms[k]            ops.knn(u, u, k, self_base=0) on the unit rows for k = 1, 20, 64; `info[k]` = rows through the exact full-row pass,
                       fp16 flag, rows whose slots overflowed, largest candidate count; TFLOP/s counts the TWO filter passes, 4 n^2 dp
  first_neighbor_ms    ops.first_neighbor of the same rows (one filter pass), the line docs/design/finch.md reports
  sim_topk_ms          ops.sim_topk (raw, k = 2) of the same rows (fp16) against themselves
  vote_ms              ops.knn_vote (softmax) on the k = 20 graph
--once runs each call a single time and times nothing: for a kernel trace, which gives the split between the two MFMA passes
(knn_bound_kernel, knn_emit_kernel) and the rest (fn_prep_kernel, knn_thresh_kernel, knn_refine_kernel).

  python tools/knn_bench.py [--shape n50k|imagenet100|both] [--ks 1 20 64] [--out profiles/knn_bench.json] [--once]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import synth                                            # noqa: E402
from scd_amd import ops                                             # noqa: E402
from scd_amd.knn import unit_rows                                   # noqa: E402


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


def shape(name, n, d, classes, ks, reps, once):
    x, y, _ = synth.clustered_features(n, d, classes, noise=0.6)
    u = unit_rows(torch.as_tensor(x).cuda())
    labels = torch.as_tensor(y).cuda().to(torch.int32)
    dp = (d + 31) // 32 * 32
    row = dict(tool="knn_bench", device=torch.cuda.get_device_name(0), shape=name, n=n, d=d, dp=dp, classes=classes, slots=int(ops._L().scd_knn_slots()),
               knn_ms={}, knn_tflops={}, info={}, ws_bytes={})
    for k in ks:
        idx, dot, info = ops.knn(u, u, k, 0)
        row["info"][str(k)] = [int(v) for v in info.cpu().tolist()]
        row["ws_bytes"][str(k)] = int(ops._L().scd_knn_ws_bytes(n, n, d, k))
        if k == 20:
            pred, _ = ops.knn_vote(idx, dot, labels)
            row["knn_acc_k20"] = float((pred.long() == labels.long()).double().mean().item())
            if not once:
                row["vote_ms"] = ev_ms(lambda: ops.knn_vote(idx, dot, labels), reps)
        if not once:
            ms = ev_ms(lambda: ops.knn(u, u, k, 0), reps)
            row["knn_ms"][str(k)] = ms
            row["knn_tflops"][str(k)] = 4.0 * n * n * dp / ms / 1e9
        print(json.dumps(dict(shape=name, k=k, info=row["info"][str(k)], knn_ms=row["knn_ms"].get(str(k)), note="probe")), flush=True)
    if not once:
        _, _, finfo = ops.first_neighbor(u)
        ms = ev_ms(lambda: ops.first_neighbor(u), reps)
        row.update(first_neighbor_ms=ms, first_neighbor_tflops=2.0 * n * n * dp / ms / 1e9, first_neighbor_exact_rows=int(finfo[0]),
                   first_neighbor_ws_bytes=int(ops._L().scd_first_neighbor_ws_bytes(n, d)))
        f16 = u.half()
        try:
            sim_ms = ev_ms(lambda: ops.sim_topk(f16, f16, 2, "raw"), reps)
            row.update(sim_topk_ms=sim_ms, sim_topk_tflops=2.0 * n * n * d / sim_ms / 1e9)
        except Exception as e:                                      # reported, not hidden: the line then carries the reason
            row.update(sim_topk_error=str(e)[:200])
    print(json.dumps(row), flush=True)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["both", "n50k", "imagenet100"], default="both")
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 20, 64])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--once", action="store_true", help="one call per k and no timing: for a kernel trace")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    rows = []
    if args.shape in ("both", "n50k"):
        rows += shape("n50k", 50000, 768, 100, args.ks, args.reps, args.once)
    if args.shape in ("both", "imagenet100"):
        rows += shape("imagenet100", 126976, 768, 100, args.ks, args.reps, args.once)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
