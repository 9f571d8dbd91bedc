#!/usr/bin/env python
"""Times FINCH (scd_amd.finch, scd_amd/csrc/finch.hip) on synthetic blobs (100 true classes, D = 768): one JSON line per shape, no
assertions - there is no earlier number for a feature that did not exist.

Shapes as tools/silhouette_bench.py: n50k (N = 50,000) and imagenet100 (N = 126,976).  HIP events, median of 10 after 2 warm-up calls
(workspace allocation included):
  first_neighbor_ms   the level-0 pass, ops.first_neighbor on the unit rows; `exact_rows` of it took the exact full-row pass;
                      TFLOP/s counts 2 n^2 dp (dp = d rounded up to 32)
  fit_ms              the whole Finch().fit (all levels, min_sim, components, means; it synchronises inside); `num_clust`, and per level
                      the rows through the exact pass
  sim_topk_ms         ops.sim_topk (raw, k = 2) of the same rows (fp16) against themselves: the same MFMA work, the yardstick
  req100_ms           ONE Finch(req_clust=100).fit, wall time between synchronisations, the fit included; `req100_steps` merges were
                      needed (0 when a partition already has 100 clusters)

  python tools/finch_bench.py [--shape n50k|imagenet100|both] [--out profiles/finch_bench.json]
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
from scd_amd.finch import Finch                                     # noqa: E402


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


def shape(name, n, d, classes, reps):
    x, _, _ = synth.clustered_features(n, d, classes, noise=0.6)
    feats = torch.as_tensor(x).cuda()
    ident = torch.arange(n + 1, device=feats.device)
    _, u = ops.segment_mean_unit(feats, ident[:n].to(torch.int32), ident)
    dp = (d + 31) // 32 * 32
    row = dict(tool="finch_bench", device=torch.cuda.get_device_name(0), shape=name, n=n, d=d, dp=dp, classes=classes,
               ws_bytes=int(ops._L().scd_first_neighbor_ws_bytes(n, d)))
    _, _, info = ops.first_neighbor(u)
    row.update(exact_rows=int(info[0]), exact_share=float(info[0]) / n)
    print(json.dumps(dict(row, note="probe")), flush=True)
    ms = ev_ms(lambda: ops.first_neighbor(u), reps)
    row.update(first_neighbor_ms=ms, first_neighbor_tflops=2.0 * n * n * dp / ms / 1e9)
    f16 = u.half()
    try:
        sim_ms = ev_ms(lambda: ops.sim_topk(f16, f16, 2, "raw"), reps)
        row.update(sim_topk_ms=sim_ms, sim_topk_tflops=2.0 * n * n * d / sim_ms / 1e9)
    except Exception as e:                                          # reported, not hidden: the line then carries the reason
        row.update(sim_topk_error=str(e)[:200])
    f = Finch().fit(feats)
    row.update(num_clust=[int(v) for v in f.num_clust_], exact_rows_per_level=[int(v) for v in f.exact_rows_], min_sim=f.min_sim_)
    row.update(fit_ms=ev_ms(lambda: Finch().fit(feats), reps))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g = Finch(req_clust=100).fit(feats)
    torch.cuda.synchronize()
    start = [v for v in g.num_clust_ if v >= 100]
    row.update(req100_ms=(time.perf_counter() - t0) * 1e3, req100_steps=(start[-1] - 100) if start else None,
               req100_clusters=int(g.req_labels_device_.max().item()) + 1)
    print(json.dumps(row), flush=True)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["both", "n50k", "imagenet100"], default="both")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available()
    rows = []
    if args.shape in ("both", "n50k"):
        rows += shape("n50k", 50000, 768, 100, args.reps)
    if args.shape in ("both", "imagenet100"):
        rows += shape("imagenet100", 126976, 768, 100, args.reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
