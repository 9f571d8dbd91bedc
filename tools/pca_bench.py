#!/usr/bin/env python
"""Times the PCA primitives (ops.pca_colsum / pca_gram / pca_transform, scd_amd/csrc/pca.hip; scd_amd.pca.PCA) on synthetic blobs (as
tools/gmm_bench.py: oracle.synth.clustered_features, noise 0.6, unit rows), D = 768, N in {50,000, 126,976} x M components in {64, 768}:
one JSON line per shape, no assertions - there is no earlier number for a feature that did not exist.

  colsum_ms, gram_ms, transform_ms, transform_unit_ms   HIP-event time of one call, median of 10 after 2 warm-up calls (workspace
                       allocation included); gram_tflops counts the upper-triangle tiles the kernel computes, 2 N 128^2 tiles
  eigh_ms              wall time of the host torch.linalg.eigh of the D x D covariance (median of 5)
  fit_transform_ms     wall time of PCA(M).fit_transform(rows, unit=True) with a synchronize at the end (median of 5)
  torch_f64_ms, torch_f64_peak_bytes   the yardstick, in the same run: the float64 torch path tsne.pca_init takes (x.double(), centring,
                       xc.T @ xc, host eigh, xc @ axes.T with M axes), HIP-event time (median of 5 after 1 warm-up call) and its peak extra
                       memory from torch.cuda.max_memory_allocated
--once runs one call of each primitive per shape and times nothing: for a rocprofv3 --kernel-trace run of its own, which gives the split
between the kernels; --kernel_trace CSV appends that run's per-kernel times to --out (it runs nothing).

  python tools/pca_bench.py [--shapes 50000x64 ...] [--out profiles/pca_bench.json] [--once]
  python tools/pca_bench.py --kernel_trace CSV --out profiles/pca_bench.json
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import synth                                            # noqa: E402
from scd_amd import ops, pca                                        # noqa: E402
from scd_amd.knn import unit_rows                                   # noqa: E402

D = 768
SHAPES = ["50000x64", "50000x768", "126976x64", "126976x768"]


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


def wall_ms(fn, reps=5):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def torch_f64(x, m):
    """tsne.pca_init's sequence with m axes: a float64 copy, a centred copy, the Gram product, the host eigh, the projection."""
    xd = x.double()
    xc = xd - xd.mean(dim=0, keepdim=True)
    cov = (xc.T @ xc).cpu()
    _, vecs = torch.linalg.eigh(cov)
    axes = torch.flip(vecs, dims=(1,))[:, :m].T.contiguous().to(x.device)
    return xc @ axes.T


def shape(n, m, once):
    x, _, _ = synth.clustered_features(n, D, 100, noise=0.6)
    u = unit_rows(torch.as_tensor(x).cuda())
    L = ops._L()
    row = dict(tool="pca_bench", device=torch.cuda.get_device_name(0), n=n, d=D, m=m, ws_bytes=int(L.scd_pca_ws_bytes(n, D, m)),
               row_tile=int(L.scd_pca_row_tile()), chain_rows=int(L.scd_pca_chain_rows()))
    a = (ops.pca_colsum(u) / n).float()
    g, info = ops.pca_gram(u, a)
    p = pca.PCA(n_components=m).fit(u)
    y, info_t = ops.pca_transform(u, p._w, a, unit=True)
    row.update(info=[int(v) for v in info.cpu().tolist()], info_transform=[int(v) for v in info_t.cpu().tolist()],
               explained=float(p.explained_variance_ratio_.sum()))
    if once:
        return row
    tiles = (D // 128) * (D // 128 + 1) // 2
    gram_ms = ev_ms(lambda: ops.pca_gram(u, a))
    cov = (g.cpu() / (n - 1))
    row.update(colsum_ms=ev_ms(lambda: ops.pca_colsum(u, a)), gram_ms=gram_ms, gram_tflops=2.0 * n * 128 * 128 * tiles / gram_ms / 1e9,
               eigh_ms=wall_ms(lambda: torch.linalg.eigh(cov)),
               transform_ms=ev_ms(lambda: ops.pca_transform(u, p._w, a)), transform_unit_ms=ev_ms(lambda: ops.pca_transform(u, p._w, a, unit=True)),
               transform_tflops=2.0 * n * D * m / ev_ms(lambda: ops.pca_transform(u, p._w, a)) / 1e9,
               fit_transform_ms=wall_ms(lambda: pca.PCA(n_components=m).fit_transform(u, unit=True)))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ref = torch_f64(u, m)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    # the two paths agree on the subspace: the largest difference of the projections' Gram matrices, for the record
    yp = ops.pca_transform(u[:2000], p._w, a)[0].double()
    r = ref[:2000]
    row.update(torch_f64_peak_bytes=int(peak), projections_agree=float(((yp @ yp.T) - (r @ r.T)).abs().max().item()))
    del ref, r, yp
    row.update(torch_f64_ms=ev_ms(lambda: torch_f64(u, m), reps=5, warm=1))
    return row


def kernel_split(path, shapes):
    """[{n, m, kernel: ms}] one per shape, from the kernel_trace CSV of a --once run over `shapes` under rocprofv3 --kernel-trace: each
    shape's LAST dispatch of every pca_ kernel (its fit and calls before end with the unit transform)."""
    with open(path) as fh:
        rows = [r for r in csv.DictReader(fh) if "pca_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    groups = [[]]
    for r in rows:                                              # a --once shape dispatches the projection kernel once, at its end
        groups[-1].append(r)
        if "pca_fwd" in r["Kernel_Name"]:
            groups.append([])
    groups = [g for g in groups if g]
    assert len(groups) == len(shapes), "the trace holds %d projection dispatches, not one per shape" % len(groups)
    out = []
    for g, s in zip(groups, shapes):
        o = {}
        for r in g:
            short = r["Kernel_Name"].split("pca_")[1].split("_kernel")[0]
            o[short] = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        o["n"], o["m"] = (int(v) for v in s.split("x"))
        out.append(o)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=SHAPES, help="NxM")
    ap.add_argument("--once", action="store_true", help="one call per shape and no timing: for a kernel trace")
    ap.add_argument("--kernel_trace", default=None, help="kernel_trace CSV of a --once run over --shapes under rocprofv3 --kernel-trace: "
                    "nothing runs, its per-kernel times are appended to --out")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if args.kernel_trace:
        row = dict(tool="pca_bench", kernel_trace="one --once run under rocprofv3 --kernel-trace", kernels_ms=kernel_split(args.kernel_trace, args.shapes))
        print(json.dumps(row), flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(json.dumps(row) + "\n")
        return
    assert torch.cuda.is_available()
    rows = []
    for s in args.shapes:
        n, m = (int(v) for v in s.split("x"))
        rows.append(shape(n, m, args.once))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
