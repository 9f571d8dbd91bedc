#!/usr/bin/env python
"""Times spectral clustering on the exact k-NN graph (scd_amd/spectral.py, scd_amd/csrc/graph.hip) on synthetic blobs (100 true classes,
D = 768, noise 0.6, tools/knn_bench.py's rows): one JSON line per measurement, no assertions - there is no earlier number for a feature
that did not exist.  docs/design/spectral.md reports the lines.

  graph       N = 126,976, n_neighbors 10: unit rows + ops.knn and ops.knn_affinity (HIP events, median of 10 after 2 warm-up calls), nnz,
              median and longest row
  spmm        ops.spmm_f64 at m = 128 on that graph, the plain product and the recurrence form (median of 20 after 3): ms, and the rate
              of the gathered bytes nnz * m * 8 alone and of all bytes the launch must move (gather + CSR entries + x, z, y rows).  The
              x block is 130 MB: it fits the 256 MiB Infinity Cache, so this is a cache figure, not an HBM one.
  solve       eigsolve at K = 100 (tol 1e-6 and 1e-8) and, with --k1000, K = 1000: sparse products, outer iterations, final residual,
              total time (host clock around a synchronise) and its shares: the sparse products, the host's m x m work (eigh, Cholesky), and
              the seeded start block (drawn and made orthonormal) and the rest = torch's dense float64 products,
              element-wise passes and copies.  The shares come from a second, instrumented solve
              that synchronises around every call; the total from an uninstrumented one.
  compare     N = 20,000, K = 100: scikit-learn's SpectralClustering(affinity='nearest_neighbors') on the host's CPUs (n_jobs = the
              thread count given) against scd_amd.spectral.SpectralClustering, wall time each and the ARI of each against the truth and
              of one against the other.

  python tools/spectral_bench.py [--parts graph spmm solve compare] [--k1000] [--threads 16] [--out profiles/spectral_bench.json]
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
from scd_amd import ops, spectral                                   # noqa: E402
from scd_amd.knn import unit_rows                                   # noqa: E402

# MI355X gather rates the sparse product is set beside (chip-wide, whole rows of about 1 KiB gathered by index)
GUIDE_RATES_TBPS = {"rows served from one XCD's L2": "16.8-18.8", "38 MB table, random rows (Infinity Cache)": "8.6",
                    "151 MB table, random rows": "7.4-7.9", "far larger than the Infinity Cache, into registers (HBM)": "5.5-5.8"}


def ev_ms(fn, reps=10, warm=2):
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
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


class Shares:
    """Wraps the operator and the host's two m x m functions with a synchronise and a clock each."""

    def __init__(self, apply):
        self.t = dict(spmm=0.0, host=0.0, start=0.0)
        self.inner = apply
        self.saved = (spectral._small_eigh, spectral._small_factor, spectral._start_block)

    def timed(self, key, fn):
        def run(*a):
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn(*a)
            torch.cuda.synchronize()
            self.t[key] += time.perf_counter() - t
            return out
        return run

    def __enter__(self):
        spectral._small_eigh, spectral._small_factor = self.timed("host", self.saved[0]), self.timed("host", self.saved[1])
        spectral._start_block = self.timed("start", self.saved[2])
        return self.timed("spmm", self.inner)

    def __exit__(self, *exc):
        spectral._small_eigh, spectral._small_factor, spectral._start_block = self.saved


def emit(rows, **row):
    row = dict(tool="spectral_bench", device=torch.cuda.get_device_name(0), **row)
    print(json.dumps(row), flush=True)
    rows.append(row)


def solve(rows, csr, n, k, tol, max_outer=500):
    op = spectral.device_operator(*csr)
    try:
        (w, v, info), total = wall(lambda: spectral.eigsolve(op, n, k, tol=tol, max_outer=max_outer, device=csr[0].device))
    except spectral.NotConverged as e:
        emit(rows, part="solve", n=n, k=k, tol=tol, **e.info)
        return
    del w, v
    shares = Shares(op)
    with shares as timed_op:
        _, total_sync = wall(lambda: spectral.eigsolve(timed_op, n, k, tol=tol, max_outer=max_outer, device=csr[0].device))
    # the start block's own m x m factorisations are counted under "start", not under "host"
    rest = total_sync - shares.t["spmm"] - shares.t["host"] - shares.t["start"]
    emit(rows, part="solve", n=n, k=k, tol=tol, solve_s=total, instrumented_solve_s=total_sync, share_spmm=shares.t["spmm"] / total_sync,
         share_host_small=shares.t["host"] / total_sync, share_start_block=shares.t["start"] / total_sync, share_dense_and_rest=rest / total_sync, ms_per_product_in_solve=1e3 * shares.t["spmm"] / info["products"],
         **info)


def big(rows, parts, k1000):
    n, d, classes, nn = 126976, 768, 100, 10
    x, _, _ = synth.clustered_features(n, d, classes, noise=0.6)
    xd = torch.as_tensor(x).cuda()
    u = unit_rows(xd)
    idx, _, _ = ops.knn(u, u, nn - 1, 0)
    rowptr, col, val, isd, nnz = ops.knn_affinity(idx)
    lens = (rowptr[1:] - rowptr[:-1]).cpu().numpy()
    if "graph" in parts:
        knn_ms = ev_ms(lambda: ops.knn(unit_rows(xd), u, nn - 1, 0))
        aff_ms = ev_ms(lambda: ops.knn_affinity(idx))
        emit(rows, part="graph", n=n, d=d, n_neighbors=nn, unit_rows_and_knn_ms=knn_ms[0], affinity_ms=aff_ms[0], affinity_ms_min_max=aff_ms[1:],
             nnz=nnz, median_row=float(np.median(lens)), max_row=int(lens.max()), rows_over_512=int((lens > 512).sum()),
             affinity_ws_bytes=int(ops._L().scd_knn_affinity_ws_bytes(n, nn - 1)))
    if "spmm" in parts:
        m = spectral.block_width(100)
        g = torch.Generator().manual_seed(0)
        xb, zb = (torch.randn(n, m, generator=g, dtype=torch.float64).cuda() for _ in range(2))
        out = torch.empty_like(xb)
        for form, args in (("plain", (1.0, 0.0, 0.0, None)), ("recurrence", (2.3, 0.4, -1.0, zb))):
            ms = ev_ms(lambda: ops.spmm_f64(rowptr, col, val, xb, *args, out=out), reps=20, warm=3)
            gathered = nnz * m * 8
            moved = gathered + nnz * 12 + (n + 1) * 8 + n * m * 8 * (3 if args[3] is not None else 2)
            emit(rows, part="spmm", form=form, n=n, m=m, nnz=nnz, ms=ms[0], ms_min_max=ms[1:], x_block_bytes=n * m * 8, gathered_bytes=gathered,
                 gathered_TBps=gathered / ms[0] / 1e9, all_bytes=moved, all_TBps=moved / ms[0] / 1e9, guide_gather_rates_TBps=GUIDE_RATES_TBPS,
                 note="the x block (130 MB) fits the 256 MiB Infinity Cache: a cache figure, not an HBM one")
        del xb, zb, out
    if "solve" in parts:
        spectral.eigsolve(spectral.device_operator(rowptr, col, val), n, 100, tol=1e-2, device=rowptr.device)      # warm-up: the BLAS's code objects
        for tol in (1e-6, 1e-8):
            solve(rows, (rowptr, col, val), n, 100, tol)
        if k1000:
            solve(rows, (rowptr, col, val), n, 1000, 1e-6, max_outer=60)


def compare(rows, threads):
    from sklearn.cluster import SpectralClustering as SkSC
    from sklearn.metrics import adjusted_rand_score as ari
    n, d, k, nn = 20000, 768, 100, 10
    x, y, _ = synth.clustered_features(n, d, k, noise=0.6)
    xd = torch.as_tensor(x).cuda()
    spectral.SpectralClustering(k, n_neighbors=nn, random_state=0).fit(xd)              # warm-up: code objects, allocator
    model, dev_s = wall(lambda: spectral.SpectralClustering(k, n_neighbors=nn, random_state=0).fit(xd))
    t = time.perf_counter()
    sk = SkSC(n_clusters=k, affinity="nearest_neighbors", n_neighbors=nn, random_state=0, n_jobs=threads).fit(x)
    sk_s = time.perf_counter() - t
    emit(rows, part="compare", n=n, d=d, k=k, n_neighbors=nn, device_s=dev_s, device_info=model.info_, sklearn_s=sk_s, sklearn_threads=threads,
         ari_device_truth=float(ari(y, model.labels_)), ari_sklearn_truth=float(ari(y, sk.labels_)), ari_device_sklearn=float(ari(sk.labels_, model.labels_)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["graph", "spmm", "solve", "compare"], choices=["graph", "spmm", "solve", "compare"])
    ap.add_argument("--k1000", action="store_true", help="also solve K = 1000 at N = 126,976 (blocks of 1.3 GB)")
    ap.add_argument("--threads", type=int, default=16, help="CPU threads scikit-learn may use in the comparison")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "spectral_bench.py needs a HIP device"
    rows = []
    try:
        if set(args.parts) & {"graph", "spmm", "solve"}:
            big(rows, args.parts, args.k1000)
        if "compare" in args.parts:
            compare(rows, args.threads)
    finally:
        if args.out and rows:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                for r in rows:
                    fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
