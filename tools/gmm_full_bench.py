#!/usr/bin/env python
"""Times the full-covariance mixture (ops.gmm_full_em_step, scd_amd/csrc/gmm_full.hip; scd_amd.gmm_full.FullGaussianMixture) on
synthetic rotated blobs (K classes, a random rotation and standard deviations from 0.5 to 2 each, centres 3 N(0, I)): N in {50,000,
126,976} x d in {16, 32, 64} x K in {100, 1000}, one JSON line per shape, no assertions on time.

  step_ms              HIP-event time of one ops.gmm_full_em_step call at the parameters of the hard M-step on the true classes: median
                       of 10 after 2 warm-up calls (workspace allocation included); step_tflops counts 4 N K d^2 (the two products
                       of the density and of S as dense ones), step_peak = that over the 157.3 TFLOP/s float32-MFMA peak
  diag_step_ms         yardstick 1: ops.gmm_em_step (the diagonal mixture) on the same rows and classes, timed in the same run
  fit_s, fit_iter, ... FullGaussianMixture(K, random_state=0, max_iter=20).fit on the same rows (k-means start, the host's M-step and
                       Cholesky factors and their copies included), wall time with a synchronize at the end; fit_purity
  sklearn_s            --sklearn, yardstick 2: scikit-learn's GaussianMixture(100, 'full', random_state=0) on the first 20,000 rows of
                       the 50000x32x100 case on the host
--once runs one step per shape and times nothing: for a rocprofv3 --kernel-trace run of its own, which gives the split between
gmmf_fwd_kernel, gmmf_moment_kernel and the rest; --kernel_trace CSV appends that run's per-step kernel times to --out (it runs nothing).

  python tools/gmm_full_bench.py [--shapes 50000x16x100 ...] [--out profiles/gmm_full_bench.json] [--once] [--sklearn] [--no_fit]
  python tools/gmm_full_bench.py --kernel_trace CSV --out profiles/gmm_full_bench.json
"""
import argparse
import csv
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scd_amd import gmm, gmm_full, ops                              # noqa: E402

PEAK_TFLOPS = 157.3
SHAPES = ["%dx%dx%d" % (n, d, k) for n in (50000, 126976) for d in (16, 32, 64) for k in (100, 1000)]


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


def rotated_blobs(n, d, k, seed=0):
    rng = np.random.default_rng(seed)
    y = np.arange(n) % k
    rng.shuffle(y)
    x = np.empty((n, d), np.float32)
    centres = 3.0 * rng.standard_normal((k, d))
    for j in range(k):
        rows = np.flatnonzero(y == j)
        q = np.linalg.qr(rng.standard_normal((d, d)))[0]
        sd = np.exp(rng.uniform(np.log(0.5), np.log(2.0), d))
        x[rows] = centres[j] + (sd * rng.standard_normal((len(rows), d))) @ q.T
    return x, y


def shape(n, d, k, once, with_sklearn, with_fit):
    x, y = rotated_blobs(n, d, k)
    u = torch.as_tensor(x).cuda()
    yd = torch.as_tensor(y).cuda().to(torch.int32)
    L = ops._L()
    row = dict(tool="gmm_full_bench", device=torch.cuda.get_device_name(0), n=n, d=d, k=k, ws_bytes=int(L.scd_gmm_full_ws_bytes(n, d, k)),
               row_tile=int(L.scd_gmm_full_row_tile()), chain_rows=int(L.scd_gmm_full_chain_rows()))
    gm0 = gmm_full.FullGaussianMixture(n_components=k)
    zero = torch.zeros((k, d), dtype=torch.float32, device=u.device)
    nk, s1, _ = gm0._hard(u, yd, zero)
    centres = (s1 / nk[:, None]).astype(np.float32)
    nk, s1c, S = gm0._hard(u, yd, torch.as_tensor(centres, device=u.device))
    w, mu, cov = gmm_full.m_step(nk, s1c, S, centres.astype(np.float64), "full", 1e-6)
    a, m32, ut = gmm_full.kernel_params(w, mu, gmm_full.precision_cholesky_t(cov), u.device)
    ll, _, _, _, _, info = ops.gmm_full_em_step(u, a, m32, ut)
    row.update(ll=float(ll.item()), info=[int(v) for v in info.cpu().tolist()])
    if once:
        return row
    ms = ev_ms(lambda: ops.gmm_full_em_step(u, a, m32, ut))
    tf = 4.0 * n * k * d * d / ms / 1e9
    row.update(step_ms=ms, step_tflops=tf, step_peak=tf / PEAK_TFLOPS)
    _, dnk, ds1, ds2, _, _ = ops.gmm_em_step(u, None, None, None, y=yd, n_components=k)
    da, db, dc = gmm.kernel_params(*gmm.m_step(dnk, ds1, ds2, "diag", 1e-6))
    row.update(diag_step_ms=ev_ms(lambda: ops.gmm_em_step(u, da, db, dc)))
    t0 = time.perf_counter()
    S.copy()                                                    # for scale: the host's share of a step
    ut64 = gmm_full.precision_cholesky_t(cov)
    row.update(host_cholesky_s=time.perf_counter() - t0)
    del ut64
    if with_fit:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", gmm.ConvergenceWarning)
            gm = gmm_full.FullGaussianMixture(n_components=k, random_state=0, max_iter=20).fit(u)
        torch.cuda.synchronize()
        row.update(fit_s=time.perf_counter() - t0, fit_iter=gm.n_iter_, fit_converged=bool(gm.converged_), fit_lower_bound=gm.lower_bound_,
                   fit_bic=gm.bic(u))
        table = np.zeros((k, k), dtype=np.int64)
        np.add.at(table, (gm.labels_, np.asarray(y, dtype=np.int64)), 1)
        row.update(fit_purity=float(table.max(axis=1).sum() / n))
    if with_sklearn:
        from sklearn.mixture import GaussianMixture
        xu = x[:20000].astype(np.float64)
        t0 = time.perf_counter()
        sk = GaussianMixture(n_components=k, covariance_type="full", random_state=0).fit(xu)
        row.update(sklearn_s=time.perf_counter() - t0, sklearn_rows=20000, sklearn_k=k, sklearn_iter=int(sk.n_iter_),
                   sklearn_threads=int(os.environ.get("OMP_NUM_THREADS", "0")))
    return row


def kernel_split(path, shapes):
    """[{n, d, k, pack, fwd, moment, nk, finish}] in ms, one per shape, from the kernel_trace CSV of a --once run over `shapes` under
    rocprofv3 --kernel-trace: a gmmf_pack_kernel dispatch opens a density step (the hard M-steps before it are not counted)."""
    with open(path) as fh:
        rows = [r for r in csv.DictReader(fh) if "gmmf_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out, open_ = [], False
    for r in rows:
        short = r["Kernel_Name"].split("gmmf_")[1].split("_kernel")[0]
        if short == "pack":
            out.append({})
            open_ = True
        if open_:
            out[-1][short] = out[-1].get(short, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if short == "finish":
            open_ = False
    assert len(out) == len(shapes), "the trace holds %d density steps, not one per shape" % len(out)
    for o, s in zip(out, shapes):
        o["n"], o["d"], o["k"] = (int(v) for v in s.split("x"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=SHAPES, help="NxDxK")
    ap.add_argument("--once", action="store_true", help="one step per shape and no timing: for a kernel trace")
    ap.add_argument("--sklearn", action="store_true", help="also time scikit-learn's full fit on 20,000 rows of the 50000x32x100 case")
    ap.add_argument("--no_fit", action="store_true", help="time the step alone")
    ap.add_argument("--kernel_trace", default=None, help="kernel_trace CSV of a --once run over --shapes under rocprofv3 --kernel-trace: "
                    "nothing runs, its per-step kernel times are appended to --out")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if args.kernel_trace:
        row = dict(tool="gmm_full_bench", kernel_trace="one --once run under rocprofv3 --kernel-trace",
                   steps_ms=kernel_split(args.kernel_trace, args.shapes))
        print(json.dumps(row), flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(json.dumps(row) + "\n")
        return
    assert torch.cuda.is_available()
    rows = []
    for s in args.shapes:
        n, d, k = (int(v) for v in s.split("x"))
        rows.append(shape(n, d, k, args.once, args.sklearn and s == "50000x32x100", not args.no_fit))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
