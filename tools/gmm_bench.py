#!/usr/bin/env python
"""Times the Gaussian mixture (ops.gmm_em_step, scd_amd/csrc/gmm.hip; scd_amd.gmm.GaussianMixture) on synthetic blobs (as
tools/probe_bench.py: oracle.synth.clustered_features, noise 0.6, unit rows), D = 768, N in {50,000, 126,976} x K components in
{100, 1000}: one JSON line per shape, no assertions - there is no earlier number for a feature that did not exist.

  step_ms              HIP-event time of one ops.gmm_em_step call at the parameters of the hard M-step on the true classes: median of 10
                       after 2 warm-up calls (workspace allocation included); step_tflops counts the four products, 8 N D K
                       (x B, x^2 C, r^T x, r^T x^2)
  fit_s, fit_iter, fit_converged, fit_lower_bound, fit_bic   GaussianMixture(K, random_state=0).fit on the same rows (k-means start
                       included), wall time with a synchronize at the end; fit_purity: rows whose component's majority class is theirs
  min_top2_gap         the smallest difference between a row's two largest log-densities at the fitted parameters (from
                       predict_proba: -log of the runner-up's share where it is above float32's floor, else reported as > 87)
  sklearn_s            --sklearn: scikit-learn's GaussianMixture(K = 100, 'diag') on the first 20,000 rows on the host, for scale
--once runs one step per shape and times nothing: for a rocprofv3 --kernel-trace run of its own, which gives the split between
gmm_fwd_kernel, gmm_moment_kernel and the rest; --kernel_trace CSV appends that run's per-step kernel times to --out (it runs nothing).

  python tools/gmm_bench.py [--shapes 50000x100 ...] [--out profiles/gmm_bench.json] [--once] [--sklearn] [--no_fit]
  python tools/gmm_bench.py --kernel_trace CSV --out profiles/gmm_bench.json
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
from scd_amd import gmm, ops                                        # noqa: E402
from scd_amd.knn import unit_rows                                   # noqa: E402

D = 768
SHAPES = ["50000x100", "50000x1000", "126976x100", "126976x1000"]


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


def shape(n, k, once, with_sklearn, with_fit):
    x, y, _ = synth.clustered_features(n, D, k, noise=0.6)
    u = unit_rows(torch.as_tensor(x).cuda())
    yd = torch.as_tensor(y).cuda().to(torch.int32)
    row = dict(tool="gmm_bench", device=torch.cuda.get_device_name(0), n=n, d=D, k=k, ws_bytes=int(ops._L().scd_gmm_ws_bytes(n, D, k)),
               row_tile=int(ops._L().scd_gmm_row_tile()), chain_rows=int(ops._L().scd_gmm_chain_rows()))
    _, nk, s1, s2, _, _ = ops.gmm_em_step(u, None, None, None, y=yd, n_components=k)
    a, b, c = gmm.kernel_params(*gmm.m_step(nk, s1, s2, "diag", 1e-6))
    ll, _, _, _, _, info = ops.gmm_em_step(u, a, b, c)
    row.update(ll=float(ll.item()), info=[int(v) for v in info.cpu().tolist()])
    if once:
        return row
    ms = ev_ms(lambda: ops.gmm_em_step(u, a, b, c))
    row.update(step_ms=ms, step_tflops=8.0 * n * D * k / ms / 1e9)
    if with_fit:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gm = gmm.GaussianMixture(n_components=k, random_state=0).fit(u)
        torch.cuda.synchronize()
        row.update(fit_s=time.perf_counter() - t0, fit_iter=gm.n_iter_, fit_converged=bool(gm.converged_), fit_lower_bound=gm.lower_bound_,
                   fit_bic=gm.bic(u))
        table = np.zeros((k, k), dtype=np.int64)
        np.add.at(table, (gm.labels_, np.asarray(y, dtype=np.int64)), 1)
        row.update(fit_purity=float(table.max(axis=1).sum() / n))
        part = gm.predict_proba(u[:20000])
        top = torch.topk(part, 2, dim=1).values.double()
        second = top[:, 1]
        gap = torch.where(second > 0, torch.log(top[:, 0]) - torch.log(second.clamp_min(1e-300)), torch.full_like(second, float("inf")))
        row.update(min_top2_gap=float(gap.min().item()) if bool(torch.isfinite(gap.min())) else "> 87",
                   rows_with_a_second_share_above_1e_3=int((second > 1e-3).sum().item()))
    if with_sklearn:
        from sklearn.mixture import GaussianMixture
        xu = u[:20000].cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        sk = GaussianMixture(n_components=100, covariance_type="diag", random_state=0).fit(xu)
        row.update(sklearn_s=time.perf_counter() - t0, sklearn_rows=20000, sklearn_k=100, sklearn_iter=int(sk.n_iter_),
                   sklearn_threads=int(os.environ.get("OMP_NUM_THREADS", "0")))
    return row


def kernel_split(path, shapes):
    """[{n, k, hard, pack, fwd, moment, nk, finish}] in ms, one per shape, from the kernel_trace CSV of a --once run over `shapes` under
    rocprofv3 --kernel-trace: the LAST gmm_pack_kernel dispatch of a shape opens its density step."""
    with open(path) as fh:
        rows = [r for r in csv.DictReader(fh) if "gmm_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out, open_ = [], False
    for r in rows:
        short = r["Kernel_Name"].split("gmm_")[1].split("_kernel")[0]
        if short == "pack":                                     # a density step: pack, fwd, moment, nk, finish; a shape's hard M-step
            out.append({})                                      # before it (hard, moment, nk, finish) is not counted
            open_ = True
        if open_:
            out[-1][short] = out[-1].get(short, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if short == "finish":
            open_ = False
    assert len(out) == len(shapes), "the trace holds %d density steps, not one per shape" % len(out)
    for o, s in zip(out, shapes):
        o["n"], o["k"] = (int(v) for v in s.split("x"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=SHAPES, help="NxK")
    ap.add_argument("--once", action="store_true", help="one step per shape and no timing: for a kernel trace")
    ap.add_argument("--sklearn", action="store_true", help="also time scikit-learn on 20,000 rows of the 50000x100 case")
    ap.add_argument("--no_fit", action="store_true", help="time the step alone")
    ap.add_argument("--kernel_trace", default=None, help="kernel_trace CSV of a --once run over --shapes under rocprofv3 --kernel-trace: "
                    "nothing runs, its per-step kernel times are appended to --out")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if args.kernel_trace:
        row = dict(tool="gmm_bench", kernel_trace="one --once run under rocprofv3 --kernel-trace", steps_ms=kernel_split(args.kernel_trace, args.shapes))
        print(json.dumps(row), flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(json.dumps(row) + "\n")
        return
    assert torch.cuda.is_available()
    rows = []
    for s in args.shapes:
        n, k = (int(v) for v in s.split("x"))
        rows.append(shape(n, k, args.once, args.sklearn and s == "50000x100", not args.no_fit))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
