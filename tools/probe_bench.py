#!/usr/bin/env python
"""Times the linear probe (ops.probe_loss_grad, scd_amd/csrc/probe.hip; scd_amd.probe.LinearProbe) on synthetic blobs (as
tools/knn_bench.py: oracle.synth.clustered_features, noise 0.6, unit rows), D = 768, N in {50,000, 63,488, 126,976} x C classes in
{100, 1000}: one JSON line per shape, no assertions - there is no earlier number for a feature that did not exist.

  eval_ms              HIP-event time of one ops.probe_loss_grad call at W = 0.01 randn, b = 0: median of 10 after 2 warm-up calls
                       (workspace allocation included); eval_tflops counts both products, 4 N D C
  fit_s, fit_iter, fit_eval, fit_train_acc      LinearProbe(C=1).fit on the same rows, wall time with a synchronize at the end
  sklearn_s            --sklearn: scikit-learn's LogisticRegression(C=1) (lbfgs, tol 1e-4) on the N = 50,000, C = 100 case on the host, for
                       scale, with its iteration count and training accuracy
--once runs one evaluation per shape and times nothing: for a rocprofv3 --kernel-trace --stats run of its own, which gives the split
between probe_fwd_kernel, probe_grad_kernel and the rest; --kernel_trace CSV appends that run's per-evaluation kernel times to --out
(it runs nothing).

  python tools/probe_bench.py [--shapes 50000x100 ...] [--out profiles/probe_bench.json] [--once] [--sklearn]
  python tools/probe_bench.py --kernel_trace CSV --out profiles/probe_bench.json
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
from scd_amd import ops                                             # noqa: E402
from scd_amd.knn import unit_rows                                   # noqa: E402
from scd_amd.probe import LinearProbe                               # noqa: E402

D = 768
SHAPES = ["50000x100", "50000x1000", "63488x100", "63488x1000", "126976x100", "126976x1000"]


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


def shape(n, classes, once, with_sklearn):
    x, y, _ = synth.clustered_features(n, D, classes, noise=0.6)
    u = unit_rows(torch.as_tensor(x).cuda())
    yd = torch.as_tensor(y).cuda().to(torch.int32)
    g = torch.Generator().manual_seed(1)
    w = (0.01 * torch.randn((classes, D), generator=g)).cuda()
    b = torch.zeros(classes, device="cuda")
    row = dict(tool="probe_bench", device=torch.cuda.get_device_name(0), n=n, d=D, classes=classes,
               ws_bytes=int(ops._L().scd_probe_ws_bytes(n, D, classes)), row_tile=int(ops._L().scd_probe_row_tile()),
               chain_rows=int(ops._L().scd_probe_chain_rows()))
    loss, _, _, _, info = ops.probe_loss_grad(u, yd, w, b)
    row.update(loss=float(loss.item()), info=[int(v) for v in info.cpu().tolist()])
    if once:
        return row
    ms = ev_ms(lambda: ops.probe_loss_grad(u, yd, w, b))
    row.update(eval_ms=ms, eval_tflops=4.0 * n * D * classes / ms / 1e9)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lp = LinearProbe(C=1.0).fit(u, y)
    torch.cuda.synchronize()
    row.update(fit_s=time.perf_counter() - t0, fit_iter=lp.n_iter_, fit_eval=lp.n_eval_, fit_converged=bool(lp.converged_),
               fit_objective=lp.objective_, fit_train_acc=lp.score(u, y))
    if with_sklearn:
        from sklearn.linear_model import LogisticRegression
        xu = u.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        sk = LogisticRegression(C=1.0, tol=1e-4, max_iter=1000).fit(xu, y)
        row.update(sklearn_s=time.perf_counter() - t0, sklearn_iter=int(sk.n_iter_[0]), sklearn_train_acc=float(sk.score(xu, y)),
                   sklearn_threads=int(os.environ.get("OMP_NUM_THREADS", "0")))
    return row


def kernel_split(path, shapes):
    """[{n, classes, pack, fwd, grad, gb, finish}] in ms, one per evaluation, from the kernel_trace CSV of a --once run over `shapes` under
    rocprofv3 --kernel-trace: every probe_pack_kernel dispatch opens an evaluation."""
    with open(path) as fh:
        rows = [r for r in csv.DictReader(fh) if "probe_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = []
    for r in rows:
        short = r["Kernel_Name"].split("probe_")[1].split("_kernel")[0]
        if short == "pack":
            out.append({})
        out[-1][short] = out[-1].get(short, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    assert len(out) == len(shapes), "the trace holds %d evaluations, not one per shape" % len(out)
    for o, s in zip(out, shapes):
        o["n"], o["classes"] = (int(v) for v in s.split("x"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=SHAPES, help="NxC")
    ap.add_argument("--once", action="store_true", help="one evaluation per shape and no timing: for a kernel trace")
    ap.add_argument("--sklearn", action="store_true", help="also time scikit-learn on the 50000x100 case")
    ap.add_argument("--kernel_trace", default=None, help="kernel_trace CSV of a --once run over --shapes under rocprofv3 --kernel-trace: "
                    "nothing runs, its per-evaluation kernel times are appended to --out")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if args.kernel_trace:
        row = dict(tool="probe_bench", kernel_trace="one --once run under rocprofv3 --kernel-trace", evaluations_ms=kernel_split(args.kernel_trace, args.shapes))
        print(json.dumps(row), flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(json.dumps(row) + "\n")
        return
    assert torch.cuda.is_available()
    rows = []
    for s in args.shapes:
        n, classes = (int(v) for v in s.split("x"))
        rows.append(shape(n, classes, args.once, args.sklearn and s == "50000x100"))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
