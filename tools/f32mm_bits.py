#!/usr/bin/env python
"""SHA-256 digests of everything the probe, gmm and pca primitives return (scd_amd/csrc/probe.hip, gmm.hip, pca.hip on f32mm.h), on the
cases of tests/probe_cases.py, tests/gmm_cases.py and tests/pca_cases.py: the three units promise that two calls return the same bits,
so a change that is meant to leave their arithmetic alone must leave every digest alone.  Run it in a fresh process on the checkout
before the change and on the one after it, and compare the two files key for key:

  python tools/f32mm_bits.py --out profiles/f32mm_bits_parent.json       (in the parent's checkout)
  python tools/f32mm_bits.py --out profiles/f32mm_bits_head.json
  python tools/f32mm_bits.py --compare profiles/f32mm_bits_parent.json profiles/f32mm_bits_head.json

The digests depend on the toolchain's expf / logf and are no golden: only two files from the same toolchain and device are comparable.

Cases: every case of probe_cases.all_cases() (probe_loss_grad with pred, probe_predict with the two largest logits), of
gmm_cases.all_cases() (gmm_em_step, soft or hard as the case says, with pred; gmm_predict with row_ll and resp), of pca_cases.gram_cases()
(pca_colsum, pca_gram) and pca_cases.transform_cases() (pca_transform, plain and unit); the specials: pca's nan and zero-row cases, and
a row with a NaN planted in a probe and a gmm case.  Uses scd_amd.ops alone."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gmm_cases as gc                                              # noqa: E402
import pca_cases as pc                                              # noqa: E402
import probe_cases as pb                                            # noqa: E402
from scd_amd import ops                                             # noqa: E402


def dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


def digest(t):
    """SHA-256 of a tensor's raw bytes (with its dtype and shape), None for an output the call does not produce."""
    if t is None:
        return None
    a = t.detach().cpu().contiguous().numpy()
    return "%s%s:%s" % (a.dtype, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest())


def probe(case):
    x, y, w, b, sw = dev(case["X"]), dev(case["y"], np.int32), dev(case["W"]), dev(case["b"]), dev(case["sw"])
    loss, gw, gb, pred, info = ops.probe_loss_grad(x, y, w, b, sw, want_pred=True)
    ppred, top2 = ops.probe_predict(x, w, b, want_top=True)
    return dict(loss=digest(loss), gW=digest(gw), gb=digest(gb), pred=digest(pred), info=digest(info), predict_pred=digest(ppred),
                top2=digest(top2))


def gmm(case):
    x, y, sw = dev(case["X"]), dev(case["y"], np.int32), dev(case["sw"])
    a, b, c = dev(case["a"]), dev(case["B"]), dev(case["C"])
    if case["hard"]:
        ll, nk, s1, s2, pred, info = ops.gmm_em_step(x, None, None, None, y=y, sample_weight=sw, n_components=int(case["a"].shape[0]))
    else:
        ll, nk, s1, s2, pred, info = ops.gmm_em_step(x, a, b, c, y=y, sample_weight=sw, want_pred=True)
    ppred, row_ll, resp = ops.gmm_predict(x, a, b, c, want_ll=True, want_resp=True)
    return dict(ll=digest(ll), nk=digest(nk), s1=digest(s1), s2=digest(s2), pred=digest(pred), info=digest(info), predict_pred=digest(ppred),
                row_ll=digest(row_ll), resp=digest(resp))


def pca_gram(case):
    x, a = dev(case["X"]), dev(case["a"])
    g, info = ops.pca_gram(x, a)
    return dict(csum=digest(ops.pca_colsum(x, a)), G=digest(g), info=digest(info))


def pca_transform(case):
    x, a, w = dev(case["X"]), dev(case["a"]), dev(case["W"])
    out = {}
    for name, unit in (("plain", False), ("unit", True)):
        y, info = ops.pca_transform(x, w, a, unit=unit)
        out["y_" + name], out["info_" + name] = digest(y), digest(info)
    return out


def with_nan_row(case):
    out = dict(case)
    out["X"] = case["X"].copy()
    out["X"][out["X"].shape[0] // 2, 0] = np.nan
    return out


def run():
    out = {}
    cases = pb.all_cases()
    cases["c33-base+nan_row"] = with_nan_row(cases["c33-base"])
    for name, case in cases.items():
        out["probe/" + name] = probe(case)
    cases = gc.all_cases()
    cases["k33-unlabelled+nan_row"] = with_nan_row(cases["k33-unlabelled"])
    for name, case in cases.items():
        out["gmm/" + name] = gmm(case)
    cases = pc.gram_cases()
    cases["nan_case"] = pc.nan_case()
    for name, case in cases.items():
        out["pca_gram/" + name] = pca_gram(case)
    cases = pc.transform_cases()
    cases["zero_row_case"] = pc.zero_row_case()
    cases["nan_case"] = dict(pc.nan_case(), W=pc.transform_cases()[pc.transform_name(231, 768, 100, "plain")]["W"][:7, :129])
    for name, case in cases.items():
        out["pca_transform/" + name] = pca_transform(case)
    torch.cuda.synchronize()
    return out


def compare(pa, pb_):
    with open(pa) as fh:
        a = json.load(fh)["digests"]
    with open(pb_) as fh:
        b = json.load(fh)["digests"]
    bad = sorted(set(a) ^ set(b)) + sorted(k for k in set(a) & set(b) if a[k] != b[k])
    for k in bad:
        print("differs: %s" % k)
        for q in sorted(set(a.get(k, {})) | set(b.get(k, {}))):
            if a.get(k, {}).get(q) != b.get(k, {}).get(q):
                print("    %s: %s | %s" % (q, a.get(k, {}).get(q), b.get(k, {}).get(q)))
    print("%d cases, %d differ" % (len(set(a) | set(b)), len(bad)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the digests to this JSON file")
    ap.add_argument("--compare", nargs=2, default=None, metavar="JSON", help="compare two such files key for key; nothing runs")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    assert torch.cuda.is_available()
    row = dict(tool="f32mm_bits", device=torch.cuda.get_device_name(0), digests=run())
    print("%d cases" % len(row["digests"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(row, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
