"""The three hot gemm_w4_kernel variants of the CLIP encoder at the smallest shapes that reach what an edit of their instruction streams
can break: a block that runs two tiles in a row (the rows a residual tile parks in its accumulator registers meet the next tile's
first, C = 0, MFMAs; the fragment reads and ring fills of a tile's last chunk belong to the next tile) and a single tile (the refills
past a block's last chunk).  Through the test entry points scd_gemm_res_stats_f16 (LN = 2: proj / fc2, residual + row statistics) and
scd_gemm_ln_apply_f16 (LN = 1: QKV with bias, fc1 with QuickGELU, and the GELU of the DINO tower).

  grid: 256 blocks at most, so 261 tiles (M = 22,272 = 87 row tiles x N = 768; M = 7,424 = 29 x N = 2304) and 264 tiles (M = 5,632 = 22
  x N = 3072, two n-groups of six tile columns) give five or eight blocks a second tile; K = 768 (12 chunks) and 3072 (48 chunks).

Each case asserts
  * the float64-oracle budget of tests/test_gpu_gemm.py (gemm_cases.budget_plain / budget_folded, imported, derived there);
  * LN = 2: the two fixed-point row sums of every row, within the bound test_gemm_real_within_budget derives (13 v of the fp32
    summation relative to sum |c| and sum c^2, one unit per 128-column partial for the rounding to fixed point; the float64 sum of
    squares this file compares with adds 768 * 2^-53 relative, taken as 2^-40);
  * that a second run gives the same bits (LN = 2: the second run is in place, as the encoder blocks run it);
  * that the bits are those of the commit BEFORE the hot variants were put on their instruction diet: sha256 of the output bytes (C;
    LN = 2 also the statistics, LN = 1 also ln_finish_kernel's {rstd, -mean * rstd}) recorded in tests/golden/gemm_hot_variants.json.
    Every operand is drawn on the host from a seeded numpy RandomState and the LayerNorm fold is gemm_cases.fold_host, so the inputs
    do not depend on any device code.  The file was written by `python tests/test_gpu_gemm_hot_variants.py --write-golden` on an MI355X
    with SCD_HIP_LIB pointing at a build of commit a8860ed (the parent of the change); it says so itself.

Run time: the float64 products dominate.  For the 22,272-row cases (105 GFLOP each at K = 3072, three of them inside gemm_f64 +
budget_plain) they run on the device in float64 (_plain_on_device: budget_plain's three lines in torch, then gemm_cases._finish), and
the test asserts on the first 256 rows that this equals co.gemm_f64 and gc.budget_plain themselves.  Rows: gemm_cases.real_rows draws
256 rows and row tile t holds them rotated by t places, so every row tile's A differs from every other's row for row while the
68 million normal deviates of a full draw (four seconds) are not needed; residual, W and bias are drawn in full.
Measured on the MI355X: the nine cases take 7.8 s, the slowest (GELU at 5,632 x 3072, its host float64 products) 2.4 s.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":      # --write-golden: the paths conftest.py sets up under pytest
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "tests")]

import gemm_cases as gc
from oracle import clip_oracle as co

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_hot_variants.json")

# (entry point, m, n, k, act)
CASES = [
    ("res_stats", 22272, 768, 768, 0),      # proj: 261 tiles
    ("res_stats", 22272, 768, 3072, 0),     # fc2
    ("ln_apply", 5632, 3072, 768, 1),       # fc1, QuickGELU: 264 tiles
    ("ln_apply", 5632, 3072, 768, 2),       # GELU
    ("ln_apply", 7424, 2304, 768, 0),       # QKV: 261 tiles
    ("res_stats", 256, 256, 768, 0),        # one tile of each variant
    ("ln_apply", 256, 256, 768, 0),
    ("ln_apply", 256, 256, 768, 1),
    ("ln_apply", 256, 256, 768, 2),
]


def _cid(c):
    return "%s-%dx%dx%d-act%d" % c


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def row_stats_fixed(x):
    """co.row_stats_int for real-valued fp16 rows without its per-element Python integers: n = x * 2^24 is an integer below 2^31, n^2
    below 2^62 is split at bit 28 so that both partial sums stay in int64, and the sum of squares (units 2^-48) is rounded to units of
    2^-20 to nearest, ties to even"""
    n = np.rint(np.asarray(x, dtype=np.float64) * 2.0 ** 24).astype(np.int64)
    assert int(np.abs(n).max(initial=0)) < 2 ** 31
    sq = n * n
    hi, lo = (sq >> 28).sum(1), (sq & ((1 << 28) - 1)).sum(1)
    q, r = hi + (lo >> 28), lo & ((1 << 28) - 1)
    q = q + ((r > (1 << 27)) | ((r == (1 << 27)) & (q & 1 == 1)))
    return np.stack([n.sum(1), q], 1)


def _inputs(case):
    kind, m, n, k, act = case
    seed = m + 3 * n + 7 * k + act
    rs = np.random.RandomState(seed)
    base, _ = gc.real_rows(256, k, seed=seed + 1)
    a = np.concatenate([np.roll(base, t, axis=0) for t in range(m // 256)])
    if kind == "res_stats":
        w = gc.f16(rs.randn(n, k) * k ** -0.5)
        bias = rs.randn(n).astype(np.float32)
        res = gc.f16(rs.randn(m, n) * 2.0 ** rs.randint(-6, 3, size=(m, 1)))
        return dict(a=a, w=w, bias=bias, res=res)
    w, gamma, beta, bias = gc.real_layer(n, k, seed=seed + 2)
    wf, colsum, biasf = gc.fold_host(w, gamma, beta, bias)
    stats = row_stats_fixed(a)
    assert np.array_equal(stats[:64], co.row_stats_int(a[:64]))
    return dict(a=a, wf=wf, colsum=colsum, biasf=biasf, stats=stats, eps=1e-5 if act != 2 else 1e-6)


def _run(ops, case, x, in_place=False):
    """one launch; returns the output tensors whose bytes are compared, C first"""
    kind, m, n, k, act = case
    if kind == "res_stats":
        st = torch.zeros((m, 2), dtype=torch.int64, device="cuda")
        res = dev(x["res"])
        c = ops.gemm_res_stats_f16(dev(x["a"]), dev(x["w"]), dev(x["bias"]), res, st, out=res if in_place else None)
        torch.cuda.synchronize()
        return [c, st]
    rsb = torch.empty((m, 2), dtype=torch.float32, device="cuda")
    c = ops.gemm_ln_apply_f16(dev(x["a"]), dev(x["wf"]), dev(x["biasf"]), dev(x["colsum"]), dev(x["stats"]), x["eps"], act, rs=rsb)
    torch.cuda.synchronize()
    return [c, rsb]


def _plain_on_device(x):
    """co.gemm_f64 and gc.budget_plain (no activation, bias and residual) with the two float64 products on the device"""
    a, w = dev(x["a"]).double(), dev(x["w"]).double().t().contiguous()
    pre = (a @ w).cpu().numpy() + x["bias"].astype(np.float64)
    mag = (a.abs() @ w.abs()).cpu().numpy()
    d_pre = gc.C1 * gc.U32 * gc.k_eff(x["a"].shape[1]) * mag + gc.U32 * np.abs(pre)
    ref, bnd = pre + x["res"].astype(np.float64), gc._finish(pre, d_pre, 0, x["res"])
    h = 256
    ref_h = co.gemm_f64(x["a"][:h], x["w"], x["bias"], 0, x["res"][:h])
    bnd_h = gc.budget_plain(x["a"][:h], x["w"], x["bias"], 0, x["res"][:h])
    assert np.abs(ref[:h] - ref_h).max() <= 1e-9 * float(bnd_h.min()) and np.allclose(bnd[:h], bnd_h, rtol=1e-9, atol=0.0)
    return ref, bnd


def _digests(outs):
    return [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in outs]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device; they must not be skipped on the GPU box"
    from scd_amd import ops as o
    return o


@pytest.fixture(scope="module")
def golden_digests():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_hot_variant(ops, golden_digests, case):
    kind, m, n, k, act = case
    x = _inputs(case)
    outs = _run(ops, case, x)
    c64 = outs[0].cpu().numpy().astype(np.float64)
    if kind == "res_stats":
        if m > 256:
            ref, bnd = _plain_on_device(x)
        else:
            ref = co.gemm_f64(x["a"], x["w"], x["bias"], 0, x["res"])
            bnd = gc.budget_plain(x["a"], x["w"], x["bias"], 0, x["res"])
    else:
        ref, parts = co.gemm_ln_folded_f64(x["a"], x["wf"], x["biasf"], x["colsum"], x["stats"], x["eps"], act)
        _, kappa = gc.rstd_rel_error(parts, x["eps"], k, False)
        assert float(kappa.max()) <= gc.KAPPA_LIMIT
        bnd = gc.budget_folded(x["a"], x["wf"], x["biasf"], x["colsum"], parts, x["eps"], act)
    err = np.abs(c64 - ref)
    assert np.isfinite(err).all()
    ratio = float((err / bnd).max())
    print("%s: worst err / budget %.3f" % (_cid(case), ratio))
    assert ratio <= 1.0, "%d elements over budget, worst err / budget %.3g" % (int((err > bnd).sum()), ratio)
    if kind == "res_stats":
        got = outs[1].cpu().numpy()
        want1 = np.rint(c64 * 2.0 ** 24).astype(np.int64).sum(1)
        want2 = (c64 * c64).sum(1) * 2.0 ** 20
        tol1 = 13 * gc.U32 * np.abs(c64).sum(1) * 2.0 ** 24 + n / 128
        tol2 = (13 * gc.U32 + 2.0 ** -40) * want2 + n / 128
        d1, d2 = np.abs(got[:, 0] - want1), np.abs(got[:, 1] - want2)
        print("row sums: worst |d| / tol %.3f, squares %.3f" % (float((d1 / tol1).max()), float((d2 / tol2).max())))
        assert (d1 <= tol1).all() and (d2 <= tol2).all()
    again = _run(ops, case, x, in_place=True)
    for i, (p, q) in enumerate(zip(outs, again)):
        assert torch.equal(p, q), "output %d of the second run differs in %d places" % (i, int((p != q).sum()))
    assert _digests(outs) == golden_digests[_cid(case)], "bits differ from the parent commit's (tests/golden/gemm_hot_variants.json)"


def _write_golden():
    from scd_amd import ops as o
    dig = {_cid(case): _digests(_run(o, case, _inputs(case))) for case in CASES}
    how = ("sha256 of the output bytes of tests/test_gpu_gemm_hot_variants.py's cases ([C, statistics] for res_stats, [C, rs] for ln_apply), "
           "written by `python tests/test_gpu_gemm_hot_variants.py --write-golden` on an MI355X with SCD_HIP_LIB = a build of commit a8860ed, "
           "the parent of the commit that removed instructions from the hot gemm_w4_kernel variants")
    with open(GOLDEN, "w") as f:
        json.dump({"how": how, "digests": dig}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)


if __name__ == "__main__":
    assert "--write-golden" in sys.argv
    _write_golden()
