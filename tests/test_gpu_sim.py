"""scd_sim_topk / scd_sim_argmax, every path of sim_topk_impl, against the float64 oracle (oracle/naming_oracle.py sim_topk / sim_argmax:
float64 logits, order value descending then index ascending).  Inputs: tests/sim_cases.py (planted ladders in units of the kernels' own
error bound E, degenerate rows, a vocabulary of one repeated name, the dense Gaussian recipe).  Inputs are finite; non-finite features are
out of scope (the library leaves index -1 / NaN in such rows, sim_init_kernel).

What is asserted per case
  * indices equal the oracle's exactly (sim_topk, both modes, and sim_argmax), on every row up to n = 4,096 and on the first 512, the last
    512 and 1,024 sampled rows beyond; on EVERY row 0 <= index < V and no index twice;
  * raw values: every returned value is recomputed - sim_refine_kernel / sim_refine4_kernel return float(scale * float64 dot) for every
    row they certify (a returned candidate has rank < k, so it is within 2 E of the k-th approximate value and is recomputed), the exact
    passes do the same for the rest.  fp16 products are exact in float64, so only the float64 summation order (<= d 2^-53 relative to
    sum |f w|) and the final rounding differ from the oracle: |val - oracle| <= 1 fp32 ulp;
  * softmax values: p = __expf(float(l) - mm) / z with l the float64 logit, mm = float(max approximate logit * scale) and z the fp32 sum
    of exp2((a_j - m) * scale * log2 e) over the APPROXIMATE fp32 logits a_j (truncated keys only order candidates, they do not enter the
    sums).  Relative to the exact softmax:
      - dense inputs: |a_j scale - l_j| <= delta = scale * (d + 2) * 2^-24 * max_j sum_x |f_x w_xj| (fp32 accumulation of exact products;
        the order in which an MFMA adds its 16 products is not documented, so the worst case over d terms is the only bound that can be
        derived), and z is off by at most expm1(delta): ~2e-3 at d = 512.  Planted and repeated-name inputs accumulate exactly in fp32
        (tests/sim_cases.py), so for them delta = 0 and the bound is the rounding below alone;
      - float(l) and mm each round a number of size L = max |logit| to fp32: 2 L 2^-24 in the exponent, expm1 of that (this is what the
        kernels do: at scale 100 a row of norm 2^6 |h| has L ~ 3e6 and the term is 0.4, at scale 1000 the value carries no digit);
      - exp2 / __expf: the fp32 argument (|arg| <= min(R log2 e, 150) with R the row's logit range - beyond that the term is below
        2^-150 and gone) carries 2 |arg| 2^-24 ln 2, the instruction ~1 ulp: (2 min(R log2 e, 150) + 8) * 2^-23;
      - each lane adds at most V / 2 terms in fp32 before the pairwise merges: (V / 2 + 16) * 2^-24;
    plus 2^-120 absolute for values below the normal range.  Rows through the exact passes sum in float64 and are inside the same bound.
    Largest |error| / bound measured on an MI355X: see "Measured" at the end of docs/design/sim_topk.md;
  * fallback count: wide ladders: exactly the rows sim_cases.proven_flagged proves uncertifiable (the all-zero rows; for k >= 7 the rows
    whose k + 1 best share a half list - eight entries per list cannot certify those, docs/design/sim_topk.md) - no other row;
    narrow ladders / repeated name: at least the proven rows; dense: <= n // 20, with the seed chosen on the CPU so that the rows whose
    k-th logit lies within 2 E of a half list's last entry (every k) and whose ranks k, k + 1 lie within 2 E (k <= 5; `_dense` says why
    not beyond) are inside that cap;
  * a second call returns the same bits.

Dispatcher coverage (sim_topk_impl)
  RB8_GO<*, 4, 0> (k = 1)            test_planted_d512[*-1], test_dense_d512[*-1], test_large_n[*-1]
  RB8_GO<*, 8, 2> (k = 2, 3)         test_planted_d512[*-2|3], test_dense_d512[*-2|3]
  RB8_GO<*, 8, 4> (k = 5)            test_planted_d512[*-5], test_dense_d512[*-5]
  RB8_GO<*, 8, 7> (k = 6, 8)         test_planted_d512[*-6|8], test_dense_d512[*-6|8], test_large_n[*-8]
  (each of the above with SM = false and true: every test runs "raw" and "softmax")
  RC_GO<*, 3, 0>, RC_GO<*, 5, 2>     test_env_switch_child[rb16] (k = 1; 2, 3)
  unsplit launch                     [300-900-*] (28 units < 32), test_large_n[33100-*] (130 blocks in the last round), test_env_switch_child[nosplit]
  split launch + merge               [300-1031-*], [129-2017-*], [300-1055-*], [129-1024-*]
  mixed launch                       test_large_n[66000-*]
  sim_refine4_kernel                 every d = 512 test; sim_refine_kernel with ks >= 0: test_env_switch_child[refine]; with ks = -1: d != 512
  exact pass, chunks of 128 names    every narrow / zero-row case (<= 256 flagged rows), test_repeated_name[100-*]
  exact pass, one block per row      test_repeated_name[300-*] (300 flagged rows: 256 through the chunks, 44 one block each)
  d < 512 (sim_topk_kernel<*, 8>)    test_dense_small_d
  d = 768 (sim_topk_kernel<*, 4, 12>) test_planted_d768
  scale 1 / 1000                     test_scale
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sim_cases as sc
import sim_child
from oracle import naming_oracle as no

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [1, 2, 3, 5, 6, 8]
_worst = {}                          # input class -> largest softmax |error| / bound of this run (printed)


@pytest.fixture(scope="module")
def ops():
    from scd_amd import ops as o
    return o


def softmax_bound(f, w, scale, lg, exact=False):
    """Relative bound per row (module docstring); exact: the fp32 logits of this input are exact."""
    d, v = w.shape
    aw = np.abs(f.astype(np.float64)) @ np.abs(w.astype(np.float64))
    delta = 0.0 * aw.max(1) if exact else scale * (d + 2) * 2.0 ** -24 * aw.max(1)
    L = np.abs(lg).max(1)
    R = lg.max(1) - lg.min(1)
    big = np.minimum(delta, 600.0), np.minimum(2 * L * 2.0 ** -24, 600.0)           # beyond e^600 the bound says nothing; keep it finite
    return np.expm1(big[0]) + np.expm1(big[1]) + (2 * np.minimum(R * 1.4427, 150.0) + 8) * 2.0 ** -23 + (v / 2 + 16) * 2.0 ** -24


def check(ops, case, modes=("raw", "softmax"), argmax=True):
    """Runs the case, asserts everything but the fallback count; returns {mode: fallback count}, {mode: idx}."""
    f, w, k, scale = case.f, case.w, case.k, case.scale
    n, v = f.shape[0], w.shape[1]
    rows = sc.oracle_rows(n)
    fd = torch.from_numpy(f).cuda()
    wt = ops.transpose_f16(torch.from_numpy(w).cuda())
    lg = sc.logits64(f[rows], w, scale)
    fbs, idxs = {}, {}
    for mode in modes:
        idx, val, fb = ops.sim_topk(fd, wt, k, mode, scale=scale, return_fallback=True)
        idx2, val2, fb2 = ops.sim_topk(fd, wt, k, mode, scale=scale, return_fallback=True)
        assert torch.equal(idx, idx2) and torch.equal(val.view(torch.int32), val2.view(torch.int32)) and torch.equal(fb, fb2)
        assert int(((idx < 0) | (idx >= v)).sum().item()) == 0
        srt = idx.sort(dim=1).values
        assert k == 1 or int((srt[:, 1:] == srt[:, :-1]).sum().item()) == 0, "an index twice in a row"
        gi, gv = idx.cpu().numpy()[rows], val.cpu().numpy()[rows]
        oi, ov = no.sim_topk(f[rows], w, k, mode, scale)
        bad = np.nonzero((gi != oi).any(1))[0]
        assert bad.size == 0, (case.tag, mode, rows[bad[:5]], gi[bad[:5]], oi[bad[:5]], case.kind[rows[bad[:5]]])
        if mode == "raw":
            assert (np.abs(gv.astype(np.float64) - ov.astype(np.float64)) <= np.spacing(np.abs(ov)).astype(np.float64)).all()
        else:
            ref = np.exp(np.take_along_axis(lg, oi, 1) - lg.max(1, keepdims=True)) / np.exp(lg - lg.max(1, keepdims=True)).sum(1, keepdims=True)
            bound = softmax_bound(f[rows], w, scale, lg, exact=case.tag != "dense")[:, None] * ref + 2.0 ** -120
            assert np.isfinite(gv).all() and (gv >= 0).all()
            ratio = float((np.abs(gv - ref) / bound).max())
            _worst[case.tag] = max(_worst.get(case.tag, 0.0), ratio)
            print("softmax error / bound: %.4f (worst so far %s)" % (ratio, _worst))
            assert ratio <= 1.0, (case.tag, ratio)
        fbs[mode] = int(fb.item())
        idxs[mode] = idx
    if argmax:
        a, av = ops.sim_argmax(fd, wt, scale=scale)
        a2, av2 = ops.sim_argmax(fd, wt, scale=scale)
        assert torch.equal(a, a2) and torch.equal(av.view(torch.int32), av2.view(torch.int32))
        oa, oav = no.sim_argmax(f[rows], w, scale)
        top1 = no.sim_topk(f[rows], w, 1, "raw", scale)[0][:, 0]              # index ascending among equal maxima
        assert np.array_equal(a.cpu().numpy()[rows], top1)
        assert (np.abs(av.cpu().numpy()[rows].astype(np.float64) - oav) <= np.spacing(np.abs(oav))).all()
    print("fallback rows %s of %d (proven %d)" % (fbs, n, len(case.flagged or ())))
    return fbs, idxs


def check_fallback(case, fbs):
    n = case.f.shape[0]
    for mode, fb in fbs.items():
        if case.tag == "planted-wide":
            assert fb == len(case.flagged), (mode, fb, len(case.flagged))
        elif case.tag == "dense":
            assert fb <= n // 20
        else:
            assert len(case.flagged) <= fb <= n


@pytest.mark.parametrize("spacing", ["wide", "narrow"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n,v", [(300, 900), (300, 1031), (129, 2017), (300, 1055), (129, 1024)])
def test_planted_d512(ops, n, v, k, spacing):
    """Unsplit (V = 900) and split launches; V mod 32 = 4, 7, 1, 31, 0; n not a multiple of 256 (rows past n clamp to n - 1); zero rows,
    all-negative rows and rows scaled by 2^-8 .. 2^6 inside each block.  The same rows with every scale factor removed give the same
    indices."""
    case = sc.planted(n, v, 512, k, spacing, neg_rows=spacing == "narrow")[0]
    fbs, idxs = check(ops, case)
    check_fallback(case, fbs)
    lad = np.nonzero(case.kind == spacing)[0]
    f1 = case.f.astype(np.float64)
    f1[lad] *= 2.0 ** -case.rows_scale[lad][:, None]
    idx1, _ = ops.sim_topk(torch.from_numpy(f1.astype(np.float16)).cuda(), ops.transpose_f16(torch.from_numpy(case.w).cuda()), k, "raw")
    assert torch.equal(idx1[lad], idxs["raw"][lad])


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("spacing", ["wide", "narrow"])
def test_planted_d768(ops, k, spacing):
    case = sc.planted(129, 1031, 768, k, spacing, neg_rows=spacing == "narrow")[0]
    check_fallback(case, check(ops, case)[0])


@pytest.mark.parametrize("scale", [1.0, 1000.0])
@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("spacing", ["wide", "narrow"])
def test_scale(ops, scale, k, spacing):
    """The row-block kernel's thresholds are in unscaled units, the refine pass's in scaled ones: the ladders are built in units of E at
    the case's own scale."""
    case = sc.planted(300, 1031, 512, k, spacing, scale=scale, neg_rows=spacing == "narrow")[0]
    check_fallback(case, check(ops, case)[0])


_DENSE = {}


def _dense(n, v, d, k):
    """The first of twelve seeds whose CPU counts are inside the cap n // 20: rows whose ranks k, k + 1 lie within 2 E (the issue's
    precondition), and rows whose k-th logit is within 2 E of a half list's last entry (what the certificate compares).
    One exception, n > 4,096 at k = 8: 2 E is ~0.012 logit units against a mean gap of ~0.2 at rank 8 of 1,031 names, so ~6 % of
    Gaussian rows at d = 512 are close (123 of the 2,048 sampled rows of n = 66,000, seed 0), and over thousands of rows no seed moves
    that rate under 5 %.  There the close count is printed and only the second count is asserted; at every other shape both are."""
    rows = sc.oracle_rows(n)
    cap = (n // 20) * len(rows)
    rate_above_cap = n > 4096 and k == 8
    for seed in range(12):
        key = (n, v, d, seed)
        if key not in _DENSE:
            case = sc.dense(n, v, d, k, seed=seed)
            _DENSE[key] = (case, sc.logits64(case.f[rows], case.w, 100.0), sc.e_bound(case.f[rows], case.w, 100.0))
        case, lg, E = _DENSE[key]
        close, crowded = len(sc.close_rows(lg, E, k)), len(sc.crowded_rows(lg, E, k, 4 if (k == 1 and d == 512) else 8))
        if crowded * n <= cap and (rate_above_cap or close * n <= cap):
            break
    else:
        raise AssertionError("no seed among twelve keeps the close rows inside n // 20")
    print("dense n=%d v=%d d=%d k=%d seed=%d: rows with ranks k, k+1 within 2 E: %d of %d; k-th within 2 E of a list end: %d"
          % (n, v, d, k, seed, close, len(rows), crowded))
    sc.check_separated(lg, k, case.w)
    return case._replace(k=k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n,v", [(300, 900), (300, 1031), (129, 2017)])
def test_dense_d512(ops, n, v, k):
    case = _dense(n, v, 512, k)
    check_fallback(case, check(ops, case)[0])


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("n", [33100, 66000])
def test_large_n(ops, n, k):
    """n = 33,100: 130 row blocks, unsplit; n = 66,000: 256 whole blocks + 2 split ones (the mixed launch).  Dense rows, and the planted
    wide case of 300 rows repeated down the matrix (the oracle's answer repeats with it)."""
    case = _dense(n, 1031, 512, k)
    check_fallback(case, check(ops, case)[0])
    base = sc.planted(256, 1031, 512, k, "wide", neg_rows=False)[0]
    reps = -(-n // 256)
    big = base._replace(f=np.tile(base.f, (reps, 1))[:n], kind=np.tile(base.kind, reps)[:n])
    flagged = {i for i in range(n) if (i % 256) in base.flagged}
    big = big._replace(flagged=flagged)
    check_fallback(big, check(ops, big, argmax=False)[0])


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("n,v", [(257, 1031), (64, 37)])
@pytest.mark.parametrize("d", [64, 128, 192, 256, 320, 384, 448])
def test_dense_small_d(ops, d, n, v, k):
    case = _dense(n, v, d, k)
    check_fallback(case, check(ops, case)[0])


@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("n", [100, 300])
def test_repeated_name(ops, n, k):
    """Every row ties on every name: indices 0 .. k - 1, softmax 1 / V, every row through the exact pass (n = 300: both of its forms)."""
    case = sc.repeated_vocab(n, 1031, 512, k)
    fbs, idxs = check(ops, case)
    check_fallback(case, fbs)
    assert fbs["raw"] == n
    assert torch.equal(idxs["raw"].cpu(), torch.arange(k).expand(n, k))


def test_zero_rows_give_the_first_names_and_a_flat_softmax(ops):
    case = sc.planted(300, 1031, 512, 5, "wide")[0]
    z = np.nonzero(case.kind == "zero")[0]
    wt = ops.transpose_f16(torch.from_numpy(case.w).cuda())
    idx, val = ops.sim_topk(torch.from_numpy(case.f).cuda(), wt, 5, "softmax")
    assert torch.equal(idx[z].cpu(), torch.arange(5).expand(len(z), 5))
    assert np.allclose(val[z].cpu().numpy(), 1.0 / 1031, rtol=1e-6, atol=0)


_DEFAULT = {}


@pytest.mark.parametrize("name,env,ks", [("rb16", {"SCD_SIM_RB": "16"}, [1, 2, 3]), ("refine", {"SCD_SIM_REFINE4": "0"}, [1, 3, 5, 8]),
                                         ("nosplit", {"SCD_SIM_SPLIT": "0"}, [1, 3, 8])], ids=["rb16", "refine", "nosplit"])
def test_env_switch_child(ops, tmp_path, name, env, ks):
    """sim_topk_rc_kernel (16x16x32 tiles, k <= 3), sim_refine_kernel at d = 512 and the unsplit launch where the default splits, each in a
    fresh child process (the library reads the switches once): planted wide / narrow and the repeated name, d = 512, n = 300, V = 1,031.
    Indices equal the oracle's and the default library's, values obey the same bounds."""
    out = str(tmp_path / "child.npz")
    e = dict(os.environ, **env)
    e.pop("SCD_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sim_child.py"), out] + [str(k) for k in ks], env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stderr[-2000:]
    got = np.load(out)
    want_path = {"rb16": ops.SIM_PATH_RC16 | ops.SIM_PATH_REFINE4, "refine": ops.SIM_PATH_RB8 | ops.SIM_PATH_SPLIT,
                 "nosplit": ops.SIM_PATH_RB8 | ops.SIM_PATH_REFINE4}[name]
    for k in ks:
        if k not in _DEFAULT:
            _DEFAULT[k] = sim_child.run_cases(ops, [k])
        for cname, c in sim_child.cases(k).items():
            lg = sc.logits64(c.f, c.w, c.scale)
            for mode in ("raw", "softmax"):
                key = "%s_%s_" % (cname, mode)
                # the switched kernels ran in the child, the default ones here (scd_sim_last_path)
                assert int(got[key + "path"]) == want_path, (name, key, int(got[key + "path"]))
                assert int(_DEFAULT[k][key + "path"]) == ops.SIM_PATH_RB8 | ops.SIM_PATH_SPLIT | ops.SIM_PATH_REFINE4
                oi, ov = no.sim_topk(c.f, c.w, k, mode, c.scale)
                assert np.array_equal(got[key + "idx"], oi), (name, key)
                assert np.array_equal(got[key + "idx"], _DEFAULT[k][key + "idx"])
                if mode == "raw":
                    assert (np.abs(got[key + "val"].astype(np.float64) - ov) <= np.spacing(np.abs(ov))).all()
                else:
                    ref = np.exp(np.take_along_axis(lg, oi, 1) - lg.max(1, keepdims=True)) / np.exp(lg - lg.max(1, keepdims=True)).sum(1, keepdims=True)
                    assert (np.abs(got[key + "val"] - ref) <= softmax_bound(c.f, c.w, c.scale, lg, exact=True)[:, None] * ref + 2.0 ** -120).all()
                fb = int(got[key + "fb"])
                print(name, key, "fallback rows", fb, "default", int(_DEFAULT[k][key + "fb"]))
                # wide ladders: exactly the proven rows on every path.  The half-list proof carries over to the quarter lists of the
                # 16x16x32 kernel at k <= 3: a list holds k + 2 entries, so the k + 2 planted names fit into any one list and everything
                # outside the candidates is at or below the ladder's last rung, >= 32 E under the k-th value; the zero rows tie everywhere
                check_fallback(c, {mode: fb})
                if name == "refine":                                # same lists, same decisions as sim_refine4_kernel
                    assert fb == int(_DEFAULT[k][key + "fb"])
