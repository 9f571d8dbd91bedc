"""Would tests/test_gpu_gemm.py see the faults its kernels could have?  CPU only: each fault is applied to the float64 restatement
(oracle/clip_oracle.py) and the result is held against the per-element budgets (tests/gemm_cases.py) on the real-valued inputs of
section B, and against bit equality on the integer inputs of section A.

FACTOR: on the real-valued inputs every fault must exceed the budget on at least one element by FACTOR = 1000.  The test prints the
margins (pytest -s); at the committed seeds the smallest is 5,063 budgets (one statistics partial missing, QuickGELU epilogue), then
5,988 (a chunk dropped in the folded form); every fault of the plain GEMM is further out.  FACTOR_ILL = 50 is the same requirement
on the rows with mean / sigma = 100 and on the constant rows ALONE (conditioning 1e4 and 2.5e4), where a budget that grew with the
conditioning of the two cancelling terms would see nothing: smallest margins 74.8 (constant rows, one statistics partial missing) and
108.6 (mean-100 rows, the same fault).  An input set on which any fault stays inside these factors is to be replaced, not excused.
"""
import numpy as np
import pytest

import gemm_cases as gc
from oracle import clip_oracle as co

FACTOR = 1000.0
FACTOR_ILL = 50.0

M, N, K, EPS = 512, 768, 768, 1e-5
TILE = (slice(256, 512), slice(256, 512))     # block tile (bm 1, bn 1)
WAVE = (slice(256, 384), slice(384, 512))     # wave (wm 0, wn 1) of that tile


def _chunk(a, w, kc, sign):
    """one 64-deep chunk of one tile dropped (sign -1) or doubled (+1)"""
    d = np.zeros((a.shape[0], w.shape[0]))
    ks = slice(64 * kc, 64 * kc + 64)
    d[TILE] = sign * (a[TILE[0], ks].astype(np.float64) @ w[TILE[1], ks].astype(np.float64).T)
    return d


def _swap_mtiles(c):
    """two 16-row m-tiles of a wave swapped"""
    c = c.copy()
    r0, cols = WAVE[0].start + 32, WAVE[1]
    c[r0:r0 + 16, cols], c[r0 + 16:r0 + 32, cols] = c[r0 + 16:r0 + 32, cols].copy(), c[r0:r0 + 16, cols].copy()
    return c


def _stale_residual(c, pre_res, res):
    """the residual of one wave's rows read after another wave's in-place store: those rows add C of the other rows, not R"""
    c = c.copy()
    rows, other, cols = slice(256, 384), slice(384, 512), WAVE[1]
    c[rows, cols] = pre_res[rows, cols] + c[other, cols]
    return c


def _plain_faults(a, w, bias, res, act):
    pre = co.gemm_f64(a, w, bias, 0, None)
    full = lambda p: co.act_f64(p, act) + (0 if res is None else res.astype(np.float64))
    out = {"chunk dropped": full(pre + _chunk(a, w, 5, -1)), "chunk doubled": full(pre + _chunk(a, w, 0, +1)),
           "m-tiles swapped": _swap_mtiles(full(pre))}
    if res is not None:
        out["stale residual"] = _stale_residual(full(pre), co.act_f64(pre, act), res)
    return out


def _folded(a, wf, bf, cs, stats, act, rs_shift=0, no_colsum=False, acc_delta=None):
    mean, ex2 = co.stats_moments(stats, a.shape[1])
    rstd = 1.0 / np.sqrt(np.maximum(ex2 - mean * mean, 0.0) + EPS)
    nmr = -mean * rstd
    if rs_shift:
        rows = np.arange(WAVE[0].start, WAVE[0].stop)
        rstd, nmr = rstd.copy(), nmr.copy()
        rstd[rows], nmr[rows] = rstd[rows + rs_shift], nmr[rows + rs_shift]
    acc = a.astype(np.float64) @ wf.astype(np.float64).T
    if acc_delta is not None:
        acc = acc + acc_delta
    pre = rstd[:, None] * acc + (0 if no_colsum else nmr[:, None] * cs.astype(np.float64)[None, :]) + bf.astype(np.float64)[None, :]
    return co.act_f64(pre, act)


def _stats_partial(c16, row_block, sign):
    """row statistics with one 128-column partial of some rows missing (sign -1) or counted twice (+1)"""
    st = co.row_stats_int(c16)
    part = co.row_stats_int(c16[row_block, 128:256])
    st[row_block] += sign * part
    return st


def _worst(faulty, ref, bnd):
    return float((np.abs(faulty - ref) / bnd).max())


def test_real_valued_faults_exceed_the_budget():
    margins, ill = {}, {}
    rs = np.random.RandomState(M + N + K)
    a, kind = gc.real_rows(M, K, seed=M + K)
    w = gc.f16(rs.randn(N, K) * K ** -0.5)
    bias = rs.randn(N).astype(np.float32)
    res = gc.f16(rs.randn(M, N) * 2.0 ** rs.randint(-6, 3, size=(M, 1)))
    for act, r in ((0, None), (1, None), (2, None), (0, res)):
        ref, bnd = co.gemm_f64(a, w, bias, act, r), gc.budget_plain(a, w, bias, act, r)
        for name, f in _plain_faults(a, w, bias, r, act).items():
            margins["plain act %d res %d: %s" % (act, r is not None, name)] = _worst(f, ref, bnd)
    # folded form, against the folded and the true budget
    w, gamma, beta, b = gc.real_layer(N, K, seed=N + K)
    wf, cs, bf = gc.fold_host(w, gamma, beta, b)
    stats = co.row_stats_int(a)
    for act in (0, 1, 2):
        ref, parts = co.gemm_ln_folded_f64(a, wf, bf, cs, stats, EPS, act)
        b_true = gc.budget_true(a, w, gamma, beta, b, wf, bf, cs, parts, EPS, act)
        bnd = np.maximum(gc.budget_folded(a, wf, bf, cs, parts, EPS, act), b_true)
        faults = {"chunk dropped": _folded(a, wf, bf, cs, stats, act, acc_delta=_chunk(a, wf, 3, -1)),
                  "chunk doubled": _folded(a, wf, bf, cs, stats, act, acc_delta=_chunk(a, wf, 11, +1)),
                  "m-tiles swapped": _swap_mtiles(ref), "rs of row m + 16": _folded(a, wf, bf, cs, stats, act, rs_shift=16),
                  "rs of row m - 16": _folded(a, wf, bf, cs, stats, act, rs_shift=-16), "no colsum": _folded(a, wf, bf, cs, stats, act, no_colsum=True),
                  "stats partial missing": _folded(a, wf, bf, cs, _stats_partial(a, WAVE[0], -1), act),
                  "stats partial doubled": _folded(a, wf, bf, cs, _stats_partial(a, WAVE[0], +1), act)}
        for name, f in faults.items():
            margins["folded act %d: %s" % (act, name)] = _worst(f, ref, bnd)
            for i in (4, 5):           # the ill-conditioned rows on their own: the budget must not have grown with their conditioning
                ill["%s rows, folded act %d: %s" % (gc.ROW_KINDS[i], act, name)] = _worst(f[kind == i], ref[kind == i], bnd[kind == i])
    # half a patch row from the neighbouring patch, Gaussian pixels
    px = gc.f16(np.random.RandomState(5).randn(3, 3, 224, 224))
    wp = gc.f16(np.random.RandomState(6).randn(N, 768) * 768 ** -0.5)
    cols = co.im2col(px)
    bad = cols.copy().reshape(-1, 3, 16, 16)
    bad[256:384, 1, 7, 8:] = bad[257:385, 1, 7, 8:]
    margins["img: half patch row"] = _worst(bad.reshape(-1, 768) @ wp.astype(np.float64).T, co.patch_conv_f64(px, wp),
                                            gc.budget_plain(cols, wp))
    weakest = min(margins, key=margins.get)
    print("smallest margin: %s, %.1f budgets" % (weakest, margins[weakest]))
    for name, v in sorted(margins.items(), key=lambda kv: kv[1])[:6]:
        print("  %-50s %10.1f" % (name, v))
    under = {k: v for k, v in margins.items() if v < FACTOR}
    assert not under, under
    for name, v in sorted(ill.items(), key=lambda kv: kv[1])[:8]:
        print("  %-60s %10.1f" % (name, v))
    under = {k: v for k, v in ill.items() if v < FACTOR_ILL}
    assert not under, under


def test_exact_faults_change_bits():
    a, w, bias, res = gc.exact_operands(M, N, K, seed=M + 3 * N + 7 * K)
    for r in (None, res):
        ref = co.gemm_f64(a, w, bias, 0, r)
        for name, f in _plain_faults(a, w, bias, r, 0).items():
            assert not np.array_equal(f.astype(np.float16), ref.astype(np.float16)), name
    # LN = 2 statistics of the exact outputs
    a, w, bias, res = gc.exact_operands(M, N, K, seed=11 * M + N + K, w_max=1, a_density=0.25)
    c = co.gemm_f64(a, w, bias, 0, res).astype(np.float16)
    want = co.row_stats_int(c)
    for sign in (-1, 1):
        got = _stats_partial(c, WAVE[0], sign)
        assert (got[WAVE[0]] != want[WAVE[0]]).any(1).all(), sign       # every affected row, both words or one
    # LN = 1 with integer statistics: {rstd, nmr} of row m +- 16, and the colsum term
    colsum = w.astype(np.float64).sum(1)
    scale = np.where(np.arange(M) % 3 == 0, 2.0, 1.0)
    acc = a.astype(np.float64) @ w.astype(np.float64).T
    mean = np.where(np.arange(M) % 3 == 2, 1.0, 0.0)
    ref = scale[:, None] * acc - mean[:, None] * colsum[None, :] + bias
    for shift in (16, -16):
        s2, m2 = scale.copy(), mean.copy()
        rows = np.arange(WAVE[0].start, WAVE[0].stop)
        s2[rows], m2[rows] = scale[rows + shift], mean[rows + shift]
        assert not np.array_equal((s2[:, None] * acc - m2[:, None] * colsum[None, :] + bias).astype(np.float16), ref.astype(np.float16)), shift
    assert not np.array_equal((scale[:, None] * acc + bias).astype(np.float16), ref.astype(np.float16))       # colsum term omitted
    # half a patch row from the neighbouring patch
    px, wp = gc.img_pixels(3, 224, seed=224 + 3 + N), gc.img_weights(N)
    cols = co.im2col(px)
    bad = cols.copy().reshape(-1, 3, 16, 16)
    bad[256:384, 1, 7, 8:] = bad[257:385, 1, 7, 8:]
    good = cols @ wp.astype(np.float64).T
    moved = (bad.reshape(-1, 768) @ wp.astype(np.float64).T != good).any(1)
    assert moved[256:384].mean() > 0.9 and not moved[:256].any()


def test_exact_seeds_meet_their_conditions():
    """the committed seeds of section A (host-generated shapes) keep max |c| <= 2048 (<= 256 for the statistics) and every partial
    sum below 2^24: checked here without a GPU for the deepest shapes"""
    for m, n, k in ((256, 1024, 4096), (256, 768, 3072), (512, 1152, 1024)):
        a, w, bias, res = gc.exact_operands(m, n, k, seed=m + 3 * n + 7 * k)
        mag = np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64)).T + np.abs(bias) + np.abs(res.astype(np.float64))
        gc.assert_exact_conditions(co.gemm_f64(a, w, bias, 0, res), mag)
    for m, n, k in ((768, 768, 3072), (1280, 1024, 4096)):
        a, w, bias, res = gc.exact_operands(m, n, k, seed=11 * m + n + k, w_max=1, a_density=0.25)
        mag = np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64)).T + np.abs(bias) + np.abs(res.astype(np.float64))
        gc.assert_exact_conditions(co.gemm_f64(a, w, bias, 0, res), mag, cap=256)
