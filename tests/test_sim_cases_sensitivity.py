"""Can the inputs of tests/sim_cases.py tell a wrong similarity kernel from a right one?  A small numpy model of the documented data flow
of the d = 512 path (per vocabulary part and half list the TM best by truncated key with the second-key admission and the shared
threshold; the merge of the two parts; the refine of the candidates within 2 E; the certificate; the exact pass) is run on the builders'
cases and judged by the assertions of tests/test_gpu_sim.py (indices equal the oracle's, in range and distinct; softmax inside the derived
bound; the fallback-count rules).  The correct model passes all of them; each planted failure fails at least one case.

Failure 6 (the shared threshold off by the factor `scale`) is the exception, and the test pins that down instead of hiding it: the
threshold only decides what is listed, and a value it drops lies below KS + 1 >= k listed approximate values of the other half.  Where the
fp32 logits are exact (every planted case) and wherever they are off by less than the misplaced margin, the dropped name cannot be
among the k best, so neither an index nor a count moves - at scale > 1 the margin only grows.  The model with failure 6 passes the planted
cases at scale 1/64; on the device that failure would show as a slower kernel or, on dense data, as a rare wrong index.
"""
import numpy as np
import pytest

import sim_cases as sc
from oracle import naming_oracle as no
from test_gpu_sim import check_fallback, softmax_bound

N, V, D = 24, 1031, 512


def _trunc_key(a, i):
    return ((np.float32(a).view(np.uint32) & np.uint32(0xFFFFFFF0)) | np.uint32(i)).view(np.float32)


def _order(key, idx):
    return (float(key), idx if key >= 0 else -idx)                  # the name index rides in the low mantissa word of a double


def _part_lists(a, v_lo, v_hi, v_all, tm, ks, e4, mut):
    """Half lists [(key, local name)] of one vocabulary part, unit by unit."""
    v = v_hi - v_lo
    L, tsh = {0: [], 1: []}, {0: -np.inf, 1: -np.inf}
    for u in range((v + 31) // 32):
        for h in (0, 1):
            keys = []
            for i in range(16):
                name = u * 32 + (i & 3) + 8 * (i >> 2) + 4 * h
                if name < v:
                    keys.append((_trunc_key(a[v_lo + name], i), name))
                elif mut == 1:
                    keys.append((_trunc_key(a[v_hi - 1], i), name))   # the padded rows are copies of row v - 1, unmasked
            keys.sort(key=lambda t: -t[0])
            for j, (kk, name) in enumerate(keys):
                thr = L[h][tm - 1][0] if len(L[h]) >= tm else -np.inf
                if j > 0 and not kk > max(thr, tsh[h]):
                    break
                if j >= 2 and mut == 5:
                    break                                           # the second-key path forgets the third value of a unit
                L[h] = sorted(L[h] + [(kk, name)], key=lambda t: _order(*t), reverse=True)[:tm]
        if u % 2 == 1:
            for h in (0, 1):
                o = L[1 - h]
                tsh[h] = (o[ks][0] - e4) if len(o) > ks else -np.inf
    return L


def model(case, mode, split=True, mut=0):
    f, w, k, scale = case.f, case.w, case.k, case.scale
    n, v = f.shape[0], w.shape[1]
    tm, ks = (4, 0) if k == 1 else (8, 2) if k <= 3 else (8, 4) if k <= 5 else (8, 7)
    lg = sc.logits64(f, w, scale)
    E = sc.e_bound(f, w, scale)
    oi, _ = no.sim_topk(f, w, k, "raw", scale)
    vs = sc.vsplit_of(v)
    parts = [(0, vs), (vs, v)] if split else [(0, v)]
    idx = np.zeros((n, k), np.int64)
    val = np.zeros((n, k))
    fb = 0
    for r in range(n):
        a = (lg[r] / scale).astype(np.float32)
        e4 = 4.2 * (E[r] if mut == 6 else E[r] / scale)
        half = {0: [], 1: []}
        for p, (lo, hi) in enumerate(parts):
            L = _part_lists(a, lo, hi, v, tm, ks, e4, mut)
            for h in (0, 1):
                half[h] += [(np.float32(kk) * np.float32(scale), nm + (0 if (mut == 2 and p == 1) else lo)) for kk, nm in L[h]]
        for h in (0, 1):
            half[h] = sorted(half[h], key=lambda t: (-t[0], t[1]))[:tm]
        cands = half[0] + half[1]
        ca = sorted((t[0] for t in cands), reverse=True)
        kap = ca[k - 1] if len(ca) >= k else -np.inf
        need = [(lg[r, min(nm, v - 1)], nm) for cv, nm in cands if cv >= kap - 2 * E[r]]
        tie = -1 if mut == 3 else 1
        need.sort(key=lambda t: (-t[0], tie * t[1]))
        astar = max([half[h][tm - 1][0] for h in (0, 1) if len(half[h]) >= tm], default=-np.inf)
        sh = [half[h][ks][0] for h in (0, 1) if len(half[h]) > ks]
        if sh:
            astar = max(astar, max(sh) - (0.0 if mut == 4 else 3.9 * E[r]))
        certified = astar == -np.inf or (len(need) >= k and need[k - 1][0] > astar + E[r])
        if certified:
            idx[r] = [nm for _, nm in need[:k]]
            ev = np.array([e for e, _ in need[:k]])
        else:
            fb += 1
            idx[r] = oi[r] if mut != 3 else sorted(range(v), key=lambda j: (-lg[r, j], -j))[:k]
            ev = lg[r, idx[r]]
        if mode == "softmax":
            use = lg[r, :vs] if (mut == 7 and split and certified) else lg[r]        # one part's (max, sum) pair lost in the merge
            with np.errstate(over="ignore"):
                val[r] = np.exp(ev - use.max()) / np.exp(use - use.max()).sum()
        else:
            val[r] = ev
    return idx, val, fb


def judge(case, mode, idx, val, fb):
    """The assertions of test_gpu_sim.check / check_fallback on a result."""
    f, w, k, scale = case.f, case.w, case.k, case.scale
    v = w.shape[1]
    assert ((idx >= 0) & (idx < v)).all()
    assert all(len(set(row)) == k for row in idx.tolist())
    oi, ov = no.sim_topk(f, w, k, mode, scale)
    assert np.array_equal(idx, oi)
    lg = sc.logits64(f, w, scale)
    if mode == "softmax":
        ref = np.exp(np.take_along_axis(lg, oi, 1) - lg.max(1, keepdims=True)) / np.exp(lg - lg.max(1, keepdims=True)).sum(1, keepdims=True)
        assert (np.abs(val - ref) <= softmax_bound(f, w, scale, lg, exact=True)[:, None] * ref + 2.0 ** -120).all()
    else:
        assert (np.abs(val - ov) <= np.spacing(np.abs(ov))).all()
    check_fallback(case, {mode: fb})


_CASES = {}


def cases():
    if not _CASES:
        for k in (3, 8):
            for spacing in ("wide", "narrow"):
                _CASES["%s-k%d" % (spacing, k)] = sc.planted(N, V, D, k, spacing, neg_rows=spacing == "narrow")[0]
        _CASES["wide-k3-scale1/64"] = sc.planted(N, V, D, 3, "wide", scale=2.0 ** -6, neg_rows=False)[0]
        _CASES["narrow-k3-scale1/64"] = sc.planted(N, V, D, 3, "narrow", scale=2.0 ** -6)[0]
        _CASES["repeat-k3"] = sc.repeated_vocab(12, V, D, 3)
    return _CASES


def fails(case, mode, mut):
    try:
        judge(case, mode, *model(case, mode, mut=mut))
    except AssertionError:
        return True
    return False


def test_the_correct_model_passes_every_case():
    for name, c in cases().items():
        for mode in ("raw", "softmax"):
            judge(c, mode, *model(c, mode))
    c = cases()["wide-k3"]
    judge(c, "raw", *model(c, "raw", split=False))


@pytest.mark.parametrize("mut,mode,what", [
    (1, "raw", "padded names not masked"),
    (2, "raw", "index offset of the second vocabulary half dropped"),
    (3, "raw", "ties resolved higher index first"),
    (4, "raw", "certificate without the - 3.9 E"),
    (5, "raw", "second-key path drops a unit's third value"),
    (7, "softmax", "softmax statistics of one half ignored in the merge"),
])
def test_each_planted_failure_fails_some_case(mut, mode, what):
    hit = next((name for name, c in cases().items() if fails(c, mode, mut)), None)
    print(what, "-> first failing case:", hit)
    assert hit is not None, what


def test_a_threshold_off_by_the_scale_factor_moves_no_index_on_exact_logits():
    """Failure 6, see the module docstring: at scale 1/64 the margin is 64 times too small and still nothing the assertions see changes."""
    for name in ("wide-k3-scale1/64", "narrow-k3-scale1/64"):
        c = cases()[name]
        good, bad = model(c, "raw"), model(c, "raw", mut=6)
        judge(c, "raw", *bad)
        assert np.array_equal(good[0], bad[0])
