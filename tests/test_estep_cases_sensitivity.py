"""Can the inputs of tests/estep_cases.py tell a wrong E-step filter from a right one?  A small numpy model of the DOCUMENTED data flow of
scd_kmeans_estep (float64 mean; power-of-two scale from max |x - mu|; x', c' rounded to fp16; ||c'||^2 in float64 rounded to float32;
products accumulated in float32; per path the key truncation - 7 index bits on the streaming paths, 11 on the single-pass path - and the
hi + lo norm of the single-pass path; the three best centres; the decision m1 - m0 > 2 E with that path's A, B; exact re-evaluation of the
flagged rows from the pair or from all centres; a live centre outside the filter's range sends every row to all centres) is run on
every case and judged by the assertions tests/test_gpu_estep_bounds.py uses (`check_labels`).

The correct model passes every case.  Each planted failure fails at least one case (CATCHES below names one per failure; the test
asserts exactly those):
  bound / 64                        long_centres[700,768,128]            (near-ties of long centres go undetected at E / 64)
  subnormal term dropped            subnormal_tie[333,896,2,1,U100], subnormal_tie[333,64,2,0,U4], subnormal_tie[700,768,128,1,U4]
                                    (the bulk's x' is a few subnormal quanta long, the two tied centres are opposite: the rounding of
                                    x' separates their scores by ~1e-9..5e-11 while the rest of E is below that - the filter decides
                                    the tie for the higher index; estep_cases.subnormal_tie has the arithmetic)
  key term dropped                  long_centres[520,512,2048,q8,W3] (rb, 11 index bits), long_centres[700,768,128,q1,W0] (stream1),
                                    long_centres[700,640,300,q1,W0] (streamN): two scores that agree above the index bits show a
                                    margin of up to 2^-12 (2^-16) of the score once the indices are OR-ed in; with rows close to the
                                    mean E is mostly the key term of B, and without it that margin passes for a decision
  tie to the higher index           ladder[333,64,8]                     (its t = 0 rows)
  pair list with the third inside   ladder[700,768,128]                  (three-way near-ties whose winner the filter ranks third)
  cmax without dead-centre exclusion  ladder[333,64,8]                   (padding centres carry +inf: E = inf, every row flagged)
  no overflow handling for c'       outside_box[420,256,129,far]         (fp16 infinities in c')
The model is not the kernel: it sums in numpy's order, not the MFMA's.  What is asserted on the device is asserted there on the device's
own output.
"""
import numpy as np
import pytest

import estep_cases as ec
from oracle import kmeans_oracle as ko

F32 = np.float32
STRADDLE = ("ladder", "long_centres", "same_sign")          # families that must have rows on both sides of the bound


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _f16(v64):
    with np.errstate(over="ignore", invalid="ignore"):
        return v64.astype(F32).astype(np.float16)          # the kernels convert double -> float -> half


def bound(path_, dp, cmax, xn, mut=()):
    """E = A ||x'|| + B of the path (kmeans.hip: estep_mfma_kernel, estep_stream_kernel, erb_decide), float32 like the kernels."""
    cmax, sq = F32(cmax), F32(np.sqrt(F32(dp)))
    sub = F32(0.0) if "no_subnormal" in mut else F32(6.0e-8)
    keyA, keyB, normB = {"legacy": (0.0, 0.0, 2.4e-7), "stream1": (3.06e-5, 1.53e-5, 2.4e-7), "streamN": (3.06e-5, 1.53e-5, 2.4e-7),
                         "rb": (4.9e-4, 2.45e-4, 4.8e-7)}[path_]
    if "no_key" in mut:
        keyA = keyB = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        A = F32(1.5) * (F32(2.02) * (F32(9.765625e-4) + F32(dp) * F32(5.9604645e-8)) * cmax + F32(4.8e-7) * cmax + sub * sq + F32(keyA) * cmax)
        B = F32(1.5) * (sub * sq * cmax + F32(normB) * cmax * cmax + F32(keyB) * cmax * cmax)
        E = (A * xn.astype(F32) + B).astype(F32)
    return E / F32(64.0) if "div64" in mut else E


def model(case, mut=()):
    """-> (labels int64 [n], refined rows int, flagged bool [n])."""
    x, c, p = case.x, case.c, case.path
    n, d = x.shape
    k = c.shape[0]
    dp, kp = (d + 127) // 128 * 128, (k + 127) // 128 * 128
    x64 = x.astype(np.float64)
    mu = x64.mean(axis=0)
    maxabs = F32(np.abs((x64 - mu).astype(F32)).max())
    e = 4 - int(np.frexp(maxabs)[1]) if maxabs > 0 and np.isfinite(maxabs) else 0
    sc = 2.0 ** e
    xp = (x64 - mu) * sc
    xn = np.sqrt((xp * xp).sum(1)).astype(F32)
    xh = _f16(xp).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        cp = (c.astype(np.float64) - mu) * sc
        t = (cp * cp).sum(1)
    dead = ~np.isfinite(c).all(axis=1)
    wild = ~dead & ((np.abs(cp) > 65504.0).any(axis=1) | ((t > 300.0 * dp) & (dp == 512 and kp <= 2048)))
    if "no_overflow" in mut:
        wild[:] = False
    ch = _f16(np.where((dead | wild)[:, None], 0.0, cp)).astype(F32)
    with np.errstate(over="ignore"):
        cn = np.where(dead, np.inf, t).astype(F32)
    live = ~(dead | wild)
    cn_f = np.concatenate([np.where(live, cn, F32(np.inf)), np.full(kp - k, np.inf, dtype=F32)])     # filter view: padded, dead = +inf
    if "cmax_dead" in mut:
        cmax = F32(np.sqrt(cn_f.max(initial=0)))
    else:
        cmax = F32(np.sqrt(cn[live].astype(np.float64).max(initial=0.0))) * F32(1.0000002)
    chp = np.concatenate([ch, np.zeros((kp - k, d), dtype=F32)])
    with np.errstate(invalid="ignore", over="ignore"):
        acc = (xh @ chp.T).astype(F32)                                      # float32 accumulation
        idx = np.arange(kp, dtype=np.uint32)[None, :]
        if p == "legacy":
            s = (cn_f[None, :] - F32(2.0) * acc).astype(F32)
            order = np.argsort(s, axis=1, kind="stable")[:, :3]             # (value, centre) ascending; NaN last
            m = np.take_along_axis(s, order, 1)
        elif p in ("stream1", "streamN"):
            s = (np.minimum(cn_f, F32(3.0e38)).astype(np.float64)[None, :] - 2.0 * acc.astype(np.float64)).astype(F32)      # one fma
            key = ((_bits(s) & np.uint32(0xFFFFFF80)) | (idx & np.uint32(127))).view(F32)
            order = np.argsort(key, axis=1, kind="stable")[:, :3]           # ties between chunks keep the earlier chunk
            m = np.take_along_axis(key, order, 1)
        else:
            hv = np.where(cn_f < F32(3.0e38), F32(0.125) * cn_f, F32(60000.0)).astype(F32)
            hi = hv.astype(np.float16)
            lo = (hv - hi.astype(F32)).astype(np.float16)
            a = (acc.astype(np.float64) - 4.0 * (hi.astype(np.float64) + lo.astype(np.float64))[None, :]).astype(F32)
            key = ((_bits(a) & np.uint32(0xFFFFF800)) | idx).view(F32)
            order = np.argsort(-key, axis=1, kind="stable")[:, :3]          # the three LARGEST keys
            m = (F32(-2.0) * np.take_along_axis(key, order, 1)).astype(F32)
        E = bound(p, dp, cmax, xn, mut)
        m0, m1, m2 = m[:, 0], m[:, 1], m[:, 2]
        flagged = ~(m1 - m0 > F32(2.0) * E)
        pair = flagged & (m2 - m0 > F32(2.0) * E)
    if "pair_always" in mut:
        pair = flagged.copy()
    if wild.any():
        flagged[:] = True
        pair[:] = False
    labels = order[:, 0].astype(np.int64)
    dist = ec.exact_dist(np.nan_to_num(x64), np.nan_to_num(c.astype(np.float64)))     # exact on the grid (any common power of two)
    dist[:, dead] = np.inf
    for r in np.nonzero(flagged)[0]:
        cand = np.sort(order[r, :2]) if pair[r] else np.arange(k)
        cand = cand[cand < k]
        dd = dist[r, cand]
        if "tie_high" in mut:
            labels[r] = cand[len(dd) - 1 - np.argmin(dd[::-1])]
        else:
            labels[r] = cand[np.argmin(dd)]
    return labels, int(flagged.sum()), flagged


_oracle = {}


def oracle(case):
    if case.name not in _oracle:
        lab, mind, _ = ko.estep(case.x, case.c)
        _oracle[case.name] = (lab, mind)
    return _oracle[case.name]


def check_labels(case, labels, refined, both_sides):
    """The assertions of test_gpu_estep_bounds on one E-step result (labels of EVERY row; the refined count where both outcomes occur)."""
    olab, _ = oracle(case)
    labels = np.asarray(labels).astype(np.int64)
    bad = np.nonzero(labels != olab)[0]
    assert bad.size == 0, "%s: %d rows differ from the float64 argmin, first %s" % (case.name, bad.size, bad[:5])
    if both_sides:
        assert 0 < refined < len(olab), (case.name, refined)
    if case.ties.size:                                           # (implied by the first assertion; spelled out: the lower index)
        d = ec.exact_dist(case.x.astype(np.float64), np.nan_to_num(case.c.astype(np.float64)))
        d[:, np.isnan(case.c).any(axis=1)] = np.inf
        assert np.array_equal(labels[case.ties], np.argmin(d[case.ties], axis=1))


ALL_CASES = ec.estep_cases() + ec.outside_box_cases()
_model = {}


def correct(case):
    if case.name not in _model:
        _model[case.name] = model(case)
    return _model[case.name]


def both_sides(case):
    """Does the (correct) model both decide rows without refine and flag rows?  The GPU test asserts 0 < refined < n where it does."""
    _, refined, _ = correct(case)
    return 0 < refined < case.x.shape[0]


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_correct_model_passes(case):
    labels, refined, flagged = correct(case)
    check_labels(case, labels, refined, both_sides(case))
    assert flagged[case.ties].all(), "an exact tie was decided by the filter"
    if case.family in STRADDLE:
        assert 0 < refined < case.x.shape[0], "%s does not straddle the bound: %d of %d flagged" % (case.name, refined, case.x.shape[0])


def family_counts():
    """family -> (cases, rows, rows the model flags), summed over the family's cases."""
    out = {}
    for case in ALL_CASES:
        f = out.setdefault(case.family, [0, 0, 0])
        f[0] += 1
        f[1] += case.x.shape[0]
        f[2] += correct(case)[1]
    return {k: tuple(v) for k, v in out.items()}


RECORDED = {           # the table in test_gpu_estep_bounds.py's docstring
    "ladder": (11, 6859, 6168), "long_centres": (13, 6679, 3584), "subnormal_tie": (6, 2732, 2724), "same_sign": (4, 2240, 1120),
    "outlier_scale": (16, 8445, 8445), "offset": (7, 3706, 3485), "degenerate": (10, 3758, 1606), "outside_box": (12, 4838, 4838),
}


def test_model_counts_are_the_recorded_ones():
    assert family_counts() == RECORDED


CATCHES = [
    ("div64", "long_centres[700,768,128]"),
    ("no_subnormal", "subnormal_tie[333,896,2,1,U100]"),
    ("no_subnormal", "subnormal_tie[333,64,2,0,U4]"),
    ("no_subnormal", "subnormal_tie[700,768,128,1,U4]"),
    ("no_key", "long_centres[520,512,2048,q8,W3]"),
    ("no_key", "long_centres[700,768,128,q1,W0]"),
    ("no_key", "long_centres[700,640,300,q1,W0]"),
    ("tie_high", "ladder[333,64,8]"),
    ("pair_always", "ladder[700,768,128]"),
    ("cmax_dead", "ladder[333,64,8]"),
    ("no_overflow", "outside_box[420,256,129,far]"),
]


@pytest.mark.parametrize("mut,name", CATCHES)
def test_planted_failure_is_caught(mut, name):
    case = ec.by_name(name)
    labels, refined, _ = model(case, mut=(mut,))
    with pytest.raises(AssertionError):
        check_labels(case, labels, refined, both_sides(case))
