"""Inputs for the similarity top-k tests (tests/test_gpu_sim.py on the device, tests/test_sim_cases_sensitivity.py on a numpy model of the
kernels' data flow).  Every value is an fp16 number; every builder checks its own preconditions in float64 and returns a `Case`.

Units.  E(row) = 1.5 * scale * (d * 2^-24 + 2.24e-6) * ||f|| * max ||w|| is the kernels' bound on |approximate - exact| logit
(sim_refine_kernel; the row-block kernel's own threshold uses the same number without `scale`), evaluated here in float64.

Planted rows.  A scenario owns a +-1 code h over the first d - 64 coordinates and k + 2 names at chosen positions.  Name r of the ladder
is h * (1 - t * 2^-11) with integer t per coordinate (fp16 numbers in (1/2, 1]), so a row f = 2^e * h scores 2^e * (d - 64 - m_r * 2^-11)
on it with an integer "deficit" m_r: every product and every partial sum is a multiple of 2^(e-11) below 2^(e+10), exact in float64 AND
in fp32, whatever the order.  All other names are +-1/4 patterns (|logit| <~ 40 * 2^e against ~448 * 2^e on the ladder), the last 64
coordinates of every name hold +1/4 (a row of -4 there makes every logit negative).  Power-of-two row scalings 2^-8 .. 2^6 are mixed
inside every 256-row block; they move neither the indices nor the ladder measured in E.
  wide    consecutive rungs >= 16 E apart (built with 20 E): the certificate must hold, unless `proven_flagged` (below) says it cannot;
  narrow  ranks k and k + 1 are one deficit step apart (2^-11 unscaled = one truncated-key bucket at these logits, ~E / 13) or identical
          name rows (an exact tie), lower or higher index first, in the same or in different half lists; every other rung is wide.  Such a
          row is flagged or resolved by the float64 refine pass.  Every narrow scenario also gets one all-negative row per block: there
          the pair is at most half a bucket apart and shares a key bucket (asserted), where negative keys order in reverse.

`proven_flagged(case, tm)`: a row cannot be certified when one half list's tm-th largest exact logit is within E / 2 of the row's k-th
largest: the certificate is kth > astar + E with astar >= that list's last entry (its approximate value is within 0.04 E of the exact one
on these inputs: exact accumulation, 2^-19 relative for the key bits).  That is the case for all-zero rows, for a vocabulary of one
repeated name and - a property of eight entries per half list, docs/design/sim_topk.md - for k >= 7 when the k + 1 best share a half.
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "f w k scale kind certified flagged rows_scale tag")
# f [n, d] fp16, w [d, V] fp16 (the oracle's layout), certified / flagged: row sets the construction decides, rows_scale: log2 of the row's
# power-of-two factor (None where the row has none), kind: per row 'wide' | 'narrow' | 'zero' | 'neg' | 'dense'

BIAS = 64


def e_bound(f, w, scale):
    """The code's E per row, in float64 (scaled logit units)."""
    f64, w64 = np.asarray(f, np.float64), np.asarray(w, np.float64)
    d = f64.shape[1]
    return 1.5 * scale * (d * 2.0 ** -24 + 2.24e-6) * np.sqrt((f64 * f64).sum(1)) * np.sqrt((w64 * w64).sum(0).max())


def logits64(f, w, scale):
    return scale * (np.asarray(f, np.float64) @ np.asarray(w, np.float64))


def half_of(name):
    return (np.asarray(name) >> 2) & 1


def vsplit_of(v):
    return ((v + 31) // 32 // 2) * 32


def check_separated(lg, k, w):
    """Among a row's top k + 2 logits any two are equal by construction (identical name rows) or differ by more than 1e-9 relative."""
    k2 = min(k + 2, lg.shape[1])
    top = np.argsort(-lg, axis=1, kind="stable")[:, :k2]
    tv = np.take_along_axis(lg, top, 1)
    w64 = np.asarray(w, np.float64)
    for j in range(k2 - 1):
        gap = tv[:, j] - tv[:, j + 1]
        close = np.nonzero(gap <= 1e-9 * np.maximum(np.abs(tv[:, j]), 1e-300))[0]
        for i in close:
            assert gap[i] == 0.0 and np.array_equal(w64[:, top[i, j]], w64[:, top[i, j + 1]]), ("float64 order undecided", i, j)


def _positions(v, k, rot):
    """Scenario -> the k + 2 ladder positions in rank order.  Covers names 0, 31, 32, v - 1, vsplit - 1, vsplit (rotated by `rot` so that
    the parametrised cases put each of them on rank 1 somewhere), one half list, one lane of one unit, the last unit, one per unit."""
    k2, nun, vs = k + 2, (v + 31) // 32, vsplit_of(v)
    used, out = set(), {}

    def take(name, cands):
        got = []
        for p in cands:
            if 0 <= p < v and p not in used and p not in got:
                got.append(p)
            if len(got) == k2:
                break
        assert len(got) == k2, (name, v, k)
        used.update(got)
        out[name] = got

    edges = [v - 1, vs, 0, vs - 1, 32, 31]
    edges = edges[rot % 6:] + edges[:rot % 6]
    spare = [64 + 33 * j for j in range(3 * k2)]
    if k2 >= 6:
        take("edges", edges + spare)
    else:
        take("edges_a", edges[:3] + spare)
        take("edges_b", edges[3:] + spare)
    # one half list AND one quarter list of the 16x16x32 kernel: names = 0..3 mod 16, from unit 3 on
    take("one_half", [96 + 16 * (j // 4) + j % 4 for j in range(4 * k2)])
    # five (or k + 2 if fewer) in the 16 positions of lane half 1 of one unit (names 4..7, 12..15, 20..23, 28..31 of unit 7), the best
    # of them NOT first in the unit; the rest one per unit
    u0 = 32 * min(7, nun - 2)
    take("one_lane", [u0 + p for p in (29, 5, 14, 22, 7)][:min(5, k2)] + [u0 + 64 + 32 * j + (5 * j) % 32 for j in range(3 * k2)])
    # as many as fit in the last (partly padded) unit, from the last name down; the rest in the unit before it
    take("last_unit", [v - 1 - j for j in range(v)])
    take("spread", [32 * ((3 + 2 * j) % nun) + (11 * j + 6) % 32 for j in range(8 * k2)] + list(range(v)))
    # narrow pairs (ranks k, k + 1): index order x same / other half list, and an exact tie across the halves
    free = [p for p in range(40, v) if p not in used]
    fa = [p for p in free if half_of(p) == 0]
    fb = [p for p in free if half_of(p) == 1]

    def narrow(name, pk, pk1, filler):
        rest = [p for p in filler if p not in (pk, pk1) and p not in used][:k2 - 2]
        lad = rest[:k - 1] + [pk, pk1] + rest[k - 1:]
        assert len(lad) == k2
        used.update(lad)
        out[name] = lad

    def pick(half, frac):
        c = [p for p in free if p not in used and half_of(p) == half]
        return c[int(frac * (len(c) - 1))]

    def filler():
        c = [p for p in free if p not in used]
        return c[::max(1, len(c) // (2 * k2))]

    narrow("n_lo_same", pick(0, 0.02), pick(0, 0.6), filler())
    narrow("n_hi_same", pick(1, 0.7), pick(1, 0.03), filler())
    narrow("n_lo_cross", pick(0, 0.1), pick(1, 0.5), filler())
    narrow("n_hi_cross", pick(0, 0.8), pick(1, 0.05), filler())
    narrow("n_tie_cross", pick(1, 0.15), pick(0, 0.4), filler())
    return out


def _name_row(code, deficit):
    """code * (1 - t 2^-11), sum t = deficit, t as even as possible (<= 1023 per coordinate: values stay in (1/2, 1])."""
    dc = code.shape[0]
    t = np.full(dc, deficit // dc, np.int64)
    t[:deficit % dc] += 1
    assert t.max() <= 1023
    return code * (1.0 - t * 2.0 ** -11)


def planted(n, v, d, k, spacing, scale=100.0, seed=0, zero_rows=True, neg_rows=True):
    """spacing 'wide' | 'narrow' (narrow: the narrow scenarios only).  Rows cycle through the scenarios; with zero_rows / neg_rows a few
    rows inside each 256-row block are all-zero / score negative on every name."""
    assert d >= 256 and v >= 600 and 1 <= k <= 8
    rs = np.random.RandomState(1000 * k + v + d + seed)
    dc, k2 = d - BIAS, k + 2
    pos = _positions(v, k, rot=k + v)
    names = [s for s in pos if s.startswith("n_") == (spacing == "narrow")]
    e_unit = 1.5 * ((d * 2.0 ** -24 + 2.24e-6) * np.sqrt(dc) * np.sqrt(dc + BIAS / 16.0))      # unscaled E of a row 1 * h
    rung = 2 * int(np.ceil(10.0 * e_unit * 2 ** 11))               # even: rank k's deficit is even, see the negative rows below
    negdiv = 16.0 if dc <= 512 else 32.0
    small = 1                                                      # one key bucket (2^-11 at logits in [256, 512)), far inside E / 4
    w = np.empty((d, v))
    w[:dc] = rs.choice([-0.25, 0.25], size=(dc, v))
    w[dc:] = 0.25
    codes = rs.choice([-1.0, 1.0], size=(len(names), dc))
    for s, name in enumerate(names):
        deficit = 0
        for r_, p in enumerate(pos[name]):
            if r_ > 0:
                if spacing == "narrow" and r_ == k:
                    deficit += 0 if name == "n_tie_cross" else small
                else:
                    deficit += rung
            w[:dc, p] = _name_row(codes[s], deficit)
    f = np.zeros((n, d))
    kind = np.empty(n, dtype=object)
    rows_scale = np.full(n, np.nan)
    scen = np.full(n, -1)
    for i in range(n):
        s = i % len(names)
        e = int(rs.randint(-8, 7))
        j = i % 256
        if zero_rows and j in (0, 77, 255):
            kind[i] = "zero"
        elif neg_rows and 1 <= j <= len(names):                    # one all-negative row per scenario and block
            f[i, :dc] = codes[s] / negdiv
            f[i, dc:] = -4.0
            kind[i] = "neg"
        else:
            f[i, :dc] = codes[s] * 2.0 ** e
            kind[i], rows_scale[i], scen[i] = spacing, e, s
    f16, w16 = f.astype(np.float16), w.astype(np.float16)
    assert np.array_equal(f16.astype(np.float64), f) and np.array_equal(w16.astype(np.float64), w)          # fp16-exact
    lg = logits64(f16, w16, scale)
    E = e_bound(f16, w16, scale)
    order = np.argsort(-lg, axis=1, kind="stable")[:, :k2 + 1]
    tv = np.take_along_axis(lg, order, 1)
    lad = (kind == spacing)
    for i in np.nonzero(lad)[0]:
        want = pos[names[scen[i]]]
        assert sorted(order[i, :k2]) == sorted(want) and (tv[i, k2 - 1] - tv[i, k2]) > 100 * E[i]       # the rest is far below
        gaps = tv[i, :k2 - 1] - tv[i, 1:k2]
        for j in range(k2 - 1):
            if spacing == "narrow" and j == k - 1:
                assert gaps[j] <= E[i] / 4 and list(order[i, k - 1:k + 1]) in (want[k - 1:k + 1], sorted(want[k - 1:k + 1]))
                if names[scen[i]] != "n_tie_cross":
                    assert gaps[j] > 0 and list(order[i, k - 1:k + 1]) == want[k - 1:k + 1]
            else:
                assert gaps[j] >= 16 * E[i], (i, j, gaps[j] / E[i])
    assert (lg[kind == "neg"] < 0).all()
    if spacing == "narrow" and neg_rows:
        # negative rows score -64 + (d - 64 - m 2^-11) / negdiv unscaled, in (-64, -32]: a key bucket (the low 4 mantissa bits) is 2^-14
        # wide, the narrow pair 2^-15 or 2^-16 apart and rank k's deficit m even: the pair shares a bucket on every scenario but the exact
        # tie, and there the key order of negative values is the reverse of their order
        for i in np.nonzero(kind == "neg")[0]:
            a = (lg[i, order[i, k - 1:k + 1]] / scale).astype(np.float32)
            assert names[i % len(names)] == "n_tie_cross" or (a[0] > a[1] and (a.view(np.uint32)[0] >> 4) == (a.view(np.uint32)[1] >> 4))
    check_separated(lg[kind != "zero"], k, w16)
    case = Case(f16, w16, k, scale, kind, None, None, rows_scale, "planted-%s" % spacing)
    pf = proven_flagged(case, tm=4 if (k == 1 and d == 512) else 8)
    cert = set(np.nonzero(kind == "wide")[0].tolist()) - pf
    return case._replace(certified=cert, flagged=pf), pos, names, scen


def proven_flagged(case, tm):
    """Rows no certificate over `tm` entries per half list can pass (module docstring)."""
    lg = logits64(case.f, case.w, case.scale)
    E = e_bound(case.f, case.w, case.scale)
    kth = -np.sort(-lg, axis=1)[:, case.k - 1]
    out = set()
    hv = half_of(np.arange(lg.shape[1]))
    for h in (0, 1):
        sub = lg[:, hv == h]
        if sub.shape[1] > tm:                                      # a list that is not full hides nothing
            tmth = -np.sort(-sub, axis=1)[:, tm - 1]
            out |= set(np.nonzero(tmth >= kth - E / 2)[0].tolist())
    return out


def repeated_vocab(n, v, d, k, scale=100.0, seed=0):
    """One name row V times: every logit of a row ties, the indices are 0 .. k - 1 and no row can be certified."""
    rs = np.random.RandomState(seed + n + v)
    w = np.repeat(rs.choice([-1.0, 1.0], size=(d, 1)) * 0.5, v, axis=1).astype(np.float16)
    f = (rs.randint(-8, 9, size=(n, d)) / 8.0).astype(np.float16)
    kind = np.full(n, "repeat", dtype=object)
    case = Case(f, w, k, scale, kind, set(), None, np.full(n, np.nan), "repeated")
    pf = proven_flagged(case, tm=8)
    assert pf == set(range(n)) or v <= 16
    return case._replace(flagged=pf)


def dense(n, v, d, k, scale=100.0, seed=0):
    """The existing recipe: Gaussian rows / names of unit expected norm, names 3 and 5 identical."""
    rs = np.random.RandomState(n + v + d + 7919 * seed)
    f = (rs.randn(n, d) / np.sqrt(d)).astype(np.float16)
    w = (rs.randn(d, v) / np.sqrt(d)).astype(np.float16)
    if v > 5:
        w[:, 5] = w[:, 3]
    return Case(f, w, k, scale, np.full(n, "dense", dtype=object), set(), set(), np.full(n, np.nan), "dense")


def oracle_rows(n):
    """The rows the float64 oracle is evaluated on: all up to 4,096, else the first 512, the last 512 and 1,024 sampled."""
    if n <= 4096:
        return np.arange(n)
    mid = np.random.RandomState(n).choice(np.arange(512, n - 512), size=1024, replace=False)
    return np.concatenate([np.arange(512), np.sort(mid), np.arange(n - 512, n)])


def close_rows(lg, E, k):
    """Rows whose ranks k and k + 1 lie within 2 E of each other (the rows a dense input can send to the exact pass)."""
    s = -np.sort(-lg, axis=1)[:, :k + 1]
    return np.nonzero(s[:, k - 1] - s[:, k] <= 2 * E)[0] if lg.shape[1] > k else np.arange(0)


def crowded_rows(lg, E, k, tm=8):
    """Rows whose k-th largest logit lies within 2 E of the tm-th largest of one half list: what the certificate itself compares."""
    kth = -np.sort(-lg, axis=1)[:, k - 1]
    hv = half_of(np.arange(lg.shape[1]))
    out = np.zeros(lg.shape[0], bool)
    for h in (0, 1):
        sub = lg[:, hv == h]
        if sub.shape[1] > tm:
            out |= kth - (-np.sort(-sub, axis=1)[:, tm - 1]) <= 2 * E
    return np.nonzero(out)[0]
