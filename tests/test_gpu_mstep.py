"""The Lloyd M-step family on exact-grid data (tests/mstep_cases.py), bit for bit: scd_kmeans_mstep / scd_kmeans_mstep_f16 on every
case (every G of mstep_segment_kernel<G, 8, 8> and <G, 64, 8>, every G2 of mstep_segment16_kernel, the three sort paths, ten label
layouts), scd_kmeans_finalize on those sums, scd_kmeans_sumsq on both branches, and scd_kmeans_lloyd_step_delta (mstep_delta_kernel,
labels_sync_kernel, the inertia from the sums inside finalize_kernel and, at k = 6,554, in inertia_dd_kernel) on scripted centre sets.

On the grid every sum, count and row-wise inertia is an exactly representable integer times a power of two, so the float64 atomics'
order does not matter and the results are compared with array_equal.  The two quantities that are NOT exact by construction carry
a-priori bounds:
  shift     (d + k + 8) 2^-52 relative to the exactly computed value: the longest float64 addition chain
  inertia from the sums   2^-52 |I| + 2^-90 (sum x^2 + sum_k n_k ||c_k||^2 + 2 sum_k |<c_k, S_k>|) around the exact rational I: one final
            rounding plus the double-double evaluation's error on its largest intermediates
  sum of squares   Fraction(hi) + Fraction(lo) equals the exact sum where it fits 106 bits of its terms' common unit, else within 2^-90 relative (non-negative
            terms, fewer than 2^12 double-double additions on any path, each accurate to ~2^-103)
Every row, every cluster and every case is asserted.  What an MI355X returned on the first run, and the double-double bug the "means"
step of the k = 7 script exposed (a product's rounding error counted twice under fp contraction: 7.1e-15 off against a bound of
4.1e-17), is recorded in docs/design/lloyd_mstep.md.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

import mstep_cases as mc
from test_mstep_cases_sensitivity import check_mstep

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device; they must not be skipped on the GPU box"
    from scd_amd import ops as o
    return o


def dev(x):
    return None if x is None else torch.as_tensor(x).cuda()


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


# ------------------------------------------------------------------------------------------------ scd_kmeans_mstep[_f16]
def _mstep_both(ops, case, ref):
    x, lab, c_old = dev(case.x), dev(case.labels), dev(case.c_old)
    s, c, i = ops.kmeans_mstep(x, lab, c_old, case.k, case.split)
    check_mstep(case.name + " float32 " + case.kern, ref, host(s), host(c), host(i))
    if case.f16:
        x16 = x.to(torch.float16)                       # exact (asserted by mstep_cases.grid_rows)
        s2, c2, i2 = ops.kmeans_mstep(x, lab, c_old, case.k, case.split, x16=x16)
        check_mstep(case.name + " fp16 copy", ref, host(s2), host(c2), host(i2))
        assert same_bits(s, s2) and torch.equal(c, c2)
    return x, s, c


@pytest.mark.parametrize("sp", mc.mstep_specs(), ids=lambda s: s.name)
def test_mstep_equals_the_exact_reference(ops, sp):
    """sums, counts and both inertia values of scd_kmeans_mstep (and of scd_kmeans_mstep_f16 where the rows have an exact fp16 copy)
    equal the integer reference on every cluster; the two kernels' sums and counts are the same bits."""
    case, ref = mc.case(sp)
    if sp.n == 1200000:
        assert (mc.cdiv(sp.n, 1024) + 1) * (sp.k + 1) * 4 > 24 * sp.n + (8 << 20)      # the counting sort's histogram does not fit
    _mstep_both(ops, case, ref)


# ------------------------------------------------------------------------------------------------ scd_kmeans_finalize
FINALIZE = [mc.spec("uniform", 1025, 130, 1, 300, seed=1), mc.spec("interleaved", 1025, 130, 7, 300, seed=2),
            mc.spec("one_giant", 31, 130, 7, 10, seed=3), mc.spec("interleaved", 4100, 64, 256, 1000, seed=4),
            mc.spec("singletons", 300, 64, 256, 100, seed=5), mc.spec("interleaved", 4100, 64, 257, 1000, seed=6),
            mc.spec("singletons", 300, 64, 257, 100, seed=7), mc.spec("interleaved", 4100, 64, 2048, 1000, seed=8),
            mc.spec("singletons", 4000, 64, 2048, 1000, seed=9), mc.spec("interleaved", 7000, 64, 6554, 1000, seed=10),
            mc.spec("singletons", 4100, 64, 6554, 1000, seed=11)]


def check_shift(got, c_new, c_old, empty, mode, d, k, what):
    """NaN iff a cluster is empty, else within (d + k + 8) 2^-52 relative of the exactly computed value.  Returns the relative error."""
    if empty.any():
        assert np.isnan(got), (what, got)
        return None
    want = mc.exact_shift(c_new, c_old, mode)
    assert np.isfinite(got), (what, got)
    err = abs(Fraction(float(got)) - want)
    rel = float(err / want) if want else float(err)
    print("%s: shift mode %d relative error %.3e, bound %.3e" % (what, mode, rel, (d + k + 8) * 2.0 ** -52))
    assert err <= want * Fraction(d + k + 8, 1 << 52), (what, got, float(want))
    return rel


def check_centres(c, sums_i, counts, what):
    """Centre bits equal float32(float64(S) / float64(n)); NaN rows exactly at the empty clusters."""
    want = mc.centres(sums_i, counts)
    empty = counts == 0
    assert np.isnan(c[empty]).all() and not np.isnan(c[~empty]).any(), what
    assert np.array_equal(c[~empty].view(np.uint32), want[~empty].view(np.uint32)), what
    return want, empty


@pytest.mark.parametrize("sp", FINALIZE, ids=lambda s: s.name)
def test_finalize_centres_and_shift(ops, sp):
    """scd_kmeans_finalize on the M-step's sums for k = 1, 7, 256, 257, 2,048, 6,554, with and without the fused E-step operand
    preparation and in both shift modes: centre bits, NaN rows, the shift's bound; with data=, the following data.estep(centres)
    returns the labels of a stand-alone E-step from the same centres."""
    case, ref = mc.case(sp)
    x, s, c = _mstep_both(ops, case, ref)
    c_old = dev(case.c_old)
    has_empty = bool((ref[1] == 0).any())
    assert has_empty == (sp.layout != "interleaved" and sp.k > 1)
    for mode in (0, 1):
        cn, sh = ops.kmeans_finalize(s, c, c_old, shift_mode=mode)
        want, empty = check_centres(host(cn), ref[0], ref[1], sp.name)
        check_shift(float(sh.item()), want, case.c_old, empty, mode, sp.d, sp.k, sp.name)
        data = ops.KMeansData(x)
        cd, shd = ops.kmeans_finalize(s, c, c_old, shift_mode=mode, data=data)
        assert torch.equal(cn.view(torch.int32), cd.view(torch.int32))
        check_shift(float(shd.item()), want, case.c_old, empty, mode, sp.d, sp.k, sp.name + " data=")
        lab = data.estep(cd)
        alone = ops.KMeansData(x).estep(cn.clone())
        assert torch.equal(lab, alone), sp.name
    cn, sh = ops.kmeans_finalize(s, c, None)                       # no C_old: centres only
    check_centres(host(cn), ref[0], ref[1], sp.name)


# ------------------------------------------------------------------------------------------------ scd_kmeans_sumsq
def _wide_f16(n, d, seed):
    """fp16 values over the format's whole range in one array: random finite bit patterns (subnormals included), 65,504 next to 2^-24."""
    rs = np.random.RandomState(seed)
    bits = rs.randint(0, 0x7C00, size=n * d).astype(np.uint16) | (rs.randint(0, 2, size=n * d).astype(np.uint16) << 15)
    v = bits.view(np.float16).copy()
    v[:2] = (65504.0, 2.0 ** -24)[:n * d]
    if n * d > 4:
        v[-2:] = (2.0 ** -24, -65504.0)
    return v.reshape(n, d)


def _wide_f32(n, d, seed):
    """float32 values from 2^-60 to 2^20 in one array (their squares span 160 bits: more than a double-double holds)."""
    rs = np.random.RandomState(seed)
    v = (rs.uniform(1.0, 2.0, size=n * d) * 2.0 ** rs.randint(-60, 20, size=n * d) * rs.choice([-1.0, 1.0], size=n * d)).astype(np.float32)
    v[:2] = (2.0 ** 20, 2.0 ** -60)[:n * d]
    return v.reshape(n, d)


def _grid_f32(n, d, seed):
    """float32 values whose sum of squares FITS a double-double: half of them integers below 2^24 times 2^-19 (up to 32), half integers
    below 2^24 times 2^-38.  The squares' common unit is 2^-76 and 2.1 M of them sum to ~2^29: 105 bits at the largest shapes."""
    rs = np.random.RandomState(seed)
    m = rs.randint(-(1 << 24) + 1, 1 << 24, size=n * d).astype(np.float64)
    v = (m * np.where(rs.rand(n * d) < 0.5, 2.0 ** -19, 2.0 ** -38)).astype(np.float32)
    v[:2] = (((1 << 24) - 1) * 2.0 ** -19, 2.0 ** -38)[:n * d]
    return v.reshape(n, d)


def _sumsq(ops, t, n, d, split, offset_bytes=0):
    from scd_amd import _lib
    ops._need_cuda(t)
    out = torch.full((4,), float("nan"), dtype=torch.float64, device=t.device)
    p = _lib._vp(t.data_ptr() + offset_bytes)
    x16, x = (p, None) if t.dtype == torch.float16 else (None, p)
    _lib.check(ops._L().scd_kmeans_sumsq(ops.handle(), x16, x, n, d, split, _lib.ptr(out), ops.stream_ptr()))
    return host(out)


SUMSQ = [  # (n, d, splits): split * d both a multiple of 8 and not; n d not a multiple of 8; n d < 8; more than one sweep of the grid
    (3, 2, (0, 1, 3)), (1, 1, (0, 1)), (37, 6, (0, 4, 5, 37)), (64, 8, (0, 1, 64)), (1000, 33, (0, 8, 333, 1000)),
    (16400, 128, (0, 1, 8191, 16400)), (16401, 130, (5, 16397))]


@pytest.mark.parametrize("kind", ["f16", "f32", "f32grid"])
@pytest.mark.parametrize("n,d,splits", SUMSQ, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_sumsq_is_a_true_double_double(ops, kind, n, d, splits):
    """scd_kmeans_sumsq called directly, fp16 branch and float32 branch (X16 == NULL), at full size on both: hi + lo of both parts
    equals the exact sum wherever that sum, counted in the common unit of its terms, fits 106 bits, and lies within 2^-90 relative
    where it does not (float32 values from 2^-60 to 2^20).  The float32 grid values always fit."""
    v = {"f16": _wide_f16, "f32": _wide_f32, "f32grid": _grid_f32}[kind](n, d, n + d)
    t = dev(v)
    worst, bits = 0.0, 0
    for split in splits:
        out = _sumsq(ops, t, n, d, split)
        for part, (a, b) in enumerate(((0, split * d), (split * d, n * d))):
            want, unit = mc.exact_sumsq(v, a, b)
            hi, lo = float(out[2 * part]), float(out[2 * part + 1])
            got = Fraction(hi) + Fraction(lo)
            assert abs(lo) <= abs(hi) * 2.0 ** -52 or hi == 0.0, (n, d, split, part, hi, lo)
            if want == 0:
                assert hi == 0.0 and lo == 0.0
                continue
            width = (want / Fraction(2) ** unit).numerator.bit_length()
            assert kind != "f32grid" or width <= 106
            if width <= 106:                                       # an integer of common units that a double-double holds: exact
                bits = max(bits, width)
                assert got == want, (n, d, split, part, width, hi, lo, float(want))
            else:
                rel = float(abs(got - want) / want)
                worst = max(worst, rel)
                assert abs(got - want) <= want * Fraction(1, 1 << 90), (n, d, split, part, hi, lo, rel)
    print("sumsq %s [%d, %d]: exact up to %d bits; largest relative error beyond 106 bits %.3e (bound 2^-90 = %.3e)"
          % (kind, n, d, bits, worst, 2.0 ** -90))


def test_sumsq_refuses_a_misaligned_base_pointer(ops):
    from scd_amd import _lib
    for v, off in ((_wide_f16(9, 8, 0), 2), (_wide_f32(9, 8, 0), 4)):
        with pytest.raises(_lib.ScdError, match="16-byte aligned"):
            _sumsq(ops, dev(v), 8, 8, 3, offset_bytes=off)


# ------------------------------------------------------------------------------------------------ scd_kmeans_lloyd_step_delta
def check_inertia(got, exact4, what, worst):
    """|got - I| <= 2^-52 |I| + 2^-90 (sum x^2 + sum_k n_k ||c_k||^2 + 2 sum_k |<c_k, S_k>|), all as exact rationals."""
    I, x2, ncc, dot = exact4
    one = 1 << (2 * mc.SCALE)
    err = abs(Fraction(float(got)) - Fraction(I, one))
    bound = Fraction(abs(I), one << 52) + Fraction(x2 + ncc + dot, one << 90)
    worst[0] = max(worst[0], float(err))
    worst[1] = max(worst[1], float(bound))
    assert np.isfinite(got) and err <= bound, (what, float(got), I / one, float(err), float(bound))


def run_script(ops, sc, steps):
    """steps: (name, centres in grid units as float32-exact float64 [k, D], full, expected changed rows or None)."""
    from scd_amd import _lib
    k, l_num, n_u = sc.k, sc.l_num, sc.n_u
    cat = dev(sc.x)
    cat16 = ops.f16_exact(cat)
    assert cat16 is not None
    buf = ops.LloydBuffers(ops.KMeansData(cat[l_num:]), cat, cat16, k)
    assert buf.inc
    buf.lab32[:l_num] = dev(sc.lab_fixed.astype(np.int32))
    prev = np.full(n_u, -1, dtype=np.int64)
    worst = [0.0, 0.0]
    for name, cu, full, expect in steps:
        what = "k=%d l_num=%d step %s" % (k, l_num, name)
        c_in = (cu * mc.UNIT).astype(np.float32)
        assert np.array_equal(c_in.astype(np.float64), cu * mc.UNIT)
        buf.c0.copy_(dev(c_in))
        stats, c_out = buf.stats[0], buf.c[0]
        buf.step_delta(buf.c0, c_out, stats, False, full)
        st = host(stats)
        want_u = sc.labels(cu)
        lab = host(buf.lab32).astype(np.int64)
        assert np.array_equal(lab[l_num:], want_u), what
        assert np.array_equal(lab[:l_num], sc.lab_fixed), what
        lp = host(buf.lab_prev).astype(np.int64)
        assert np.array_equal(lp[l_num:], lab[l_num:]) and (lp[:l_num] == -1).all(), what
        changed = int((want_u != prev).sum())
        if expect is not None:
            assert changed == expect, (what, changed)
        assert st[4] == changed, (what, st[4], changed)
        prev = want_u
        lab32 = lab.astype(np.int32)
        s_i, cnt = mc.sums_counts(sc.xi, lab32, k)
        assert np.array_equal(host(buf.counts), cnt), what
        assert np.array_equal(host(buf.sums), s_i.astype(np.float64) * mc.UNIT), what
        want_c, empty = check_centres(host(c_out), s_i, cnt, what)
        check_shift(st[2], want_c, c_in, empty, 0, mc.D, k, what)
        ex = mc.exact_inertia(sc.xi, lab32, k, c_in, row0=l_num)
        check_inertia(st[0], ex[0], what + " labelled", worst)
        check_inertia(st[1], ex[1], what + " unlabelled", worst)
        if l_num == 0:
            assert st[0] == 0.0, what
    print("k=%d l_num=%d: largest inertia error %.3e, largest bound %.3e" % (k, l_num, worst[0], worst[1]))
    return buf


@pytest.mark.parametrize("k,n_u,l_num", [(7, 6 * 64 + 37, 0), (7, 6 * 64 + 37, 37), (300, 450, 0), (300, 450, 37)])
def test_incremental_step_on_controlled_change_sets(ops, k, n_u, l_num):
    """A full step, then incremental steps whose centre sets make: no row change; exactly one; the four rows at unlabelled positions
    63 / 64 / 65 / n_u - 1 (the last ragged wave); all 64 rows of one wave; a cluster lose every row and get them back; two centres
    swap; centres off the grid; every row (centres rotated by one index).  After every step: labels, sums, counts, labels_prev, the
    change count, centre bits, shift and both inertia values."""
    sc = mc.Scene(k, n_u, l_num, seed=k + l_num)
    base = sc.a.astype(np.float64)
    far = base.copy()
    if sc.block:
        h = next(j for j in range(k) if j not in sc.P and j not in sc.Q) if k > 8 else sc.Q[1]
        wave_rows, wave = 64, None
    else:
        h = 10                                                 # two unlabelled rows, no labelled one (their labels are multiples of 3)
        w0 = 64 * 3                                            # rows 192 .. 255: their homes have one row each (n_u = 1.5 k)
        idx = sc.home[w0:w0 + 64]
        assert not set(idx) & set(sc.P + sc.Q) and (np.bincount(sc.home, minlength=k)[idx] == 1).all()
        wave = base.copy()
        wave[idx] = base[np.roll(idx, 1)]
    far[h] = base[h] + 4000.0
    lost = int((sc.home == h).sum())
    A, B = [j for j in range(k) if j not in sc.P and j not in sc.Q and j != h][:2] if k > 8 else (sc.P[0], sc.P[2])
    swap = base.copy()
    swap[[A, B]] = base[[B, A]]
    n_swap = int(((sc.home == A) | (sc.home == B)).sum())
    steps = [("full", base, True, n_u), ("none", base, False, 0), ("one", sc.pulled([0]).astype(np.float64), False, 1),
             ("one back", base, False, 1), ("edges", sc.pulled([0, 1, 2, 3]).astype(np.float64), False, 4), ("edges back", base, False, 4)]
    if wave is not None:
        steps += [("wave", wave, False, 64), ("wave back", base, False, 64)]
    steps += [("emptied", far, False, lost), ("refilled", base, False, lost), ("swap", swap, False, n_swap), ("swap back", base, False, n_swap),
              ("means", mc.scene_means(sc), False, 0), ("full again", base, True, 0), ("all", np.roll(base, -1, axis=0), False, n_u)]
    if sc.block:
        assert lost == 64                                       # the emptied cluster IS one whole wave
    run_script(ops, sc, steps)


@pytest.mark.parametrize("k", [6553, 6554])
def test_incremental_step_inertia_at_the_fused_limit(ops, k):
    """k = 6,553 is the last k whose inertia from the sums is evaluated inside finalize_kernel (5 k <= 32,768 scratch doubles), 6,554 the
    first that launches inertia_dd_kernel: the same bound for both.  The step after the full one keeps every label, so the row-wise
    inertia (full step) and the sums-based one (incremental) of the same assignment both lie within the bound of the exact value."""
    assert (5 * k <= 32768) == (k == 6553)
    sc = mc.Scene(k, 7000, 37, seed=k)
    base = sc.a.astype(np.float64)
    steps = [("full", base, True, 7000), ("none", base, False, 0), ("edges", sc.pulled([0, 1, 2, 3]).astype(np.float64), False, 4),
             ("means", mc.scene_means(sc), False, 4)]
    run_script(ops, sc, steps)
