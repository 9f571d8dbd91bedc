"""Can the inputs of tests/mstep_cases.py tell a wrong M-step from a right one?  A small numpy model of the DOCUMENTED data flow of
scd_kmeans_mstep[_f16] (mstep.hip) and of mstep_delta_kernel (kmeans.hip) is run on every case and judged by the assertions
tests/test_gpu_mstep.py uses (`check_mstep`, `check_delta`):
  sort      bucket = label, or k for a label outside [0, k); counting sort: a histogram per 1,024-row block, per bucket the exclusive scan
            over the blocks, the buckets' starts from the totals, a key lands at start + rows of its bucket in earlier blocks + arrival
            order inside the block; k > 8,191 or a histogram that does not fit the workspace: a radix sort of (bucket, row)
  segment   a wave takes ROWS consecutive sorted keys, MU at a time; a key whose bucket is not below k is passed over; a change of label
            flushes the register run (sums and run length) to the old label; the row-wise inertia goes to the first or the second
            total by ROW id < split
  merge     the last run of each of a block's four waves goes to LDS; wave w is the leader of its label unless an earlier wave of the block
            ends in the same one; a leader adds the sums AND the run lengths of the waves w .. lw - 1 that end in its label (lw = live
            waves of the block, at most 4) and flushes once
  delta     waves of 64 rows from row0: a row whose label differs from labels_prev is added to its new cluster and subtracted from its old
            one (each only if (unsigned) label < k), counts +-1, labels_prev updated, the changes counted

The correct model passes every case.  Each planted failure fails at least one case; CATCHES names one per failure and kernel schedule
and the test asserts exactly those:
  follower waves' sums merged but not their run counts   tails[167,3,40,s0] (few32), tails[32513,33,200,s10837] (prod32), tails[1317,64,40,s659] (f16)
  every wave flushes as well as its leader               the same three
  flush skipped when the label changes on the first key of an MU group
                                                         boundaries[33000,33,64,s0] (prod32), boundaries[1030,64,64,s343] (f16); with
                                                         ROWS = MU = 8 a wave is one group and the failure does not exist
  invalid labels folded into cluster k - 1               uniform[257,768,11,s85], uniform[33000,33,11,s1] (and every case with an invalid label)
  block offsets ignored by the scatter                   interleaved[1025,1000,13,s341], interleaved[33000,33,13,s1]: every label in every
                                                         1,024-row block (any case with a label in two blocks)
  split test on the sorted position instead of the row   uniform[257,768,11,s85], uniform[33000,8,8192,s11000], boundaries[1030,64,64,s343]
  delta: the old cluster not decremented                 one[l0]
  delta: the last ragged wave dropped                    ragged[l0]
  delta: row0 ignored                                    last_row[l37]   (a change in the last l_num rows)
The model is not the kernel; what is asserted on the device is asserted there on the device's own output.
"""
import numpy as np
import pytest

import mstep_cases as mc

SCHEDULES = {"few32": (8, 8), "prod32": (64, 8), "f16": (64, 8)}          # kernel -> (ROWS, MU)


def sort_model(labels, k, path, mut=()):
    """-> (bucket, row) of every sorted position; a position no key was written to holds bucket k."""
    n = len(labels)
    lab = labels.astype(np.int64)
    b = np.where((lab < 0) | (lab >= k), k - 1 if "fold_invalid" in mut else k, lab)
    if path != "count":
        order = np.argsort(b, kind="stable")
        return b[order], order
    blk = np.arange(n) // 1024
    nblk = mc.cdiv(n, 1024)
    comp = blk * (k + 1) + b
    hist = np.bincount(comp, minlength=nblk * (k + 1)).reshape(nblk, k + 1)
    offs = np.cumsum(hist, axis=0) - hist
    tot = hist.sum(axis=0)
    start = np.cumsum(tot) - tot
    order = np.argsort(comp, kind="stable")
    cs = comp[order]
    first = np.nonzero(np.r_[True, cs[1:] != cs[:-1]])[0]
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n) - np.repeat(first, np.diff(np.r_[first, n]))
    pos = start[b] + (0 if "no_block_offs" in mut else offs[blk, b]) + rank
    kb, kr = np.full(n, k, dtype=np.int64), np.zeros(n, dtype=np.int64)
    kb[pos], kr[pos] = b, np.arange(n)
    return kb, kr


def mstep_model(case, ref, kernel, mut=()):
    """-> (sums float64 [k, d], counts int64 [k], inertia float64 [2]) as the device returns them."""
    R, MU = SCHEDULES[kernel]
    xi, k, n = case.xi, case.k, case.xi.shape[0]
    kb, kr = sort_model(case.labels, k, case.sort, mut)
    sums, counts = np.zeros((k, xi.shape[1]), dtype=np.int64), np.zeros(k, dtype=np.int64)
    p = np.nonzero(kb < k)[0]
    inert = [0, 0]
    if len(p):
        l, r, w = kb[p], kr[p], p // R
        first = np.r_[True, (l[1:] != l[:-1]) | (w[1:] != w[:-1])]
        starts = np.nonzero(first)[0]
        run_lab, run_wave, run_cnt = l[starts], w[starts], np.diff(np.r_[starts, len(p)])
        run_sum = np.add.reduceat(xi[r], starts, axis=0, dtype=np.int64)
        last = np.r_[run_wave[1:] != run_wave[:-1], True]
        direct = ~last
        if "skip_mu" in mut:                               # the flush that the NEXT run's first key triggers
            direct &= ~np.r_[(p[starts[1:]] - run_wave[1:] * R) % MU == 0, False]
        np.add.at(sums, run_lab[direct], run_sum[direct])
        np.add.at(counts, run_lab[direct], run_cnt[direct])
        fl = {int(wv): int(i) for wv, i in zip(run_wave[last], np.nonzero(last)[0])}
        for blk in sorted({wv // 4 for wv in fl}):
            lw = min(4, mc.cdiv(n - blk * 4 * R, R))
            ends = [fl.get(blk * 4 + wv, -1) for wv in range(4)]
            for wv in range(4):
                if ends[wv] < 0:
                    continue
                mine = run_lab[ends[wv]]
                if any(ends[w2] >= 0 and run_lab[ends[w2]] == mine for w2 in range(wv)):
                    if "all_flush" in mut:
                        sums[mine] += run_sum[ends[wv]]
                        counts[mine] += run_cnt[ends[wv]]
                    continue
                same = [ends[w2] for w2 in range(wv, lw) if ends[w2] >= 0 and run_lab[ends[w2]] == mine]
                sums[mine] += run_sum[same].sum(axis=0)
                counts[mine] += run_cnt[ends[wv]] if "no_follower_counts" in mut else run_cnt[same].sum()
        a = ref[3][r]
        first_part = (p < case.split) if "split_pos" in mut else (r < case.split)
        inert = [int(a[first_part].sum()), int(a[~first_part].sum())]
    return sums.astype(np.float64) * mc.UNIT, counts, np.array(inert, dtype=np.float64) * (mc.UNIT * mc.UNIT)


def check_mstep(name, ref, sums, counts, inertia):
    """The assertions of test_gpu_mstep on one M-step result: every sum, every count and both inertia values, bit for bit."""
    rs, rc, ri = mc.device_reference(ref)
    counts = np.asarray(counts).astype(np.int64)
    bad = np.nonzero(counts != rc)[0]
    assert bad.size == 0, "%s: %d clusters' counts differ, first %s: %s != %s" % (name, bad.size, bad[:5], counts[bad[:5]], rc[bad[:5]])
    bad = np.nonzero((np.asarray(sums) != rs).any(axis=1))[0]
    assert bad.size == 0, "%s: %d clusters' sums differ from the exact ones, first %s" % (name, bad.size, bad[:5])
    assert np.array_equal(np.asarray(inertia), ri), "%s: inertia %s != %s" % (name, np.asarray(inertia).tolist(), ri.tolist())


def kernels(sp):
    return (mc.kernel32(sp.n),) + (("f16",) if sp.f16 else ())


SPECS = mc.mstep_specs()


@pytest.mark.parametrize("sp", SPECS, ids=lambda s: s.name)
def test_correct_model_passes(sp):
    case, ref = mc.case(sp)
    for kern in kernels(sp):
        check_mstep(sp.name, ref, *mstep_model(case, ref, kern))


def test_case_list_reaches_every_instantiation():
    """Every G of both float32 schedules, every G2 of the fp16 kernel below and above the threshold, the three sort paths, every layout
    on the production kernel, and the workspace inequality of the counting sort's fallback."""
    seen32 = {(mc.kernel32(s.n), mc.g32(s.d)) for s in SPECS}
    assert seen32 >= {(kn, g) for kn in ("few32", "prod32") for g in (1, 2, 4, 8, 12, 16)}
    seen16 = {(s.n > 32512, mc.g16(s.d)) for s in SPECS if s.f16}
    assert seen16 >= {(above, g) for above in (False, True) for g in (1, 2, 4, 6, 8)}
    assert {mc.sort_path(s.n, s.k) for s in SPECS} == {"count", "rocprim", "fallback"}
    assert {s.k for s in SPECS} >= {1, 8191, 8192}
    assert {s.layout for s in SPECS if mc.kernel32(s.n) == "prod32"} == set(mc.LAYOUTS)
    big = [s for s in SPECS if mc.sort_path(s.n, s.k) == "fallback"]
    assert [(s.n, s.d, s.k) for s in big] == [(1200000, 8, 8191)]
    assert (mc.cdiv(1200000, 1024) + 1) * (8191 + 1) * 4 > 24 * 1200000 + (8 << 20)
    assert 32513 in {s.n for s in SPECS} and mc.kernel32(32512) == "few32" and mc.kernel32(32513) == "prod32"


def test_tails_and_boundaries_are_what_they_claim():
    """After the sort the `tails` layout ends the four waves of its first five blocks in AAAA, AAAB, ABBB, AABC, ABCD, its last block has
    1, 2 or 3 live waves and, with 2 or 3, a last wave of invalid keys only; `boundaries` ends runs on m - 1, m, m + 1 for m = 4 .. 768."""
    seen_nw = set()
    for sp in SPECS:
        if sp.layout == "tails":
            R = dict(sp.kw)["rows"]
            kb, _ = sort_model(mc.LAYOUTS["tails"](sp.n, sp.k, sp.seed, rows=R), sp.k, "radix")
            pat = []
            for blk in range(5):
                e = kb[blk * 4 * R + R - 1:(blk + 1) * 4 * R:R]
                pat.append("".join("ABCD"[list(dict.fromkeys(e)).index(v)] for v in e))
            assert pat == ["AAAA", "AAAB", "ABBB", "AABC", "ABCD"], (sp.name, pat)
            B = sp.n // (4 * R)
            nw = mc.cdiv(sp.n - B * 4 * R, R)
            seen_nw.add((R, nw))
            if nw > 1:
                assert (kb[B * 4 * R + (nw - 1) * R:] == sp.k).all() and (kb[B * 4 * R:B * 4 * R + (nw - 1) * R] < sp.k).all(), sp.name
        if sp.layout == "boundaries" and sp.n >= 1030:
            kb, _ = sort_model(mc.LAYOUTS["boundaries"](sp.n, sp.k, sp.seed), sp.k, "radix")
            ends = set((np.nonzero(kb[1:] != kb[:-1])[0] + 1).tolist())
            assert ends >= {m * j + o for m in (4, 8, 32, 64, 256) for j in (1, 2, 3) for o in (-1, 0, 1)}, sp.name
    assert seen_nw >= {(8, 1), (8, 2), (8, 3), (64, 1), (64, 2), (64, 3)}


CATCHES = [
    ("no_follower_counts", "tails[167,3,40,s0]", "few32"),
    ("no_follower_counts", "tails[32513,33,200,s10837]", "prod32"),
    ("no_follower_counts", "tails[1317,64,40,s659]", "f16"),
    ("all_flush", "tails[167,3,40,s0]", "few32"),
    ("all_flush", "tails[32513,33,200,s10837]", "prod32"),
    ("all_flush", "tails[1317,64,40,s659]", "f16"),
    ("skip_mu", "boundaries[33000,33,64,s0]", "prod32"),       # (ROWS = MU = 8 on the few-rows schedule: a wave is ONE group, its first key
    ("skip_mu", "boundaries[1030,64,64,s343]", "f16"),         # starts the first run and flushes nothing - the failure does not exist there)
    ("fold_invalid", "uniform[257,768,11,s85]", "few32"),
    ("fold_invalid", "uniform[33000,33,11,s1]", "prod32"),
    ("no_block_offs", "interleaved[1025,1000,13,s341]", "few32"),
    ("no_block_offs", "interleaved[33000,33,13,s1]", "prod32"),
    ("split_pos", "uniform[257,768,11,s85]", "few32"),
    ("split_pos", "uniform[33000,8,8192,s11000]", "prod32"),
    ("split_pos", "boundaries[1030,64,64,s343]", "f16"),
]


@pytest.mark.parametrize("mut,name,kern", CATCHES)
def test_planted_failure_is_caught(mut, name, kern):
    sp = mc.by_name(name)
    assert kern in kernels(sp)
    case, ref = mc.case(sp)
    with pytest.raises(AssertionError):
        check_mstep(name, ref, *mstep_model(case, ref, kern, mut=(mut,)))


# ------------------------------------------------------------------------------------------------ incremental M-step
def delta_model(dc, sums, counts, mut=()):
    """mstep_delta_kernel on (sums, counts) of dc.prev -> (sums, counts, labels_prev, changed)."""
    xi, k, row0 = dc.xi, dc.k, dc.l_num
    n = len(dc.new)
    prev, sums, counts, changed = dc.prev.copy(), sums.copy(), counts.copy(), 0
    for w in range(mc.cdiv(n - row0, 64)):
        base = (0 if "no_row0" in mut else row0) + w * 64
        if base >= n or ("drop_ragged" in mut and base + 64 > n):
            continue
        for row in range(base, min(base + 64, n)):
            a, b = int(dc.new[row]), int(prev[row])
            if a == b:
                continue
            prev[row] = a
            changed += 1
            if 0 <= a < k:
                sums[a] += xi[row]
                counts[a] += 1
            if 0 <= b < k and "no_decrement" not in mut:
                sums[b] -= xi[row]
                counts[b] -= 1
    return sums, counts, prev, changed


def check_delta(dc, sums, counts, prev, changed):
    """The assertions of test_gpu_mstep on the state an incremental step leaves (integers of grid units here)."""
    rs, rc = mc.sums_counts(dc.xi, dc.new, dc.k)
    assert np.array_equal(counts, rc), dc.name
    assert np.array_equal(sums, rs), dc.name
    assert np.array_equal(prev[dc.l_num:], dc.new[dc.l_num:]), dc.name
    assert changed == int((dc.prev[dc.l_num:] != dc.new[dc.l_num:]).sum()), dc.name


def _delta(name):
    return next(dc for dc in mc.delta_cases() if dc.name == name)


@pytest.mark.parametrize("dc", mc.delta_cases(), ids=lambda d: d.name)
def test_correct_delta_model_passes(dc):
    check_delta(dc, *delta_model(dc, *mc.sums_counts(dc.xi, dc.prev, dc.k)))


DELTA_CATCHES = [("no_decrement", "one[l0]"), ("drop_ragged", "ragged[l0]"), ("no_row0", "last_row[l37]")]


@pytest.mark.parametrize("mut,name", DELTA_CATCHES)
def test_planted_delta_failure_is_caught(mut, name):
    dc = _delta(name)
    with pytest.raises(AssertionError):
        check_delta(dc, *delta_model(dc, *mc.sums_counts(dc.xi, dc.prev, dc.k), mut=(mut,)))


# ------------------------------------------------------------------------------------------------ the double-double inertia, emulated
def _dd_inertia_emulated(sc, c_in, lab, contracted):
    """finalize_kernel's inertia from the sums (unlabelled part, no labelled rows, d = 64) in IEEE double arithmetic, the fma taken
    exactly with Fractions.  contracted: dd_add_prod as it was compiled with floating-point contraction on - `a.hi + p` and `p - bb`
    fused with the product (fma(x, y, a.hi), fma(x, y, -bb)) while fma(x, y, -p) is still added."""
    from fractions import Fraction as Fr

    def fma(x, y, z):
        return float(Fr(x) * Fr(y) + Fr(z))

    def add_d(a, b):
        s = a[0] + b
        bb = s - a[0]
        e = (a[0] - (s - bb)) + (b - bb)
        lo = a[1] + e
        hi = s + lo
        return hi, lo - (hi - s)

    def add(a, b):
        return add_d(add_d(a, b[0]), b[1])

    def add_prod(a, x, y):
        p = x * y
        e = fma(x, y, -p)
        if not contracted:
            return add_d(add_d(a, p), e)
        s = fma(x, y, a[0])
        bb = s - a[0]
        lo = a[1] + ((a[0] - (s - bb)) + fma(x, y, -bb))
        hi = s + lo
        return add_d((hi, lo - (hi - s)), e)

    def wave_sum(v):
        for o in (32, 16, 8, 4, 2, 1):
            v = [add(v[i], v[i ^ o]) for i in range(64)]
        return v[0]

    s_i, cnt = mc.sums_counts(sc.xi, lab, sc.k)
    S = s_i.astype(np.float64) * mc.UNIT
    t = []
    for c in range(sc.k):
        n2 = wave_sum([add_prod((0.0, 0.0), float(c_in[c, j]), float(c_in[c, j])) for j in range(mc.D)])
        pu = wave_sum([add_prod((0.0, 0.0), float(c_in[c, j]), float(S[c, j])) for j in range(mc.D)])
        nu = float(cnt[c])
        tu = add_prod(add_prod((0.0, 0.0), nu, n2[0]), nu, n2[1])
        t.append(add_d(add_d(tu, -2.0 * pu[0]), -2.0 * pu[1]))
    t += [(0.0, 0.0)] * (8 - len(t))
    for o in (4, 2, 1):                                        # the fixed tree over the threads that hold a partial
        for i in range(o):
            t[i] = add(t[i], t[i + o])
    ex = mc.exact_inertia(sc.xi, lab, sc.k, c_in, row0=0)[1]
    one = 1 << (2 * mc.SCALE)
    x2 = Fr(ex[1], one)
    f = add((float(x2), float(x2 - Fr(float(x2)))), t[0])
    got = f[0] + f[1]
    return got, abs(Fr(got) - Fr(ex[0], one)), Fr(abs(ex[0]), one << 52) + Fr(ex[1] + ex[2] + ex[3], one << 90)


def test_contraction_degrades_the_double_double_inertia():
    """The bug test_gpu_mstep's k = 7 script found, on the CPU: the "means" step's inertia evaluated as the source of dd_add_prod reads
    meets the bound; evaluated as the contracted instruction sequence it is the value the device returned before the fix
    (0.184128197061185, 7.1e-15 off) and misses the bound by two orders of magnitude."""
    sc = mc.Scene(7, 6 * 64 + 37, 0, seed=7)
    cu = mc.scene_means(sc)
    c_in = (cu * mc.UNIT).astype(np.float32)
    lab = sc.labels(cu).astype(np.int32)
    got, err, bound = _dd_inertia_emulated(sc, c_in, lab, contracted=False)
    assert err <= bound
    got, err, bound = _dd_inertia_emulated(sc, c_in, lab, contracted=True)
    assert got == 0.184128197061185 and err > 100 * bound
