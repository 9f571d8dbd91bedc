"""The k-means++ draws, the distance update and the whole seedings against the float64 oracle on exact-grid data (tests/seeding_cases.py:
rules G, P and S make every index and every float32 the ONE right answer), on a real MI355X.  Every assertion is array_equal on
indices or on float32 / float64 bits; nothing here carries a tolerance.

  draws      ops.kpp_draw / kpp_draw_multi / the shard form (total=, prefix=, want_probsum=) against ko.kpp_draw: r on, one float32
             below and one above the prefix at thread, wave and tile borders and the last element; runs of zeros; the float32 compare
             inside a tile and on a tile sum; r = 1, r beyond the total, all zeros, NaN, inf; 1,025 tiles (the unstaged pick)
  search     ops.kpp_searchsorted against np.searchsorted on the exact float64 prefixes: targets on a prefix, u = 0, the clip, trailing
             zeros; 1, 3 and 8 draws per launch; the potential's bits
  update     ops.min_update_multi against float32(exact distance) folded by minimum: every group split of minupd_all, J = 1 / 2,
             VEC on / off, d2 from inf and one float32 either side of the distance, centres that are rows and that are not
  greedy     ops.kpp_greedy_lockstep against ko.sklearn_kpp(compat="1.0.2"), with the fp16 copy (dense rounds up to SCD_KM_FILTER_FROM,
             then the filter: every batch / group form) and without (dense), incl. first-round ties by construction and 1,025 tiles
  SSKM       ops.kpp_seed_lockstep and KMeansEngine.kpp_lockstep against ko.kpp per restart, SCD_KPP_FILTER on and off: picks, centres
             and the final d2
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import seeding_cases as sc
from oracle import kmeans_oracle as ko

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device; they must not be skipped on the GPU box"
    from scd_amd import ops as o
    return o


def dev(x):
    return torch.as_tensor(x).cuda()


def f64_dev(v):
    return torch.tensor([float(v)], dtype=torch.float64, device="cuda")


# ------------------------------------------------------------------------------------------------ draws
def _padded(rows, pad=37, fill=float("nan")):
    """[R, n] as a view of a [R, n + pad] tensor: a row stride larger than n, NaN behind every row."""
    rows = np.stack(rows)
    full = np.full((rows.shape[0], rows.shape[1] + pad), fill, dtype=F32)
    full[:, :rows.shape[1]] = rows
    return dev(full)[:, :rows.shape[1]]


def test_draw_single_vector_cases(ops):
    """Every case of seeding_cases.draw_cases through scd_kpp_draw and, as a one-row launch, through scd_kpp_draw_multi."""
    cases = sc.draw_cases()
    last, t = None, None
    bad = []
    for c in cases:
        if c.d2 is not last:
            last, t = c.d2, dev(c.d2)
        got = int(ops.kpp_draw(t, c.r)[0].item())
        got_m = int(ops.kpp_draw_multi(t.reshape(1, -1), np.array([c.r]))[0].item())
        if got != c.want or got_m != c.want:
            bad.append((c.name, float(c.r), c.want, got, got_m))
    assert not bad, "%d of %d draws differ (name, r, oracle, single, multi): %s" % (len(bad), len(cases), bad[:12])


@pytest.mark.parametrize("group", sc.multi_groups(), ids=lambda g: g[0])
def test_draw_multi_rows_differ(ops, group):
    """scd_kpp_draw_multi with a different case in every row and a row stride larger than n (NaN behind the rows)."""
    name, cases = group
    d2 = _padded([c.d2 for c in cases])
    assert d2.stride(0) > d2.shape[1] or d2.shape[0] == 1
    r = np.array([c.r for c in cases], dtype=F32)
    got = ops.kpp_draw_multi(d2, r)[0].cpu().numpy()
    want = np.array([c.want for c in cases])
    assert np.array_equal(got, want), (name, [c.name for c in cases], got.tolist(), want.tolist())
    got = ops.kpp_draw_multi(d2, dev(r))[0].cpu().numpy()                     # the uniforms already on the device
    assert np.array_equal(got, want), name


def test_draw_shards(ops):
    """The shard form: shard 0 returns the hit or -1 and its probability mass (bits), shard 1 continues from it."""
    bad = []
    for c in sc.shard_cases():
        a, b = dev(c.d2[:c.cut]), dev(c.d2[c.cut:])
        tot = f64_dev(np.sum(c.d2.astype(F64)))
        _, pa = ops.kpp_draw(a, c.r, total=tot, want_idx=False, want_probsum=True)
        ia, pa2 = ops.kpp_draw(a, c.r, total=tot, want_probsum=True)
        ib, _ = ops.kpp_draw(b, c.r, total=tot, prefix=pa)
        ia, ib = int(ia.item()), int(ib.item())
        got = ia if ia >= 0 else c.cut + ib
        ok = got == c.want and (ia >= 0) == (c.want < c.cut) and float(pa.item()) == c.probsum0 == float(pa2.item())
        # the same through the _multi entry point (two equal rows, a row stride larger than the shard)
        tm = torch.cat([tot, tot])
        am, bm = _padded([c.d2[:c.cut]] * 2), _padded([c.d2[c.cut:]] * 2)
        rr = np.array([c.r, c.r], dtype=F32)
        _, pm = ops.kpp_draw_multi(am, rr, total=tm, want_idx=False, want_probsum=True)
        iam, _ = ops.kpp_draw_multi(am, rr, total=tm)
        ibm, _ = ops.kpp_draw_multi(bm, rr, total=tm, prefix=pm)
        gm = [int(iam[j]) if int(iam[j]) >= 0 else c.cut + int(ibm[j]) for j in range(2)]
        ok = ok and gm == [c.want, c.want] and pm.cpu().tolist() == [c.probsum0] * 2
        if not ok:
            bad.append((c.name, c.want, ia, ib, float(pa.item()), c.probsum0, gm))
    assert not bad, bad[:8]


def test_draw_unstaged_tile_sums(ops):
    """n = 1,024 * 4,096 + 5, R = 2: 1,025 tiles, more than a pick block stages in LDS; the hits lie in the last tile and in tile 1,023."""
    d2, r, want = sc.staged_draw()
    t = dev(d2)
    got = ops.kpp_draw_multi(t, r)[0].cpu().numpy()
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    for j in range(2):
        sc.check_draw("staged[%d]" % j, want[j], ops.kpp_draw(t[j], r[j])[0].item())


def test_search_cases(ops):
    """scd_kpp_searchsorted on every case of seeding_cases.search_cases: indices and the float64 potential's bits."""
    bad = []
    for c in sc.search_cases():
        idx, pot = ops.kpp_searchsorted(dev(c.d2), c.u)
        try:
            sc.check_search(c, idx.cpu().numpy(), float(pot.item()))
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "%d search launches differ: %s" % (len(bad), bad[:8])


# ------------------------------------------------------------------------------------------------ the distance update
@pytest.mark.parametrize("n,d", sc.MINUPD_SHAPES + [sc.MINUPD_BIG], ids=lambda v: str(v))
def test_min_update_multi_exact(ops, n, d):
    """scd_kmeans_min_update_multi on rule-G rows: d2 = min(d2, float32(exact distance)) bit for bit, for every R of the issue (all
    group splits of minupd_all: the two-group RB = 5 launch, 4, 1; at 65,836 rows RB = 10 and two rows per thread)."""
    big = n == sc.MINUPD_BIG[0]
    for R in ((1, 10, 13) if big else sc.MINUPD_R):
        x, c, exact, start, want = sc.minupd_case(n, d, R)
        full = torch.full((R, n + 70), -1.0, dtype=torch.float32, device="cuda")      # a row stride larger than n; nothing behind a row is written
        d2 = full[:, :n]
        d2.copy_(dev(start))
        ops.min_update_multi(dev(x), dev(c), d2)
        sc.check_bits("min_update_multi[n=%d,d=%d,R=%d] groups %s" % (n, d, R, sc.minupd_groups(n, R)), want, d2.cpu().numpy())
        assert bool((full[:, n:] == -1.0).all())
        if R in (1, 13):                                      # from inf alone: the distances themselves
            d2 = torch.full((R, n), float("inf"), dtype=torch.float32, device="cuda")
            ops.min_update_multi(dev(x), dev(c), d2)
            sc.check_bits("min_update_multi[n=%d,d=%d,R=%d] from inf" % (n, d, R), exact, d2.cpu().numpy())


# ------------------------------------------------------------------------------------------------ greedy seedings
def _greedy(ops, x, first, u, k, exact16):
    xt = dev(x)
    x16 = ops.f16_exact(xt) if exact16 else None
    assert not exact16 or x16 is not None
    cent, picks = ops.kpp_greedy_lockstep(xt, x16, first, u, k)
    return cent.cpu().numpy(), picks.cpu().numpy().T


@pytest.mark.parametrize("sp", sc.GREEDY_SPECS, ids=lambda s: "%s-%dx%d-R%d-k%d" % (s.family, s.n, s.d, s.R, s.k))
def test_greedy_lockstep_equals_oracle(ops, sp):
    """scd_kpp_greedy_lockstep against ko.sklearn_kpp(compat="1.0.2") (R seedings on one stream) on rule-G rows: with the exact fp16 copy
    (dense rounds up to SCD_KM_FILTER_FROM = 4 centres, then muf_filter_kernel / kg_exact_kernel / kg_apply_kernel; at d = 96, which
    the filter does not serve, all rounds dense) and without it (dense).  Picks and centres equal the oracle's and each other."""
    x, first, u, opicks, ties = sc.greedy_case(sp)
    res = {}
    for exact16 in (True, False):
        cent, picks = _greedy(ops, x, first, u, sp.k, exact16)
        sc.check_picks("%s x16=%s" % (sp, exact16), opicks, picks)
        sc.check_bits("%s centres x16=%s" % (sp, exact16), x[opicks], cent)
        res[exact16] = (cent, picks)
    assert np.array_equal(res[True][1], res[False][1]) and np.array_equal(res[True][0].view(np.uint32), res[False][0].view(np.uint32))
    for j, (hi, lo) in ties:                                   # the constructed first-round tie went to the first candidate
        assert res[True][1][j, 1] == hi and res[False][1][j, 1] == hi


def test_greedy_filter_from_the_first_round_child(ops, tmp_path):
    """SCD_KM_FILTER_FROM = 1 in a fresh child process (the library reads it once): EVERY round goes through the filter, so the
    constructed first-round ties of the `mirror` and `duplicates` seedings are decided by kg_exact_kernel's potential differences and
    kg_apply_kernel (at the default the dense path decides them), in every batch / group form.  Picks and centres equal the oracle's."""
    idx = [i for i, sp in enumerate(sc.GREEDY_SPECS) if sp.n == 700 and sp.family in ("mirror", "duplicates")
           and sc.greedy_filter_serves(sp.d, sp.R, 2 + int(np.log(sp.k)))]
    forms = {tuple(sc.greedy_dispatch(sc.GREEDY_SPECS[i].R, 2 + int(np.log(sc.GREEDY_SPECS[i].k)))) for i in idx}
    assert len(forms) == 5
    out = str(tmp_path / "child.npz")
    e = dict(os.environ, SCD_KM_FILTER_FROM="1")
    e.pop("SCD_HIP_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "seeding_child.py"), out] + [str(i) for i in idx], env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stderr[-2000:]
    got = np.load(out)
    for i in idx:
        sp = sc.GREEDY_SPECS[i]
        x, first, u, opicks, ties = sc.greedy_case(sp)
        assert ties
        sc.check_picks("%s filter from round 1" % (sp,), opicks, got["picks_%d" % i])
        sc.check_bits("%s centres, filter from round 1" % (sp,), x[opicks], got["cent_%d" % i])


def test_greedy_lockstep_unstaged_search(ops):
    """n = 1,024 * 4,096 + 5, d = 4, k = 2, R = 2 (dense): kg_search_kernel with 1,025 tile sums, candidates in the last tile and tile 1,023."""
    x, first, u, opicks, hits = sc.greedy_big()
    cent, picks = _greedy(ops, x, first, u, 2, False)
    sc.check_picks("greedy_big", opicks, picks)
    sc.check_bits("greedy_big centres", x[opicks], cent)


# ------------------------------------------------------------------------------------------------ SSKM lock-step seedings
@pytest.mark.parametrize("sp", sc.SEED_SPECS, ids=lambda s: "%s-%dx%d-R%d-k%d" % (s.family, s.n, s.d, s.R, s.k))
def test_seed_lockstep_equals_oracle(ops, monkeypatch, sp):
    """scd_kpp_seed_lockstep and KMeansEngine.kpp_lockstep, SCD_KPP_FILTER on and off, against ko.kpp per restart on rows under rules G
    and P (asserted on the oracle's d2 before every round): the picks, the centres and the final d2."""
    from scd_amd.kmeans import KMeansEngine
    x, first, rv, opicks, worst = sc.seed_case(sp)
    assert worst >= 2.0 ** -28
    n, d, R, k = sp.n, sp.d, sp.R, sp.k
    xt = dev(x)
    x16 = ops.f16_exact(xt)
    assert x16 is not None
    want_c = np.concatenate([x[first][:, None], x[opicks]], axis=1)                                  # [R, k, d]
    want_d2 = np.stack([ko.dist_f32(x, want_c[j, :k - 1]).min(axis=1) for j in range(R)])            # the last centre is not folded in
    for filt in ("1", "0"):
        monkeypatch.setenv("SCD_KPP_FILTER", filt)
        buf = torch.zeros((R, k, d), dtype=torch.float32, device="cuda")
        buf[:, 0] = xt[torch.as_tensor(first, device="cuda")]
        d2 = torch.full((R, n), float("inf"), dtype=torch.float32, device="cuda")
        ops.min_update_multi(xt, buf[:, 0].contiguous(), d2)
        picks = ops.kpp_seed_lockstep(xt, x16, d2, dev(rv), buf, 1)
        sc.check_picks("%s filter=%s" % (sp, filt), opicks, picks.cpu().numpy().T)
        sc.check_bits("%s centres filter=%s" % (sp, filt), want_c, buf.cpu().numpy())
        sc.check_bits("%s d2 filter=%s" % (sp, filt), want_d2, d2.cpu().numpy())
        eng = KMeansEngine(k=k, n_init=R, random_state=sp.seed)
        cent = eng.kpp_lockstep(eng._be().prepare(xt), None, k, np.random.RandomState(sp.seed), R, x16=x16)
        sc.check_bits("%s engine filter=%s" % (sp, filt), want_c, cent.cpu().numpy())
