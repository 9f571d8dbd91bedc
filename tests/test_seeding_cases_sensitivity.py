"""Can the inputs of tests/seeding_cases.py tell a wrong k-means++ draw from a right one?  A small numpy model of the DOCUMENTED data flow
of the draw kernels (scd_amd/csrc/kmeans.hip, kmeans_sk_impl.h) is run on every case and judged by the checker tests/test_gpu_seeding.py
uses (`check_draw`, `check_search`, `check_picks`):
  draw      prob = float32(d2 / float32(total)); per tile of 4,096 elements the float64 sum of prob; the OWNER tile is the first whose
            running sum (from `prefix`), rounded to float32, is >= r; that tile is scanned in index order from the running sum in front of
            it, again with the float32 compare; a scan that finds nothing carries the tile's sum into the next tile; no owner: -1
  search    per tile the float64 sum of d2; pot = their sum, the target u * float64(float32(pot)); owner tile and scan as above with
            float64 `>=` (searchsorted side `left`); no owner: n - 1 (numpy's clip)
  greedy    per round and start: L candidates by the search, each candidate's potential sum_i min(d2_i, ||x_i - x_cand||^2) in float64,
            the FIRST candidate with the smallest potential is added

The correct model passes every case.  Each planted fault fails the case CATCHES names, and the test asserts exactly that:
  gt          `>` instead of `>=` (owner and scan)                   draw   prefix[n=4097],i=4095,on (r on a tile's last prefix)
  owner_f64   the owner tile chosen with a float64 compare            draw   f32cmp_tile_sum - and NO other case but its twin catches it
  no_carry    the running sum in front of the owner tile dropped      draw   prefix[n=4097],i=4096,on (the hit is the first entry of tile 1)
  zero_last   a run of equal prefixes resolved to its last index      draw   zeros_across[n=8192],flat; search zeros_across
  side_right  searchsorted side `right`                               search prefix[n=4097],i=4095 (the target on tile 0's last prefix)
  pot_f64     pot not rounded through float32                         search clip[n=257] (the last non-zero entry instead of n - 1)
  no_clip     the clip missing (n instead of n - 1)                   search clip[n=257]
  tie_last    candidate ties given to the last candidate              greedy the first round of the `mirror` and `duplicates` seedings
(The scan's carry INTO THE NEXT tile cannot be planted: under rule P the owner tile's last running sum is the very value the owner
search compared, so the scan always ends in the owner tile; the kernels keep that loop for data whose sums depend on the association.)
The model is not the kernel; what is asserted on the device is asserted there on the device's own output.
"""
import numpy as np
import pytest

import seeding_cases as sc
from oracle import kmeans_oracle as ko

F32, F64 = np.float32, np.float64


def _tiles(v):
    nb = -(-len(v) // sc.TILE)
    pad = np.zeros(nb * sc.TILE, dtype=F64)
    pad[:len(v)] = v
    return pad.reshape(nb, sc.TILE)


def _scan(tiles, n, owner, pre, hit_fn, mut):
    """The in-tile scan from tile `owner` on: -> the index found, or None."""
    for b in range(owner, len(tiles)):
        cum = pre + np.cumsum(tiles[b])
        hit = hit_fn(cum) & (np.arange(sc.TILE) < n - b * sc.TILE)
        at = np.nonzero(hit)[0]
        if at.size:
            i = int(at[0])
            if "zero_last" in mut:
                same = np.nonzero((cum == cum[i]) & (np.arange(sc.TILE) < n - b * sc.TILE))[0]
                i = int(same[-1])
            return b * sc.TILE + i
        pre = cum[-1]
    return None


def draw_model(d2, r, mut=(), total=None, prefix=0.0):
    """-> (index or -1, the probability mass of the vector)"""
    d2 = np.asarray(d2, dtype=F32)
    r = F32(r)
    with np.errstate(all="ignore"):
        tot = F32(np.sum(d2.astype(F64)) if total is None else total)
        tiles = _tiles((d2 / tot).astype(F32).astype(F64))
        psum = tiles.sum(axis=1)
        ge = (lambda a, b: a > b) if "gt" in mut else (lambda a, b: a >= b)
        run, owner, opre = F64(prefix), -1, 0.0
        for b in range(len(psum)):
            nxt = run + psum[b]
            if owner < 0 and (ge(nxt, F64(r)) if "owner_f64" in mut else ge(F32(nxt), r)):
                owner, opre = b, run
            run = nxt
        if owner < 0:
            return -1, run - prefix
        got = _scan(tiles, len(d2), owner, 0.0 if "no_carry" in mut else opre, lambda cum: ge(cum.astype(F32), r), mut)
    return (-1 if got is None else got), run - prefix


def search_model(d2, u, mut=()):
    """-> (indices [L], pot)"""
    d64 = np.asarray(d2, dtype=F32).astype(F64)
    n = len(d64)
    tiles = _tiles(d64)
    bsum = tiles.sum(axis=1)
    pot = float(bsum.sum())
    ge = (lambda a, b: a > b) if "side_right" in mut else (lambda a, b: a >= b)
    out = []
    for uu in np.atleast_1d(u):
        rv = uu * (pot if "pot_f64" in mut else F64(F32(pot)))
        pre = np.cumsum(bsum)
        own = np.nonzero(ge(pre, rv))[0]
        got = None
        if own.size:
            owner = int(own[0])
            got = _scan(tiles, n, owner, pre[owner] - bsum[owner], lambda cum: ge(cum, rv), mut)
        out.append((n if "no_clip" in mut else n - 1) if got is None else got)
    return np.array(out), pot


def greedy_model(x, first, u, k, mut=()):
    """-> picks [R, k]"""
    picks = []
    for j in range(len(first)):
        p = [int(first[j])]
        d2 = ko.dist_f32(x, x[p[0]][None])[:, 0]
        for t in range(k - 1):
            cand, _ = search_model(d2, u[j, t])
            dc = np.minimum(d2[None, :], ko.dist_f32(x[cand], x))
            pots = dc.astype(F64).sum(axis=1)
            best = int(np.nonzero(pots == pots.min())[0][-1]) if "tie_last" in mut else int(np.argmin(pots))
            p.append(int(cand[best]))
            d2 = dc[best]
        picks.append(p)
    return np.array(picks)


# ------------------------------------------------------------------------------------------------ the correct model passes
def _draw_failures(mut):
    bad = []
    for c in sc.draw_cases():
        try:
            sc.check_draw(c.name, c.want, draw_model(c.d2, c.r, mut)[0])
        except AssertionError:
            bad.append(c.name)
    return bad


def test_correct_draw_model_passes():
    assert _draw_failures(()) == []
    for c in sc.shard_cases():
        a, b = c.d2[:c.cut], c.d2[c.cut:]
        tot = float(np.sum(c.d2.astype(F64)))
        ia, pa = draw_model(a, c.r, total=tot)
        ib, _ = draw_model(b, c.r, total=tot, prefix=pa)
        assert pa == c.probsum0
        sc.check_draw(c.name, c.want, ia if ia >= 0 else c.cut + ib)
        assert (ia >= 0) == (c.want < c.cut)
    d2, r, want = sc.staged_draw()
    for j in range(2):
        sc.check_draw("staged[%d]" % j, want[j], draw_model(d2[j], r[j])[0])


def test_correct_search_model_passes():
    for c in sc.search_cases():
        sc.check_search(c, *search_model(c.d2, c.u))


GREEDY_SMALL = [sp for sp in sc.GREEDY_SPECS if sp.n == 700 and sp.d == 128 and sp.k == 8 and sp.R <= 5]


@pytest.mark.parametrize("sp", GREEDY_SMALL, ids=lambda s: "%s-R%d" % (s.family, s.R))
def test_correct_greedy_model_passes(sp):
    x, first, u, picks, ties = sc.greedy_case(sp)
    sc.check_picks(str(sp), picks, greedy_model(x, first, u, sp.k))


def test_case_lists_reach_every_dispatch():
    """The draw lengths and borders of the issue, the staged threshold, every group split of the distance update and every batch / group
    form of the greedy filter rounds."""
    names = {c.name for c in sc.draw_cases()}
    for n in sc.LENGTHS:
        for i in sorted({b for b in sc.BORDERS if b < n} | {n - 1}):
            assert {"prefix[n=%d],i=%d,%s" % (n, i, how) for how in ("on", "below", "above")} <= names
    assert -(-sc.N_STAGED // sc.TILE) == sc.STAGE + 1
    assert {len(cs) for _, cs in sc.multi_groups()} == {1, 2, 10, 16}
    assert {len(c.u) for c in sc.search_cases()} == {1, 3, 8}
    launches = set()
    for n, d in sc.MINUPD_SHAPES:
        for R in sc.MINUPD_R:
            launches.update(sc.minupd_groups(n, R))
    assert launches == {(5, 2), (4, 1), (1, 1)} and sc.minupd_groups(255, 13) == [(5, 2), (4, 1)] and sc.minupd_groups(255, 20) == [(5, 2), (5, 2)]
    assert sc.minupd_groups(sc.MINUPD_BIG[0], 13) == [(10, 1), (4, 1)] and -(-sc.MINUPD_BIG[0] // 256) >= 256
    assert {d % 4 == 0 for _, d in sc.MINUPD_SHAPES} == {True, False}
    forms = set()
    for sp in sc.GREEDY_SPECS:
        L = 2 + int(np.log(sp.k))
        if sc.greedy_filter_serves(sp.d, sp.R, L):
            forms.add(tuple(sc.greedy_dispatch(sp.R, L)))
    assert forms == {((4, 1),), ((20, 2),), ((40, 4),), ((64, 4), (6, 1)), ((64, 4),) * 4}
    assert {(sp.family, sp.d, sp.n) for sp in sc.GREEDY_SPECS} >= {(f, d, n) for f in sc.FAMILIES for d in (128, 768) for n in (700, 4100)}
    assert any(not sc.greedy_filter_serves(sp.d, sp.R, 2 + int(np.log(sp.k))) for sp in sc.GREEDY_SPECS)
    assert {sp.R for sp in sc.SEED_SPECS} == {1, 10, 16} and {sp.d for sp in sc.SEED_SPECS} == {128, 512, 768}
    assert {sp.n for sp in sc.SEED_SPECS} == {700, 4100} and min(sp.k for sp in sc.SEED_SPECS) >= 12
    assert {sp.family for sp in sc.SEED_SPECS} == set(sc.FAMILIES)


# ------------------------------------------------------------------------------------------------ planted faults
DRAW_CATCHES = [("gt", "prefix[n=4097],i=4095,on"), ("owner_f64", "f32cmp_tile_sum"), ("no_carry", "prefix[n=4097],i=4096,on"),
                ("zero_last", "zeros_across[n=8192],flat"), ("zero_last", "zeros_leading[n=8192,z=4100],r=0")]
SEARCH_CATCHES = [("side_right", "prefix[n=4097],i=4095"), ("pot_f64", "clip[n=257]"), ("no_clip", "clip[n=257]"), ("zero_last", "zeros_across")]


@pytest.mark.parametrize("mut,name", DRAW_CATCHES)
def test_planted_draw_fault_is_caught(mut, name):
    c = sc.draw_by_name(name)
    with pytest.raises(AssertionError):
        sc.check_draw(name, c.want, draw_model(c.d2, c.r, (mut,))[0])


def test_only_the_tile_sum_case_sees_a_float64_owner_compare():
    """Under rule P a float64 and a float32 owner compare differ only where a tile's running sum crosses r by the rounding: the two
    f32cmp_tile_sum cases are what pins the float32 compare of the owner search."""
    assert _draw_failures(("owner_f64",)) == ["f32cmp_tile_sum", "f32cmp_tile_sum_2"]


@pytest.mark.parametrize("mut,name", SEARCH_CATCHES)
def test_planted_search_fault_is_caught(mut, name):
    c = sc.search_by_name(name)
    with pytest.raises(AssertionError):
        sc.check_search(c, *search_model(c.d2, c.u, (mut,)))


def test_clip_case_tells_the_three_answers_apart():
    """clip[n=257]: n - 1 = 256 (right), 200 (pot not rounded through float32: the target stays below the last prefix), 257 (no clip)."""
    c = sc.search_by_name("clip[n=257]")
    assert search_model(c.d2, c.u)[0][0] == 256
    assert search_model(c.d2, c.u, ("pot_f64",))[0][0] == 200
    assert search_model(c.d2, c.u, ("no_clip",))[0][0] == 257


@pytest.mark.parametrize("sp", [sp for sp in GREEDY_SMALL if sp.family in ("mirror", "duplicates")], ids=lambda s: s.family)
def test_planted_tie_fault_is_caught(sp):
    x, first, u, picks, ties = sc.greedy_case(sp)
    assert ties
    got = greedy_model(x, first, u, sp.k, ("tie_last",))
    for j, (hi, lo) in ties:
        assert picks[j, 1] == hi and got[j, 1] == lo
    with pytest.raises(AssertionError):
        sc.check_picks(str(sp), picks, got)


def test_rule_helpers_reject_what_breaks_the_rules():
    with pytest.raises(AssertionError):
        ko.rule_p(np.array([1.0, 3.0, 1e-12], dtype=F32))                  # a probability below 2^-52's grid
    with pytest.raises(AssertionError):
        sc.assert_rule_g(np.full((2, 768), 74))                           # 768 * 148^2 >= 2^24
    with pytest.raises(AssertionError):
        sc.assert_rule_g(np.array([[4097, 0]]))                           # not exact in fp16 (and beyond 2,048)
    assert sc.limit_g(768) == 73 and sc.limit_g(128) == 181
