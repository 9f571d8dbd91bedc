"""Inputs and exact references for the k-means++ seedings: the draw (scd_amd/csrc/kmeans.hip: kpp_tile_sum / kpp_tile_prob / kpp_pick and
their _multi forms), the scikit-learn candidate search (kpp_search_kernel, kmeans_sk_impl.h: kg_search_kernel), the distance update
(minupd_tile_kernel) and the whole seedings (scd_kpp_seed_lockstep, scd_kpp_greedy_lockstep).  numpy only, deterministic.

On random floats none of this has ONE right answer: the kernels sum a tile tree where numpy sums sequentially.  Every case here is built so
that it has, and the builders assert the rule they rely on:

  Rule G (rows)    coordinates are integers times UNIT = 2^-7, exact in fp16, and D (2 max|int|)^2 < 2^24: every squared distance is an
                   integer below 2^24 grid units - exact in float32, its float64 sum exact in any order, so float32(float64 distance) is
                   unique; potentials (float64 sums of at most 2^29 such values) are exact in any order, atomic or not, and two candidates
                   with equal potentials are a REAL tie, which np.argmin and kg_best_of both give to the first candidate.  `assert_rule_g`.
  Rule P (SSKM draw, prob = d2 / float32(sum))
                   the float32 probabilities are multiples of 2^-52 with a total below 2, so every prefix is exact in float64 in any
                   association and oracle.kmeans_oracle.kpp_draw's sequential cumsum is the one right answer.  Every non-zero
                   d2 >= 2^-28 sum(d2) is sufficient (asserted for the whole seedings, before every round); the hand-built vectors are
                   small integers with a power-of-two total (`dyadic`).  `ko.rule_p`.
  Rule S (scikit-learn draw, searchsorted(cumsum_f64(d2), u * float32(pot)))
                   d2 are integers of grid units, so the float64 prefixes are exact; u = prefix / pot with pot a power of two, so that
                   u * pot lands exactly on a prefix.  `search_cases` asserts it.

The draw kernels work on tiles of TILE = 4,096 elements, thread t of 1,024 owning elements 4 t .. 4 t + 3, a wave 256; a pick / search
block stages the per-tile sums in LDS up to STAGE = 1,024 tiles and reads them from global memory beyond (n > 4,194,304).
"""
import collections

import numpy as np

from oracle import kmeans_oracle as ko

F32, F64 = np.float32, np.float64
TILE, STAGE = 4096, 1024
UNIT_LOG2 = -7
UNIT = 2.0 ** UNIT_LOG2
LENGTHS = (1, 4, 255, 256, 257, 4095, 4096, 4097, 8192, 12289)
BORDERS = (0, 3, 4, 255, 256, 4095, 4096)                       # thread, wave and tile borders; n - 1 is added per length
N_STAGED = STAGE * TILE + 5                                     # the first tile count the LDS stage does not hold: 1,025

_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def next_f32(v, up):
    return np.nextafter(F32(v), F32(np.inf if up else -np.inf), dtype=F32)


# ------------------------------------------------------------------------------------------------ draw vectors (rule P)
DrawCase = collections.namedtuple("DrawCase", "name d2 r want")
ShardCase = collections.namedtuple("ShardCase", "name d2 r cut want probsum0")


def dyadic(n, seed, zeros=(), hi=8):
    """float32 [n]: integers in [1, hi) (0 on the index ranges `zeros`), raised evenly until the total is a power of two <= 2^24.
    prob = d2 / total and every prefix are then exact in float32."""
    rs = np.random.RandomState(seed)
    m = rs.randint(1, hi, size=n).astype(np.int64)
    live = np.ones(n, dtype=bool)
    for a, b in zeros:
        live[a:b] = False
    m[~live] = 0
    idx = np.nonzero(live)[0]
    assert idx.size
    s = int(m.sum())
    tot = 1 << (s - 1).bit_length()
    rem = tot - s
    m[idx] += rem // idx.size
    m[idx[:rem % idx.size]] += 1
    assert int(m.sum()) == tot <= 1 << 24 and (m[idx] > 0).all()
    return m.astype(F32)


def probs(d2):
    d2 = np.asarray(d2, dtype=F32)
    return (d2 / F32(np.sum(d2.astype(F64)))).astype(F32).astype(F64)


def prefixes(d2):
    """The exact float64 prefixes of the draw's probabilities (rule P asserted) - each also an exact float32 for a `dyadic` vector."""
    ko.rule_p(d2)
    return np.cumsum(probs(d2))


def draw_want(d2, r):
    with np.errstate(all="ignore"):
        return ko.kpp_draw(d2, r)


def _draw(name, d2, r, expect=None, rule=True):
    d2 = np.ascontiguousarray(d2, dtype=F32)
    if rule:
        ko.rule_p(d2)
    want = draw_want(d2, r)
    assert expect is None or want == expect, (name, want, expect)
    return DrawCase(name, d2, F32(r), want)


def _next_live(d2, i):
    nz = np.nonzero(d2[i + 1:] > 0)[0]
    return i + 1 + int(nz[0]) if nz.size else -1


def _on_prefix(tag, d2, i):
    """r on the prefix at i (d2[i] > 0), one float32 below and one above: i, i, and the next index with a non-zero entry (-1: none)."""
    pre = prefixes(d2)
    r = F32(pre[i])
    assert float(r) == pre[i] and d2[i] > 0
    return [_draw("%s,i=%d,on" % (tag, i), d2, r, i),
            _draw("%s,i=%d,below" % (tag, i), d2, next_f32(r, False), i),
            _draw("%s,i=%d,above" % (tag, i), d2, next_f32(r, True), _next_live(d2, i))]


F32CMP = [2.0 ** 24] * 31 + [2.0 ** 24 - 1, 1.0] + [2.0 ** 24] * 32      # prefix at 31: 0.5 - 2^-30, a float32 0.5; total 2^30


def _f32cmp(n, at):
    d2 = np.zeros(n, dtype=F32)
    d2[at:at + len(F32CMP)] = F32CMP
    pre = np.cumsum(probs(d2))
    assert pre[at + 31] < 0.5 and F32(pre[at + 31]) == F32(0.5) and pre[at + 32] == 0.5
    return d2


def draw_cases():
    """Every single-vector case but the staged one (which `staged_draw` builds): see the module docstring of test_gpu_seeding."""
    return _cached("draw", _draw_cases)


def _draw_cases():
    out = []
    for n in LENGTHS:
        d2 = dyadic(n, seed=n)
        for i in sorted({b for b in BORDERS if b < n} | {n - 1}):
            out += _on_prefix("prefix[n=%d]" % n, d2, i)
    # runs of zeros before, across and behind a tile border: r on the flat prefix -> the entry in front of the run (the first index of
    # the run of EQUAL prefixes); one float32 above -> the first entry behind it
    for tag, (a, b) in (("before", (4000, 4090)), ("across", (4090, 4100)), ("behind", (4096, 4200))):
        for n in (8192, 12289):
            d2 = dyadic(n, seed=n + a, zeros=((a, b),))
            pre = prefixes(d2)
            r = F32(pre[a - 1])
            assert pre[b - 1] == pre[a - 1] == float(r)
            out.append(_draw("zeros_%s[n=%d],flat" % (tag, n), d2, r, a - 1))
            out.append(_draw("zeros_%s[n=%d],above" % (tag, n), d2, next_f32(r, True), b))
    for n, z in ((257, 5), (8192, 4096), (8192, 4100)):
        d2 = dyadic(n, seed=n + z, zeros=((0, z),))
        out.append(_draw("zeros_leading[n=%d,z=%d],r=0" % (n, z), d2, 0.0, 0))
        out.append(_draw("zeros_leading[n=%d,z=%d],tiny" % (n, z), d2, F32(2.0 ** -30), z))
    # the float32 compare: a prefix below r in float64 that equals r as a float32
    out.append(_draw("f32cmp_in_tile", _f32cmp(4096, 100), 0.5, 131))
    out.append(_draw("f32cmp_in_tile_2", _f32cmp(12289, 4096 + 1000), 0.5, 4096 + 1031))
    out.append(_draw("f32cmp_tile_sum", _f32cmp(8192, 4096 - 32), 0.5, 4095))          # tile 0 sums to 0.5 - 2^-30
    out.append(_draw("f32cmp_tile_sum_2", _f32cmp(12289, 8192 - 32), 0.5, 8191))
    # other edges
    d2 = dyadic(257, seed=1, zeros=((250, 257),))
    out.append(_draw("total_one,r=1", d2, 1.0, 249))
    out.append(_draw("beyond_total", d2, next_f32(1.0, True), -1))
    d2 = dyadic(4097, seed=2)
    out.append(_draw("total_one[n=4097],r=1", d2, 1.0, 4096))
    out.append(_draw("beyond_total[n=4097]", d2, 1.5, -1))
    out.append(_draw("all_zero,r=0.5", np.zeros(256, dtype=F32), 0.5, rule=False))
    out.append(_draw("all_zero,r=0", np.zeros(4097, dtype=F32), 0.0, rule=False))
    for tag, bad in (("nan", np.nan), ("inf", np.inf)):
        for at in (100, 4096):
            d2 = dyadic(4097, seed=3)
            d2[at] = bad
            out.append(_draw("%s[at=%d]" % (tag, at), d2, 0.25, -1, rule=False))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def draw_by_name(name):
    return next(c for c in draw_cases() if c.name == name)


def shard_cases():
    """A vector cut in two shards (`total=` / `prefix=` / `want_probsum=`): the cut on a tile border and one behind it, the hit on the
    last row of shard 0 and on the first row of shard 1 (and one float32 either side)."""
    def build():
        out = []
        for n, cut in ((12289, 4096), (12289, 4097), (8192, 4096), (8192, 4097)):
            d2 = dyadic(n, seed=n + cut)
            pre = prefixes(d2)
            for tag, i in (("last_of_0", cut - 1), ("first_of_1", cut)):
                for how, r in (("on", F32(pre[i])), ("below", next_f32(pre[i], False)), ("above", next_f32(pre[i], True))):
                    want = draw_want(d2, r)
                    assert want == (i + 1 if how == "above" else i)
                    out.append(ShardCase("shard[n=%d,cut=%d],%s,%s" % (n, cut, tag, how), d2, r, cut, want, float(pre[cut - 1])))
        return out
    return _cached("shard", build)


def multi_groups():
    """(name, cases of one length) for the _multi form: R = 1, 2, 10, 16, a different case per row."""
    def build():
        by_n = collections.defaultdict(list)
        for c in draw_cases():
            by_n[len(c.d2)].append(c)
        out = []
        for n, R, step in ((4097, 1, 1), (4097, 2, 5), (4097, 10, 2), (4097, 16, 1), (12289, 10, 3), (8192, 16, 1), (257, 16, 1), (1, 2, 1)):
            pool = by_n[n][::step]
            assert len(pool) >= R, (n, R, len(pool))
            out.append(("multi[n=%d,R=%d]" % (n, R), pool[:R]))
        return out
    return _cached("multi", build)


def staged_draw():
    """R = 2 vectors of N_STAGED elements (1,025 tiles: the pick block reads the tile sums from global memory); the hit lies in the last
    tile for row 0 and in tile 1,023 - the last one a stage would hold - for row 1.  -> (d2 [2, n], r [2], want [2])"""
    def build():
        n = N_STAGED
        hits = (n - 2, (STAGE - 1) * TILE + 17)
        d2 = np.stack([dyadic(n, seed=j, hi=4) for j in range(2)])
        r = np.array([F32(prefixes(d2[j])[hits[j]]) for j in range(2)], dtype=F32)
        want = [draw_want(d2[j], r[j]) for j in range(2)]
        assert tuple(want) == hits and hits[0] // TILE == STAGE and hits[1] // TILE == STAGE - 1
        return d2, r, np.array(want)
    return _cached("staged", build)


# ------------------------------------------------------------------------------------------------ search vectors (rule S)
SearchCase = collections.namedtuple("SearchCase", "name d2 u want pot")


def search_want(d2, u):
    d64 = np.asarray(d2, dtype=F32).astype(F64)
    pot = F64(F32(d64.sum()))
    return np.clip(np.searchsorted(np.cumsum(d64), np.asarray(u, dtype=F64) * pot), None, len(d64) - 1)


def _search(name, ints, u, expect=None):
    """ints: the distances in grid units^2 (integers: every float64 prefix is exact in any order)."""
    ints = np.asarray(ints, dtype=np.int64)
    assert ints.min() >= 0 and ints.max() < 1 << 24 and int(ints.sum()) < 1 << 53
    d2 = (ints.astype(F32) * F32(UNIT * UNIT))
    assert np.array_equal(d2.astype(F64) / (UNIT * UNIT), ints)
    u = np.atleast_1d(np.asarray(u, dtype=F64))
    want = search_want(d2, u)
    assert expect is None or np.array_equal(want, expect), (name, want, expect)
    return SearchCase(name, d2, u, want, float(int(ints.sum())) * UNIT * UNIT)


def _u_on(ints, i):
    """u with u * float32(pot) exactly on the prefix at i (pot a power of two), one float64 below and one above."""
    tot = int(ints.sum())
    assert tot & (tot - 1) == 0
    pre = int(ints[:i + 1].sum())
    u = pre / tot
    assert u * tot == pre
    return [u, np.nextafter(u, 0.0), np.nextafter(u, 2.0)]


def search_cases():
    return _cached("search", _search_cases)


def _search_cases():
    out = []
    for n in LENGTHS:
        ints = dyadic(n, seed=100 + n).astype(np.int64)
        idx = sorted({b for b in BORDERS if b < n} | {n - 1})
        for i in idx:                                                   # three draws per launch
            nxt = _next_live(ints, i)
            out.append(_search("prefix[n=%d],i=%d" % (n, i), ints, _u_on(ints, i), [i, i, nxt if nxt >= 0 else n - 1]))
        out.append(_search("u=0[n=%d]" % n, ints, [0.0], [0]))           # one draw
        if len(idx) == 8:                                                # eight
            out.append(_search("eight[n=%d]" % n, ints, [_u_on(ints, i)[0] for i in idx], idx))
    for tag, (a, b) in (("before", (4000, 4090)), ("across", (4090, 4100)), ("behind", (4096, 4200))):
        ints = dyadic(8192, seed=200 + a, zeros=((a, b),)).astype(np.int64)
        out.append(_search("zeros_%s" % tag, ints, _u_on(ints, a - 1), [a - 1, a - 1, b]))      # side `left`: the head of the flat run
    ints = dyadic(8192, seed=7, zeros=((0, 4100),)).astype(np.int64)
    out.append(_search("zeros_leading", ints, [0.0, np.nextafter(0.0, 1.0), 2.0 ** -30], [0, 4100, 4100]))
    ints = dyadic(4097, seed=8, zeros=((4000, 4097),)).astype(np.int64)
    out.append(_search("zeros_trailing", ints, [1.0, np.nextafter(1.0, 0.0), _u_on(ints, 3999)[0]], [3999, 3999, 3999]))
    # the clip: the sum 2^24 + 3 is no float32 and rounds UP to 2^24 + 4: u * pot passes the last prefix and searchsorted returns n
    for n, last in ((257, 200), (4100, 4097), (8192, 4000)):
        ints = np.zeros(n, dtype=np.int64)
        ints[0], ints[last // 2], ints[last] = 1 << 23, 1 << 23, 3
        assert F32(float(ints.sum())) == F32(2.0 ** 24 + 4)
        u = np.nextafter(1.0, 0.0)
        assert u * (2.0 ** 24 + 4) > ints.sum() and np.searchsorted(np.cumsum(ints.astype(F64)), u * float(ints.sum())) == last
        out.append(_search("clip[n=%d]" % n, ints, [u, 0.5, 0.25], [n - 1, last // 2, 0]))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def search_by_name(name):
    return next(c for c in search_cases() if c.name == name)


# ------------------------------------------------------------------------------------------------ rows (rule G)
def limit_g(d):
    """The largest |integer| a coordinate may have at dimension d."""
    m = int(np.sqrt((2 ** 24 - 1) / d) / 2)
    while d * (2 * (m + 1)) ** 2 < 2 ** 24:
        m += 1
    return min(m, 2048)


def assert_rule_g(xi, *more):
    """Rule G for the integer rows xi (and further integer rows, e.g. centres, of the same dimension); -> the float32 rows."""
    xi = np.asarray(xi, dtype=np.int64)
    d = xi.shape[1]
    m = max(int(np.abs(v).max(initial=0)) for v in (xi,) + more)
    assert all(np.asarray(v).shape[1] == d for v in more)
    assert d * (2 * m) ** 2 < 2 ** 24 and m <= 2048, (d, m)
    x = xi.astype(F32) * F32(UNIT)
    assert np.array_equal(x.astype(F64) / UNIT, xi) and np.array_equal(x.astype(np.float16).astype(F32), x)
    return x


def exact_d2(xi, ci):
    """float32 [n, k]: the one right float32(float64 squared distance) of integer rows and centres under rule G."""
    x, c = np.asarray(xi, dtype=F64), np.asarray(ci, dtype=F64)
    g = (x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * (x @ c.T)        # integers below 2^24: exact
    assert g.min(initial=0) >= 0 and g.max(initial=0) < 2 ** 24
    out = (g * (UNIT * UNIT)).astype(F32)
    assert np.array_equal(out.astype(F64), g * (UNIT * UNIT))
    return out


def mirror(n, d, seed=0, first=0):
    """Every row also present negated; the origin row at index `first` (n even: one more origin row).  From the origin, d2 is symmetric
    and the candidates x and -x have equal potentials.  -> (xi, partner): partner[i] = the index of row i's negative."""
    rs = np.random.RandomState(seed)
    h = (n - 1) // 2
    b = min(6, limit_g(d))
    half = rs.randint(-b, b + 1, size=(h, d))
    half[np.abs(half).sum(1) == 0, 0] = 1
    xi = np.concatenate([half, -half, np.zeros((n - 2 * h, d), dtype=half.dtype)])
    partner = np.concatenate([np.arange(h) + h, np.arange(h), np.arange(2 * h, n)])
    perm = rs.permutation(n)
    o = int(np.nonzero(perm == 2 * h)[0][0])                  # where the (first) origin row went
    perm[[o, first]] = perm[[first, o]]
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    xi, partner = xi[perm], inv[partner[perm]]
    assert not xi[first].any() and np.array_equal(xi[partner], -xi)
    return xi.astype(np.int64), partner


def duplicates(n, d, seed=0):
    """A third of the rows are repeats of earlier ones: runs of d2 = 0 and candidates with equal rows.  -> (xi, partner): partner[i] =
    another index with the same row (i itself where there is none)."""
    rs = np.random.RandomState(seed)
    nb = n - n // 3
    b = min(6, limit_g(d))
    base = rs.randint(-b, b + 1, size=(nb, d))
    src = rs.choice(nb, n - nb, replace=False)
    xi = np.concatenate([base, base[src]])
    partner = np.arange(n)
    partner[src], partner[nb:] = np.arange(nb, n), src
    perm = rs.permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    xi, partner = xi[perm], inv[partner[perm]]
    assert np.array_equal(xi[partner], xi) and (partner != np.arange(n)).sum() == 2 * (n - nb)
    return xi.astype(np.int64), partner


def lattice(n, d, seed=0):
    """Coordinates in {-1, 0, 1}: squared distances are small integers, equal for many pairs of rows."""
    rs = np.random.RandomState(seed)
    return rs.randint(-1, 2, size=(n, d)).astype(np.int64), None


def blobs(n, d, seed=0):
    """Twelve clusters on the grid, noise +-3 per coordinate: the ordinary case."""
    rs = np.random.RandomState(seed)
    b = min(40, limit_g(d) - 3)
    cent = rs.randint(-b, b + 1, size=(12, d))
    return (cent[rs.randint(0, 12, size=n)] + rs.randint(-3, 4, size=(n, d))).astype(np.int64), None


FAMILIES = {"mirror": mirror, "duplicates": duplicates, "lattice": lattice, "blobs": blobs}


def rows(family, n, d, seed=0, **kw):
    """-> (xi int64 [n, d], x float32 [n, d] (rule G asserted), partner or None)"""
    def build():
        xi, partner = FAMILIES[family](n, d, seed, **kw)
        return xi, assert_rule_g(xi), partner
    return _cached(("rows", family, n, d, seed, tuple(sorted(kw.items()))), build)


# ------------------------------------------------------------------------------------------------ the distance update
MINUPD_SHAPES = [(1, 5), (127, 3), (129, 33), (255, 64), (257, 130), (4100, 768)]
MINUPD_R = (1, 2, 3, 5, 9, 10, 13, 16, 20)
MINUPD_BIG = (65536 + 300, 32)                 # cdiv(n, 256) >= 256: two rows per thread (J = 2); R = 1, 10 (RB = 10) and 13 (RB = 10, 4)


def minupd_groups(n, R, L=1):
    """The launches minupd_all makes for R centres: (RB, groups in the launch) in order."""
    out, r0 = [], 0
    while R - r0 >= 10 and -(-n // 128) * L <= 256:
        out.append((5, 2)); r0 += 10
    while R - r0 >= 10:
        out.append((10, 1)); r0 += 10
    while R - r0 >= 3:
        out.append((4, 1)); r0 += 4
    while R - r0 >= 1:
        out.append((1, 1)); r0 += 1
    return out


def minupd_case(n, d, R, seed=0):
    """Rule-G rows, R centres (even: rows of x; odd: grid points that are no rows), the exact float32 distances [R, n] and a start
    d2 [R, n] that cycles, element by element, through inf, one float32 above the exact distance, the distance itself, one below."""
    def build():
        rs = np.random.RandomState(seed + n + d)
        b = min(30, limit_g(d))
        xi = rs.randint(-b, b + 1, size=(n, d)).astype(np.int64)
        ci = xi[rs.randint(0, n, size=R)].copy()
        off = rs.randint(-b, b + 1, size=(R, d))
        ci[1::2] = off[1::2]
        x, c = assert_rule_g(xi, ci), assert_rule_g(ci, xi)
        exact = exact_d2(xi, ci).T.copy()
        assert (exact[::2] == 0).any(axis=1).all()
        mode = (np.arange(R * n).reshape(R, n) + rs.randint(0, 4)) % 4
        up, down = np.nextafter(exact, F32(np.inf)), np.where(exact > 0, np.nextafter(exact, F32(-np.inf)), exact)
        start = np.select([mode == 0, mode == 1, mode == 2], [np.full_like(exact, np.inf), up, exact], down).astype(F32)
        return x, c, exact, start, np.minimum(start, exact)
    return _cached(("minupd", n, d, R, seed), build)


# ------------------------------------------------------------------------------------------------ SSKM seedings (rules G and P)
SeedSpec = collections.namedtuple("SeedSpec", "family n d R k seed")
SEED_SPECS = [SeedSpec(list(FAMILIES)[(i + j + l) % 4], n, d, R, 12 + (i + 2 * j + l) % 5, 9 * i + 3 * j + l)
              for i, R in enumerate((1, 10, 16)) for j, d in enumerate((128, 512, 768)) for l, n in enumerate((700, 4100))]


def seed_case(sp):
    """The R restarts of an SSKM seeding on ONE RandomState(sp.seed), as K_Means._run consumes it (randint, then k - 1 uniforms, per
    restart): -> x, first [R], rv float32 [k - 1, R], the oracle's picks [R, k - 1] and the worst rule-P ratio over all rounds."""
    def build():
        _, x, _ = rows(sp.family, sp.n, sp.d, seed=sp.seed)
        rs = np.random.RandomState(sp.seed)
        first, rv = np.empty(sp.R, dtype=np.int64), np.empty((sp.R, sp.k - 1))
        for j in range(sp.R):
            first[j] = rs.randint(0, sp.n)
            rv[j] = rs.rand(sp.k - 1)
        rs = np.random.RandomState(sp.seed)
        picks, worst = [], []

        def rule(d2):
            ratio = ko.rule_p(d2)
            assert ratio >= 2.0 ** -28, (sp, ratio)
            worst.append(ratio)
        for j in range(sp.R):
            trace = []
            c = ko.kpp(x, None, sp.k, rs, trace, before_draw=rule)
            assert np.array_equal(c, x[[first[j]] + trace])
            picks.append(trace)
        return x, first, np.ascontiguousarray(rv.T.astype(F32)), np.array(picks), min(worst)
    return _cached(("seed", sp), build)


# ------------------------------------------------------------------------------------------------ greedy seedings (rule G)
GreedySpec = collections.namedtuple("GreedySpec", "family n d R k seed")
# (R, k) -> M = R L candidates per round: the filter's dispatch (batches of 64 candidates, 1 / 2 / 4 groups of 16 in a batch)
#   (1, 8)    L = 4, M = 4     one batch, one group
#   (5, 8)    M = 20           one batch, two groups
#   (10, 8)   M = 40           one batch, four groups
#   (10, 150) L = 7, M = 70    a four-group batch and a second batch of 6 candidates: one group
#   (64, 8)   M = 256          four four-group batches: the R L <= 256 limit
GREEDY_SPECS = ([GreedySpec(f, n, d, R, 8, 100 * i + 10 * j + 3 * l + m)
                 for i, f in enumerate(FAMILIES) for j, d in enumerate((128, 768)) for l, n in enumerate((700, 4100)) for m, R in enumerate((1, 5, 10))] +
                [GreedySpec(f, 700, d, 64, 8, 500 + 10 * i + j) for i, f in enumerate(FAMILIES) for j, d in enumerate((128, 768))] +
                [GreedySpec(f, 700, 128, 10, 150, 600 + i) for i, f in enumerate(FAMILIES)] +
                [GreedySpec("duplicates", 700, 96, 5, 8, 700), GreedySpec("mirror", 4100, 96, 10, 8, 701)])       # d = 96: not served by the filter


def greedy_filter_serves(d, R, L):
    dp = (d + 31) // 32 * 32
    return R * L <= 256 and R <= 64 and d % 32 == 0 and dp in (128, 256, 384, 512, 768)


def greedy_dispatch(R, L):
    """[(candidates, groups)] of the batches of one filtered round."""
    M = R * L
    return [(mb, 1 if mb <= 16 else 2 if mb <= 32 else 4) for mb in (min(64, M - 64 * b) for b in range((M + 63) // 64))]


class ReplayState(np.random.RandomState):
    """A RandomState that hands out prepared draws: what sklearn_kpp(compat="1.0.2") takes - randint(n), then uniform(size=L) per added
    centre - for one seeding after another."""

    def __init__(self, first, u):
        super().__init__(0)
        self._first, self._u, self._at = list(first), [row for start in u for row in start], [0, 0]

    def randint(self, n):
        self._at[0] += 1
        return int(self._first[self._at[0] - 1])

    def uniform(self, size=None):
        self._at[1] += 1
        out = self._u[self._at[1] - 1]
        assert len(out) == size
        return np.array(out, dtype=F64)


def u_for(d2, idx):
    """A uniform for which searchsorted(cumsum_f64(d2), u * float32(pot)) is idx (d2[idx] > 0): the middle of its interval."""
    d64 = d2.astype(F64)
    cum = np.cumsum(d64)
    pot = F64(F32(d64.sum()))
    u = (cum[idx] - 0.5 * d64[idx]) / pot
    assert d64[idx] > 0 and 0 <= u < 1 and np.searchsorted(cum, u * pot) == idx
    return u


def greedy_potentials(x, d2, cand):
    dc = np.minimum(d2[None, :], ko.dist_f32(x[cand], x))
    return dc.astype(F64).sum(axis=1)


def greedy_inputs(sp):
    """R consecutive scikit-learn 1.0.2 seedings on one stream.  -> x, first [R], u [R, k - 1, L], ties: the (start, (hi, lo)) whose
    first round is an all-candidates tie by construction - every candidate of that round is row hi or its partner lo (the negative
    from the origin; an equal row), hi first and lo last, so the pick must be hi."""
    def build():
        n, d, R, k = sp.n, sp.d, sp.R, sp.k
        L = 2 + int(np.log(k))
        rs = np.random.RandomState(sp.seed)
        first, u = np.empty(R, dtype=np.int64), np.empty((R, k - 1, L))
        for j in range(R):
            first[j] = rs.randint(n)
            for c in range(k - 1):
                u[j, c] = rs.uniform(size=L)
        kw = {"first": int(first[0])} if sp.family == "mirror" else {}
        _, x, partner = rows(sp.family, n, d, seed=sp.seed, **kw)
        ties = []
        if partner is not None:
            for j in range(R if sp.family == "duplicates" else 1):
                d2 = ko.dist_f32(x, x[first[j]][None])[:, 0]
                pool = np.nonzero((partner != np.arange(n)) & (d2 > 0))[0]
                a = int(pool[(7 * j + 3) % len(pool)])
                hi, lo = max(a, int(partner[a])), min(a, int(partner[a]))
                cand = [hi, lo] * L
                cand = cand[:L - 1] + [lo]
                u[j, 0] = [u_for(d2, c) for c in cand]
                pots = greedy_potentials(x, d2, np.array(cand))
                assert (pots == pots[0]).all(), (sp, j, pots)
                ties.append((j, (hi, lo)))
        return x, first, u, ties
    return _cached(("greedy_in", sp), build)


def greedy_case(sp):
    """greedy_inputs with the oracle's picks [R, k]: -> x, first, u, picks, ties"""
    def build():
        x, first, u, ties = greedy_inputs(sp)
        picks = np.stack([ko.sklearn_kpp(x, sp.k, rep, compat="1.0.2") for rep in [ReplayState(first, u)] for _ in range(sp.R)])
        assert np.array_equal(picks[:, 0], first) and all(picks[j, 1] == hi for j, (hi, lo) in ties)
        return x, first, u, picks, ties
    return _cached(("greedy", sp), build)


def greedy_big():
    """The dense path at N_STAGED rows (d = 4, k = 2, R = 2): kg_search_kernel reads the 1,025 tile sums from global memory.  Start 0's
    first candidate lies in the last tile, start 1's in tile 1,023."""
    def build():
        n, d, k, R, L = N_STAGED, 4, 2, 2, 2
        rs = np.random.RandomState(9)
        xi = rs.randint(-100, 101, size=(n, d)).astype(np.int64)
        x = assert_rule_g(xi)
        first = np.array([rs.randint(n), rs.randint(n)], dtype=np.int64)
        u = rs.uniform(size=(R, k - 1, L))
        hits = (n - 3, (STAGE - 1) * TILE + 2000)
        for j in range(R):
            d2 = ko.dist_f32(x, x[first[j]][None])[:, 0]
            u[j, 0, 0] = u_for(d2, hits[j])
        picks = np.stack([ko.sklearn_kpp(x, k, rep, compat="1.0.2") for rep in [ReplayState(first, u)] for _ in range(R)])
        return x, first, u, picks, hits
    return _cached("greedy_big", build)


# ------------------------------------------------------------------------------------------------ the shared checker
def check_draw(name, want, got):
    """One draw: the index, exactly."""
    assert int(got) == int(want), "%s: drew %d, the oracle %d" % (name, int(got), int(want))


def check_search(case, idx, pot):
    """One search launch: every index and the bits of the potential."""
    idx = np.asarray(idx).astype(np.int64).reshape(-1)
    assert np.array_equal(idx, case.want), "%s: found %s, the oracle %s" % (case.name, idx.tolist(), case.want.tolist())
    assert np.array_equal(np.array([pot], dtype=F64).view(np.uint64), np.array([case.pot], dtype=F64).view(np.uint64)), \
        "%s: potential %r, exact %r" % (case.name, float(pot), case.pot)


def check_picks(name, want, got):
    """The picks of whole seedings [R, k]: every index."""
    got = np.asarray(got).astype(np.int64)
    bad = np.argwhere(got != np.asarray(want))
    assert bad.size == 0, "%s: %d picks differ from the oracle's, first (start, centre) %s: %d != %d" % (
        name, len(bad), bad[0].tolist(), got[tuple(bad[0])], np.asarray(want)[tuple(bad[0])])


def check_bits(name, want, got):
    """float32 arrays, bit for bit."""
    want, got = np.ascontiguousarray(want, dtype=F32), np.ascontiguousarray(got, dtype=F32)
    assert want.shape == got.shape, (name, want.shape, got.shape)
    bad = np.argwhere(want.view(np.uint32) != got.view(np.uint32))
    assert bad.size == 0, "%s: %d values differ in their bits, first at %s: %r != %r" % (
        name, len(bad), bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))
