"""Inputs, exact references and checkers for the kernels that turn clusters into names: the vote histograms (scd_amd/csrc/vote.hip:
scd_vote_hist, scd_vote_table, scd_vote_table_topm) and the small kernels at the end of scd_amd/csrc/sim.hip (scd_select_rows,
scd_gather_rows_f16, scd_transpose_f16, scd_mean2_f16, scd_l2norm_rows, scd_prompt_pool).  numpy only, every input from a seed.

VOTES.  The semantics are collections.Counter(...).most_common(m) over the row-major flattened first top_k columns of the rows a cluster
owns, names in `known` dropped (oracle/naming_oracle.cluster_counters): count descending, ties in first-seen order.  `hist_counter`
states that with Counter; `hist_unique` is the vectorised equal used for the one large case (np.unique of cluster * 2^24 + name with
return_index / return_counts in row-major order, sorted by (-count, first index)); tests/test_naming_cases_sensitivity.py shows the two
equal on every small case.  scd_vote_hist sorts 64-bit keys

    slot (16 bits) | name (24 bits) | position (24 bits)        then        slot (16) | 2^24 - 1 - count (24) | position (24)

so it has LIMITS, which the cases sit on: cluster ids and predictions in [0, 65536) (a prediction outside it, or in no requested
cluster, votes for nothing), at most 65,536 clusters, n * top_k < 2^24, and names in [0, 2^24): the key has no room for any other name,
so names -1 and 2^24 are DROPPED like a `known` name, while 0 and 2^24 - 1 are counted.  The references drop them the same way.
scd_vote_table / scd_vote_table_topm keep a dense [cluster, name] table instead (counts int32, first-seen position int64 below 2^40,
NEVER = 0x7f7f7f7f7f7f7f7f in a cell never seen); the top-m takes (count descending, first ascending) over cells with a count > 0,
compares the whole int32 count and the whole position, and zeroes the cells it takes.

HELPERS.  transpose / gather / select move bits: compared with indexing.  mean2 is fp16((a + b) / 2) of the EXACT sum (float64 holds
it).  l2norm and prompt_pool are checked twice:
  (a) on exact-grid rows, bit for bit: every entry is 0 or +/-2^e and the sum of squares of a row is 4^p, so every partial sum of
      squares (a sum of at most 1,024 terms 4^e spread over at most 20 binades) is exact in float32 in any order, the square root 2^p,
      its reciprocal and every product are exact; outputs stay >= 2^-14 (fp16 normal).  `grid_row` asserts the rule.
  (b) on random rows against float64 with a bound DERIVED from the kernel's operations (u = 2^-24, all first order, then doubled):
      l2norm_rows, one wave per row: s = sum x^2 by ceil(d/64) fmas per lane and six butterfly additions, all terms non-negative, so
        |s' - s| <= (ceil(d/64) + 6) u s and the norm carries half of it; one square root, one reciprocal and one product add u each:
        |out - ref| <= ((ceil(d/64) + 6) / 2 + 3) u |ref|.  The test allows TWICE that; an fp16 output adds its rounding
        max(2^-11 |ref|, 2^-25).
      prompt_pool, one block per name, lane-strided over 16 slots of 64 columns: per prompt row t the squared norm takes 16 fmas and 6
        butterfly additions (error (16 + 6) u, the norm half of it = 11 u), square root and reciprocal add 2 u: inv_t carries 13 u.
        A wave accumulates its ceil(t_per / 4) rows by fma (one rounding each, on partial sums bounded by A_j = sum_t |x_tj| / ||x_t||,
        since the terms have both signs), the four waves merge by 3 additions and the mean divides once:
            a_j = |mean'_j - mean_j| <= (13 + ceil(t_per / 4) + 3 + 1) u A_j / t_per.
        The second norm sees means perturbed by a (relative change of the norm <= ||a|| / ||mean||) and adds its own 4 fmas + 6
        butterfly + 3 merge additions (13 roundings on the square, 6.5 u on the norm), square root, reciprocal and the final product
        (3 u):
            F_j = a_j / ||mean|| + |ref_j| (||a|| / ||mean|| + 9.5 u).
        The test allows 2^-11 |ref_j| (the fp16 half ulp, 2^-25 for a subnormal) + 2 F_j.
      tests/test_naming_cases_sensitivity.py runs a float32 model of both flows inside these bounds: the reference alone fits.
"""
import collections

import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64
U32 = 2.0 ** -24
NAME_BITS, POS_BITS, SLOT_BITS = 24, 24, 16
NAME_LIM = 1 << NAME_BITS                                        # names in [0, NAME_LIM) are counted by scd_vote_hist
MAX_CLUSTER_ID = 1 << SLOT_BITS
NEVER = 0x7F7F7F7F7F7F7F7F

_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


# ================================================================================================ vote_hist
VoteCase = collections.namedtuple("VoteCase", "name idx top_k preds clusters m known")


def _slot_of(c):
    assert len(set(c.clusters)) == len(c.clusters), c.name
    return {int(cl): i for i, cl in enumerate(c.clusters)}


def hist_counter(c):
    """Counter.most_common(m) per requested cluster -> (keys int64 [C, m] padded -1, counts int32 [C, m] padded 0)."""
    slot = _slot_of(c)
    known = set(int(x) for x in (c.known or ()))
    ctr = [collections.Counter() for _ in c.clusters]
    for i in range(c.idx.shape[0]):
        s = slot.get(int(c.preds[i]))
        if s is None:
            continue
        for x in c.idx[i, :c.top_k].tolist():
            if 0 <= x < NAME_LIM and x not in known:
                ctr[s][x] += 1
    keys = np.full((len(ctr), c.m), -1, dtype=np.int64)
    counts = np.zeros((len(ctr), c.m), dtype=np.int32)
    for s, cc in enumerate(ctr):
        for j, (a, b) in enumerate(cc.most_common(c.m)):
            keys[s, j], counts[s, j] = a, b
    return keys, counts


def hist_runs(c):
    """The (slot, name) runs of a case, vectorised: -> (slot, name, count, first) int64 arrays, one entry per distinct pair."""
    cl = np.asarray(c.clusters, dtype=np.int64)
    order = np.argsort(cl, kind="stable")
    pos = np.searchsorted(cl[order], c.preds)
    pos = np.minimum(pos, len(cl) - 1)
    hit = cl[order][pos] == c.preds
    slot = np.where(hit, order[pos], -1)                                        # [n]
    names = np.ascontiguousarray(c.idx[:, :c.top_k]).reshape(-1)
    slots = np.repeat(slot, c.top_k)
    keep = (slots >= 0) & (names >= 0) & (names < NAME_LIM)
    if c.known is not None and len(c.known):
        keep &= ~np.isin(names, np.asarray(c.known, dtype=np.int64))
    e = np.nonzero(keep)[0]
    key = slots[e] * NAME_LIM + names[e]
    uk, first, count = np.unique(key, return_index=True, return_counts=True)
    return uk >> NAME_BITS, uk & (NAME_LIM - 1), count.astype(np.int64), e[first]


def rank_runs(n_clusters, m, slot, name, count, first):
    """most_common(m) of every slot from its runs: sort by (slot, -count, first), keep the first m of each slot."""
    order = np.lexsort((first, -count, slot))
    slot, name, count = slot[order], name[order], count[order]
    start = np.searchsorted(slot, np.arange(n_clusters))
    rank = np.arange(len(slot)) - start[slot]
    keys = np.full((n_clusters, m), -1, dtype=np.int64)
    counts = np.zeros((n_clusters, m), dtype=np.int32)
    ok = rank < m
    keys[slot[ok], rank[ok]] = name[ok]
    counts[slot[ok], rank[ok]] = count[ok]
    return keys, counts


def hist_unique(c):
    return rank_runs(len(c.clusters), c.m, *hist_runs(c))


def hist_want(c):
    return _cached(("hist", c.name), lambda: hist_unique(c) if c.idx.shape[0] > 50000 else hist_counter(c))


def check_pair(name, got, want, what=("keys", "counts")):
    """array_equal on dtype, shape and every element of the two outputs; -> list of messages."""
    bad = []
    for w, g, r in zip(what, got, want):
        g = np.asarray(g)
        if g.dtype != r.dtype or g.shape != r.shape:
            bad.append("%s: %s is %s %s, want %s %s" % (name, w, g.dtype, g.shape, r.dtype, r.shape))
        elif not np.array_equal(g, r):
            at = np.argwhere(g != r)[0]
            bad.append("%s: %s differ in %d cells, first at %s: got %s, want %s (row got %s, want %s)"
                       % (name, w, int((g != r).sum()), at.tolist(), g[tuple(at)], r[tuple(at)], g[at[0]][:8].tolist(), r[at[0]][:8].tolist()))
    return bad


def check_hist(c, keys, counts):
    return check_pair(c.name, (keys, counts), hist_want(c))


SPECIAL_NAMES = (0, NAME_LIM - 1, -1, NAME_LIM, NAME_LIM + 5, -NAME_LIM, (1 << 40) + 3)      # the first two are counted, the rest dropped
BAD_PREDS = (-1, -5, MAX_CLUSTER_ID, MAX_CLUSTER_ID + 7, 1 << 40, -(1 << 40))


def _names(rs, shape, v, special=0.15):
    """Zipf-ish names below v, with SPECIAL_NAMES mixed in (5 stands beside 2^24 + 5, which must not alias it)."""
    a = (rs.zipf(1.4, size=shape) % v).astype(np.int64)
    sp = rs.rand(*shape) < special
    a[sp] = np.asarray(SPECIAL_NAMES, dtype=np.int64)[rs.randint(0, len(SPECIAL_NAMES), size=int(sp.sum()))]
    return a


def _slots_case():
    """40,000 requested ids, six of them predicted: slots 0, 1, 32,767, 32,768, 32,769 and 39,999 carry votes (bit 15 of the slot
    field on both sides), cluster ids 0 and 65,535 among them; predictions outside [0, 65536) and ids in no requested cluster."""
    rs = np.random.RandomState(11)
    ids = rs.permutation(MAX_CLUSTER_ID)
    ids = ids[(ids != 0) & (ids != MAX_CLUSTER_ID - 1)]
    clusters = ids[:40000].copy()
    spare = ids[40000:40010]                                                    # valid ids nobody asked for
    clusters[0], clusters[39999] = MAX_CLUSTER_ID - 1, 0
    live = clusters[[0, 1, 32767, 32768, 32769, 39999]]
    pool = np.concatenate([live, live, live, spare[:3], np.asarray(BAD_PREDS, dtype=np.int64)])
    n = 3000
    preds = pool[rs.randint(0, len(pool), size=n)]
    return VoteCase("slots_bit15", _names(rs, (n, 5), 40), 5, preds, clusters.tolist(), 3, None)


def _plain(name, seed, n, ld, top_k, k, v, m, known=None, special=0.1, poison=None):
    rs = np.random.RandomState(seed)
    idx = _names(rs, (n, ld), v, special)
    if poison is not None:
        idx[:, top_k:] = poison                                                 # columns beyond top_k: must not be counted
    preds = rs.randint(-1, k + 2, size=n).astype(np.int64)
    clusters = [int(x) for x in rs.permutation(k)[: max(1, k - 1)]]             # one id nobody asked for, table rows not in id order
    return VoteCase(name, idx, top_k, preds, clusters, m, known)


def _all_known_case():
    """Cluster 2 holds only names of `known` (40 entries): an all-padding row beside ordinary ones."""
    rs = np.random.RandomState(17)
    known = [int(x) for x in rs.permutation(90)[:40]]
    n = 1200
    idx = rs.randint(0, 90, size=(n, 5)).astype(np.int64)
    preds = rs.randint(0, 4, size=n).astype(np.int64)
    own = preds == 2
    idx[own] = np.asarray(known, dtype=np.int64)[rs.randint(0, 40, size=(int(own.sum()), 5))]
    return VoteCase("known[40],cluster_all_known", idx, 5, preds, [3, 2, 0, 1], 6, known)


def _ties_desc_case():
    """Names 9, 8, .. 0 appear in that order, three times round: ten names of count 3 (and 11 of count 2 / 12 of count 1 behind
    them) whose first-seen order is the DESCENDING name order - the opposite of the order the first sort leaves them in."""
    seq = list(range(9, -1, -1)) * 3 + [11, 12, 11]
    seq += [13] * (-len(seq) % 5)
    idx = np.asarray(seq, dtype=np.int64).reshape(-1, 5)
    other = np.full_like(idx, 3)
    return VoteCase("ties_descending", np.concatenate([idx[:2], other[:1], idx[2:]]), 5,
                    np.asarray([4, 4, 1] + [4] * (idx.shape[0] - 2), dtype=np.int64), [1, 4], 12, None)


def _ties_case(seed):
    rs = np.random.RandomState(seed)
    n = 60
    return VoteCase("ties[seed=%d]" % seed, rs.randint(0, 6, size=(n, 5)).astype(np.int64), 5, rs.randint(0, 5, size=n).astype(np.int64),
                    [4, 0, 2, 1, 3], 8, None)


def hist_cases():
    def build():
        out = [_slots_case(),
               _plain("ld>top_k[ld=7,top_k=3]", 21, 900, 7, 3, 6, 30, 5, poison=0),
               _plain("top_k=1[ld=5]", 22, 900, 5, 1, 6, 30, 5, poison=NAME_LIM - 1),
               _plain("top_k=ld=5", 23, 900, 5, 5, 6, 30, 5)]
        base = _plain("m", 24, 2500, 5, 5, 4, 400, 1, special=0.02)
        for m in (1, 64, 65, 130, 700):                                         # 700: more than the distinct names of any cluster
            out.append(base._replace(name="m=%d" % m, m=m))
        kn = [int(x) for x in np.random.RandomState(25).permutation(60)[:40]]
        for q in (0, 1, 40):
            out.append(_plain("known[%d]" % q, 26, 1500, 5, 4, 5, 60, 7, known=kn[:q]))
        out += [_all_known_case(), _ties_desc_case(), _ties_case(31), _ties_case(32), _ties_case(33),
                VoteCase("single[n*top_k=1]", np.asarray([[7]], dtype=np.int64), 1, np.asarray([2], dtype=np.int64), [5, 2], 2, None),
                VoteCase("single[ld=3]", np.asarray([[NAME_LIM - 1, 7, 7]], dtype=np.int64), 1, np.asarray([0], dtype=np.int64), [0], 1, None)]
        for c in out:
            assert c.idx.dtype == np.int64 and c.preds.dtype == np.int64 and c.idx.shape[0] * c.top_k < 1 << POS_BITS
        names = [c.name for c in out]
        assert len(set(names)) == len(names)
        return out
    return _cached("hist_cases", build)


BIG_N, BIG_TOP_K = 3355443, 5                                     # n * top_k = 2^24 - 1: bit 23 of the position field is set
BIG_CLUSTERS = [9, 0, 65535, 32768, 4, 77, 1000, 65534]
BIG_HEAVY = (65535, 12345)                                        # (cluster, name) with a count above 2^23: the count field's top bit
BIG_LATE = 32768                                                  # the cluster of the planted late names


def big_case():
    """The one case above a few thousand rows.  Cluster 65,535 owns three rows in four and name 12,345 fills three cells in four
    of them: its count is above 2^23.  Cluster 32,768 holds planted ties whose first positions differ in bit 23 only (`BIG_PLANTS`)."""
    def build():
        rs = np.random.RandomState(41)
        n = BIG_N
        idx = rs.randint(0, 3000, size=(n, BIG_TOP_K)).astype(np.int64)
        idx[rs.rand(n, BIG_TOP_K) < 0.0001] = NAME_LIM                          # dropped
        pool = [c for c in BIG_CLUSTERS if c != BIG_LATE] + [5, -1, 70000]      # BIG_LATE owns the planted rows only
        preds = np.asarray(pool, dtype=np.int64)[rs.randint(0, len(pool), size=n)]
        heavy = rs.rand(n) < 0.75
        preds[heavy] = BIG_HEAVY[0]
        cells = heavy[:, None] & (rs.rand(n, BIG_TOP_K) < 0.75)
        idx[cells] = BIG_HEAVY[1]
        for q, (row, col, name) in enumerate(BIG_PLANTS):
            preds[row] = BIG_LATE
            idx[row] = 3000 + 5 * q + np.arange(5)                              # names nobody else holds, count 1 each
            idx[row, col] = name
        return VoteCase("big[n*top_k=2^24-1]", idx, BIG_TOP_K, preds, list(BIG_CLUSTERS), 6, [17, 18])
    return _cached("big_case", build)


# (row, column, name): cluster BIG_LATE owns these four rows only.  Name 2^24 - 2 is first seen at position 100, name 2^24 - 3 at
# 2^23 + 10; both have count 2 and every other name of the cluster (almost surely) count 1, so most_common starts with 2^24 - 2,
# 2^24 - 3 - and with 2^24 - 3, 2^24 - 2 if the position lost bit 23 (10 < 100).  big_want asserts the first.
_H = 1 << (POS_BITS - 1)
BIG_PLANTS = (((100 // 5), 0, NAME_LIM - 2), ((_H + 10) // 5, (_H + 10) % 5, NAME_LIM - 3),
              ((_H + 4000) // 5, (_H + 4000) % 5, NAME_LIM - 2), ((_H + 5000) // 5, (_H + 5000) % 5, NAME_LIM - 3))


def big_runs():
    return _cached("big_runs", lambda: hist_runs(big_case()))


def big_want():
    def build():
        c = big_case()
        keys, counts = rank_runs(len(c.clusters), c.m, *big_runs())
        late, heavy = c.clusters.index(BIG_LATE), c.clusters.index(BIG_HEAVY[0])
        assert keys[late, :2].tolist() == [NAME_LIM - 2, NAME_LIM - 3] and counts[late, :3].tolist() == [2, 2, 1]
        assert keys[heavy, 0] == BIG_HEAVY[1] and counts[heavy, 0] > 1 << 23
        return keys, counts
    return _cached("big_want", build)


# ================================================================================================ vote_table
TableCase = collections.namedtuple("TableCase", "name idx top_k preds clusters n_slots row_offset v")


def table_want(c, rows=slice(None), row_offset=None):
    """Dense tables of the rows `rows` of a case: counts int32 [C, v], first int64 [C, v] (NEVER where the count is 0)."""
    idx, preds = c.idx[rows], c.preds[rows]
    off = c.row_offset if row_offset is None else row_offset
    slot_of = np.full(c.n_slots, -1, dtype=np.int64)
    slot_of[np.asarray(c.clusters, dtype=np.int64)] = np.arange(len(c.clusters))
    inside = (preds >= 0) & (preds < c.n_slots)
    slot = np.where(inside, slot_of[np.where(inside, preds, 0)], -1)
    names = idx[:, :c.top_k]
    pos = (off + np.arange(idx.shape[0], dtype=np.int64))[:, None] * c.top_k + np.arange(c.top_k, dtype=np.int64)[None, :]
    keep = (slot[:, None] >= 0) & (names >= 0) & (names < c.v)
    s = np.broadcast_to(slot[:, None], names.shape)[keep]
    counts = np.zeros((len(c.clusters), c.v), dtype=np.int32)
    first = np.full((len(c.clusters), c.v), NEVER, dtype=np.int64)
    np.add.at(counts, (s, names[keep]), 1)
    np.minimum.at(first, (s, names[keep]), pos[keep])
    return counts, first


def table_loop(c):
    """The same tables by a plain loop with Counter: the statement `table_want` is checked against on the CPU."""
    slot = {int(cl): i for i, cl in enumerate(c.clusters)}
    counts = np.zeros((len(c.clusters), c.v), dtype=np.int32)
    first = np.full((len(c.clusters), c.v), NEVER, dtype=np.int64)
    for i in range(c.idx.shape[0]):
        p = int(c.preds[i])
        s = slot.get(p) if 0 <= p < c.n_slots else None
        if s is None:
            continue
        for j in range(c.top_k):
            nm = int(c.idx[i, j])
            if 0 <= nm < c.v:
                counts[s, nm] += 1
                first[s, nm] = min(int(first[s, nm]), (c.row_offset + i) * c.top_k + j)
    return counts, first


def _table(name, seed, n, v, top_k=3, ld=5, n_slots=12, clusters=(3, 0, 11, 7), row_offset=0):
    rs = np.random.RandomState(seed)
    idx = rs.randint(-3, v + 3, size=(n, ld)).astype(np.int64)                  # names outside [0, v) on both sides
    idx[rs.rand(n, ld) < 0.3] = v - 1                                           # the last column of the table is busy
    preds = rs.randint(-2, n_slots + 2, size=n).astype(np.int64)                # predictions outside [0, n_slots) on both sides
    return TableCase(name, idx, top_k, preds, list(clusters), n_slots, row_offset, v)


def table_cases():
    def build():
        out = [_table("v=%d" % v, 50 + i, 1500, v) for i, v in enumerate((1, 50, 255, 256, 257, 2100))]
        out.append(TableCase("n=0", np.zeros((0, 5), dtype=np.int64), 3, np.zeros(0, dtype=np.int64), [1, 0], 4, 0, 9))
        out.append(TableCase("contention[20000 rows, one cell]", np.full((20000, 1), 2, dtype=np.int64), 1, np.zeros(20000, dtype=np.int64), [0], 1, 0, 3))
        out.append(_table("row_offset=2^37", 60, 1500, 50, top_k=5, row_offset=1 << 37))
        return out
    return _cached("table_cases", build)


def shard_cases():
    """(case, cuts): the rows of `case` in shards [cuts[i], cuts[i + 1]); one shard of each is empty."""
    return [(_table("shards[2]", 61, 1200, 257, top_k=5, row_offset=1 << 37), (0, 1200, 1200)),
            (_table("shards[3]", 62, 1300, 50, top_k=2), (0, 500, 500, 1300)),
            (_table("shards[3,first empty]", 63, 900, 256, top_k=5), (0, 0, 301, 900))]


def counts_as_hist(c, m):
    """The VoteCase a TableCase amounts to (names and predictions the table skips are names / predictions vote_hist drops too, as long
    as v <= 2^24 and n_slots <= 65,536): ties the table form to Counter.most_common through the top-m."""
    idx = np.where((c.idx >= 0) & (c.idx < c.v), c.idx, -1)
    preds = np.where((c.preds >= 0) & (c.preds < c.n_slots), c.preds, -1)
    return VoteCase(c.name, idx, c.top_k, preds, list(c.clusters), m, None)


# ================================================================================================ vote_table_topm
TopmCase = collections.namedtuple("TopmCase", "name counts first m")


def topm_want(counts, first, m):
    """-> (keys int64 [C, m], cnt int32 [C, m], the counts table after the call: taken cells zeroed).  Cells with a count > 0 in
    (count descending, first ascending) order; the name breaks a tie of both, which no table of scd_vote_table holds."""
    keys = np.full((counts.shape[0], m), -1, dtype=np.int64)
    cnt = np.zeros((counts.shape[0], m), dtype=np.int32)
    after = counts.copy()
    for s in range(counts.shape[0]):
        nz = np.nonzero(counts[s] > 0)[0]
        order = sorted(nz.tolist(), key=lambda nm: (-int(counts[s, nm]), int(first[s, nm]), nm))[:m]
        for j, nm in enumerate(order):
            keys[s, j], cnt[s, j] = nm, counts[s, nm]
            after[s, nm] = 0
    return keys, cnt, after


COUNT_BITS_ROW = (1 << 24, 3, (1 << 31) - 1, (1 << 24) - 1, 0, 1, (1 << 24) + 5, 0)


def _topm_random(name, seed, v, m, n_rows=3, hi=50):
    rs = np.random.RandomState(seed)
    counts = rs.randint(0, hi, size=(n_rows, v)).astype(np.int32)
    counts[rs.rand(n_rows, v) < 0.3] = 0
    first = np.stack([rs.permutation(v * 7)[:v] for _ in range(n_rows)]).astype(np.int64)
    first[counts == 0] = NEVER
    counts[0, v - 1], first[0, v - 1] = 1000, 5 * v                              # the winner sits in the last column
    if n_rows > 1:
        counts[1], first[1] = 0, NEVER                                          # a row of zeros: all -1 / 0
    return TopmCase(name, counts, first, m)


def topm_cases():
    def build():
        row = np.asarray([COUNT_BITS_ROW], dtype=np.int32)
        out = [TopmCase("count_bits", row, (np.arange(8, dtype=np.int64)[None, :] * 11 + 5), 8)]
        # equal counts, positions that differ only above bit 32 (all below 2^40, as scd_vote_table produces them)
        hi = np.asarray([5, 1, 7, 0, 3, 6, 2, 4], dtype=np.int64)
        out.append(TopmCase("first_above_bit32", np.full((1, 8), 4, dtype=np.int32), ((hi << 33) + 12345)[None, :], 8))
        out.append(TopmCase("first_above_bit32,counts 2^24", np.full((1, 8), 1 << 24, dtype=np.int32), ((hi << 36) + 9)[None, :], 5))
        for i, v in enumerate((1, 255, 256, 257, 1031)):
            out.append(_topm_random("v=%d" % v, 70 + i, v, 5, n_rows=3 if v > 1 else 2))
        out.append(_topm_random("ties[v=300]", 80, 300, 40, hi=3))
        out.append(_topm_random("m>cells[v=40,m=64]", 81, 40, 64))
        for c in out:
            assert c.counts.dtype == np.int32 and c.first.dtype == np.int64 and c.counts.shape == c.first.shape
        return out
    return _cached("topm_cases", build)


# ================================================================================================ bit movers
TRANSPOSE_SHAPES = ((1, 1), (63, 65), (64, 64), (65, 63), (1, 4097), (513, 70), (512, 1031))
# (d, k, m): every d, k and m of the issue at least once; d = 100 is the scalar path, 520 a second trip of the 8-wide loop
SELECT_SHAPES = ((8, 1, 1), (64, 5, 3), (100, 64, 4), (512, 5, 5), (520, 1, 1025), (768, 64, 5), (1032, 5, 4), (100, 5, 1025))
GATHER_SHAPES = ((1, 1), (63, 3), (64, 4), (65, 5), (512, 1025), (1000, 5))     # (d, m)
SELECT_ROWS = 37


def any_f16_bits(seed, shape):
    """Every bit pattern, NaNs included: for kernels that only move fp16."""
    return np.random.RandomState(seed).randint(0, 1 << 16, size=shape).astype(np.uint16)


def finite_f16(seed, shape):
    """fp16 values with the specials a float32 image keeps: zeros of both signs, subnormals, the largest normal, infinities (no NaN)."""
    rs = np.random.RandomState(seed)
    x = (rs.randn(*shape) * 4).astype(F16)
    sp = np.asarray([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -14, 65504.0, -65504.0, np.inf, -np.inf, 2.0 ** -15], dtype=F16)
    hit = rs.rand(*shape) < 0.1
    x[hit] = sp[rs.randint(0, len(sp), size=int(hit.sum()))]
    return x


def select_index(seed, m, n_rows=SELECT_ROWS):
    """m row numbers: random (so with duplicates once m > 1), then the same sorted descending."""
    idx = np.random.RandomState(seed).randint(0, n_rows, size=m).astype(np.int64)
    if m >= 3:
        idx[1] = idx[0]
    return idx, np.sort(idx)[::-1].copy()


# ================================================================================================ mean2
def mean2_want(a, b):
    with np.errstate(all="ignore"):
        return ((a.astype(F64) + b.astype(F64)) / 2).astype(F16)


def same_f16(got, want):
    """Bit equality, any NaN equal to any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint16)[~nan], want.view(np.uint16)[~nan])


_E = 2.0 ** -10
MEAN2_PAIRS = (
    (65504.0, 65504.0),                 # overflow: the sum is not an fp16, the mean is
    (1.0, 1.0 + _E),                    # exact tie, to even: 1.0
    (1.0 + _E, 1.0 + 2 * _E),           # exact tie, to even: 1 + 2^-9
    (-65504.0, -65504.0),
    (65504.0, -65504.0),
    (0.0, -0.0), (-0.0, -0.0), (0.0, 0.0),
    (2.0 ** -24, 0.0),                  # half the smallest subnormal: tie to even, 0
    (2.0 ** -24, 2.0 ** -24), (3 * 2.0 ** -24, 0.0), (3 * 2.0 ** -24, 2.0 ** -23), (-2.0 ** -24, 0.0), (2.0 ** -14, 2.0 ** -24),
    (2.0 ** -14, -2.0 ** -24), (2.0 ** -15, 2.0 ** -16), (2.0 ** -14 + 2.0 ** -24, 2.0 ** -14),          # subnormal results and their border
    (65504.0, 2.0 ** -24), (65504.0, -2.0 ** -24), (2048.0, -2.0 ** -24), (2048.0, 2.0 ** -24), (4096.0, -1.0), (4100.0, 2.0 + 2.0 ** -9),
    (1024.0, 2.0 ** -14), (-1024.0, 2.0 ** -14), (1.0, -2.0 ** -24), (32768.0, 2.0 ** -10),            # many binades apart
    (np.inf, 1.0), (-np.inf, 65504.0), (np.inf, np.inf), (np.inf, -np.inf), (np.nan, 1.0), (np.nan, np.inf), (0.0, np.nan),
    (65504.0, 65472.0), (65504.0, 32.0), (3.0, 2.0 ** -10), (1.0 + _E, -1.0),
)
MEAN2_NUMELS = (8, 8 * 255, 8 * 256, 8 * 257)


def mean2_inputs(numel):
    """The hand-made pairs first (the first 8 alone at numel = 8), then random bit patterns (about 1 in 30 inf / NaN)."""
    a, b = any_f16_bits(90, numel).view(F16).copy(), any_f16_bits(91, numel).view(F16).copy()
    k = min(numel, len(MEAN2_PAIRS))
    with np.errstate(all="ignore"):
        a[:k] = np.asarray([p[0] for p in MEAN2_PAIRS[:k]], dtype=F16)
        b[:k] = np.asarray([p[1] for p in MEAN2_PAIRS[:k]], dtype=F16)
    return a, b


# ================================================================================================ exact grids (l2norm, prompt_pool)
def grid_row(rs, d, p, splits):
    """float64 [d]: entries 0 or +/-2^e whose squares sum to 4^p.  One entry 2^p; `splits` times an entry 2^e becomes four entries
    2^(e-1) (4 * 4^(e-1) = 4^e), while places are left."""
    exps = [p]
    for _ in range(splits):
        if len(exps) + 3 > d:
            break
        j = rs.randint(0, len(exps))
        if exps[j] <= p - 10:
            continue
        e = exps.pop(j)
        exps += [e - 1] * 4
    row = np.zeros(d, dtype=F64)
    at = rs.permutation(d)[:len(exps)]
    row[at] = np.exp2(np.asarray(exps, dtype=F64)) * rs.choice([-1.0, 1.0], size=len(exps))
    assert float((row * row).sum()) == 4.0 ** p and np.array_equal(row.astype(F16).astype(F64), row)
    assert np.abs(row[row != 0]).min() >= 2.0 ** (p - 10)
    return row


L2_GRID_D = (1, 63, 64, 65, 512, 768, 1000)
L2_GRID_N = (1, 4, 5, 1025)


def l2_grid(d, n, seed=0):
    """-> (x float64 [n, d] on the grid, want float64 [n, d] = x / ||x||, exact): 16 patterns rolled along the row; with n > 1 the row
    before the last is all zeros (result zeros).  |x| in [2^-14, 2^4] and |want| >= 2^-10: both exact in fp16 and float32."""
    rs = np.random.RandomState(1000 * d + seed)
    ps = (-4, -2, 0, 1, 2, 3, 4, 0, -1, 2, -3, 1, 0, 4, -4, 3)
    pats = [grid_row(rs, d, p, s) for p, s in zip(ps, (0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 200, 250, 40, 300))]
    x = np.stack([np.roll(pats[i % 16], i // 16) for i in range(n)])
    want = np.stack([x[i] / 2.0 ** ps[i % 16] for i in range(n)])
    if n > 1:
        x[n - 2], want[n - 2] = 0.0, 0.0
    assert np.array_equal(want.astype(F16).astype(F64), want) and (np.abs(want[want != 0]) >= 2.0 ** -14).all()
    return x, want


POOL_D = (64, 100, 512, 768, 1024)


def pool_grid_same(d, t_per, n_names=3, seed=0):
    """t_per identical unit-norm grid rows per name -> (emb fp16 [n_names * t_per, d], want fp16 [d, n_names]: that row)."""
    rs = np.random.RandomState(77 * d + t_per + seed)
    rows = [grid_row(rs, d, 0, s) for s in (3, 9, 1)[:n_names]]
    emb = np.concatenate([np.tile(r[None, :], (t_per, 1)) for r in rows]).astype(F16)
    return emb, np.stack(rows, axis=1).astype(F16)


def pool_grid_disjoint(d, t_per, n_names=2, seed=0):
    """Per name four unit-norm grid rows on disjoint quarters of the columns, each t_per / 4 times, in a shuffled order: the mean is
    r_i / 4 on quarter i, its norm 1/2, the result r_i / 2."""
    assert t_per % 4 == 0 and d >= 16
    rs = np.random.RandomState(99 * d + t_per + seed)
    q = d // 4
    emb, want = [], []
    for _ in range(n_names):
        rows = []
        for i in range(4):
            r = np.zeros(d, dtype=F64)
            r[i * q:(i + 1) * q] = grid_row(rs, q, 0, int(rs.randint(0, 6)))
            rows.append(r)
        order = rs.permutation(np.repeat(np.arange(4), t_per // 4))
        emb.append(np.stack([rows[i] for i in order]))
        want.append(sum(rows) / 2.0)
    return np.concatenate(emb).astype(F16), np.stack(want, axis=1).astype(F16)


# ================================================================================================ toleranced references (float64)
def l2_random(d, n, seed, f16):
    """Rows of magnitudes log-uniform over [2^-40, 2^40] (fp16: [2^-14, 2^14]); every fourth row spans the whole range, the others
    16 binades around a row-wise centre."""
    rs = np.random.RandomState(seed)
    lim = 14.0 if f16 else 40.0
    centre = rs.uniform(-lim + 8, lim - 8, size=(n, 1))
    e = centre + rs.uniform(-8, 8, size=(n, d))
    wide = np.arange(n) % 4 == 3
    e[wide] = rs.uniform(-lim, lim, size=(int(wide.sum()), d))
    x = np.exp2(e) * rs.choice([-1.0, 1.0], size=(n, d))
    return x.astype(F16 if f16 else F32)


def l2_want(x):
    x = x.astype(F64)
    return x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), F64(F32(1e-12)))       # the kernel's clamp is the float32 1e-12


def l2_bound(ref, d, f16):
    """|out - ref| allowed: twice the first-order bound of the module docstring, plus the fp16 rounding of an fp16 output."""
    tol = 2.0 * ((-(-d // 64) + 6) / 2.0 + 3.0) * U32 * np.abs(ref)
    if f16:
        tol = tol + np.maximum(2.0 ** -11 * np.abs(ref), 2.0 ** -25)
    return tol


PoolCase = collections.namedtuple("PoolCase", "name emb n_names t_per d col0 ld_out")
POOL_T = (1, 3, 4, 5, 9, 80)


def pool_cases():
    """Random prompt embeddings whose rows differ in norm by up to 16x (so that the per-prompt normalisation matters), partly
    correlated inside a name (so that the mean is neither tiny nor a single row)."""
    def build():
        out = []
        for i, (d, t_per, n_names) in enumerate(((64, 1, 7), (100, 3, 1), (512, 4, 7), (768, 5, 1), (1024, 9, 7), (512, 80, 7), (100, 80, 1),
                                                 (1024, 3, 1), (64, 9, 1), (768, 4, 7))):
            rs = np.random.RandomState(300 + i)
            base = rs.randn(n_names, 1, d)
            emb = (base + 1.5 * rs.randn(n_names, t_per, d)) * np.exp2(rs.uniform(-2, 2, size=(n_names, t_per, 1)))
            out.append(PoolCase("d=%d,t_per=%d,n_names=%d" % (d, t_per, n_names), emb.reshape(-1, d).astype(F16), n_names, t_per, d,
                                1 + i % 3, 1 + i % 3 + n_names + 1 + i % 4))
        return out
    return _cached("pool_cases", build)


def pool_want(c):
    """-> (ref float64 [d, n_names], tol float64 [d, n_names]) by the derivation of the module docstring."""
    x = c.emb.astype(F64).reshape(c.n_names, c.t_per, c.d)
    xn = x / np.sqrt((x * x).sum(axis=2, keepdims=True))
    mean = xn.mean(axis=1)                                                      # [names, d]
    nrm = np.sqrt((mean * mean).sum(axis=1, keepdims=True))
    ref = mean / nrm
    a = (13 + -(-c.t_per // 4) + 3 + 1) * U32 * np.abs(xn).sum(axis=1) / c.t_per
    f = a / nrm + np.abs(ref) * (np.sqrt((a * a).sum(axis=1, keepdims=True)) / nrm + 9.5 * U32)
    tol = np.maximum(2.0 ** -11 * np.abs(ref), 2.0 ** -25) + 2.0 * f
    return ref.T.copy(), tol.T.copy()


POOL_SENTINEL = F16(-7.5)


def check_pool(c, out):
    """out: the whole [d, ld_out] fp16 tensor, filled with POOL_SENTINEL before the call -> list of messages."""
    ref, tol = pool_want(c)
    got = out[:, c.col0:c.col0 + c.n_names].astype(F64)
    bad = []
    err = np.abs(got - ref)
    if not (err <= tol).all():                                                  # NaN fails
        j = np.unravel_index(np.argmax(np.where(np.isnan(err), np.inf, err / tol)), err.shape)
        bad.append("%s: |out - ref| %.3e > %.3e at %s (%d cells over)" % (c.name, err[j], tol[j], j, int((~(err <= tol)).sum())))
    rest = np.delete(out, np.arange(c.col0, c.col0 + c.n_names), axis=1)
    if not (rest.view(np.uint16) == POOL_SENTINEL.view(np.uint16)).all():
        bad.append("%s: %d cells outside columns [%d, %d) were written" % (c.name, int((rest.view(np.uint16) != POOL_SENTINEL.view(np.uint16)).sum()),
                                                                          c.col0, c.col0 + c.n_names))
    return bad
