"""Inputs and exact references for the Lloyd M-step family (scd_amd/csrc/mstep.hip: the counting sort, mstep_segment_kernel,
mstep_segment16_kernel; scd_amd/csrc/kmeans.hip: finalize_kernel, sumsq_dd_kernel, mstep_delta_kernel, labels_sync_kernel,
inertia_dd_kernel).  numpy only, deterministic.

Every case lies on an EXACT GRID: a row is integers times one power of two (`unit` = 2^-10), |integer| <= 2^20 for float32 rows and
<= 2,048 for rows that also have an exact fp16 copy; C_old lies on the same grid.  Every per-cluster sum and the row-wise inertia are
then integers below 2^53 grid units (`grid_rows` and `case` assert it): float64 holds every partial sum exactly in any order of additions, so the
device's atomics have ONE right answer and the tests compare with array_equal.  References are computed in integers; inertia for
arbitrary float32 centres and sums of squares in exact integer arithmetic on Python ints (`exact_ints`, `exact_inertia`).

Which kernel a shape reaches (mstep_impl):
  float32 rows, cdiv(n, 256) < 128 (n <= 32,512)   mstep_segment_kernel<G, 8, 8>      8 sorted keys per wave, 32 per block    "few32"
  float32 rows, n >= 32,513                        mstep_segment_kernel<G, 64, 8>    64 sorted keys per wave, 256 per block   "prod32"
      G = 1, 2, 4, 8, 12, 16 for d <= 64, 128, 256, 512, 768, 1024
  fp16 copy, any n                                 mstep_segment16_kernel<G2, 64, 8>                                          "f16"
      G2 = 1, 2, 4, 6, 8 for d <= 128, 256, 512, 768, 1024
  sort: k <= 8,191 and (cdiv(n, 1024) + 1) (k + 1) 4 bytes within the workspace: counting sort (histogram per 1,024-row block, scan,
  scatter), "count"; k = 8,192: rocPRIM radix sort, "rocprim"; k = 8,191 with n = 1,200,000: the histogram does not fit, "fallback".

Label layouts (functions of (n, k, seed) -> int32 labels; each but all_invalid carries min(3, n // 8) labels of -1 and as many of k):
  uniform          random labels
  one_giant        ~97 % of the rows in one cluster: a run over many waves and blocks
  singletons       random labels with k >= n / 2: most clusters have 0, 1 or 2 rows
  boundaries       cluster sizes such that, after the sort, runs end on and one either side of multiples of 4 (MU at ROWS = 64 is 8, the
                   other schedules' 4), 8, 32, 64 and 256
  tails            the first five blocks of `rows` * 4 sorted keys end their four waves in the patterns AAAA, AAAB, ABBB, AABC, ABCD; the
                   last block has 1, 2 or 3 live waves (by n); for 2 and 3 the last wave holds invalid keys only
  sorted           (i // 1024) % k: one label per 1,024-row block of the histogram / scatter stage
  reverse_sorted   the same, reversed
  interleaved      i % k: every label in every block
  all_invalid      -1, k, k + 5, INT_MIN, INT_MAX
  all_one          one cluster holds every row
"""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name layout xi x labels k ci c_old split f16 kern sort")      # built from a Spec by case()

UNIT_LOG2 = -10
UNIT = 2.0 ** UNIT_LOG2
LIMIT32, LIMIT16 = 1 << 20, 2048
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def cdiv(a, b):
    return -(-a // b)


def g32(d):
    return next(g for g, lim in ((1, 64), (2, 128), (4, 256), (8, 512), (12, 768), (16, 1024)) if d <= lim)


def g16(d):
    return next(g for g, lim in ((1, 128), (2, 256), (4, 512), (6, 768), (8, 1024)) if d <= lim)


def kernel32(n):
    return "few32" if cdiv(n, 256) < 128 else "prod32"


def ws_temp_bytes(n):
    """The part of scd_kmeans_mstep_ws_bytes behind the two key arrays (what the histogram or rocPRIM may use)."""
    return 24 * n + (8 << 20)


def sort_path(n, k):
    if k > 8191:
        return "rocprim"
    return "count" if (cdiv(n, 1024) + 1) * (k + 1) * 4 <= ws_temp_bytes(n) else "fallback"


# ------------------------------------------------------------------------------------------------ label layouts
def _n_inv(n):
    return min(3, n // 8)


def _with_invalid(valid, n, k, rs):
    """Insert _n_inv(n) labels of -1 and as many of k at random places (they sort behind every valid key: run positions do not move)."""
    m = _n_inv(n)
    assert len(valid) + 2 * m == n, (len(valid), n)
    out = np.empty(n, dtype=np.int64)
    where = rs.choice(n, 2 * m, replace=False)
    mask = np.zeros(n, dtype=bool)
    mask[where] = True
    out[where[:m]], out[where[m:]] = -1, k
    out[~mask] = valid
    return out.astype(np.int32)


def _nv(n):
    """Valid labels a layout of n rows holds."""
    return n - 2 * _n_inv(n)


def uniform(n, k, seed=0):
    rs = np.random.RandomState(seed)
    return _with_invalid(rs.randint(0, k, size=_nv(n)), n, k, rs)


def one_giant(n, k, seed=0):
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, k, size=_nv(n))
    lab[rs.rand(len(lab)) < 0.97] = k // 2
    return _with_invalid(lab, n, k, rs)


def singletons(n, k, seed=0):
    assert 2 * k >= n
    return uniform(n, k, seed)


def _from_sizes(sizes, n, k, rs):
    assert len(sizes) <= k, (len(sizes), k)
    lab = np.repeat(np.arange(len(sizes)), sizes)
    return _with_invalid(lab[rs.permutation(len(lab))], n, k, rs)


def boundary_ends(nv):
    ends = set()
    for m in (4, 8, 32, 64, 256):
        for j in range(1, 4):
            ends.update((j * m - 1, j * m, j * m + 1))
    ends.update((1, 2))
    return sorted(e for e in ends if 0 < e <= nv)


def boundaries(n, k, seed=0):
    rs = np.random.RandomState(seed)
    nv = _nv(n)
    ends = boundary_ends(nv)
    sizes = list(np.diff([0] + ends))
    rest = nv - (ends[-1] if ends else 0)
    free = k - len(sizes)
    assert free >= 1 or rest == 0, (n, k, len(sizes))
    if rest:
        sizes += list(rs.multinomial(rest, np.ones(free) / free))
    return _from_sizes(sizes, n, k, rs)


def tails(n, k, seed=0, rows=8):
    """See the module docstring.  The live waves of the last block: cdiv(n - 4 rows (n // (4 rows)), rows), must be 1, 2 or 3."""
    rs = np.random.RandomState(seed)
    R, B = rows, n // (4 * rows)
    nw = cdiv(n - B * 4 * R, R)
    assert B >= 5 and 1 <= nw <= 3, (n, rows, B, nw)
    h = R // 2
    sizes = [4 * R,                                   # AAAA
             3 * R + h, R - h,                        # AAAB
             R, 3 * R,                                # ABBB
             2 * R, h, R - h, h, R - h,               # AABC (two short runs inside waves 2 and 3)
             R, R, R, R]                              # ABCD
    tail = n - B * 4 * R
    ninv = 2 * _n_inv(n) if nw == 1 else tail - (nw - 1) * R
    last = [max(0, tail - ninv)] if nw == 1 else ([R] if nw == 2 else [R + h, R - h])      # nw = 3: wave 0 = E, wave 1 = E then F
    fill = n - ninv - sum(sizes) - sum(last)                    # whole blocks, but for nw = 1 with fewer keys in the last block than invalid ones
    nfill = min(k - len(sizes) - 2, max(1, fill // (3 * R)))
    assert fill >= 0 and ninv >= 1 and (fill == 0 or nfill >= 1), (n, rows, fill)
    if fill:
        sizes += list(rs.multinomial(fill, np.ones(nfill) / nfill))
    sizes += [v for v in last if v]
    assert len(sizes) <= k
    if nw == 1:
        lab = np.repeat(np.arange(len(sizes)), sizes)
        return _with_invalid(lab[rs.permutation(len(lab))], n, k, rs)
    # nw = 2, 3: the last wave holds invalid keys only
    lab = np.concatenate([np.repeat(np.arange(len(sizes)), sizes), np.where(np.arange(ninv) % 2 == 0, -1, k)])
    return lab[rs.permutation(len(lab))].astype(np.int32)


def sorted_(n, k, seed=0):
    rs = np.random.RandomState(seed)
    return _with_invalid((np.arange(_nv(n)) // 1024) % k, n, k, rs)


def reverse_sorted(n, k, seed=0):
    rs = np.random.RandomState(seed)
    return _with_invalid(((np.arange(_nv(n)) // 1024) % k)[::-1], n, k, rs)


def interleaved(n, k, seed=0):
    rs = np.random.RandomState(seed)
    return _with_invalid(np.arange(_nv(n)) % k, n, k, rs)


def all_invalid(n, k, seed=0):
    return np.array([-1, k, k + 5, INT_MIN, INT_MAX], dtype=np.int64)[np.arange(n) % 5].astype(np.int32)


def all_one(n, k, seed=0):
    rs = np.random.RandomState(seed)
    return _with_invalid(np.full(_nv(n), k // 2), n, k, rs)


LAYOUTS = {"uniform": uniform, "one_giant": one_giant, "singletons": singletons, "boundaries": boundaries, "tails": tails,
           "sorted": sorted_, "reverse_sorted": reverse_sorted, "interleaved": interleaved, "all_invalid": all_invalid, "all_one": all_one}


# ------------------------------------------------------------------------------------------------ rows, centres, references
_rows_cache = collections.OrderedDict()                  # (n, d, f16, seed) -> (xi, x): the last few only (a production-size pair is 260 MB)


def grid_rows(n, d, f16, seed=0):
    """(int32 [n, d] grid integers, the float32 rows): the bulk in +-1,000; a few values at +-2,048 and 2,047 when the rows must have an
    exact fp16 copy, else at +-2^20 and 2^20 - 1.  Asserts the grid property."""
    key = (n, d, f16, seed)
    if key in _rows_cache:
        _rows_cache.move_to_end(key)
        return _rows_cache[key]
    rs = np.random.RandomState(1000 + seed + 7 * d + n % 9973)
    xi = rs.randint(-1000, 1001, size=(n, d), dtype=np.int32)
    m = min(n * d, 6)
    at = (np.arange(m) * (n * d // m) + rs.randint(0, n * d // m, size=m))       # m distinct places
    big = (LIMIT16, -LIMIT16, LIMIT16 - 1) if f16 else (LIMIT32, -LIMIT32, LIMIT32 - 1)
    xi.reshape(-1)[at] = np.array(big * 2, dtype=np.int32)[:m]
    x = to_f32(xi)
    assert np.abs(xi).max(initial=0) <= (LIMIT16 if f16 else LIMIT32) and d <= 1024
    assert np.array_equal(x.astype(np.float64) * (1.0 / UNIT), xi)
    if f16:
        assert d % 2 == 0 and np.array_equal(x.astype(np.float16).astype(np.float32), x)
    assert np.abs(xi).astype(np.int64).sum(axis=0).max() < 2 ** 53          # bounds every per-cluster sum
    _rows_cache[key] = (xi, x)
    while len(_rows_cache) > 3:
        _rows_cache.popitem(last=False)
    return xi, x


def to_f32(vi):
    v = (vi.astype(np.float32) * np.float32(UNIT))
    return v


def sums_counts(xi, labels, k):
    """Exact per-cluster sums (int64 [k, d], grid units) and counts of the rows with 0 <= label < k."""
    ok = (labels >= 0) & (labels < k)
    lab = labels[ok].astype(np.int64)
    order = np.argsort(lab, kind="stable")
    ls = lab[order]
    sums = np.zeros((k, xi.shape[1]), dtype=np.int64)
    if len(ls):
        starts = np.nonzero(np.r_[True, ls[1:] != ls[:-1]])[0]
        sums[ls[starts]] = np.add.reduceat(xi[ok][order], starts, axis=0, dtype=np.int64)
    return sums, np.bincount(lab, minlength=k).astype(np.int64)


def row_inertia(xi, labels, k, ci):
    """int64 [n]: ||x_i - c_label||^2 in grid units^2 (0 for a row whose label is not in [0, k)); ci None = centres at 0."""
    n = xi.shape[0]
    out = np.zeros(n, dtype=np.int64)
    ok = (labels >= 0) & (labels < k)
    for a in range(0, n, 8192):
        s = slice(a, a + 8192)
        df = xi[s].astype(np.float64)                       # exact: |difference| < 2^22, a row's sum of squares < 2^53
        if ci is not None:
            df -= ci[np.clip(labels[s], 0, k - 1)]
        out[s] = np.where(ok[s], np.einsum("ij,ij->i", df, df).astype(np.int64), 0)
    return out


def centres(sums, counts):
    """The project's definition (oracle.kmeans_oracle.mstep): float32(float64(S) / float64(n)), NaN for an empty cluster."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((sums.astype(np.float64) * UNIT) / counts.astype(np.float64)[:, None]).astype(np.float32)


SCALE = 400                                             # exact_ints: value * 2^SCALE (covers every finite float32 and the doubles used here)


def exact_ints(a, scale=SCALE):
    """Object array of Python ints: a * 2^scale, exactly (asserted)."""
    a = np.asarray(a, dtype=np.float64)
    assert np.isfinite(a).all()
    m, e = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64)
    sh = e.astype(np.int64) - 53 + scale
    assert (sh[mi != 0] >= 0).all()
    sh = np.where(mi == 0, 0, sh)
    return np.left_shift(mi.astype(object), sh.astype(object))


def exact_inertia(xi, labels, k, c, row0=0):
    """The rows [0, row0) and [row0, n): sum_i ||x_i - c_label||^2 for arbitrary finite float32 centres as EXACT rationals, each
    returned as a Python int scaled by 2^(2 SCALE), with the three magnitudes of the a-priori bound of the sums-based evaluation
    (sum x^2, sum_k n_k ||c_k||^2, 2 sum_k |<c_k, S_k>|, same scaling, the last two rounded down to integers - they enter a bound only)."""
    co = exact_ints(c)
    out = []
    for a, b in ((0, row0), (row0, xi.shape[0])):
        s, cnt = sums_counts(xi[a:b], labels[a:b], k)
        ok = (labels[a:b] >= 0) & (labels[a:b] < k)
        x2 = sum(int(v) for v in row_inertia(xi[a:b], labels[a:b], k, None)) << (2 * SCALE + 2 * UNIT_LOG2)
        live = np.nonzero(cnt)[0]
        cc = (co[live] * co[live]).sum(axis=1) if len(live) else np.zeros(0, dtype=object)
        cs = (co[live] * s[live].astype(object)).sum(axis=1) if len(live) else np.zeros(0, dtype=object)
        ncc = sum(int(n_) * int(v) for n_, v in zip(cnt[live], cc))
        dot = sum(int(v) for v in cs) << (SCALE + UNIT_LOG2)
        absdot = sum(abs(int(v)) for v in cs) << (SCALE + UNIT_LOG2)
        out.append((x2 + ncc - 2 * dot, x2, ncc, 2 * absdot))
    return out


Spec = collections.namedtuple("Spec", "name layout n d k split seed f16 c_old kw")


def spec(layout, n, d, k, split, seed=0, f16=None, c_old=True, **kw):
    f16 = (d % 2 == 0) if f16 is None else f16
    tag = "" if f16 == (d % 2 == 0) else ",f32only"
    return Spec("%s[%d,%d,%d,s%d%s]" % (layout, n, d, k, split, tag), layout, n, d, k, split, seed, f16, c_old, tuple(sorted(kw.items())))


def case(sp):
    """The Spec's data (rows shared between the specs of one shape) with its exact reference:
    Case + (sums int64, counts, (inertia of rows [0, split), of [split, n)) as ints of grid units^2, the row-wise values)."""
    xi, x = grid_rows(sp.n, sp.d, sp.f16)
    labels = np.ascontiguousarray(LAYOUTS[sp.layout](sp.n, sp.k, sp.seed, **dict(sp.kw)), dtype=np.int32)
    assert labels.shape == (sp.n,) and 0 <= sp.split <= sp.n, sp.name
    ci = c_old = None
    if sp.c_old:
        ci = np.random.RandomState(sp.seed + 77).randint(-1000, 1001, size=(sp.k, sp.d)).astype(np.int64)
        ci.reshape(-1)[:: max(1, sp.k * sp.d // 3)] = 1 << 15                     # (centres need no fp16 copy)
        c_old = to_f32(ci)
        assert np.abs(ci).max() <= LIMIT32 and np.array_equal(c_old.astype(np.float64) / UNIT, ci), sp.name
    s, c = sums_counts(xi, labels, sp.k)
    ri = row_inertia(xi, labels, sp.k, ci)
    i0, i1 = int(ri[:sp.split].sum()), int(ri[sp.split:].sum())
    assert i0 + i1 < 2 ** 53 and np.abs(s).max(initial=0) < 2 ** 53, sp.name      # every partial sum is an exact float64
    return Case(sp.name, sp.layout, xi, x, labels, sp.k, ci, c_old, sp.split, sp.f16, kernel32(sp.n), sort_path(sp.n, sp.k)), (s, c, (i0, i1), ri)


def device_reference(ref):
    """(sums float64 [k, d], counts int64 [k], inertia float64 [2]): what the device must return, bit for bit."""
    s, c, (i0, i1), _ = ref
    return s.astype(np.float64) * UNIT, c, np.array([i0, i1], dtype=np.float64) * (UNIT * UNIT)


_cache = {}

FEW_N = (1, 31, 257, 1025, 4100)
FEW_D = (3, 64, 65, 130, 512, 768, 1000)
PROD_D = (33, 128, 130, 512, 768, 1000)
F16_D = (64, 130, 512, 768, 1024)
_K = {"uniform": 11, "one_giant": 7, "boundaries": 64, "sorted": 5, "reverse_sorted": 5, "interleaved": 13, "all_invalid": 4, "all_one": 3}
_CYCLE = ("uniform", "one_giant", "singletons", "boundaries", "sorted", "reverse_sorted", "interleaved", "all_invalid", "all_one")


def _split(i, n):
    """0, n, n // 3, 1, and a value inside a run, in turn."""
    return (0, n, n // 3, min(1, n), n // 2 + 1)[i % 5]


def _one(layout, n, d, i, **kw):
    k = max(n, 1) if layout == "singletons" else _K[layout]
    return spec(layout, n, d, k, _split(i, n), seed=i, **kw)


def mstep_specs():
    if "m" in _cache:
        return _cache["m"]
    out = []
    i = j = 0
    # few-rows float32 kernel <G, 8, 8> (and the fp16 kernel at small n where d is even)
    for d in FEW_D:
        for n in FEW_N:
            out.append(_one(_CYCLE[j % len(_CYCLE)], n, d, i))
            i, j = i + 1, j + 1
        for n in (160 + 7, 160 + 8 + 3, 160 + 16 + 7):                    # 1, 2 and 3 live waves of 8 keys in the last block
            out.append(spec("tails", n, d, 40, _split(i, n), seed=i, rows=8))
            i += 1
        out.append(spec("boundaries", 1030, d, 64, _split(i, 1030), seed=i))
        i += 1
    out.append(spec("uniform", 1025, 768, 11, 400, seed=i, f16=False))       # even d without an fp16 copy: values at +-2^20
    # the fp16 kernel's own tails (64 keys per wave at every n) and d = 1,024
    for d, n in zip(F16_D, (1280 + 37, 1280 + 64 + 20, 1280 + 128 + 50, 1280 + 64 + 1, 1280 + 128 + 63)):
        i += 1
        out.append(spec("tails", n, d, 40, _split(i, n), seed=i, rows=64))
    for j, layout in enumerate(("boundaries", "one_giant", "uniform")):
        i += 1
        out.append(_one(layout, 4100, 1024, i))
    # production float32 kernel <G, 64, 8>: n = 32,513 is the first n that reaches it (one key in the last block)
    for d in PROD_D + (64, 1024):
        i += 1
        out.append(spec("tails", 32513, d, 200, _split(i, 32513), seed=i, rows=64))
    big = ("boundaries", "one_giant", "interleaved", "singletons", "sorted", "uniform", "reverse_sorted", "boundaries")
    for d, layout in zip(PROD_D + (64, 1024), big):
        i += 1
        out.append(_one(layout, 33000, d, i))
    for layout in _CYCLE:                                                  # every layout on the production kernel, at the cheapest d
        if layout != "boundaries":
            i += 1
            out.append(_one(layout, 33000, 33, i))
    for layout in ("boundaries", "one_giant", "singletons"):               # and on the fp16 kernel above the threshold
        i += 1
        out.append(_one(layout, 33000, 130, i))
    out.append(spec("tails", 32768 + 100, 130, 200, 7, seed=i + 1, rows=64))          # two live waves
    out.append(spec("tails", 32768 + 150, 33, 200, 32000, seed=i + 2, rows=64))       # three
    # the sort stage
    out.append(spec("uniform", 4100, 64, 1, 1000, seed=3))
    out.append(spec("singletons", 4100, 8, 8191, 1367, seed=4))
    out.append(spec("singletons", 4100, 8, 8192, 1367, seed=5))
    out.append(spec("interleaved", 33000, 8, 8191, 11000, seed=6))
    out.append(spec("uniform", 33000, 8, 8192, 11000, seed=7))
    out.append(spec("uniform", 1200000, 8, 8191, 400000, seed=8))
    out.sort(key=lambda sp: (sp.n, sp.d, sp.f16))                          # specs of one shape share their rows: keep them together
    names = [c.name for c in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    _cache["m"] = out
    return out


def by_name(name):
    for c in mstep_specs():
        if c.name == name:
            return c
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ incremental M-step: label-level cases
Delta = collections.namedtuple("Delta", "name xi k l_num prev new")


def delta_cases():
    """(labels_prev -> labels) transitions for mstep_delta_kernel, rows [labelled ; unlabelled], fp16-exact grid rows with
    rows * max|x| < 2^29.  Labelled rows never change.  `prev` may hold -1 (never assigned: the first step) and `new` labels outside [0, k)."""
    if "d" in _cache:
        return _cache["d"]
    out = []
    k = 9
    for l_num in (0, 37):
        n_u = 64 * 4 + 29
        n = l_num + n_u
        xi, _ = grid_rows(n, 64, True, seed=5)
        assert n * np.abs(xi).max() * UNIT < 2 ** 29
        rs = np.random.RandomState(l_num)
        base = rs.randint(0, k, size=n).astype(np.int32)

        def mk(tag, new, prev=base):
            new = new.copy()
            new[:l_num] = prev[:l_num]
            out.append(Delta("%s[l%d]" % (tag, l_num), xi, k, l_num, prev.copy(), new))
        mk("none", base)
        one = base.copy(); one[l_num + 5] = (one[l_num + 5] + 1) % k
        mk("one", one)
        wave = base.copy(); wave[l_num + 64:l_num + 128] = (wave[l_num + 64:l_num + 128] + 3) % k
        mk("wave", wave)
        edge = base.copy()
        for p in (63, 64, 65, n_u - 1):
            edge[l_num + p] = (edge[l_num + p] + 1) % k
        mk("edges", edge)
        last = base.copy(); last[n - 29:] = (last[n - 29:] + 2) % k
        mk("ragged", last)
        tailonly = base.copy(); tailonly[n - 1] = (tailonly[n - 1] + 1) % k      # a change nowhere but in the last l_num rows' range
        mk("last_row", tailonly)
        empt = base.copy(); empt[(empt == 4) & (np.arange(n) >= l_num)] = 5
        mk("emptied", empt)
        mk("refilled", base, prev=np.where(np.arange(n) < l_num, base, empt).astype(np.int32))
        mk("all", ((base + 1) % k).astype(np.int32))
        inv = base.copy(); inv[l_num + 7], inv[l_num + 70] = -1, k
        mk("to_invalid", inv)
        mk("from_invalid", base, prev=np.where(np.arange(n) < l_num, base, inv).astype(np.int32))
    _cache["d"] = out
    return out


# ------------------------------------------------------------------------------------------------ exact centre shift, sums of squares
def exact_shift(c_new, c_old, mode):
    """scd_kmeans_finalize's shift of two finite float32 centre sets as a Fraction: mode 1 sum_k ||dc_k||^2 (exact); mode 0
    (sum_k ||dc_k||)^2 with every square root taken to ~SCALE bits (floor: a relative error below 2^-300)."""
    from fractions import Fraction
    from math import isqrt
    df = exact_ints(c_new) - exact_ints(c_old)
    q = (df * df).sum(axis=1)                                   # scaled by 2^(2 SCALE)
    if mode:
        return Fraction(sum(int(v) for v in q), 1 << (2 * SCALE))
    t = sum(isqrt(int(v)) for v in q)
    return Fraction(t * t, 1 << (2 * SCALE))


def exact_sumsq(v, a, b):
    """(sum of v[a:b]^2 as a Fraction, log2 of the squares' common unit) for a flat fp16 / float32 array of any length, vectorised: a
    value is M 2^E with an integer |M| < 2^24; M^2 < 2^48 is split in two 24-bit halves whose per-exponent sums stay below 2^53.
    The common unit is the largest power of two that divides every square (None for an empty or all-zero part)."""
    from fractions import Fraction
    v = np.asarray(v).reshape(-1)[a:b].astype(np.float64)
    assert np.isfinite(v).all() and len(v) < 2 ** 28
    f, e = np.frexp(v)
    M = np.abs(f) * 2.0 ** 24
    assert np.array_equal(M, np.floor(M))                       # a 24-bit significand: fp16 or float32 input
    M = M.astype(np.int64)
    nz = M != 0
    if not nz.any():
        return Fraction(0), None
    M, E = M[nz], e[nz].astype(np.int64) - 24
    low = M & -M                                                  # the lowest set bit: M 2^E = odd * low * 2^E
    unit = int((2 * (E + np.frexp(low.astype(np.float64))[1] - 1)).min())
    sq = M * M
    e0 = int(E.min())
    idx = E - e0
    hi = np.bincount(idx, weights=(sq >> 24).astype(np.float64))          # exact: each below 2^24 * 2^28
    lo = np.bincount(idx, weights=(sq & ((1 << 24) - 1)).astype(np.float64))
    tot = sum(((int(h) << 24) + int(l)) << (2 * i) for i, (h, l) in enumerate(zip(hi, lo)))
    return Fraction(tot) * Fraction(2) ** (2 * e0), unit


# ------------------------------------------------------------------------------------------------ scenes for the incremental step
D = 64
SPECIAL = (63, 64, 65, -1)                 # unlabelled positions (the last: in the ragged wave) that single centres can pull over


class Scene:
    """fp16-exact grid rows round k anchors (random in +-512 units, ~1e7 units^2 apart), noise +-4 units per coordinate.  Row i of the
    unlabelled part has the home anchor (i // 64) % k for k < 128 (a home is one 64-row wave) or i % k (most homes have ONE row).  Each
    SPECIAL row sits 64 units off its home P in one coordinate j, and a cluster Q of its own has its anchor at a_P + 256 e_j: with
    c_Q = a_P + 100 e_j the special row (36^2 against 64^2) moves to Q and no other row does."""

    def __init__(self, k, n_u, l_num, seed):
        rs = np.random.RandomState(seed)
        self.k, self.n_u, self.l_num = k, n_u, l_num
        self.block = k < 128
        assert not self.block or n_u <= 64 * k
        self.home = (np.arange(n_u) // 64) % k if self.block else np.arange(n_u) % k
        a = rs.randint(-512, 513, size=(k, D)).astype(np.int64)
        self.sp = [p % n_u for p in SPECIAL]
        P = [int(self.home[p]) for p in self.sp]
        free = [j for j in range(k) if j not in P]
        stride = max(1, min(3, len(free) // 4))
        self.Q = [free[-1 - i * stride] for i in range(4)]
        assert len(set(self.Q)) == 4
        self.J = [(7 * i + 3) % D for i in range(4)]
        for p, q, j in zip(P, self.Q, self.J):
            a[q] = a[p]
            a[q, j] += 256
        self.a, self.P = a, P
        xu = a[self.home] + rs.randint(-4, 5, size=(n_u, D))
        for s, p, j in zip(self.sp, P, self.J):
            xu[s, j] = a[p, j] + 64
        self.lab_fixed = (np.arange(l_num) * 3) % k
        xl = a[self.lab_fixed] + rs.randint(-4, 5, size=(l_num, D))
        self.xi = np.concatenate([xl, xu]).astype(np.int32)
        self.x = to_f32(self.xi)
        assert np.abs(self.xi).max() <= LIMIT16 and np.array_equal(self.x.astype(np.float16).astype(np.float32), self.x)
        assert len(self.xi) * float(np.abs(self.x).max()) < 2.0 ** 29          # the incremental M-step's exact-sums condition
        self._labels = {}

    def pulled(self, which):
        c = self.a.copy()
        for i in which:
            c[self.Q[i]] = self.a[self.P[i]]
            c[self.Q[i], self.J[i]] += 100
        return c

    def labels(self, c):
        """Exact argmin of the unlabelled rows for float32 centres given in grid units (float64 [k, D]), asserted unique: on the grid the
        float64 distances are exact integers; off the grid (means) they are within ~1e-6 units^2, and the margin is asserted above 1."""
        key = c.tobytes()
        if key not in self._labels:
            xu = self.xi[self.l_num:].astype(np.float64)
            cn = (c * c).sum(axis=1)
            out = np.empty(self.n_u, dtype=np.int64)
            for s in range(0, self.n_u, 1024):
                dist = (xu[s:s + 1024] ** 2).sum(axis=1)[:, None] + cn[None, :] - 2.0 * (xu[s:s + 1024] @ c.T)
                best = np.argmin(dist, axis=1)
                out[s:s + 1024] = best
                if self.k > 1:
                    rows = np.arange(len(best))
                    first = dist[rows, best].copy()
                    dist[rows, best] = np.inf
                    assert (dist.min(axis=1) - first >= 1.0).all(), "the scene has a row without a unique nearest centre"
            self._labels[key] = out
        return self._labels[key]


def scene_means(sc):
    """float32 means of the base assignment, in grid units: centres OFF the grid (thirds, sevenths) for the double-double evaluation."""
    lab = np.concatenate([sc.lab_fixed, sc.labels(sc.a.astype(np.float64))]).astype(np.int32)
    s, c = sums_counts(sc.xi, lab, sc.k)
    assert (c > 0).all()
    return centres(s, c).astype(np.float64) / UNIT
