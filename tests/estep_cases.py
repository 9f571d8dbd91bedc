"""Adversarial inputs for the k-means E-step filters (scd_amd/csrc/kmeans.hip: estep_stream_kernel, estep_rb_kernel, estep_mfma_kernel,
muf_filter_kernel).  numpy only, deterministic.

Every case lies on an EXACT GRID: each coordinate of a row or a centre is an integer times one power of two, |integer| <= 2^20, D <= 1024.
A difference then has <= 21 bits, its square <= 42, a sum of <= 1024 squares <= 52: the float64 difference-form distance is exact in any
summation order, with or without FMA, and so is the float64 form ||x||^2 + ||c||^2 - 2 x.c.  The oracle's argmin (ties to the lowest
index) is therefore the one right label of EVERY row - no tolerance band, no row left out.  `_finish` asserts the grid property.

Which filter a shape reaches (scd_kmeans_estep, Dp = D rounded up to 128, Kp = K rounded up to 128): `path`.
  rb        Dp = 512 and 128 < Kp <= 2048        estep_rb_kernel
  stream1   Kp = 128, Dp <= 768                  estep_stream_kernel, one pass
  streamN   128 < Kp <= 2048, Dp <= 768          estep_stream_kernel, one pass per 128 centres
  legacy    everything else                      estep_mfma_kernel
The split last round of estep_rb_kernel (+ estep_rb_merge_kernel) needs more 256-row blocks than the chip has compute units
(`nblk > ncu`, i.e. n > 65,536 rows on an MI355X): no small n reaches it.  It is covered by test_estep_rb_split_last_round and by the
ladder family at that test's smaller shape (test_gpu_estep_bounds.test_estep_rb_split_last_round_ladder).

The ladder construction shared by the families: for a pair c_b = c_a + 2 g on a coordinate set J, a row with x_J = c_a,J + g + t has
d(x, c_b) - d(x, c_a) = -4 t g |J| whatever its other coordinates are: t runs over 0, +-1, +-2, +-4, ...; t = 0 is an exact tie.  A third
centre c_3 = c_a + g on J, + h on one more coordinate l with h^2 = |J| g^2, seen from a row with x_l = c_a,l, lies at
d(x, c_3) - d(x, c_a) = -2 t g |J|: halfway between the two (a three-way tie at t = 0).
"""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name family x c path ties")     # ties: rows whose two smallest exact distances are equal

LIMIT = 1 << 20
SHAPES = {                                # path -> (D, K) of the issue's table
    "stream1": [(64, 8), (768, 128)],
    "streamN": [(256, 129), (640, 300)],
    "rb": [(512, 129), (448, 300), (512, 2048)],
    "legacy": [(64, 2049), (896, 16), (1024, 130)],
}


def path(d, k):
    dp, kp = (d + 127) // 128 * 128, (k + 127) // 128 * 128
    if dp == 512 and 128 < kp <= 2048:
        return "rb"
    if kp <= 2048 and dp <= 768:
        return "stream1" if kp == 128 else "streamN"
    return "legacy"


def exact_dist(xi, ci):
    """Exact squared distances of integer rows / centres (float64 holds every partial sum: all are integers below 2^53)."""
    x, c = xi.astype(np.float64), ci.astype(np.float64)
    return (x * x).sum(1)[:, None] + (c * c).sum(1)[None, :] - 2.0 * (x @ c.T)


def _finish(name, family, xi, ci, unit_log2=-10, nan_rows=()):
    xi, ci = np.asarray(xi, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    assert xi.ndim == 2 and ci.ndim == 2 and xi.shape[1] == ci.shape[1] <= 1024
    assert np.abs(xi).max(initial=0) <= LIMIT and np.abs(ci).max(initial=0) <= LIMIT, name        # the grid property
    d = exact_dist(xi, ci)
    if len(nan_rows):
        d[:, list(nan_rows)] = np.inf
    two = np.partition(d, 1, axis=1)[:, :2] if ci.shape[0] > 1 else np.stack([d[:, 0], d[:, 0] + 1], 1)
    unit = np.float32(2.0 ** unit_log2)
    x, c = xi.astype(np.float32) * unit, ci.astype(np.float32) * unit
    assert np.array_equal(x.astype(np.float64) / float(unit), xi) and np.array_equal(c.astype(np.float64) / float(unit), ci)
    for r in nan_rows:
        c[r] = np.nan                                             # a dead centre (empty cluster): never wins
    return Case(name, family, x, c, path(xi.shape[1], ci.shape[0]), np.nonzero(two[:, 0] == two[:, 1])[0])


def _ts(n, tmax_log2, rs):
    """n ladder steps: 0, +-1, +-2, ..., +-2^tmax_log2, cycled (about one row in 2 tmax_log2 + 3 is an exact tie)."""
    lad = [0] + [s * (1 << p) for p in range(tmax_log2 + 1) for s in (1, -1)]
    return np.array([lad[i % len(lad)] for i in rs.permutation(n)], dtype=np.int64)


def _pair_slots(k, npairs, rs):
    """Centre indices (a, b, third) of the pairs: spread over the index range, b > a and b < a; with more than 130 centres the first
    pair sits astride the first 128-centre chunk border with its third centre in the last chunk."""
    if k < 3:
        return [(0, 1, None)] if k == 2 else []
    perm = [int(v) for v in rs.permutation(k)]
    if k > 130:
        perm = [127, 128, k - 1] + [v for v in perm if v not in (127, 128, k - 1)]
    return [tuple(perm[3 * p:3 * p + 3]) for p in range(min(npairs, k // 3))]


# ------------------------------------------------------------------------------------------------ families
def ladder(n, d, k, seed=0, S=1 << 10, W=24, g=1 << 7, tmax=9, nJ=(1, 4)):
    """Pairs of centres inside the data box, rows on a geometric ladder of true margins -4 t g |J| from ~S^2 down to one grid step and to
    0, both signs.  Pairs with an even number get a third centre inside the ladder, seen by every other of their rows (see the module
    docstring); for all other rows every other centre is far (~D S^2 / 6).  Pairs b > a and b < a, also astride a 128-centre chunk border."""
    rs = np.random.RandomState(seed)
    ci = rs.randint(-S // 2, S // 2 + 1, size=(k, d)).astype(np.int64)
    slots = _pair_slots(k, 4, rs)
    xi = np.empty((n, d), dtype=np.int64)
    ts = _ts(n, tmax, rs)
    for s, (a, b, t3) in enumerate(slots):
        m = nJ[(s // 2) % len(nJ)]
        J, l = _J(d, s, m), _L(d, s)
        assert l not in J
        ci[b] = ci[a]
        ci[b, J] += 2 * g
        if s % 2 == 0:
            ci[t3] = ci[a]
            ci[t3, J] += g
            ci[t3, l] += int(round(np.sqrt(m))) * g
        rows = np.arange(s, n, len(slots))
        xi[rows] = ci[a][None, :] + rs.randint(-W, W + 1, size=(len(rows), d))
        xi[np.ix_(rows, J)] = (ci[a, J] + g)[None, :] + ts[rows][:, None]
        xi[rows[1::2], l] = ci[a, l]
    return _finish("ladder[%d,%d,%d]" % (n, d, k), "ladder", xi, ci)


def _J(d, slot, m):
    return (np.arange(m) * 3 + 7 * slot + 1) % d


def _L(d, slot):
    return (7 * slot + 2) % d


def long_centres(n, d, k, seed=0, S=1 << 10, W=3, q=24, tmax=9):
    """Rows near the data mean, every centre on a corner of the data box (|c'_j| ~ 16 in every column, ||c'||^2 ~ 256 D): the largest
    key-truncation and hi + lo errors.  Pairs: c_b = c_a with ONE coordinate's sign flipped; a row leans to its pair's corner by q and has
    x_j = t on that coordinate: d(x, c_b) - d(x, c_a) = +-4 t (S - 1), t on the ladder.  Two rows at +-(S - 1) pin the box."""
    rs = np.random.RandomState(seed)
    sig = rs.randint(0, 2, size=(k, d)).astype(np.int64) * 2 - 1
    slots = _pair_slots(k, 4, rs)
    for s, (a, b, t3) in enumerate(slots):
        sig[b] = sig[a]
        sig[b, _L(d, s)] *= -1
    ci = sig * (S - 1)
    xi = rs.randint(-W, W + 1, size=(n, d)).astype(np.int64)
    ts = _ts(n, tmax, rs)
    for r in range(n):
        a = slots[r % len(slots)][0] if slots else 0
        xi[r] += q * sig[a]
        if slots:
            xi[r, _L(d, r % len(slots))] = ts[r]
    xi[0], xi[1] = S - 1, -(S - 1)
    tag = "" if (q, W) == (24, 3) else ",q%d,W%d" % (q, W)
    return _finish("long_centres[%d,%d,%d%s]" % (n, d, k, tag), "long_centres", xi, ci)


def same_sign(n, d, k, seed=0, S=1 << 10, g=1 << 7, tmax=8):
    """Every product x'_j c'_j of a row with its near centres is positive in all D columns (rows come with their mirror images, so the
    mean is 0 and centring changes nothing; pairs live in the positive orthant, mirrored pairs in the negative one): the fp32
    accumulation of D same-sign terms of size ~144.  Ladder of margins -4 t g |J| with |J| = 1 and 16."""
    rs = np.random.RandomState(seed)
    assert n % 2 == 0
    ci = rs.randint(S // 2, S, size=(k, d)).astype(np.int64) * (rs.randint(0, 2, size=(k, 1)) * 2 - 1)
    slots = _pair_slots(k, 4, rs)
    h = n // 2
    xi = np.empty((n, d), dtype=np.int64)
    ts = _ts(h, tmax, rs)
    for s, (a, b, t3) in enumerate(slots):
        m = (1, 16)[s % 2]
        J = _J(d, s, m)
        ci[a] = np.abs(ci[a])
        ci[a, J] = S // 2
        ci[b] = ci[a]
        ci[b, J] += 2 * g                                          # S / 2 + 2 g < S
        rows = np.arange(s, h, len(slots))
        xi[rows] = ci[a][None, :] + rs.randint(-8, 9, size=(len(rows), d))
        xi[np.ix_(rows, J)] = (ci[a, J] + g)[None, :] + ts[rows][:, None]
    xi[h:] = -xi[:h]
    # mirrored pairs serve the mirrored rows
    for s, (a, b, t3) in enumerate(slots):
        if t3 is not None:
            ci[t3] = -ci[a if s % 2 == 0 else b]                   # one mirrored centre per pair: mirrored rows see a far second
    return _finish("same_sign[%d,%d,%d]" % (n, d, k), "same_sign", xi, ci)


def outlier_scale(n, d, k, seed=0, spread=8, centre_outlier=False):
    """One row at 2^20 grid units sets the scale; the bulk sits at 0..spread units, so its x' is fp16-subnormal or zero (one unit is
    2^-17 after scaling).  The centres that matter differ by ONE unit in one coordinate (ties at the rows halfway - spread >= 2 - and
    margins of one and three units^2).  centre_outlier: one coordinate of one more centre at 2^20 units (a long centre: cmax ~ 8)."""
    rs = np.random.RandomState(seed)
    xi = rs.randint(0, spread + 1, size=(n, d)).astype(np.int64)
    ci = rs.randint(0, spread + 1, size=(k, d)).astype(np.int64)
    for p in range(k // 2):                                       # pairs (2p, 2p + 1) or reversed: one unit apart in coordinate p % d
        a, b = (2 * p, 2 * p + 1) if p % 2 == 0 else (2 * p + 1, 2 * p)
        ci[b] = ci[a]
        ci[b, p % d] = ci[a, p % d] + (1 if ci[a, p % d] < spread else -1)
    for r in range(n):                                            # a row sits on / next to its pair's first centre
        p = r % max(1, k // 2)
        xi[r] = ci[min(2 * p, k - 1)]
        flip = rs.randint(0, d, size=min(d, 3))
        xi[r, flip] = rs.randint(0, spread + 1, size=len(flip))
    xi[0] = 0
    xi[0, 0] = LIMIT
    if centre_outlier:
        ci[k - 1, d - 1] = LIMIT
    return _finish("outlier_scale[%d,%d,%d,%d,%d]" % (n, d, k, spread, centre_outlier), "outlier_scale", xi, ci, unit_log2=-20)


def offset(n, d, k, seed=0, spread=6):
    """Every coordinate carries the common offset 2^19 units, the data spread is a few units: centring has to remove the offset (a
    filter on the raw values would see nothing but 2^19).  Centres are rows, rows + one unit, and near-tie pairs one unit apart."""
    rs = np.random.RandomState(seed)
    base = 1 << 19
    xi = base + rs.randint(-spread, spread + 1, size=(n, d)).astype(np.int64)
    ci = xi[rs.choice(n, k, replace=n < k)].copy()
    for p in range(k // 2):
        a, b = (2 * p, 2 * p + 1) if p % 2 else (2 * p + 1, 2 * p)
        ci[b] = ci[a]
        ci[b, (3 * p) % d] += 2
    for r in range(0, n, 2):                                      # every other row: on a pair's midpoint +- one unit
        p = (r // 2) % max(1, k // 2)
        a = 2 * p + 1 if p % 2 == 0 else 2 * p
        if k >= 2:
            xi[r] = ci[min(a, k - 1)] + (rs.randint(-1, 2, size=d) * (rs.rand(d) < 0.05))
            xi[r, (3 * p) % d] = min(ci[2 * p, (3 * p) % d], ci[2 * p + 1, (3 * p) % d]) + 1 + (r // 2 // max(1, k // 2)) % 3 - 1
    return _finish("offset[%d,%d,%d]" % (n, d, k), "offset", xi, ci, unit_log2=-8)


def outside_box(n, d, k, variant, seed=0):
    """Rows in a box of +-8 units (x' = x: scale 2^0); centres at 2, 64, 1024, 8192 and 2^17 times the box in one coordinate: at 8192 and
    2^17 c' overflows fp16, at 1024 (and, for Dp <= 512, at 64) only ||c'||^2 leaves the range of the single-pass filter's extension column.
    variant "near": the other centres are in the box (the far ones must simply lose - an fp16 infinity makes them win or poisons the row).
    variant "far":  the in-box centres are pushed out to 2^20 in TWO coordinates, so every row's nearest centre is one of the two centres at
    1024 x, which differ by two units in coordinate 3: ties at x_3 = 1, margins of 4 units^2 per step."""
    rs = np.random.RandomState(seed)
    xi = rs.randint(-8, 9, size=(n, d)).astype(np.int64)
    ci = rs.randint(-8, 9, size=(k, d)).astype(np.int64)
    fac = [2, 64, 1024, 1024, 8192, 1 << 17]
    where = [int(v) for v in np.linspace(0, k - 1, len(fac)).round()] if k >= len(fac) else list(range(k))
    far = {}
    for f, idx in zip(fac[-len(where):] if k < len(fac) else fac, where):
        far[idx] = f
    if variant == "far":
        ci[:, 1] = LIMIT
        ci[:, 2] = -LIMIT
    pair = [i for i, f in far.items() if f == 1024]
    for idx, f in far.items():
        ci[idx] = rs.randint(-8, 9, size=d)
        if f == 1024 and len(pair) == 2:
            ci[idx] = 0
            ci[idx, 3] = 0 if idx == pair[1] else 2               # the higher index is the nearer one for x_3 < 1
        ci[idx, 0] = 8 * f * (1 if f != 8192 else -1)
        if variant == "far" and f < 1024:
            ci[idx, 1], ci[idx, 2] = LIMIT, -LIMIT
    xi[:, 3] = np.arange(n) % 5 - 1                               # -1 .. 3: both sides of the tie at x_3 = 1
    return _finish("outside_box[%d,%d,%d,%s]" % (n, d, k, variant), "outside_box", xi, ci, unit_log2=0)


def degenerate(kind, n=333, d=64, k=8, seed=0):
    """constant: every row the same constant vector (maxabs = 0, scale 2^0); repeated: one arbitrary row n times; k1: K = 1;
    same_centres: all centres identical; rows_as_centres: centres are rows (distance exactly 0), some twice; nan_centre: dead centres."""
    rs = np.random.RandomState(seed)
    xi = rs.randint(-500, 501, size=(n, d)).astype(np.int64)
    ci = rs.randint(-500, 501, size=(k, d)).astype(np.int64)
    nan_rows = ()
    if kind == "constant":
        xi[:] = 37
        ci[k // 2] = 37
        ci[k - 1] = 37
    elif kind == "repeated":
        xi[:] = xi[0]
        ci[k - 1] = xi[0]
        ci[1] = xi[0]
        ci[1, 5] += 1
    elif kind == "k1":
        ci = ci[:1]
    elif kind == "same_centres":
        ci[:] = ci[0]
    elif kind == "rows_as_centres":
        ci = xi[rs.choice(n, k, replace=False)].copy()
        ci[k - 1] = ci[0]                                          # a duplicate: its rows tie, the lower index wins
    elif kind == "nan_centre":
        ci[0] = xi[0]
        nan_rows = (0, k - 2)
    else:
        raise ValueError(kind)
    return _finish("degenerate[%s,%d,%d,%d]" % (kind, n, d, ci.shape[0]), "degenerate", xi, ci, nan_rows=nan_rows)


# ------------------------------------------------------------------------------------------------ the case lists
_N = {"stream1": (333, 700), "streamN": (700, 420), "rb": (700, 333, 520), "legacy": (333, 420, 300)}     # 333: ragged unit; 700, 420: ragged block


def _shapes(paths):
    for p in paths:
        for (d, k), n in zip(SHAPES[p], _N[p]):
            assert path(d, k) == p
            yield n, d, k


ALL = ("stream1", "streamN", "rb", "legacy")
THREE = ("stream1", "streamN", "rb")
_cache = {}


def estep_cases():
    """Every E-step case but outside_box: (ladder, long_centres on all four paths; same_sign at Dp = 768 / 1024 and on rb; the rest on the
    two stream forms and rb)."""
    if "e" not in _cache:
        out = []
        for n, d, k in _shapes(ALL):
            out.append(ladder(n, d, k, seed=d + k))
            out.append(long_centres(n, d, k, seed=d + k + 1))
        out.append(ladder(2100, 512, 300, seed=5))                # more than eight 256-row blocks, ragged
        # rows CLOSE to the mean (small lean q, no scatter): ||x'|| is small, so E is mostly B, and B mostly the key term
        out.append(long_centres(520, 512, 2048, seed=0, q=8))
        out.append(long_centres(700, 768, 128, seed=0, q=1, W=0))
        out.append(long_centres(700, 640, 300, seed=0, q=1, W=0))
        for swap in (0, 1):                                       # (the single-pass path's key term is too large for this family)
            out.append(subnormal_tie(333, 896, 2, swap, seed=898, U=100))
            out.append(subnormal_tie(333, 64, 2, swap, seed=66, U=4))
            out.append(subnormal_tie(700, 768, 128, swap, seed=896, U=4))
        for n, d, k in [(700, 768, 128), (420, 1024, 130), (700, 512, 129), (420, 640, 300)]:
            out.append(same_sign(n, d, k, seed=d + k + 2))
        for n, d, k in _shapes(THREE):
            out.append(outlier_scale(n, d, k, seed=d + k + 3, spread=8))
            out.append(outlier_scale(n, d, k, seed=d + k + 4, spread=1))
            out.append(offset(n, d, k, seed=d + k + 5))
        out.append(outlier_scale(333, 64, 8, seed=9, spread=8, centre_outlier=True))
        out.append(outlier_scale(700, 512, 129, seed=9, spread=8, centre_outlier=True))
        for kind in ("constant", "repeated", "k1", "same_centres", "rows_as_centres", "nan_centre"):
            out.append(degenerate(kind))
        out.append(degenerate("rows_as_centres", n=520, d=512, k=200))
        out.append(degenerate("nan_centre", n=520, d=512, k=200))
        out.append(degenerate("nan_centre", n=420, d=256, k=129))
        out.append(degenerate("same_centres", n=300, d=896, k=16))
        _cache["e"] = out
    return _cache["e"]


def outside_box_cases():
    if "o" not in _cache:
        out = []
        for n, d, k in [(333, 64, 8), (420, 256, 129), (700, 512, 129), (333, 448, 300), (300, 896, 16), (333, 64, 2049)]:
            for variant in ("near", "far"):
                out.append(outside_box(n, d, k, variant, seed=d + k))
        _cache["o"] = out
    return _cache["o"]


def by_name(name):
    for c in estep_cases() + outside_box_cases():
        if c.name == name:
            return c
    raise KeyError(name)


def subnormal_tie(n, d, k, swap, seed=0, U=100, rmax=8):
    """The fp16-subnormal term of the bounds as the deciding one.  All rows but two are ONE grid point v; the two others are outliers at
    +-(2^20 - 4) units in coordinate 0 (they set the scale: one grid unit is 2^-17 of x') and differ from mirror images by a few units, so
    the mean sits a fraction of a unit off v: the bulk's x' is a few fp16-subnormal quanta (2^-24) long and rounds by up to half of one.
    Centres 0 and 1 are v +- U sigma (sigma a sign vector; `swap` exchanges them): exactly equidistant from v - every bulk row is an
    exact tie and belongs to centre 0 - and OPPOSITE, so the rounding of x' does not cancel between them: the filter's two scores differ
    by ~2 * 2^-25 * ||c_0' - c_1'|| ~ 2e-10, while every other term of E is ~1e-11 (||c'|| ~ 6e-3, ||x'|| ~ 1e-6).  Without 6e-8 sqrt(Dp)
    the filter decides the tie itself, and in one of the two `swap` variants for the higher index.  The other centres are v + U sigma_k
    with one coordinate at U + 1: 2 U + 1 units^2 farther, no longer."""
    rs = np.random.RandomState(seed)
    v = rs.randint(-3, 4, size=d).astype(np.int64)
    xi = np.tile(v, (n, 1))
    xi[0, 0] += LIMIT - 4
    xi[1, 0] -= LIMIT - 4
    xi[1, 1:] += rs.randint(-rmax, rmax + 1, size=d - 1)
    sig = rs.randint(0, 2, size=(k, d)).astype(np.int64) * 2 - 1
    ci = v[None, :] + U * sig
    ci[1] = v - U * sig[0]
    if swap:
        ci[[0, 1]] = ci[[1, 0]]
    for j in range(2, k):
        ci[j, j % d] += sig[j, j % d]
    return _finish("subnormal_tie[%d,%d,%d,%d,U%d]" % (n, d, k, swap, U), "subnormal_tie", xi, ci, unit_log2=-20)
