"""The PCA contract restated in float64 numpy (scd_pca_colsum / scd_pca_gram / scd_pca_transform, scd_amd/pca.py), its error model, the
cases and the planted mistakes.  docs/design/pca.md derives the bounds.  Everything here is evaluated at the SAME float32
c = fl32(x - a) the device forms (one IEEE subtraction, which numpy float32 reproduces bit for bit), so the only difference a test sees
is the device's rounding."""
import numpy as np

import f32mm_plan as fp

U = 2.0 ** -24                                  # unit roundoff of float32
EPS64 = float(np.finfo(np.float64).eps)
ROW_TILE = 32                                   # scd_pca_row_tile(); the host test asserts the library agrees
CHAIN_ROWS = 256                                # scd_pca_chain_rows()
TILE = 128                                      # the Gram tile
T = CHAIN_ROWS


def gamma(k):
    return k * U / (1.0 - k * U)


def gamma64(k):
    return k * (EPS64 / 2) / (1.0 - k * (EPS64 / 2))


def eps_m(m):
    """Relative error of a unit row's element beyond the projection's own: the float32 sum of m squares (m roundings in any order, all
    terms >= 0: relative gamma_m, and |1 / sqrt(1 + t) - 1| <= |t| for |t| <= 1/2), the correctly rounded sqrtf (u) and division (u),
    and the products of these factors: (m + 4) u covers (1 + gamma_m)(1 + u)^2 - 1 for m <= 1024."""
    return (m + 4) * U


# ------------------------------------------------------------------------------------------------- the contract
def centred(X, a, mistake=None):
    """c = fl32(x - a) as float64 [n, d]; a None means no shift."""
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    if a is None or mistake == "shift_not_subtracted":
        return X32.astype(np.float64)
    return (X32 - np.asarray(a, np.float32)[None, :]).astype(np.float64)


def rounded_mean(X):
    return np.asarray(X, np.float64).mean(axis=0).astype(np.float32)


def colsum_f64(X, a, mistake=None):
    if mistake == "csum_from_x":
        return np.asarray(X, np.float64).sum(axis=0)
    c = centred(X, a, mistake)
    if mistake == "colsum_range_tail_dropped":                  # a column-sum range loses the rows past its last whole group of eight
        n = c.shape[0]
        keep = np.ones(n)
        for lo, hi in fp.range_bounds(n, *fp.colsum_ranges(n)):
            keep[hi - (hi - lo) % fp.CS_GROUPS:hi] = 0.0
        return (c * keep[:, None]).sum(axis=0)
    return c.sum(axis=0)


def gram_f64(X, a, mistake=None):
    """G = c^T c in float64, with `mistake` (one of MISTAKES) planted."""
    c = centred(X, a, mistake)
    n, d = c.shape
    mult = np.ones(n)
    if mistake == "ragged_block_dropped":
        mult[n // ROW_TILE * ROW_TILE:] = 0.0
    if mistake == "chain_row_twice" and n > CHAIN_ROWS:
        mult[CHAIN_ROWS - 1] = 2.0
    plan = fp.pca_plan(n, d)
    if mistake == "last_range_dropped":
        mult[(plan["R"] - 1) * plan["rows"]:] = 0.0
    if mistake == "range_added_twice":
        mult[plan["rows"]:2 * plan["rows"]] = 2.0
    G = (c * mult[:, None]).T @ c
    if mistake == "range_stride_of_one_tile":                   # every tile but the first reads range 0's partial R times
        first = (np.arange(d)[:, None] < TILE) & (np.arange(d)[None, :] < TILE)
        G = np.where(first, G, plan["R"] * (c[:plan["rows"]].T @ c[:plan["rows"]]))
    tiles = [(s, min(s + TILE, d)) for s in range(0, d, TILE)]
    if mistake == "diag_tile_twice":
        for lo, hi in tiles:
            G[lo:hi, lo:hi] *= 2.0
    if mistake == "mirror_untransposed":
        for i, (a0, a1) in enumerate(tiles):
            for b0, b1 in tiles[i + 1:]:
                blk = np.zeros((b1 - b0, a1 - a0))
                r, s = min(b1 - b0, a1 - a0), min(a1 - a0, b1 - b0)
                blk[:r, :s] = G[a0:a0 + r, b0:b0 + s]           # the upper tile as it lies, not its transpose
                G[b0:b1, a0:a1] = blk
    return G


def scatter_f64(X, a, mistake=None):
    """(S = G - csum csum^T / n, mean = a + csum / n) in float64: exactly the centred scatter and the mean of the rows a + c."""
    n = np.shape(X)[0]
    G, cs = gram_f64(X, a, mistake), colsum_f64(X, a, mistake)
    S = G if mistake == "no_correction" else G - np.outer(cs, cs) / n
    a64 = np.zeros(G.shape[0]) if a is None else np.asarray(a, np.float64)
    return S, a64 + cs / n


def svd_flip_rows(v):
    idx = np.argmax(np.abs(v), axis=1)
    s = np.sign(v[np.arange(v.shape[0]), idx])
    s[s == 0] = 1.0
    return v * s[:, None]


def fit_f64(X, a, n_components=None, whiten=False, mistake=None):
    """scikit-learn 1.7's PCA(svd_solver='covariance_eigh') on the rows a + c.  Returns a dict: var [d] (all eigenvalues, descending,
    negatives 0), comps [d, d] (rows), ratio, sing, mean, m (the resolved n_components), noise, W [m, d] float32 (what transform
    multiplies by), cov."""
    n, d = np.shape(X)
    S, mean = scatter_f64(X, a, mistake)
    cov = S / (n if mistake == "div_n" else n - 1)
    vals, vecs = np.linalg.eigh(cov)
    if mistake != "ascending":
        vals, vecs = vals[::-1], vecs[:, ::-1]
    vals = np.where(vals < 0.0, 0.0, vals)
    comps = svd_flip_rows(np.ascontiguousarray(vecs.T))
    if mistake == "sign_flipped":
        comps[0] = -comps[0]
    ratio = vals / vals.sum()
    if n_components is None:
        m = min(n, d)
    elif isinstance(n_components, float):
        m = int(np.searchsorted(np.cumsum(ratio), n_components, side="right") + 1)
    else:
        m = int(n_components)
    noise = float(vals[m:].mean()) if m < min(n, d) else 0.0
    W = comps[:m]
    if whiten:
        W = W * np.sqrt(vals[:m])[:, None] if mistake == "whiten_mul" else W / np.sqrt(vals[:m])[:, None]
    return dict(var=vals, comps=comps, ratio=ratio, sing=np.sqrt(vals * (n - 1)), mean=mean, m=m, noise=noise,
                W=np.ascontiguousarray(W, dtype=np.float32), cov=cov)


def phantom_columns(m):
    """Columns a block computes beyond the padded width mp = m up to 32: four waves take NT = 1, 2, 4 or 8 tiles each; a tile past mp
    repeats the packed row mp - 1 (a real column only when m == mp).  tests/f32mm_plan.py restates the dispatch."""
    return fp.phantom_columns(m)


def transform_f64(X, a, W, unit=False, mistake=None):
    """y = c W^T in float64 at the float32 W; unit: rows divided by their L2 norm over the m real columns, a zero row stays zero."""
    c = centred(X, a, mistake)
    y = c @ np.asarray(W, np.float64).T
    if not unit:
        return y
    ss = (y * y).sum(axis=1)
    if mistake == "unit_over_padded":
        # every column of the block past m repeats the last real column and is counted.  With m == mp that is the kernel's own clamp to
        # the packed row mp - 1 with the mask left out; with m < mp it is that clamp taken to m - 1 instead (the row mp - 1 is zero)
        extra, mp = phantom_columns(y.shape[1])
        ss = ss + (extra + mp - y.shape[1]) * y[:, -1] ** 2
    nrm = np.sqrt(ss)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(nrm[:, None] == 0.0, 0.0, y / nrm[:, None])


# ------------------------------------------------------------------------------------------------- the error model
def colsum_bound(X, a):
    """Float64 sums of float64 conversions of c, in some order: gamma64_n sum_i |c_ij|."""
    c = centred(X, a)
    return gamma64(c.shape[0]) * np.abs(c).sum(axis=0)


def gram_bound(X, a):
    """|G_jl - G64_jl| <= gamma_T sum_i |c_ij| |c_il|: a chain of at most T float32 fmas from zero; the float64 additions across chains
    and ranges are not charged."""
    c = np.abs(centred(X, a))
    return gamma(T) * (c.T @ c)


def scatter_bound(X, a):
    """Element bounds of S = G - csum csum^T / n from those of G and csum."""
    n = np.shape(X)[0]
    cs, bc = np.abs(colsum_f64(X, a)), colsum_bound(X, a)
    return gram_bound(X, a) + (np.outer(cs, bc) + np.outer(bc, cs) + np.outer(bc, bc)) / n


def weyl_bound(X, a):
    """|lambda_k - lambda64_k| of cov = S / (n - 1): ||Bnd||_F / (n - 1) (Weyl, ||E||_2 <= ||E||_F), plus the two float64 eigensolvers'
    own backward error, d eps64 lambda_max each."""
    n, d = np.shape(X)
    lam_max = float(np.linalg.eigvalsh(scatter_f64(X, a)[0] / (n - 1))[-1])
    return float(np.linalg.norm(scatter_bound(X, a))) / (n - 1) + 2.0 * d * EPS64 * lam_max


def davis_kahan_bound(X, a, m):
    """The sine of the largest principal angle between the top-m subspaces: 2 ||E||_F / (lambda64_m - lambda64_{m+1})."""
    n = np.shape(X)[0]
    lam = np.linalg.eigvalsh(scatter_f64(X, a)[0] / (n - 1))[::-1]
    return 2.0 * weyl_bound(X, a) / (lam[m - 1] - lam[m])


def subspace_sine(V, Vh):
    """The sine of the largest principal angle between the row spaces of V and Vh (orthonormal rows)."""
    V, Vh = np.asarray(V, np.float64), np.asarray(Vh, np.float64)
    return float(np.linalg.norm(Vh.T - V.T @ (V @ Vh.T), 2))


def transform_bound(X, a, W, unit=False):
    """|y_ik - y64_ik| <= delta_ik = gamma_d sum_j |c_ij| |W_kj|.  unit: delta carried through y / ||y|| in float64,
        D_ik = delta_ik / (||y_i|| - ||delta_i||) + |y_ik| ||delta_i|| / (||y_i|| (||y_i|| - ||delta_i||)),
    then the relative eps_m on the device's own quotient: D_ik + eps_m (|yhat64_ik| + D_ik).  A row with ||y|| <= ||delta|| that is not
    exactly zero has no bound (inf); an exactly zero row (c = 0) is exact."""
    c = centred(X, a)
    W64 = np.asarray(W, np.float64)
    delta = gamma(c.shape[1]) * (np.abs(c) @ np.abs(W64).T)
    if not unit:
        return delta
    y = c @ W64.T
    ny, nd = np.linalg.norm(y, axis=1), np.linalg.norm(delta, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        D = delta / (ny - nd)[:, None] + np.abs(y) * (nd / (ny * (ny - nd)))[:, None]
        out = D + eps_m(y.shape[1]) * (np.abs(y) / ny[:, None] + D)
    out[ny <= nd] = np.inf
    out[(ny == 0.0) & (nd == 0.0)] = 0.0
    return out


def ratio(got, ref, bound):
    """The largest |got - ref| / bound; an element with a zero bound must be exact (else inf)."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.max(q)) if q.size else 0.0


# ------------------------------------------------------------------------------------------------- the cases
def unit_rows(n, d, seed):
    """Unit rows with a common offset, so the mean matters, as feature caches have."""
    rs = np.random.RandomState(seed)
    off = 1.5 * rs.standard_normal(d)
    z = rs.standard_normal((n, d)) + off[None, :]
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    return np.ascontiguousarray(z, dtype=np.float32)


# the range plans and the forward regimes of tests/f32mm_plan.py, by name
NAMED_GRAM = {name: c["gram"] for name, c in fp.RANGE_CASES.items() if "gram" in c}
NAMED_TRANSFORM = {**{name: shape for name, (shape, _) in fp.NT_CASES.items()}, "ranges_x_tiles": fp.RANGE_CASES["ranges_x_tiles"]["wide"]}
GRAM_SHAPES = [(1, 1), (31, 5), (33, 64), (T + 1, 96), (3 * T + 5, 129), (9 * T + 3, 33), (64, 1024), (231, 768)] + list(NAMED_GRAM.values())
TRANSFORM_SHAPES = [(1, 1, 1), (31, 5, 3), (33, 64, 33), (231, 768, 100), (64, 1024, 1024), (257, 96, 31), (70, 33, 257),
                    (40, 16, 32)                # m == mp and three waves on tiles past mp (unit_over_padded shows there)
                    ] + list(NAMED_TRANSFORM.values())
FIT_SHAPES = [(1500, 64, 8), (2000, 96, 16), (1200, 33, 4)]


def gram_name(n, d, shifted):
    return "n%d_d%d-%s" % (n, d, "mean" if shifted else "noshift")


def gram_cases():
    """name -> dict(X, a): every shape with the rounded mean as shift and without a shift."""
    out = {}
    for i, (n, d) in enumerate(GRAM_SHAPES):
        X = unit_rows(n, d, 100 + i)
        out[gram_name(n, d, True)] = dict(X=X, a=rounded_mean(X))
        out[gram_name(n, d, False)] = dict(X=X, a=None)
    return out


def nan_case():
    """One row with non-finite values in both dim tiles: it is counted once."""
    X = unit_rows(70, 129, 77)
    X[7, 3], X[7, 128] = np.nan, np.inf
    return dict(X=X, a=rounded_mean(unit_rows(70, 129, 77)))


def transform_name(n, d, m, kind):
    return "n%d_d%d_m%d-%s" % (n, d, m, kind)


def transform_cases():
    """name -> dict(X, a, W, unit): plain, unit, and with a whitening-scaled W (rows of very different length), the last one unit too."""
    out = {}
    for i, (n, d, m) in enumerate(TRANSFORM_SHAPES):
        rs = np.random.RandomState(200 + i)
        X = unit_rows(n, d, 300 + i)
        a = rounded_mean(X)
        W = rs.standard_normal((m, d)) / np.sqrt(d)
        scale = 1.0 / np.sqrt(np.geomspace(3.0, 1e-4, m))
        out[transform_name(n, d, m, "plain")] = dict(X=X, a=a, W=W.astype(np.float32), unit=False)
        out[transform_name(n, d, m, "unit")] = dict(X=X, a=a, W=W.astype(np.float32), unit=True)
        out[transform_name(n, d, m, "whitened")] = dict(X=X, a=a, W=(W * scale[:, None]).astype(np.float32), unit=True)
    return out


def zero_row_case():
    """A row equal to the shift: c = 0, so a zero row, counted in info[1] under unit."""
    X = unit_rows(45, 20, 55)
    a = rounded_mean(X)
    X[5] = a
    W = (np.random.RandomState(56).standard_normal((6, 20)) / np.sqrt(20)).astype(np.float32)
    return dict(X=X, a=a, W=W, unit=True)


def fit_case(n, d, m, held_out=70):
    """Rows with a planted spectrum: m directions of scale 3 to 1.5 over a floor of 0.3, a random rotation and a common offset.  Returns
    (X [n, d], held-out rows [held_out, d]) float32."""
    rs = np.random.RandomState(1000 + n + d + m)
    q, _ = np.linalg.qr(rs.standard_normal((d, d)))
    s = np.full(d, 0.3)
    s[:m] = np.linspace(3.0, 1.5, m)
    off = 2.0 * rs.standard_normal(d)
    z = (rs.standard_normal((n + held_out, d)) * s[None, :]) @ q.T + off[None, :]
    z = np.ascontiguousarray(z, dtype=np.float32)
    return z[:n], z[n:]


def fit_name(n, d, m):
    return "n%d_d%d_m%d" % (n, d, m)


def km_cache():
    """400 unit rows in 96 dimensions: five classes at the vertices of a regular simplex in a 4-dimensional subspace, a common offset and
    a little noise everywhere.  The classes are tight (their spread in the reduced space is below sqrt(reg_covar) of the mixture): a
    unit-normalised class is a tilted pancake that a DIAGONAL mixture fits better in two halves, and with a wider spread the BIC is flat
    beyond the planted K; at this spread reg_covar rounds every class to a ball, an extra component gains nothing and each one costs
    its 9 log(400) = 54.  Returns (X float32 [400, 96], labels int64 [400], 5)."""
    rs = np.random.RandomState(4242)
    k, d, n = 5, 96, 400
    e = np.eye(k) - 1.0 / k                                     # simplex vertices: 5 points that span 4 dimensions
    basis, _ = np.linalg.qr(rs.standard_normal((d, k)))
    centres = e @ basis.T                                       # [5, 96]
    z = np.arange(n) % k
    off = 3.0 * np.linalg.qr(rs.standard_normal((d, 1)))[0][:, 0]
    x = centres[z] + 0.001 * rs.standard_normal((n, d)) + off[None, :]
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x, dtype=np.float32), z.astype(np.int64), k


# ------------------------------------------------------------------------------------------------- the planted mistakes
# mistake -> (what it is, the case it must show on, the bound it must break)
MISTAKES = {
    "shift_not_subtracted": ("the shift is not subtracted", gram_name(33, 64, True), "gram"),
    "csum_from_x": ("csum taken from x instead of c", gram_name(33, 64, True), "colsum"),
    "mirror_untransposed": ("the mirrored tile written untransposed", gram_name(231, 768, True), "gram"),
    "diag_tile_twice": ("a diagonal tile added twice", gram_name(3 * T + 5, 129, True), "gram"),
    "ragged_block_dropped": ("the last ragged row block dropped", gram_name(T + 1, 96, True), "gram"),
    "chain_row_twice": ("a chain-boundary row counted twice", gram_name(3 * T + 5, 129, True), "gram"),
    "div_n": ("division by n instead of n - 1", fit_name(1500, 64, 8), "weyl"),
    "whiten_mul": ("whitening multiplied by sqrt(lambda)", fit_name(1500, 64, 8), "transform_whitened"),
    "ascending": ("components in ascending order", fit_name(1200, 33, 4), "davis_kahan"),
    "sign_flipped": ("a flipped sign", fit_name(2000, 96, 16), "transform"),
    "unit_over_padded": ("the unit norm taken over the padded columns of an unmasked accumulator", transform_name(40, 16, 32, "unit"),
                         "transform"),
    "no_correction": ("the correction csum csum^T / n omitted", fit_name(1200, 33, 4) + "-shift0", "weyl"),
    "last_range_dropped": ("the last range (ONE row) left out", gram_name(*NAMED_GRAM["ranges_x_tiles"], True), "gram"),
    "range_added_twice": ("the second range's partial counted twice", gram_name(*NAMED_GRAM["cap32"], True), "gram"),
    "range_stride_of_one_tile": ("a partial stride that forgets the tile count", gram_name(*NAMED_GRAM["ranges_x_tiles"], True), "gram"),
    "colsum_range_tail_dropped": ("the last rows % 8 rows of each column-sum range left out", gram_name(*NAMED_GRAM["colsum_cap"], False),
                                  "colsum"),
}
# the mistakes that must show on further cases as well: (mistake, case, kind)
ALSO = [("unit_over_padded", transform_name(*NAMED_TRANSFORM[name], "unit"), "transform") for name in ("nt2_phantom", "nt8_phantom")]


def mistake_cases():
    return [(m, case, kind) for m, (_, case, kind) in MISTAKES.items()] + ALSO
