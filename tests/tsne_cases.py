"""A numpy float64 restatement of scd_tsne_calibrate / scd_tsne_gradient / scd_tsne_update and of scd_amd.tsne (include/scd_hip.h,
docs/design/tsne.md), the named cases of the t-SNE tests and planted mistakes.

Every function takes `mistake`: one of MISTAKES plants the named error, so that a test can show its bound would catch it.  The cases
of more than 32 column chunks (LARGE) come with the host's range rule restated (ranges), a P built without n x n arrays (banded_p), the
float64 sums in torch (repulsion_f64_torch) and the mistakes of the chunk loop and the range sum (RANGE_MISTAKES, dropped_columns)."""
import os

import numpy as np

import finch_cases as fc
import knn_cases as kc

MISTAKES = ("log2", "div_n", "no_reverse", "exag_repulsive", "no_factor_4", "self_in_z", "padding_column", "z_half", "momentum_switch",
            "gains_inverted")
CALIBRATION_MISTAKES = ("log2", "div_n", "no_reverse")
GRADIENT_MISTAKES = ("exag_repulsive", "no_factor_4", "self_in_z", "padding_column", "z_half")
OPTIMISER_MISTAKES = ("momentum_switch", "gains_inverted")

SEARCH_STEPS = 200
KMAX = 64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne_blobs.npz")

# the kernel's error bound (docs/design/tsne.md, "The bound"): per pair 14 roundings of 2^-24 on a force term (6 on a q term), plus the
# fp32 run of 64 columns; the float64 folds, the range sums and the test's own -grad Z / 4 are below 2^-40 of the same magnitudes
C_BOUND = 80
# the mass of a row's dense conditional distribution at perplexity 30 that lies beyond its 64th / 91st neighbour on the committed blob
# case (mean, max), measured on the CPU in float64 by tools/gen_tsne_golden.py --tail: what k = 64 in place of scikit-learn's 91 leaves out
TAIL_BEYOND_64 = (0.0297, 0.0871)
TAIL_BEYOND_91 = (0.0083, 0.0400)
# the largest relative difference between joint_f64 and sklearn.manifold._t_sne._joint_probabilities_nn over the entries of the
# committed CPU cases (scikit-learn 1.7.2: float32 distances, 100 steps to an entropy tolerance of 1e-5), measured; the test asserts
# ten times this
SKLEARN_JOINT_REL = 1.01e-4                                      # s200_p5: 1.002e-4; s400_p10: 5.9e-5; s300_p21: 5.0e-5


# ---------------------------------------------------------------------------------------------------- neighbourhood
def neighbours(n, perplexity):
    return min(n - 1, KMAX, int(3.0 * perplexity))


def graph_f64(x, k):
    """(idx int64 [n, k], dist2 float64 [n, k]) of the unit rows of x: knn_cases.knn_f64's graph, d = max(0, 2 - 2 dot)."""
    u = fc.unit_rows(x)
    idx, dot = kc.knn_f64(u, u, k, 0)
    return idx, np.maximum(0.0, 2.0 - 2.0 * dot)


# ---------------------------------------------------------------------------------------------------- calibration
def entropy(d, beta):
    """H(b) of rows d [n, k] (already shifted by the row minimum) at beta [n], natural logarithms."""
    e = np.exp(-d * beta[:, None])
    s = e.sum(1)
    return np.log(s) + beta * (d * e).sum(1) / s


def calibrate_f64(dist2, perplexity, mistake=None, steps=SEARCH_STEPS):
    """(p [n, k], beta [n], unreached bool [n]): the fixed-step search of scd_tsne_calibrate, all rows at once."""
    dist2 = np.asarray(dist2, dtype=np.float64)
    n, k = dist2.shape
    d = dist2 - dist2.min(1, keepdims=True)
    target = np.log2(perplexity) if mistake == "log2" else np.log(perplexity)
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    for _ in range(steps):
        up = entropy(d, beta) - target > 0.0
        lo = np.where(up, beta, lo)
        hi = np.where(up, hi, beta)
        beta = np.where(up, np.where(hi == np.inf, beta * 2.0, (beta + hi) * 0.5), np.where(lo == -np.inf, beta * 0.5, (beta + lo) * 0.5))
    e = np.exp(-d * beta[:, None])
    return e / e.sum(1, keepdims=True), beta, (hi == np.inf) | (lo == -np.inf)


def joint_f64(idx, p, mistake=None):
    """CSR (indptr int64 [n + 1], indices int32, values float64) of P_ij = (p_j|i + p_i|j) / (2 n), columns ascending within a row."""
    n, k = idx.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    cols = idx.reshape(-1).astype(np.int64)
    fwd = rows * n + cols
    keys = np.concatenate([fwd, cols * n + rows])
    vals = np.concatenate([p.reshape(-1), p.reshape(-1)])
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    same_next = np.zeros(len(keys), dtype=bool)
    same_next[:-1] = keys[1:] == keys[:-1]
    first = np.ones(len(keys), dtype=bool)
    first[1:] = ~same_next[:-1]
    summed = vals + np.where(same_next, np.concatenate([vals[1:], [0.0]]), 0.0)
    keys, values = keys[first], summed[first] / (float(n) if mistake == "div_n" else 2.0 * n)
    if mistake == "no_reverse":                                 # only the pattern of the graph itself
        keep = np.isin(keys, fwd)
        keys, values = keys[keep], values[keep]
    r = keys // n
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(r, minlength=n))
    return indptr, (keys - r * n).astype(np.int32), values


def affinities_f64(x, perplexity, mistake=None):
    """scd_amd.tsne.joint_affinities restated: (indptr, indices, values, unreached rows)."""
    k = neighbours(x.shape[0], perplexity)
    idx, dist2 = graph_f64(x, k)
    p, _, unreached = calibrate_f64(dist2, perplexity, mistake)
    return joint_f64(idx, p, mistake) + (int(unreached.sum()),)


def csr_dense(P, n):
    indptr, indices, values = P[:3]
    out = np.zeros((n, n))
    out[np.repeat(np.arange(n), np.diff(indptr)), indices] = values
    return out


def dense_csr(M):
    n = M.shape[0]
    r, c = np.nonzero(M)
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(r, minlength=n))
    return indptr, c.astype(np.int32), M[r, c].astype(np.float64)


# ---------------------------------------------------------------------------------------------------- gradient
def repulsion_f64(Y, mistake=None, drop_column=None, rows_per_step=512, rows=None):
    """Per row i the float64 sums over j != i of (q^2 dx, q^2 dy, q) as F [n, 2], z [n], and the sums of the terms' magnitudes MF [n, 2]
    (Mz = z).  Y is taken as given (float32 values in float64 arithmetic).  rows (optional, int [m]): only these rows, outputs [m, ..]."""
    Y = np.asarray(Y).astype(np.float64)
    n = Y.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    m = len(rows)
    F, MF, z = np.zeros((m, 2)), np.zeros((m, 2)), np.zeros(m)
    cols = Y if mistake != "padding_column" else np.concatenate([Y, np.zeros((1, 2))])       # a padding column sits at (0, 0)
    for a in range(0, m, rows_per_step):
        b = min(m, a + rows_per_step)
        dx = Y[rows[a:b], None, 0] - cols[None, :, 0]
        dy = Y[rows[a:b], None, 1] - cols[None, :, 1]
        q = 1.0 / (1.0 + dx * dx + dy * dy)
        if mistake != "self_in_z":
            q[np.arange(b - a), rows[a:b]] = 0.0
        if drop_column is not None:
            q[:, drop_column] = 0.0
        t = q * q
        F[a:b, 0], F[a:b, 1] = (t * dx).sum(1), (t * dy).sum(1)
        MF[a:b, 0], MF[a:b, 1] = (t * np.abs(dx)).sum(1), (t * np.abs(dy)).sum(1)
        z[a:b] = q.sum(1)
    return F, z, MF


def repulsion_f64_torch(Y, device="cpu", rows_per_step=256):
    """repulsion_f64's sums (F, z, MF as numpy float64) in float64 torch operations over blocks of rows, on `device`: the float64 answer
    at sizes where numpy takes a minute per state.  Plain elementwise operations and row sums; nothing of scd_amd."""
    import torch
    y = torch.as_tensor(np.ascontiguousarray(Y)).to(device=device, dtype=torch.float64)
    n = y.shape[0]
    cx, cy = y[:, 0].contiguous()[None, :], y[:, 1].contiguous()[None, :]
    F, MF = torch.zeros((n, 2), dtype=torch.float64, device=device), torch.zeros((n, 2), dtype=torch.float64, device=device)
    z = torch.zeros(n, dtype=torch.float64, device=device)
    for a in range(0, n, rows_per_step):
        b = min(n, a + rows_per_step)
        dx, dy = y[a:b, 0:1] - cx, y[a:b, 1:2] - cy
        q = 1.0 / (1.0 + dx * dx + dy * dy)
        q[torch.arange(b - a, device=device), torch.arange(a, b, device=device)] = 0.0
        t = q * q
        F[a:b, 0], F[a:b, 1] = (t * dx).sum(1), (t * dy).sum(1)
        MF[a:b, 0], MF[a:b, 1] = (t * dx.abs()).sum(1), (t * dy.abs()).sum(1)
        z[a:b] = q.sum(1)
    return F.cpu().numpy(), z.cpu().numpy(), MF.cpu().numpy()


def column_terms(Y, col):
    """What one column at `col` (x, y) adds to every row's sums: (q^2 dx, q^2 dy, q), float64 [n] each."""
    Y = np.asarray(Y).astype(np.float64)
    dx, dy = Y[:, 0] - float(col[0]), Y[:, 1] - float(col[1])
    q = 1.0 / (1.0 + dx * dx + dy * dy)
    return q * q * dx, q * q * dy, q


def attraction_f64(Y, P):
    """(A [n, 2] = sum_j P_ij q_ij (y_i - y_j), sum P (log P - log q), sum P, MA [n, 2] = the sums of the terms' magnitudes) in float64 over
    the CSR entries."""
    Y = np.asarray(Y).astype(np.float64)
    indptr, indices, values = P[:3]
    n = Y.shape[0]
    rows = np.repeat(np.arange(n), np.diff(indptr))
    dx, dy = Y[rows, 0] - Y[indices, 0], Y[rows, 1] - Y[indices, 1]
    d2 = dx * dx + dy * dy
    w = values / (1.0 + d2)
    A, MA = np.zeros((n, 2)), np.zeros((n, 2))
    np.add.at(A[:, 0], rows, w * dx)
    np.add.at(A[:, 1], rows, w * dy)
    np.add.at(MA[:, 0], rows, np.abs(w * dx))
    np.add.at(MA[:, 1], rows, np.abs(w * dy))
    pos = values > 0
    return A, float((values[pos] * (np.log(values[pos]) + np.log1p(d2[pos]))).sum()), float(values.sum()), MA


def gradient_f64(Y, P, exaggeration=1.0, mistake=None):
    """(grad [n, 2], Z, KL) of scd_tsne_gradient in float64."""
    F, z, _ = repulsion_f64(Y, mistake)
    Z = float(z.sum())
    if mistake == "z_half":
        Z *= 0.5
    A, klp, psum, _ = attraction_f64(Y, P)
    rep = F / Z * (exaggeration if mistake == "exag_repulsive" else 1.0)
    grad = (1.0 if mistake == "no_factor_4" else 4.0) * (exaggeration * A - rep)
    return grad, Z, klp + np.log(Z) * psum


# ---------------------------------------------------------------------------------------------------- optimiser
def update_f64(grad, y, vel, gains, momentum, learning_rate, min_gain=0.01, mistake=None):
    """One _gradient_descent step; returns (y, vel, gains, gains * grad), new arrays."""
    inc = vel * grad < 0.0
    if mistake == "gains_inverted":
        inc = ~inc
    gains = np.where(inc, gains + 0.2, gains * 0.8)
    gains = np.maximum(gains, min_gain)
    gg = grad * gains
    vel = momentum * vel - learning_rate * gg
    return y + vel, vel, gains, gg


def descend_f64(P, y0, max_iter, early_exaggeration=12.0, learning_rate=None, switch_iter=250, mistake=None):
    """TSNE's two phases on the float64 restatement without the stopping checks: the force kernels see the float32 rounding of the
    master state, as on the device, and the second phase starts from zero velocity and unit gains, as scikit-learn's second
    _gradient_descent call does.  Returns the float64 master."""
    n = y0.shape[0]
    lr = max(n / early_exaggeration / 4.0, 50.0) if learning_rate is None else learning_rate
    momentum_switch = switch_iter + 20 if mistake == "momentum_switch" else switch_iter
    y = np.asarray(y0, dtype=np.float32).astype(np.float64)
    vel, gains = np.zeros_like(y), np.ones_like(y)
    for i in range(max_iter):
        if i == switch_iter:
            vel, gains = np.zeros_like(y), np.ones_like(y)
        grad, _, _ = gradient_f64(y.astype(np.float32), P, early_exaggeration if i < switch_iter else 1.0)
        y, vel, gains, _ = update_f64(grad, y, vel, gains, 0.5 if i < momentum_switch else 0.8, lr, mistake=mistake)
    return y


def pca_init_f64(x, scale=1e-4):
    """scd_amd.tsne.pca_init restated on the unit rows."""
    u = fc.unit_rows(x).astype(np.float64)
    xc = u - u.mean(0, keepdims=True)
    w, v = np.linalg.eigh(xc.T @ xc)
    axes = v[:, [-1, -2]].T.copy()
    for a in axes:
        if a[np.argmax(np.abs(a))] < 0:
            a *= -1
    y = xc @ axes.T
    return y / y[:, 0].std() * scale


def trustworthiness_f64(x, y, k=5):
    """sklearn.manifold.trustworthiness(x, y, n_neighbors=k) with Euclidean distances: 1 - 2 / (n k (2 n - 3 k - 1)) sum over i and the k
    nearest j of i in y of max(0, rank_x(i, j) - k), ranks from 1 without i itself."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.shape[0]

    def sq(a):
        g = (a * a).sum(1)
        d = g[:, None] + g[None, :] - 2.0 * a @ a.T
        np.fill_diagonal(d, -np.inf)                            # self sorts first in both spaces
        return d

    order_x = np.argsort(sq(x), axis=1, kind="stable")
    rank = np.empty((n, n), dtype=np.int64)
    rank[np.arange(n)[:, None], order_x] = np.arange(n)[None, :]                # rank 0 = self, 1 = nearest
    nn_y = np.argsort(sq(y), axis=1, kind="stable")[:, 1:k + 1]
    t = np.maximum(0, rank[np.arange(n)[:, None], nn_y] - k).sum()
    return 1.0 - t * 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))


# ---------------------------------------------------------------------------------------------------- cases
def blob_rows(n, d, classes, seed, noise=0.6):
    from oracle import synth
    x, y, _ = synth.clustered_features(n, d, classes, seed=seed, center_seed=seed + 100, noise=noise)
    return np.ascontiguousarray(x.astype(np.float32)), y


def golden():
    """The committed end-to-end case: rows float32 [1500, 32], labels, scikit-learn's five kl_divergence_ and trustworthiness values."""
    g = np.load(GOLDEN)
    return {key: g[key] for key in g.files}


# CPU cases for the comparisons with scipy and scikit-learn: name -> (n, d, classes, seed, perplexity)
SMALL = {"s400_p10": (400, 16, 6, 70, 10.0), "s300_p21": (300, 24, 4, 71, 21.0), "s200_p5": (200, 8, 3, 72, 5.0)}


def small_case(name):
    n, d, classes, seed, perplexity = SMALL[name]
    x, y = blob_rows(n, d, classes, seed)
    return x, y, perplexity


def calibration_case(k, n=300):
    """dist2 [n, k] for scd_tsne_calibrate, perplexity k / 3: blob rows and, in front, a row with duplicate distances (0), a row with all k
    distances equal (1: its entropy is log k at every b), a row with one neighbour at distance 0 (2), a row whose nearest distance occurs
    more often than the perplexity (3: unreachable too) and very tight clusters (4 .. 19: distances scaled by 1e-6, b > 1e4)."""
    x, _ = blob_rows(n, 16, 5, 73 + k)
    _, dist2 = graph_f64(x, k)
    dist2 = np.ascontiguousarray(dist2)
    dist2[0, 1:3] = dist2[0, 1]
    dist2[0, k - 2:] = dist2[0, k - 1]
    dist2[1, :] = 0.37
    dist2[2, 0] = 0.0
    dist2[3, :int(k / 3.0) + 1] = dist2[3, 0]
    dist2[4:20] *= 1e-6
    return dist2, k / 3.0


def hub_rows(n=1000, d=64, seed=74):
    """Rows scattered around the direction of row 0, which is then among the nearest neighbours of (nearly) every other row: its row of
    the joint matrix holds a long reverse list."""
    r = np.random.RandomState(seed)
    base = r.randn(d)
    x = base[None, :] + 0.5 * r.randn(n, d)
    x[0] = base
    return np.ascontiguousarray(x.astype(np.float32))


def sparse_p(n, seed, per_row=6):
    """A symmetric CSR P with positive entries summing to 1 for the gradient tests (no k-NN search needed): each row links to per_row
    pseudo-random others."""
    r = np.random.RandomState(seed)
    per_row = min(per_row, n - 1)
    M = np.zeros((n, n))
    for i in range(n):
        others = np.delete(np.arange(n), i)
        js = others if n - 1 <= per_row else r.choice(others, size=per_row, replace=False)
        M[i, js] = r.uniform(0.5, 1.5, size=len(js))
    M = M + M.T
    return dense_csr(M / M.sum())


# ---------------------------------------------------------------------------------------------------- ranges of several chunks
ROWS = CHUNK = 1024             # scd_tsne_row_tile(), scd_tsne_col_chunk()
RUN = 64                        # columns per fp32 run: a chunk stops after the run in which the columns end
YMAX = 32                       # the most column ranges


def cdiv(a, b):
    return -(-a // b)


def ranges(n, n_cu):
    """scd_tsne_gradient's split of the column chunks into ranges on a device of n_cu compute units, restated:
    (ny, chunks_per_y, chunks in the last range)."""
    chunks, tiles = cdiv(n, CHUNK), cdiv(n, ROWS)
    ny = max(1, min(cdiv(4 * n_cu, tiles), min(chunks, YMAX)))
    chunks_per_y = cdiv(chunks, ny)
    ny = cdiv(chunks, chunks_per_y)                             # no empty range
    return ny, chunks_per_y, chunks - (ny - 1) * chunks_per_y


# n of the cases whose ranges hold several chunks on every device (chunks > YMAX): 33 chunks, the last chunk and the last row tile with
# ONE valid row; 50 chunks, the same
LARGE = {"c33": 32769, "c50": 50177}
LARGE_STATES = {"c33": ("initial", "converged", "coincident", "pairs", "outlier"), "c50": ("converged", "coincident")}


def banded_p(n, hub_links=200, seed=0):
    """A symmetric CSR P with positive entries summing to 1, built without an n x n array: row i links to i +- 1, i +- 2, i +- 1024 and
    i +- 1025 (its own chunk and the next), and row 0 to hub_links more rows spread over all chunks, so its entries take the attract
    kernel's lane loop (64 entries a trip) round more than three times."""
    r = np.random.RandomState(seed)
    i = np.arange(n, dtype=np.int64)
    lo = [i[:n - o] for o in (1, 2, CHUNK, CHUNK + 1) if o < n]
    hi = [i[o:] for o in (1, 2, CHUNK, CHUNK + 1) if o < n]
    spread = 3 + (np.arange(hub_links, dtype=np.int64) * (n - 4)) // max(hub_links - 1, 1)  # from column 3 to column n - 1, ascending
    lo.append(np.zeros(len(spread), dtype=np.int64))
    hi.append(spread)
    keys = np.unique(np.concatenate(lo) * n + np.concatenate(hi))                           # the pairs i < j, each once
    w = r.uniform(0.5, 1.5, size=len(keys))
    a, b = keys // n, keys - (keys // n) * n
    rows, cols, vals = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([w, w])
    order = np.argsort(rows * n + cols, kind="stable")
    rows, cols, vals = rows[order], cols[order], vals[order]
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return indptr, cols.astype(np.int32), vals / vals.sum()


RANGE_MISTAKES = ("first_chunk_only", "last_range_dropped", "stale_range", "own_chunk_unchecked")


def dropped_columns(n, n_cu, row, mistake):
    """What a tsne_repulse_kernel / tsne_finish_kernel pair with one of RANGE_MISTAKES gets wrong in the sums of `row` on a device of n_cu
    compute units: (lost, extra), int64 arrays of column indices.  `lost` columns' terms are missing.  `extra` columns' terms are counted
    once more than they should be: a column j != row a second time, j == row the self pair (q = 1, no force), j >= n a padding column,
    which sits at the origin.

    first_chunk_only     a block stops after the first chunk of its range (the chunk loop never makes its second trip)
    last_range_dropped   the sum over the ranges stops one short
    stale_range          the sum runs over the range count from BEFORE the 'no empty range' step: partial sums that no block wrote.  What
                         they hold is arbitrary; the model is a second copy of range 0's sums.  Nothing when the step changes nothing.
    own_chunk_unchecked  a block decides `check` and the index it excludes once, at the first chunk of its range.  First chunk foreign
                         and full: the later chunks run unchecked, so the own chunk counts the self pair and the last chunk its padding
                         columns up to the end of the run of 64.  First chunk the tile's own: in every later chunk the column at the row's
                         offset is excluded in place of the row, and the padding columns pass `col < n`."""
    ny, cpy, _ = ranges(n, n_cu)
    chunks, tile, off = cdiv(n, CHUNK), row // ROWS, row % ROWS
    stop = lambda ch: min((ch + 1) * CHUNK, cdiv(n, RUN) * RUN)                              # where the chunk's column loop ends
    real = lambda cols: cols[(cols < n) & (cols != row)]
    span = lambda a, b: np.arange(a * CHUNK, min(b, chunks) * CHUNK, dtype=np.int64)
    none = np.zeros(0, dtype=np.int64)
    if mistake == "first_chunk_only":
        return real(np.concatenate([span(y * cpy + 1, (y + 1) * cpy) for y in range(ny)])), none
    if mistake == "last_range_dropped":
        return real(span((ny - 1) * cpy, chunks)), none
    if mistake == "stale_range":
        before = max(1, min(cdiv(4 * n_cu, cdiv(n, ROWS)), min(chunks, YMAX)))
        return none, (real(span(0, cpy)) if before > ny else none)
    if mistake == "own_chunk_unchecked":
        lost, extra = [], []
        for y in range(ny):
            first, last = y * cpy, min((y + 1) * cpy, chunks)
            if first == tile:
                for ch in range(first + 1, last):
                    j = ch * CHUNK + off
                    if j < n:
                        lost.append(j)
                    pad = np.arange(max(n, ch * CHUNK), stop(ch), dtype=np.int64)
                    extra.extend(pad[pad != j].tolist())
            elif (first + 1) * CHUNK <= n:                      # foreign and full: unchecked from here on
                for ch in range(first + 1, last):
                    if ch == tile:
                        extra.append(row)
                    extra.extend(range(max(n, ch * CHUNK), stop(ch)))
        return np.array(lost, dtype=np.int64), np.array(extra, dtype=np.int64)
    raise KeyError(mistake)


def range_mistake_shift(Y, rows, n_cu, mistake, padding=True):
    """(dF [m, 2], dz [m]): by how much `mistake` moves the float64 sums of `rows` (dropped_columns' terms, extra minus lost);
    padding=False leaves the padding columns out, whose terms are no whole numbers when all rows coincide."""
    Y = np.asarray(Y).astype(np.float64)
    n = Y.shape[0]
    cols = np.concatenate([Y, np.zeros((cdiv(n, RUN) * RUN - n, 2))])                       # the padding columns sit at (0, 0)
    dF, dz = np.zeros((len(rows), 2)), np.zeros(len(rows))
    for m, i in enumerate(rows):
        for sign, js in zip((-1.0, 1.0), dropped_columns(n, n_cu, int(i), mistake)):
            js = js if padding else js[js < n]
            dx, dy = Y[i, 0] - cols[js, 0], Y[i, 1] - cols[js, 1]
            q = 1.0 / (1.0 + dx * dx + dy * dy)
            dF[m] += sign * np.array([(q * q * dx).sum(), (q * q * dy).sum()])
            dz[m] += sign * q.sum()
    return dF, dz


def range_rows(n, seed=81, seeded=57):
    """The rows of the sensitivity test: the first and last rows of the first tiles, the last full tile's last row, the lone row of the
    last tile, and `seeded` others."""
    fixed = [0, ROWS - 1, ROWS, 2 * ROWS - 1, 2 * ROWS, n - 2, n - 1]
    others = np.setdiff1d(np.arange(n), fixed)
    return np.array(fixed + sorted(np.random.RandomState(seed).choice(others, size=seeded, replace=False).tolist()), dtype=np.int64)


STATES = ("initial", "converged", "coincident", "pairs", "outlier")


def state(name, n, seed=80):
    """Y float32 [n, 2] of the issue's inputs."""
    r = np.random.RandomState(seed + n)
    if name == "initial":
        y = 1e-4 * r.randn(n, 2)
    elif name == "converged":
        centres = r.uniform(-80, 80, size=(10, 2))
        y = np.clip(centres[r.randint(0, 10, size=n)] + 4.0 * r.randn(n, 2), -100, 100)
    elif name == "coincident":
        y = np.tile(np.array([[3.25, -1.5]]), (n, 1))
    elif name == "pairs":
        y = 20.0 * r.randn(n, 2)
        y[1::2] = y[0:n - 1:2][:len(y[1::2])]                   # rows 2 m and 2 m + 1 coincide
    elif name == "outlier":
        y = 5.0 * r.randn(n, 2)
        y[n // 2] = (1e6, -1e6)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(y.astype(np.float32))
