"""The float64 restatement of spectral clustering on the k-NN graph (docs/design/spectral.md) and the cases of its tests: the affinity
from exact float64 k-NN lists (knn_cases.knn_f64), S = D^-1/2 A D^-1/2, scd_spmm_f64's chunked summation order in numpy, and the
embedding from a dense numpy.linalg.eigh; affinity_sparse restates the affinity without n x n arrays for the cases of more than one
tile of graph_scan_kernel (SCAN).  Nothing here uses a device or scd_amd."""
import numpy as np

import knn_cases as kc

CHUNK = 512                     # scd_spmm_f64: entries of a row summed before a partial sum is formed


# ---------------------------------------------------------------------------------------------------- the rules
def knn_lists(x, n_neighbors):
    """scikit-learn's kneighbors_graph(x, n_neighbors, include_self=True) without the row itself: int32 [n, n_neighbors - 1]."""
    idx, _ = kc.knn_f64(x, x, n_neighbors - 1, 0)
    return idx.astype(np.int32)


def affinity(idx, n=None):
    """idx int [n, k] -> dict(rowptr int64 [n + 1], col int32 [nnz], val float64 [nnz], inv_sqrt_deg float64 [n], nnz, deg, A dense):
    A = 0.5 (C + C^T) without its diagonal; negative entries and idx[i][j] == i are ignored, a repeated neighbour counts once."""
    idx = np.asarray(idx)
    n = idx.shape[0] if n is None else n
    c = np.zeros((n, n))
    for i in range(n):
        for t in idx[i]:
            if t >= 0 and t != i:
                if t >= n:
                    raise ValueError("index >= n")
                c[i, t] = 1.0
    a = 0.5 * (c + c.T)
    deg = a.sum(1)                                              # multiples of 0.5 below 2^52: exact in any order
    root = np.where(deg > 0, np.sqrt(deg), 1.0)
    rows, cols = np.nonzero(a)                                  # row-major: columns ascend inside a row
    val = a[rows, cols] / (root[rows] * root[cols])
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return dict(rowptr=rowptr, col=cols.astype(np.int32), val=val, inv_sqrt_deg=1.0 / root, nnz=len(cols), deg=deg, A=a)


def affinity_sparse(idx, n=None):
    """affinity() without the n x n arrays, for lists of many rows: the same dict without `A`, every field with the same bits."""
    idx = np.asarray(idx).astype(np.int64)
    n = idx.shape[0] if n is None else n
    rows = np.repeat(np.arange(idx.shape[0], dtype=np.int64), idx.shape[1])
    t = idx.reshape(-1)
    keep = (t >= 0) & (t != rows)
    if (t[keep] >= n).any():
        raise ValueError("index >= n")
    fwd = np.unique(rows[keep] * n + t[keep])                   # the entries of C: a repeated neighbour counts once
    back = (fwd % n) * n + fwd // n
    keys = np.union1d(fwd, back)                                # row-major: columns ascend inside a row
    r, c = keys // n, keys % n
    a = np.where(np.isin(keys, fwd) & np.isin(c * n + r, fwd), 1.0, 0.5)
    deg = np.bincount(r, weights=a, minlength=n)                # multiples of 0.5 below 2^52: exact in any order
    root = np.where(deg > 0, np.sqrt(deg), 1.0)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rowptr[1:])
    return dict(rowptr=rowptr, col=c.astype(np.int32), val=a / (root[r] * root[c]), inv_sqrt_deg=1.0 / root, nnz=len(keys), deg=deg)


SCAN_TILE = 4096                # graph_scan_kernel: rows per tile of the prefix sum, GRAPH_SCAN_THREADS * GRAPH_SCAN_PER


def carry_zero(rowptr):
    """The planted mistake of the scan: every tile of SCAN_TILE rows starts from 0 instead of the rows before it."""
    i = np.arange(len(rowptr))
    return rowptr - rowptr[(i // SCAN_TILE) * SCAN_TILE]


def dense_s(aff):
    n = len(aff["rowptr"]) - 1
    s = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(aff["rowptr"]))
    s[rows, aff["col"]] = aff["val"]
    return s


def spmm(aff, x, alpha=1.0, beta=0.0, gamma=0.0, z=None):
    """alpha (S x) + beta x + gamma z in scd_spmm_f64's order: per row and chunk of 512 entries a sum from 0, left to right, a multiply
    and an add per term; a row of several chunks adds the chunk sums from 0 in chunk order; then (alpha sum + beta x) + gamma z."""
    rowptr, col, val = aff["rowptr"], aff["col"], aff["val"]
    n = len(rowptr) - 1
    lens = np.diff(rowptr)
    total = np.zeros((n, x.shape[1]))
    for c in range(max(1, -(-int(lens.max()) // CHUNK))):
        part = np.zeros_like(total)
        for p in range(CHUNK):
            pos = c * CHUNK + p
            live = np.nonzero(lens > pos)[0]
            if not len(live):
                break
            e = rowptr[live] + pos
            part[live] = part[live] + val[e][:, None] * x[col[e]]
        live = lens > c * CHUNK
        if c == 0:
            total = part                                        # one chunk: its sum.  (0 + a sum from +0 has the same bits.)
        else:
            total[live] = total[live] + part[live]
    y = alpha * total + beta * x
    return y if z is None else y + gamma * z


def dense_eigs(aff):
    """All eigenvalues of S descending, and the eigenvectors in that order."""
    w, v = np.linalg.eigh(dense_s(aff))
    return w[::-1].copy(), v[:, ::-1].copy()


def embed(v, inv_sqrt_deg):
    """Eigenvectors -> scikit-learn's embedding: V / sqrt(d) row-wise, then _deterministic_vector_sign_flip per column."""
    e = v * inv_sqrt_deg[:, None]
    big = np.abs(e).argmax(0)
    sign = np.sign(e[big, np.arange(e.shape[1])])
    return e * np.where(sign == 0, 1.0, sign)


def dense_embedding(aff, k):
    w, v = dense_eigs(aff)
    return embed(v[:, :k], aff["inv_sqrt_deg"]), w


def sin_largest_angle(u, v):
    """Sine of the largest principal angle between span(u) and span(v) (equal dimensions), by orthonormal bases."""
    qu, qv = np.linalg.qr(u)[0], np.linalg.qr(v)[0]
    return float(np.linalg.norm(qu - qv @ (qv.T @ qu), 2))


def components(aff):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(aff["rowptr"]) - 1
    return connected_components(csr_matrix((aff["val"], aff["col"], aff["rowptr"]), shape=(n, n)), directed=False)[0]


def same_partition(a, b):
    """Equal up to a relabelling."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    pairs = len(np.unique(a * (b.max() + 1) + b))
    return pairs == len(np.unique(a)) == len(np.unique(b))


def kmeans_partition(emb, k, seed):
    from sklearn.cluster import KMeans
    return KMeans(n_clusters=k, n_init=10, random_state=seed).fit(np.asarray(emb, dtype=np.float32)).labels_


# ---------------------------------------------------------------------------------------------------- the cases
def _unit32(x):
    x = np.asarray(x, dtype=np.float64)
    return (x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float32)


def blobs():
    """600 rows around six unit-norm centres in 16 dimensions, noise 1 / sqrt(d) per coordinate, rows normalised; n_neighbors 10."""
    rs = np.random.RandomState(0)
    n, d, k = 600, 16, 6
    cent = rs.randn(k, d)
    cent /= np.sqrt((cent * cent).sum(1, keepdims=True))
    truth = np.arange(n) % k
    x = _unit32(cent[truth] + rs.randn(n, d) / np.sqrt(d))
    return dict(x=x, truth=truth, n_clusters=k, n_neighbors=10)


def rings():
    """900 rows on three concentric circles of radius 1, 2, 3 in a random 2-plane of 16 dimensions, noise 0.05, a constant 17th
    coordinate of 6 appended, rows normalised; n_neighbors 8: three connected components."""
    rs = np.random.RandomState(1)
    n, d = 900, 16
    plane = np.linalg.qr(rs.randn(d, 2))[0]
    truth = np.arange(n) % 3
    ang = rs.uniform(0, 2 * np.pi, n)
    flat = (truth + 1.0)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    x = flat @ plane.T + 0.05 * rs.randn(n, d)
    x = _unit32(np.concatenate([x, np.full((n, 1), 6.0)], 1))
    return dict(x=x, truth=truth, n_clusters=3, n_neighbors=8)


def hub():
    """Hand-written lists, n = 1500, k = 3: row 0 is in every list, so row 0 of S has 1,499 entries - three chunks."""
    n = 1500
    i = np.arange(n)
    idx = np.stack([np.zeros(n, dtype=np.int64), (i + 1) % n, (i + 7) % n], 1)
    idx[0] = [1, 2, 3]
    return idx.astype(np.int32)


def hub_wide():
    """As hub with n = 2600, k = 2: row 0 has 2,599 entries, six chunks - more than the four waves of a block take in one round."""
    n = 2600
    idx = np.stack([np.zeros(n, dtype=np.int64), (np.arange(n) + 1) % n], 1)
    idx[0] = [1, 2]
    return idx.astype(np.int32)


def tiny():
    """n = 5, k = 4: the complete graph."""
    return np.array([[j for j in range(5) if j != i] for i in range(5)], dtype=np.int32)


def ragged():
    """n = 1003, k = 7: random lists with -1 entries, a self index and a repeated neighbour."""
    rs = np.random.RandomState(2)
    n, k = 1003, 7
    idx = rs.randint(0, n, size=(n, k))
    idx[rs.rand(n, k) < 0.15] = -1
    idx[::5, 2] = np.arange(n)[::5]                             # the row itself
    idx[1::7, 4] = idx[1::7, 1]                                 # a neighbour (or a -1) twice
    idx[3::11, 0] = idx[3::11, 6]
    return idx.astype(np.int32)


def scan_lists(n, k, seed):
    """Lists for more than one tile of the row-length scan, in ragged()'s style (-1 entries, a self index, a repeated neighbour), with a
    hub at the first row of the second tile - row 4,096 is in the list of every 4th row, so its own row is longer than one wave ranks
    alone (1,024) and than two chunks of the product - and, just before it, row 4,095 with an empty list that nobody points to."""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, n, size=(n, k))
    idx[rs.rand(n, k) < 0.15] = -1
    idx[::5, 2] = np.arange(n)[::5]                             # the row itself
    idx[1::7, 1] = idx[1::7, 0]                                 # a neighbour (or a -1) twice
    idx[::4, 0] = SCAN_TILE
    idx[idx == SCAN_TILE - 1] = -1
    idx[SCAN_TILE - 1] = -1
    return idx.astype(np.int32)


SCAN = {"scan_4097": (4097, 3, 3), "scan_8200": (8200, 5, 4)}   # name -> (n, k, seed): a second tile of ONE row; three tiles


def scan_cases():
    """name -> idx int32 [n, k]: too many rows for affinity()'s dense arrays; affinity_sparse is their restatement."""
    return {name: scan_lists(*args) for name, args in SCAN.items()}


def list_cases():
    """name -> idx int32 [n, k] for the affinity tests: the two data cases' exact lists and the hand-written ones."""
    b, r = blobs(), rings()
    return dict(blobs=knn_lists(b["x"], b["n_neighbors"]), rings=knn_lists(r["x"], r["n_neighbors"]), hub=hub(), tiny=tiny(), ragged=ragged(),
                hub_wide=hub_wide())


def spread_block(seed, n, m):
    """float64 [n, m] with magnitudes spread over 2^-20 .. 2^20 and both signs."""
    rs = np.random.RandomState(seed)
    return rs.randn(n, m) * np.exp2(rs.uniform(-20, 20, size=(n, m)))
