"""Spectral clustering on the exact k-NN graph: scikit-learn 1.7's SpectralClustering(affinity='nearest_neighbors',
assign_labels='kmeans') on the HIP primitives of scd_amd/csrc/knn.hip and scd_amd/csrc/graph.hip.  docs/design/spectral.md has the
semantics, the summation order, the solver and what differs from scikit-learn.

The n x n x d neighbour search (ops.knn), the normalised affinity in CSR form (ops.knn_affinity) and the float64 sparse-times-block
product (ops.spmm_f64) are HIP.  The eigensolver on top of the product is Chebyshev-filtered subspace iteration (Zhou & Saad, "A
Chebyshev-Davidson algorithm for large symmetric eigenproblems", SIAM J. Matrix Anal. Appl. 2007; Zhou, Saad, Tiago & Chelikowsky, J. Comput.
Phys. 2006) in float64 over torch tensors and an operator callback, so that the same code runs over ops.spmm_f64 on the device and over a
scipy or torch.sparse operator on the CPU.  Its tall products (X^T Y, X Q) are torch matmuls; its m x m problems (eigh, Cholesky) go to
the host in numpy, as the t-SNE calibration's and Munkres' small problems do.
"""
import numpy as np
import torch

from . import ops

MAX_NEIGHBORS = 65              # scikit-learn's n_neighbors counts the row itself: scd_knn's k = n_neighbors - 1 <= 64
MAX_COMPONENTS = 1024           # the k-means E-step's width: the embedding is its input


class NotConverged(RuntimeError):
    """eigsolve ran max_outer iterations without reaching tol; .info is the dict a converged solve returns."""

    def __init__(self, msg, info):
        super().__init__(msg)
        self.info = info


def block_width(n_components, pad=None):
    """m = n_components + pad rounded up to a multiple of 8 (scd_spmm_f64's column rule); the default pad is max(8, n_components // 4)."""
    pad = max(8, n_components // 4) if pad is None else int(pad)
    return (n_components + pad + 7) // 8 * 8


def _small_eigh(h):
    """The m x m Rayleigh-Ritz problem on the host: eigenvalues descending and their vectors, numpy float64."""
    w, q = np.linalg.eigh(0.5 * (h + h.T))
    return w[::-1].copy(), np.ascontiguousarray(q[:, ::-1])


def _small_factor(g):
    """T with T^T G T = I for an m x m Gram matrix G, on the host: the inverse of G's Cholesky factor, or, for a G that is not positive
    definite to working precision, the eigenvalue form Q L^-1/2."""
    g = 0.5 * (g + g.T)
    try:
        return np.ascontiguousarray(np.linalg.inv(np.linalg.cholesky(g).T))         # g = r^T r, t = r^-1
    except np.linalg.LinAlgError:
        w, q = np.linalg.eigh(g)
        return np.ascontiguousarray(q / np.sqrt(np.maximum(w, w[-1] * 1e-28 + 1e-300)))


def _orthonormalise(x):
    """Columns of x -> an orthonormal basis of their span: columns scaled to unit length, then Cholesky QR twice."""
    x = x / torch.linalg.vector_norm(x, dim=0, keepdim=True).clamp_min(1e-300)
    for _ in range(2):
        x = x @ torch.as_tensor(_small_factor((x.T @ x).cpu().numpy()), device=x.device)
    return x


def _start_block(n, m, seed, device):
    """The seeded random start, made orthonormal.  Drawn by the device's own generator (16 M normal deviates at n = 126,976, m = 128 took
    the host 0.26 s, longer than the rest of the solve): the same seed gives the same block on the same kind of device."""
    gen = torch.Generator(device=device).manual_seed(int(seed))
    return _orthonormalise(torch.randn(n, m, generator=gen, dtype=torch.float64, device=device))


def eigsolve(apply, n, n_components, tol=1e-6, degree=12, pad=None, max_outer=500, random_state=0, device="cpu"):
    """The n_components largest eigenvalues of a symmetric operator S whose spectrum lies in [-1, 1], by Chebyshev-filtered subspace
    iteration in float64.

    apply(X, alpha, beta, gamma, Z) -> alpha (S X) + beta X + gamma Z for float64 blocks [n, m] on `device` (Z None: no third term); the
    result must be a new tensor.  Per outer iteration: Rayleigh-Ritz on the block (H = X^T (S X), eigh on the host, rotation), the
    residual 2-norms of the leading n_components Ritz pairs (stop when the largest is <= tol), a degree-`degree` Chebyshev filter that
    damps [-1, the block's smallest Ritz value], and re-orthonormalisation.

    Returns (eigenvalues float64 [n_components] descending, vectors float64 [n, n_components] orthonormal, info) with info = dict(outer,
    products, residual, converged, m).  Not converged after max_outer iterations raises NotConverged (a RuntimeError) carrying info.
    Inside a multiple eigenvalue the basis is arbitrary."""
    n, k = int(n), int(n_components)
    m = block_width(k, pad)
    if k < 1:
        raise ValueError("eigsolve: n_components = %d must be at least 1" % k)
    if m > n:
        raise ValueError("eigsolve: the block width m = %d (n_components + pad, rounded up to 8) exceeds n = %d: m <= n" % (m, n))
    if degree < 2:
        raise ValueError("eigsolve: degree = %d must be at least 2" % degree)
    x = _start_block(n, m, random_state, device)
    info = dict(outer=0, products=0, residual=float("inf"), converged=False, m=m)
    while info["outer"] < max_outer:
        info["outer"] += 1
        y = apply(x, 1.0, 0.0, 0.0, None)
        info["products"] += 1
        w, q = _small_eigh((x.T @ y).cpu().numpy())
        q = torch.as_tensor(q, device=x.device)
        x, y = x @ q, y @ q                                     # Ritz vectors and their images
        wk = torch.as_tensor(w[:k], device=x.device)
        info["residual"] = float(torch.linalg.vector_norm(y[:, :k] - x[:, :k] * wk, dim=0).max().item())
        if info["residual"] <= tol:
            info["converged"] = True
            return wk, x[:, :k].contiguous(), info
        # T_0 = X, T_1 = (S X - c X) / e, T_{j+1} = (2 / e) (S T_j - c T_j) - T_{j-1}: the filter's interval [-1, a] mapped to [-1, 1]
        a = min(max(float(w[-1]), -1.0 + 1e-3), 1.0 - 1e-6)
        e, c = 0.5 * (a + 1.0), 0.5 * (a - 1.0)
        t0, t1 = x, (y - c * x) / e
        for _ in range(degree - 1):
            t0, t1 = t1, apply(t1, 2.0 / e, -2.0 * c / e, -1.0, t0)
            info["products"] += 1
        x = _orthonormalise(t1)
    raise NotConverged("eigsolve: the largest residual norm is %.3g > tol = %.3g after max_outer = %d iterations (%d sparse products)"
                       % (info["residual"], tol, max_outer, info["products"]), info)


def _check_limits(n, n_neighbors, n_components=None, pad=None):
    if not 2 <= n_neighbors <= MAX_NEIGHBORS:
        raise ValueError("n_neighbors = %d outside the limit 2 <= n_neighbors <= %d" % (n_neighbors, MAX_NEIGHBORS))
    if not n > n_neighbors:
        raise ValueError("n = %d rows do not satisfy the limit n > n_neighbors = %d" % (n, n_neighbors))
    if n_components is not None:
        if not 1 <= n_components <= min(n - 1, MAX_COMPONENTS):
            raise ValueError("n_components = %d outside the limit n_components <= min(n - 1, %d) = %d"
                             % (n_components, MAX_COMPONENTS, min(n - 1, MAX_COMPONENTS)))
        if block_width(n_components, pad) > n:
            raise ValueError("the block width m = %d exceeds n = %d: the limit is m <= n" % (block_width(n_components, pad), n))


def knn_affinity(x, n_neighbors=10):
    """x: device fp16 / fp32 tensor or numpy [n, d].  The unit rows' exact k-NN lists (k = n_neighbors - 1: scikit-learn's
    kneighbors_graph(include_self=True) counts the row itself) -> (rowptr int64 [n + 1], col int32 [nnz], val float64 [nnz],
    inv_sqrt_deg float64 [n], info) on the device: S = D^-1/2 A D^-1/2 with A = 0.5 (C + C^T), diagonal removed, in CSR form with
    ascending columns.  info: dict(nnz, median_row, max_row, knn = ops.knn's info as a list)."""
    from .knn import _as_device_f32, unit_rows
    x = _as_device_f32(x)
    _check_limits(x.shape[0], int(n_neighbors))
    u = unit_rows(x)
    idx, _, kinfo = ops.knn(u, u, int(n_neighbors) - 1, self_base=0)
    rowptr, col, val, isd, nnz = ops.knn_affinity(idx)
    lens = rowptr[1:] - rowptr[:-1]
    info = dict(nnz=nnz, median_row=int(lens.median().item()), max_row=int(lens.max().item()), knn=kinfo.cpu().tolist())
    return rowptr, col, val, isd, info


def device_operator(rowptr, col, val):
    """The callback eigsolve wants, over ops.spmm_f64."""
    def apply(x, alpha, beta, gamma, z):
        return ops.spmm_f64(rowptr, col, val, x, alpha, beta, gamma, z)
    return apply


def embed(vectors, inv_sqrt_deg):
    """Eigenvectors of S -> scikit-learn's embedding: V / sqrt(d) row-wise (as V * (1 / sqrt(d))), then every column's sign flipped so
    that its entry of largest magnitude is positive (sklearn.utils.extmath._deterministic_vector_sign_flip, after the scaling)."""
    e = vectors * inv_sqrt_deg[:, None]
    big = e.abs().argmax(dim=0)
    sign = torch.sign(e[big, torch.arange(e.shape[1], device=e.device)])
    return e * torch.where(sign == 0, torch.ones_like(sign), sign)


def spectral_embedding(x, n_components, n_neighbors=10, tol=1e-6, degree=12, pad=None, max_outer=500, random_state=0, return_all=False):
    """sklearn.manifold.spectral_embedding(kneighbors affinity of x, n_components, drop_first=False) on the device: float64
    [n, n_components], column j belonging to the j-th largest eigenvalue of S.  return_all: (embedding, eigenvalues, affinity, info)
    with affinity = (rowptr, col, val, inv_sqrt_deg) and info = eigsolve's merged with knn_affinity's."""
    n = x.shape[0]
    _check_limits(n, int(n_neighbors), int(n_components), pad)
    rowptr, col, val, isd, ginfo = knn_affinity(x, n_neighbors)
    w, v, info = eigsolve(device_operator(rowptr, col, val), n, int(n_components), tol=tol, degree=degree, pad=pad, max_outer=max_outer,
                          random_state=random_state, device=rowptr.device)
    info.update(ginfo)
    emb = embed(v, isd)
    return (emb, w, (rowptr, col, val, isd), info) if return_all else emb


class SpectralClustering:
    """SpectralClustering(n_clusters, n_neighbors=10, n_init=10, random_state=None, tol=1e-6).fit(x): scikit-learn's
    SpectralClustering(affinity='nearest_neighbors', assign_labels='kmeans') with n_components = n_clusters.

    After fit: labels_ (numpy int [n]), embedding_ (device float32 [n, n_clusters]: what k-means saw), eigenvalues_ (numpy float64,
    descending, of S = I - the normalised Laplacian), affinity_ = (rowptr, col, val, inv_sqrt_deg) on the device and info_."""

    def __init__(self, n_clusters=8, n_neighbors=10, n_init=10, random_state=None, tol=1e-6):
        self.n_clusters, self.n_neighbors, self.n_init, self.random_state, self.tol = int(n_clusters), int(n_neighbors), n_init, random_state, tol

    def fit(self, x, y=None):
        from .cluster import KMeans
        seed = 0 if self.random_state is None else int(self.random_state)
        emb, w, aff, info = spectral_embedding(x, self.n_clusters, self.n_neighbors, tol=self.tol, random_state=seed, return_all=True)
        self.embedding_ = emb.to(torch.float32).contiguous()
        self.eigenvalues_ = w.cpu().numpy()
        self.affinity_, self.info_ = aff, info
        km = KMeans(n_clusters=self.n_clusters, n_init=self.n_init, random_state=self.random_state).fit(self.embedding_)
        self.labels_ = np.asarray(km.labels_)
        return self

    def fit_predict(self, x, y=None):
        return self.fit(x).labels_
