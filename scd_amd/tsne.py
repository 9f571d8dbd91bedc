"""Exact t-SNE on the HIP primitives of scd_amd/csrc/tsne.hip: scikit-learn 1.7's TSNE(n_components=2) as the reference's save_tsne
calls it (local_utils/util.py:178-216), with the exact all-pairs gradient in place of Barnes-Hut's.  docs/design/tsne.md has the
definitions.

The k-NN graph (ops.knn), the perplexity calibration (ops.tsne_calibrate), the gradient (ops.tsne_gradient) and the update step
(ops.tsne_update) are HIP; torch does the index plumbing of the graph's transpose (an integer sort) and the two principal components
of the initial state.  No floating-point scatter-add anywhere: two runs return the same bits.
"""
import numpy as np
import torch

from . import knn, ops

KMAX = 64
N_ITER_CHECK, EXPLORATION_ITER = 50, 250                        # sklearn's _N_ITER_CHECK and _EXPLORATION_MAX_ITER
MOMENTUM = (0.5, 0.8)
MIN_GAIN = 0.01


def neighbours(n, perplexity):
    """k = min(n - 1, 64, floor(3 * perplexity)): scikit-learn's neighbourhood up to perplexity 21, capped by scd_knn's 64 above."""
    return min(n - 1, KMAX, int(3.0 * perplexity))


def _check_perplexity(n, perplexity):
    k = neighbours(n, perplexity)
    if not (1.0 < perplexity < k):
        raise ValueError("the perplexity must lie in (1, k) with k = min(n - 1, 64, floor(3 * perplexity)) = %d, not %r" % (k, perplexity))
    return k


def joint_affinities(x, perplexity):
    """The symmetric joint affinities of the rows of x (made unit by knn.unit_rows) as a CSR matrix on the device:
    (indptr int64 [n + 1], indices int32 [nnz] ascending within a row, values float64 [nnz], info).  P_ij = (p_j|i + p_i|j) / (2 n) over
    the k-NN graph, a missing direction counting 0.  info: dict(k, untied = rows whose entropy cannot reach the target, bad_rows, knn =
    ops.knn's info)."""
    x = knn._as_device_f32(x)
    n = x.shape[0]
    k = _check_perplexity(n, perplexity)
    idx, sim, knn_info = knn.knn_graph(x, k)
    dist2 = torch.clamp(2.0 - 2.0 * sim, min=0.0)
    p, _, info = ops.tsne_calibrate(dist2, perplexity)
    rows = torch.arange(n, device=x.device, dtype=torch.int64).repeat_interleave(k)
    cols = idx.reshape(-1)
    keys = torch.cat([rows * n + cols, cols * n + rows])        # (i, j) carries p_j|i once as given and once transposed
    vals = torch.cat([p.reshape(-1), p.reshape(-1)])
    keys, order = torch.sort(keys, stable=True)
    vals = vals[order]
    same_next = torch.zeros(keys.numel(), dtype=torch.bool, device=x.device)
    same_next[:-1] = keys[1:] == keys[:-1]                      # a key occurs at most twice: the graph has no repeated edge
    first = torch.ones_like(same_next)
    first[1:] = ~same_next[:-1]
    nxt = torch.cat([vals[1:], vals.new_zeros(1)])
    summed = vals + torch.where(same_next, nxt, torch.zeros_like(nxt))          # a + b is commutative: the sort's tie order is immaterial
    keys, values = keys[first], summed[first] / (2.0 * n)
    r = keys // n
    indices = (keys - r * n).to(torch.int32)
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=x.device)
    indptr[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
    info = info.cpu().tolist()
    return indptr, indices.contiguous(), values.contiguous(), dict(k=k, untied=int(info[0]), bad_rows=int(info[1]),
                                                                 knn=[int(v) for v in knn_info.cpu().tolist()])


def tsne_gradient(Y, P, exaggeration=1.0, exact_pairs=False):
    """(grad float64 [n, 2], Z, KL) of scd_tsne_gradient at Y for P = (indptr, indices, values): grad on the device, Z and KL Python
    floats; exact_pairs: the all-pairs sums in float64.  ValueError when the device flags a CSR entry out of range or a row of Y that is not finite below 2^60."""
    indptr, indices, values = P[:3]
    Y = torch.as_tensor(Y)
    if not Y.is_cuda:
        Y = Y.cuda()
    grad, z, kl, info = ops.tsne_gradient(Y.float().contiguous(), indptr, indices, values, exaggeration, exact_pairs=exact_pairs)
    bad = info.cpu().tolist()
    if bad[0] or bad[1]:
        raise ValueError("tsne_gradient: %d rows with a CSR entry out of range, %d rows of Y not finite below 2^60" % (bad[0], bad[1]))
    return grad, float(z.item()), float(kl.item())


def pca_init(x, scale=1e-4):
    """The first two principal components of x (float64 covariance, signs as scikit-learn's svd_flip: the largest-magnitude entry of each
    axis is positive), scaled so that the first has standard deviation `scale`: TSNE(init='pca')."""
    x64 = x.double()
    xc = x64 - x64.mean(0, keepdim=True)
    d = xc.shape[1]
    if d < 2:
        raise ValueError("init='pca' needs at least two feature columns")
    w, v = torch.linalg.eigh((xc.T @ xc).cpu())                 # ascending eigenvalues; D x D on the host: deterministic
    axes = v[:, [d - 1, d - 2]].T.contiguous()
    for a in axes:
        if a[torch.argmax(a.abs())] < 0:
            a.neg_()
    y = xc @ axes.T.to(xc.device)
    return y / y[:, 0].std(unbiased=False) * scale


class TSNE:
    """scikit-learn's TSNE for two components on the device, exact gradient.  fit_transform(x) -> float32 numpy [n, 2]; embedding_,
    kl_divergence_ (KL at the returned embedding, exaggeration 1), n_iter_, info_ afterwards."""

    def __init__(self, n_components=2, perplexity=30.0, early_exaggeration=12.0, learning_rate='auto', max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, init='pca', random_state=None):
        if n_components != 2:
            raise ValueError("only n_components = 2 is built")
        if init not in ('pca', 'random'):
            raise ValueError("init must be 'pca' or 'random'")
        if learning_rate != 'auto' and not float(learning_rate) > 0:
            raise ValueError("learning_rate must be 'auto' or positive")
        if not float(early_exaggeration) >= 1.0:
            raise ValueError("early_exaggeration must be at least 1")
        self.n_components, self.perplexity, self.early_exaggeration = n_components, float(perplexity), float(early_exaggeration)
        self.learning_rate, self.max_iter, self.n_iter_without_progress = learning_rate, int(max_iter), int(n_iter_without_progress)
        self.min_grad_norm, self.init, self.random_state = float(min_grad_norm), init, random_state
        self.momentum_switch_iter = EXPLORATION_ITER

    def _descend(self, P, state, it, max_iter, momentum, exaggeration, n_iter_without_progress, lr):
        """_gradient_descent, which starts every call from zero velocity and unit gains: returns the last iteration index run."""
        y64, vel, gains, y32, gg, ws = state
        vel.zero_()
        gains.fill_(1.0)
        best_error, best_iter, i = np.finfo(float).max, it, it
        for i in range(it, max_iter):
            check = (i + 1) % N_ITER_CHECK == 0
            grad, z, kl, info = ops.tsne_gradient(y32, P[0], P[1], P[2], exaggeration, want_kl=check, ws=ws)
            ops.tsne_update(grad, y64, vel, gains, y32, momentum, lr, MIN_GAIN, gg_out=gg if check else None)
            if check:
                bad = info.cpu().tolist()
                if bad[0] or bad[1]:
                    raise FloatingPointError("t-SNE: the embedding left the finite range at iteration %d" % i)
                error = float(kl.item())
                if error < best_error:
                    best_error, best_iter = error, i
                elif i - best_iter > n_iter_without_progress:
                    break
                if float(torch.linalg.vector_norm(gg).item()) <= self.min_grad_norm:
                    break
        return i

    def fit_transform(self, x, y=None):
        x = knn._as_device_f32(x)
        n = x.shape[0]
        _check_perplexity(n, self.perplexity)
        P = joint_affinities(x, self.perplexity)
        self.info_ = P[3]
        if self.init == 'pca':
            y64 = pca_init(knn.unit_rows(x)).contiguous()
        else:
            rng = np.random.RandomState(self.random_state)      # the seeded host generator: 1e-4 * standard normal, as scikit-learn
            y64 = torch.as_tensor(1e-4 * rng.standard_normal(size=(n, 2))).to(x.device).contiguous()
        lr = max(n / self.early_exaggeration / 4.0, 50.0) if self.learning_rate == 'auto' else float(self.learning_rate)
        y32 = y64.float().contiguous()
        y64 = y32.double()                                      # the master starts at the float32 state the force kernels read
        nb = ops._L().scd_tsne_gradient_ws_bytes(n, P[1].numel())
        state = (y64, torch.zeros_like(y64), torch.ones_like(y64), y32, torch.empty_like(y64), ops._ws(max(nb, 16), x.device))
        explore = min(self.momentum_switch_iter, self.max_iter)
        it = self._descend(P, state, 0, explore, MOMENTUM[0], self.early_exaggeration, explore, lr)
        if it < explore - 1 or self.max_iter > explore:
            it = self._descend(P, state, it + 1, self.max_iter, MOMENTUM[1], 1.0, self.n_iter_without_progress, lr)
        self.n_iter_ = it                                       # the index of the last iteration run, as scikit-learn reports it
        _, _, kl, _ = ops.tsne_gradient(y32, P[0], P[1], P[2], 1.0, ws=state[5], exact_pairs=True)        # Z in float64 for the report
        self.kl_divergence_ = float(kl.item())
        self.learning_rate_ = lr
        self.embedding_ = y32.cpu().numpy()
        return self.embedding_
