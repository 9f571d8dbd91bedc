"""Principal component analysis: scikit-learn 1.7's PCA(svd_solver='covariance_eigh') on the HIP primitives of scd_amd/csrc/pca.hip.
docs/design/pca.md has the semantics and the error model.

The rows are never copied, centred or widened: the kernels subtract a float32 shift a (the rounded mean) in a register, the Gram matrix
G = c^T c of c = fl32(x - a) and the residual column sums csum of c come back in float64, and

    S = G - csum csum^T / n,    mean_ = a + csum / n,    cov = S / (n - 1)

are exact restatements of the centred scatter in float64.  The eigensolver of the d x d matrix runs on the host (torch.linalg.eigh on
the CPU, one LAPACK whatever the device).  transform is one ops.pca_transform call at the same shift, so it projects x - a and not
x - mean_: the two differ by csum / n, below one float32 ulp of the mean.  Rows are taken as given.
"""
import numpy as np
import torch

from . import ops
from .gmm import _as_device_f32

D_MAX = 1024


def svd_flip_rows(v):
    """scikit-learn's svd_flip(u_based_decision=False) on the rows of v (float64 tensor [m, d]): the entry of largest magnitude of each
    row (the first one on a tie) becomes positive."""
    idx = torch.argmax(v.abs(), dim=1)
    signs = torch.sign(v[torch.arange(v.shape[0]), idx])
    signs = torch.where(signs == 0, torch.ones_like(signs), signs)
    return v * signs[:, None]


def spectrum(cov, n_samples):
    """The host half of the fit, float64 CPU tensors: cov [d, d] -> (explained_variance [d] descending with negatives set to 0,
    components [d, d] as rows with svd_flip's signs, singular_values [d])."""
    vals, vecs = torch.linalg.eigh(cov)
    vals = torch.flip(vals, dims=(0,)).clone()
    vecs = torch.flip(vecs, dims=(1,))
    vals[vals < 0.0] = 0.0
    return vals, svd_flip_rows(vecs.T.contiguous()), torch.sqrt(vals * (n_samples - 1))


def choose_n_components(n_components, ratio, n, d):
    """scikit-learn's rule: None -> min(n, d); a float in (0, 1) -> searchsorted(cumsum(ratio), f, side='right') + 1; an int as given."""
    if n_components is None:
        return min(n, d)
    if isinstance(n_components, (float, np.floating)):
        if not 0.0 < n_components < 1.0:
            raise ValueError("a float n_components lies in (0, 1) (got %r)" % (n_components,))
        return int(np.searchsorted(np.cumsum(ratio, dtype=np.float64), n_components, side="right") + 1)
    m = int(n_components)
    if m < 1 or m > min(n, d):
        raise ValueError("n_components = %d must lie in [1, min(n_samples, n_features) = %d]" % (m, min(n, d)))
    return m


class PCA:
    """PCA(n_components=None, whiten=False): fit(X), transform(X, unit=False), fit_transform(X, unit=False), inverse_transform(Y).
    After fit, as float64 numpy arrays: components_ [m, d], explained_variance_, explained_variance_ratio_, singular_values_ [m],
    mean_ [d], and noise_variance_, n_components_, n_samples_, n_features_in_.  transform returns float32 [n, m] on the device; with
    unit=True every row is divided by its L2 norm (a row equal to the shift gives zeros)."""

    def __init__(self, n_components=None, whiten=False):
        if n_components is not None and not isinstance(n_components, (int, float, np.integer, np.floating)):
            raise ValueError("n_components is None, an int or a float in (0, 1) (got %r)" % (n_components,))
        if isinstance(n_components, (int, np.integer)) and n_components > D_MAX:
            raise ValueError("n_components = %d is beyond the kernel's limit of %d" % (n_components, D_MAX))
        self.n_components, self.whiten = n_components, bool(whiten)

    def fit(self, X):
        x = _as_device_f32(X)
        n, d = int(x.shape[0]), int(x.shape[1])
        if d > D_MAX:
            raise ValueError("at most %d features (got %d)" % (D_MAX, d))
        if n < 2:
            raise ValueError("a covariance needs at least 2 rows (got %d)" % n)
        a = (ops.pca_colsum(x) / n).float()
        g, info = ops.pca_gram(x, a)
        csum = ops.pca_colsum(x, a)
        bad = int(info[0].item())
        if bad:
            raise ValueError("%d rows hold a non-finite value" % bad)
        g, csum, a64 = g.cpu(), csum.cpu(), a.double().cpu()
        s = g - torch.outer(csum, csum) / n
        mean = a64 + csum / n
        var, comps, sing = spectrum(s / (n - 1), n)
        total = var.sum()
        ratio = var / total
        m = choose_n_components(self.n_components, ratio.numpy(), n, d)
        self.noise_variance_ = float(var[m:].mean().item()) if m < min(n, d) else 0.0
        self.n_samples_, self.n_components_, self.n_features_in_ = n, m, d
        self.components_ = comps[:m].contiguous().numpy().copy()
        self.explained_variance_ = var[:m].numpy().copy()
        self.explained_variance_ratio_ = ratio[:m].numpy().copy()
        self.singular_values_ = sing[:m].numpy().copy()
        self.mean_ = mean.numpy().copy()
        w = comps[:m]
        if self.whiten:
            w = w / torch.sqrt(var[:m])[:, None]                # float64, rounded once below
        self._shift = a
        self._w = w.float().contiguous().to(x.device)
        return self

    def _project(self, x, unit):
        y, info = ops.pca_transform(x, self._w, self._shift, unit=unit)
        self.info_ = info
        return y

    def transform(self, X, unit=False):
        if not hasattr(self, "_w"):
            raise ValueError("this PCA is not fitted")
        x = _as_device_f32(X)
        if x.shape[1] != self.n_features_in_:
            raise ValueError("X has %d features, the fit had %d" % (x.shape[1], self.n_features_in_))
        return self._project(x, unit)

    def fit_transform(self, X, unit=False):
        x = _as_device_f32(X)
        return self.fit(x)._project(x, unit)

    def inverse_transform(self, Y):
        """Rows in the original space, float64 on Y's device (a plain product, as scikit-learn's)."""
        if not hasattr(self, "_w"):
            raise ValueError("this PCA is not fitted")
        y = torch.as_tensor(Y).double()
        comps = torch.as_tensor(self.components_, device=y.device)
        if self.whiten:
            comps = comps * torch.sqrt(torch.as_tensor(self.explained_variance_, device=y.device))[:, None]
        return y @ comps + torch.as_tensor(self.mean_, device=y.device)
