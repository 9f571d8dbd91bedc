"""Gaussian mixtures with a full covariance matrix per component, or one shared by all ('tied'), on rows of at most 64 dimensions:
scikit-learn 1.7's GaussianMixture(covariance_type='full' | 'tied') on the HIP primitives of scd_amd/csrc/gmm_full.hip, with labelled
rows clamped to their class as in scd_amd.gmm.  docs/design/gmm_full.md has the semantics and the error model.

The estimator is scd_amd.gmm.GaussianMixture's (the loop, the stopping rule, the warnings, n_init, both init_params, the matching of a
k-means start to the labelled classes, the final forward pass), with another parameter family.  Every E-step, with the sufficient
statistics of the M-step, is one ops.gmm_full_em_step call.  The kernel receives, rounded to float32,

    mu [k, d],    Ut [k, d, d] = the transposes of the upper-triangular U_k with U_k U_k^T = Sigma_k^-1,    a_k = log w_k + sum_j log U_k[j][j]

and returns nk, s1c = sum_i r_ik (x_i - mu_k) and S = sum_i r_ik (x_i - mu_k)(x_i - mu_k)^T about those float32 means.  The M-step and
the Cholesky factors are float64 numpy on the host: k d^3 / 3 operations, against a copy of S (32 MB at k = 1000, d = 64) and of Ut
(16 MB) per step.  'tied' is the same kernel with one factor replicated k times.  The constant -(d / 2) log 2 pi is added in float64.
"""
import numpy as np
import torch

from . import ops
from .gmm import EPS64, GaussianMixture, _as_device_f32  # noqa: F401  (the estimator is shared by import)

COVARIANCE_TYPES = ("full", "tied")
MAX_FEATURES = 64
ILL_DEFINED = ("Fitting the mixture model failed because some components have ill-defined empirical covariance (for instance caused by "
               "singleton or collapsed samples). Try to decrease the number of components, increase reg_covar, or scale the input data.")


def m_step(nk, s1c, S, m, covariance_type, reg_covar):
    """scikit-learn's _estimate_gaussian_parameters from the statistics about the means m (float64 numpy: nk [k], s1c [k, d],
    S [k, d, d], m [k, d]): (weights [k], means [k, d], covariances [k, d, d] for 'full' or [d, d] for 'tied').  A component without
    mass gets mean 0 and covariance reg_covar I, as there."""
    nk2 = nk + 10.0 * EPS64
    mu = (s1c + nk[:, None] * m) / nk2[:, None]
    delta = mu - m
    scat = (S - delta[:, :, None] * s1c[:, None, :] - s1c[:, :, None] * delta[:, None, :]
            + nk[:, None, None] * delta[:, :, None] * delta[:, None, :])
    d = m.shape[1]
    if covariance_type == "full":
        cov = scat / nk2[:, None, None]
        cov[:, np.arange(d), np.arange(d)] += reg_covar
    elif covariance_type == "tied":
        cov = scat.sum(axis=0) / nk2.sum()
        cov[np.arange(d), np.arange(d)] += reg_covar
    else:
        raise ValueError(covariance_type)
    return nk2 / nk2.sum(), mu, cov


def precision_cholesky_t(cov):
    """Ut [k, d, d] (or [d, d]) float64 from covariances of the same shape: Ut = L^-1 with cov = L L^T, the transpose of scikit-learn's
    precisions_cholesky_; lower triangular with exact zeros above the diagonal.  Forward substitution, batched over the components."""
    cov = np.asarray(cov, np.float64)
    try:
        L = np.linalg.cholesky(cov)
    except np.linalg.LinAlgError:
        raise ValueError(ILL_DEFINED)
    if not np.all(np.isfinite(L)):
        raise ValueError(ILL_DEFINED)
    Lb = L.reshape((-1,) + L.shape[-2:])
    d = Lb.shape[-1]
    inv = np.zeros_like(Lb)
    for i in range(d):
        inv[:, i, i] = 1.0
        if i:
            inv[:, i, :i] = -np.einsum("km,kml->kl", Lb[:, i, :i], inv[:, :i, :i])
        inv[:, i, :i + 1] /= Lb[:, i, i][:, None]
    return inv.reshape(L.shape)


def kernel_params(w, mu, ut, device):
    """(a [k], mu [k, d], Ut [k, d, d]) float32 on the device from float64 numpy weights, means and Ut ([k, d, d], or [d, d] for a tied
    factor, which is replicated); a without -(d / 2) log 2 pi."""
    k, d = mu.shape
    if ut.ndim == 2:
        ut = np.broadcast_to(ut, (k, d, d))
    a = np.log(w) + np.log(np.diagonal(ut, axis1=1, axis2=2)).sum(axis=1)
    return tuple(torch.as_tensor(np.ascontiguousarray(t, dtype=np.float32), device=device) for t in (a, mu, ut))


def n_parameters(k, d, covariance_type):
    """Free parameters: the covariance triangles (one for 'tied'), the means, and the weights less one."""
    return (k if covariance_type == "full" else 1) * d * (d + 1) // 2 + k * d + k - 1


class FullGaussianMixture(GaussianMixture):
    """FullGaussianMixture(n_components=1, covariance_type='full', tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1,
    init_params='kmeans', weights_init=None, means_init=None, precisions_init=None, random_state=None): scd_amd.gmm.GaussianMixture
    with covariance_type 'full' | 'tied', for rows of at most 64 features.  precisions_init has scikit-learn's shape, (k, d, d) or
    (d, d).  After fit: weights_, means_, covariances_, precisions_, precisions_cholesky_ ([k, d, d], or [d, d] for 'tied') and the
    rest as there."""

    def __init__(self, n_components=1, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, init_params="kmeans",
                 weights_init=None, means_init=None, precisions_init=None, random_state=None):
        if covariance_type not in COVARIANCE_TYPES:
            raise ValueError("covariance_type must be one of %s (got %r); scd_amd.gmm.GaussianMixture has 'diag' and 'spherical'" %
                             (COVARIANCE_TYPES, covariance_type))
        super().__init__(n_components, "diag", tol, reg_covar, max_iter, n_init, init_params, weights_init, means_init, precisions_init,
                         random_state)
        self.covariance_type = covariance_type

    def _check_features(self, d):
        if d > MAX_FEATURES:
            raise ValueError("full and tied covariances take at most %d features (got %d): reduce the rows first, with scd_amd.pca.PCA "
                             "or --pca_dim M of the scripts" % (MAX_FEATURES, d))

    # ------------------------------------------------------------------ the start
    def _explicit(self, d, device):
        """(w, mu, cov) float64 numpy from weights_init / means_init / precisions_init where all three are given, else None."""
        given = [t is not None for t in (self.weights_init, self.means_init, self.precisions_init)]
        if not any(given):
            return None
        if not all(given):
            raise ValueError("weights_init, means_init and precisions_init are given together or not at all")
        k = self.n_components
        w = np.asarray(self.weights_init, np.float64)
        mu = np.asarray(self.means_init, np.float64)
        prec = np.asarray(self.precisions_init, np.float64)
        if w.shape != (k,) or not np.all(w > 0) or abs(w.sum() - 1.0) > 1e-8:
            raise ValueError("weights_init: %d positive numbers that sum to 1" % k)
        if mu.shape != (k, d):
            raise ValueError("means_init: shape (%d, %d)" % (k, d))
        want = (k, d, d) if self.covariance_type == "full" else (d, d)
        if prec.shape != want or not np.allclose(prec, np.swapaxes(prec, -1, -2)) or np.any(np.linalg.eigvalsh(prec) <= 0):
            raise ValueError("precisions_init: symmetric positive definite, shape %s for covariance_type=%r" % (want, self.covariance_type))
        return w, mu, np.linalg.inv(prec)

    def _hard(self, x, lab, centres):
        _, nk, s1c, S, _, _ = ops.gmm_full_em_step(x, None, centres, None, y=lab)
        return nk.cpu().numpy(), s1c.cpu().numpy(), S.cpu().numpy()

    def _start(self, x, y, seed):
        """The hard M-step on the starting labels, taken about the classes' own means (a first pass about 0 finds them)."""
        k, d = self.n_components, x.shape[1]
        lab = self._start_labels(x, y, seed)
        zero = torch.zeros((k, d), dtype=torch.float32, device=x.device)
        nk, s1, _ = self._hard(x, lab, zero)
        centres = (s1 / (nk + 10.0 * EPS64)[:, None]).astype(np.float32)
        nk, s1c, S = self._hard(x, lab, torch.as_tensor(centres, device=x.device))
        return m_step(nk, s1c, S, centres.astype(np.float64), self.covariance_type, self.reg_covar)

    # ------------------------------------------------------------------ the loop (scikit-learn's BaseMixture.fit_predict)
    def _run(self, x, y, params):
        n, d = x.shape
        const = -0.5 * d * np.log(2.0 * np.pi)
        w, mu, cov = params
        lower, trace, converged, n_iter, info = -np.inf, [], False, 0, None
        for n_iter in range(1, self.max_iter + 1):
            prev = lower
            a, m32, ut = kernel_params(w, mu, precision_cholesky_t(cov), x.device)
            ll, nk, s1c, S, _, info = ops.gmm_full_em_step(x, a, m32, ut, y=y)
            w, mu, cov = m_step(nk.cpu().numpy(), s1c.cpu().numpy(), S.cpu().numpy(), m32.double().cpu().numpy(), self.covariance_type,
                                self.reg_covar)
            lower = float(ll.item()) / n + const
            trace.append(lower)
            if abs(lower - prev) < self.tol:
                converged = True
                break
        return dict(w=w, mu=mu, cov=cov, lower=lower, trace=trace, converged=converged, n_iter=n_iter, info=info)

    def _store(self, best):
        w, mu, cov = best["w"], best["mu"], best["cov"]
        ut = precision_cholesky_t(cov)
        dev = best["info"].device
        self._abc = kernel_params(w, mu, ut, dev)
        self.weights_, self.means_, self.covariances_ = w, mu, cov
        self.precisions_cholesky_ = np.swapaxes(ut, -1, -2).copy()
        self.precisions_ = self.precisions_cholesky_ @ np.swapaxes(self.precisions_cholesky_, -1, -2)

    def _kernel_forward(self, x, want_ll=False, want_resp=False):
        return ops.gmm_full_predict(x, *self._abc, want_ll=want_ll, want_resp=want_resp)

    def _n_parameters(self):
        return n_parameters(self.n_components, self.n_features_in_, self.covariance_type)
