"""Gaussian mixtures with diagonal covariances: scikit-learn 1.7's GaussianMixture(covariance_type='diag' | 'spherical') on the HIP
primitives of scd_amd/csrc/gmm.hip, with labelled rows clamped to their class (the semi-supervised mixture of GPC, "Learning
semi-supervised Gaussian mixture models for generalized category discovery").  docs/design/gmm.md has the semantics and the error model.

Every E-step, with the sufficient statistics of the M-step, is one ops.gmm_em_step call (float32-input MFMA on x and x^2, the softmax in
registers, the moments accumulated in float64); predict, predict_proba and score_samples are ops.gmm_predict.  The parameters live as
float64 device tensors; the M-step is a few lines of torch on [k, d] numbers.  The kernel receives

    a_k = log w_k - 0.5 sum_d mu_kd^2 / v_kd - 0.5 sum_d log v_kd,    B = mu / v,    C = -1 / (2 v)

rounded to float32; the constant -(d / 2) log 2 pi is left out of a (the softmax does not see it, and a float32 a_k keeps more of
log w_k without it) and added to every log-likelihood in float64.  Rows are taken as given.
"""
import math
import warnings

import numpy as np
import torch

from . import ops

COVARIANCE_TYPES = ("diag", "spherical")
INIT_PARAMS = ("kmeans", "random")
EPS64 = float(np.finfo(np.float64).eps)


class ConvergenceWarning(UserWarning):
    """The fit reached max_iter before the lower bound's change fell below tol (scikit-learn's warning of the same name)."""


def _as_device_f32(x):
    if isinstance(x, np.ndarray):
        x = torch.as_tensor(np.ascontiguousarray(x))
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError("the mixture needs a 2-d array of rows")
    if not x.is_cuda:
        x = x.cuda()
    return x.float().contiguous()


def m_step(nk, s1, s2, covariance_type, reg_covar):
    """scikit-learn's _estimate_gaussian_parameters and the weights' normalisation from the sufficient statistics (float64 tensors):
    (weights [k], means [k, d], variances [k, d]; 'spherical' holds each component's mean variance in every column).  A component
    without mass gets mean 0 and variance reg_covar, as there."""
    nk = nk + 10.0 * EPS64
    mu = s1 / nk[:, None]
    v = s2 / nk[:, None] - mu * mu + reg_covar
    if covariance_type == "spherical":
        v = v.mean(dim=1, keepdim=True).expand_as(mu).contiguous()
    return nk / nk.sum(), mu, v


def kernel_params(w, mu, v):
    """(a, B, C) float32 for the kernel from float64 weights, means and variances [k, d]; a without -(d / 2) log 2 pi."""
    a = torch.log(w) - 0.5 * (mu * mu / v).sum(dim=1) - 0.5 * torch.log(v).sum(dim=1)
    return a.float(), (mu / v).float(), (-0.5 / v).float()


def n_parameters(k, d, covariance_type):
    """Free parameters: means, variances, and the weights less one."""
    return 2 * k * d + k - 1 if covariance_type == "diag" else k * d + 2 * k - 1


class GaussianMixture:
    """GaussianMixture(n_components=1, covariance_type='diag', tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, init_params='kmeans',
    weights_init=None, means_init=None, precisions_init=None, random_state=None): fit(X, y=None), fit_predict, predict, predict_proba,
    score_samples, score, bic, aic.  y holds labels in [0, n_components) for the rows that are clamped to their class and -1 for the
    others.  After fit: weights_ [k], means_ [k, d], covariances_ and precisions_ ([k, d] for 'diag', [k] for 'spherical') as float64
    numpy arrays, converged_, n_iter_, lower_bound_, lower_bounds_, labels_ (numpy int64) and labels_device_ (int32 on the device)."""

    def __init__(self, n_components=1, covariance_type="diag", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, init_params="kmeans",
                 weights_init=None, means_init=None, precisions_init=None, random_state=None):
        if covariance_type not in COVARIANCE_TYPES:
            raise ValueError("covariance_type must be one of %s (got %r); full and tied covariances are out of scope" %
                             (COVARIANCE_TYPES, covariance_type))
        if init_params not in INIT_PARAMS:
            raise ValueError("init_params must be one of %s (got %r)" % (INIT_PARAMS, init_params))
        if int(n_components) < 1 or int(n_components) > 1024:
            raise ValueError("n_components must lie in [1, 1024] (got %r)" % (n_components,))
        if not tol >= 0 or not reg_covar >= 0 or int(max_iter) < 1 or int(n_init) < 1:
            raise ValueError("tol >= 0, reg_covar >= 0, max_iter >= 1 and n_init >= 1 are required")
        self.n_components, self.covariance_type, self.tol, self.reg_covar = int(n_components), covariance_type, float(tol), float(reg_covar)
        self.max_iter, self.n_init, self.init_params, self.random_state = int(max_iter), int(n_init), init_params, random_state
        self.weights_init, self.means_init, self.precisions_init = weights_init, means_init, precisions_init

    # ------------------------------------------------------------------ the start
    def _explicit(self, d, device):
        """(w, mu, v) from weights_init / means_init / precisions_init where all three are given, else None."""
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
        want = (k, d) if self.covariance_type == "diag" else (k,)
        if prec.shape != want or not np.all(prec > 0):
            raise ValueError("precisions_init: positive, shape %s for covariance_type=%r" % (want, self.covariance_type))
        v = 1.0 / prec
        if v.ndim == 1:
            v = np.repeat(v[:, None], d, axis=1)
        return tuple(torch.as_tensor(np.ascontiguousarray(t), device=device) for t in (w, mu, v))

    def _start_labels(self, x, y, seed):
        """Starting labels int32 [n] on the device: k-means' (scd_amd.cluster.KMeans, one start) or seeded random ones; a labelled row
        keeps its class."""
        k = self.n_components
        if self.init_params == "kmeans":
            from .cluster import KMeans
            lab = KMeans(n_clusters=k, n_init=1, random_state=seed).fit(x).labels_device_.to(torch.int32)
        else:
            gen = torch.Generator(device=x.device)
            gen.manual_seed(int(seed))
            lab = torch.randint(0, k, (x.shape[0],), generator=gen, device=x.device, dtype=torch.int32)
        if y is not None:
            if self.init_params == "kmeans":
                # k-means numbers its clusters as it pleases: give each cluster the class most of its labelled rows carry (a one-to-one
                # assignment that keeps the most labelled rows, the host solver of the naming stage), so that component j starts on class j
                known = y >= 0
                table = torch.zeros((k, k), dtype=torch.int64, device=x.device)
                table.index_put_((lab[known].long(), y[known].long()), torch.ones((), dtype=torch.int64, device=x.device), accumulate=True)
                table = table.cpu().numpy()
                pairs = ops.munkres(table.max() - table)
                perm = np.arange(k)
                perm[pairs[:, 0]] = pairs[:, 1]
                lab = torch.as_tensor(perm.astype(np.int32), device=x.device)[lab.long()]
            lab = torch.where(y >= 0, y, lab)
        return lab.contiguous()

    def _start(self, x, y, seed):
        """The hard M-step on the starting labels."""
        _, nk, s1, s2, _, _ = ops.gmm_em_step(x, None, None, None, y=self._start_labels(x, y, seed), n_components=self.n_components)
        return m_step(nk, s1, s2, self.covariance_type, self.reg_covar)

    # ------------------------------------------------------------------ the loop (scikit-learn's BaseMixture.fit_predict)
    def _run(self, x, y, params):
        n, d = x.shape
        const = -0.5 * d * math.log(2.0 * math.pi)
        w, mu, v = params
        lower, trace, converged, n_iter = -math.inf, [], False, 0
        for n_iter in range(1, self.max_iter + 1):
            prev = lower
            a, b, c = kernel_params(w, mu, v)
            ll, nk, s1, s2, _, info = ops.gmm_em_step(x, a, b, c, y=y)
            w, mu, v = m_step(nk, s1, s2, self.covariance_type, self.reg_covar)
            lower = float(ll.item()) / n + const
            trace.append(lower)
            if abs(lower - prev) < self.tol:
                converged = True
                break
        return dict(w=w, mu=mu, v=v, lower=lower, trace=trace, converged=converged, n_iter=n_iter, info=info)

    # ------------------------------------------------------------------ what a covariance family supplies (scd_amd.gmm_full overrides these)
    def _check_features(self, d):
        if d > 1024:
            raise ValueError("at most 1024 features (got %d)" % d)

    def _store(self, best):
        """The fitted parameters of the best run: the kernel's operands and scikit-learn's attributes."""
        self._w, self._mu, self._v = best["w"], best["mu"], best["v"]
        self._abc = kernel_params(self._w, self._mu, self._v)
        self.weights_ = self._w.cpu().numpy()
        self.means_ = self._mu.cpu().numpy()
        cov = self._v.cpu().numpy()
        self.covariances_ = cov if self.covariance_type == "diag" else cov[:, 0].copy()
        self.precisions_ = 1.0 / self.covariances_

    def _kernel_forward(self, x, want_ll=False, want_resp=False):
        return ops.gmm_predict(x, *self._abc, want_ll=want_ll, want_resp=want_resp)

    def fit(self, X, y=None):
        x = _as_device_f32(X)
        n, d = int(x.shape[0]), int(x.shape[1])
        k = self.n_components
        if n < k:
            raise ValueError("n_components = %d needs at least as many rows (got %d)" % (k, n))
        self._check_features(d)
        yd = None
        if y is not None:
            y_np = np.asarray(y.cpu() if torch.is_tensor(y) else y)
            if y_np.shape != (n,) or not np.issubdtype(y_np.dtype, np.integer):
                raise ValueError("y: one integer label per row, -1 for an unlabelled row")
            if y_np.min() < -1 or y_np.max() >= k:
                raise ValueError("y: labels lie in [0, n_components), -1 marks an unlabelled row")
            yd = torch.as_tensor(y_np.astype(np.int32), device=x.device)
        seeds = np.random.RandomState(self.random_state).randint(0, 2 ** 31 - 1, size=self.n_init)
        explicit = self._explicit(d, x.device)
        best = None
        for j in range(self.n_init):
            run = self._run(x, yd, explicit if explicit is not None else self._start(x, yd, int(seeds[j])))
            if best is None or run["lower"] > best["lower"]:
                best = run
        if not best["converged"]:
            warnings.warn("GaussianMixture: the best of %d start(s) did not converge in max_iter = %d iterations; raise max_iter or tol"
                          % (self.n_init, self.max_iter), ConvergenceWarning)
        bad = best["info"].cpu().numpy()
        if bad[1]:
            warnings.warn("GaussianMixture: %d rows had a non-finite log-density at the last E-step" % bad[1])
        self._store(best)
        self.converged_, self.n_iter_ = best["converged"], best["n_iter"]
        self.lower_bound_, self.lower_bounds_ = best["lower"], list(best["trace"])
        self.n_features_in_ = d
        # a final E-step makes the labels consistent with the parameters; a clamped row keeps its class
        pred = self._kernel_forward(x)[0]
        if yd is not None:
            pred = torch.where(yd >= 0, yd, pred)
        self.labels_device_ = pred
        self.labels_ = pred.cpu().numpy().astype(np.int64)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X, y).labels_

    # ------------------------------------------------------------------ the forward pass
    def _forward(self, X, want_ll=False, want_resp=False):
        if not hasattr(self, "_abc"):
            raise ValueError("this GaussianMixture is not fitted")
        x = _as_device_f32(X)
        if x.shape[1] != self.n_features_in_:
            raise ValueError("X has %d features, the fit had %d" % (x.shape[1], self.n_features_in_))
        return self._kernel_forward(x, want_ll=want_ll, want_resp=want_resp)

    def predict(self, X):
        """The most likely component of each row, int64 on the device."""
        return self._forward(X)[0].long()

    def predict_proba(self, X):
        """The membership probabilities float32 [n, k] on the device."""
        return self._forward(X, want_resp=True)[2]

    def score_samples(self, X):
        """The log-likelihood of each row, float64 [n] on the device (the kernel's float32 lse plus the constant)."""
        row = self._forward(X, want_ll=True)[1]
        return row.double() - 0.5 * self.n_features_in_ * math.log(2.0 * math.pi)

    def score(self, X, y=None):
        return float(self.score_samples(X).mean().item())

    def _n_parameters(self):
        return n_parameters(self.n_components, self.n_features_in_, self.covariance_type)

    def bic(self, X):
        n = int(X.shape[0])
        return -2.0 * self.score(X) * n + self._n_parameters() * math.log(n)

    def aic(self, X):
        return -2.0 * self.score(X) * int(X.shape[0]) + 2.0 * self._n_parameters()
