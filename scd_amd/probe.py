"""The linear probe of the DINO / DINOv2 evaluation protocol: multinomial logistic regression on frozen features, scikit-learn's
LogisticRegression(C) written as a sum,

    F(W, b) = sum_i s_i [lse_c(z_ic) - z_{i, y_i}] + (1 / 2C) |W|_F^2,    z_ic = W_c . x_i + b_c,

on the HIP primitives of scd_amd/csrc/probe.hip.  docs/design/probe.md has the semantics and the error model.

Every evaluation of the data term and its gradient is one ops.probe_loss_grad call (float32-input MFMA, the softmax in registers, the
gradient accumulated in float64); predict and score are ops.probe_predict.  The optimiser is L-BFGS with its state as float64 device
tensors: a few dot products over c (d + 1) numbers per iteration, which is torch plumbing.  Rows are taken as given: the caller
normalises (scd_amd.knn.unit_rows).
"""
import warnings

import numpy as np
import torch

from . import ops

ARMIJO = 1e-4               # F_new <= F + ARMIJO t g.p
PAIR_MIN = 1e-10            # a pair (s, y) is kept only when s.y > PAIR_MIN y.y
MIN_STEP = 2.0 ** -60       # the line search gives up below this step
NOISE_FLOOR = "LinearProbe: the line search could not decrease the objective (the float32 evaluation's noise floor); the fit stops here"
OUT_OF_BUDGET = "LinearProbe: max_iter = %d reached before max |grad| <= tol * sum of weights"


def _as_device_f32(x):
    if isinstance(x, np.ndarray):
        x = torch.as_tensor(np.ascontiguousarray(x))
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError("the probe needs a 2-d array of rows")
    if not x.is_cuda:
        x = x.cuda()
    return x.float().contiguous()


def _as_numpy(a):
    return np.asarray(a.cpu() if torch.is_tensor(a) else a)


class LinearProbe:
    """LinearProbe(C=1.0, fit_intercept=True, tol=1e-4, max_iter=1000, memory=10): fit(X, y, sample_weight=None), predict,
    decision_function, score.  After fit: classes_ (numpy), coef_ float64 [c, d] and intercept_ float64 [c] on the device, n_iter_,
    n_eval_ (evaluations of the kernel), objective_ (F at the result), grad_norm_ (max |grad F| there), converged_."""

    def __init__(self, C=1.0, fit_intercept=True, tol=1e-4, max_iter=1000, memory=10):
        if not C > 0:
            raise ValueError("C must be positive")
        self.C, self.fit_intercept, self.tol, self.max_iter, self.memory = float(C), bool(fit_intercept), float(tol), int(max_iter), int(memory)

    # the data term through the kernel at the float32 rounding of the float64 iterate, the L2 term in float64
    def _evaluate(self, x, y, sw, theta, c, d):
        W = theta[: c * d].view(c, d)
        b32 = theta[c * d:].float() if self.fit_intercept else None
        loss, gW, gb, _, info = ops.probe_loss_grad(x, y, W.float(), b32, sw)
        self.n_eval_ += 1
        lam = 1.0 / self.C
        F = float(loss.item()) + 0.5 * lam * float(torch.dot(theta[: c * d], theta[: c * d]).item())
        gW = gW + lam * W
        g = torch.cat([gW.reshape(-1), gb]) if self.fit_intercept else gW.reshape(-1)
        return F, g, info

    def fit(self, X, y, sample_weight=None):
        x = _as_device_f32(X)
        y_np = _as_numpy(y)
        if y_np.ndim != 1 or y_np.shape[0] != x.shape[0]:
            raise ValueError("one label per row")
        self.classes_, y_idx = np.unique(y_np, return_inverse=True)
        c, d = int(self.classes_.shape[0]), int(x.shape[1])
        if c < 2:
            raise ValueError("the probe needs at least two classes")
        yd = torch.as_tensor(y_idx.astype(np.int32)).to(x.device)
        sw = None
        wsum = float(x.shape[0])
        if sample_weight is not None:
            sw = torch.as_tensor(_as_numpy(sample_weight).astype(np.float32)).to(x.device).contiguous()
            if sw.shape != (x.shape[0],):
                raise ValueError("one sample weight per row")
            wsum = float(sw.double().sum().item())
        self.n_eval_, self.n_iter_, self.converged_ = 0, 0, False
        theta = torch.zeros(c * d + (c if self.fit_intercept else 0), dtype=torch.float64, device=x.device)
        F, g, info = self._evaluate(x, yd, sw, theta, c, d)
        pairs = []
        while True:
            gmax = float(g.abs().max().item())
            if gmax <= self.tol * wsum:
                self.converged_ = True
                break
            if self.n_iter_ >= self.max_iter or self.n_eval_ >= self.max_iter:
                warnings.warn(OUT_OF_BUDGET % self.max_iter)
                break
            q = g.clone()                                       # the two-loop recursion
            alphas = []
            for s_, y_, rho in reversed(pairs):
                a = rho * torch.dot(s_, q)
                alphas.append(a)
                q -= a * y_
            if pairs:
                s_, y_, _ = pairs[-1]
                q *= torch.dot(s_, y_) / torch.dot(y_, y_)
            for (s_, y_, rho), a in zip(pairs, reversed(alphas)):
                q += (a - rho * torch.dot(y_, q)) * s_
            p = -q
            gp = float(torch.dot(g, p).item())
            if not gp < 0:
                pairs, p = [], -g
                gp = float(torch.dot(g, p).item())
            t, done = 1.0, False
            while self.n_eval_ < self.max_iter and t > MIN_STEP:
                cand = theta + t * p
                Fn, gn, info = self._evaluate(x, yd, sw, cand, c, d)
                if Fn <= F + ARMIJO * t * gp:
                    done = True
                    break
                t *= 0.5
            if not done:
                warnings.warn(NOISE_FLOOR)
                break
            s_, y_ = cand - theta, gn - g
            sy, yy = float(torch.dot(s_, y_).item()), float(torch.dot(y_, y_).item())
            if sy > PAIR_MIN * yy:
                pairs.append((s_, y_, 1.0 / sy))
                pairs = pairs[-self.memory:]
            theta, F, g = cand, Fn, gn
            self.n_iter_ += 1
        bad = info.cpu().tolist()
        if bad[1]:
            warnings.warn("LinearProbe: %d rows had a non-finite logit at the last evaluation" % bad[1])
        self.coef_ = theta[: c * d].view(c, d).clone()
        self.intercept_ = theta[c * d:].clone() if self.fit_intercept else torch.zeros(c, dtype=torch.float64, device=x.device)
        self.objective_, self.grad_norm_ = F, float(g.abs().max().item())
        return self

    def _params32(self):
        return self.coef_.float().contiguous(), (self.intercept_.float().contiguous() if self.fit_intercept else None)

    def predict_index(self, X):
        """The class index (into classes_) of each row, int64 on the device: ops.probe_predict at the float32 parameters."""
        W, b = self._params32()
        return ops.probe_predict(_as_device_f32(X), W, b).long()

    def predict(self, X):
        return self.classes_[self.predict_index(X).cpu().numpy()]

    def decision_function(self, X):
        """The logits float64 [n, c] on the device, from the float64 parameters (a plain product: this is not on the fit's or predict's
        path, which never hold n x c logits)."""
        return _as_device_f32(X).double() @ self.coef_.t() + self.intercept_

    def score(self, X, y):
        """The accuracy: the exact count over the row count, a Python float."""
        pred = self.predict(X)
        want = _as_numpy(y)
        if want.shape != pred.shape:
            raise ValueError("one target per row")
        return int((pred == want).sum()) / pred.shape[0]
