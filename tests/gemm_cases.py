"""Inputs and error budgets of the GEMM-family tests (tests/test_gpu_gemm.py runs the kernels against them, tests/
test_gemm_budget_sensitivity.py checks on the CPU that the budgets would see the faults these kernels could have).  numpy float64 only.

The budgets are derived in the docstring of tests/test_gpu_gemm.py; this file is their one implementation.
"""
import math

import numpy as np

from oracle import clip_oracle as co

U16 = 2.0 ** -11            # half an fp16 ulp, relative
U32 = 2.0 ** -24            # half an fp32 ulp, relative
C1 = 1.0
LIP = 1.13                  # max |d act / d x| of QuickGELU (1.10) and erf-GELU (1.13)
SLACK = 1.0 + 2.0 ** -9     # second-order terms (a rounding error of a value that already carries an error)
KAPPA_LIMIT = 2.0 ** 18     # E[x^2] / (var + eps) up to which the folded form is asserted (docs/design/gemm.md)

# gemm.hip SCD_GELU_K0..K6: logit Phi(x) ~ -x p(x^2) / log2(e)
GELU_K = (-2.30220745, -0.104839488, 9.69095658e-05, 0.000158966471, -1.14071321e-05, 3.83554556e-07, -5.212611e-09)


def k_eff(k):
    """roundings a product can pass through in the fp32 accumulation: a chain of k / 16 (v_mfma_f32_32x32x16_f16; k / 32 for the
    16x16x32 form) instructions plus at most 31 inside the instruction that adds its products, whatever order the hardware uses"""
    return k / 16.0 + 32.0


def _gelu_poly(x):
    s = x * x
    p = np.zeros_like(x)
    pabs = np.zeros_like(x)
    for c in reversed(GELU_K):
        p = p * s + c
        pabs = pabs * s + abs(c)
    return p, pabs


def _gelu_fit_error():
    """largest distance of the kernel's GELU formula, evaluated exactly, from erf-GELU: the approximation error of the fit"""
    x = np.concatenate([np.linspace(-40, 40, 400001), np.linspace(-10, 10, 400001)])
    p, _ = _gelu_poly(x)
    with np.errstate(over="ignore"):
        y = x / (1.0 + np.exp2(x * p))
    return float(np.abs(y - co.act_f64(x, 2)).max()) * 1.05


GELU_FIT = _gelu_fit_error()


def act_term(x, act):
    """error of evaluating the activation in fp32 at an exact pre-activation x (the docstring's activation term)"""
    x = np.asarray(x, dtype=np.float64)
    if act == 0:
        return np.zeros_like(x)
    with np.errstate(over="ignore"):
        if act == 1:
            e = 1.702 * math.log2(math.e) * x
            one_minus_s = 1.0 / (1.0 + np.exp2(e))
            err_e = U32 * 2.0 * np.abs(e)
            fit = 0.0
        else:
            p, pabs = _gelu_poly(x)
            e = -x * p
            one_minus_s = 1.0 / (1.0 + np.exp2(e))
            err_e = U32 * (14.0 * np.abs(x) * pabs + 2.0 * np.abs(e))
            fit = GELU_FIT
    rel = 6.0 * U32 + math.log(2.0) * one_minus_s * err_e
    return fit + rel * np.abs(co.act_f64(x, act))


def budget_plain(a, w, bias=None, act=0, residual=None, extra_pre=None):
    """per-element budget of C = fp16(act(a w^T + bias)) (+ residual, rounded again) against gemm_f64.  extra_pre: a further
    pre-activation error (operands that carry an error of their own)."""
    a, w = np.asarray(a, np.float64), np.asarray(w, np.float64)
    mag = np.abs(a) @ np.abs(w).T
    pre = a @ w.T
    d_pre = C1 * U32 * k_eff(a.shape[1]) * mag
    if bias is not None:
        pre = pre + np.asarray(bias, np.float64)
        d_pre = d_pre + U32 * np.abs(pre)
    if extra_pre is not None:
        d_pre = d_pre + extra_pre
    return _finish(pre, d_pre, act, residual)


def _finish(pre, d_pre, act, residual):
    x = co.act_f64(pre, act)
    b = (LIP if act else 1.0) * d_pre + act_term(pre, act) + U16 * np.abs(x)
    if residual is not None:
        b = b + U16 * np.abs(x + np.asarray(residual, np.float64))
    return SLACK * b + U32


def rstd_rel_error(parts, eps, k, stats_rounded):
    """relative error of ln_finish_kernel's rstd (and the conditioning kappa it carries) for the rows of `parts`"""
    kappa = parts["ex2"] / (parts["var"] + eps)
    x = 10.0 * U32 * kappa                       # delta var / (var + eps): 3 u32 on E[x^2], 6 u32 on mean^2, u32 on the difference
    if stats_rounded:
        x = x + 2.0 ** -21 / k / (parts["var"] + eps)
    return 0.5 * x / (1.0 - np.minimum(x, 0.5)) + 2.5 * U32, kappa


def budget_folded(a, wf, biasf, colsum, parts, eps, act=0, stats_rounded=False, extra_pre=None):
    """per-element budget of the LN = 1 GEMM against gemm_ln_folded_f64 on the same folded operands and statistics"""
    a, wf = np.asarray(a, np.float64), np.asarray(wf, np.float64)
    k = a.shape[1]
    rho, _ = rstd_rel_error(parts, eps, k, stats_rounded)
    rstd = parts["rstd"][:, None]
    t1 = np.abs(rstd * parts["acc"])
    t2 = np.abs((parts["mean"] * parts["rstd"])[:, None] * np.asarray(colsum, np.float64)[None, :])
    t3 = np.abs(np.asarray(biasf, np.float64))[None, :]
    # rstd is rounded once and nmr = -mean * rstd is formed from that same number: its error rho moves the cancelled sum pre - b';
    # only the independent roundings (mean 3 v, nmr's product, nmr * colsum, + b', the final multiply-add) scale with t1 + t2
    d_pre = (rstd * C1 * U32 * k_eff(k) * (np.abs(a) @ np.abs(wf).T) + rho[:, None] * np.abs(parts["pre"] - np.asarray(biasf, np.float64)[None, :])
             + 7.0 * U32 * (t1 + t2) + 2.0 * U32 * t3)
    if extra_pre is not None:
        d_pre = d_pre + extra_pre
    return _finish(parts["pre"], d_pre, act, None)


def fold_errors(w, gamma, beta, bias):
    """what fold_ln_kernel may add: |Wf - W gamma|, |colsum - sum Wf|, |biasf - (b + W beta)| (lane-strided fp32 sums of k / 64 terms,
    six wave-reduction steps, one more addition)"""
    w, gamma, beta = np.asarray(w, np.float64), np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    k = w.shape[1]
    wg = np.abs(w * gamma[None, :])
    d_w = (U16 + 2 * U32) * wg + 2.0 ** -25
    d_cs = (k / 64.0 + 7.0) * U32 * (wg + d_w).sum(1)
    d_b = (k / 64.0 + 8.0) * U32 * (np.abs(w * beta[None, :]).sum(1) + np.abs(np.asarray(bias, np.float64)))
    return d_w, d_cs, d_b


def budget_true(a, w, gamma, beta, bias, wf, biasf, colsum, parts, eps, act=0):
    """budget of the LN = 1 GEMM (operands folded by fold_ln_kernel, statistics = row_stats_int of a) against ln_linear_f64"""
    a = np.asarray(a, np.float64)
    d_w, d_cs, d_b = fold_errors(w, gamma, beta, bias)
    rstd, mean = parts["rstd"][:, None], parts["mean"][:, None]
    extra = rstd * (np.abs(a - mean) @ d_w.T) + np.abs(mean * rstd) * d_cs[None, :] + d_b[None, :]
    return budget_folded(a, wf, biasf, colsum, parts, eps, act, stats_rounded=True, extra_pre=extra)


def layernorm_error(x, gamma, beta, eps):
    """per-element budget of layernorm_kernel's fp16 output against layernorm_f64 (two-pass fp32: lane sums of width / 64 terms, six
    wave-reduction steps, rsqrtf within 2 ulps)"""
    x = np.asarray(x, np.float64)
    gamma, beta = np.asarray(gamma, np.float64)[None, :], np.asarray(beta, np.float64)[None, :]
    k = x.shape[1]
    n = k / 64.0 + 6.0
    mean = x.mean(1, keepdims=True)
    d = x - mean
    var = (d * d).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    d_mean = n * U32 * np.abs(x).mean(1, keepdims=True)
    r_rel = (n + 2.0) * U32 + d_mean * np.abs(d).mean(1, keepdims=True) / (var + eps) + 2.0 ** -22
    y = d * rstd * gamma + beta
    b = (d_mean + U32 * np.abs(d)) * rstd * np.abs(gamma) + np.abs(d * rstd * gamma) * (r_rel + 3.0 * U32) + U32 * np.abs(y)
    return SLACK * (b + U16 * np.abs(y)) + 2.0 ** -25


def budget_unfused(a, w, gamma, beta, bias, eps, act=0):
    """budget of layernorm_kernel -> scd_gemm_f16 against ln_linear_f64"""
    y = co.layernorm_f64(a, gamma, beta, eps)
    extra = layernorm_error(a, gamma, beta, eps) @ np.abs(np.asarray(w, np.float64)).T
    return budget_plain(y, w, bias, act, None, extra_pre=extra)


# ------------------------------------------------------------------------------------------------ inputs
ROW_KINDS = ("gauss", "outlier", "mean1", "mean10", "mean100", "const", "zeros")


def f16(x):
    return np.asarray(x, dtype=np.float64).astype(np.float16)


def real_rows(m, k, seed):
    """fp16 [m, k]: the row kinds of ROW_KINDS in turn (row i has kind i % 7).  Every row stays below KAPPA_LIMIT for eps >= 1e-6."""
    rs = np.random.RandomState(seed)
    a = rs.randn(m, k) * 0.5
    kind = np.arange(m) % len(ROW_KINDS)
    for i in np.nonzero(kind == 1)[0]:
        a[i, rs.randint(k)] = rs.uniform(50, 200) * 0.5 * rs.choice([-1, 1])
    a[kind == 2] += 0.5
    a[kind == 3] = a[kind == 3] * 0.2 + 1.0
    a[kind == 4] = a[kind == 4] * 0.1 + 5.0
    a[kind == 5] = 0.5
    a[kind == 6] = 0.0
    return f16(a), kind


def real_layer(n, k, seed):
    """W fp16 [n, k], gamma (with large and tiny entries), beta, bias float32"""
    rs = np.random.RandomState(seed)
    w = f16(rs.randn(n, k) * k ** -0.5)
    gamma = np.exp(rs.randn(k) * 0.3)
    gamma[rs.choice(k, 8, replace=False)] = [8.0, -6.0, 12.0, 5.0, 2.0 ** -10, -2.0 ** -12, 1e-4, 3e-5]
    beta = rs.randn(k) * 0.1
    bias = rs.randn(n) * 0.5
    return w, gamma.astype(np.float32), beta.astype(np.float32), bias.astype(np.float32)


def fold_host(w, gamma, beta, bias):
    """fold_ln_kernel's outputs computed on the host (for the CPU sensitivity test): W' = fp16(W gamma), colsum, b'"""
    wg, bf = co.fold_ln_f64(w, gamma, beta, bias)
    wf = f16(wg)
    return wf, wf.astype(np.float64).sum(1).astype(np.float32), bf.astype(np.float32)


def exact_operands(m, n, k, seed, w_max=2, a_density=1.0, cap=8):
    """integers in fp16: a in {-1, 0, 1}, w in {-w_max..w_max}, bias and residual in {-cap..cap}"""
    rs = np.random.RandomState(seed)
    a = rs.randint(-1, 2, size=(m, k))
    if a_density < 1.0:
        a = a * (rs.random_sample((m, k)) < a_density)
    w = rs.randint(-w_max, w_max + 1, size=(n, k))
    bias = rs.randint(-cap, cap + 1, size=n)
    res = rs.randint(-cap, cap + 1, size=(m, n))
    return a.astype(np.float16), w.astype(np.float16), bias.astype(np.float32), res.astype(np.float16)


def assert_exact_conditions(ref, mag, cap=2048):
    """the two conditions under which every product, fp32 partial sum and the fp16 result are exact"""
    assert float(np.abs(ref).max()) <= cap, float(np.abs(ref).max())
    assert float(mag.max()) < 2.0 ** 24, float(mag.max())


def img_weights(n):
    """W [n, 768] in {-2..2}: column k carries the base-5 digits of k (spread over the rows), so every (channel, row, column) of a
    patch has a weight pattern of its own"""
    k = np.arange(768)[None, :]
    r = np.arange(n)[:, None]
    w = ((k + 7 * (r // 5)) // 5 ** (r % 5)) % 5 - 2
    assert len(np.unique(w.T, axis=0)) == 768
    return w.astype(np.float16)


def img_pixels(batch, image, seed):
    return np.random.RandomState(seed).randint(-2, 3, size=(batch, 3, image, image)).astype(np.float16)
