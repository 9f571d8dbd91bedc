"""The Gaussian mixture's contract restated in float64 numpy (scd_gmm_em_step / scd_gmm_predict, scd_amd/gmm.py), its error model, the
cases and the planted mistakes.  docs/design/gmm.md derives the bounds.  Everything here is evaluated at the SAME float32 X, a, B, C the
device receives, so the only difference a test sees is the device's rounding."""
import numpy as np

import f32mm_plan as fp

U = 2.0 ** -24                                  # unit roundoff of float32
TINY = 2.0 ** -126                              # smallest normal float32: the absolute floor of an underflowing e
ROW_TILE = 32                                   # scd_gmm_row_tile(); the host test asserts the library agrees
CHAIN_ROWS = 256                                # scd_gmm_chain_rows()
EPS64 = float(np.finfo(np.float64).eps)
LOG_2PI = float(np.log(2.0 * np.pi))


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------- parameters
def abc_f64(w, mu, v, mistake=None):
    """(a, B, C) in float64 of z_ik = a_k + x_i . B_k + x_i^2 . C_k from weights [k], means [k, d] and variances [k, d] (a spherical
    variance is broadcast by the caller), WITHOUT the constant -(d / 2) log 2 pi: shift(d) holds it and is added to the row
    log-likelihoods in float64 (the softmax does not see a constant, and a float32 a_k keeps more of log w_k without it)."""
    w, mu, v = np.asarray(w, np.float64), np.asarray(mu, np.float64), np.asarray(v, np.float64)
    a = -0.5 * (mu * mu / v).sum(axis=1) - 0.5 * np.log(v).sum(axis=1)
    if mistake != "no_log_w":
        a = a + np.log(w)
    return a, mu / v, -0.5 / v


def shift(d):
    return -0.5 * d * LOG_2PI


def abc_f32(w, mu, v):
    return tuple(np.ascontiguousarray(t, dtype=np.float32) for t in abc_f64(w, mu, v))


# ------------------------------------------------------------------------------------------------- the contract
def em_step_f64(X, y, a, B, C, sw=None, mistake=None):
    """One E-step and the M-step's sufficient statistics in float64: ll, nk [k], s1 [k, d], s2 [k, d], pred (ties to the lowest
    component), info = [rows with y >= k, rows with a non-finite logit].  y None or int [n] (0 <= y_i < k clamps the row).  The hard
    M-step is em_hard_f64.  `mistake`: one of MISTAKES, planted."""
    X64 = np.asarray(X, np.float64)
    n, d = X64.shape
    a64, B64, C64 = np.asarray(a, np.float64), np.asarray(B, np.float64), np.asarray(C, np.float64)
    k = a64.shape[0]
    yy = np.full(n, -1, np.int64) if y is None else np.asarray(y, np.int64)
    s = np.ones(n) if sw is None else np.asarray(sw, np.float64).copy()
    lab = (yy >= 0) & (yy < k)
    yc = np.where(lab, yy, 0)
    X2 = X64 * X64
    z = (X64 @ C64.T + X2 @ B64.T if mistake == "slabs_swapped" else X64 @ B64.T + X2 @ C64.T) + a64[None, :]
    m = z.max(axis=1, keepdims=True)
    if mistake == "no_max_subtraction":
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(z.astype(np.float32)).astype(np.float64)                 # float32 exp of the raw logit
            m = np.zeros_like(m)
    else:
        e = np.exp(z - m)
    tot = e.sum(axis=1, keepdims=True)
    if mistake == "padding_in_sum":
        kp = -(-k // 32) * 32
        with np.errstate(over="ignore"):
            tot = tot + (kp - k) * np.exp(0.0 - m)                              # the padding logits are 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        lse = (m + np.log(tot))[:, 0]
        p = e / tot
    onehot = np.zeros((n, k))
    onehot[np.arange(n), yc] = lab
    zy = z[np.arange(n), yc]
    soft_rows = np.zeros(n, bool) if mistake != "labelled_softmax" else lab
    with np.errstate(invalid="ignore"):
        resp = np.where((lab & ~soft_rows)[:, None], onehot, p)
        r = s[:, None] * resp
        row = np.where(lab & (mistake != "labelled_lse"), zy, lse)
        rowll = np.where(s != 0, s * row, 0.0)
    keep = np.ones(n, bool)
    if mistake == "ragged_tile_dropped":
        keep[n // ROW_TILE * ROW_TILE:] = False
    plan = fp.gmm_plan(n, d, k)
    if mistake == "last_range_dropped":
        keep[(plan["R"] - 1) * plan["rows"]:] = False
    mult = keep.astype(np.float64)
    if mistake == "chain_row_twice" and n > CHAIN_ROWS:
        mult[CHAIN_ROWS - 1] = 2.0
    if mistake == "range_added_twice":
        mult[plan["rows"]:2 * plan["rows"]] = 2.0
    rm = r * mult[:, None]
    mult_cs = mult.copy()
    if mistake == "colsum_range_tail_dropped":                  # a column-sum range loses the rows past its last whole group of eight
        for lo, hi in fp.range_bounds(n, plan["RB"], plan["cs_rows"]):
            mult_cs[hi - (hi - lo) % fp.CS_GROUPS:hi] = 0.0
    nk = (resp * mult[:, None]).sum(axis=0) if mistake == "weight_ignored" else (r * mult_cs[:, None]).sum(axis=0)
    s1 = rm.T @ X64
    s2 = rm.T @ (X64 if mistake == "x_for_x2_in_s2" else X2)
    if mistake == "range_stride_of_one_tile":                   # every tile but the first reads range 0's partial R times
        first = (np.arange(k)[:, None] < fp.GT) & (np.arange(d)[None, :] < fp.GT)
        r0 = plan["R"] * r[:plan["rows"]].T
        s1, s2 = np.where(first, s1, r0 @ X64[:plan["rows"]]), np.where(first, s2, r0 @ X2[:plan["rows"]])
    pred = (k - 1 - np.argmax(z[:, ::-1], axis=1)) if mistake == "ties_to_highest" else np.argmax(z, axis=1)
    info = np.array([int((yy >= k).sum()), int((~np.isfinite(z)).any(axis=1).sum())])
    return dict(ll=float((rowll * keep).sum()), nk=nk, s1=s1, s2=s2, pred=pred.astype(np.int64), info=info, z=z, lse=lse, p=p, r=r, s=s,
                lab=lab, rowll=rowll)


def em_hard_f64(X, y, k, sw=None):
    """The hard M-step (a == B == C == NULL): one-hots of the rows with a label in [0, k), nothing else, ll = 0."""
    X64 = np.asarray(X, np.float64)
    n = X64.shape[0]
    yy = np.asarray(y, np.int64)
    s = np.ones(n) if sw is None else np.asarray(sw, np.float64)
    lab = (yy >= 0) & (yy < k)
    r = np.zeros((n, k))
    r[np.arange(n), np.where(lab, yy, 0)] = np.where(lab, s, 0.0)
    return dict(ll=0.0, nk=r.sum(axis=0), s1=r.T @ X64, s2=r.T @ (X64 * X64), info=np.array([int((yy >= k).sum()), 0]), r=r)


def top2_gap(z):
    if z.shape[1] == 1:
        return np.full(z.shape[0], np.inf)
    zs = np.sort(z, axis=1)
    return zs[:, -1] - zs[:, -2]


# ------------------------------------------------------------------------------------------------- the error model
def bounds(X, y, a, B, C, sw=None):
    """Per-quantity bounds of |device - float64| (docs/design/gmm.md): delta [n] for a logit, ll (scalar), nk [k], s1, s2 [k, d]; for
    scd_gmm_predict resp [n, k] and row_ll [n]."""
    ref = em_step_f64(X, y, a, B, C, sw)
    X64 = np.asarray(X, np.float64)
    n, d = X64.shape
    aa, BB, CC = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(B, np.float64)), np.abs(np.asarray(C, np.float64))
    k = aa.shape[0]
    AX, X2 = np.abs(X64), X64 * X64
    # a chain of 2 d fused multiply-adds and the final add of a_k: 2 d + 1 roundings on a term, one more on an x^2 term for its own
    # rounding; gamma_{2 d + 2} covers every term
    delta = gamma(2 * d + 2) * (AX @ BB.T + X2 @ CC.T + aa[None, :]).max(axis=1)
    eps = (k + 128) * 2.0 ** -23
    s, p, lab = ref["s"], ref["p"], ref["lab"]
    soft_b = p * np.expm1(2.0 * delta)[:, None] + eps * p + U * p + TINY
    r_b = np.where(lab[:, None], 0.0, s[:, None] * soft_b)                      # a labelled row's r is its weight, exactly
    row_b = np.where(lab, delta, 2.0 * delta + eps * (1.0 + np.abs(ref["lse"])))
    ar = np.abs(ref["r"])
    gT = gamma(CHAIN_ROWS)
    return dict(delta=delta, ll=float((s * row_b).sum()), nk=r_b.sum(axis=0) + gT * ar.sum(axis=0),
                s1=r_b.T @ AX + gT * (ar.T @ AX), s2=(1.0 + U) * (r_b.T @ X2) + gamma(CHAIN_ROWS + 1) * (ar.T @ X2),
                resp=soft_b, row_ll=2.0 * delta + eps * (1.0 + np.abs(ref["lse"])), gap=top2_gap(ref["z"]), ref=ref)


def decided_rows(bd, exact_ties=False):
    """Rows whose argmax the device must reproduce: top-two gap above 2 delta; with exact_ties also the rows whose two best logits are
    bit-equal on the device because two components are identical (gap exactly 0)."""
    dec = bd["gap"] > 2.0 * bd["delta"]
    return dec | (bd["gap"] == 0.0) if exact_ties else dec


def ratio(got, want, bound):
    """Largest |got - want| / bound; an exact value scores 0 whatever its bound, NaN counts as infinite."""
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
        q = np.where(err == 0, 0.0, err / np.asarray(bound, np.float64))
    return float(np.max(np.where(np.isnan(q), np.inf, q)))


def ratios(got, bd, keys=("ll", "nk", "s1", "s2")):
    return {key: ratio(got[key], bd["ref"][key], bd[key]) for key in keys if got.get(key) is not None}


def violates(got, bd, exact_ties=False):
    """True when `got` (ll, nk, s1, s2, pred) breaks a bound of the clean restatement or disagrees on a decided row."""
    if any(v > 1.0 for v in ratios(got, bd).values()):
        return True
    dec = decided_rows(bd, exact_ties)
    return bool(np.any(np.asarray(got["pred"])[dec] != bd["ref"]["pred"][dec]))


# ------------------------------------------------------------------------------------------------- cases
def mixture(n, d, k, seed, sep=None, vlo=0.3, vhi=1.5):
    """Rows drawn from a mixture of k diagonal Gaussians; the parameters the step is evaluated at are the true ones."""
    rng = np.random.default_rng(seed)
    if sep is None:
        sep = 1.0 if d >= 512 else min(1.0, 3.0 / np.sqrt(d))                   # small d: overlapping components, soft rows
    mu = sep * rng.standard_normal((k, d))
    v = np.exp(rng.uniform(np.log(vlo), np.log(vhi), (k, d)))
    w = rng.dirichlet(np.full(k, 5.0))
    z = rng.integers(0, k, n)
    X = (mu[z] + np.sqrt(v[z]) * rng.standard_normal((n, d))).astype(np.float32)
    a, B, C = abc_f32(w, mu, v)
    return dict(X=X, y=None, a=a, B=B, C=C, sw=None, exact_ties=False, hard=False, truth=z, logw=np.log(w), w=w, mu=mu, v=v)


def shapes():
    rt, T = ROW_TILE, CHAIN_ROWS
    return {"n1_d1_k1": (1, 1, 1), "ragged_tile": (rt - 1, 5, 3), "k33": (rt + 1, 64, 33), "d768_k100": (3 * rt + 7, 768, 100),
            "full_width": (2 * rt, 1024, 1024), "two_chains": (T + 1, 96, 31), "four_chains": (3 * T + 5, 33, 257),
            "two_ranges": (9 * T + 3, 33, 33),                  # R = 2 row ranges of several chains each in the moments
            # the forward kernel's NT = 2 and NT = 8 with phantom tiles, then the range plans (tests/f32mm_plan.py has each regime)
            **{name: shape for name, (shape, _) in fp.NT_CASES.items()},
            **{name: c["wide"] for name, c in fp.RANGE_CASES.items() if "wide" in c}}


VARIANTS = ("unlabelled", "mixed", "all_labelled", "hard", "weights", "bad_labels")
LARGE_VARIANTS = ("unlabelled", "weights", "hard")              # of the cases with n >= f32mm_plan.LARGE_N: the rest do not bear on the ranges
# chosen so that in every variant every row's top-two gap exceeds 2 delta (tests/test_gmm_host.py asserts it): no row is excused.  The
# cases with n >= f32mm_plan.LARGE_N keep the default seed and carry an undecided_cap instead: of 10^4 - 10^5 random rows one or two have
# a gap within 2 delta, and predictions do not depend on the ranges
SHAPE_SEEDS = {"n1_d1_k1": 2000, "ragged_tile": 2000, "k33": 2000, "d768_k100": 2000, "full_width": 2000, "two_chains": 2000,
               "four_chains": 2000, "two_ranges": 2000}


def variants_of(name, menu=None):
    return LARGE_VARIANTS if (menu or shapes())[name][0] >= fp.LARGE_N else VARIANTS


def _mixed_labels(case, rng):
    """A third of the rows labelled: most with the component they were drawn from, some with another (the clamp must still hold)."""
    n, k = case["X"].shape[0], case["a"].shape[0]
    y = np.full(n, -1, np.int32)
    pick = rng.random(n) < 1.0 / 3.0
    if n <= 2:
        pick[:] = True
    wrong = rng.random(n) < 0.25
    y[pick] = np.where(wrong, rng.integers(0, k, n), case["truth"])[pick]
    return y


def shape_case(name, variant="unlabelled"):
    n, d, k = shapes()[name]
    case = mixture(n, d, k, seed=SHAPE_SEEDS.get(name, 2000))
    case["undecided_cap"] = fp.undecided_cap(n)
    rng = np.random.default_rng(78)
    if variant in ("mixed", "hard", "weights", "bad_labels"):
        case["y"] = _mixed_labels(case, rng)
    if variant == "all_labelled":
        case["y"] = case["truth"].astype(np.int32)
    elif variant == "hard":
        case["hard"] = True
    elif variant == "weights":
        sw = rng.uniform(0.25, 2.0, n).astype(np.float32)
        sw[::3] = 0.0
        if n == 1:
            sw[:] = 0.75
        case["sw"] = sw
    elif variant == "bad_labels":                               # two more rows, labels k and k + 5: they count as unlabelled
        extra = mixture(2, d, k, seed=SHAPE_SEEDS.get(name, 2000))["X"]
        case["X"] = np.concatenate([case["X"][: n // 2], extra[:1], case["X"][n // 2:], extra[1:]])
        case["y"] = np.concatenate([case["y"][: n // 2], [k], case["y"][n // 2:], [k + 5]]).astype(np.int32)
        case["truth"] = np.concatenate([case["truth"][: n // 2], [0], case["truth"][n // 2:], [0]])
    elif variant not in ("unlabelled", "mixed"):
        raise KeyError(variant)
    return case


def bad_labels_as_unlabelled(case):
    out = dict(case)
    out["y"] = np.where(case["y"] >= case["a"].shape[0], -1, case["y"]).astype(np.int32)
    return out


def variance_span_case():
    """Variances from 1e-4 to 1 within every component: B and C span four decades."""
    case = mixture(100, 24, 12, seed=11, sep=1.0, vlo=1e-4, vhi=1.0)
    case["y"] = _mixed_labels(case, np.random.default_rng(12))
    return case


def far_rows_case():
    """Half of the rows lie 30 standard deviations from their component: logits of -7000, every exponential but one underflows, and
    a float32 exp of the raw logit is 0 on every component."""
    case = mixture(50, 16, 20, seed=13, sep=1.0)
    X = case["X"].astype(np.float64)
    z = case["truth"]
    X[::2] = case["mu"][z[::2]] + 30.0 * (X[::2] - case["mu"][z[::2]])
    case["X"] = X.astype(np.float32)
    return case


def identical_components_case():
    """Components 3 and 17 are identical and sit on the data's mean, so they tie for the maximum (bit-equal logits) on many rows and
    share their responsibilities equally."""
    case = mixture(90, 40, 35, seed=14)
    mu, v, w = case["mu"], case["v"], case["w"]
    mu[17] = mu[3] = case["X"].astype(np.float64).mean(axis=0)
    v[17] = v[3] = 1.5
    w[17] = w[3] = 0.2
    w /= w.sum()
    case["a"], case["B"], case["C"] = abc_f32(w, mu, v)
    case["logw"] = np.log(w)
    case["exact_ties"] = True
    return case


def unreached_component_case():
    """Component 5 is a tight Gaussian far from every row: its logit is below the row maximum by thousands, its e is exactly 0 in
    float32 and float64 alike, and its nk, s1 and s2 are exactly 0."""
    case = mixture(70, 12, 9, seed=15, sep=2.0)
    mu, v, w = case["mu"], case["v"], case["w"]
    mu[5] = 40.0
    v[5] = 0.05
    case["a"], case["B"], case["C"] = abc_f32(w, mu, v)
    case["unreached"] = 5
    return case


def least_likely_label_case():
    """Every third row is labelled with its LEAST likely component: the clamp must hold against the density."""
    case = mixture(80, 20, 7, seed=16, sep=1.0)
    z = em_step_f64(case["X"], None, case["a"], case["B"], case["C"])["z"]
    y = np.full(80, -1, np.int32)
    y[::3] = z.argmin(axis=1)[::3]
    case["y"] = y
    return case


def special_cases():
    return {"variance_span": variance_span_case(), "far_rows": far_rows_case(), "identical": identical_components_case(),
            "unreached": unreached_component_case(), "least_likely_label": least_likely_label_case()}


def all_cases():
    out = {}
    for name in shapes():
        for v in variants_of(name):
            out["%s-%s" % (name, v)] = shape_case(name, v)
    out.update(special_cases())
    return out


def reference(case):
    """The restatement's outputs for a case (the hard M-step where the case asks for it)."""
    if case["hard"]:
        return em_hard_f64(case["X"], case["y"], case["a"].shape[0], case["sw"])
    return em_step_f64(case["X"], case["y"], case["a"], case["B"], case["C"], case["sw"])


# planted mistake -> the named case on which it must exceed the bounds
MISTAKES = {
    "no_log_w": "k33-unlabelled",
    "slabs_swapped": "k33-unlabelled",
    "x_for_x2_in_s2": "k33-unlabelled",
    "padding_in_sum": "far_rows",
    "no_max_subtraction": "far_rows",
    "labelled_softmax": "least_likely_label",
    "labelled_lse": "least_likely_label",
    "weight_ignored": "d768_k100-weights",
    "ragged_tile_dropped": "ragged_tile-unlabelled",
    "chain_row_twice": "two_chains-unlabelled",
    "ties_to_highest": "identical",
    "last_range_dropped": "ranges_x_tiles-unlabelled",          # a last range of ONE row
    "range_added_twice": "cap32-unlabelled",
    "range_stride_of_one_tile": "ranges_x_tiles-unlabelled",
    "colsum_range_tail_dropped": "colsum_cap-unlabelled",
}
# the mistakes that must show on further cases as well
ALSO = [("padding_in_sum", "nt2_phantom-unlabelled"), ("padding_in_sum", "nt8_phantom-unlabelled")]
RANGE_MISTAKES = ("last_range_dropped", "range_added_twice", "range_stride_of_one_tile", "colsum_range_tail_dropped")


def mistake_cases():
    return list(MISTAKES.items()) + ALSO


def planted(case, mistake):
    """The restatement of a case with one mistake planted."""
    a = case["a"]
    if mistake == "no_log_w":
        a = (a.astype(np.float64) - case["logw"]).astype(np.float32)
    return em_step_f64(case["X"], case["y"], a, case["B"], case["C"], case["sw"], mistake=mistake)


# ------------------------------------------------------------------------------------------------- the M-step and the fit, restated
def m_step_f64(nk, s1, s2, covariance_type="diag", reg_covar=1e-6, mistake=None):
    """scikit-learn's _estimate_gaussian_parameters + the weights' normalisation from the sufficient statistics: (w [k], mu [k, d],
    covariances [k, d] for 'diag' or [k] for 'spherical')."""
    nk2 = np.asarray(nk, np.float64) + 10.0 * EPS64
    mu = s1 / nk2[:, None]
    if mistake == "reg_before_spherical_mean":                                  # reg_covar added, then the mean over d taken on mu^2 alone
        return nk2 / nk2.sum(), mu, (s2 / nk2[:, None] + reg_covar - (mu * mu).mean(axis=1, keepdims=True))[:, 0]
    cov = s2 / nk2[:, None] - mu * mu + reg_covar
    if covariance_type == "spherical":
        cov = cov.mean(axis=1)
    elif covariance_type != "diag":
        raise ValueError(covariance_type)
    return nk2 / nk2.sum(), mu, cov


def full_var(cov, d):
    cov = np.asarray(cov, np.float64)
    return cov if cov.ndim == 2 else np.repeat(cov[:, None], d, axis=1)


def n_parameters(k, d, covariance_type):
    return 2 * k * d + k - 1 if covariance_type == "diag" else k * d + 2 * k - 1


def fit_f64(X, w0, mu0, cov0, covariance_type="diag", tol=1e-3, reg_covar=1e-6, max_iter=100, y=None, float32_params=False):
    """scikit-learn's EM loop from an explicit start, in float64; float32_params evaluates every E-step at (a, B, C) rounded to
    float32, as the device does.  Labelled rows (y) are clamped.  Returns the parameters, n_iter, converged, lower_bound (the mean row
    log-likelihood of the last E-step of the loop), the trace, and the final E-step's labels, z and delta-free gap."""
    X64 = np.asarray(X, np.float64)
    n, d = X64.shape
    w, mu, cov = np.asarray(w0, np.float64), np.asarray(mu0, np.float64), np.asarray(cov0, np.float64)

    def e_step(w, mu, cov):
        a, B, C = abc_f64(w, mu, full_var(cov, d))
        if float32_params:
            a, B, C = a.astype(np.float32), B.astype(np.float32), C.astype(np.float32)
        return em_step_f64(X64, y, a, B, C), (a, B, C)

    lower, trace, converged, n_iter = -np.inf, [], False, 0
    for n_iter in range(1, max_iter + 1):
        prev = lower
        st, _ = e_step(w, mu, cov)
        lower = st["ll"] / n + shift(d)
        trace.append(lower)
        w, mu, cov = m_step_f64(st["nk"], st["s1"], st["s2"], covariance_type, reg_covar)
        if abs(lower - prev) < tol:
            converged = True
            break
    st, abc = e_step(w, mu, cov)
    return dict(w=w, mu=mu, cov=cov, n_iter=n_iter, converged=converged, lower_bound=lower, trace=trace, labels=st["pred"], final=st,
                abc=abc)


def bic_f64(fit, X, covariance_type):
    n, d = np.asarray(X).shape
    score = fit["final"]["lse"].mean() + shift(d)
    return -2.0 * score * n + n_parameters(fit["w"].shape[0], d, covariance_type) * np.log(n)


# (n, d, k, spread of the cluster scales, separation): blobs with unequal cluster scales, soft enough that top-two gaps are small
FIT_CASES = {"n1500_d16_k6": (1500, 16, 6, 1.1), "n2000_d32_k10": (2000, 32, 10, 0.9), "n1200_d8_k4": (1200, 8, 4, 1.3)}


# chosen so that, for both covariance types, no row's top-two gap at the final parameters is within 2 delta (tests/test_gmm_host.py
# asserts it)
FIT_SEEDS = {"n1500_d16_k6": 400, "n2000_d32_k10": 403, "n1200_d8_k4": 401}


def blob_case(name):
    """(X float32 [n, d], truth [n], (w0, mu0, cov0 diag [k, d])): blobs whose scales differ fourfold, and a start near the truth."""
    n, d, k, sep = FIT_CASES[name]
    rng = np.random.default_rng(FIT_SEEDS[name])
    centers = sep * rng.standard_normal((k, d))
    scale = np.linspace(0.5, 2.0, k)
    z = np.arange(n) % k
    rng.shuffle(z)
    X = (centers[z] + scale[z][:, None] * rng.standard_normal((n, d))).astype(np.float32)
    mu0 = centers + 0.3 * rng.standard_normal((k, d))
    return X, z, (np.full(k, 1.0 / k), mu0, np.ones((k, d)))


def start_for(start, covariance_type):
    """The explicit start in scikit-learn's form: (weights_init, means_init, precisions_init) and our (w0, mu0, cov0)."""
    w0, mu0, cov0 = start
    if covariance_type == "spherical":
        cov0 = cov0.mean(axis=1)
    return (w0, mu0, 1.0 / cov0), (w0, mu0, cov0)


def overlap_case():
    """Semi-supervised: four classes in d = 6, classes 0 and 1 overlap heavily (centres 1.2 sigma apart).  A third of the rows carry
    their label.  (X, truth, y with -1 on unlabelled rows, start)."""
    rng = np.random.default_rng(500)
    n, d, k = 900, 6, 4
    centers = 4.0 * rng.standard_normal((k, d))
    centers[1] = centers[0] + 1.2 / np.sqrt(d)
    z = np.arange(n) % k
    rng.shuffle(z)
    X = (centers[z] + rng.standard_normal((n, d))).astype(np.float32)
    y = np.where(np.arange(n) % 3 == 0, z, -1).astype(np.int32)
    mu0 = centers + 0.5 * rng.standard_normal((k, d))
    mu0[1], mu0[0] = mu0[0].copy(), mu0[1].copy()              # a start that has the two overlapping classes the wrong way round
    return X, z, y, (np.full(k, 1.0 / k), mu0, np.ones((k, d)))


def planted_k_case():
    """A cache-sized case for BIC: 400 rows, d = 8, five well-separated blobs; candidates 2 ... 8."""
    rng = np.random.default_rng(600)
    n, d, k = 400, 8, 5
    centers = 6.0 * rng.standard_normal((k, d))
    z = np.arange(n) % k
    X = (centers[z] + rng.standard_normal((n, d))).astype(np.float32)
    return X, z, k
