"""The full-covariance mixture's contract restated in float64 numpy (scd_gmm_full_em_step / scd_gmm_full_predict,
scd_amd/gmm_full.py), its error model, the cases and the planted mistakes.  docs/design/gmm_full.md derives the bounds.  Everything here is
evaluated at the SAME float32 X, a, mu, Ut the device receives, the centred rows c = fl32(x - mu) formed in float32 as the kernel forms
them, so the only difference a test sees is the device's rounding."""
import numpy as np

import f32mm_plan as fp
from gmm_cases import EPS64, TINY, U, _mixed_labels, decided_rows, gamma, ratio, shift, top2_gap, variants_of  # noqa: F401

ROW_TILE = 32                                   # scd_gmm_full_row_tile(); the host test asserts the library agrees
CHAIN_ROWS = 256                                # scd_gmm_full_chain_rows()
MAX_D = 64


# ------------------------------------------------------------------------------------------------- parameters
def chol_t(cov):
    """Ut = L^-1 with cov = L L^T, float64 [..., d, d]: the transpose of scikit-learn's precisions_cholesky_, exact zeros above the
    diagonal."""
    return np.tril(np.linalg.inv(np.linalg.cholesky(np.asarray(cov, np.float64))))


def params_f64(w, mu, cov, mistake=None):
    """(a [k], mu [k, d], Ut [k, d, d]) in float64 from weights, means and covariances ([k, d, d], or [d, d] tied), a WITHOUT the
    constant -(d / 2) log 2 pi (shift(d) holds it)."""
    w, mu, cov = np.asarray(w, np.float64), np.asarray(mu, np.float64), np.asarray(cov, np.float64)
    k, d = mu.shape
    ut = chol_t(cov)
    if ut.ndim == 2:
        ut = np.broadcast_to(ut, (k, d, d)).copy()
    a = np.log(w)
    if mistake != "no_log_det":
        a = a + np.log(np.diagonal(ut, axis1=1, axis2=2)).sum(axis=1)
    return a, mu, ut


def params_f32(w, mu, cov):
    return tuple(np.ascontiguousarray(t, dtype=np.float32) for t in params_f64(w, mu, cov))


def centred(X, mu):
    """c [n, k, d] float64.  float32 means: c = fl32(x - mu), one IEEE subtraction, as the kernel forms it; float64 means (the pure
    float64 loop that is compared with scikit-learn): the float64 difference."""
    mu = np.asarray(mu)
    if mu.dtype == np.float32:
        return (np.asarray(X, np.float32)[:, None, :] - mu[None, :, :]).astype(np.float64)
    return np.asarray(X, np.float64)[:, None, :] - mu[None, :, :]


def _weighted_outer(wgt, c, c2=None):
    """sum_i wgt_ik c_ikj c2_ikl -> [k, d, d]."""
    c2 = c if c2 is None else c2
    return np.matmul((wgt[:, :, None] * c).transpose(1, 2, 0), c2.transpose(1, 0, 2))


# ------------------------------------------------------------------------------------------------- the contract
def em_step_f64(X, y, a, mu, Ut, sw=None, mistake=None):
    """One E-step and the M-step's sufficient statistics about mu in float64: ll, nk [k], s1c [k, d], S [k, d, d], pred (ties to the
    lowest component), info = [rows with y >= k, rows with a non-finite logit].  `mistake`: one of MISTAKES, planted."""
    X64 = np.asarray(X, np.float64)
    n, d = X64.shape
    a64, U64 = np.asarray(a, np.float64), np.asarray(Ut, np.float64)
    k = a64.shape[0]
    yy = np.full(n, -1, np.int64) if y is None else np.asarray(y, np.int64)
    s = np.ones(n) if sw is None else np.asarray(sw, np.float64).copy()
    lab = (yy >= 0) & (yy < k)
    yc = np.where(lab, yy, 0)
    c = centred(X, mu)
    cz = centred(X, np.roll(np.asarray(mu), 1, axis=0)) if mistake == "mu_of_wrong_component" else c
    # y_ikj = sum_l c_ikl U_k[l][j] = sum_l c_ikl Ut[k][j][l]
    Uop = U64 if mistake == "u_untransposed" else U64.transpose(0, 2, 1)
    yv = np.matmul(cz.transpose(1, 0, 2), Uop)                                  # [k, n, j]
    if mistake == "second_j_tile_dropped":
        yv = yv[:, :, :32]
    q = (yv * yv).sum(axis=2).T                                                 # [n, k]
    z = a64[None, :] - (1.0 if mistake == "no_half" else 0.5) * q
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    tot = e.sum(axis=1, keepdims=True)
    if mistake == "padding_in_sum":
        kp = -(-k // 32) * 32
        with np.errstate(over="ignore"):
            tot = tot + (kp - k) * np.exp(0.0 - m)                              # a padding component's logit is 0
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
        rowll = np.where(s != 0, s * np.where(lab, zy, lse), 0.0)
    keep = np.ones(n, bool)
    if mistake == "ragged_tile_dropped":
        keep[n // ROW_TILE * ROW_TILE:] = False
    plan = fp.gmm_full_plan(n, d, k)
    if mistake == "last_range_dropped":
        keep[(plan["R"] - 1) * plan["rows"]:] = False
    mult = keep.astype(np.float64)
    if mistake == "chain_row_twice" and n > CHAIN_ROWS:
        mult[CHAIN_ROWS - 1] = 2.0
    if mistake == "range_added_twice":
        mult[plan["rows"]:2 * plan["rows"]] = 2.0
    rm = r * mult[:, None]
    st = _moments(rm, c, X64, mult, mistake)
    if mistake == "colsum_range_tail_dropped":                  # a column-sum range loses the rows past its last whole group of eight
        mult_cs = mult.copy()
        for lo, hi in fp.range_bounds(n, plan["RB"], plan["cs_rows"]):
            mult_cs[hi - (hi - lo) % fp.CS_GROUPS:hi] = 0.0
        st["nk"] = (r * mult_cs[:, None]).sum(axis=0)
    if mistake == "range_stride_of_one_tile":                   # every moment block but the first reads range 0's partial R times
        rows = plan["rows"]
        alt = _moments(plan["R"] * rm[:rows], c[:rows], X64[:rows])
        st["S"][fp.GMMF_CG:], st["s1c"][fp.GMMF_CG:] = alt["S"][fp.GMMF_CG:], alt["s1c"][fp.GMMF_CG:]
    if mistake == "second_j_tile_first_chain_only":             # the accumulators of the second j-tile carried into float64 once
        alt = _moments(rm[:CHAIN_ROWS], c[:CHAIN_ROWS], X64[:CHAIN_ROWS])
        st["S"][:, 32:, :], st["S"][:, :, 32:], st["s1c"][:, 32:] = alt["S"][:, 32:, :], alt["S"][:, :, 32:], alt["s1c"][:, 32:]
    info = np.array([int((yy >= k).sum()), int((~np.isfinite(z)).any(axis=1).sum())])
    st.update(ll=float((rowll * keep).sum()), pred=np.argmax(z, axis=1).astype(np.int64), info=info, z=z, lse=lse, p=p, r=r, s=s, lab=lab,
              rowll=rowll, c=c, y=yv, q=q)
    return st


def _moments(rm, c, X64, mult=None, mistake=None):
    if mistake == "r_missing_from_S":
        S = _weighted_outer(np.broadcast_to(mult[:, None], rm.shape), c)
    elif mistake == "S_about_zero":
        S = _weighted_outer(rm, np.broadcast_to(X64[:, None, :], c.shape))
    else:
        S = _weighted_outer(rm, c)
    if mistake == "upper_triangle_only":
        S = np.triu(S)
    return dict(nk=rm.sum(axis=0), s1c=np.einsum("ik,ikj->kj", rm, c), S=S)


def em_hard_f64(X, y, mu, sw=None):
    """The hard M-step (a == Ut == NULL) about the centres mu: one-hots of the rows with a label in [0, k), nothing else, ll = 0."""
    X64 = np.asarray(X, np.float64)
    n, k = X64.shape[0], np.asarray(mu).shape[0]
    yy = np.asarray(y, np.int64)
    s = np.ones(n) if sw is None else np.asarray(sw, np.float64)
    lab = (yy >= 0) & (yy < k)
    r = np.zeros((n, k))
    r[np.arange(n), np.where(lab, yy, 0)] = np.where(lab, s, 0.0)
    c = centred(X, mu)
    st = _moments(r, c, X64)
    st.update(ll=0.0, info=np.array([int((yy >= k).sum()), 0]), r=r, c=c, s=s, lab=lab)
    return st


# ------------------------------------------------------------------------------------------------- the error model
def bounds(case):
    """Per-quantity bounds of |device - float64| (docs/design/gmm_full.md): delta [n] for a logit, ll (scalar), nk [k], s1c [k, d],
    S [k, d, d]; for scd_gmm_full_predict resp [n, k] and row_ll [n].  A hard case has the chain terms alone."""
    X, y, sw = case["X"], case["y"], case["sw"]
    gT, gT1 = gamma(CHAIN_ROWS), gamma(CHAIN_ROWS + 1)
    if case["hard"]:
        ref = em_hard_f64(X, y, case["mu"], sw)
        ar, ac = np.abs(ref["r"]), np.abs(ref["c"])
        return dict(ref=ref, ll=0.0, nk=gT * ar.sum(axis=0), s1c=gT * np.einsum("ik,ikj->kj", ar, ac), S=gT1 * _weighted_outer(ar, ac))
    a, mu, Ut = case["a"], case["mu"], case["Ut"]
    ref = em_step_f64(X, y, a, mu, Ut, sw)
    n, d = np.asarray(X).shape
    k = a.shape[0]
    ac = np.abs(ref["c"])
    # y_j: a chain of at most d fused multiply-adds from zero (the skipped and the padding products are exact zeros)
    Y = np.matmul(ac.transpose(1, 0, 2), np.abs(np.asarray(Ut, np.float64)).transpose(0, 2, 1))         # [k, n, j]
    e = gamma(d) * Y
    ay = np.abs(ref["y"])
    # q: each square carries y's error; the d squares and their sum, in any order, are at most d + 1 roundings on a term; d + 2 charged
    dq = ((2.0 * ay * e + e * e).sum(axis=2) + gamma(d + 2) * ((ay + e) ** 2).sum(axis=2)).T          # [n, k]
    # z = fl(a - 0.5 q): one rounding of the result
    dz = 0.5 * dq + U * (np.abs(np.asarray(a, np.float64))[None, :] + 0.5 * (ref["q"] + dq))
    delta = dz.max(axis=1)
    eps = (k + 128) * 2.0 ** -23
    s, p, lab = ref["s"], ref["p"], ref["lab"]
    soft_b = p * np.expm1(2.0 * delta)[:, None] + eps * p + U * p + TINY
    r_b = np.where(lab[:, None], 0.0, s[:, None] * soft_b)                      # a labelled row's r is its weight, exactly
    row_b = np.where(lab, delta, 2.0 * delta + eps * (1.0 + np.abs(ref["lse"])))
    ar = np.abs(ref["r"])
    return dict(delta=delta, ll=float((s * row_b).sum()), nk=r_b.sum(axis=0) + gT * ar.sum(axis=0),
                s1c=np.einsum("ik,ikj->kj", r_b, ac) + gT * np.einsum("ik,ikj->kj", ar, ac),
                # A = fl(r c_j) is one more rounding than the chain's T
                S=(1.0 + gT1) * _weighted_outer(r_b, ac) + gT1 * _weighted_outer(ar, ac),
                resp=soft_b, row_ll=2.0 * delta + eps * (1.0 + np.abs(ref["lse"])), gap=top2_gap(ref["z"]), ref=ref)


KEYS = ("ll", "nk", "s1c", "S")


def ratios(got, bd, keys=KEYS):
    return {key: ratio(got[key], bd["ref"][key], bd[key]) for key in keys if got.get(key) is not None}


def violates(got, bd, exact_ties=False):
    """True when `got` (ll, nk, s1c, S, pred) breaks a bound of the clean restatement or disagrees on a decided row."""
    if any(v > 1.0 for v in ratios(got, bd).values()):
        return True
    dec = decided_rows(bd, exact_ties)
    return bool(np.any(np.asarray(got["pred"])[dec] != bd["ref"]["pred"][dec]))


# ------------------------------------------------------------------------------------------------- cases
def random_covariances(rng, k, d, slo, shi):
    """k covariances Q diag(s^2) Q^T: a random rotation each, standard deviations log-uniform in [slo, shi]; also (Q, s)."""
    Q = np.stack([np.linalg.qr(rng.standard_normal((d, d)))[0] for _ in range(k)])
    sd = np.exp(rng.uniform(np.log(slo), np.log(shi), (k, d)))
    return np.matmul(Q * (sd * sd)[:, None, :], Q.transpose(0, 2, 1)), Q, sd


def mixture(n, d, k, seed, sep=None, slo=0.55, shi=1.25):
    """Rows drawn from a mixture of k rotated Gaussians; the parameters the step is evaluated at are the true ones."""
    rng = np.random.default_rng(seed)
    if sep is None:
        sep = min(1.0, 3.0 / np.sqrt(d))                                        # overlapping components: soft rows
    mu = sep * rng.standard_normal((k, d))
    cov, Q, sd = random_covariances(rng, k, d, slo, shi)
    w = rng.dirichlet(np.full(k, 5.0))
    z = rng.integers(0, k, n)
    X = (mu[z] + np.einsum("ijl,il->ij", Q[z], sd[z] * rng.standard_normal((n, d)))).astype(np.float32)
    a, m32, Ut = params_f32(w, mu, cov)
    return dict(X=X, y=None, a=a, mu=m32, Ut=Ut, sw=None, exact_ties=False, hard=False, truth=z, logw=np.log(w), w=w, mu64=mu, cov=cov)


def set_params(case, w, mu, cov):
    case["a"], case["mu"], case["Ut"] = params_f32(w, mu, cov)
    case.update(w=w, mu64=mu, cov=cov, logw=np.log(w))


def shapes():
    rt, T = ROW_TILE, CHAIN_ROWS
    return {"n1_d1_k1": (1, 1, 1), "ragged_tile": (rt - 1, 5, 3), "one_j_tile": (rt + 1, 32, 33), "ragged_j_tile": (3 * rt + 7, 33, 5),
            "full_width": (2 * rt, 64, 1024), "two_chains": (T + 1, 24, 31), "four_chains": (3 * T + 5, 8, 257),
            "ranges": (9 * T + 3, 17, 9),                       # several row ranges of several chains each in the moments
            # JT = 2 across chains, then the range plans (tests/f32mm_plan.py has each regime)
            **{name: c["full"] for name, c in fp.RANGE_CASES.items()}}


VARIANTS = ("unlabelled", "mixed", "all_labelled", "hard", "weights", "bad_labels")
# chosen so that in every variant every row's top-two gap exceeds 2 delta (tests/test_gmm_full_host.py asserts it): no row is excused.  The
# cases with n >= f32mm_plan.LARGE_N run in gmm_cases.LARGE_VARIANTS, keep the default seed and carry an undecided_cap instead
SHAPE_SEEDS = {"n1_d1_k1": 2000, "ragged_tile": 2000, "one_j_tile": 2000, "ragged_j_tile": 2000, "full_width": 2000, "two_chains": 2000,
               "four_chains": 2000, "ranges": 2000}


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


def condition_case():
    """Standard deviations from 1e-2 to 1 within every component: covariances with condition numbers up to 1e4."""
    case = mixture(100, 24, 12, seed=11, sep=1.0, slo=1e-2, shi=1.0)
    case["y"] = _mixed_labels(case, np.random.default_rng(12))
    return case


def far_rows_case():
    """Half of the rows lie 30 standard deviations from their component: logits of -7000, every exponential but one underflows."""
    case = mixture(50, 16, 20, seed=13, sep=1.0)
    X = case["X"].astype(np.float64)
    z = case["truth"]
    X[::2] = case["mu64"][z[::2]] + 30.0 * (X[::2] - case["mu64"][z[::2]])
    case["X"] = X.astype(np.float32)
    return case


def identical_components_case():
    """Components 3 and 17 are identical and sit on the data's mean, so they tie for the maximum (bit-equal logits) on many rows and
    share their responsibilities equally."""
    case = mixture(90, 40, 35, seed=14)
    mu, cov, w = case["mu64"], case["cov"], case["w"]
    mu[17] = mu[3] = case["X"].astype(np.float64).mean(axis=0)
    cov[17] = cov[3] = 0.8 * np.eye(40) + 0.02
    w[17] = w[3] = 0.3
    w /= w.sum()
    set_params(case, w, mu, cov)
    case["exact_ties"] = True
    return case


def unreached_component_case():
    """Component 5 is a tight Gaussian far from every row: its e is exactly 0 in float32 and float64 alike, and its nk, s1c and S are
    exactly 0."""
    case = mixture(70, 12, 9, seed=15, sep=2.0)
    mu, cov, w = case["mu64"], case["cov"], case["w"]
    mu[5] = 40.0
    cov[5] = 0.05 * np.eye(12)
    set_params(case, w, mu, cov)
    case["unreached"] = 5
    return case


def least_likely_label_case():
    """Every third row is labelled with its LEAST likely component: the clamp must hold against the density."""
    case = mixture(80, 20, 7, seed=16, sep=1.0)
    z = em_step_f64(case["X"], None, case["a"], case["mu"], case["Ut"])["z"]
    y = np.full(80, -1, np.int32)
    y[::3] = z.argmin(axis=1)[::3]
    case["y"] = y
    return case


def special_cases():
    return {"condition_1e4": condition_case(), "far_rows": far_rows_case(), "identical": identical_components_case(),
            "unreached": unreached_component_case(), "least_likely_label": least_likely_label_case()}


def all_cases():
    out = {}
    for name in shapes():
        for v in variants_of(name, shapes()):
            out["%s-%s" % (name, v)] = shape_case(name, v)
    out.update(special_cases())
    return out


def reference(case):
    """The restatement's outputs for a case (the hard M-step where the case asks for it)."""
    if case["hard"]:
        return em_hard_f64(case["X"], case["y"], case["mu"], case["sw"])
    return em_step_f64(case["X"], case["y"], case["a"], case["mu"], case["Ut"], case["sw"])


# planted mistake of the kernel -> the named case on which it must exceed the bounds
MISTAKES = {
    "u_untransposed": "one_j_tile-unlabelled",
    "no_log_det": "one_j_tile-unlabelled",
    "no_half": "one_j_tile-unlabelled",
    "mu_of_wrong_component": "one_j_tile-unlabelled",
    "second_j_tile_dropped": "ragged_j_tile-unlabelled",
    "r_missing_from_S": "one_j_tile-unlabelled",
    "S_about_zero": "one_j_tile-unlabelled",
    "upper_triangle_only": "one_j_tile-unlabelled",
    "chain_row_twice": "two_chains-unlabelled",
    "ragged_tile_dropped": "ragged_tile-unlabelled",
    "padding_in_sum": "far_rows",
    "labelled_softmax": "least_likely_label",
    "last_range_dropped": "ranges_x_tiles-unlabelled",          # a last range of ONE row
    "range_added_twice": "cap32-unlabelled",
    "range_stride_of_one_tile": "ranges_x_tiles-unlabelled",
    "colsum_range_tail_dropped": "colsum_cap-unlabelled",
    "second_j_tile_first_chain_only": "jt2_chains-unlabelled",
}
RANGE_MISTAKES = ("last_range_dropped", "range_added_twice", "range_stride_of_one_tile", "colsum_range_tail_dropped",
                  "second_j_tile_first_chain_only")
# planted mistakes of the M-step: shown against scikit-learn's parameters (tests/test_gmm_full_host.py)
M_STEP_MISTAKES = ("cross_term_sign", "reg_off_diagonal", "tied_over_k")


def planted(case, mistake):
    """The restatement of a case with one mistake planted."""
    a = case["a"]
    if mistake == "no_log_det":
        a = params_f64(case["w"], case["mu64"], case["cov"], mistake=mistake)[0].astype(np.float32)
    return em_step_f64(case["X"], case["y"], a, case["mu"], case["Ut"], case["sw"], mistake=mistake)


# ------------------------------------------------------------------------------------------------- the M-step and the fit, restated
def m_step_f64(nk, s1c, S, m, covariance_type="full", reg_covar=1e-6, mistake=None):
    """scikit-learn's _estimate_gaussian_parameters + the weights' normalisation from the statistics about the means m: (w [k],
    mu [k, d], covariances [k, d, d] for 'full' or [d, d] for 'tied')."""
    nk, m = np.asarray(nk, np.float64), np.asarray(m, np.float64)
    k, d = m.shape
    nk2 = nk + 10.0 * EPS64
    mu = (s1c + nk[:, None] * m) / nk2[:, None]
    delta = mu - m
    cross = np.einsum("kj,kl->kjl", delta, s1c)
    cross = cross + cross.transpose(0, 2, 1)
    scat = S + (cross if mistake == "cross_term_sign" else -cross) + nk[:, None, None] * np.einsum("kj,kl->kjl", delta, delta)
    reg = reg_covar * (np.ones((d, d)) if mistake == "reg_off_diagonal" else np.eye(d))
    if covariance_type == "full":
        cov = scat / nk2[:, None, None] + reg[None]
    elif covariance_type == "tied":
        cov = scat.sum(axis=0) / (k if mistake == "tied_over_k" else nk2.sum()) + reg
    else:
        raise ValueError(covariance_type)
    return nk2 / nk2.sum(), mu, cov


def n_parameters(k, d, covariance_type):
    return (k if covariance_type == "full" else 1) * d * (d + 1) // 2 + k * d + k - 1


def fit_f64(X, w0, mu0, cov0, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, y=None, float32_params=False):
    """scikit-learn's EM loop from an explicit start, in float64; float32_params evaluates every E-step at (a, mu, Ut) rounded to
    float32 with c = fl32(x - mu), as the device does.  Labelled rows (y) are clamped.  Returns the parameters, n_iter, converged,
    lower_bound (the mean row log-likelihood of the last E-step of the loop), the trace, and the final E-step's labels and statistics."""
    X32 = np.asarray(X, np.float32)
    n, d = X32.shape
    w, mu, cov = np.asarray(w0, np.float64), np.asarray(mu0, np.float64), np.asarray(cov0, np.float64)

    def e_step(w, mu, cov):
        prm = params_f64(w, mu, cov)
        if float32_params:
            prm = tuple(t.astype(np.float32) for t in prm)
        return em_step_f64(X32, y, *prm), prm

    lower, trace, converged, n_iter = -np.inf, [], False, 0
    for n_iter in range(1, max_iter + 1):
        prev = lower
        st, prm = e_step(w, mu, cov)
        lower = st["ll"] / n + shift(d)
        trace.append(lower)
        w, mu, cov = m_step_f64(st["nk"], st["s1c"], st["S"], prm[1], covariance_type, reg_covar)
        if abs(lower - prev) < tol:
            converged = True
            break
    st, prm = e_step(w, mu, cov)
    return dict(w=w, mu=mu, cov=cov, n_iter=n_iter, converged=converged, lower_bound=lower, trace=trace, labels=st["pred"], final=st,
                params=prm)


def bic_f64(fit, X, covariance_type):
    n, d = np.asarray(X).shape
    score = fit["final"]["lse"].mean() + shift(d)
    return -2.0 * score * n + n_parameters(fit["w"].shape[0], d, covariance_type) * np.log(n)


def as_case(X, params, y=None):
    """A case dict (for bounds) from rows and float32 kernel parameters."""
    a, mu, Ut = params
    return dict(X=np.asarray(X, np.float32), y=y, a=a, mu=mu, Ut=Ut, sw=None, exact_ties=False, hard=False)


# (n, d, k, separation): blobs with rotated, elongated covariances, soft enough that top-two gaps are small.  d stays at 8 or below
# here: the likelihood bound over n grows with d (2.4e-4 at d = 8, 6e-4 at d = 16) and the stopping rule can only be pinned where twice
# that bound is well below tol = 1e-3; the wider kernels are covered by the step cases
FIT_CASES = {"n1500_d6_k6": (1500, 6, 6, 1.6), "n2000_d4_k5": (2000, 4, 5, 1.8), "n1200_d8_k4": (1200, 8, 4, 1.3)}
# chosen so that, for both covariance types, no row's top-two gap at the final parameters is within 2 delta and the last two changes of
# the lower bound are further from tol than twice the likelihood bound over n (tests/test_gmm_full_host.py asserts it)
FIT_SEEDS = {"n1500_d6_k6": 614, "n2000_d4_k5": 413, "n1200_d8_k4": 443}


def blob_case(name):
    """(X float32 [n, d], truth [n], (w0, mu0, cov0 [k, d, d])): blobs with a random rotation and standard deviations from 0.5 to 2
    each, and a start near the truth with unit covariances."""
    n, d, k, sep = FIT_CASES[name]
    rng = np.random.default_rng(FIT_SEEDS[name])
    centers = sep * rng.standard_normal((k, d))
    _, Q, sd = random_covariances(rng, k, d, 0.5, 2.0)
    z = np.arange(n) % k
    rng.shuffle(z)
    X = (centers[z] + np.einsum("ijl,il->ij", Q[z], sd[z] * rng.standard_normal((n, d)))).astype(np.float32)
    mu0 = centers + 0.3 * rng.standard_normal((k, d))
    return X, z, (np.full(k, 1.0 / k), mu0, np.broadcast_to(np.eye(d), (k, d, d)).copy())


def start_for(start, covariance_type):
    """The explicit start in scikit-learn's form: (weights_init, means_init, precisions_init) and our (w0, mu0, cov0)."""
    w0, mu0, cov0 = start
    if covariance_type == "tied":
        cov0 = cov0.mean(axis=0)
    return (w0, mu0, np.linalg.inv(cov0)), (w0, mu0, cov0)


def rotated_classes_case(seed=0):
    """Four classes of 400 rows in d = 8: a random rotation each, axis scales (1, 0.5, 0.05, ..., 0.05), means 0.3 N(0, I).  Only a
    covariance matrix per class tells them apart."""
    rng = np.random.default_rng(seed)
    k, per, d = 4, 400, 8
    sd = np.array([1.0, 0.5] + [0.05] * (d - 2))
    rows, z = [], []
    for j in range(k):
        Q = np.linalg.qr(rng.standard_normal((d, d)))[0]
        rows.append(0.3 * rng.standard_normal(d) + (sd * rng.standard_normal((per, d))) @ Q.T)
        z += [j] * per
    return np.concatenate(rows).astype(np.float32), np.array(z), k


def overlap_case():
    """Semi-supervised: four classes in d = 6, classes 0 and 1 share a centre region and differ by their elongation.  A third of the
    rows carry their label.  (X, truth, y with -1 on unlabelled rows, start)."""
    rng = np.random.default_rng(500)
    n, d, k = 900, 6, 4
    centers = 4.0 * rng.standard_normal((k, d))
    centers[1] = centers[0] + 1.2 / np.sqrt(d)
    _, Q, sd = random_covariances(rng, k, d, 0.6, 1.6)
    z = np.arange(n) % k
    rng.shuffle(z)
    X = (centers[z] + np.einsum("ijl,il->ij", Q[z], sd[z] * rng.standard_normal((n, d)))).astype(np.float32)
    y = np.where(np.arange(n) % 3 == 0, z, -1).astype(np.int32)
    mu0 = centers + 0.5 * rng.standard_normal((k, d))
    mu0[1], mu0[0] = mu0[0].copy(), mu0[1].copy()              # a start that has the two overlapping classes the wrong way round
    return X, z, y, (np.full(k, 1.0 / k), mu0, np.broadcast_to(np.eye(d), (k, d, d)).copy())


def planted_k_case():
    """A cache-sized case for BIC: 400 rows, d = 8, five well-separated rotated blobs; candidates 2 ... 8."""
    rng = np.random.default_rng(600)
    n, d, k = 400, 8, 5
    centers = 6.0 * rng.standard_normal((k, d))
    _, Q, sd = random_covariances(rng, k, d, 0.4, 1.6)
    z = np.arange(n) % k
    X = (centers[z] + np.einsum("ijl,il->ij", Q[z], sd[z] * rng.standard_normal((n, d)))).astype(np.float32)
    return X, z, k
