"""The linear probe's contract restated in float64 numpy (scd_probe_loss_grad / scd_probe_predict, scd_amd/probe.py), its error model,
the cases and the planted mistakes.  docs/design/probe.md derives the bounds.  Everything here is evaluated at the SAME float32 X, W, b
the device receives, so the only difference a test sees is the device's rounding."""
import warnings

import numpy as np

import f32mm_plan as fp

U = 2.0 ** -24                                  # unit roundoff of float32
TINY = 2.0 ** -126                              # smallest normal float32: the absolute floor of an underflowing e (docs/design/probe.md)
ROW_TILE = 32                                   # scd_probe_row_tile(); the host test asserts the library agrees
CHAIN_ROWS = 256                                # scd_probe_chain_rows()


def gamma(k):
    return k * U / (1.0 - k * U)


def logsumexp_rows(z):
    m = z.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))[:, 0]


# ------------------------------------------------------------------------------------------------- the contract
def loss_grad_f64(X, y, W, b=None, sw=None, mistake=None):
    """The data term sum_i s_i [lse(z_i) - z_{i, y_i}], gW = r^T X, gb = column sums of r, pred (ties to the lowest class) and info =
    [rows with a label outside [0, c), rows with a non-finite logit] in float64.  `mistake`: one of MISTAKES, planted."""
    X64, W64 = np.asarray(X, np.float64), np.asarray(W, np.float64)
    n, d = X64.shape
    c = W64.shape[0]
    y = np.asarray(y, np.int64)
    b64 = np.zeros(c) if b is None else np.asarray(b, np.float64)
    s = np.ones(n) if (sw is None or mistake == "weight_ignored") else np.asarray(sw, np.float64).copy()
    ok = (y >= 0) & (y < c)
    s = np.where(ok, s, 0.0)
    yy = np.where(ok, y, 0)
    z = X64 @ W64.T + (0.0 if mistake == "no_bias" else b64[None, :])
    m = z.max(axis=1, keepdims=True)
    if mistake == "no_max_subtraction":
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(z.astype(np.float32)).astype(np.float64)                 # float32 exp of the raw logit: overflows past 88.7
            m = np.zeros_like(m)
    else:
        e = np.exp(z - m)
    tot = e.sum(axis=1, keepdims=True)
    if mistake == "padding_in_sum":
        cp = -(-c // 32) * 32
        tot = tot + (cp - c) * np.exp(0.0 - m)                                  # the padding logits are 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        lse = (m + np.log(tot))[:, 0]
        p = e / tot
    onehot = np.zeros((n, c))
    onehot[np.arange(n), yy] = ok
    zy = z[np.arange(n), yy]
    with np.errstate(invalid="ignore"):
        rowloss = np.where(s != 0, s * (lse - zy), 0.0)
        r = s[:, None] * p - onehot if mistake == "onehot_before_weight" else s[:, None] * (p - onehot)
    keep = np.ones(n, bool)
    if mistake == "ragged_tile_dropped":
        keep[n // ROW_TILE * ROW_TILE:] = False
    plan = fp.probe_plan(n, d, c)
    if mistake == "last_range_dropped":
        keep[(plan["R"] - 1) * plan["rows"]:] = False
    mult = keep.astype(np.float64)
    if mistake == "chain_row_twice" and n > CHAIN_ROWS:
        mult[CHAIN_ROWS - 1] = 2.0
    if mistake == "range_added_twice":
        mult[plan["rows"]:2 * plan["rows"]] = 2.0
    loss = float((rowloss * keep).sum())
    gW = (r * mult[:, None]).T @ X64
    if mistake == "range_stride_of_one_tile":                   # every tile but the first reads range 0's partial R times
        first = (np.arange(c)[:, None] < fp.GT) & (np.arange(d)[None, :] < fp.GT)
        gW = np.where(first, gW, plan["R"] * (r[:plan["rows"]].T @ X64[:plan["rows"]]))
    keep_cs = keep.copy()
    if mistake == "colsum_range_tail_dropped":                  # a column-sum range loses the rows past its last whole group of eight
        for lo, hi in fp.range_bounds(n, plan["RB"], plan["cs_rows"]):
            keep_cs[hi - (hi - lo) % fp.CS_GROUPS:hi] = False
    gb = ((p - onehot) * ok[:, None] * keep[:, None]).sum(axis=0) if mistake == "gb_unweighted" else (r * keep_cs[:, None]).sum(axis=0)
    pred = (c - 1 - np.argmax(z[:, ::-1], axis=1)) if mistake == "ties_to_highest" else np.argmax(z, axis=1)
    info = np.array([int((~ok).sum()), int((~np.isfinite(z)).any(axis=1).sum())])
    return dict(loss=loss, gW=gW, gb=gb, pred=pred.astype(np.int64), info=info, z=z, lse=lse, p=p, r=r, s=s, ok=ok)


def top2_f64(z):
    zs = np.sort(z, axis=1)
    return zs[:, -1], zs[:, -2]


# ------------------------------------------------------------------------------------------------- the error model
def bounds(X, y, W, b=None, sw=None):
    """Per-quantity bounds of |device - float64| (docs/design/probe.md): delta [n] for a logit, loss (scalar), gW [c, d], gb [c]."""
    ref = loss_grad_f64(X, y, W, b, sw)
    X64, W64 = np.asarray(X, np.float64), np.asarray(W, np.float64)
    n, d = X64.shape
    c = W64.shape[0]
    ab = np.zeros(c) if b is None else np.abs(np.asarray(b, np.float64))
    delta = gamma(d + 1) * (np.abs(X64) @ np.abs(W64).T + ab[None, :]).max(axis=1)
    eps = (c + 128) * 2.0 ** -23
    s, p = ref["s"], ref["p"]
    onehot = np.zeros((n, c))
    onehot[np.arange(n), np.where(ref["ok"], np.asarray(y, np.int64), 0)] = ref["ok"]
    loss_b = float((s * (2.0 * delta + eps * (1.0 + np.abs(ref["lse"])))).sum())
    # the residual: the logit error moves p by e^{2 delta}, the softmax stage by eps, the one rounding of r by u; e below the smallest
    # normal float32 may come out as 0 (an absolute TINY, which the relative terms cannot cover: `most e are 0` in the large-logit case)
    res_b = s[:, None] * (p * np.expm1(2.0 * delta)[:, None] + eps * p + U * np.abs(p - onehot) + TINY)
    gW_b = res_b.T @ np.abs(X64) + gamma(CHAIN_ROWS) * (np.abs(ref["r"]).T @ np.abs(X64))
    gb_b = res_b.sum(axis=0) + gamma(CHAIN_ROWS) * np.abs(ref["r"]).sum(axis=0)
    t1, t2 = top2_f64(ref["z"])
    return dict(delta=delta, loss=loss_b, gW=gW_b, gb=gb_b, gap=t1 - t2, ref=ref)


def decided_rows(bd, exact_ties=False):
    """Rows whose argmax the device must reproduce: top-two gap above 2 delta; with exact_ties also the rows whose two best logits are
    bit-equal on the device because two rows of W (and of b) are (gap exactly 0)."""
    dec = bd["gap"] > 2.0 * bd["delta"]
    return dec | (bd["gap"] == 0.0) if exact_ties else dec


def ratios(got, bd):
    """Largest |got - float64| / bound per quantity; NaN counts as infinite."""
    ref = bd["ref"]
    out = {}
    for key in ("loss", "gW", "gb"):
        if got.get(key) is None:
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(np.asarray(got[key], np.float64) - ref[key])
            q = np.where(err == 0, 0.0, err / np.asarray(bd[key]))
        out[key] = float(np.max(np.where(np.isnan(q), np.inf, q)))
    return out


def violates(got, bd, exact_ties=False):
    """True when `got` (loss, gW, gb, pred) breaks a bound of the clean restatement or disagrees on a decided row."""
    if any(v > 1.0 for v in ratios(got, bd).values()):
        return True
    dec = decided_rows(bd, exact_ties)
    return bool(np.any(np.asarray(got["pred"])[dec] != bd["ref"]["pred"][dec]))


# ------------------------------------------------------------------------------------------------- cases
def _unit(a):
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-30)


def base_case(n, d, c, seed, scale=6.0):
    """Unit rows, W of row norm `scale` (logits of a few units), a bias, labels that follow the logits half of the time."""
    rng = np.random.default_rng(seed)
    X = _unit(rng.standard_normal((n, d))).astype(np.float32)
    W = (scale * _unit(rng.standard_normal((c, d)))).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    z = X.astype(np.float64) @ W.astype(np.float64).T + b
    y = np.where(rng.random(n) < 0.5, z.argmax(axis=1), rng.integers(0, c, n)).astype(np.int32)
    return dict(X=X, y=y, W=W, b=b, sw=None, exact_ties=False)


def shapes():
    rt, T = ROW_TILE, CHAIN_ROWS
    return {"n1_d1_c2": (1, 1, 2), "ragged_tile": (rt - 1, 5, 3), "c33": (rt + 1, 64, 33), "d768_c100": (3 * rt + 7, 768, 100),
            "full_width": (2 * rt, 1024, 1024), "two_chains": (T + 1, 96, 31), "four_chains": (3 * T + 5, 33, 257),
            "two_ranges": (9 * T + 3, 33, 33),                  # R = 2 row ranges of several chains each in the gradient
            # the forward kernel's NT = 2 and NT = 8 with phantom tiles, then the range plans (tests/f32mm_plan.py has each regime)
            **{name: shape for name, (shape, _) in fp.NT_CASES.items()},
            **{name: c["wide"] for name, c in fp.RANGE_CASES.items() if "wide" in c}}


VARIANTS = ("base", "weights", "no_bias", "bad_labels")
LARGE_VARIANTS = ("base", "weights")            # of the cases with n >= f32mm_plan.LARGE_N: the variants do not bear on the range plans
# chosen so that in every variant every row's top-two gap exceeds 2 delta (tests/test_probe_host.py asserts it): no row is excused.  The
# cases with n >= f32mm_plan.LARGE_N keep the default seed and carry an undecided_cap instead: of 10^4 - 10^5 random rows a few have a
# gap within 2 delta, and predictions do not depend on the ranges
SHAPE_SEEDS = {"n1_d1_c2": 1000, "ragged_tile": 1000, "c33": 1000, "d768_c100": 1002, "full_width": 1000, "two_chains": 1000,
               "four_chains": 1000, "two_ranges": 1000}


def variants_of(name):
    return LARGE_VARIANTS if shapes()[name][0] >= fp.LARGE_N else VARIANTS


def shape_case(name, variant="base"):
    n, d, c = shapes()[name]
    case = base_case(n, d, c, seed=SHAPE_SEEDS.get(name, 1000))
    case["undecided_cap"] = fp.undecided_cap(n)
    rng = np.random.default_rng(77)
    if variant == "weights":
        sw = rng.uniform(0.25, 2.0, n).astype(np.float32)
        sw[::3] = 0.0
        if n == 1:
            sw[:] = 0.75
        case["sw"] = sw
    elif variant == "no_bias":
        case["b"] = None
    elif variant == "bad_labels":                               # two more rows, labels -1 and c: the result is the base case's
        extra = _unit(rng.standard_normal((2, d))).astype(np.float32)
        case["X"] = np.concatenate([case["X"][: n // 2], extra[:1], case["X"][n // 2:], extra[1:]])
        case["y"] = np.concatenate([case["y"][: n // 2], [-1], case["y"][n // 2:], [c]]).astype(np.int32)
    elif variant != "base":
        raise KeyError(variant)
    return case


def without_bad_rows(case):
    keep = (case["y"] >= 0) & (case["y"] < case["W"].shape[0])
    out = dict(case)
    out["X"], out["y"] = case["X"][keep], case["y"][keep]
    return out


def large_logit_case():
    """Logits reach +-300: float32 exp(z) overflows without the max subtraction, most e underflow to 0 with it."""
    rng = np.random.default_rng(5)
    n, d, c = 40, 16, 50
    X = _unit(rng.standard_normal((n, d))).astype(np.float32)
    W = 300.0 * _unit(rng.standard_normal((c, d)))
    W[:20] = 300.0 * X[:20]
    W[20:40] = -300.0 * X[:20]
    W = W.astype(np.float32)
    y = rng.integers(0, c, n).astype(np.int32)
    y[:10] = np.arange(10)
    return dict(X=X, y=y, W=W, b=np.zeros(c, np.float32), sw=None, exact_ties=False)


def all_equal_case():
    """W = 0: every logit equal, argmax class 0 on every row, loss n log c."""
    case = base_case(70, 24, 37, seed=8)
    case["W"] = np.zeros_like(case["W"])
    case["b"] = np.zeros_like(case["b"])
    case["exact_ties"] = True
    return case


def tie_case():
    """Rows 3 and 17 of W (and of b) are identical and pulled towards the data, so they tie for the maximum on many rows."""
    case = base_case(90, 40, 35, seed=9)
    mean = _unit(case["X"].astype(np.float64).mean(axis=0, keepdims=True))[0]
    case["W"][17] = case["W"][3] = (case["W"][3] + 30.0 * mean).astype(np.float32)
    case["b"][17] = case["b"][3]
    case["exact_ties"] = True
    return case


def special_cases():
    return {"large_logit": large_logit_case(), "all_equal": all_equal_case(), "ties": tie_case()}


def all_cases():
    out = {}
    for name in shapes():
        for v in variants_of(name):
            out["%s-%s" % (name, v)] = shape_case(name, v)
    out.update(special_cases())
    return out


# planted mistake -> the named case on which it must exceed the bounds
MISTAKES = {
    "no_bias": "c33-base",
    "padding_in_sum": "c33-base",
    "no_max_subtraction": "large_logit",
    "weight_ignored": "d768_c100-weights",
    "ragged_tile_dropped": "ragged_tile-base",
    "onehot_before_weight": "c33-weights",
    "gb_unweighted": "c33-weights",
    "ties_to_highest": "ties",
    "chain_row_twice": "two_chains-base",
    "last_range_dropped": "ranges_x_tiles-base",                # a last range of ONE row
    "range_added_twice": "cap32-base",
    "range_stride_of_one_tile": "ranges_x_tiles-base",
    "colsum_range_tail_dropped": "colsum_cap-base",
}
# the mistakes that must show on further cases as well
ALSO = [("padding_in_sum", "nt2_phantom-base"), ("padding_in_sum", "nt8_phantom-base")]


def mistake_cases():
    return list(MISTAKES.items()) + ALSO


# ------------------------------------------------------------------------------------------------- the fit, restated
def objective_f64(X, y, W, b, lam, sw=None):
    """F = data term + lam / 2 |W|_F^2 and its gradient (gW, gb) in float64."""
    o = loss_grad_f64(X, y, W, b, sw)
    W64 = np.asarray(W, np.float64)
    return o["loss"] + 0.5 * lam * float((W64 * W64).sum()), o["gW"] + lam * W64, o["gb"]


def lbfgs_fit(evaluate, c, d, fit_intercept, wsum, tol=1e-4, max_iter=1000, memory=10):
    """scd_amd/probe.py's L-BFGS in numpy float64.  evaluate(W, b or None) -> (F, gW, gb or None).  Start at zero, Armijo backtracking
    from step 1 (F_new <= F + 1e-4 t g.p, halving), a pair (s, y) kept only when s.y > 1e-10 y.y, stop at max |grad| <= tol * wsum; a line
    search that cannot decrease F ends the fit with converged = False."""
    nw = c * d

    def ev(theta):
        W = theta[:nw].reshape(c, d)
        F, gW, gb = evaluate(W, theta[nw:] if fit_intercept else None)
        return F, np.concatenate([gW.ravel(), gb]) if fit_intercept else gW.ravel()

    theta = np.zeros(nw + (c if fit_intercept else 0))
    F, g = ev(theta)
    n_eval, n_iter, pairs, converged = 1, 0, [], False
    while True:
        if np.abs(g).max() <= tol * wsum:
            converged = True
            break
        if n_iter >= max_iter or n_eval >= max_iter:
            break
        q = g.copy()
        alphas = []
        for s_, y_, rho in reversed(pairs):
            a = rho * s_.dot(q)
            alphas.append(a)
            q -= a * y_
        if pairs:
            s_, y_, _ = pairs[-1]
            q *= s_.dot(y_) / y_.dot(y_)
        for (s_, y_, rho), a in zip(pairs, reversed(alphas)):
            q += (a - rho * y_.dot(q)) * s_
        p = -q
        gp = g.dot(p)
        if not gp < 0:
            pairs, p = [], -g
            gp = g.dot(p)
        t, done = 1.0, False
        while n_eval < max_iter and t > 2.0 ** -60:
            cand = theta + t * p
            Fn, gn = ev(cand)
            n_eval += 1
            if Fn <= F + 1e-4 * t * gp:
                done = True
                break
            t *= 0.5
        if not done:
            warnings.warn("the line search could not decrease the objective: the fit stops at the evaluation's noise floor")
            break
        s_, y_ = cand - theta, gn - g
        sy = s_.dot(y_)
        if sy > 1e-10 * y_.dot(y_):
            pairs.append((s_, y_, 1.0 / sy))
            pairs = pairs[-memory:]
        theta, F, g = cand, Fn, gn
        n_iter += 1
    W = theta[:nw].reshape(c, d)
    return dict(W=W, b=theta[nw:] if fit_intercept else None, F=F, g=g, n_iter=n_iter, n_eval=n_eval, converged=converged)


def fit_f64(X, y, C=1.0, fit_intercept=True, tol=1e-4, max_iter=1000, sw=None, float32_params=False):
    """The fit in float64; float32_params evaluates at the iterate rounded to float32, as the device does."""
    c, d, lam = int(np.max(y)) + 1, X.shape[1], 1.0 / C
    wsum = float(X.shape[0] if sw is None else np.sum(sw, dtype=np.float64))

    def evaluate(W, b):
        if float32_params:
            o = loss_grad_f64(X, y, W.astype(np.float32), None if b is None else b.astype(np.float32), sw)
            return o["loss"] + 0.5 * lam * float((W * W).sum()), o["gW"] + lam * W, o["gb"]
        return objective_f64(X, y, W, b, lam, sw)

    return lbfgs_fit(evaluate, c, d, fit_intercept, wsum, tol, max_iter)


FIT_CASES = {"n1500_c10": (1500, 64, 10, 1.0), "n3000_c33": (3000, 128, 33, 10.0), "n2000_c100": (2000, 96, 100, 1.0)}


# noise of the blobs around their centres: at these every row's scikit-learn margin clears the excuse of prediction_check with room
# (the float32-evaluation fit of tests/test_probe_host.py confirms it on the CPU)
BLOB_NOISE = {"n1500_c10": 1.5, "n3000_c33": 1.0, "n2000_c100": 1.5}


def blob_case(name):
    """Blobs with unit rows: (X float32 [n, d], y int32 [n], C)."""
    n, d, c, C = FIT_CASES[name]
    rng = np.random.default_rng(300 + sorted(FIT_CASES).index(name))
    centers = rng.standard_normal((c, d))
    y = (np.arange(n) % c).astype(np.int32)
    rng.shuffle(y)
    X = _unit(centers[y] + BLOB_NOISE[name] * rng.standard_normal((n, d))).astype(np.float32)
    return X, y, C


def prediction_check(X, W_ref, b_ref, W32, b32, pred):
    """(excused rows, wrong rows): a row is compared when the reference's top-two margin exceeds 2 delta_i + |dW|_rowmax |x_i| + |db|, the
    logit error at the float32 parameters plus what the coefficient difference can move a logit by."""
    X64, W_ref, W64 = np.asarray(X, np.float64), np.asarray(W_ref, np.float64), np.asarray(W32, np.float64)
    c, d = W64.shape
    b_ref = np.zeros(c) if b_ref is None else np.asarray(b_ref, np.float64)
    b64 = np.zeros(c) if b32 is None else np.asarray(b32, np.float64)
    z = X64 @ W_ref.T + b_ref
    t1, t2 = top2_f64(z)
    delta = gamma(d + 1) * (np.abs(X64) @ np.abs(W64).T + np.abs(b64)[None, :]).max(axis=1)
    thr = 2.0 * delta + np.linalg.norm(W64 - W_ref, axis=1).max() * np.linalg.norm(X64, axis=1) + np.abs(b64 - b_ref).max()
    dec = (t1 - t2) > thr
    return int((~dec).sum()), int((np.asarray(pred)[dec] != z.argmax(axis=1)[dec]).sum())


def stratified_split(targets, period=5, slot=4):
    """score_features.py's rule, restated: within each class, in row order, the rows whose within-class index is `slot` mod `period` are
    validation.  Returns (train mask, validation mask)."""
    targets = np.asarray(targets)
    val = np.zeros(targets.shape[0], bool)
    seen = {}
    for i, t in enumerate(targets.tolist()):
        k = seen.get(t, 0)
        val[i] = k % period == slot
        seen[t] = k + 1
    return ~val, val
