"""CPU checks of the linear probe's restatement (tests/probe_cases.py), its error model, the planted mistakes, the float64 L-BFGS against
scikit-learn, the ABI and score_features.py's split.  docs/design/probe.md has the rules."""
import os
import re

import numpy as np
import pytest

import f32mm_plan as fp
import probe_cases as pc

GIB = 1 << 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = pc.all_cases()


@pytest.fixture(autouse=True)
def needs_the_probe():
    from scd_amd import _lib
    assert "scd_probe_loss_grad" in _lib.SIGNATURES, "the library under test has no linear probe: these cases restate its contract"


@pytest.fixture(scope="module")
def L():
    from scd_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["c33-base", "d768_c100-weights", "two_chains-no_bias", "four_chains-bad_labels", "large_logit", "ties"])
def test_restatement_against_an_independent_formula(name):
    from scipy.special import logsumexp
    case = CASES[name]
    X, W = case["X"].astype(np.float64), case["W"].astype(np.float64)
    n, c = X.shape[0], W.shape[0]
    y = case["y"].astype(np.int64)
    ok = (y >= 0) & (y < c)
    s = (np.ones(n) if case["sw"] is None else case["sw"].astype(np.float64)) * ok
    z = X @ W.T + (0 if case["b"] is None else case["b"].astype(np.float64))
    Y = np.zeros((n, c))
    Y[np.flatnonzero(ok), y[ok]] = 1.0
    lse = logsumexp(z, axis=1)
    loss = float(s @ (lse - (z * Y).sum(axis=1)))
    R = s[:, None] * (np.exp(z - lse[:, None]) - Y)
    got = pc.loss_grad_f64(case["X"], case["y"], case["W"], case["b"], case["sw"])
    assert abs(got["loss"] - loss) <= 1e-12 * max(abs(loss), 1e-300)
    assert np.abs(got["gW"] - R.T @ X).max() <= 1e-12 * np.abs(R.T @ X).max()
    assert np.abs(got["gb"] - R.sum(axis=0)).max() <= 1e-12 * max(np.abs(R).sum(axis=0).max(), 1e-300)
    assert got["info"][0] == int((~ok).sum()) and got["info"][1] == 0


def test_restatement_gradient_is_the_derivative_of_its_loss():
    case = pc.shape_case("c33", "weights")
    X, y, sw = case["X"], case["y"], case["sw"]
    W, b = case["W"].astype(np.float64), case["b"].astype(np.float64)
    ref = pc.loss_grad_f64(X, y, W, b, sw)
    rng = np.random.default_rng(0)
    h = 1e-5
    for _ in range(12):
        ci, di = rng.integers(0, W.shape[0]), rng.integers(0, W.shape[1])
        Wp, Wm = W.copy(), W.copy()
        Wp[ci, di] += h
        Wm[ci, di] -= h
        fd = (pc.loss_grad_f64(X, y, Wp, b, sw)["loss"] - pc.loss_grad_f64(X, y, Wm, b, sw)["loss"]) / (2 * h)
        assert abs(fd - ref["gW"][ci, di]) <= 1e-6 * max(1.0, abs(fd))
        bp, bm = b.copy(), b.copy()
        bp[ci] += h
        bm[ci] -= h
        fd = (pc.loss_grad_f64(X, y, W, bp, sw)["loss"] - pc.loss_grad_f64(X, y, W, bm, sw)["loss"]) / (2 * h)
        assert abs(fd - ref["gb"][ci]) <= 1e-6 * max(1.0, abs(fd))


def test_special_cases_are_what_they_claim():
    ll = pc.loss_grad_f64(**{k: CASES["large_logit"][k] for k in ("X", "y", "W", "b", "sw")})
    assert ll["z"].max() > 299 and ll["z"].min() < -299
    m = ll["z"].max(axis=1, keepdims=True)
    assert (np.exp((ll["z"] - m).astype(np.float32)) == 0).mean() > 0.5      # most e are 0 in float32
    ae = CASES["all_equal"]
    r = pc.loss_grad_f64(ae["X"], ae["y"], ae["W"], ae["b"])
    n, c = ae["X"].shape[0], ae["W"].shape[0]
    assert abs(r["loss"] - n * np.log(c)) < 1e-9 and (r["pred"] == 0).all()
    t = CASES["ties"]
    bd = pc.bounds(t["X"], t["y"], t["W"], t["b"])
    assert ((bd["gap"] == 0) & (bd["ref"]["pred"] == 3)).sum() >= 30        # rows 3 and 17 of W tie for the maximum


@pytest.mark.parametrize("name", list(CASES))
def test_no_row_is_excused_outside_the_tie_cases(name):
    case = CASES[name]
    bd = pc.bounds(case["X"], case["y"], case["W"], case["b"], case["sw"])
    dec = pc.decided_rows(bd, case["exact_ties"])
    cap = case.get("undecided_cap", 0.0)                        # 0 below f32mm_plan.LARGE_N rows: no row is excused there
    assert cap == (fp.UNDECIDED_CAP if case["X"].shape[0] >= fp.LARGE_N else 0.0)
    if name == "ties":
        assert dec.all()                                        # the tied rows are decided exactly, the others by their gap
    else:
        assert (~dec).mean() <= cap, "rows %s have a top-two gap within 2 delta" % np.flatnonzero(~dec)


@pytest.mark.parametrize("variant", ["weights", "no_bias", "bad_labels"])
def test_variants_differ_only_where_they_should(variant):
    base, case = pc.shape_case("c33"), pc.shape_case("c33", variant)
    if variant == "bad_labels":
        got = pc.loss_grad_f64(case["X"], case["y"], case["W"], case["b"])
        assert list(got["info"]) == [2, 0] and sorted(case["y"][(case["y"] < 0) | (case["y"] >= 33)]) == [-1, 33]
        clean = pc.without_bad_rows(case)
        assert np.array_equal(clean["X"], base["X"]) and np.array_equal(clean["y"], base["y"])
        want = pc.loss_grad_f64(base["X"], base["y"], base["W"], base["b"])
        assert abs(got["loss"] - want["loss"]) <= 1e-12 * want["loss"] and np.allclose(got["gW"], want["gW"], rtol=0, atol=1e-12)
    elif variant == "weights":
        assert (case["sw"] == 0).any() and (case["sw"] > 0).any()
    else:
        assert case["b"] is None


# ------------------------------------------------------------------------------------------------- the bounds see the mistakes
@pytest.mark.parametrize("mistake,on", pc.mistake_cases(), ids=[m if (m, on) in pc.MISTAKES.items() else "%s-%s" % (m, on) for m, on in pc.mistake_cases()])
def test_every_planted_mistake_exceeds_the_bounds(mistake, on):
    case = CASES[on]
    bd = pc.bounds(case["X"], case["y"], case["W"], case["b"], case["sw"])
    clean = pc.loss_grad_f64(case["X"], case["y"], case["W"], case["b"], case["sw"])
    assert not pc.violates(clean, bd, case["exact_ties"])
    wrong = pc.loss_grad_f64(case["X"], case["y"], case["W"], case["b"], case["sw"], mistake=mistake)
    print("planted %-26s on %-22s: difference / bound %s" % (mistake, on, {k: "%.3g" % v for k, v in pc.ratios(wrong, bd).items()}))
    assert pc.violates(wrong, bd, case["exact_ties"]), "%s goes unseen on %s" % (mistake, on)
    if mistake in ("last_range_dropped", "range_added_twice", "range_stride_of_one_tile", "colsum_range_tail_dropped"):
        assert any(v > 1.0 for v in pc.ratios(wrong, bd).values())              # a sum breaks its bound, not a prediction


def test_bounds_leave_little_room():
    """The bounds are those of float32 arithmetic over d = 768 terms: a relative error of 1e-3 in any output is outside them."""
    case = CASES["d768_c100-base"]
    bd = pc.bounds(case["X"], case["y"], case["W"], case["b"])
    ref = bd["ref"]
    assert bd["loss"] < 1e-3 * abs(ref["loss"])
    assert np.median(bd["gW"] / np.maximum(np.abs(ref["r"]).T @ np.abs(case["X"].astype(np.float64)), 1e-300)) < 1e-3


# ------------------------------------------------------------------------------------------------- the fit against scikit-learn
@pytest.mark.parametrize("name", list(pc.FIT_CASES))
def test_lbfgs_restatement_against_sklearn(name):
    from sklearn.linear_model import LogisticRegression
    X, y, C = pc.blob_case(name)
    lam = 1.0 / C
    sk = LogisticRegression(C=C, tol=1e-10, max_iter=20000).fit(X.astype(np.float64), y)
    F_sk = pc.objective_f64(X, y, sk.coef_, sk.intercept_, lam)[0]
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                         # at tol = 1e-9 the last steps may sit at float64's own noise floor
        fit = pc.fit_f64(X, y, C=C, tol=1e-9, max_iter=20000)
    F = pc.objective_f64(X, y, fit["W"], fit["b"], lam)[0]
    print("%s: F %.15g, scikit-learn %.15g, relative difference %.2e, %d iterations, %d evaluations, max |g| %.2e"
          % (name, F, F_sk, abs(F - F_sk) / F_sk, fit["n_iter"], fit["n_eval"], np.abs(fit["g"]).max()))
    assert abs(F - F_sk) <= 1e-9 * F_sk
    assert np.array_equal(sk.classes_, np.arange(pc.FIT_CASES[name][2]))


@pytest.mark.parametrize("name", list(pc.FIT_CASES))
def test_float32_evaluation_excuses_no_prediction(name):
    """The fit as the device runs it (parameters rounded to float32 at every evaluation, tol = 1e-4) predicts what scikit-learn does on
    every row whose scikit-learn margin exceeds 2 delta_i + |dW|_rowmax |x_i| + |db|; on these cases that is every row."""
    from sklearn.linear_model import LogisticRegression
    X, y, C = pc.blob_case(name)
    sk = LogisticRegression(C=C, tol=1e-10, max_iter=20000).fit(X.astype(np.float64), y)
    fit = pc.fit_f64(X, y, C=C, tol=1e-4, float32_params=True)
    assert fit["converged"]
    excused, wrong = pc.prediction_check(X, sk.coef_, sk.intercept_, fit["W"].astype(np.float32), fit["b"].astype(np.float32),
                                         pc.loss_grad_f64(X, y, fit["W"].astype(np.float32), fit["b"].astype(np.float32))["pred"])
    assert excused == 0 and wrong == 0


# ------------------------------------------------------------------------------------------------- ABI, limits, the split
def test_abi_declares_the_probe(L):
    from scd_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "scd_hip.h")).read()
    for sym in ("scd_probe_ws_bytes", "scd_probe_row_tile", "scd_probe_chain_rows", "scd_probe_loss_grad", "scd_probe_predict"):
        assert sym in _lib.SIGNATURES and re.search(r"\b%s\(" % sym, hdr) and hasattr(L, sym)
    assert L.scd_probe_row_tile() == pc.ROW_TILE and L.scd_probe_chain_rows() == pc.CHAIN_ROWS <= 1024


def test_workspace_limits(L):
    nb = L.scd_probe_ws_bytes(126976, 768, 1000)
    print("scd_probe workspace at 126,976 x 768, c = 1000: %.1f MB" % (nb / 1e6))
    assert 0 < nb <= 2 * GIB
    assert L.scd_probe_ws_bytes(1, 1, 2) > 0 and L.scd_probe_ws_bytes(10, 1024, 1024) > 0
    for n, d, c in ((0, 8, 4), (1 << 31, 8, 4), (10, 0, 4), (10, 1025, 4), (10, 8, 1), (10, 8, 1025)):
        assert L.scd_probe_ws_bytes(n, d, c) == 0


def test_split_is_deterministic_and_stratified():
    import score_features as sf
    rng = np.random.default_rng(3)
    t = rng.integers(0, 7, 500) * 3 - 4                         # labels need not be 0 .. c-1
    t[:4] = 99                                                  # a class of 4 rows: no validation row
    train, val = sf.stratified_split(t)
    train2, val2 = pc.stratified_split(t)
    assert np.array_equal(train, train2) and np.array_equal(val, val2) and np.array_equal(train, ~val)
    assert np.array_equal(sf.stratified_split(t)[1], val)
    for cls in np.unique(t):
        rows = np.flatnonzero(t == cls)
        assert np.array_equal(np.flatnonzero(val[rows]), np.arange(4, rows.size, 5))
    assert not val[t == 99].any() and val.sum() == sum(np.sum(t == cls) // 5 for cls in np.unique(t))
