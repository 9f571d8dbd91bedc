"""CPU checks of the Gaussian mixture's restatement (tests/gmm_cases.py), its error model, the planted mistakes, the float64 EM against
scikit-learn, the clamped E-step, the ABI, and the arguments of the estimator and the three scripts.  docs/design/gmm.md has the rules."""
import os
import re

import numpy as np
import pytest

import f32mm_plan as fp
import gmm_cases as gc

GIB = 1 << 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = gc.all_cases()
SOFT = [n for n, c in CASES.items() if not c["hard"]]


@pytest.fixture(autouse=True)
def needs_the_mixture():
    from scd_amd import _lib
    assert "scd_gmm_em_step" in _lib.SIGNATURES, "the library under test has no Gaussian mixture: these cases restate its contract"


@pytest.fixture(scope="module")
def L():
    from scd_amd import _lib
    return _lib.load()


def _sk_params(case):
    """A scikit-learn GaussianMixture carrying a case's float64 parameters."""
    from sklearn.mixture import GaussianMixture
    from sklearn.mixture._gaussian_mixture import _compute_precision_cholesky
    sk = GaussianMixture(n_components=case["w"].shape[0], covariance_type="diag")
    sk.weights_, sk.means_, sk.covariances_ = case["w"], case["mu"], case["v"]
    sk.precisions_cholesky_ = _compute_precision_cholesky(case["v"], "diag")
    return sk


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["k33-unlabelled", "two_chains-unlabelled", "variance_span", "ragged_tile-unlabelled"])
def test_weighted_log_densities_are_scikit_learns(name):
    """a + x . B + x^2 . C (+ the constant) from the float64 parameters is _estimate_weighted_log_prob."""
    case = CASES[name]
    if name == "variance_span":
        case = gc.mixture(100, 24, 12, seed=11, sep=1.0, vlo=1e-4, vhi=1.0)
    X = case["X"].astype(np.float64)
    a, B, C = gc.abc_f64(case["w"], case["mu"], case["v"])
    z = gc.em_step_f64(X, None, a, B, C)["z"] + gc.shift(X.shape[1])
    want = _sk_params(case)._estimate_weighted_log_prob(X)
    assert np.abs(z - want).max() <= 1e-10 * np.abs(want).max()


@pytest.mark.parametrize("covariance_type", ["diag", "spherical"])
def test_m_step_is_scikit_learns(covariance_type):
    from sklearn.mixture._gaussian_mixture import _estimate_gaussian_parameters
    case = CASES["four_chains-unlabelled"]
    X = case["X"].astype(np.float64)
    st = gc.em_step_f64(X, None, case["a"], case["B"], case["C"])
    nk, mu, cov = _estimate_gaussian_parameters(X, st["p"], 1e-6, covariance_type)
    w, mu2, cov2 = gc.m_step_f64(st["nk"], st["s1"], st["s2"], covariance_type, 1e-6)
    assert np.abs(w - nk / nk.sum()).max() <= 1e-10 and np.abs(mu - mu2).max() <= 1e-10 and np.abs(cov - cov2).max() <= 1e-10
    assert cov2.shape == ((257, 33) if covariance_type == "diag" else (257,))
    if covariance_type == "spherical":                          # the planted M-step mistake is outside that tolerance
        bad = gc.m_step_f64(st["nk"], st["s1"], st["s2"], "spherical", 1e-6, mistake="reg_before_spherical_mean")[2]
        assert np.abs(bad - cov).max() > 1e-3


def test_an_empty_component_keeps_scikit_learns_result():
    from sklearn.mixture._gaussian_mixture import _estimate_gaussian_parameters
    case = CASES["unreached"]
    X = case["X"].astype(np.float64)
    st = gc.reference(case)
    j = case["unreached"]
    assert st["nk"][j] == 0.0 and not st["s1"][j].any() and not st["s2"][j].any()
    assert (st["z"].max(axis=1) - st["z"][:, j]).min() > 1000.0
    w, mu, cov = gc.m_step_f64(st["nk"], st["s1"], st["s2"], "diag", 1e-6)
    _, mu_sk, cov_sk = _estimate_gaussian_parameters(X, st["p"], 1e-6, "diag")
    assert not mu[j].any() and np.all(cov[j] == 1e-6) and np.array_equal(mu[j], mu_sk[j]) and np.array_equal(cov[j], cov_sk[j])


def test_special_cases_are_what_they_claim():
    v = CASES["variance_span"]["v"]
    assert v.min() < 2e-4 and v.max() > 0.5
    far = gc.reference(CASES["far_rows"])
    e32 = np.exp((far["z"] - far["z"].max(axis=1, keepdims=True)).astype(np.float32))
    assert ((e32 > 0).sum(axis=1)[::2] == 1).mean() > 0.7 and far["z"][::2].max() < -1000      # on most far rows one e survives
    t = CASES["identical"]
    bd = gc.bounds(t["X"], t["y"], t["a"], t["B"], t["C"])
    tied = (bd["gap"] == 0) & (bd["ref"]["pred"] == 3)
    assert tied.sum() >= 5 and np.array_equal(bd["ref"]["p"][:, 3], bd["ref"]["p"][:, 17])
    lab = CASES["least_likely_label"]
    r = gc.reference(lab)
    rows = np.flatnonzero(lab["y"] >= 0)
    assert (r["z"][rows, lab["y"][rows]] == r["z"][rows].min(axis=1)).all() and (r["r"][rows, lab["y"][rows]] == 1).all()


@pytest.mark.parametrize("name", SOFT)
def test_no_row_is_excused(name):
    case = CASES[name]
    bd = gc.bounds(case["X"], case["y"], case["a"], case["B"], case["C"], case["sw"])
    dec = gc.decided_rows(bd, case["exact_ties"])
    cap = case.get("undecided_cap", 0.0)                        # 0 below f32mm_plan.LARGE_N rows: no row is excused there
    assert cap == (fp.UNDECIDED_CAP if case["X"].shape[0] >= fp.LARGE_N else 0.0)
    assert (~dec).mean() <= cap, "rows %s have a top-two gap within 2 delta" % np.flatnonzero(~dec)


def test_variants_differ_only_where_they_should():
    k = 33
    bad = gc.shape_case("k33", "bad_labels")
    got = gc.reference(bad)
    assert list(got["info"]) == [2, 0] and sorted(bad["y"][bad["y"] >= k]) == [k, k + 5]
    want = gc.reference(gc.bad_labels_as_unlabelled(bad))
    assert got["ll"] == want["ll"] and np.array_equal(got["s1"], want["s1"]) and list(want["info"]) == [0, 0]
    w = gc.shape_case("k33", "weights")
    assert (w["sw"] == 0).any() and (w["sw"] > 0).any() and (w["y"] >= 0).any() and (w["y"] < 0).any()
    hard = gc.shape_case("two_ranges", "hard")
    h = gc.reference(hard)
    assert h["ll"] == 0.0 and h["nk"].sum() == (hard["y"] >= 0).sum() and set(np.unique(h["r"])) == {0.0, 1.0}
    al = gc.shape_case("k33", "all_labelled")
    assert (al["y"] >= 0).all()


# ------------------------------------------------------------------------------------------------- the bounds see the mistakes
@pytest.mark.parametrize("mistake,on", gc.mistake_cases(), ids=[m if (m, on) in gc.MISTAKES.items() else "%s-%s" % (m, on) for m, on in gc.mistake_cases()])
def test_every_planted_mistake_exceeds_the_bounds(mistake, on):
    case = CASES[on]
    bd = gc.bounds(case["X"], case["y"], case["a"], case["B"], case["C"], case["sw"])
    assert not gc.violates(gc.reference(case), bd, case["exact_ties"])
    wrong = gc.planted(case, mistake)
    print("planted %-26s on %-26s: difference / bound %s" % (mistake, on, {k: "%.3g" % v for k, v in gc.ratios(wrong, bd).items()}))
    assert gc.violates(wrong, bd, case["exact_ties"]), "%s goes unseen on %s" % (mistake, on)
    if mistake in gc.RANGE_MISTAKES:
        assert any(v > 1.0 for v in gc.ratios(wrong, bd).values())              # a sum breaks its bound, not a prediction


def test_bounds_are_those_the_design_note_quotes():
    """delta is about 0.3 at d = 768 and 1e-3 at d = 64; numpy float32 products are a few hundred times inside it."""
    for name, lo, hi in (("d768_k100-unlabelled", 0.1, 0.6), ("k33-unlabelled", 3e-4, 3e-3)):
        case = CASES[name]
        bd = gc.bounds(case["X"], None, case["a"], case["B"], case["C"])
        X = case["X"]
        z32 = (X @ case["B"].T + (X * X) @ case["C"].T + case["a"]).astype(np.float64)
        err = np.abs(z32 - bd["ref"]["z"]).max(axis=1)
        print("%s: delta %.3g, float32 numpy logits off by %.3g" % (name, bd["delta"].max(), err.max()))
        assert lo < bd["delta"].max() < hi and (err < bd["delta"]).all()


# ------------------------------------------------------------------------------------------------- the fit against scikit-learn
@pytest.mark.parametrize("covariance_type", ["diag", "spherical"])
@pytest.mark.parametrize("name", list(gc.FIT_CASES))
def test_em_restatement_against_sklearn(name, covariance_type):
    from sklearn.mixture import GaussianMixture
    X, _, start = gc.blob_case(name)
    (wi, mi, pi), (w0, mu0, c0) = gc.start_for(start, covariance_type)
    X64 = X.astype(np.float64)
    sk = GaussianMixture(n_components=len(wi), covariance_type=covariance_type, weights_init=wi, means_init=mi, precisions_init=pi).fit(X64)
    fit = gc.fit_f64(X, w0, mu0, c0, covariance_type)
    print("%s %s: %d iterations, lower bound %.12g (scikit-learn %.12g)" % (name, covariance_type, fit["n_iter"], fit["lower_bound"], sk.lower_bound_))
    assert sk.converged_ and fit["converged"] and fit["n_iter"] == sk.n_iter_
    assert abs(fit["lower_bound"] - sk.lower_bound_) <= 1e-9 * abs(sk.lower_bound_)
    assert np.array_equal(fit["labels"], sk.predict(X64))
    assert np.abs(fit["cov"] - sk.covariances_).max() <= 1e-9 and fit["cov"].shape == sk.covariances_.shape
    # bic and aic, with the free-parameter counts written out
    k, d = mi.shape
    assert gc.n_parameters(k, d, covariance_type) == sk._n_parameters() == (2 * k * d + k - 1 if covariance_type == "diag" else k * d + 2 * k - 1)
    bic = gc.bic_f64(fit, X, covariance_type)
    assert abs(bic - sk.bic(X64)) <= 1e-9 * abs(bic)
    aic = bic - gc.n_parameters(k, d, covariance_type) * (np.log(X.shape[0]) - 2.0)
    assert abs(aic - sk.aic(X64)) <= 1e-9 * abs(aic)
    # the soft part of the claim: these blobs have rows the mixture is unsure of
    assert (fit["final"]["p"].max(axis=1) < 0.99).sum() >= 100


@pytest.mark.parametrize("covariance_type", ["diag", "spherical"])
@pytest.mark.parametrize("name", list(gc.FIT_CASES))
def test_float32_parameters_change_neither_iterations_nor_labels(name, covariance_type):
    """The loop as the device runs it (a, B, C rounded to float32 at every E-step): the same n_iter and labels, and at its final
    parameters no row's top-two gap is within 2 delta, so the device test excuses no row."""
    X, _, start = gc.blob_case(name)
    _, (w0, mu0, c0) = gc.start_for(start, covariance_type)
    f64 = gc.fit_f64(X, w0, mu0, c0, covariance_type)
    f32 = gc.fit_f64(X, w0, mu0, c0, covariance_type, float32_params=True)
    assert f32["converged"] and f32["n_iter"] == f64["n_iter"] and np.array_equal(f32["labels"], f64["labels"])
    a, B, C = f32["abc"]
    bd = gc.bounds(X, None, a, B, C)
    assert gc.decided_rows(bd).all()


# ------------------------------------------------------------------------------------------------- the clamped E-step
def test_all_rows_labelled_gives_the_class_conditional_moments():
    case = gc.shape_case("two_chains", "all_labelled")
    X, y = case["X"].astype(np.float64), case["y"]
    st = gc.reference(case)
    w, mu, cov = gc.m_step_f64(st["nk"], st["s1"], st["s2"], "diag", 0.0)
    for j in range(case["a"].shape[0]):
        rows = X[y == j]
        assert st["nk"][j] == len(rows)
        if len(rows):
            assert np.abs(mu[j] - rows.mean(axis=0)).max() <= 1e-12 and np.abs(cov[j] - rows.var(axis=0)).max() <= 1e-12
    assert abs(st["ll"] - st["z"][np.arange(len(y)), y].sum()) <= 1e-9 * abs(st["ll"])
    hard = gc.em_hard_f64(case["X"], y, case["a"].shape[0])
    assert np.array_equal(hard["nk"], st["nk"]) and np.array_equal(hard["s1"], st["s1"]) and np.array_equal(hard["s2"], st["s2"])


def test_semi_supervised_fit_helps_where_two_classes_overlap():
    X, z, y, start = gc.overlap_case()
    _, (w0, mu0, c0) = gc.start_for(start, "diag")
    unsup = gc.fit_f64(X, w0, mu0, c0, "diag", float32_params=True)
    semi = gc.fit_f64(X, w0, mu0, c0, "diag", y=y, float32_params=True)
    assert unsup["converged"] and semi["converged"]
    # the complete-data likelihood (clamped rows at their class) is nondecreasing over the iterations
    assert (np.diff(semi["trace"]) >= -1e-12).all() and (np.diff(unsup["trace"]) >= -1e-12).all()
    rest = y < 0
    acc_u, acc_s = (unsup["labels"][rest] == z[rest]).mean(), (semi["labels"][rest] == z[rest]).mean()
    print("accuracy on the unlabelled rows: unsupervised %.3f, semi-supervised %.3f" % (acc_u, acc_s))
    assert acc_s >= acc_u and acc_s > 0.8
    a, B, C = semi["abc"]
    assert gc.decided_rows(gc.bounds(X, None, a, B, C)).all()


def test_bic_finds_the_planted_k_with_scikit_learn():
    """The cache of the device test: scikit-learn's own k-means-started mixture has its lowest BIC at the planted K on unit rows."""
    from sklearn.mixture import GaussianMixture
    X, _, k = gc.planted_k_case()
    U = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float64)
    bic = {K: GaussianMixture(n_components=K, covariance_type="diag", random_state=0).fit(U).bic(U) for K in range(2, 9)}
    assert min(bic, key=bic.get) == k


# ------------------------------------------------------------------------------------------------- ABI, limits, arguments
def test_abi_declares_the_mixture(L):
    from scd_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "scd_hip.h")).read()
    for sym in ("scd_gmm_ws_bytes", "scd_gmm_row_tile", "scd_gmm_chain_rows", "scd_gmm_em_step", "scd_gmm_predict"):
        assert sym in _lib.SIGNATURES and re.search(r"\b%s\(" % sym, hdr) and hasattr(L, sym)
    assert len(_lib.SIGNATURES["scd_gmm_em_step"][1]) == 19 and len(_lib.SIGNATURES["scd_gmm_predict"][1]) == 14
    assert L.scd_gmm_row_tile() == gc.ROW_TILE and L.scd_gmm_chain_rows() == gc.CHAIN_ROWS <= 1024
    assert callable(ops.gmm_em_step) and callable(ops.gmm_predict)


def test_workspace_limits(L):
    nb = L.scd_gmm_ws_bytes(126976, 768, 1000)
    print("scd_gmm workspace at 126,976 x 768, k = 1000: %.1f MB" % (nb / 1e6))
    assert 0 < nb <= 2 * GIB
    assert L.scd_gmm_ws_bytes(1, 1, 1) > 0 and L.scd_gmm_ws_bytes(10, 1024, 1024) > 0
    for n, d, k in ((0, 8, 4), (1 << 31, 8, 4), (10, 0, 4), (10, 1025, 4), (10, 8, 0), (10, 8, 1025)):
        assert L.scd_gmm_ws_bytes(n, d, k) == 0


def test_estimator_validates_its_arguments():
    from scd_amd.gmm import GaussianMixture, n_parameters
    for kw in (dict(covariance_type="full"), dict(covariance_type="tied"), dict(init_params="k-means++"), dict(n_components=0),
               dict(n_components=1025), dict(tol=-1.0), dict(reg_covar=-1e-6), dict(max_iter=0), dict(n_init=0)):
        with pytest.raises(ValueError):
            GaussianMixture(**kw)
    gm = GaussianMixture(n_components=3, covariance_type="spherical", weights_init=[0.2, 0.3, 0.5])
    with pytest.raises(ValueError, match="together"):
        gm._explicit(4, "cpu")
    bad = dict(weights_init=[0.2, 0.3, 0.4], means_init=np.zeros((3, 4)), precisions_init=np.ones(3))
    with pytest.raises(ValueError, match="sum to 1"):
        GaussianMixture(n_components=3, covariance_type="spherical", **bad)._explicit(4, "cpu")
    bad["weights_init"] = [0.2, 0.3, 0.5]
    with pytest.raises(ValueError, match="precisions_init"):
        GaussianMixture(n_components=3, covariance_type="diag", **bad)._explicit(4, "cpu")
    w, mu, v = GaussianMixture(n_components=3, covariance_type="spherical", **bad)._explicit(4, "cpu")
    assert v.shape == (3, 4) and mu.shape == (3, 4) and float(w.sum()) == 1.0
    with pytest.raises(ValueError, match="not fitted"):
        GaussianMixture(2).predict(np.zeros((3, 2), np.float32))
    assert n_parameters(7, 5, "diag") == 2 * 7 * 5 + 6 and n_parameters(7, 5, "spherical") == 7 * 5 + 2 * 7 - 1


def test_torch_m_step_is_the_restatements():
    import torch
    from scd_amd import gmm
    case = CASES["four_chains-unlabelled"]
    st = gc.reference(case)
    st["nk"][7] = 0.0                                           # an empty component: mean 0, variance reg_covar
    st["s1"][7] = st["s2"][7] = 0.0
    for ct in ("diag", "spherical"):
        w, mu, cov = gc.m_step_f64(st["nk"], st["s1"], st["s2"], ct, 1e-6)
        tw, tmu, tv = gmm.m_step(*(torch.as_tensor(st[q]) for q in ("nk", "s1", "s2")), ct, 1e-6)
        assert np.abs(tw.numpy() - w).max() <= 1e-15 and np.abs(tmu.numpy() - mu).max() <= 1e-13
        assert np.abs(tv.numpy() - gc.full_var(cov, 33)).max() <= 1e-12 and np.all(tv.numpy()[7] == 1e-6)
        a, B, C = gmm.kernel_params(tw, tmu, tv)
        a2, B2, C2 = gc.abc_f32(w, mu, gc.full_var(cov, 33))
        assert np.array_equal(B.numpy(), B2) and np.array_equal(C.numpy(), C2) and np.abs(a.numpy() - a2).max() <= 4e-6 * np.abs(a2).max()


def test_scripts_accept_the_new_options():
    import estimate_k
    import main_ptsup
    import main_unsup
    a = main_unsup.build_parser().parse_args(["--cluster", "GMM", "--covariance_type", "spherical", "--n_cluster", "7"])
    assert (a.cluster, a.covariance_type) == ("GMM", "spherical") and main_unsup.cluster_result_name(a).startswith("GMM_") \
        and main_unsup.cluster_result_name(a).endswith("_7.pt")
    assert main_unsup.build_parser().parse_args([]).covariance_type == "diag"
    assert main_ptsup.build_parser().parse_args(["--cluster", "GMM"]).covariance_type == "diag"
    with pytest.raises(SystemExit):
        main_unsup.build_parser().parse_args(["--covariance_type", "full"])
    e = estimate_k.parse_args(["--root_dir", "r", "--dataset_name", "d", "--criterion", "bic"])
    assert (e.search_mode, e.min_classes, e.covariance_type) == ("grid", 2, "diag")
    e = estimate_k.parse_args(["--root_dir", "r", "--dataset_name", "d", "--criterion", "bic", "--search_mode", "finch", "--covariance_type", "spherical"])
    assert (e.search_mode, e.covariance_type) == ("finch", "spherical")
    for crit, mode, lo in (("acc", "brent", None), ("silhouette", "grid", 2)):          # the other two criteria keep their defaults
        e = estimate_k.parse_args(["--root_dir", "r", "--dataset_name", "d", "--criterion", crit])
        assert (e.search_mode, e.min_classes) == (mode, lo)
    with pytest.raises(SystemExit):
        estimate_k.parse_args(["--root_dir", "r", "--dataset_name", "d", "--criterion", "aic"])


def test_bic_search_over_a_stub_evaluator():
    """The searches maximise, the criterion is -BIC: the lowest BIC wins, the lowest K wins a tie, each K is fitted once."""
    from scd_amd import estimate_k as ek
    calls = []

    def neg_bic(K):
        calls.append(K)
        return -(1000.0 + 3.0 * abs(K - 37) + (0.0 if K >= 37 else 5.0))

    k, trace = ek.grid_search(neg_bic, 2, 200)
    assert k == 37 and len(calls) == len(set(calls)) and all(len(ks) == len(sc) for ks, sc, _ in trace)
    k, _ = ek.grid_search(lambda K: -float(max(K, 10)), 2, 40)                          # BIC flat below 10: the lowest K
    assert k == 2
    k, trace = ek.finch_search(neg_bic, [512, 90, 40, 33, 9, 2], 2, 200)
    assert k == 40 and trace[0][0] == [2, 9, 33, 40, 90, 200]
