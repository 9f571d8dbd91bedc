"""CPU checks of the full-covariance mixture's restatement (tests/gmm_full_cases.py), its error model, the planted mistakes, the float64
EM against scikit-learn, the fairness of the seeds the device tests use, the ABI, and the arguments of the estimator and the three
scripts.  docs/design/gmm_full.md has the rules."""
import os
import re

import numpy as np
import pytest

import f32mm_plan as fp
import gmm_cases as gc
import gmm_full_cases as fc

GIB = 1 << 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fc.all_cases()
SOFT = [n for n, c in CASES.items() if not c["hard"]]
TYPES = ("full", "tied")


@pytest.fixture(autouse=True)
def needs_the_mixture():
    from scd_amd import _lib
    assert "scd_gmm_full_em_step" in _lib.SIGNATURES, "the library under test has no full-covariance mixture: these cases restate its contract"


@pytest.fixture(scope="module")
def L():
    from scd_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def fits():
    """The float64 and the float32-parameter loops of every fit case and type, and scikit-learn's fit from the same start: computed once."""
    from sklearn.mixture import GaussianMixture
    out = {}
    for name in fc.FIT_CASES:
        X, _, start = fc.blob_case(name)
        for ct in TYPES:
            (wi, mi, pi), (w0, mu0, c0) = fc.start_for(start, ct)
            sk = GaussianMixture(n_components=len(wi), covariance_type=ct, weights_init=wi, means_init=mi, precisions_init=pi).fit(X.astype(np.float64))
            out[name, ct] = (X, sk, fc.fit_f64(X, w0, mu0, c0, ct), fc.fit_f64(X, w0, mu0, c0, ct, float32_params=True))
    return out


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("covariance_type", TYPES)
@pytest.mark.parametrize("name", ["ragged_tile-unlabelled", "ragged_j_tile-unlabelled", "two_chains-unlabelled", "condition_1e4"])
def test_log_densities_and_m_step_are_scikit_learns(name, covariance_type):
    """a - 0.5 |(x - mu) U|^2 (+ the constant) from the float64 parameters is log w + _estimate_log_gaussian_prob, and the M-step from
    the statistics about the current means is _estimate_gaussian_parameters, both to 1e-10."""
    from sklearn.mixture._gaussian_mixture import _compute_precision_cholesky, _estimate_gaussian_parameters, _estimate_log_gaussian_prob
    case = CASES[name]
    X = case["X"].astype(np.float64)
    cov = case["cov"] if covariance_type == "full" else case["cov"].mean(axis=0)
    a, mu, Ut = fc.params_f64(case["w"], case["mu64"], cov)
    st = fc.em_step_f64(X, None, a, mu, Ut)
    want = _estimate_log_gaussian_prob(X, case["mu64"], _compute_precision_cholesky(cov, covariance_type), covariance_type) + case["logw"]
    assert np.abs(st["z"] + fc.shift(X.shape[1]) - want).max() <= 1e-10 * np.abs(want).max()
    nk, mean_sk, cov_sk = _estimate_gaussian_parameters(X, st["p"], 1e-6, covariance_type)
    w, mean, cov2 = fc.m_step_f64(st["nk"], st["s1c"], st["S"], mu, covariance_type, 1e-6)
    assert np.abs(w - nk / nk.sum()).max() <= 1e-10 and np.abs(mean - mean_sk).max() <= 1e-10 and np.abs(cov2 - cov_sk).max() <= 1e-10
    assert cov2.shape == cov_sk.shape
    for mistake in fc.M_STEP_MISTAKES:                          # every planted M-step mistake is far outside that tolerance
        if mistake == "tied_over_k" and covariance_type == "full":
            continue
        bad = fc.m_step_f64(st["nk"], st["s1c"], st["S"], mu, covariance_type, 1e-6, mistake=mistake)[2]
        assert np.abs(bad - cov_sk).max() > 1e-7, mistake


def test_the_hosts_m_step_and_factors_are_the_restatements():
    from scd_amd import gmm_full
    case = CASES["four_chains-unlabelled"]
    st = fc.reference(case)
    st["nk"][7] = 0.0                                           # an empty component: mean 0, covariance reg_covar I
    st["s1c"][7] = 0.0
    st["S"][7] = 0.0
    m = case["mu"].astype(np.float64)
    for ct in TYPES:
        w, mu, cov = fc.m_step_f64(st["nk"], st["s1c"], st["S"], m, ct, 1e-6)
        hw, hmu, hcov = gmm_full.m_step(st["nk"], st["s1c"], st["S"], m, ct, 1e-6)
        assert np.abs(hw - w).max() <= 1e-15 and np.abs(hmu - mu).max() <= 1e-13 and np.abs(hcov - cov).max() <= 1e-12
        if ct == "full":
            assert not hmu[7].any() and np.array_equal(hcov[7], 1e-6 * np.eye(8))
        ut = gmm_full.precision_cholesky_t(hcov)
        assert np.abs(ut - fc.chol_t(cov)).max() <= 1e-9 * np.abs(ut).max() and not np.triu(ut, 1).any()
        a, m32, u32 = gmm_full.kernel_params(hw, hmu, ut, "cpu")
        a2, m2, u2 = fc.params_f32(w, mu, cov)
        assert u32.shape == (257, 8, 8) and np.array_equal(m32.numpy(), m2)
        assert np.abs(u32.numpy() - u2).max() <= 1e-6 * np.abs(u2).max() and np.abs(a.numpy() - a2).max() <= 4e-6 * np.abs(a2).max()
    bad = np.eye(4)
    bad[3, 3] = -1.0
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        gmm_full.precision_cholesky_t(np.stack([np.eye(4), bad]))


def test_an_empty_component_keeps_scikit_learns_result():
    from sklearn.mixture._gaussian_mixture import _estimate_gaussian_parameters
    case = CASES["unreached"]
    X = case["X"].astype(np.float64)
    st = fc.reference(case)
    j = case["unreached"]
    assert st["nk"][j] == 0.0 and not st["s1c"][j].any() and not st["S"][j].any()
    assert (st["z"].max(axis=1) - st["z"][:, j]).min() > 1000.0
    w, mu, cov = fc.m_step_f64(st["nk"], st["s1c"], st["S"], case["mu"].astype(np.float64), "full", 1e-6)
    _, mu_sk, cov_sk = _estimate_gaussian_parameters(X, st["p"], 1e-6, "full")
    assert not mu[j].any() and np.array_equal(cov[j], 1e-6 * np.eye(12)) and np.array_equal(mu[j], mu_sk[j]) and np.array_equal(cov[j], cov_sk[j])


def test_special_cases_are_what_they_claim():
    cond = np.linalg.cond(CASES["condition_1e4"]["cov"])
    assert cond.max() > 2e3 and cond.max() < 1e4
    far = fc.reference(CASES["far_rows"])
    e32 = np.exp((far["z"] - far["z"].max(axis=1, keepdims=True)).astype(np.float32))
    assert ((e32 > 0).sum(axis=1)[::2] == 1).mean() > 0.7 and far["z"][::2].max() < -1000      # on most far rows one e survives
    t = CASES["identical"]
    bd = fc.bounds(t)
    tied = (bd["gap"] == 0) & (bd["ref"]["pred"] == 3)
    assert tied.sum() >= 5 and np.array_equal(bd["ref"]["p"][:, 3], bd["ref"]["p"][:, 17])
    assert np.array_equal(bd["ref"]["S"][3], bd["ref"]["S"][17])
    lab = CASES["least_likely_label"]
    r = fc.reference(lab)
    rows = np.flatnonzero(lab["y"] >= 0)
    assert (r["z"][rows, lab["y"][rows]] == r["z"][rows].min(axis=1)).all() and (r["r"][rows, lab["y"][rows]] == 1).all()


@pytest.mark.parametrize("name", list(CASES))
def test_ut_is_non_zero_only_where_allowed(name):
    """Ut[k][j][l] = U_k[l][j] with U_k upper triangular: exact zeros for l > j, a positive diagonal."""
    Ut = CASES[name]["Ut"]
    assert Ut.dtype == np.float32 and not np.triu(Ut, 1).any() and (np.diagonal(Ut, axis1=1, axis2=2) > 0).all()


@pytest.mark.parametrize("name", SOFT)
def test_no_row_is_excused(name):
    case = CASES[name]
    bd = fc.bounds(case)
    dec = fc.decided_rows(bd, case["exact_ties"])
    cap = case.get("undecided_cap", 0.0)                        # 0 below f32mm_plan.LARGE_N rows: no row is excused there
    assert cap == (fp.UNDECIDED_CAP if case["X"].shape[0] >= fp.LARGE_N else 0.0)
    assert (~dec).mean() <= cap, "rows %s have a top-two gap within 2 delta" % np.flatnonzero(~dec)


def test_shapes_are_those_the_kernel_branches_on():
    rt, T = fc.ROW_TILE, fc.CHAIN_ROWS
    assert list(fc.shapes().values()) == [(1, 1, 1), (rt - 1, 5, 3), (rt + 1, 32, 33), (3 * rt + 7, 33, 5), (2 * rt, 64, 1024), (T + 1, 24, 31),
                                          (3 * T + 5, 8, 257), (9 * T + 3, 17, 9),
                                          # the range plans of tests/f32mm_plan.py: n, with d on either side of the second j-tile
                                          (5121, 64, 9), (5153, 33, 5), (3 * T + 5, 33, 5), (40000, 17, 9), (126976, 8, 5), (140001, 5, 3)]
    # every variant below f32mm_plan.LARGE_N rows, unlabelled / weights / hard from there on
    assert sum(not c["hard"] for c in CASES.values()) == len(SOFT) == 9 * 5 + 5 * 2 + 5


def test_variants_differ_only_where_they_should():
    k = 33
    bad = fc.shape_case("one_j_tile", "bad_labels")
    got = fc.reference(bad)
    assert list(got["info"]) == [2, 0] and sorted(bad["y"][bad["y"] >= k]) == [k, k + 5]
    want = fc.reference(fc.bad_labels_as_unlabelled(bad))
    assert got["ll"] == want["ll"] and np.array_equal(got["S"], want["S"]) and list(want["info"]) == [0, 0]
    w = fc.shape_case("one_j_tile", "weights")
    assert (w["sw"] == 0).any() and (w["sw"] > 0).any() and (w["y"] >= 0).any() and (w["y"] < 0).any()
    hard = fc.shape_case("ranges", "hard")
    h = fc.reference(hard)
    assert h["ll"] == 0.0 and h["nk"].sum() == (hard["y"] >= 0).sum() and set(np.unique(h["r"])) == {0.0, 1.0}
    al = fc.shape_case("one_j_tile", "all_labelled")
    assert (al["y"] >= 0).all()


def test_all_rows_labelled_gives_the_class_conditional_moments():
    case = fc.shape_case("two_chains", "all_labelled")
    X, y = case["X"].astype(np.float64), case["y"]
    st = fc.reference(case)
    w, mu, cov = fc.m_step_f64(st["nk"], st["s1c"], st["S"], case["mu"].astype(np.float64), "full", 0.0)
    for j in range(case["a"].shape[0]):
        rows = X[y == j]
        assert st["nk"][j] == len(rows)
        if len(rows) > 1:
            # c = fl32(x - mu) is rounded once (u |c|, 6e-8 relative), which is part of the contract; nothing else separates the two
            assert np.abs(mu[j] - rows.mean(axis=0)).max() <= 1e-6 and np.abs(cov[j] - np.cov(rows.T, bias=True)).max() <= 1e-6
    hard = fc.em_hard_f64(case["X"], y, case["mu"])
    assert np.array_equal(hard["nk"], st["nk"]) and np.array_equal(hard["s1c"], st["s1c"]) and np.array_equal(hard["S"], st["S"])


# ------------------------------------------------------------------------------------------------- the bounds see the mistakes
@pytest.mark.parametrize("mistake", list(fc.MISTAKES))
def test_every_planted_mistake_exceeds_the_bounds(mistake):
    case = CASES[fc.MISTAKES[mistake]]
    bd = fc.bounds(case)
    assert not fc.violates(fc.reference(case), bd, case["exact_ties"])
    wrong = fc.planted(case, mistake)
    print("planted %-30s on %-26s: difference / bound %s" % (mistake, fc.MISTAKES[mistake], {k: "%.3g" % v for k, v in fc.ratios(wrong, bd).items()}))
    assert fc.violates(wrong, bd, case["exact_ties"]), "%s goes unseen on %s" % (mistake, fc.MISTAKES[mistake])
    if mistake in fc.RANGE_MISTAKES:
        assert any(v > 1.0 for v in fc.ratios(wrong, bd).values())              # a sum breaks its bound, not a prediction


def test_bounds_are_those_the_design_note_quotes():
    """delta is about 2e-3 at d = 64 and 6e-4 at d = 32; a float32 numpy evaluation of the centred form is well inside it."""
    for name, lo, hi in (("full_width-unlabelled", 5e-4, 8e-3), ("one_j_tile-unlabelled", 1e-4, 3e-3)):
        case = CASES[name]
        bd = fc.bounds(case)
        c32 = case["X"][:, None, :] - case["mu"][None, :, :]
        y32 = np.matmul(c32.transpose(1, 0, 2), case["Ut"].transpose(0, 2, 1))
        z32 = (case["a"][None, :] - np.float32(0.5) * (y32 * y32).sum(axis=2).T).astype(np.float64)
        err = np.abs(z32 - bd["ref"]["z"]).max(axis=1)
        print("%s: delta %.3g, float32 numpy logits off by %.3g" % (name, bd["delta"].max(), err.max()))
        assert lo < bd["delta"].max() < hi and (err < bd["delta"]).all()


# ------------------------------------------------------------------------------------------------- the fit against scikit-learn
@pytest.mark.parametrize("covariance_type", TYPES)
@pytest.mark.parametrize("name", list(fc.FIT_CASES))
def test_em_restatement_against_sklearn(fits, name, covariance_type):
    X, sk, fit, _ = fits[name, covariance_type]
    X64 = X.astype(np.float64)
    print("%s %s: %d iterations, lower bound %.12g (scikit-learn %.12g)" % (name, covariance_type, fit["n_iter"], fit["lower_bound"], sk.lower_bound_))
    assert sk.converged_ and fit["converged"] and fit["n_iter"] == sk.n_iter_
    assert abs(fit["lower_bound"] - sk.lower_bound_) <= 1e-9 * abs(sk.lower_bound_)
    assert np.array_equal(fit["labels"], sk.predict(X64))
    assert np.abs(fit["cov"] - sk.covariances_).max() <= 1e-9 and fit["cov"].shape == sk.covariances_.shape
    k, d = fit["mu"].shape
    want = k * d * (d + 1) // 2 + k * d + k - 1 if covariance_type == "full" else d * (d + 1) // 2 + k * d + k - 1
    assert fc.n_parameters(k, d, covariance_type) == sk._n_parameters() == want
    bic = fc.bic_f64(fit, X, covariance_type)
    assert abs(bic - sk.bic(X64)) <= 1e-9 * abs(bic)
    aic = bic - fc.n_parameters(k, d, covariance_type) * (np.log(X.shape[0]) - 2.0)
    assert abs(aic - sk.aic(X64)) <= 1e-9 * abs(aic)
    assert (fit["final"]["p"].max(axis=1) < 0.99).sum() >= 100  # these blobs have rows the mixture is unsure of


@pytest.mark.parametrize("covariance_type", TYPES)
@pytest.mark.parametrize("name", list(fc.FIT_CASES))
def test_the_fit_seeds_are_fair(fits, name, covariance_type):
    """The loop as the device runs it (a, mu, Ut rounded to float32, c formed in float32): the same n_iter and labels as float64; at
    its final parameters no row's top-two gap is within 2 delta; and the last two changes of the lower bound are further from tol than
    twice the likelihood bound over n, so rounding cannot move the stop.  The device test then excuses nothing."""
    X, _, f64, f32 = fits[name, covariance_type]
    assert f32["converged"] and f32["n_iter"] == f64["n_iter"] >= 3 and np.array_equal(f32["labels"], f64["labels"])
    bd = fc.bounds(fc.as_case(X, f32["params"]))
    assert fc.decided_rows(bd).all()
    tr, slack = f32["trace"], 2.0 * bd["ll"] / len(X)
    changes = [abs(tr[-1] - tr[-2]), abs(tr[-2] - tr[-3])]
    print("%s %s: last changes %.3g, %.3g; twice the likelihood bound over n %.3g" % (name, covariance_type, changes[0], changes[1], slack))
    assert changes[0] < 1e-3 - slack and changes[1] > 1e-3 + slack


def test_rotated_classes_need_a_covariance_matrix():
    """Four rotated, elongated classes on nearly the same centre: from one k-means start the full mixture recovers them (ARI >= 0.99),
    the diagonal restatement does not (ARI < 0.5)."""
    from sklearn.cluster import KMeans
    from sklearn.metrics import adjusted_rand_score
    X, z, k = fc.rotated_classes_case(0)
    X64 = X.astype(np.float64)
    lab = KMeans(k, n_init=1, random_state=0).fit(X64).labels_
    nk = np.bincount(lab, minlength=k).astype(np.float64)
    mu0 = np.stack([X64[lab == j].mean(axis=0) for j in range(k)])
    cov0 = np.stack([np.cov(X64[lab == j].T, bias=True) + 1e-6 * np.eye(X.shape[1]) for j in range(k)])
    full = fc.fit_f64(X, nk / nk.sum(), mu0, cov0, "full")
    diag = gc.fit_f64(X, nk / nk.sum(), mu0, np.stack([X64[lab == j].var(axis=0) + 1e-6 for j in range(k)]), "diag")
    ari_f, ari_d = adjusted_rand_score(z, full["labels"]), adjusted_rand_score(z, diag["labels"])
    print("rotated classes: ARI full %.3f, diag %.3f, the k-means start %.3f" % (ari_f, ari_d, adjusted_rand_score(z, lab)))
    assert full["converged"] and ari_f >= 0.99 and ari_d < 0.5


def test_semi_supervised_fit_helps_where_two_classes_overlap():
    X, z, y, start = fc.overlap_case()
    _, (w0, mu0, c0) = fc.start_for(start, "full")
    unsup = fc.fit_f64(X, w0, mu0, c0, "full", float32_params=True)
    semi = fc.fit_f64(X, w0, mu0, c0, "full", y=y, float32_params=True)
    assert unsup["converged"] and semi["converged"]
    assert (np.diff(semi["trace"]) >= -1e-12).all() and (np.diff(unsup["trace"]) >= -1e-12).all()
    rest = y < 0
    acc_u, acc_s = (unsup["labels"][rest] == z[rest]).mean(), (semi["labels"][rest] == z[rest]).mean()
    print("accuracy on the unlabelled rows: unsupervised %.3f, semi-supervised %.3f" % (acc_u, acc_s))
    assert acc_s >= acc_u and acc_s > 0.8
    assert fc.decided_rows(fc.bounds(fc.as_case(X, semi["params"]))).all()


def test_bic_finds_the_planted_k_with_scikit_learn():
    """The cache of the device test: scikit-learn's own k-means-started full mixture has its lowest BIC at the planted K on unit rows."""
    from sklearn.mixture import GaussianMixture
    X, _, k = fc.planted_k_case()
    Un = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float64)
    bic = {K: GaussianMixture(n_components=K, covariance_type="full", random_state=0).fit(Un).bic(Un) for K in range(2, 9)}
    assert min(bic, key=bic.get) == k


# ------------------------------------------------------------------------------------------------- ABI, limits, arguments
def test_abi_declares_the_mixture(L):
    from scd_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "scd_hip.h")).read()
    for sym in ("scd_gmm_full_ws_bytes", "scd_gmm_full_row_tile", "scd_gmm_full_chain_rows", "scd_gmm_full_em_step", "scd_gmm_full_predict"):
        assert sym in _lib.SIGNATURES and re.search(r"\b%s\(" % sym, hdr) and hasattr(L, sym)
    assert len(_lib.SIGNATURES["scd_gmm_full_em_step"][1]) == 19 and len(_lib.SIGNATURES["scd_gmm_full_predict"][1]) == 14
    assert L.scd_gmm_full_row_tile() == fc.ROW_TILE and L.scd_gmm_full_chain_rows() == fc.CHAIN_ROWS <= 1024
    assert callable(ops.gmm_full_em_step) and callable(ops.gmm_full_predict)


def test_workspace_limits(L):
    nb = L.scd_gmm_full_ws_bytes(126976, 64, 1000)
    print("scd_gmm_full workspace at 126,976 x 64, k = 1000: %.1f MB" % (nb / 1e6))
    assert 126976 * 1024 * 4 < nb <= 2 * GIB
    assert L.scd_gmm_full_ws_bytes(1, 1, 1) > 0 and L.scd_gmm_full_ws_bytes(10, 64, 1024) > 0
    assert L.scd_gmm_full_ws_bytes((1 << 31) - 1, 1, 1) > 0
    assert L.scd_gmm_full_ws_bytes(1, 64, 1000) < 64 << 20       # what scd_gmm_full_predict needs: no r, one range of partials
    for n, d, k in ((0, 8, 4), (1 << 31, 8, 4), (10, 0, 4), (10, 65, 4), (10, 8, 0), (10, 8, 1025)):
        assert L.scd_gmm_full_ws_bytes(n, d, k) == 0


def test_estimator_validates_its_arguments():
    from scd_amd.gmm import GaussianMixture
    from scd_amd.gmm_full import FullGaussianMixture, n_parameters
    for kw in (dict(covariance_type="diag"), dict(covariance_type="spherical"), dict(init_params="k-means++"), dict(n_components=0),
               dict(n_components=1025), dict(tol=-1.0), dict(reg_covar=-1e-6), dict(max_iter=0), dict(n_init=0)):
        with pytest.raises(ValueError):
            FullGaussianMixture(**kw)
    assert issubclass(FullGaussianMixture, GaussianMixture) and FullGaussianMixture().covariance_type == "full"
    assert FullGaussianMixture.fit is GaussianMixture.fit and FullGaussianMixture._start_labels is GaussianMixture._start_labels
    gm = FullGaussianMixture(n_components=3, weights_init=[0.2, 0.3, 0.5])
    with pytest.raises(ValueError, match="together"):
        gm._explicit(4, "cpu")
    eye = np.broadcast_to(np.eye(4), (3, 4, 4))
    bad = dict(weights_init=[0.2, 0.3, 0.4], means_init=np.zeros((3, 4)), precisions_init=eye)
    with pytest.raises(ValueError, match="sum to 1"):
        FullGaussianMixture(n_components=3, **bad)._explicit(4, "cpu")
    bad["weights_init"] = [0.2, 0.3, 0.5]
    with pytest.raises(ValueError, match="precisions_init"):
        FullGaussianMixture(n_components=3, covariance_type="tied", **bad)._explicit(4, "cpu")     # (d, d) wanted
    with pytest.raises(ValueError, match="precisions_init"):
        FullGaussianMixture(n_components=3, **dict(bad, precisions_init=-eye))._explicit(4, "cpu")
    w, mu, cov = FullGaussianMixture(n_components=3, **dict(bad, precisions_init=4.0 * eye))._explicit(4, "cpu")
    assert cov.shape == (3, 4, 4) and np.allclose(cov, 0.25 * eye) and float(w.sum()) == 1.0
    w, mu, cov = FullGaussianMixture(n_components=3, covariance_type="tied", **dict(bad, precisions_init=np.eye(4)))._explicit(4, "cpu")
    assert cov.shape == (4, 4)
    with pytest.raises(ValueError, match="not fitted"):
        FullGaussianMixture(2).predict(np.zeros((3, 2), np.float32))
    with pytest.raises(ValueError, match=r"scd_amd\.pca\.PCA.*--pca_dim"):
        FullGaussianMixture(2)._check_features(65)
    FullGaussianMixture(2)._check_features(64)
    assert n_parameters(7, 5, "full") == 7 * 15 + 35 + 6 and n_parameters(7, 5, "tied") == 15 + 35 + 6


def test_scripts_accept_the_new_options():
    import estimate_k
    import main_ptsup
    import main_unsup
    for value in ("GMM_FULL", "GMM_TIED"):
        a = main_unsup.build_parser().parse_args(["--cluster", value, "--n_cluster", "7", "--pca_dim", "16"])
        assert a.cluster == value and a.covariance_type == "diag"
        name = main_unsup.cluster_result_name(a)
        assert name.startswith(value + "_") and name.endswith("_7_pca16.pt")
        assert main_ptsup.build_parser().parse_args(["--cluster", value]).cluster == value
    assert main_unsup.FULL_COVARIANCE == {"GMM_FULL": "full", "GMM_TIED": "tied"}
    a = main_unsup.build_parser().parse_args(["--cluster", "GMM_FULL", "--n_cluster", "3"])
    with pytest.raises(SystemExit, match=r"--pca_dim M with M <= 64"):        # refused before anything touches a device
        main_unsup.run_clustering(a, np.zeros((10, 65), np.float32), np.zeros((0, 65), np.float32), np.zeros(0))
    with pytest.raises(SystemExit):                             # the diagonal mixture's option keeps its two choices
        main_unsup.build_parser().parse_args(["--covariance_type", "full"])
    for ct in ("full", "tied", "diag", "spherical"):
        e = estimate_k.parse_args(["--root_dir", "r", "--dataset_name", "d", "--criterion", "bic", "--covariance_type", ct])
        assert (e.search_mode, e.min_classes, e.covariance_type) == ("grid", 2, ct)
    with pytest.raises(SystemExit):
        estimate_k.parse_args(["--root_dir", "r", "--dataset_name", "d", "--criterion", "bic", "--covariance_type", "banded"])
