"""GPU checks of scd_gmm_full_em_step / scd_gmm_full_predict (scd_amd/csrc/gmm_full.hip), scd_amd.gmm_full.FullGaussianMixture,
main_unsup.py --cluster GMM_FULL and estimate_k.py --criterion bic --covariance_type full against the float64 restatement and the error
model of tests/gmm_full_cases.py: every element within its bound, no row excused.  docs/design/gmm_full.md has the rules and records the
printed error / bound ratios."""
import json
import os

import numpy as np
import pytest
import torch

import gmm_full_cases as fc

pytestmark = pytest.mark.gpu
CASES = fc.all_cases()
TYPES = ("full", "tied")


@pytest.fixture(scope="module")
def ops():
    from scd_amd import ops as o
    return o


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def run(ops, case):
    if case["hard"]:
        ll, nk, s1c, S, pred, info = ops.gmm_full_em_step(dev(case["X"]), None, dev(case["mu"]), None, y=dev(case["y"]), sample_weight=dev(case["sw"]))
    else:
        ll, nk, s1c, S, pred, info = ops.gmm_full_em_step(dev(case["X"]), dev(case["a"]), dev(case["mu"]), dev(case["Ut"]), y=dev(case["y"]),
                                                          sample_weight=dev(case["sw"]), want_pred=True)
    return dict(ll=float(ll.item()), nk=nk.cpu().numpy(), s1c=s1c.cpu().numpy(), S=S.cpu().numpy(),
                pred=None if pred is None else pred.cpu().numpy().astype(np.int64), info=info.cpu().numpy())


# ------------------------------------------------------------------------------------------------- every case within its bounds
@pytest.mark.parametrize("name", list(CASES))
def test_step_within_the_bounds(ops, name):
    case = CASES[name]
    got = run(ops, case)
    n, d = case["X"].shape
    k = case["a"].shape[0]
    bd = fc.bounds(case)
    q = fc.ratios(got, bd)
    print("gmm_full %-28s n %5d d %3d k %4d: error / bound  ll %.3f  nk %.3f  s1c %.3f  S %.3f" % (name, n, d, k, q["ll"], q["nk"], q["s1c"], q["S"]))
    assert list(got["info"]) == list(bd["ref"]["info"])
    if name.endswith("bad_labels"):
        assert got["info"][0] == 2
    assert abs(got["ll"] - bd["ref"]["ll"]) <= bd["ll"]
    for key in ("nk", "s1c", "S"):
        assert (np.abs(got[key] - bd["ref"][key]) <= bd[key]).all(), key
    assert np.array_equal(got["S"], got["S"].transpose(0, 2, 1))                # both halves written from the same sum
    if case["hard"]:
        assert got["ll"] == 0.0 and got["pred"] is None and np.array_equal(got["nk"], bd["ref"]["nk"])
        return
    dec = fc.decided_rows(bd, case["exact_ties"])               # pred_out covers every row, whatever its label
    assert (~dec).mean() <= case.get("undecided_cap", 0.0)      # 0 below f32mm_plan.LARGE_N rows: no row is excused there
    assert np.array_equal(got["pred"][dec], bd["ref"]["pred"][dec])
    if "unreached" in case:                                     # no underflowing mass reaches it: exact zeros
        j = case["unreached"]
        assert got["nk"][j] == 0.0 and not got["s1c"][j].any() and not got["S"][j].any()
        from scd_amd import gmm_full
        _, mu, cov = gmm_full.m_step(got["nk"], got["s1c"], got["S"], case["mu"].astype(np.float64), "full", 1e-6)
        assert not mu[j].any() and np.array_equal(cov[j], 1e-6 * np.eye(d))
    if name == "identical":
        assert np.array_equal(got["S"][3], got["S"][17]) and np.array_equal(got["s1c"][3], got["s1c"][17]) and got["nk"][3] == got["nk"][17] > 0


def test_bad_labels_equal_the_unlabelled_result(ops):
    case = fc.shape_case("one_j_tile", "bad_labels")
    a, b = run(ops, case), run(ops, fc.bad_labels_as_unlabelled(case))
    assert list(a["info"]) == [2, 0] and list(b["info"]) == [0, 0]
    assert a["ll"] == b["ll"] and all(np.array_equal(a[q], b[q]) for q in ("nk", "s1c", "S", "pred"))


@pytest.mark.parametrize("name", ["four_chains-weights", "ranges-mixed", "ragged_j_tile-unlabelled", "ranges_x_tiles-weights", "cap32-weights",
                                  "colsum_cap-weights"])
def test_two_calls_return_the_same_bits(ops, name):
    case = CASES[name]
    a, b = run(ops, case), run(ops, case)
    assert a["ll"] == b["ll"] and all(np.array_equal(a[q], b[q]) for q in ("nk", "s1c", "S", "pred", "info"))
    assert np.isfinite(a["S"]).all() and np.abs(a["s1c"]).max() > 0


def test_cached_workspace_holds_no_stale_partials(ops):
    """One range, then the 32 ranges of cap32 through the same cached workspace, then the one range again: the finish kernel reads the R
    partials of its own call and nothing a larger call left behind."""
    small, big = CASES["jt2_chains-weights"], CASES["cap32-weights"]
    a = run(ops, small)
    mid = run(ops, big)
    b = run(ops, small)
    assert a["ll"] == b["ll"] and all(np.array_equal(a[q], b[q]) for q in ("nk", "s1c", "S", "pred", "info"))
    assert np.isfinite(mid["S"]).all() and np.abs(mid["s1c"]).max() > 0


@pytest.mark.parametrize("name", ["n1_d1_k1-unlabelled", "one_j_tile-mixed", "ragged_j_tile-unlabelled", "full_width-unlabelled",
                                  "four_chains-weights", "ranges-unlabelled", "condition_1e4", "far_rows", "identical", "jt2_chains-unlabelled",
                                  "ranges_x_tiles-unlabelled"])
def test_predict_equals_the_steps_argmax(ops, name):
    case = CASES[name]
    prm = (dev(case["X"]), dev(case["a"]), dev(case["mu"]), dev(case["Ut"]))
    pred, row_ll, resp = ops.gmm_full_predict(*prm, want_ll=True, want_resp=True)
    got = run(ops, case)
    assert np.array_equal(pred.cpu().numpy(), got["pred"])
    bd = fc.bounds(dict(case, y=None, sw=None))
    resp, row_ll = resp.cpu().numpy(), row_ll.cpu().numpy()
    assert resp.shape == (case["X"].shape[0], case["a"].shape[0])
    q_r, q_l = fc.ratio(resp, bd["ref"]["p"], bd["resp"]), fc.ratio(row_ll, bd["ref"]["lse"], bd["row_ll"])
    print("predict %-26s: error / bound  resp %.3f  row_ll %.3f" % (name, q_r, q_l))
    assert (np.abs(resp - bd["ref"]["p"]) <= bd["resp"]).all() and (np.abs(row_ll - bd["ref"]["lse"]) <= bd["row_ll"]).all()
    if name == "identical":
        assert np.array_equal(resp[:, 3], resp[:, 17])
    only = ops.gmm_full_predict(*prm)
    assert only[1] is None and only[2] is None and np.array_equal(only[0].cpu().numpy(), got["pred"])


def test_limits_are_refused(ops):
    from scd_amd._lib import ScdError, SCD_EINVAL
    x = torch.zeros((4, 65), dtype=torch.float32, device="cuda")
    mu = torch.zeros((3, 65), dtype=torch.float32, device="cuda")
    ut = torch.zeros((3, 65, 65), dtype=torch.float32, device="cuda")
    a = torch.zeros(3, dtype=torch.float32, device="cuda")
    with pytest.raises(ScdError) as e:
        ops.gmm_full_em_step(x, a, mu, ut)
    assert e.value.code == SCD_EINVAL
    with pytest.raises(ScdError) as e:
        ops.gmm_full_predict(x, a, mu, ut)
    assert e.value.code == SCD_EINVAL
    x8, mu8 = x[:, :8].contiguous(), mu[:, :8].contiguous()
    with pytest.raises(ScdError):
        ops.gmm_full_predict(x8, a, mu8, ut[:, :8, :9].contiguous())
    with pytest.raises(ScdError):
        ops.gmm_full_em_step(x8, None, mu8, None, y=None)       # the hard M-step needs labels
    with pytest.raises(ScdError):
        ops.gmm_full_em_step(x8, a, mu8, None)                  # a and ut together


# ------------------------------------------------------------------------------------------------- a fit, step by step through ops
def test_steps_of_a_fit_follow_the_restatement(ops):
    """EM driven by hand: every device step is within the bounds of the restatement taken from the SAME parameters, and the trace of
    the log-likelihood is nondecreasing up to twice the likelihood bound."""
    from scd_amd import gmm_full
    X, _, start = fc.blob_case("n1200_d8_k4")
    w, mu, cov = start
    x = dev(X)
    trace, allowed, worst = [], [], {}
    for _ in range(6):
        a, m32, ut = gmm_full.kernel_params(w, mu, gmm_full.precision_cholesky_t(cov), x.device)
        ll, nk, s1c, S, _, info = ops.gmm_full_em_step(x, a, m32, ut)
        got = dict(ll=float(ll.item()), nk=nk.cpu().numpy(), s1c=s1c.cpu().numpy(), S=S.cpu().numpy())
        bd = fc.bounds(fc.as_case(X, (a.cpu().numpy(), m32.cpu().numpy(), ut.cpu().numpy())))
        q = fc.ratios(got, bd)
        worst = {key: max(v, worst.get(key, 0.0)) for key, v in q.items()}
        assert all(v <= 1.0 for v in q.values()) and not info.cpu().numpy().any()
        trace.append(got["ll"])
        allowed.append(bd["ll"])
        w, mu, cov = gmm_full.m_step(got["nk"], got["s1c"], got["S"], m32.double().cpu().numpy(), "full", 1e-6)
    print("stepwise fit: largest error / bound over 6 steps %s" % {key: round(v, 4) for key, v in worst.items()})
    for i in range(1, len(trace)):
        assert trace[i] >= trace[i - 1] - 2.0 * max(allowed[i], allowed[i - 1])


# ------------------------------------------------------------------------------------------------- the estimator
@pytest.mark.parametrize("covariance_type", TYPES)
@pytest.mark.parametrize("name", list(fc.FIT_CASES))
def test_fit_from_an_explicit_start(name, covariance_type):
    from scd_amd.gmm_full import FullGaussianMixture
    X, _, start = fc.blob_case(name)
    (wi, mi, pi), (w0, mu0, c0) = fc.start_for(start, covariance_type)
    ref = fc.fit_f64(X, w0, mu0, c0, covariance_type, float32_params=True)
    gm = FullGaussianMixture(n_components=len(wi), covariance_type=covariance_type, weights_init=wi, means_init=mi, precisions_init=pi).fit(X)
    print("fit %-14s %-5s: %d iterations (restatement %d), lower bound %.9g (restatement %.9g)"
          % (name, covariance_type, gm.n_iter_, ref["n_iter"], gm.lower_bound_, ref["lower_bound"]))
    assert gm.converged_ and gm.n_iter_ == ref["n_iter"] and len(gm.lower_bounds_) == gm.n_iter_
    n, d = X.shape
    k = len(wi)
    bd = fc.bounds(fc.as_case(X, tuple(t.cpu().numpy() for t in gm._abc)))     # at the device's own final float32 parameters
    dec = fc.decided_rows(bd)
    labels = gm.predict(X).cpu().numpy()
    assert dec.all() and np.array_equal(labels, bd["ref"]["pred"]) and np.array_equal(gm.labels_, labels)
    assert np.array_equal(labels, ref["labels"])                # no row excused
    want_bic = -2.0 * (bd["ref"]["lse"].sum() + n * fc.shift(d)) + fc.n_parameters(k, d, covariance_type) * np.log(n)
    assert abs(gm.bic(X) - want_bic) <= 2.0 * bd["row_ll"].sum()
    assert abs(gm.aic(X) - (want_bic - fc.n_parameters(k, d, covariance_type) * (np.log(n) - 2.0))) <= 2.0 * bd["row_ll"].sum()
    shape = (k, d, d) if covariance_type == "full" else (d, d)
    assert gm.covariances_.shape == gm.precisions_.shape == gm.precisions_cholesky_.shape == shape and gm.means_.shape == (k, d)
    assert np.allclose(gm.precisions_ @ gm.covariances_, np.eye(d), atol=1e-8) and abs(gm.weights_.sum() - 1.0) < 1e-12
    assert not np.tril(gm.precisions_cholesky_, -1).any()       # scikit-learn's upper-triangular factor
    assert np.abs(gm.covariances_ - ref["cov"]).max() <= 1e-3 * np.abs(ref["cov"]).max()
    proba = gm.predict_proba(X).cpu().numpy()
    assert (np.abs(proba - bd["ref"]["p"]) <= bd["resp"]).all() and np.abs(proba.sum(axis=1) - 1.0).max() < 1e-4
    assert abs(gm.score(X) - (bd["ref"]["lse"].mean() + fc.shift(d))) <= bd["row_ll"].mean()


def test_semi_supervised_fit_keeps_the_clamped_rows_and_helps_the_rest():
    from scd_amd.gmm_full import FullGaussianMixture
    X, z, y, start = fc.overlap_case()
    (wi, mi, pi), _ = fc.start_for(start, "full")
    kw = dict(n_components=4, weights_init=wi, means_init=mi, precisions_init=pi)
    unsup = FullGaussianMixture(**kw).fit(X)
    semi = FullGaussianMixture(**kw).fit(X, y)
    lab, rest = y >= 0, y < 0
    assert semi.converged_ and np.array_equal(semi.labels_[lab], y[lab])
    acc_u, acc_s = (unsup.labels_[rest] == z[rest]).mean(), (semi.labels_[rest] == z[rest]).mean()
    print("accuracy on the unlabelled rows: unsupervised %.3f, semi-supervised %.3f" % (acc_u, acc_s))
    assert acc_s >= acc_u and acc_s > 0.8
    slack = 2.0 * fc.bounds(fc.as_case(X, tuple(t.cpu().numpy() for t in semi._abc), y=y))["ll"] / len(y)
    assert (np.diff(semi.lower_bounds_) >= -slack).all()        # the complete-data likelihood rises, up to twice its bound


def test_rotated_classes_are_recovered_on_the_device():
    """The case of tests/test_gmm_full_host.py: a covariance matrix per component recovers four rotated, elongated classes from a
    k-means start that does not (ARI >= 0.99); the diagonal mixture from the same seed stays below 0.5."""
    from sklearn.metrics import adjusted_rand_score
    from scd_amd.gmm import GaussianMixture
    from scd_amd.gmm_full import FullGaussianMixture
    X, z, k = fc.rotated_classes_case(0)
    full = FullGaussianMixture(n_components=k, random_state=0).fit(X)
    diag = GaussianMixture(n_components=k, random_state=0).fit(X)
    ari_f, ari_d = adjusted_rand_score(z, full.labels_), adjusted_rand_score(z, diag.labels_)
    print("rotated classes on the device: ARI full %.3f (%d iterations), diag %.3f" % (ari_f, full.n_iter_, ari_d))
    assert full.converged_ and ari_f >= 0.99 and ari_d < 0.5
    assert full.bic(X) < diag.bic(X) - 1e4                      # BIC separates them by tens of thousands


def test_kmeans_and_random_starts_and_an_unconverged_fit():
    from scd_amd.gmm import ConvergenceWarning
    from scd_amd.gmm_full import FullGaussianMixture
    X, z, k = fc.planted_k_case()
    for ct in TYPES:
        gm = FullGaussianMixture(n_components=k, covariance_type=ct, random_state=0).fit(X)
        assert gm.converged_ and len({(int(a), int(b)) for a, b in zip(gm.labels_, z)}) == k     # the components are the blobs
    y = np.where(np.arange(len(z)) % 4 == 0, z, -1)
    semi = FullGaussianMixture(n_components=k, random_state=0).fit(X, y)
    assert np.array_equal(semi.labels_[y >= 0], y[y >= 0]) and (semi.labels_ == z).mean() > 0.99
    with pytest.warns(ConvergenceWarning):
        r = FullGaussianMixture(n_components=k, init_params="random", random_state=3, max_iter=2, n_init=2).fit(X)
    assert not r.converged_ and r.n_iter_ == 2 and np.isfinite(r.lower_bound_)
    with pytest.raises(ValueError, match=r"scd_amd\.pca\.PCA.*--pca_dim"):
        FullGaussianMixture(n_components=2).fit(np.zeros((80, 65), np.float32))


# ------------------------------------------------------------------------------------------------- the scripts
def _wide_cache():
    """The planted-K rows embedded in 48 dimensions by a fixed rotation, with a little noise in the other directions: what a feature
    cache looks like to --pca_dim."""
    X, z, k = fc.planted_k_case()
    rng = np.random.default_rng(601)
    Q = np.linalg.qr(rng.standard_normal((48, 48)))[0]
    wide = np.concatenate([X, 0.05 * rng.standard_normal((len(X), 40)).astype(np.float32)], axis=1) @ Q.T.astype(np.float32)
    return wide.astype(np.float32), z, k


def test_main_unsup_cluster_gmm_full_with_pca():
    """main_unsup.py --cluster GMM_FULL --pca_dim 16 and the clamped path of main_ptsup.py, through pca_reduce and run_clustering."""
    import importlib
    mu = importlib.import_module("main_unsup")
    X, z, k = _wide_cache()
    for value in ("GMM_FULL", "GMM_TIED"):
        args = mu.build_parser().parse_args(["--cluster", value, "--n_cluster", str(k), "--pca_dim", "16"])
        u, l = mu.pca_reduce(args, X, X[:0])
        assert u.shape == (len(z), 16)
        all_preds, preds = mu.run_clustering(args, u, l, np.zeros(0))
        assert all_preds is None and len({(int(a), int(b)) for a, b in zip(preds, z)}) == k
    args = mu.build_parser().parse_args(["--cluster", "GMM_FULL", "--n_cluster", str(k), "--pca_dim", "16"])
    lab = np.arange(len(z)) % 3 == 0                            # main_ptsup.py: labelled rows first, clamped, labels for all rows
    targets = z * 10 + 7                                        # the labelled classes need not be 0 .. c-1
    u, l = mu.pca_reduce(args, X[~lab], X[lab])
    all_preds, preds = mu.run_clustering(args, u, l, targets[lab], semi_supervised=True)
    assert all_preds.shape == (len(z),) and np.array_equal(all_preds[lab.sum():], preds)
    assert np.array_equal(all_preds[:lab.sum()], z[lab]) and (preds == z[~lab]).mean() > 0.99


def test_estimate_k_criterion_bic_full(tmp_path):
    import estimate_k
    X, z, k = fc.planted_k_case()
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "extracted_features"))
    torch.save(dict(all_feats=X, mask_lab=np.zeros(len(z), dtype=bool), targets=z), os.path.join(root, "extracted_features", "clip_toy_all.pt"))
    out = estimate_k.main(["--root_dir", root, "--dataset_name", "toy", "--criterion", "bic", "--covariance_type", "full", "--max_classes", "8"])
    with open(os.path.join(root, "cluster", "estimated_k_clip_toy.json")) as fh:
        js = json.load(fh)
    assert out["k"] == js["k"] == k and js["criterion"] == "bic" and js["search_mode"] == "grid"
    assert set(js["scores"]) == {str(K) for K in range(2, 9)}
    assert all(np.isfinite(v["bic"]) and np.isfinite(v["lower_bound"]) for v in js["scores"].values())
    assert min(js["scores"], key=lambda K: js["scores"][K]["bic"]) == str(k)
