"""GPU checks of scd_gmm_em_step / scd_gmm_predict (scd_amd/csrc/gmm.hip), scd_amd.gmm.GaussianMixture, main_unsup.py --cluster GMM and
estimate_k.py --criterion bic against the float64 restatement and the error model of tests/gmm_cases.py: every element within its
bound, no row excused.  docs/design/gmm.md has the rules and records the printed error / bound ratios."""
import json
import os

import numpy as np
import pytest
import torch

import gmm_cases as gc

pytestmark = pytest.mark.gpu
CASES = gc.all_cases()


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
    k = case["a"].shape[0]
    if case["hard"]:
        ll, nk, s1, s2, pred, info = ops.gmm_em_step(dev(case["X"]), None, None, None, y=dev(case["y"]), sample_weight=dev(case["sw"]), n_components=k)
    else:
        ll, nk, s1, s2, pred, info = ops.gmm_em_step(dev(case["X"]), dev(case["a"]), dev(case["B"]), dev(case["C"]), y=dev(case["y"]),
                                                     sample_weight=dev(case["sw"]), want_pred=True)
    return dict(ll=float(ll.item()), nk=nk.cpu().numpy(), s1=s1.cpu().numpy(), s2=s2.cpu().numpy(),
                pred=None if pred is None else pred.cpu().numpy().astype(np.int64), info=info.cpu().numpy())


# ------------------------------------------------------------------------------------------------- every case within its bounds
@pytest.mark.parametrize("name", list(CASES))
def test_step_within_the_bounds(ops, name):
    case = CASES[name]
    got = run(ops, case)
    n, d = case["X"].shape
    k = case["a"].shape[0]
    if case["hard"]:                                            # one-hots times float32 x: only the chain's rounding
        ref = gc.reference(case)
        ar, X64 = np.abs(ref["r"]), case["X"].astype(np.float64)
        bd = dict(ref=ref, ll=0.0, nk=gc.gamma(gc.CHAIN_ROWS) * ar.sum(axis=0), s1=gc.gamma(gc.CHAIN_ROWS) * (ar.T @ np.abs(X64)),
                  s2=gc.gamma(gc.CHAIN_ROWS + 1) * (ar.T @ (X64 * X64)))
    else:
        bd = gc.bounds(case["X"], case["y"], case["a"], case["B"], case["C"], case["sw"])
    q = gc.ratios(got, bd)
    print("gmm %-26s n %5d d %4d k %4d: error / bound  ll %.3f  nk %.3f  s1 %.3f  s2 %.3f" % (name, n, d, k, q["ll"], q["nk"], q["s1"], q["s2"]))
    assert list(got["info"]) == list(bd["ref"]["info"])
    if name.endswith("bad_labels"):
        assert got["info"][0] == 2
    assert abs(got["ll"] - bd["ref"]["ll"]) <= bd["ll"]
    for key in ("nk", "s1", "s2"):
        assert (np.abs(got[key] - bd["ref"][key]) <= bd[key]).all(), key
    if case["hard"]:
        assert got["ll"] == 0.0 and got["pred"] is None and np.array_equal(got["nk"], bd["ref"]["nk"])
        return
    dec = gc.decided_rows(bd, case["exact_ties"])               # pred_out covers every row, whatever its label
    assert (~dec).mean() <= case.get("undecided_cap", 0.0)      # 0 below f32mm_plan.LARGE_N rows: no row is excused there
    assert np.array_equal(got["pred"][dec], bd["ref"]["pred"][dec])
    if "unreached" in case:                                     # no underflowing mass reaches it: exact zeros
        j = case["unreached"]
        assert got["nk"][j] == 0.0 and not got["s1"][j].any() and not got["s2"][j].any()
    if name == "identical":
        assert np.array_equal(got["s1"][3], got["s1"][17]) and got["nk"][3] == got["nk"][17] > 0


def test_bad_labels_equal_the_unlabelled_result(ops):
    case = gc.shape_case("k33", "bad_labels")
    a, b = run(ops, case), run(ops, gc.bad_labels_as_unlabelled(case))
    assert list(a["info"]) == [2, 0] and list(b["info"]) == [0, 0]
    assert a["ll"] == b["ll"] and all(np.array_equal(a[q], b[q]) for q in ("nk", "s1", "s2", "pred"))


def test_two_calls_return_the_same_bits(ops, name="four_chains-weights"):
    case = CASES[name]
    a, b = run(ops, case), run(ops, case)
    assert a["ll"] == b["ll"] and all(np.array_equal(a[q], b[q]) for q in ("nk", "s1", "s2", "pred", "info"))
    assert np.isfinite(a["s2"]).all() and np.abs(a["s1"]).max() > 0


@pytest.mark.parametrize("name", ["ranges_x_tiles-weights", "cap32-weights", "colsum_cap-weights"])
def test_two_calls_return_the_same_bits_over_the_range_plans(ops, name):
    test_two_calls_return_the_same_bits(ops, name)


def test_cached_workspace_holds_no_stale_partials(ops):
    """One range, then the 32 ranges of cap32 through the same cached workspace, then the one range again: the finish kernel reads the R
    partials of its own call and nothing a larger call left behind."""
    small, big = CASES["four_chains-weights"], CASES["cap32-weights"]
    a = run(ops, small)
    mid = run(ops, big)
    b = run(ops, small)
    assert a["ll"] == b["ll"] and all(np.array_equal(a[q], b[q]) for q in ("nk", "s1", "s2", "pred", "info"))
    assert np.isfinite(mid["s2"]).all() and np.abs(mid["s1"]).max() > 0


@pytest.mark.parametrize("name", ["n1_d1_k1-unlabelled", "k33-mixed", "d768_k100-unlabelled", "full_width-unlabelled", "four_chains-weights",
                                  "two_ranges-unlabelled", "variance_span", "far_rows", "identical", "nt2_phantom-unlabelled",
                                  "nt2_exact-mixed", "nt8_phantom-unlabelled", "ranges_x_tiles-unlabelled"])
def test_predict_equals_the_steps_argmax(ops, name):
    case = CASES[name]
    pred, row_ll, resp = ops.gmm_predict(dev(case["X"]), dev(case["a"]), dev(case["B"]), dev(case["C"]), want_ll=True, want_resp=True)
    got = run(ops, case)
    assert np.array_equal(pred.cpu().numpy(), got["pred"])
    bd = gc.bounds(case["X"], None, case["a"], case["B"], case["C"])
    resp, row_ll = resp.cpu().numpy(), row_ll.cpu().numpy()
    assert resp.shape == (case["X"].shape[0], case["a"].shape[0])
    q_r, q_l = gc.ratio(resp, bd["ref"]["p"], bd["resp"]), gc.ratio(row_ll, bd["ref"]["lse"], bd["row_ll"])
    print("predict %-22s: error / bound  resp %.3f  row_ll %.3f" % (name, q_r, q_l))
    assert (np.abs(resp - bd["ref"]["p"]) <= bd["resp"]).all() and (np.abs(row_ll - bd["ref"]["lse"]) <= bd["row_ll"]).all()
    if name == "identical":
        assert np.array_equal(resp[:, 3], resp[:, 17])
    only = ops.gmm_predict(dev(case["X"]), dev(case["a"]), dev(case["B"]), dev(case["C"]))
    assert only[1] is None and only[2] is None and np.array_equal(only[0].cpu().numpy(), got["pred"])


def test_limits_are_refused(ops):
    from scd_amd._lib import ScdError, SCD_EINVAL
    x = torch.zeros((4, 1025), dtype=torch.float32, device="cuda")
    p = torch.zeros((3, 1025), dtype=torch.float32, device="cuda")
    with pytest.raises(ScdError) as e:
        ops.gmm_em_step(x, p[:, 0].contiguous(), p, p)
    assert e.value.code == SCD_EINVAL
    with pytest.raises(ScdError):
        ops.gmm_predict(x[:, :8].contiguous(), p[:, 0].contiguous(), p[:, :9].contiguous(), p[:, :8].contiguous())
    with pytest.raises(ScdError):
        ops.gmm_em_step(x[:, :8].contiguous(), None, None, None, y=None, n_components=3)         # the hard M-step needs labels


# ------------------------------------------------------------------------------------------------- a fit, step by step through ops
def test_steps_of_a_fit_follow_the_restatement(ops):
    """EM driven by hand: every device step is within the bounds of the restatement taken from the SAME parameters, and the trace of
    the log-likelihood is nondecreasing up to twice the likelihood bound."""
    from scd_amd import gmm
    X, _, start = gc.blob_case("n1200_d8_k4")
    w, mu, cov = (torch.as_tensor(t).cuda() for t in start)
    x = dev(X)
    trace, allowed, worst = [], [], {}
    for _ in range(6):
        a, B, C = gmm.kernel_params(w, mu, cov)
        ll, nk, s1, s2, _, info = ops.gmm_em_step(x, a, B, C)
        got = dict(ll=float(ll.item()), nk=nk.cpu().numpy(), s1=s1.cpu().numpy(), s2=s2.cpu().numpy())
        bd = gc.bounds(X, None, a.cpu().numpy(), B.cpu().numpy(), C.cpu().numpy())
        q = gc.ratios(got, bd)
        worst = {key: max(v, worst.get(key, 0.0)) for key, v in q.items()}
        assert all(v <= 1.0 for v in q.values()) and not info.cpu().numpy().any()
        trace.append(got["ll"])
        allowed.append(bd["ll"])
        w, mu, cov = gmm.m_step(nk, s1, s2, "diag", 1e-6)
    print("stepwise fit: largest error / bound over 6 steps %s" % {key: round(v, 4) for key, v in worst.items()})
    for i in range(1, len(trace)):
        assert trace[i] >= trace[i - 1] - 2.0 * max(allowed[i], allowed[i - 1])


# ------------------------------------------------------------------------------------------------- the estimator
@pytest.mark.parametrize("covariance_type", ["diag", "spherical"])
@pytest.mark.parametrize("name", list(gc.FIT_CASES))
def test_fit_from_an_explicit_start(name, covariance_type):
    from scd_amd.gmm import GaussianMixture
    X, _, start = gc.blob_case(name)
    (wi, mi, pi), (w0, mu0, c0) = gc.start_for(start, covariance_type)
    ref = gc.fit_f64(X, w0, mu0, c0, covariance_type, float32_params=True)
    gm = GaussianMixture(n_components=len(wi), covariance_type=covariance_type, weights_init=wi, means_init=mi, precisions_init=pi).fit(X)
    assert gm.converged_ and gm.n_iter_ == ref["n_iter"] and len(gm.lower_bounds_) == gm.n_iter_
    d = X.shape[1]
    a, B, C = (t.cpu().numpy() for t in gm._abc)
    bd = gc.bounds(X, None, a, B, C)                            # at the device's own final float32 parameters
    dec = gc.decided_rows(bd)
    labels = gm.predict(X).cpu().numpy()
    print("fit %-14s %-9s: %d iterations, lower bound %.9g (restatement %.9g), %d rows excused, bic %.9g"
          % (name, covariance_type, gm.n_iter_, gm.lower_bound_, ref["lower_bound"], int((~dec).sum()), gm.bic(X)))
    assert dec.all() and np.array_equal(labels, bd["ref"]["pred"]) and np.array_equal(gm.labels_, labels)
    assert np.array_equal(labels, ref["labels"])
    want_bic = -2.0 * (bd["ref"]["lse"].sum() + X.shape[0] * gc.shift(d)) + gc.n_parameters(len(wi), d, covariance_type) * np.log(X.shape[0])
    assert abs(gm.bic(X) - want_bic) <= 2.0 * bd["row_ll"].sum()
    assert abs(gm.aic(X) - (want_bic - gc.n_parameters(len(wi), d, covariance_type) * (np.log(X.shape[0]) - 2.0))) <= 2.0 * bd["row_ll"].sum()
    assert gm.covariances_.shape == ref["cov"].shape and gm.means_.shape == ref["mu"].shape
    assert np.allclose(gm.precisions_ * gm.covariances_, 1.0) and abs(gm.weights_.sum() - 1.0) < 1e-12
    proba = gm.predict_proba(X).cpu().numpy()
    assert (np.abs(proba - bd["ref"]["p"]) <= bd["resp"]).all() and np.abs(proba.sum(axis=1) - 1.0).max() < 1e-4
    assert abs(gm.score(X) - (bd["ref"]["lse"].mean() + gc.shift(d))) <= bd["row_ll"].mean()


def test_semi_supervised_fit_keeps_the_clamped_rows_and_helps_the_rest():
    from scd_amd.gmm import GaussianMixture
    X, z, y, start = gc.overlap_case()
    (wi, mi, pi), _ = gc.start_for(start, "diag")
    kw = dict(n_components=4, weights_init=wi, means_init=mi, precisions_init=pi)
    unsup = GaussianMixture(**kw).fit(X)
    semi = GaussianMixture(**kw).fit(X, y)
    lab, rest = y >= 0, y < 0
    assert semi.converged_ and np.array_equal(semi.labels_[lab], y[lab])
    acc_u, acc_s = (unsup.labels_[rest] == z[rest]).mean(), (semi.labels_[rest] == z[rest]).mean()
    print("accuracy on the unlabelled rows: unsupervised %.3f, semi-supervised %.3f" % (acc_u, acc_s))
    assert acc_s >= acc_u and acc_s > 0.8
    a, B, C = (t.cpu().numpy() for t in semi._abc)
    slack = 2.0 * gc.bounds(X, y, a, B, C)["ll"] / len(y)       # the complete-data likelihood rises, up to twice its bound
    assert (np.diff(semi.lower_bounds_) >= -slack).all()


def test_kmeans_and_random_starts_and_an_unconverged_fit():
    from scd_amd.gmm import ConvergenceWarning, GaussianMixture
    X, z, k = gc.planted_k_case()
    gm = GaussianMixture(n_components=k, random_state=0).fit(X)
    assert gm.converged_ and len(np.unique(gm.labels_)) == k
    pairs = {(int(a), int(b)) for a, b in zip(gm.labels_, z)}
    assert len(pairs) == k                                      # well-separated blobs: the components are the blobs
    y = np.where(np.arange(len(z)) % 4 == 0, z, -1)
    semi = GaussianMixture(n_components=k, random_state=0).fit(X, y)
    assert np.array_equal(semi.labels_[y >= 0], y[y >= 0]) and (semi.labels_ == z).mean() > 0.99
    with pytest.warns(ConvergenceWarning):
        r = GaussianMixture(n_components=k, init_params="random", random_state=3, max_iter=2, n_init=2).fit(X)
    assert not r.converged_ and r.n_iter_ == 2 and np.isfinite(r.lower_bound_)


# ------------------------------------------------------------------------------------------------- the scripts
def test_main_unsup_cluster_gmm():
    import importlib
    mu = importlib.import_module("main_unsup")
    X, z, k = gc.planted_k_case()
    args = mu.build_parser().parse_args(["--cluster", "GMM", "--n_cluster", str(k)])
    all_preds, preds = mu.run_clustering(args, X, X[:0], np.zeros(0))
    assert all_preds is None and len({(int(a), int(b)) for a, b in zip(preds, z)}) == k
    lab = np.arange(len(z)) % 3 == 0                            # main_ptsup.py: labelled rows first, clamped, labels for all rows
    targets = z * 10 + 7                                        # the labelled classes need not be 0 .. c-1
    all_preds, preds = mu.run_clustering(args, X[~lab], X[lab], targets[lab], semi_supervised=True)
    assert all_preds.shape == (len(z),) and np.array_equal(all_preds[lab.sum():], preds)
    assert np.array_equal(all_preds[:lab.sum()], z[lab]) and (preds == z[~lab]).mean() > 0.99


def test_estimate_k_criterion_bic(tmp_path):
    import estimate_k
    X, z, k = gc.planted_k_case()
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "extracted_features"))
    torch.save(dict(all_feats=X, mask_lab=np.zeros(len(z), dtype=bool), targets=z), os.path.join(root, "extracted_features", "clip_toy_all.pt"))
    out = estimate_k.main(["--root_dir", root, "--dataset_name", "toy", "--criterion", "bic", "--max_classes", "8"])
    with open(os.path.join(root, "cluster", "estimated_k_clip_toy.json")) as fh:
        js = json.load(fh)
    assert out["k"] == js["k"] == k and js["criterion"] == "bic" and js["search_mode"] == "grid"
    assert set(js["scores"]) == {str(K) for K in range(2, 9)}
    assert all(np.isfinite(v["bic"]) and np.isfinite(v["lower_bound"]) for v in js["scores"].values())
    assert min(js["scores"], key=lambda K: js["scores"][K]["bic"]) == str(k)
