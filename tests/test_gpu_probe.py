"""GPU checks of scd_probe_loss_grad / scd_probe_predict (scd_amd/csrc/probe.hip), scd_amd.probe.LinearProbe and score_features.py
--probe against the float64 restatement and the error model of tests/probe_cases.py: every element within its bound, no element
excused.  docs/design/probe.md has the rules and records the printed error / bound ratios."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import probe_cases as pc

pytestmark = pytest.mark.gpu
CASES = pc.all_cases()


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
    loss, gW, gb, pred, info = ops.probe_loss_grad(dev(case["X"]), dev(case["y"]), dev(case["W"]), dev(case["b"]), dev(case["sw"]), want_pred=True)
    return dict(loss=float(loss.item()), gW=gW.cpu().numpy(), gb=None if gb is None else gb.cpu().numpy(), pred=pred.cpu().numpy().astype(np.int64),
                info=info.cpu().numpy())


# ------------------------------------------------------------------------------------------------- every case within its bounds
@pytest.mark.parametrize("name", list(CASES))
def test_loss_and_gradient_within_the_bounds(ops, name):
    case = CASES[name]
    got = run(ops, case)
    ref_case = pc.without_bad_rows(case)                        # rows with a label outside [0, c) contribute nothing
    bd = pc.bounds(ref_case["X"], ref_case["y"], ref_case["W"], ref_case["b"], ref_case["sw"])
    q = pc.ratios(got, bd)
    print("probe %-24s n %5d d %4d c %4d: error / bound  loss %.3f  gW %.3f  gb %s"
          % (name, case["X"].shape[0], case["X"].shape[1], case["W"].shape[0], q["loss"], q["gW"], "%.3f" % q["gb"] if "gb" in q else "-"))
    assert list(got["info"]) == [int(((case["y"] < 0) | (case["y"] >= case["W"].shape[0])).sum()), 0]
    if name.endswith("bad_labels"):
        assert got["info"][0] == 2
    assert abs(got["loss"] - bd["ref"]["loss"]) <= bd["loss"]
    assert (np.abs(got["gW"] - bd["ref"]["gW"]) <= bd["gW"]).all()
    if case["b"] is None:
        assert got["gb"] is None
    else:
        assert (np.abs(got["gb"] - bd["ref"]["gb"]) <= bd["gb"]).all()
    full = pc.bounds(case["X"], case["y"], case["W"], case["b"], case["sw"])       # pred_out covers every row, whatever its label
    dec = pc.decided_rows(full, case["exact_ties"])
    assert (~dec).mean() <= case.get("undecided_cap", 0.0)      # 0 below f32mm_plan.LARGE_N rows: no row is excused there
    assert np.array_equal(got["pred"][dec], full["ref"]["pred"][dec])
    if name == "all_equal":
        assert (got["pred"] == 0).all() and abs(got["loss"] - case["X"].shape[0] * np.log(case["W"].shape[0])) <= bd["loss"]


def test_two_calls_return_the_same_bits(ops, name="four_chains-weights"):
    case = CASES[name]
    a, b = run(ops, case), run(ops, case)
    assert a["loss"] == b["loss"] and np.array_equal(a["gW"], b["gW"]) and np.array_equal(a["gb"], b["gb"])
    assert np.array_equal(a["pred"], b["pred"]) and np.array_equal(a["info"], b["info"])
    assert np.isfinite(a["gW"]).all() and np.abs(a["gW"]).max() > 0


@pytest.mark.parametrize("name", ["ranges_x_tiles-weights", "cap32-weights", "colsum_cap-weights"])
def test_two_calls_return_the_same_bits_over_the_range_plans(ops, name):
    test_two_calls_return_the_same_bits(ops, name)


def test_cached_workspace_holds_no_stale_partials(ops):
    """One range, then the 32 ranges of cap32 through the same cached workspace, then the one range again: the finish kernels read the R
    partials of their own call and nothing a larger call left behind."""
    small, big = CASES["four_chains-weights"], CASES["cap32-weights"]
    a = run(ops, small)
    mid = run(ops, big)
    b = run(ops, small)
    assert a["loss"] == b["loss"] and all(np.array_equal(a[q], b[q]) for q in ("gW", "gb", "pred", "info"))
    assert np.isfinite(mid["gW"]).all() and np.abs(mid["gW"]).max() > 0


@pytest.mark.parametrize("name", ["n1_d1_c2-base", "c33-base", "d768_c100-no_bias", "full_width-base", "four_chains-base", "large_logit", "ties",
                                  "nt2_phantom-base", "nt2_exact-base", "nt8_phantom-no_bias", "ranges_x_tiles-base"])
def test_predict_equals_the_loss_calls_argmax(ops, name):
    case = CASES[name]
    pred, top = ops.probe_predict(dev(case["X"]), dev(case["W"]), dev(case["b"]), want_top=True)
    got = run(ops, case)
    assert np.array_equal(pred.cpu().numpy(), got["pred"])
    bd = pc.bounds(case["X"], case["y"], case["W"], case["b"], case["sw"])
    t1, t2 = pc.top2_f64(bd["ref"]["z"])
    top = top.cpu().numpy().astype(np.float64)
    err = np.maximum(np.abs(top[:, 0] - t1), np.abs(top[:, 1] - t2))
    print("predict %-20s: largest top-logit error / delta %.3f" % (name, float((err / bd["delta"]).max())))
    assert (err <= bd["delta"]).all()
    assert np.array_equal(ops.probe_predict(dev(case["X"]), dev(case["W"]), dev(case["b"])).cpu().numpy(), got["pred"])


def test_limits_are_refused(ops):
    from scd_amd._lib import ScdError, SCD_EINVAL
    x = torch.zeros((4, 1025), dtype=torch.float32, device="cuda")
    with pytest.raises(ScdError) as e:
        ops.probe_loss_grad(x, torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros((3, 1025), dtype=torch.float32, device="cuda"))
    assert e.value.code == SCD_EINVAL
    with pytest.raises(ScdError):
        ops.probe_predict(x[:, :8].contiguous(), torch.zeros((1, 8), dtype=torch.float32, device="cuda"))


# ------------------------------------------------------------------------------------------------- the fit
@pytest.fixture(scope="module")
def sk_fits():
    """scikit-learn's fit and the float64 restatement's F* of each blob case, computed once."""
    from sklearn.linear_model import LogisticRegression
    out = {}
    for name in pc.FIT_CASES:
        X, y, C = pc.blob_case(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            star = pc.fit_f64(X, y, C=C, fit_intercept=False, tol=1e-9, max_iter=20000)
        sk = LogisticRegression(C=C, tol=1e-10, max_iter=20000).fit(X.astype(np.float64), y)
        out[name] = dict(X=X, y=y, C=C, F_star=star["F"], sk=sk)
    return out


@pytest.mark.parametrize("name", list(pc.FIT_CASES))
def test_fit_without_intercept_reaches_the_minimum(sk_fits, name):
    """F is lambda-strongly convex: F(W) - F* <= |grad F(W)|^2 / (2 lambda), evaluated in float64 at the returned float32 parameters."""
    from scd_amd.probe import LinearProbe
    f = sk_fits[name]
    lam = 1.0 / f["C"]
    lp = LinearProbe(C=f["C"], fit_intercept=False).fit(f["X"], f["y"])
    W32 = lp.coef_.float().cpu().numpy()
    F64, gW, _ = pc.objective_f64(f["X"], f["y"], W32, None, lam)
    loss_b = pc.bounds(f["X"], f["y"], W32, None)["loss"]
    print("fit %-12s no intercept: F - F* = %.3e, allowed %.3e (|g|^2 / 2 lambda = %.3e, loss bound %.3e), %d iterations, %d evaluations"
          % (name, F64 - f["F_star"], float((gW * gW).sum()) / (2 * lam) + loss_b, float((gW * gW).sum()) / (2 * lam), loss_b, lp.n_iter_, lp.n_eval_))
    assert lp.converged_ and lp.n_iter_ < lp.max_iter
    assert F64 - f["F_star"] <= float((gW * gW).sum()) / (2 * lam) + loss_b


@pytest.mark.parametrize("name", list(pc.FIT_CASES))
def test_fit_with_intercept_is_stationary_and_predicts_as_sklearn(sk_fits, name):
    from scd_amd.probe import LinearProbe
    f = sk_fits[name]
    X, y, lam = f["X"], f["y"], 1.0 / f["C"]
    lp = LinearProbe(C=f["C"]).fit(X, y)
    W32, b32 = lp.coef_.float().cpu().numpy(), lp.intercept_.float().cpu().numpy()
    _, gW, gb = pc.objective_f64(X, y, W32, b32, lam)
    bd = pc.bounds(X, y, W32, b32)
    n = X.shape[0]
    print("fit %-12s intercept: max |g64| %.3e (tol n = %.3e), %d iterations, %d evaluations, objective %.9g"
          % (name, max(np.abs(gW).max(), np.abs(gb).max()), lp.tol * n, lp.n_iter_, lp.n_eval_, lp.objective_))
    assert lp.converged_ and lp.n_iter_ < lp.max_iter and lp.n_eval_ >= lp.n_iter_ + 1
    assert (np.abs(gW) <= lp.tol * n + bd["gW"]).all() and (np.abs(gb) <= lp.tol * n + bd["gb"]).all()
    assert lp.grad_norm_ <= lp.tol * n
    pred = lp.predict(X)
    excused, wrong = pc.prediction_check(X, f["sk"].coef_, f["sk"].intercept_, W32, b32, pred)
    print("fit %-12s: %d rows excused, %d wrong, training accuracy %.4f (scikit-learn %.4f)"
          % (name, excused, wrong, lp.score(X, y), f["sk"].score(X.astype(np.float64), y)))
    assert excused == 0 and wrong == 0
    assert np.array_equal(lp.classes_, f["sk"].classes_)
    z = lp.decision_function(X).cpu().numpy()
    assert z.shape == (n, lp.classes_.size) and (lp.classes_[z.argmax(axis=1)] == pred).mean() > 0.99


def test_sample_weights_and_arbitrary_labels():
    """Integer weights are repetitions, and the labels need not be 0 .. c-1."""
    from scd_amd.probe import LinearProbe
    X, y, C = pc.blob_case("n1500_c10")
    X, y = X[:400], y[:400]
    w = (np.arange(400) % 3).astype(np.float32)
    a = LinearProbe(C=C, tol=1e-5).fit(X, y * 7 - 3, sample_weight=w)
    rep = np.repeat(np.arange(400), w.astype(int))
    b = LinearProbe(C=C, tol=1e-5).fit(X[rep], y[rep] * 7 - 3)
    assert a.converged_ and b.converged_ and np.array_equal(a.classes_, b.classes_) and a.classes_[0] == -3
    assert abs(a.objective_ - b.objective_) <= 2e-5 * abs(b.objective_)
    assert set(np.unique(a.predict(X))) <= set(a.classes_.tolist())


def test_noise_floor_ends_the_fit():
    from scd_amd.probe import LinearProbe
    X, y, C = pc.blob_case("n1500_c10")
    lp = LinearProbe(C=C, tol=0.0, max_iter=400)
    with pytest.warns(UserWarning):
        lp.fit(X[:300, :16].copy(), y[:300])
    print("noise floor: %d iterations, %d evaluations, max |g| %.3e" % (lp.n_iter_, lp.n_eval_, lp.grad_norm_))
    assert not lp.converged_ and lp.n_eval_ <= 400


# ------------------------------------------------------------------------------------------------- score_features.py --probe
def test_score_features_probe(tmp_path, capsys):
    import score_features as sf
    from oracle import synth
    from scd_amd.knn import unit_rows
    from scd_amd.probe import LinearProbe
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "extracted_features"))
    mask = np.zeros(700, dtype=bool)
    mask[:600] = True
    feats = {}
    for name, d, noise in (("dino_vit", 48, 1.0), ("clip", 32, 40.0)):
        x, y, _ = synth.clustered_features(700, d, 6, seed=60, center_seed=160, noise=noise)
        feats[name] = (x, y)
        torch.save(dict(all_feats=x, mask_lab=mask, targets=y), os.path.join(root, "extracted_features", f"{name}_toy_all.pt"))
    argv = ["--root_dir", root, "--dataset_name", "toy", "--feat_models", "clip", "dino_vit", "--k", "10"]
    sf.main(argv)
    kpath = os.path.join(root, "cluster", "knn_score_toy.json")
    plain = open(kpath, "rb").read()
    assert not os.path.exists(os.path.join(root, "cluster", "probe_score_toy.json"))
    capsys.readouterr()
    out = sf.main(argv + ["--probe", "--probe_C", "1.0", "100.0"])
    text = capsys.readouterr().out
    assert open(kpath, "rb").read() == plain                    # the k-NN file does not know about the probe
    with open(os.path.join(root, "cluster", "probe_score_toy.json")) as fh:
        js = json.load(fh)
    assert js["towers"].keys() == {"clip", "dino_vit"} and js["best"] == "dino_vit" == out["probe"]["best"]
    best = {fm: max(f["val_acc"] for f in t["fits"]) for fm, t in js["towers"].items()}
    assert best["dino_vit"] > best["clip"] and best["dino_vit"] > 0.5
    assert js["args"]["probe_C"] == [1.0, 100.0] and [f["C"] for f in js["towers"]["clip"]["fits"]] == [1.0, 100.0]
    x, y = feats["dino_vit"]
    x, y = x[:600], np.asarray(y)[:600]
    train, val = pc.stratified_split(y)
    t = js["towers"]["dino_vit"]
    assert (t["N_train"], t["N_val"], t["D"], t["classes"], t["classes_without_validation"]) == (int(train.sum()), int(val.sum()), 48, 6, 0)
    u = unit_rows(torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).cuda())
    lp = LinearProbe(C=100.0).fit(u[torch.as_tensor(np.flatnonzero(train)).cuda()], y[train])
    acc = lp.score(u[torch.as_tensor(np.flatnonzero(val)).cuda()], y[val])
    assert t["fits"][1]["val_acc"] == acc and t["fits"][1]["n_iter"] == lp.n_iter_ and t["fits"][1]["n_eval"] == lp.n_eval_
    assert ("%9.4f" % acc) in text and "linear probe" in text
