"""GPU checks of scd_pca_colsum / scd_pca_gram / scd_pca_transform (scd_amd/csrc/pca.hip), scd_amd.pca.PCA, --pca_dim of main_unsup.py
and estimate_k.py against the float64 restatement and the error model of tests/pca_cases.py: every element within its bound.
docs/design/pca.md has the rules and records the printed error / bound ratios."""
import json
import os

import numpy as np
import pytest
import torch

import pca_cases as pc

pytestmark = pytest.mark.gpu
GRAM = pc.gram_cases()
TRANSFORM = pc.transform_cases()


@pytest.fixture(scope="module")
def ops():
    from scd_amd import ops as o
    return o


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------- column sums and the Gram matrix
@pytest.mark.parametrize("name", list(GRAM))
def test_gram_and_colsum_within_the_bounds(ops, name):
    c = GRAM[name]
    x, a = dev(c["X"]), dev(c["a"])
    g, info = ops.pca_gram(x, a)
    cs = ops.pca_colsum(x, a).cpu().numpy()
    g2, info2 = ops.pca_gram(x, a)
    g = g.cpu().numpy()
    q_g = pc.ratio(g, pc.gram_f64(c["X"], c["a"]), pc.gram_bound(c["X"], c["a"]))
    q_c = pc.ratio(cs, pc.colsum_f64(c["X"], c["a"]), pc.colsum_bound(c["X"], c["a"]))
    print("pca %-22s: error / bound  gram %.3f  colsum %.3f" % (name, q_g, q_c))
    assert g.shape == (c["X"].shape[1],) * 2 and list(info.cpu().numpy()) == [0, 0]
    assert q_g <= 1.0 and q_c <= 1.0
    assert np.array_equal(g, g.T)                               # bit-symmetric
    assert np.array_equal(g, g2.cpu().numpy()) and np.array_equal(cs, ops.pca_colsum(x, a).cpu().numpy())       # two calls, the same bits
    assert np.array_equal(info.cpu().numpy(), info2.cpu().numpy())
    if c["X"].shape == (1, 1):
        assert g[0, 0] == (0.0 if c["a"] is not None else 1.0)


@pytest.mark.parametrize("name", ["ranges_x_tiles", "cap32", "colsum_cap"])
def test_two_calls_return_the_same_bits(ops, name):
    c = GRAM[pc.gram_name(*pc.NAMED_GRAM[name], True)]
    x, a = dev(c["X"]), dev(c["a"])
    (g1, i1), (g2, i2) = ops.pca_gram(x, a), ops.pca_gram(x, a)
    assert np.array_equal(g1.cpu().numpy(), g2.cpu().numpy()) and np.array_equal(i1.cpu().numpy(), i2.cpu().numpy())
    assert np.array_equal(ops.pca_colsum(x, a).cpu().numpy(), ops.pca_colsum(x, a).cpu().numpy())
    assert np.isfinite(g1.cpu().numpy()).all() and np.abs(g1.cpu().numpy()).max() > 0


def test_cached_workspace_holds_no_stale_partials(ops):
    """One range, then the 32 ranges of cap32 through the same cached workspace, then the one range again: the finish kernels read the
    R and RB partials of their own call and nothing a larger call left behind."""
    small, big = GRAM[pc.gram_name(3 * pc.T + 5, 129, True)], GRAM[pc.gram_name(*pc.NAMED_GRAM["cap32"], True)]

    def run(c):
        g, info = ops.pca_gram(dev(c["X"]), dev(c["a"]))
        return g.cpu().numpy(), info.cpu().numpy(), ops.pca_colsum(dev(c["X"]), dev(c["a"])).cpu().numpy()

    a = run(small)
    mid = run(big)
    b = run(small)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert np.isfinite(mid[0]).all() and np.abs(mid[0]).max() > 0


def test_a_non_finite_row_is_counted_once(ops):
    c = pc.nan_case()
    g, info = ops.pca_gram(dev(c["X"]), dev(c["a"]))
    assert list(info.cpu().numpy()) == [1, 0] and not np.isfinite(g.cpu().numpy()).all()


# ------------------------------------------------------------------------------------------------- the projection
@pytest.mark.parametrize("name", list(TRANSFORM))
def test_transform_within_the_bounds(ops, name):
    c = TRANSFORM[name]
    y, info = ops.pca_transform(dev(c["X"]), dev(c["W"]), dev(c["a"]), unit=c["unit"])
    y = y.cpu().numpy()
    ref = pc.transform_f64(c["X"], c["a"], c["W"], c["unit"])
    q = pc.ratio(y, ref, pc.transform_bound(c["X"], c["a"], c["W"], c["unit"]))
    print("pca %-26s: error / bound  y %.3f" % (name, q))
    zero_rows = int((~ref.any(axis=1)).sum()) if c["unit"] else 0
    assert y.shape == ref.shape and y.dtype == np.float32 and list(info.cpu().numpy()) == [0, zero_rows]
    assert q <= 1.0
    y2, _ = ops.pca_transform(dev(c["X"]), dev(c["W"]), dev(c["a"]), unit=c["unit"])
    assert np.array_equal(y, y2.cpu().numpy())


def test_a_row_equal_to_the_shift_is_a_zero_row(ops):
    c = pc.zero_row_case()
    y, info = ops.pca_transform(dev(c["X"]), dev(c["W"]), dev(c["a"]), unit=True)
    y = y.cpu().numpy()
    assert list(info.cpu().numpy()) == [0, 1] and not y[5].any()
    assert pc.ratio(y, pc.transform_f64(c["X"], c["a"], c["W"], True), pc.transform_bound(c["X"], c["a"], c["W"], True)) <= 1.0
    plain, info = ops.pca_transform(dev(c["X"]), dev(c["W"]), dev(c["a"]))
    assert list(info.cpu().numpy()) == [0, 0] and not plain.cpu().numpy()[5].any()
    noshift, _ = ops.pca_transform(dev(c["X"]), dev(c["W"]))
    assert pc.ratio(noshift.cpu().numpy(), pc.transform_f64(c["X"], None, c["W"]), pc.transform_bound(c["X"], None, c["W"])) <= 1.0


def test_limits_are_refused(ops):
    from scd_amd._lib import ScdError
    from scd_amd.pca import PCA
    x = torch.zeros((4, 1025), dtype=torch.float32, device="cuda")
    for call in (lambda: ops.pca_gram(x), lambda: ops.pca_colsum(x), lambda: ops.pca_transform(x, x[:2].contiguous()),
                 lambda: ops.pca_transform(x[:, :8].contiguous(), torch.zeros((1025, 8), dtype=torch.float32, device="cuda")),
                 lambda: ops.pca_gram(x[:, :8].contiguous(), x[0, :9].contiguous())):
        with pytest.raises(ScdError):
            call()
    with pytest.raises(ValueError, match="1024"):
        PCA(2).fit(x)


# ------------------------------------------------------------------------------------------------- the estimator
@pytest.mark.parametrize("shape", pc.FIT_SHAPES)
@pytest.mark.parametrize("whiten", [False, True])
def test_fit_within_weyl_and_davis_kahan(shape, whiten):
    from scd_amd.pca import PCA
    n, d, m = shape
    X, held = pc.fit_case(*shape)
    p = PCA(n_components=m, whiten=whiten).fit(X)
    a = p._shift.cpu().numpy()                                  # the restatement at the device's own rounded mean
    assert np.abs(a.astype(np.float64) - X.astype(np.float64).mean(axis=0)).max() <= pc.U * np.abs(a).max() * 1.0000001
    ref = pc.fit_f64(X, a, m, whiten=whiten)
    weyl, dk = pc.weyl_bound(X, a), pc.davis_kahan_bound(X, a, m)
    q_l = np.abs(p.explained_variance_ - ref["var"][:m]).max() / weyl
    sine = pc.subspace_sine(ref["comps"][:m], p.components_)
    print("fit %s whiten %d: eigenvalue error / Weyl %.4f, subspace sine %.3g / Davis-Kahan %.3g = %.4f" % (shape, whiten, q_l, sine, dk, sine / dk))
    assert q_l <= 1.0 and sine <= dk
    assert p.components_.shape == (m, d) and p.n_components_ == m and p.n_samples_ == n and p.mean_.shape == (d,)
    assert np.abs(p.mean_ - ref["mean"]).max() <= 2 * pc.colsum_bound(X, a).max() / n + 4 * pc.EPS64 * np.abs(a).max()
    assert np.abs(p.components_ @ p.components_.T - np.eye(m)).max() < 1e-12
    assert (p.components_[np.arange(m), np.abs(p.components_).argmax(axis=1)] > 0).all()            # svd_flip
    assert abs(p.noise_variance_ - ref["noise"]) <= weyl and np.abs(p.singular_values_ - np.sqrt(p.explained_variance_ * (n - 1))).max() < 1e-9
    assert abs(p.explained_variance_ratio_.sum() - ref["ratio"][:m].sum()) <= 2 * d * weyl / ref["var"].sum()
    # held-out rows: within the projection bound of the restatement at the device's own components
    W = p._w.cpu().numpy()
    w64 = p.components_ / np.sqrt(p.explained_variance_)[:, None] if whiten else p.components_
    assert np.array_equal(W, w64.astype(np.float32))            # formed in float64, rounded once
    for unit in (False, True):
        y = p.transform(held, unit=unit).cpu().numpy()
        q = pc.ratio(y, pc.transform_f64(held, a, W, unit), pc.transform_bound(held, a, W, unit))
        print("    transform of %d held-out rows, unit %d: error / bound %.3f" % (len(held), unit, q))
        assert q <= 1.0 and y.shape == (len(held), m)
    # fit_transform is fit then transform, bit for bit
    for unit in (False, True):
        assert np.array_equal(PCA(n_components=m, whiten=whiten).fit_transform(X, unit=unit).cpu().numpy(), p.transform(X, unit=unit).cpu().numpy())
    if whiten:
        assert np.abs(p.transform(X).cpu().numpy().astype(np.float64).var(axis=0, ddof=1) - 1.0).max() < 1e-3
    back = p.inverse_transform(p.transform(held)).cpu().numpy()
    resid = held.astype(np.float64) - back                      # what is lost lies outside the kept subspace, up to the projection's error
    scale = np.sqrt(p.explained_variance_)[None, :] if whiten else 1.0
    assert (np.abs(resid @ p.components_.T) <= pc.transform_bound(held, a, W) * scale + 1e-6).all()


def test_float_and_default_n_components():
    from scd_amd.pca import PCA
    X, _ = pc.fit_case(1200, 33, 4)
    p = PCA(n_components=0.85).fit(X)                           # three components keep 0.80 of the variance, four 0.89
    assert p.n_components_ == pc.fit_f64(X, p._shift.cpu().numpy(), 0.85)["m"] == 4
    full = PCA().fit(X[:20])
    assert full.n_components_ == 20 and full.noise_variance_ == 0.0 and full.components_.shape == (20, 33)
    with pytest.raises(ValueError, match="non-finite"):
        bad = X.copy()
        bad[3, 2] = np.nan
        PCA(2).fit(bad)


# ------------------------------------------------------------------------------------------------- the scripts
def test_main_unsup_pca_dim():
    import importlib
    from sklearn.metrics import adjusted_rand_score
    mu = importlib.import_module("main_unsup")
    X, z, k = pc.km_cache()
    args = mu.build_parser().parse_args(["--cluster", "KM", "--n_cluster", str(k), "--pca_dim", "4"])
    lab = np.arange(len(z)) % 4 == 0                            # the fit sees all rows, labelled first
    u, l = mu.pca_reduce(args, X[~lab], X[lab])
    assert u.shape == (int((~lab).sum()), 4) and l.shape == (int(lab.sum()), 4) and u.dtype == np.float32
    assert np.abs(np.linalg.norm(np.concatenate([u, l]).astype(np.float64), axis=1) - 1.0).max() < 1e-6
    all_preds, preds = mu.run_clustering(args, u, l, z[lab])
    assert all_preds is None and adjusted_rand_score(z[~lab], preds) == 1.0
    args = mu.build_parser().parse_args(["--cluster", "KM", "--n_cluster", str(k), "--pca_dim", "4", "--pca_whiten"])
    u, _ = mu.pca_reduce(args, X, X[:0])
    assert adjusted_rand_score(z, mu.run_clustering(args, u, X[:0], np.zeros(0))[1]) == 1.0


def test_estimate_k_criterion_bic_pca_dim(tmp_path):
    import estimate_k
    X, z, k = pc.km_cache()
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "extracted_features"))
    torch.save(dict(all_feats=X, mask_lab=np.zeros(len(z), dtype=bool), targets=z), os.path.join(root, "extracted_features", "clip_toy_all.pt"))
    out = estimate_k.main(["--root_dir", root, "--dataset_name", "toy", "--criterion", "bic", "--max_classes", "8", "--pca_dim", "4"])
    with open(os.path.join(root, "cluster", "estimated_k_clip_toy.json")) as fh:
        js = json.load(fh)
    print("BIC on the reduced cache: %s" % {K: round(v["bic"], 1) for K, v in js["scores"].items()})
    assert out["k"] == js["k"] == k and js["criterion"] == "bic" and js["pca_dim"] == 4 and js["pca_whiten"] is False
    assert min(js["scores"], key=lambda K: js["scores"][K]["bic"]) == str(k)
