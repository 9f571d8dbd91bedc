"""CPU checks of the PCA restatement (tests/pca_cases.py) against scikit-learn, of its error model and planted mistakes, of the ABI and of
the scripts' arguments.  docs/design/pca.md has the rules."""
import argparse
import os
import re

import numpy as np
import pytest

import pca_cases as pc

GIB = 1 << 30
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAM = pc.gram_cases()
TRANSFORM = pc.transform_cases()


@pytest.fixture(autouse=True)
def needs_the_pca():
    from scd_amd import _lib
    assert "scd_pca_gram" in _lib.SIGNATURES, "the library under test has no PCA: these cases restate its contract"


@pytest.fixture(scope="module")
def L():
    from scd_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------------- the restatement against scikit-learn
@pytest.mark.parametrize("shape", pc.FIT_SHAPES)
def test_restatement_against_scikit_learn(shape):
    """The restatement is the exact PCA of the rows a + c, which differ from x by the one rounding of x - a: |E_ij| <= u |c_ij|.  The
    centred matrix moves by at most eta = ||E||_F <= u ||c||_F in the 2-norm, so each singular value sigma_k moves by at most eta and
    lambda_k = sigma_k^2 / (n - 1) by the relative 2 eta / sigma_k + (eta / sigma_k)^2; the two float64 eigensolvers add
    2 d eps64 lambda_1 / lambda_k.  A float64 tolerance does not apply."""
    from sklearn.decomposition import PCA as SkPCA
    n, d, m = shape
    X, _ = pc.fit_case(*shape)
    a = pc.rounded_mean(X)
    ref = pc.fit_f64(X, a, m)
    sk = SkPCA(n_components=m, svd_solver="covariance_eigh").fit(X.astype(np.float64))
    eta = pc.U * np.linalg.norm(pc.centred(X, a))
    sigma = np.sqrt(sk.explained_variance_ * (n - 1))
    bound = 2 * eta / sigma + (eta / sigma) ** 2 + 2 * d * pc.EPS64 * sk.explained_variance_[0] / sk.explained_variance_
    rel = np.abs(ref["var"][:m] - sk.explained_variance_) / sk.explained_variance_
    print("restatement vs scikit-learn %s: explained variance relative difference %.3g, bound %.3g" % (shape, rel.max(), bound.min()))
    assert (rel <= bound).all() and bound.max() < 1e-5
    assert abs(ref["noise"] - sk.noise_variance_) <= bound.max() * ref["var"][0]
    assert np.abs(ref["mean"] - sk.mean_).max() <= pc.U * np.abs(pc.centred(X, a)).max()
    assert np.abs(ref["sing"][:m] - sk.singular_values_).max() <= eta + 1e-9
    # same subspace and same signs: the components agree up to the perturbation over the gap
    gap = sk.explained_variance_[m - 1] - ref["var"][m]
    sine = pc.subspace_sine(sk.components_, ref["comps"][:m])
    assert sine <= 2 * (2 * eta * sigma[0] + eta * eta) / (n - 1) / gap + 1e-12
    assert (np.sign(np.sum(ref["comps"][:m] * sk.components_, axis=1)) == 1).all()


def test_float_n_components_and_noise_variance_follow_scikit_learn():
    from sklearn.decomposition import PCA as SkPCA
    from scd_amd.pca import choose_n_components
    X, _ = pc.fit_case(1200, 33, 4)
    a = pc.rounded_mean(X)
    for frac in (0.5, 0.8, 0.95, 0.999):
        sk = SkPCA(n_components=frac, svd_solver="covariance_eigh").fit(X.astype(np.float64))
        ref = pc.fit_f64(X, a, frac)
        assert ref["m"] == sk.n_components_ == choose_n_components(frac, ref["ratio"], 1200, 33)
        assert abs(ref["noise"] - sk.noise_variance_) <= 1e-6 * sk.noise_variance_ + 1e-300
    assert choose_n_components(None, ref["ratio"], 20, 33) == 20 and choose_n_components(7, ref["ratio"], 1200, 33) == 7
    assert pc.fit_f64(X, a, None)["noise"] == 0.0
    for bad in (0, 34, 1.5):
        with pytest.raises(ValueError):
            choose_n_components(bad, ref["ratio"], 1200, 33)


def test_svd_flip_signs():
    import torch
    from sklearn.utils.extmath import svd_flip
    from scd_amd.pca import spectrum, svd_flip_rows
    rs = np.random.RandomState(3)
    v = rs.standard_normal((6, 9))
    v[2, 4] = -7.0
    v[3, 1], v[3, 5] = -5.0, 5.0                                 # a tie in magnitude: the first one decides
    _, want = svd_flip(None, v.copy(), u_based_decision=False)
    got = svd_flip_rows(torch.as_tensor(v)).numpy()
    assert np.array_equal(got, want) and np.array_equal(pc.svd_flip_rows(v.copy()), want)
    assert got[2, 4] == 7.0 and got[3, 1] == 5.0
    X, _ = pc.fit_case(1200, 33, 4)
    ref = pc.fit_f64(X, pc.rounded_mean(X), 4)
    var, comps, sing = spectrum(torch.as_tensor(ref["cov"]), 1200)
    assert np.allclose(var.numpy(), ref["var"], rtol=1e-12, atol=1e-15) and (np.diff(var.numpy()) <= 0).all() and (var.numpy() >= 0).all()
    assert pc.subspace_sine(comps.numpy()[:4], ref["comps"][:4]) < 1e-10
    assert (np.abs(comps.numpy()).max(axis=1) == comps.numpy()[np.arange(33), np.abs(comps.numpy()).argmax(axis=1)]).all()


# ------------------------------------------------------------------------------------------------- ABI, limits, arguments
def test_abi_declares_the_pca(L):
    from scd_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "scd_hip.h")).read()
    for sym in ("scd_pca_ws_bytes", "scd_pca_row_tile", "scd_pca_chain_rows", "scd_pca_colsum", "scd_pca_gram", "scd_pca_transform"):
        assert sym in _lib.SIGNATURES and re.search(r"\b%s\(" % sym, hdr) and hasattr(L, sym)
    assert len(_lib.SIGNATURES["scd_pca_colsum"][1]) == 9 and len(_lib.SIGNATURES["scd_pca_gram"][1]) == 10
    assert len(_lib.SIGNATURES["scd_pca_transform"][1]) == 13
    assert L.scd_pca_row_tile() == pc.ROW_TILE and L.scd_pca_chain_rows() == pc.CHAIN_ROWS <= 1024
    assert callable(ops.pca_colsum) and callable(ops.pca_gram) and callable(ops.pca_transform)


def test_workspace_limits(L):
    nb = L.scd_pca_ws_bytes(126976, 768, 1024)
    print("scd_pca workspace at 126,976 x 768, m = 1024: %.1f MB" % (nb / 1e6))
    assert 0 < nb <= 2 * GIB
    assert L.scd_pca_ws_bytes(1, 1, 1) > 0 and 0 < L.scd_pca_ws_bytes((1 << 31) - 1, 1024, 1024)
    assert L.scd_pca_ws_bytes(1, 768, 64) <= L.scd_pca_ws_bytes(126976, 768, 64)
    for n, d, m in ((0, 8, 4), (1 << 31, 8, 4), (10, 0, 4), (10, 1025, 4), (10, 8, 0), (10, 8, 1025)):
        assert L.scd_pca_ws_bytes(n, d, m) == 0


def test_estimator_validates_its_arguments():
    from scd_amd.pca import PCA
    with pytest.raises(ValueError, match="1024"):
        PCA(n_components=1025)
    with pytest.raises(ValueError):
        PCA(n_components="mle")
    with pytest.raises(ValueError, match="not fitted"):
        PCA(2).transform(np.zeros((3, 2), np.float32))
    with pytest.raises(ValueError, match="not fitted"):
        PCA(2).inverse_transform(np.zeros((3, 2)))


def test_scripts_accept_the_new_options():
    import estimate_k
    import main_ptsup
    import main_unsup
    a = main_unsup.build_parser().parse_args([])
    assert (a.pca_dim, a.pca_whiten) == (0, False) and main_unsup.pca_tag(a) == ""
    base = main_unsup.cluster_result_name(a)
    assert base == "KM_dino_vit_imagenet_1000_1000.pt"
    a = main_unsup.build_parser().parse_args(["--pca_dim", "32"])
    assert main_unsup.cluster_result_name(a) == "KM_dino_vit_imagenet_1000_1000_pca32.pt"
    a = main_unsup.build_parser().parse_args(["--pca_dim", "32", "--pca_whiten", "--cluster", "HDBSCAN"])
    assert a.pca_whiten is True and main_unsup.cluster_result_name(a) == "HDBSCAN_dino_vit_imagenet_1000_mcs5_pca32w.pt"
    # a Namespace of the caller's own, without the new attributes: the name of today
    ns = argparse.Namespace(cluster="KM", feat_model="dino_vit", dataset_name="cub", n_cluster=200, clip_model="ViT-B/16")
    assert main_unsup.cluster_result_name(ns) == "KM_dino_vit_cub_200.pt"
    p = main_ptsup.build_parser().parse_args(["--pca_dim", "16"])
    assert p.pca_dim == 16 and p.cluster == "ConSSKM" and main_unsup.pca_tag(p) == "_pca16"
    e = estimate_k.parse_args(["--root_dir", "r", "--dataset_name", "d", "--criterion", "bic", "--pca_dim", "4", "--pca_whiten"])
    assert (e.pca_dim, e.pca_whiten, e.search_mode) == (4, True, "grid")
    assert estimate_k.parse_args(["--root_dir", "r", "--dataset_name", "d"]).pca_dim == 0
    # without the flag the features pass through untouched: the same objects
    u, l = np.zeros((3, 5), np.float32), np.zeros((0, 5), np.float32)
    assert main_unsup.pca_reduce(main_unsup.build_parser().parse_args([]), u, l) == (u, l)
    assert main_unsup.pca_reduce(ns, u, l) == (u, l)


# ------------------------------------------------------------------------------------------------- the bounds are not vacuous
@pytest.mark.parametrize("shape", pc.FIT_SHAPES)
def test_davis_kahan_bound_is_small_on_the_fit_cases(shape):
    X, _ = pc.fit_case(*shape)
    a = pc.rounded_mean(X)
    dk, weyl = pc.davis_kahan_bound(X, a, shape[2]), pc.weyl_bound(X, a)
    lam = pc.fit_f64(X, a, shape[2])["var"]
    print("fit %s: Weyl bound %.3g (lambda_m %.3g, lambda_m+1 %.3g), Davis-Kahan bound %.3g" % (shape, weyl, lam[shape[2] - 1], lam[shape[2]], dk))
    assert 0 < dk < 0.01 and weyl < 0.01 * lam[shape[2] - 1]


def test_cases_cover_what_they_claim():
    assert len(GRAM) == 2 * len(pc.GRAM_SHAPES) and len(TRANSFORM) == 3 * len(pc.TRANSFORM_SHAPES)
    for c in GRAM.values():
        assert c["X"].dtype == np.float32 and np.abs(np.linalg.norm(c["X"].astype(np.float64), axis=1) - 1).max() < 1e-6
    one = GRAM[pc.gram_name(1, 1, True)]
    assert pc.gram_f64(one["X"], one["a"])[0, 0] == 0.0 and pc.gram_f64(one["X"], None)[0, 0] == 1.0
    # the rounded mean leaves a residual column sum that is not zero, and the mean matters
    big = GRAM[pc.gram_name(231, 768, True)]
    cs = pc.colsum_f64(big["X"], big["a"])
    assert 0 < np.abs(cs).max() < 231 * pc.U and np.abs(big["a"]).max() > 0.01
    nan = pc.nan_case()
    assert (~np.isfinite(nan["X"])).any(axis=1).sum() == 1 and not np.isfinite(nan["X"][7, [3, 128]]).any()
    z = pc.zero_row_case()
    y = pc.transform_f64(z["X"], z["a"], z["W"], unit=True)
    assert not y[5].any() and (np.abs(np.linalg.norm(np.delete(y, 5, axis=0), axis=1) - 1) < 1e-12).all()
    assert pc.transform_bound(z["X"], z["a"], z["W"], unit=True)[5].max() == 0.0
    for name, c in TRANSFORM.items():
        b = pc.transform_bound(c["X"], c["a"], c["W"], c["unit"])
        y = pc.transform_f64(c["X"], c["a"], c["W"], c["unit"])
        if c["X"].shape[0] > 1:                                 # (the one-row case is its own mean: c = 0, an exact zero row)
            assert np.isfinite(b).all() and (b <= 1e-2 * np.abs(y).max()).all(), name        # far below any planted mistake
    assert pc.phantom_columns(32) == (96, 32) and pc.phantom_columns(257) == (512 - 288, 288) and pc.phantom_columns(1024) == (0, 1024)
    assert pc.phantom_columns(129) == (96, 160) and pc.phantom_columns(256) == (0, 256) and pc.phantom_columns(545) == (448, 576)


def test_km_cache_is_recovered_by_the_restatement_and_scikit_learn():
    """The script test's cache: the float64 restatement's four unit-normalised components and scikit-learn's KMeans give the planted
    partition, and a diagonal mixture's BIC has its minimum at the planted K."""
    from sklearn.cluster import KMeans
    from sklearn.metrics import adjusted_rand_score
    from sklearn.mixture import GaussianMixture
    X, z, k = pc.km_cache()
    assert X.shape == (400, 96) and k == 5
    a = pc.rounded_mean(X)
    ref = pc.fit_f64(X, a, 4)
    assert ref["ratio"][:4].sum() > 0.9
    y = pc.transform_f64(X, a, ref["W"], unit=True)
    assert adjusted_rand_score(z, KMeans(n_clusters=k, n_init=10, random_state=0).fit(y).labels_) == 1.0
    bic = {K: GaussianMixture(K, covariance_type="diag", random_state=0).fit(y).bic(y) for K in range(2, 9)}
    print("BIC of the reduced cache: %s" % {K: round(v, 1) for K, v in bic.items()})
    assert min(bic, key=bic.get) == k and min(v for K, v in bic.items() if K != k) - bic[k] > 40


# ------------------------------------------------------------------------------------------------- the planted mistakes
def _fit_inputs(name):
    shift0 = name.endswith("-shift0")
    n, d, m = (int(t[1:]) for t in name.replace("-shift0", "").split("_"))
    X, held = pc.fit_case(n, d, m)
    return X, held, (None if shift0 else pc.rounded_mean(X)), m


@pytest.mark.parametrize("mistake,case,kind", pc.mistake_cases(),
                         ids=[m if pc.MISTAKES[m][1] == case else "%s-%s" % (m, case) for m, case, _ in pc.mistake_cases()])
def test_planted_mistake_breaks_its_bound(mistake, case, kind):
    what = pc.MISTAKES[mistake][0]
    if kind == "gram":
        c = GRAM[case]
        q = pc.ratio(pc.gram_f64(c["X"], c["a"], mistake), pc.gram_f64(c["X"], c["a"]), pc.gram_bound(c["X"], c["a"]))
    elif kind == "colsum":
        c = GRAM[case]
        q = pc.ratio(pc.colsum_f64(c["X"], c["a"], mistake), pc.colsum_f64(c["X"], c["a"]), pc.colsum_bound(c["X"], c["a"]))
    elif kind == "transform" and case in TRANSFORM:
        c = TRANSFORM[case]
        q = pc.ratio(pc.transform_f64(c["X"], c["a"], c["W"], c["unit"], mistake), pc.transform_f64(c["X"], c["a"], c["W"], c["unit"]),
                     pc.transform_bound(c["X"], c["a"], c["W"], c["unit"]))
    else:
        X, held, a, m = _fit_inputs(case)
        good = pc.fit_f64(X, a, m, whiten=kind == "transform_whitened")
        bad = pc.fit_f64(X, a, m, whiten=kind == "transform_whitened", mistake=mistake)
        if kind == "weyl":
            q = np.abs(bad["var"] - good["var"]).max() / pc.weyl_bound(X, a)
        elif kind == "davis_kahan":
            q = pc.subspace_sine(good["comps"][:m], bad["comps"][:m]) / pc.davis_kahan_bound(X, a, m)
        else:                                                   # the projection of the held-out rows, unit rows as the scripts ask for
            q = pc.ratio(pc.transform_f64(held, a, bad["W"], True), pc.transform_f64(held, a, good["W"], True),
                         pc.transform_bound(held, a, good["W"], True))
    print("planted %-22s (%s) on %s: difference / bound %.3g" % (mistake, what, case, q))
    assert q > 1.0
    if mistake == "no_correction":                              # it matters only away from the mean: at the rounded mean it hides
        X, _, _, m = _fit_inputs(case)
        a = pc.rounded_mean(X)
        hidden = np.abs(pc.fit_f64(X, a, m, mistake=mistake)["var"] - pc.fit_f64(X, a, m)["var"]).max() / pc.weyl_bound(X, a)
        print("   the same mistake at the rounded mean: difference / bound %.3g" % hidden)
        assert hidden < 1.0
