"""CPU checks of the numpy restatement tests/tsne_cases.py that the GPU tests of t-SNE compare the device against: calibration against
scipy's brentq roots, the joint matrix, the gradient, KL, the optimiser, the PCA start and trustworthiness against scikit-learn 1.7,
and every planted mistake of tsne_cases.MISTAKES against the bound of the test that is meant to catch it.  docs/design/tsne.md."""
import os

import numpy as np
import pytest

import tsne_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def small():
    out = {}
    for name in tc.SMALL:
        x, y, perplexity = tc.small_case(name)
        k = tc.neighbours(x.shape[0], perplexity)
        idx, dist2 = tc.graph_f64(x, k)
        out[name] = dict(x=x, y=y, perplexity=perplexity, k=k, idx=idx, dist2=dist2)
    return out


# ------------------------------------------------------------------------------------------------- 1. calibration against roots
@pytest.mark.parametrize("name", list(tc.SMALL))
def test_calibration_rows_are_brentq_roots(small, name):
    from scipy.optimize import brentq
    c = small[name]
    p, beta, unreached = tc.calibrate_f64(c["dist2"], c["perplexity"])
    assert not unreached.any() and np.allclose(p.sum(1), 1.0, rtol=1e-14)
    d = c["dist2"] - c["dist2"].min(1, keepdims=True)
    target = np.log(c["perplexity"])
    worst = 0.0
    for i in range(d.shape[0]):
        root = brentq(lambda b: tc.entropy(d[i:i + 1], np.array([b]))[0] - target, beta[i] * 0.5, beta[i] * 2.0, xtol=1e-300, rtol=1e-13)
        e = np.exp(-d[i] * root)
        want = e / e.sum()
        worst = max(worst, float(np.abs(p[i] / want - 1.0).max()))
    print("calibration %s: largest relative difference to the brentq rows %.3e" % (name, worst))
    assert worst <= 1e-10
    assert abs(np.exp(tc.entropy(d, beta)) / c["perplexity"] - 1.0).max() < 1e-12       # the perplexity of every row is the target


def test_calibration_special_rows():
    for k in (5, 60, 64):
        dist2, perplexity = tc.calibration_case(k)
        p, beta, unreached = tc.calibrate_f64(dist2, perplexity)
        assert np.isfinite(p).all() and np.allclose(p.sum(1), 1.0, rtol=1e-14)
        assert unreached[1] and unreached[3] and unreached.sum() == 2                   # all distances equal; the minimum too often
        assert np.array_equal(p[1], np.full(k, 1.0 / k))
        assert beta[4:20].min() > 1e4 and not unreached[4:20].any()                     # the tight clusters need a large b, and get it
        assert p[0, 1] == p[0, 2] and p[2, 0] == p[2].max()


# ------------------------------------------------------------------------------------------------- 2. the joint matrix against scikit-learn
def sklearn_joint(c):
    from scipy.sparse import csr_matrix
    from sklearn.manifold._t_sne import _joint_probabilities_nn
    n, k = c["idx"].shape
    dist = csr_matrix((c["dist2"].astype(np.float32).reshape(-1), c["idx"].reshape(-1), np.arange(0, n * k + 1, k)), shape=(n, n))
    return _joint_probabilities_nn(dist, c["perplexity"], 0).toarray()


def joint_rel(c, mistake=None):
    want = sklearn_joint(c)
    p, _, _ = tc.calibrate_f64(c["dist2"], c["perplexity"], mistake)
    got = tc.csr_dense(tc.joint_f64(c["idx"], p, mistake), want.shape[0])
    assert ((got > 0) <= (want > 0)).all()                                              # never an entry scikit-learn does not have
    return float((np.abs(got - want)[want > 0] / want[want > 0]).max())


@pytest.mark.parametrize("name", list(tc.SMALL))
def test_joint_matrix_against_sklearn(small, name):
    c = small[name]
    rel = joint_rel(c)
    print("joint %s (k = %d): largest relative difference to _joint_probabilities_nn %.3e" % (name, c["k"], rel))
    assert rel <= 10 * tc.SKLEARN_JOINT_REL
    P = tc.joint_f64(c["idx"], tc.calibrate_f64(c["dist2"], c["perplexity"])[0])
    n = c["x"].shape[0]
    dense = tc.csr_dense(P, n)
    assert np.array_equal(dense, dense.T) and abs(P[2].sum() - 1.0) < 1e-13 and (np.diff(P[0]) >= c["k"]).all()
    for i in (0, n // 2, n - 1):
        assert (np.diff(P[1][P[0][i]:P[0][i + 1]]) > 0).all()                           # ascending within a row


@pytest.mark.parametrize("mistake", tc.CALIBRATION_MISTAKES)
def test_calibration_mistakes_exceed_the_margin(small, mistake):
    for name, c in small.items():
        assert joint_rel(c, mistake) > 10 * tc.SKLEARN_JOINT_REL, (name, mistake)


def test_hub_row_has_a_long_reverse_list():
    x = tc.hub_rows()
    P = tc.affinities_f64(x, 5.0)
    assert P[0][1] - P[0][0] >= x.shape[0] // 2 and P[3] == 0


# ------------------------------------------------------------------------------------------------- 3. gradient and KL against scikit-learn
def dense_p(n, seed):
    r = np.random.RandomState(seed)
    M = r.uniform(0.2, 1.0, size=(n, n))
    M = M + M.T
    np.fill_diagonal(M, 0.0)
    return M / M.sum()


def sklearn_kl(Y, M):
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _kl_divergence
    n = Y.shape[0]
    kl, grad = _kl_divergence(Y.astype(np.float64).ravel(), squareform(M, checks=False), 1, n, 2)
    return kl, grad.reshape(n, 2)


GRAD_RTOL = 1e-6


@pytest.mark.parametrize("state", ["initial", "converged", "pairs"])
def test_gradient_and_kl_against_sklearn(state):
    n = 200
    Y, M = tc.state(state, n), dense_p(n, 5)
    want_kl, want_grad = sklearn_kl(Y, M)
    grad, Z, kl = tc.gradient_f64(Y, tc.dense_csr(M))
    rel_g, rel_k = np.abs(grad - want_grad).max() / np.abs(want_grad).max(), abs(kl - want_kl) / abs(want_kl)
    print("gradient %s: relative difference to _kl_divergence: grad %.3e, KL %.3e" % (state, rel_g, rel_k))
    assert rel_g <= GRAD_RTOL and rel_k <= GRAD_RTOL
    F, z, _ = tc.repulsion_f64(Y)
    assert Z == float(z.sum()) and Z > 0


def test_coincident_points_count_in_z():
    for n in (2, 65):
        Y = tc.state("coincident", n)
        grad, Z, kl = tc.gradient_f64(Y, tc.sparse_p(n, 3))
        assert Z == n * (n - 1) and not grad.any()


# ------------------------------------------------------------------------------------------------- 4. planted mistakes
def test_every_mistake_is_planted_somewhere():
    assert set(tc.MISTAKES) == set(tc.CALIBRATION_MISTAKES) | set(tc.GRADIENT_MISTAKES) | set(tc.OPTIMISER_MISTAKES) and len(tc.MISTAKES) == 10


@pytest.mark.parametrize("mistake", tc.GRADIENT_MISTAKES)
def test_gradient_mistakes_exceed_the_bound(mistake):
    n = 200
    Y, M = tc.state("converged", n), dense_p(n, 5)
    a = 12.0 if mistake == "exag_repulsive" else 1.0
    P = tc.dense_csr(M)
    grad, Z, kl = tc.gradient_f64(Y, P, a)
    bad_grad, bad_Z, bad_kl = tc.gradient_f64(Y, P, a, mistake)
    rel = max(np.abs(bad_grad - grad).max() / np.abs(grad).max(), abs(bad_kl - kl) / abs(kl), abs(bad_Z - Z) / Z)
    assert rel > 100 * GRAD_RTOL, (mistake, rel)


GPU_SIZES = (2, 1023, 1024, 1025, 3001)                        # tests/test_gpu_tsne.py: around the row tile and the column chunk, and several ranges


@pytest.mark.parametrize("n", GPU_SIZES)
def test_the_device_bound_catches_a_column(n):
    """Dropping one column, counting the self pair and counting one padding column (at the origin) each exceed the bound the device's
    all-pairs sums are held to, C_BOUND * 2^-24 * the sum of the terms' magnitudes, on every case of the GPU gradient test - in the forces
    of some row or in Z."""
    u = 2.0 ** -24
    for state in tc.STATES:
        Y = tc.state(state, n)
        F, z, MF = tc.repulsion_f64(Y)
        Z = float(z.sum())
        j = n // 3
        tx, ty, q = tc.column_terms(Y, Y[j])
        tx[j] = ty[j] = q[j] = 0.0                                                      # row j never had its own column
        px, py, pq = tc.column_terms(Y, (0.0, 0.0))
        for what, dF, dZ in (("drop", np.stack([tx, ty], 1), q.sum()), ("self", np.zeros((n, 2)), float(n)), ("padding", np.stack([px, py], 1), pq.sum())):
            assert (np.abs(dF) > tc.C_BOUND * u * MF).any() or dZ > tc.C_BOUND * u * Z, (n, state, what)
        if n == 1023 and state == "converged":                                          # the helper is the restatement's own column
            F2, z2, _ = tc.repulsion_f64(Y, drop_column=j)
            assert np.allclose(F2, F - np.stack([tx, ty], 1), rtol=0, atol=1e-12 * MF.max()) and np.allclose(z2, z - q, rtol=1e-12)


def sklearn_descent(P, y0, max_iter, mistake=None):
    """scikit-learn's own _gradient_descent, in TSNE's two phases, driven by the restatement's gradient (evaluated at the float32 rounding of
    the state, as on the device)."""
    from sklearn.manifold._t_sne import _gradient_descent
    n = y0.shape[0]
    lr = max(n / 12.0 / 4.0, 50.0)

    def objective(p, exaggeration, compute_error=True):
        grad, _, kl = tc.gradient_f64(p.reshape(n, 2).astype(np.float32), P, exaggeration)
        return kl, grad.ravel()

    common = dict(n_iter_check=50, n_iter_without_progress=10 ** 6, learning_rate=lr, min_gain=0.01, min_grad_norm=0.0, verbose=0)
    p, _, it = _gradient_descent(objective, y0.astype(np.float64).ravel(), it=0, max_iter=min(250, max_iter), momentum=0.5, args=[12.0], **common)
    if max_iter > 250:
        p, _, it = _gradient_descent(objective, p, it=it + 1, max_iter=max_iter, momentum=0.8, args=[1.0], **common)
    return p.reshape(n, 2), it


def _optimiser_case():
    x, _ = tc.blob_rows(40, 8, 3, 75)
    return tc.affinities_f64(x, 5.0)[:3], tc.pca_init_f64(x).astype(np.float32)


def test_optimiser_against_sklearn_first_phase():
    P, y0 = _optimiser_case()
    want, it = sklearn_descent(P, y0, 250)
    got = tc.descend_f64(P, y0, 250)
    rel = np.abs(got - want).max() / np.abs(want).max()
    print("optimiser: relative difference to _gradient_descent after 250 iterations %.3e" % rel)
    assert it == 249 and rel <= 1e-9
    assert np.abs(tc.descend_f64(P, y0, 250, mistake="gains_inverted") - want).max() / np.abs(want).max() > 1e-3


def test_optimiser_against_sklearn_both_phases():
    """TSNE calls _gradient_descent twice, and each call starts from zero velocity and unit gains: so do the restatement and the device
    at the switch."""
    P, y0 = _optimiser_case()
    want, it = sklearn_descent(P, y0, 300)
    got = tc.descend_f64(P, y0, 300)
    rel = np.abs(got - want).max() / np.abs(want).max()
    print("optimiser, both phases: relative difference to scikit-learn's two _gradient_descent calls %.3e" % rel)
    assert it == 299 and rel <= 1e-9
    wrong = tc.descend_f64(P, y0, 300, mistake="momentum_switch")
    assert np.abs(wrong - want).max() / np.abs(want).max() > 1e-3


# ------------------------------------------------------------------------------------------------- the helpers of the end-to-end test
def test_pca_start_against_sklearn():
    from sklearn.decomposition import PCA
    import finch_cases as fc
    x, _ = tc.blob_rows(300, 24, 4, 71)
    u = fc.unit_rows(x)
    emb = PCA(n_components=2, svd_solver="full").fit_transform(u.astype(np.float64))
    want = emb / np.std(emb[:, 0]) * 1e-4
    got = tc.pca_init_f64(x)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


def test_trustworthiness_against_sklearn():
    from sklearn.manifold import trustworthiness
    r = np.random.RandomState(6)
    x, _ = tc.blob_rows(250, 8, 3, 76)
    y = x[:, :2] + 0.05 * r.randn(250, 2)
    assert abs(tc.trustworthiness_f64(x, y, 5) - trustworthiness(x, y, n_neighbors=5)) < 1e-12


def test_golden_fixture():
    g = tc.golden()
    assert g["rows"].shape == (1500, 32) and g["rows"].dtype == np.float32 and g["labels"].shape == (1500,)
    assert g["sklearn_kl"].shape == (5,) and g["sklearn_trust"].shape == (5,) and float(g["perplexity"]) == 20.0
    assert np.abs((g["rows"].astype(np.float64) ** 2).sum(1) - 1.0).max() < 1e-6
    assert os.path.getsize(tc.GOLDEN) < (1 << 20)


# ------------------------------------------------------------------------------------------------- the library's host side
def test_workspace_query_limits():
    from scd_amd import _lib
    L = _lib.load()
    assert L.scd_tsne_gradient_ws_bytes(1, 0) == 0 and L.scd_tsne_gradient_ws_bytes(1 << 31, 0) == 0 and L.scd_tsne_gradient_ws_bytes(10, -1) == 0
    nb = L.scd_tsne_gradient_ws_bytes(126976, 126976 * 100)
    print("scd_tsne_gradient workspace at n = 126,976: %.1f MB" % (nb / 1e6))
    assert 0 < nb < (1 << 30)
    assert L.scd_tsne_row_tile() == 1024 and L.scd_tsne_col_chunk() == 1024
    # no handle: refused before anything is launched
    assert L.scd_tsne_gradient(None, None, None, None, None, 10, 0, 1.0, 0, None, None, None, None, None, 0, None) == _lib.SCD_EINVAL
    assert L.scd_tsne_calibrate(None, None, 10, 5, 2.0, None, None, None, None) == _lib.SCD_EINVAL
    assert L.scd_tsne_update(None, None, None, None, None, None, 10, 0.5, 1.0, 0.01, None, None) == _lib.SCD_EINVAL


def test_python_layer_refuses_bad_arguments():
    from scd_amd import tsne
    with pytest.raises(ValueError):
        tsne.TSNE(n_components=3)
    for n, perplexity in ((100, 1.0), (100, 0.5), (10, 30.0), (4, 3.0)):
        with pytest.raises(ValueError):
            tsne._check_perplexity(n, perplexity)
    assert tsne._check_perplexity(1500, 20.0) == 60 and tsne._check_perplexity(1500, 30.0) == 64 and tsne._check_perplexity(50, 20.0) == 49
    t = tsne.TSNE()
    assert (t.perplexity, t.early_exaggeration, t.learning_rate, t.max_iter, t.n_iter_without_progress, t.min_grad_norm, t.init) == \
        (30.0, 12.0, 'auto', 1000, 300, 1e-7, 'pca')
