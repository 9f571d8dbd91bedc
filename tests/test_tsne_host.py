"""CPU checks of the numpy restatement tests/tsne_cases.py that the GPU tests of t-SNE compare the device against: calibration against
scipy's brentq roots, the joint matrix, the gradient, KL, the optimiser, the PCA start and trustworthiness against scikit-learn 1.7,
and every planted mistake of tsne_cases.MISTAKES and RANGE_MISTAKES against the bound of the test that is meant to catch it; the range
rule, banded_p and the torch restatement of the cases whose column ranges hold several chunks.  docs/design/tsne.md."""
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


# ------------------------------------------------------------------------------------------------- ranges of several chunks
def test_ranges_of_the_large_cases():
    """The figures the large cases are named for, from the restated rule alone: 33 and 50 chunks, on 64, 256 and 304 compute units."""
    c33, c50 = tc.LARGE["c33"], tc.LARGE["c50"]
    assert (tc.cdiv(c33, tc.CHUNK), tc.cdiv(c50, tc.CHUNK)) == (33, 50) and c33 % tc.CHUNK == 1 and c50 % tc.CHUNK == 1
    assert tc.ranges(c33 - 1, 256) == (32, 1, 1)                                        # c33 is the smallest n that reaches the path
    assert tc.ranges(c33, 256) == (17, 2, 1) and tc.ranges(c33, 304) == (17, 2, 1) and tc.ranges(c33, 64) == (7, 5, 3)
    assert tc.ranges(c50, 256) == (17, 3, 2) and tc.ranges(c50, 304) == (25, 2, 2) and tc.ranges(c50, 64) == (6, 9, 5)
    assert tc.ranges(3001, 256) == (3, 1, 1) and tc.ranges(2, 256) == (1, 1, 1)         # the earlier cases: one chunk a range
    for n in tc.LARGE.values():
        for n_cu in range(1, 1025):
            ny, cpy, last = tc.ranges(n, n_cu)
            assert cpy >= 2 and 1 <= last <= cpy and (ny - 1) * cpy + last == tc.cdiv(n, tc.CHUNK) and ny <= tc.YMAX
    assert set(tc.LARGE_STATES["c33"]) == set(tc.STATES) and tc.LARGE_STATES["c50"] == ("converged", "coincident")


TORCH_RTOL = 1e-13              # repulsion_f64_torch against repulsion_f64: float64 sums of the same terms in another order


def test_torch_restatement_equals_numpy():
    n = 3001
    worst_f = worst_z = 0.0
    for state in tc.STATES:
        Y = tc.state(state, n)
        F, z, MF = tc.repulsion_f64(Y)
        Ft, zt, MFt = tc.repulsion_f64_torch(Y, device="cpu")
        with np.errstate(divide="ignore", invalid="ignore"):
            worst_f = max(worst_f, float(np.nanmax(np.where(MF > 0, np.abs(Ft - F) / MF, 0.0))))
        worst_z = max(worst_z, float((np.abs(zt - z) / z).max()))
        assert (np.abs(Ft - F) <= TORCH_RTOL * MF).all() and (np.abs(MFt - MF) <= TORCH_RTOL * MF).all(), state
        assert (np.abs(zt - z) <= TORCH_RTOL * z).all(), state
        if state == "coincident":
            assert (zt == n - 1).all() and not Ft.any()
    print("torch against numpy at n = %d: forces within %.2e M_i, q sums within %.2e z_i" % (n, worst_f, worst_z))
    rows = np.array([0, 7, 3000])
    Y = tc.state("converged", n)
    F, z, MF = tc.repulsion_f64(Y)
    Fr, zr, MFr = tc.repulsion_f64(Y, rows=rows)                                         # rows= is a slice of the same sums
    assert np.array_equal(Fr, F[rows]) and np.array_equal(zr, z[rows]) and np.array_equal(MFr, MF[rows])


def test_banded_p():
    import time
    t0 = time.perf_counter()
    big = tc.banded_p(tc.LARGE["c50"], seed=11)
    took = time.perf_counter() - t0
    print("banded_p at n = %d: %d entries, row 0 has %d, %.3f s" % (tc.LARGE["c50"], len(big[1]), big[0][1], took))
    for n, P in ((3001, tc.banded_p(3001, seed=11)), (tc.LARGE["c33"], tc.banded_p(tc.LARGE["c33"], seed=11)), (tc.LARGE["c50"], big)):
        indptr, indices, values = P
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
        cols = indices.astype(np.int64)
        assert indptr[-1] == len(indices) == len(values) and (values > 0).all() and (rows != cols).all()
        assert (np.diff(rows * n + cols) > 0).all()                                      # rows in order, columns ascending, no repeat
        back = np.argsort(cols * n + rows, kind="stable")                               # the transpose in the same order
        assert np.array_equal(rows[back], cols) and np.array_equal(cols[back], rows) and np.array_equal(values[back], values)
        assert abs(values.sum() - 1.0) <= 1e-12
        assert indptr[1] - indptr[0] > 192                                               # more than three trips of the lane loop
        assert len(np.unique(indices[:indptr[1]] // tc.CHUNK)) == tc.cdiv(n, tc.CHUNK)   # the hub reaches every chunk
        other = np.zeros(n, dtype=bool)
        other[rows[cols // tc.CHUNK != rows // tc.CHUNK]] = True
        assert other[:tc.ROWS].all()                                                     # every row of the first tile leaves its chunk
        assert (np.diff(indptr) >= 4).all()


@pytest.fixture(scope="module")
def range_sums():
    """state -> (Y, rows, F, z, MF) on c33: the float64 sums over all columns of the 64 rows."""
    n = tc.LARGE["c33"]
    rows = tc.range_rows(n)
    out = {}
    for state in ("converged", "coincident"):
        Y = tc.state(state, n)
        out[state] = (Y, rows) + tc.repulsion_f64(Y, rows=rows)
    return out


def test_range_rows():
    rows = tc.range_rows(tc.LARGE["c33"])
    assert len(rows) == len(set(rows.tolist())) == 64 and {0, 1023, 1024, 2047, 2048, 32767, 32768} <= set(rows.tolist())
    assert len(tc.RANGE_MISTAKES) == 4


@pytest.mark.parametrize("n_cu", [64, 256, 304])
@pytest.mark.parametrize("mistake", tc.RANGE_MISTAKES)
def test_range_mistakes_exceed_the_bound(range_sums, mistake, n_cu):
    """Each planted mistake of the chunk loop and the range sum moves a force of one of the 64 rows by more than the device bound on
    `converged`, and a q sum by a whole number on `coincident`, where every term is exactly 1 or 0."""
    u = 2.0 ** -24
    n = tc.LARGE["c33"]
    Y, rows, F, z, MF = range_sums["converged"]
    dF, dz = tc.range_mistake_shift(Y, rows, n_cu, mistake)
    over = np.abs(dF) > tc.C_BOUND * u * MF
    print("%s on %d CUs, converged: %d of 64 rows over the bound, largest shift %.3g x 2^-24 M_i" % (mistake, n_cu, over.any(1).sum(), (np.abs(dF) / (u * MF)).max()))
    assert over.any(), (mistake, n_cu)
    Y, rows, F, z, MF = range_sums["coincident"]
    assert (z == n - 1).all() and not F.any()
    dF, dz = tc.range_mistake_shift(Y, rows, n_cu, mistake, padding=False)              # the rows' own columns: every term is 1 or 0
    assert not dF.any() and np.array_equal(dz, np.round(dz)) and (np.abs(dz) >= 1).any(), (mistake, n_cu)
    lost, extra = tc.dropped_columns(n, n_cu, 1024, mistake)
    assert (extra < n).sum() - len(lost) == dz[list(rows).index(1024)]


def test_dropped_columns_by_hand():
    """The model on c33 with 256 compute units, 17 ranges of 2 and a last range of one chunk with ONE column, worked by hand."""
    n = tc.LARGE["c33"]
    lost, extra = tc.dropped_columns(n, 256, 5, "first_chunk_only")                     # the odd chunks, all full
    assert len(extra) == 0 and len(lost) == 16 * 1024 and lost[0] == 1024 and lost[-1] == 32767
    lost, extra = tc.dropped_columns(n, 256, 1500, "first_chunk_only")                  # its own column is in an odd chunk
    assert len(lost) == 16 * 1024 - 1 and 1500 not in lost
    assert tc.dropped_columns(n, 256, 5, "last_range_dropped")[0].tolist() == [32768]
    assert len(tc.dropped_columns(n, 256, 32768, "last_range_dropped")[0]) == 0         # the lone row of the last tile loses nothing
    lost, extra = tc.dropped_columns(n, 256, 5, "stale_range")
    assert len(lost) == 0 and len(extra) == 2047 and 5 not in extra
    assert len(tc.dropped_columns(tc.LARGE["c50"], 304, 5, "stale_range")[1]) == 0      # 25 ranges before and after
    for row, want in ((0, ([1024], [])), (1023, ([2047], [])), (1024, ([], [1024])), (2047, ([], [2047])), (2048, ([3072], [])),
                      (32767, ([], [32767])), (32768, ([], []))):
        lost, extra = tc.dropped_columns(n, 256, row, "own_chunk_unchecked")
        assert (lost.tolist(), extra.tolist()) == want, row
    # 64 compute units: 7 ranges of 5, the last one chunks 30, 31 and 32; chunk 32 stops after its first run of 64
    lost, extra = tc.dropped_columns(n, 64, 5, "own_chunk_unchecked")
    assert lost.tolist() == [1029, 2053, 3077, 4101] and extra.tolist() == list(range(n, n + 63))      # its block of the last range
    lost, extra = tc.dropped_columns(n, 64, 31 * 1024 + 7, "own_chunk_unchecked")
    assert len(lost) == 0 and extra.tolist() == [31 * 1024 + 7] + list(range(n, n + 63))
    lost, extra = tc.dropped_columns(n, 64, 30 * 1024 + 7, "own_chunk_unchecked")       # own chunk first: offset 7 of chunk 32 is padding
    assert lost.tolist() == [31 * 1024 + 7] and extra.tolist() == [j for j in range(n, n + 63) if j != 32 * 1024 + 7]


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
