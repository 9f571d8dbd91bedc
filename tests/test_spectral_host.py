"""CPU checks of the spectral tests' own yardstick (tests/spectral_cases.py) against scikit-learn, of the cases' conditions, of
scd_amd.spectral.eigsolve over a CPU operator, and of the host side of the feature (ABI, CLI, workspace).  No device is used.
docs/design/spectral.md has the rules."""
import os
import re

import numpy as np
import pytest
import torch

import spectral_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-8


@pytest.fixture(scope="module")
def data():
    """name -> dict(case, aff, w, v, emb, part): the restated affinity, the dense eigenpairs, the dense embedding and its partition."""
    out = {}
    for name in ("blobs", "rings"):
        case = getattr(sc, name)()
        aff = sc.affinity(sc.knn_lists(case["x"], case["n_neighbors"]))
        w, v = sc.dense_eigs(aff)
        k = case["n_clusters"]
        emb = sc.embed(v[:, :k], aff["inv_sqrt_deg"])
        out[name] = dict(case=case, aff=aff, w=w, v=v, emb=emb, part=sc.kmeans_partition(emb, k, 0))
    return out


def sklearn_affinity(case):
    """sklearn/cluster/_spectral.py:_fit for affinity='nearest_neighbors', then spectral_embedding's removal of the diagonal."""
    from sklearn.neighbors import kneighbors_graph
    c = kneighbors_graph(case["x"].astype(np.float64), n_neighbors=case["n_neighbors"], include_self=True)
    a = (0.5 * (c + c.T)).toarray()
    np.fill_diagonal(a, 0.0)
    return a


@pytest.mark.parametrize("name", ["blobs", "rings"])
def test_restated_affinity_equals_sklearn(data, name):
    d = data[name]
    a = sklearn_affinity(d["case"])
    assert np.array_equal(d["aff"]["A"], a)
    assert np.array_equal(d["aff"]["deg"], a.sum(1)) and np.array_equal(d["aff"]["deg"] * 2, np.round(d["aff"]["deg"] * 2))
    s = sc.dense_s(d["aff"])
    assert np.array_equal(s, s.T)                               # bitwise symmetric
    root = np.sqrt(a.sum(1))
    assert np.array_equal(s, a / (root[:, None] * root[None, :]))
    assert np.all(np.diff(d["aff"]["col"])[np.diff(np.repeat(np.arange(len(a)), np.diff(d["aff"]["rowptr"]))) == 0] > 0)    # columns ascend


def test_restated_embedding_spans_sklearn(data):
    from sklearn.manifold import spectral_embedding
    d = data["blobs"]
    a = sklearn_affinity(d["case"])
    emb = spectral_embedding(a, n_components=6, eigen_solver="arpack", random_state=0, drop_first=False)
    sine = sc.sin_largest_angle(emb, d["emb"])
    print("sine of the largest principal angle to scikit-learn's embedding: %.3g" % sine)
    assert sine <= 1e-6


def test_restated_product_equals_dense(data):
    """The chunked order against a dense float64 product, within the rounding of a sum of |terms|; the hub cases have three and six chunks."""
    for idx in (sc.hub(), sc.hub_wide(), sc.ragged(), sc.tiny()):
        aff = sc.affinity(idx)
        n = len(idx)
        x, z = sc.spread_block(5, n, 8), sc.spread_block(6, n, 8)
        s = sc.dense_s(aff)
        got = sc.spmm(aff, x, 2.0, -0.3, -1.0, z)
        bound = (np.diff(aff["rowptr"]).max() + 3) * 2.0 ** -52 * (2.0 * np.abs(s) @ np.abs(x) + 0.3 * np.abs(x) + np.abs(z))
        assert np.all(np.abs(got - (2.0 * (s @ x) - 0.3 * x - z)) <= bound)
    assert np.diff(sc.affinity(sc.hub())["rowptr"])[0] == 1499 and np.diff(sc.affinity(sc.hub_wide())["rowptr"])[0] == 2599


def cpu_operator(aff):
    from scipy.sparse import csr_matrix
    n = len(aff["rowptr"]) - 1
    s = csr_matrix((aff["val"], aff["col"], aff["rowptr"]), shape=(n, n))

    def apply(x, alpha, beta, gamma, z):
        y = alpha * torch.as_tensor(s @ x.numpy()) + beta * x
        return y if z is None else y + gamma * z
    return s, apply


@pytest.mark.parametrize("name", ["blobs", "rings"])
def test_eigsolve_over_a_cpu_operator(data, name):
    from scd_amd.spectral import eigsolve
    d = data[name]
    k, n = d["case"]["n_clusters"], len(d["case"]["x"])
    s, apply = cpu_operator(d["aff"])
    w, v, info = eigsolve(apply, n, k, tol=TOL)
    print("%s: %s" % (name, info))
    assert info["converged"] and info["residual"] <= TOL and info["m"] == 16
    w, v = w.numpy(), v.numpy()
    res = np.linalg.norm(s @ v - v * w, axis=0)
    assert res.max() <= TOL + 1e-12
    assert np.all(np.abs(w - d["w"][:k]) <= res)        # a Ritz value lies within its residual norm of an eigenvalue
    assert np.abs(v.T @ v - np.eye(k)).max() <= 1e-12
    part = sc.kmeans_partition(sc.embed(v, d["aff"]["inv_sqrt_deg"]), k, 0)
    assert sc.same_partition(part, d["part"])


def test_eigsolve_reports_no_convergence(data):
    from scd_amd.spectral import NotConverged, eigsolve
    d = data["rings"]
    _, apply = cpu_operator(d["aff"])
    with pytest.raises(RuntimeError) as e:
        eigsolve(apply, len(d["case"]["x"]), 3, tol=1e-13, max_outer=2)
    assert isinstance(e.value, NotConverged) and e.value.info["outer"] == 2 and not e.value.info["converged"]
    assert e.value.info["residual"] > 1e-13 and e.value.info["products"] == 2 * 12


def test_eigsolve_limits():
    from scd_amd.spectral import block_width, eigsolve
    assert [block_width(k) for k in (1, 3, 6, 8, 100, 1000)] == [16, 16, 16, 16, 128, 1256]
    with pytest.raises(ValueError, match="m <= n"):
        eigsolve(None, 12, 3)


# ------------------------------------------------------------------------------------------------- the cases' own conditions
def test_blobs_conditions(data):
    from sklearn.metrics import adjusted_rand_score
    d = data["blobs"]
    w = d["w"]
    gaps = -np.diff(w[:7])
    print("blobs: lambda_6 - lambda_7 = %.4f, smallest gap of the seven leading %.3g, longest row %d"
          % (gaps[5], gaps.min(), np.diff(d["aff"]["rowptr"]).max()))
    assert sc.components(d["aff"]) == 1
    assert gaps[5] >= 0.2 and gaps.min() >= 1e-3                # against a residual of 1e-8: the pairing is unambiguous
    assert np.diff(d["aff"]["rowptr"]).max() <= 64
    parts = [sc.kmeans_partition(d["emb"], 6, seed) for seed in range(5)]
    assert all(sc.same_partition(parts[0], p) for p in parts)
    ari = adjusted_rand_score(d["case"]["truth"], parts[0])
    print("blobs: ARI of the dense-embedding partition against the truth %.3f" % ari)
    assert ari >= 0.9


def test_rings_conditions(data):
    from sklearn.cluster import KMeans
    from sklearn.metrics import adjusted_rand_score
    d = data["rings"]
    w = d["w"]
    print("rings: leading eigenvalues %s" % w[:5])
    assert sc.components(d["aff"]) == 3
    assert np.all(np.abs(w[:3] - 1.0) <= 1e-12) and 1e-4 <= w[2] - w[3] <= 1e-3         # eigenvalue 1 is threefold
    parts = [sc.kmeans_partition(d["emb"], 3, seed) for seed in range(5)]
    assert all(sc.same_partition(p, d["case"]["truth"]) for p in parts)
    raw = KMeans(n_clusters=3, n_init=10, random_state=0).fit(d["case"]["x"]).labels_
    ari = adjusted_rand_score(d["case"]["truth"], raw)
    print("rings: ARI of k-means on the raw rows %.4f" % ari)
    assert ari < 0.1


def test_list_cases_have_what_they_are_for():
    ragged = sc.ragged()
    n = len(ragged)
    assert (ragged < 0).any() and (ragged == np.arange(n)[:, None]).any()
    assert any(len(set(r[r >= 0])) < (r >= 0).sum() for r in ragged)
    assert sc.affinity(sc.tiny())["nnz"] == 20 and np.all(sc.affinity(sc.tiny())["val"] == 0.25)
    with pytest.raises(ValueError):
        sc.affinity(np.array([[1], [2]]))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_sparse_affinity_equals_the_dense_restatement():
    """Field by field, the values as bits, on the six cases the dense restatement can hold."""
    cases = sc.list_cases()
    assert len(cases) == 6
    for name, idx in cases.items():
        want, got = sc.affinity(idx), sc.affinity_sparse(idx)
        assert set(got) == set(want) - {"A"} and got["nnz"] == want["nnz"], name
        assert np.array_equal(got["rowptr"], want["rowptr"]) and got["rowptr"].dtype == want["rowptr"].dtype, name
        assert np.array_equal(got["col"], want["col"]) and got["col"].dtype == want["col"].dtype, name
        for key in ("val", "inv_sqrt_deg", "deg"):
            assert np.array_equal(bits(got[key]), bits(want[key])), (name, key)
    with pytest.raises(ValueError):
        sc.affinity_sparse(np.array([[1], [2]]))


def test_scan_cases_carry():
    """The two cases of more than 4,096 rows: a carry that is not zero, an empty row before the tile border, a hub right after it - and
    a scan whose tiles each start from 0 gives another rowptr."""
    cases = sc.scan_cases()
    assert [len(cases[name]) for name in ("scan_4097", "scan_8200")] == [4097, 8200]
    assert [sc.SCAN[name][1] for name in ("scan_4097", "scan_8200")] == [3, 5]
    assert [-(-len(idx) // sc.SCAN_TILE) for idx in cases.values()] == [2, 3]
    for name, idx in cases.items():
        n = len(idx)
        aff = sc.affinity_sparse(idx)
        rowptr, lens = aff["rowptr"], np.diff(aff["rowptr"])
        print("%s: nnz %d, rowptr[4096] %d, row 4096 has %d entries, median row %d" % (name, aff["nnz"], rowptr[4096], lens[4096], np.median(lens)))
        assert rowptr[4096] > 0 and lens[4095] == 0 and aff["deg"][4095] == 0 and aff["inv_sqrt_deg"][4095] == 1.0
        assert not (aff["col"] == 4095).any() and lens[4096] > 1024 and lens[4096] == lens.max()
        assert lens[4096] >= (n + 3) // 4 - 1                                            # every 4th row but itself
        assert (idx < 0).any() and (idx == np.arange(n)[:, None]).any()
        assert any(len(set(r[r >= 0])) < (r >= 0).sum() for r in idx)
        bad = sc.carry_zero(rowptr)
        assert np.array_equal(bad[:4096], rowptr[:4096]) and (bad[4096:] != rowptr[4096:]).all() and bad[4096] == 0
        rows = np.repeat(np.arange(n), lens)
        assert (np.diff(aff["col"].astype(np.int64) + rows * n) > 0).all()               # columns ascend inside a row
    assert len(sc.affinity_sparse(cases["scan_8200"])["rowptr"]) == 8201
    for name in ("hub", "ragged"):                                                       # one tile: the mistake cannot show
        rowptr = sc.affinity(sc.list_cases()[name])["rowptr"]
        assert np.array_equal(sc.carry_zero(rowptr), rowptr)


# ------------------------------------------------------------------------------------------------- ABI, CLI, workspace
def test_abi_declares_the_graph_entry_points():
    from scd_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scd_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("scd_knn_affinity_ws_bytes", "scd_knn_affinity", "scd_spmm_f64"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES and hasattr(lib, name)


def test_affinity_workspace():
    from scd_amd import _lib
    lib = _lib.load()
    nb = lib.scd_knn_affinity_ws_bytes(126976, 64)
    assert 0 < nb < 2 << 30
    assert lib.scd_knn_affinity_ws_bytes(126976, 65) == 0 and lib.scd_knn_affinity_ws_bytes(1, 1) == 0


def test_cli_parses_spectral_clustering():
    import importlib
    mu = importlib.import_module("main_unsup")
    a = mu.build_parser().parse_args(["--cluster", "SC", "--n_cluster", "100"])
    assert (a.cluster, a.n_neighbors, a.n_cluster) == ("SC", 10, 100)
    assert mu.build_parser().parse_args(["--cluster", "SC", "--n_neighbors", "15"]).n_neighbors == 15
    assert "SC" in mu.build_parser().format_help()


def test_refusals_name_the_limit():
    from scd_amd import spectral
    x = np.zeros((40, 4), dtype=np.float32)
    for kwargs, word in ((dict(n_neighbors=1), "n_neighbors <= 65"), (dict(n_neighbors=66), "n_neighbors <= 65"),
                         (dict(n_neighbors=40), "n > n_neighbors"), (dict(n_components=40), "n_components <= min"),
                         (dict(n_components=35), "m <= n")):          # 35 + 8 rounded up to 48 > 40
        args = dict(n_components=3, n_neighbors=10)
        args.update(kwargs)
        with pytest.raises(ValueError, match=re.escape(word)):
            spectral.spectral_embedding(x, **args)
