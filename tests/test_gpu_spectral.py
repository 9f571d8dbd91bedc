"""GPU checks of scd_knn_affinity / scd_spmm_f64 (scd_amd/csrc/graph.hip) and scd_amd.spectral against the float64 restatement of
tests/spectral_cases.py: the affinity and the sparse product bit for bit, the solver by residuals, orthonormality, eigenvalues and the
Davis-Kahan angle recomputed on the CPU from the returned vectors and the restated S, the clustering by its partition.
docs/design/spectral.md has the rules."""
import re

import numpy as np
import pytest
import torch

import spectral_cases as sc

pytestmark = pytest.mark.gpu
TOL = 1e-8


@pytest.fixture(scope="module")
def ops():
    from scd_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lists():
    return dict(sc.list_cases(), **sc.scan_cases())


@pytest.fixture(scope="module")
def affs(lists):
    return {name: (sc.affinity_sparse if name in sc.SCAN else sc.affinity)(idx) for name, idx in lists.items()}


@pytest.fixture(scope="module")
def dense(affs):
    """name -> (eigenvalues descending, eigenvectors) of the restated S, for the two data cases."""
    return {name: sc.dense_eigs(affs[name]) for name in ("blobs", "rings")}


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_affinity(got, want):
    rowptr, col, val, isd, nnz = got
    assert nnz == want["nnz"] and col.numel() == nnz and val.numel() == nnz
    assert np.array_equal(rowptr.cpu().numpy(), want["rowptr"])
    assert np.array_equal(col.cpu().numpy(), want["col"])
    assert np.array_equal(bits(val.cpu().numpy()), bits(want["val"]))
    assert np.array_equal(bits(isd.cpu().numpy()), bits(want["inv_sqrt_deg"]))


# ------------------------------------------------------------------------------------------------- the affinity
@pytest.mark.parametrize("name", ["blobs", "rings", "hub", "tiny", "ragged", "hub_wide", "scan_4097", "scan_8200"])
def test_affinity_bit_for_bit(ops, lists, affs, name):
    idx = dev(lists[name])
    first = ops.knn_affinity(idx)
    lens = np.diff(affs[name]["rowptr"])
    print("affinity %-6s n %4d k %2d: nnz %5d, median row %d, longest row %d" % (name, idx.shape[0], idx.shape[1], first[4], np.median(lens), lens.max()))
    if name in sc.SCAN:                                         # graph_scan_kernel hands a carry from tile to tile
        assert affs[name]["rowptr"][sc.SCAN_TILE] > 0 and lens[sc.SCAN_TILE] > 1024
    assert_affinity(first, affs[name])
    second = ops.knn_affinity(idx, cap=2 * idx.numel() + 100)
    for a, b in zip(first[:4], second[:4]):
        assert torch.equal(a, b)


def test_affinity_from_rows_equals_the_restatement_on_the_device_unit_rows():
    from scd_amd import spectral
    from scd_amd.knn import unit_rows
    case = sc.blobs()
    x = dev(case["x"])
    rowptr, col, val, isd, info = spectral.knn_affinity(x, case["n_neighbors"])
    want = sc.affinity(sc.knn_lists(unit_rows(x).cpu().numpy(), case["n_neighbors"]))
    assert_affinity((rowptr, col, val, isd, info["nnz"]), want)
    assert info["max_row"] == np.diff(want["rowptr"]).max()


def test_affinity_refusals(ops, lists):
    from scd_amd import _lib
    idx = dev(lists["tiny"])
    with pytest.raises(_lib.ScdError) as e:
        ops.knn_affinity(idx, cap=2 * idx.numel() - 1)
    assert e.value.code == _lib.SCD_EINVAL and "cap" in str(e.value)
    bad = lists["ragged"].copy()
    bad[500, 3] = len(bad)
    with pytest.raises(_lib.ScdError) as e:
        ops.knn_affinity(dev(bad))
    assert e.value.code == _lib.SCD_EINVAL and ">= n" in str(e.value)
    assert_affinity(ops.knn_affinity(dev(lists["ragged"])), sc.affinity(lists["ragged"]))        # and the next call is unharmed


# ------------------------------------------------------------------------------------------------- the sparse product
E, C_ = 0.85, -0.15             # the filter's half-width and centre for the interval [-1, 0.7]
COEFFS = {"plain": (1.0, 0.0, 0.0, False), "recurrence": (2.0 / E, -2.0 * C_ / E, -1.0, True), "shifted": (1.0, -0.3, 0.0, False)}


def upload(aff):
    return dev(aff["rowptr"]), dev(aff["col"]), dev(aff["val"])


@pytest.mark.parametrize("coeffs", list(COEFFS))
@pytest.mark.parametrize("name,m", [(name, m) for m in (8, 40, 136) for name in ("blobs", "hub", "ragged", "hub_wide")]
                         + [(name, m) for m in (8, 136) for name in sc.SCAN])
def test_spmm_bit_for_bit(ops, affs, name, m, coeffs):
    aff = affs[name]
    n = len(aff["rowptr"]) - 1
    alpha, beta, gamma, with_z = COEFFS[coeffs]
    x, z = sc.spread_block(11, n, m), sc.spread_block(12, n, m) if with_z else None
    buf = torch.zeros((n, m + 16), dtype=torch.float64, device="cuda")
    xd = buf[:, 8:8 + m]                                        # a column slice: ldx = m + 16 > m
    xd.copy_(dev(x))
    got = ops.spmm_f64(*upload(aff), xd, alpha, beta, gamma, None if z is None else dev(z))
    want = sc.spmm(aff, x, alpha, beta, gamma, z)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert torch.equal(buf[:, :8], torch.zeros_like(buf[:, :8])) and torch.equal(buf[:, 8 + m:], torch.zeros_like(buf[:, 8 + m:]))


def test_spmm_refusals(ops, affs):
    from scd_amd import _lib
    aff = affs["tiny"]
    csr = upload(aff)
    x = dev(sc.spread_block(1, 5, 8))
    for kwargs, word in ((dict(out=x), "alias"), (dict(z=x.clone(), out=x), "alias")):
        with pytest.raises(_lib.ScdError) as e:
            ops.spmm_f64(*csr, x, **kwargs)
        assert e.value.code == _lib.SCD_EINVAL and word in str(e.value)
    y = torch.empty_like(x)
    with pytest.raises(_lib.ScdError) as e:
        ops.spmm_f64(*csr, x, gamma=1.0, z=y, out=y)
    assert e.value.code == _lib.SCD_EINVAL and "alias" in str(e.value)
    with pytest.raises(_lib.ScdError) as e:
        ops.spmm_f64(*csr, dev(sc.spread_block(1, 5, 12)))
    assert e.value.code == _lib.SCD_EINVAL and "m % 8" in str(e.value)
    wide = torch.zeros((5, 20), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.ScdError) as e:                     # a leading dimension that is no multiple of 8
        ops.spmm_f64(*csr, wide[:, :8])
    assert e.value.code == _lib.SCD_EINVAL
    got = ops.spmm_f64(*csr, x)                                 # K5: every entry 1/4, the row sum of the others
    assert np.array_equal(bits(got.cpu().numpy()), bits(sc.spmm(aff, x.cpu().numpy())))


# ------------------------------------------------------------------------------------------------- the solver
@pytest.mark.parametrize("name,k", [("blobs", 6), ("rings", 3)])
def test_eigsolve_on_the_device(affs, dense, name, k):
    from scd_amd import spectral
    aff = affs[name]
    n = len(aff["rowptr"]) - 1
    w, v, info = spectral.eigsolve(spectral.device_operator(*upload(aff)), n, k, tol=TOL, device=torch.device("cuda"))
    print("eigsolve %-6s: %s" % (name, info))
    assert info["converged"] and v.is_cuda and v.dtype == torch.float64
    w, v = w.cpu().numpy(), v.cpu().numpy()
    s = sc.dense_s(aff)
    r = s @ v - v * w
    res = np.linalg.norm(r, axis=0)
    assert res.max() <= TOL + 1e-12
    assert np.abs(v.T @ v - np.eye(k)).max() <= 1e-12
    wd, vd = dense[name]
    if name == "blobs":
        assert np.all(np.abs(w - wd[:k]) <= res)        # index by index: the 4.8e-3 gap against a 1e-8 residual pairs them
    else:
        assert np.all(np.abs(w - 1.0) <= res)           # the threefold eigenvalue
    gap = wd[k - 1] - wd[k]
    sine = sc.sin_largest_angle(v, vd[:, :k])
    print("  largest residual %.3g, sine of the largest angle %.3g, Davis-Kahan bound %.3g (gap %.3g)" % (res.max(), sine, np.linalg.norm(r) / gap, gap))
    assert sine <= np.linalg.norm(r) / gap


# ------------------------------------------------------------------------------------------------- the clustering
def dense_partition(aff, wv, k):
    return sc.kmeans_partition(sc.embed(wv[1][:, :k], aff["inv_sqrt_deg"]), k, 0)


def test_spectral_clustering_blobs(affs, dense):
    from scd_amd.spectral import SpectralClustering
    case = sc.blobs()
    m = SpectralClustering(6, n_neighbors=10, random_state=0, tol=TOL).fit(case["x"])
    print("blobs: %s" % m.info_)
    assert sc.same_partition(m.labels_, dense_partition(affs["blobs"], dense["blobs"], 6))
    assert m.embedding_.shape == (600, 6) and m.embedding_.dtype == torch.float32 and len(m.affinity_) == 4
    assert np.all(np.abs(m.eigenvalues_ - dense["blobs"][0][:6]) <= 1e-7) and m.info_["converged"]
    emb = m.embedding_.cpu().numpy()
    assert np.all(emb[np.abs(emb).argmax(0), np.arange(6)] > 0)                            # the sign rule


def test_spectral_clustering_rings_and_the_driver():
    import importlib
    from scd_amd.spectral import SpectralClustering
    case = sc.rings()
    labels = SpectralClustering(3, n_neighbors=8, random_state=0, tol=TOL).fit_predict(torch.as_tensor(case["x"]).cuda())
    assert sc.same_partition(labels, case["truth"])
    mu = importlib.import_module("main_unsup")
    args = mu.build_parser().parse_args(["--cluster", "SC", "--n_cluster", "3", "--n_neighbors", "8"])
    all_preds, preds = mu.run_clustering(args, case["x"], case["x"][:0], np.zeros(0))
    assert all_preds is None and sc.same_partition(preds, case["truth"])


def test_refusals_name_the_limit():
    from scd_amd.spectral import SpectralClustering
    x = torch.zeros((40, 4), device="cuda")
    for kwargs, word in ((dict(n_neighbors=1), "n_neighbors <= 65"), (dict(n_neighbors=66), "n_neighbors <= 65"),
                         (dict(n_neighbors=40), "n > n_neighbors"), (dict(n_clusters=40), "n_components <= min"),
                         (dict(n_clusters=35), "m <= n")):
        args = dict(n_clusters=3, n_neighbors=10)
        args.update(kwargs)
        with pytest.raises(ValueError, match=re.escape(word)):
            SpectralClustering(**args).fit(x)
