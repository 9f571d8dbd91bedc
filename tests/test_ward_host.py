"""CPU tests of the Ward feature (docs/design/ward.md): the float64 restatement of tests/ward_cases.py against scipy's linkage(x, 'ward')
and scikit-learn's AgglomerativeClustering(linkage='ward'), cut_tree against fcluster, the key order of the linkage rows, each case's
named property, each planted mistake, the ABI and the arguments.  No GPU."""
import os
import re

import numpy as np
import pytest

import ward_cases as wc

scipy_h = pytest.importorskip("scipy.cluster.hierarchy")
sklearn = pytest.importorskip("sklearn")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the largest relative deviation of a sorted height from scipy's on the blob cases is 1.57e-7 (blobs600; 6.0e-8 on the other two): the
# float32 rounding of a centroid, 6e-8 per coordinate.  Ten times that covers other seeds of the same construction.
HEIGHT_TOL = 1.6e-6


def _lib():
    from scd_amd import _lib
    return _lib.load()


def _cuts(name):
    n, k = len(wc.solved(name)["x"]), wc.BLOBS[name]
    return (2, k, 3 * k, n // 10)


# ---------------------------------------------------------------------------------------------------- against scipy and scikit-learn
@pytest.mark.parametrize("name", sorted(wc.BLOBS))
def test_restated_fit_equals_scipy_and_sklearn(name):
    from sklearn.cluster import AgglomerativeClustering
    from sklearn.metrics import adjusted_rand_score
    from scd_amd.ward import cut_tree
    f = wc.solved(name)
    x64, z = f["x"].astype(np.float64), f["Z"]
    n = len(x64)
    zs = scipy_h.linkage(x64, "ward")
    hs, hz = np.sort(zs[:, 2]), np.sort(z[:, 2])
    dev = float((np.abs(hs - hz) / hs).max())
    print("%s: largest relative height deviation %.3e" % (name, dev))
    for k in _cuts(name):                                       # the cut is well defined: from scipy's own heights
        gap = (hs[n - k] - hs[n - k - 1]) / hs[n - k]
        assert gap > 100 * dev, (k, gap, dev)
    assert dev <= HEIGHT_TOL
    assert f["full_requeries"] == 0 and f["inversions"] == 0
    for k in _cuts(name):
        mine = cut_tree(z, k)
        assert len(np.unique(mine)) == k
        assert adjusted_rand_score(mine, scipy_h.fcluster(zs, k, "maxclust")) == 1.0
        sk = AgglomerativeClustering(n_clusters=k, linkage="ward", compute_distances=True).fit(x64)
        assert adjusted_rand_score(mine, sk.labels_) == 1.0
        assert np.abs(np.sort(sk.distances_) - hz).max() <= HEIGHT_TOL * hz.max()


@pytest.mark.parametrize("name", sorted(wc.BLOBS))
def test_cut_tree_equals_fcluster_on_scipys_own_tree(name):
    from scd_amd.ward import cut_tree
    x64 = wc.solved(name)["x"].astype(np.float64)
    zs = scipy_h.linkage(x64, "ward")
    for k in _cuts(name) + (1, len(x64)):
        mine = cut_tree(zs, k)
        assert np.array_equal(mine, wc.partition_of(scipy_h.fcluster(zs, k, "maxclust")))
        assert np.array_equal(mine, wc.partition_of(mine))      # numbered by the lowest member row


def test_linkage_rows_follow_the_key_order():
    """A hand-made tree: merge 1 is the parent of merge 0 and an ulp lower; merge 2 lies between them in creation but below both."""
    from scd_amd.ward import cut_tree, linkage_from_merges
    lower = np.nextafter(1.0, 0.0)
    # leaves 0..4; created: t0 = (0, 1) at 1.0, t1 = (node 5, 2) at 1 - ulp (inverted), t2 = (3, 4) at 0.5, t3 = (6, 7) at 3.0
    for build in (linkage_from_merges, wc.linkage):
        z, inv = build(5, [0, 5, 3, 6], [1, 2, 4, 7], [1.0, lower, 0.5, 3.0])
        assert inv == 1
        assert z.tolist() == [[3.0, 4.0, 0.5, 2.0], [0.0, 1.0, 1.0, 2.0], [2.0, 6.0, lower, 3.0], [5.0, 7.0, 3.0, 5.0]]
    assert cut_tree(z, 3).tolist() == [0, 0, 1, 2, 2] and cut_tree(z, 2).tolist() == [0, 0, 0, 1, 1]
    with pytest.raises(ValueError):
        cut_tree(z, 6)


# ---------------------------------------------------------------------------------------------------- the cases say what they claim
def test_case_properties():
    sc = wc.search_cases()
    for name, c in sc.items():
        nn, cost = wc.nearest(c["q"], c["qcnt"], c["qself"], c["x"], c["xcnt"])
        c["nn"], c["cost"] = nn, cost
        live = nn >= 0
        assert (c["xcnt"][nn[live]] > 0).all() and (nn[live] != c["qself"][live]).all()
    assert sc["dead_all_but_self"]["nn"].tolist() == [-1] and np.isinf(sc["dead_all_but_self"]["cost"]).all()
    assert sc["dead_all_but_two"]["nn"].tolist() == [599, 77]
    assert sc["dead_all_but_two"]["cost"][0] == sc["dead_all_but_two"]["cost"][1]                 # the value is symmetric
    assert sc["rect_q1_free"]["nn"].tolist() == [999] and sc["rect_q1_free"]["cost"][0] == 0.0   # identical rows: exactly 0
    assert sc["rect_q1_self"]["nn"][0] != 999
    # the weight decides against the distance: for many queries the nearest row by distance alone is another one
    c = sc["sizes"]
    plain, _ = wc.nearest(c["q"], np.ones_like(c["qcnt"]), c["qself"], c["x"], (c["xcnt"] > 0).astype(np.int32))
    assert (plain != c["nn"]).sum() >= 20 and c["xcnt"].max() == 2 ** 20
    # exact ties on the grid, cost 0 ties on the duplicates, a column in the last tile as an answer
    g = wc.solved("grid1000")["rounds"][0]
    x = wc.solved("grid1000")["x"]
    cm = wc.pair_costs(x, g["cnt"], x, g["cnt"])
    np.fill_diagonal(cm, np.inf)
    assert ((cm == cm.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum() >= 100
    d = wc.solved("dups900")["rounds"][0]
    xd = wc.solved("dups900")["x"]
    same = (xd[:, None, :] == xd[None, :, :]).all(axis=2) & ~np.eye(900, dtype=bool)
    assert (d["cost"] == 0.0).all() and np.array_equal(d["nn"], np.argmax(same, axis=1))            # the lowest identical row
    t = wc.solved("t34_4300")["rounds"][0]
    assert t["nn"][wc.TWIN["t34_4300"]] == 4299
    assert len(wc.solved("n2")["rounds"]) == 1 and wc.solved("n2")["Z"].shape == (1, 4)
    assert (wc.solved("hub4200")["rounds"][0]["cost"][:3000] == 0.0).all()


def test_whole_fits_are_trees():
    for name in wc.FIT_CASES:
        f = wc.solved(name)
        z, n = f["Z"], len(f["x"])
        assert z.shape == (n - 1, 4) and z[-1, 3] == n
        assert (z[:, 0] < z[:, 1]).all() and (z[:, 1] < n + np.arange(n - 1)).all()               # a child comes before its parent
        assert len(np.unique(z[:, :2])) == 2 * n - 2
        work = sum(len(r["stale"]) * int((r["cnt"] > 0).sum()) for r in f["rounds"]) / n / n
        assert work < 4.0 or n < 10, (name, work)


# ---------------------------------------------------------------------------------------------------- the filter on the CPU
@pytest.mark.parametrize("name", sorted(wc.BLOBS) + ["grid1000"])
def test_filter_simulation_keeps_the_answer(name):
    rounds = wc.solved(name)["rounds"]
    walked = queries = 0
    for r in rounds[::4]:
        s = r["stale"]
        counts, bounded, covered = wc.simulate_filter(r["x"][s], r["cnt"][s], s, r["x"], r["cnt"], with_answer=True)
        assert covered.all()
        info = wc.filter_info(counts, bounded)
        walked += info[0]
        queries += len(s)
    if name in wc.BLOBS:                                        # the filter path is the common one
        assert walked < 0.1 * queries, (walked, queries)


# ---------------------------------------------------------------------------------------------------- planted mistakes
def test_planted_mistakes_are_shown():
    sc = wc.search_cases()

    def differs(name, mistake):
        c = sc[name]
        good, bad = wc.nearest(c["q"], c["qcnt"], c["qself"], c["x"], c["xcnt"]), wc.nearest(c["q"], c["qcnt"], c["qself"], c["x"], c["xcnt"], mistake)
        return not np.array_equal(good[0], bad[0])
    shown = {}
    shown["no_weight"] = differs("sizes", "no_weight")
    shown["sum_as_product"] = differs("sizes", "sum_as_product")
    shown["no_dead_mask"] = differs("dead_every_other_near", "no_dead_mask")
    shown["self"] = differs("rect_q130_self", "self")
    g = wc.solved("grid1000")["rounds"][0]
    shown["tie_high"] = not np.array_equal(wc.nearest(g["x"], g["cnt"], g["stale"], g["x"], g["cnt"], "tie_high")[0], g["nn"])
    r = wc.solved("blobs600")["rounds"][3]
    for mistake in ("unweighted_centroid", "merge_at_hi"):
        xa, ca = wc.merge(r["x"], r["cnt"], r["lo"], r["hi"], mistake)
        shown[mistake] = not (np.array_equal(xa, r["x_after"]) and np.array_equal(ca, r["cnt_after"]))
    shown["stale_kept"] = not np.array_equal(wc.fit(wc.make_case("blobs600"), "stale_kept")["Z"], wc.solved("blobs600")["Z"])
    r = wc.solved("blobs1500")["rounds"][0]
    s = r["stale"]
    assert wc.simulate_filter(r["x"][s], r["cnt"][s], s, r["x"], r["cnt"], with_answer=True)[2].all()
    shown["threshold_without_2wb"] = not wc.simulate_filter(r["x"][s], r["cnt"][s], s, r["x"], r["cnt"], mistake="threshold_without_2wb",
                                                            with_answer=True)[2].all()
    assert set(shown) == set(wc.MISTAKES)
    assert all(shown.values()), shown


# ---------------------------------------------------------------------------------------------------- ABI, workspace, arguments
def test_abi_has_the_ward_entries():
    from scd_amd import _lib as abi, build
    hdr = open(os.path.join(ROOT, "include", "scd_hip.h")).read()
    lib = _lib()
    for name in ("scd_ward_nearest_ws_bytes", "scd_ward_nearest", "scd_ward_merge"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in abi.SIGNATURES and hasattr(lib, name)
    assert len(abi.SIGNATURES["scd_ward_nearest"][1]) == 16 and len(abi.SIGNATURES["scd_ward_merge"][1]) == 11
    assert "ward.hip" in build.SOURCES


def test_workspace_of_a_fit_fits():
    L = _lib()
    nb = L.scd_ward_nearest_ws_bytes(126976, 126976, 768)
    assert 0 < nb <= 2 << 30
    assert L.scd_ward_nearest_ws_bytes(1, 126976, 768) < nb
    assert L.scd_ward_nearest_ws_bytes(0, 8, 8) == 0 and L.scd_ward_nearest_ws_bytes(1, 1, 8) == 0
    assert L.scd_ward_nearest_ws_bytes(1, 1 << 29, 8) == 0 and L.scd_ward_nearest_ws_bytes(10, 100, 1025) == 0


def test_estimator_names_what_it_does_not_support():
    from scd_amd.ward import Ward
    for kw, word in ((dict(linkage="average"), "linkage"), (dict(linkage="complete"), "linkage"), (dict(connectivity=np.eye(3)), "connectivity"),
                     (dict(distance_threshold=0.5), "distance_threshold"), (dict(metric="manhattan"), "metric"), (dict(n_clusters=None), "n_clusters"),
                     (dict(n_clusters=0), "n_clusters"), (dict(bogus=1), "bogus")):
        with pytest.raises(ValueError, match=word):
            Ward(**kw)
    w = Ward(n_clusters=7, linkage="ward", metric="euclidean", compute_distances=True, connectivity=None)
    assert (w.n_clusters, w.normalize) == (7, False)


def test_scripts_take_ward():
    import importlib
    mu = importlib.import_module("main_unsup")
    a = mu.build_parser().parse_args(["--cluster", "WARD", "--n_cluster", "100", "--dataset_name", "cub", "--feat_model", "clip", "--pca_dim", "32"])
    assert mu.cluster_result_name(a) == "WARD_clip_cub_100_pca32.pt"
    assert "WARD" in mu.build_parser().format_help()
    ek = importlib.import_module("estimate_k")
    a = ek.parse_args(["--root_dir", "r", "--dataset_name", "d", "--clusterer", "ward", "--criterion", "silhouette"])
    assert (a.clusterer, a.search_mode, a.min_classes) == ("ward", "grid", 2)
    assert ek.parse_args(["--root_dir", "r", "--dataset_name", "d"]).clusterer == "kmeans"
    with pytest.raises(SystemExit, match="bic"):
        ek.parse_args(["--root_dir", "r", "--dataset_name", "d", "--clusterer", "ward", "--criterion", "bic"])
    with pytest.raises(SystemExit):
        ek.parse_args(["--root_dir", "r", "--dataset_name", "d", "--clusterer", "average"])
