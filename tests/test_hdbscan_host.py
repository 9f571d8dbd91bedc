"""CPU tests of the HDBSCAN feature (docs/design/hdbscan.md): the float64 restatement of tests/hdbscan_cases.py against scipy and
scikit-learn, each case's named property, each planted mistake, and the host solver scd_hdbscan_tree against scikit-learn's own
make_single_linkage + tree_to_labels on the same sorted edges.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import hdbscan_cases as hc
import knn_cases as kc

sklearn = pytest.importorskip("sklearn")


def _lib():
    from scd_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------------- the cases say what they claim
def test_case_properties():
    c = hc.solved("blobs660")
    assert len(c["x"]) == 5 * 128 + 20                          # 6 panels, the last with 20 rows
    c = hc.solved("plain900")
    assert np.isinf(c["core"]).all() and np.array_equal(c["r"], c["v"])       # no clamp: the Euclidean MST
    c = hc.solved("t34_4300")
    n = len(c["x"])
    assert n % 128 == 76 and all(hc.ranges(n, cu) == (17, 2) for cu in (256, 304)) and hc.ranges(n, 64)[1] > 1
    assert hc.nearest_round(c["r"], np.arange(n))[0][c["twin"]] == n - 1    # the last column is a row's answer
    c = hc.solved("grid1000")
    assert np.array_equal(kc.f16_flushed(c["x"]), c["x"])                     # every fp16 copy is exact
    assert len(c["r_mst"]) - len(np.unique(c["r_mst"])) >= 300                # hundreds of exact ties among the tree's edges
    c = hc.solved("dups900")
    assert int((c["weight"] == 0.0).sum()) == 600                             # lambda = inf in the tree
    assert np.array_equal(c["x"], c["raw"])                                   # exactly unit rows: normalising changes nothing
    c = hc.solved("hub4200")
    counts, bounded, _ = hc.simulate_filter(c["x"], c["core"], np.arange(len(c["x"])))
    # the 3,000 copies tie with each other: their slots overflow (2,999 candidates) and they walk; the 1,200 rows around them have
    # nearer rows among themselves than the hub and pass the filter; one round joins everything
    assert bounded.all() and (counts[:3000] > hc.SLOTS).all() and (counts[3000:] <= hc.SLOTS).any() and len(c["comps"]) == 1
    assert -(-len(c["x"]) // kc.CHUNK) == 10
    for name in ("flagged449", "flagged1345"):
        c = hc.solved(name)
        with np.errstate(over="ignore"):
            assert np.isinf(c["x"].astype(np.float16)).any()                 # the fp16 flag
    assert len(hc.solved("flagged449")["x"]) == kc.CHUNK + 1 and len(hc.solved("flagged1345")["x"]) == 3 * kc.CHUNK + 1
    assert len(hc.solved("n2")["x"]) == 2 and len(hc.solved("n129")["x"]) == 129


def test_plain_mst_weight_equals_scipy():
    from scipy.sparse.csgraph import minimum_spanning_tree
    c = hc.solved("plain900")
    x = c["x"].astype(np.float64)
    dist = np.sqrt(np.maximum(0.0, 2.0 - 2.0 * (x @ x.T)))
    want = minimum_spanning_tree(dist).sum()
    assert abs(c["weight"].sum() - want) <= 1e-9 * want


@pytest.mark.parametrize("name", hc.CASES)
def test_mst_is_a_sorted_spanning_tree(name):
    c = hc.solved(name)
    n = len(c["x"])
    lo, hi, r = c["lo"], c["hi"], c["r_mst"]
    assert len(lo) == n - 1 and (lo < hi).all()
    assert np.array_equal(np.lexsort((hi, lo, -r)), np.arange(n - 1)) and (np.diff(c["weight"]) >= 0).all()
    assert len(np.unique(hc.merge(np.arange(n), lo, hi))) == 1
    assert np.array_equal(r, c["r"][lo, hi])


@pytest.mark.parametrize("name", hc.BLOBS)
def test_pipeline_equals_sklearn_brute(name):
    from sklearn.cluster import HDBSCAN
    from sklearn.metrics import adjusted_rand_score
    c = hc.solved(name)
    ref = HDBSCAN(min_cluster_size=c["min_cluster_size"], min_samples=c["min_samples"], algorithm="brute", metric="euclidean",
                  copy=True).fit(c["x"].astype(np.float64))
    lab, _ = hc.sklearn_labels(c["lo"], c["hi"], c["weight"], c["min_cluster_size"])
    assert (int(ref.labels_.max()) + 1, int((ref.labels_ < 0).sum())) == hc.SKLEARN_FINDS[name]
    assert adjusted_rand_score(ref.labels_, lab) == 1.0 and np.array_equal(ref.labels_ < 0, lab < 0)
    if name == "blobs900":
        assert np.array_equal(ref.labels_, lab)                 # the numbering as well


@pytest.mark.parametrize("name", hc.BLOBS)
def test_filter_simulation_keeps_the_answer_and_the_slots(name):
    c = hc.solved(name)
    for comp in c["comps"]:
        counts, bounded, covered = hc.simulate_filter(c["x"], c["core"], comp, v=c["v"])
        assert bounded.all() and covered.all() and int((counts > hc.SLOTS).sum()) == 0


def test_filter_cap_holds_on_the_cpu():
    """The cap of tests/test_gpu_hdbscan.py on the simulation: no row walks on the cap's cases."""
    for name in hc.FILTER_CAP_CASES:
        c = hc.solved(name)
        walk = sum(hc.filter_info(*hc.simulate_filter(c["x"], c["core"], comp)[:2])[0] for comp in c["comps"])
        assert walk == 0


# ---------------------------------------------------------------------------------------------------- planted mistakes
def _same_mst(c, got):
    return np.array_equal(got[0], c["lo"]) and np.array_equal(got[1], c["hi"]) and np.array_equal(got[2], c["r_mst"])


def test_planted_mistakes_are_shown():
    c = hc.solved("blobs660")
    assert not _same_mst(c, hc.boruvka(hc.reach(c["v"], hc.core_dots(c["v"], c["min_samples"], "core_off_by_one"))))
    c = hc.solved("blobs1650")
    n = len(c["x"])
    first = hc.nearest_round(c["r"], np.arange(n))
    assert not np.array_equal(hc.nearest_round(hc.reach(c["v"], c["core"], "no_cj_clamp"), np.arange(n))[1], first[1])
    sevens = hc.masks(n)["sevens"]
    assert not np.array_equal(hc.nearest_round(c["r"], sevens, "no_mask")[0], hc.nearest_round(c["r"], sevens)[0])
    c = hc.solved("grid1000")
    n = len(c["x"])
    assert not np.array_equal(hc.nearest_round(c["r"], np.arange(n), "tie_high")[0], hc.nearest_round(c["r"], np.arange(n))[0])
    assert not _same_mst(c, hc.boruvka(c["r"], "component_best_by_r"))
    c = hc.solved("blobs660")                                   # the threshold without min(c_i, .) loses the answer of some row
    assert not hc.simulate_filter(c["x"], c["core"], c["comps"][0], v=c["v"], mistake="threshold_without_ci")[2].all()
    assert set(hc.MISTAKES) == {"core_off_by_one", "no_cj_clamp", "tie_high", "no_mask", "component_best_by_r", "threshold_without_ci"}


# ---------------------------------------------------------------------------------------------------- the host solver
def _tree(lo, hi, w, mcs, method, single):
    from scd_amd import ops
    return ops.hdbscan_tree(lo, hi, w, mcs, method, single)


def _check_tree(lo, hi, w, what):
    n = len(lo) + 1
    for method in ("eom", "leaf"):
        for single in (False, True):
            for mcs in (2, 5, 15):
                want, wprob = hc.sklearn_labels(lo, hi, w, mcs, method, single)
                got, prob, k = _tree(lo, hi, w, mcs, method, single)
                tag = "%s n=%d %s single=%s mcs=%d" % (what, n, method, single, mcs)
                assert np.array_equal(got, want), tag
                assert np.array_equal(np.isnan(prob), np.isnan(wprob)) and np.all(np.abs(prob - wprob)[~np.isnan(wprob)] <= 1e-12), tag
                assert k == int(want.max()) + 1, tag


@pytest.mark.parametrize("name", hc.CASES)
def test_tree_equals_sklearn_on_the_cases(name):
    """Fails without the feature: the symbol scd_hdbscan_tree is absent."""
    c = hc.solved(name)
    _check_tree(c["lo"], c["hi"], c["weight"], name)


def _random_tree(rs, n, weights):
    perm = rs.permutation(n)
    a = perm[1:]
    b = np.array([perm[rs.randint(0, i + 1)] for i in range(n - 1)])
    w = weights(rs, n - 1)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    order = np.lexsort((hi, lo, w))
    return lo[order].astype(np.int32), hi[order].astype(np.int32), w[order]


WEIGHTS = {"random": lambda rs, m: rs.rand(m) + 0.01, "tied": lambda rs, m: rs.randint(1, 6, size=m) / 4.0,
           "zeros": lambda rs, m: np.where(rs.rand(m) < 0.3, 0.0, rs.randint(1, 4, size=m) / 2.0)}


@pytest.mark.parametrize("kind", sorted(WEIGHTS))
def test_tree_equals_sklearn_on_random_trees(kind):
    rs = np.random.RandomState(7)
    for n in (2, 3, 16, 17, 64, 200, 700):
        for _ in range(3):
            _check_tree(*_random_tree(rs, n, WEIGHTS[kind]), what=kind)


def test_tree_equals_sklearn_on_a_path_a_star_and_two_points():
    rs = np.random.RandomState(8)
    n = 400
    i = np.arange(n - 1, dtype=np.int32)
    for w in (np.sort(rs.rand(n - 1)), np.full(n - 1, 0.5), np.linspace(0.0, 1.0, n - 1)):
        _check_tree(i, i + 1, w, "path")
        _check_tree(np.zeros(n - 1, dtype=np.int32), i + 1, w, "star")
    _check_tree(np.array([0], dtype=np.int32), np.array([1], dtype=np.int32), np.array([0.25]), "n2")
    _check_tree(np.array([0], dtype=np.int32), np.array([1], dtype=np.int32), np.array([0.0]), "n2 at weight 0")


def test_tree_takes_a_long_path_without_recursion():
    n = 126976
    i = np.arange(n - 1, dtype=np.int32)
    labels, prob, k = _tree(i, i + 1, np.linspace(0.1, 1.0, n - 1), 5, "eom", True)
    assert labels.shape == (n,) and prob.shape == (n,) and k >= 1 and labels.max() == k - 1


def test_tree_rejects_what_is_no_spanning_tree():
    from scd_amd import _lib
    L = _lib.load()
    lo, hi, w = np.array([0, 1, 2], dtype=np.int32), np.array([1, 2, 3], dtype=np.int32), np.array([0.1, 0.2, 0.3])
    labels, prob = np.zeros(8, dtype=np.int32), np.zeros(8)

    def args(lo, hi, w, n, mcs):
        return L.scd_hdbscan_tree(_lib.ptr(lo), _lib.ptr(hi), _lib.ptr(w), n, mcs, 0, 0, _lib.ptr(labels), _lib.ptr(prob), C.byref(C.c_int32(0)))
    assert args(lo, hi, w, 4, 2) == 0
    assert args(lo, hi, w, 1, 2) == _lib.SCD_EINVAL                                           # n < 2
    assert args(lo, hi, w, 4, 1) == _lib.SCD_EINVAL                                           # min_cluster_size < 2
    assert args(lo, np.array([1, 2, 0], dtype=np.int32), w, 4, 2) == _lib.SCD_EINVAL          # a cycle, row 3 in no edge
    assert args(lo, np.array([1, 2, 4], dtype=np.int32), w, 4, 2) == _lib.SCD_EINVAL          # an index outside [0, n)
    assert args(np.array([0, -1, 2], dtype=np.int32), hi, w, 4, 2) == _lib.SCD_EINVAL
    with pytest.raises(_lib.ScdError):
        _tree(lo, hi, w, 5, "median", False)


def test_workspace_of_a_round_fits():
    L = _lib()
    nb = L.scd_mr_nearest_ws_bytes(126976, 768)
    assert 0 < nb <= 2 << 30
    assert L.scd_mr_nearest_ws_bytes(1, 8) == 0 and L.scd_mr_nearest_ws_bytes(1 << 31, 8) == 0 and L.scd_mr_nearest_ws_bytes(100, 1025) == 0


def test_estimator_names_what_it_does_not_support():
    from scd_amd.hdbscan import HDBSCAN, _check_min_samples
    for kw, word in ((dict(cluster_selection_epsilon=0.5), "cluster_selection_epsilon"), (dict(max_cluster_size=100), "max_cluster_size"),
                     (dict(metric="manhattan"), "metric"), (dict(alpha=0.5), "alpha"), (dict(store_centers="centroid"), "store_centers"),
                     (dict(cluster_selection_method="median"), "cluster_selection_method"), (dict(min_cluster_size=1), "min_cluster_size"),
                     (dict(leaf_size=40), "leaf_size")):
        with pytest.raises(ValueError, match=word):
            HDBSCAN(**kw)
    HDBSCAN(cluster_selection_epsilon=0.0, metric="euclidean")
    for n, ms in ((100, 66), (100, 0), (10, 11), (1, 1)):
        with pytest.raises(ValueError, match="limit"):
            _check_min_samples(n, ms)


def test_tree_under_sanitizers(tmp_path):
    """hdbscan_tree.cpp compiled for the host with clang's AddressSanitizer + UndefinedBehaviorSanitizer and driven by
    tests/sanitize_hdbscan.cpp, a stand-alone program: paths, stars and random trees at every parameter combination, a path of 126,976
    nodes, the refused inputs - and no sanitizer report."""
    import os
    import shutil
    import subprocess
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        clang = shutil.which("clang++")
    if not clang:
        pytest.skip("no clang++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "scd_amd", "csrc")
    exe = str(tmp_path / "sanitize_hdbscan")
    cmd = [clang, "-x", "c++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(root, "include"), "-I", src,
           os.path.join(src, "hdbscan_tree.cpp"), os.path.join(root, "tests", "sanitize_hdbscan.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr


def test_main_unsup_takes_hdbscan():
    import importlib
    mu = importlib.import_module("main_unsup")
    a = mu.build_parser().parse_args(["--cluster", "HDBSCAN", "--min_cluster_size", "50", "--dataset_name", "cub", "--feat_model", "clip"])
    assert (a.cluster, a.min_cluster_size, a.min_samples) == ("HDBSCAN", 50, None)
    assert mu.cluster_result_name(a) == "HDBSCAN_clip_cub_mcs50.pt"
    a = mu.build_parser().parse_args(["--cluster", "HDBSCAN", "--min_samples", "10", "--dataset_name", "cub", "--feat_model", "clip"])
    assert mu.cluster_result_name(a) == "HDBSCAN_clip_cub_mcs5_ms10.pt"
    a = mu.build_parser().parse_args(["--cluster", "KM", "--n_cluster", "100", "--dataset_name", "cub", "--feat_model", "clip"])
    assert mu.cluster_result_name(a) == "KM_clip_cub_100.pt"                  # every other --cluster value names its file as before
    assert "HDBSCAN" in mu.build_parser().format_help()
