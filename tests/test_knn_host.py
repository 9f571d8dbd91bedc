"""CPU checks of the k-NN tests' own yardstick (tests/knn_cases.py) and of score_features.py's host side.  No device is used.

The restatement is compared with scikit-learn on blob cases whose margins make that a fair demand - the margins are asserted first, so
no row is left out of a comparison.  The two larger blob cases that the GPU test sends through the filter (knn_cases.BLOBS) have rows
whose k-th and (k + 1)-th values lie closer than 1e-5 (3,000 rows cannot all keep that distance), so they are not compared with
scikit-learn; for them this file asserts what the GPU test relies on: the simulated filter gives every row at most half the slots."""
import argparse
import os

import numpy as np
import pytest
import torch

import knn_cases as kc

SLOTS = 512             # scd_knn_slots(); tests/test_gpu_knn.py asserts the library agrees


@pytest.fixture(scope="module")
def small():
    return {name: kc.blob_case(name) for name in kc.SMALL_BLOBS}


@pytest.mark.parametrize("name", list(kc.SMALL_BLOBS))
def test_restatement_equals_sklearn_neighbours(small, name):
    from sklearn.neighbors import NearestNeighbors
    case = small[name]
    gap, _ = kc.margins(case)
    print("%s: smallest k-th / (k+1)-th gap %.3g" % (name, gap))
    assert gap >= kc.MIN_VALUE_GAP
    x64 = case["x"].astype(np.float64)
    nn = NearestNeighbors(n_neighbors=case["k"] + 1, metric="cosine", algorithm="brute").fit(x64)
    dist, ind = nn.kneighbors(x64)
    assert np.array_equal(ind[:, 0], np.arange(len(x64)))      # a row is its own nearest: the graph drops it
    idx, dot = kc.knn_f64(case["q"], case["x"], case["k"], 0)
    assert np.array_equal(idx, ind[:, 1:])
    nrm = np.sqrt((x64 * x64).sum(1))                           # fp32 unit rows are unit to 2^-24 or so; scikit-learn divides by the norms
    np.testing.assert_allclose(dot / (nrm[:, None] * nrm[idx]), 1.0 - dist[:, 1:], rtol=0, atol=1e-12)


def test_restatement_equals_sklearn_classifier(small):
    """Leave-one-out uniform vote = KNeighborsClassifier asked for k + 1 neighbours of a training row, minus the row itself; done with
    kneighbors + the classifier's own rule on a query set instead: fit on all rows but one block, predict the block."""
    from sklearn.neighbors import KNeighborsClassifier
    case = small["v500"]
    gap, score_gap = kc.margins(case)
    print("v500: value gap %.3g, class-score gap %.3g" % (gap, score_gap))
    assert gap >= kc.MIN_VALUE_GAP and score_gap >= kc.MIN_SCORE_GAP
    x, y, k = case["x"], case["labels"], case["k"]
    train, test = np.arange(100, 500), np.arange(0, 100)
    q_gap, q_score = kc.margins(dict(q=x[test], x=x[train], k=k, self_base=-1, labels=y[train]))
    assert q_gap >= kc.MIN_VALUE_GAP and q_score >= kc.MIN_SCORE_GAP
    clf = KNeighborsClassifier(n_neighbors=k, weights="uniform", metric="cosine", algorithm="brute").fit(x[train].astype(np.float64), y[train])
    idx, dot = kc.knn_f64(x[test], x[train], k, -1)
    pred, score = kc.vote_f64(idx, dot, y[train], mode="uniform")
    assert np.array_equal(pred, clf.predict(x[test].astype(np.float64)))
    assert np.array_equal(score, np.round(score)) and score.max() <= k


def test_dot64_is_order_exact_on_grid_rows():
    case = kc.tie_case()
    x = case["x"]
    g = x.astype(np.float64) @ x.astype(np.float64).T          # grid rows: exact in any order
    a, b = np.random.RandomState(0).randint(0, len(x), size=(2, 500))
    assert np.array_equal(kc.dot64(x[a], x[b]), g[a, b])


def test_tie_and_order_rules():
    case = kc.tie_case()
    idx, dot = kc.knn_f64(case["q"], case["x"], case["k"], 0)
    assert list(idx[10][:3]) == [11, 12, 13] and list(idx[13][:3]) == [10, 11, 12]         # duplicates tie: lowest columns first
    assert (np.diff(dot, axis=1) <= 0).all()
    ties = np.diff(dot, axis=1) == 0
    assert ties.any() and (np.diff(idx, axis=1)[ties] > 0).all()


# ------------------------------------------------------------------------------------------------- planted mistakes
def _knn_differs(case, mistake):
    a = kc.knn_f64(case["q"], case["x"], case["k"], case["self_base"])
    b = kc.knn_f64(case["q"], case["x"], case["k"], case["self_base"], mistake=mistake)
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


def test_every_planted_mistake_shows_on_a_named_case():
    named = {n: c for n, c in kc.shape_cases().items() if c["x"].shape[1] <= 64}                # the wide ones add time, not rules
    named.update(ties=kc.tie_case(), shard=kc.shard_case())
    shown = {m: [n for n, c in named.items() if _knn_differs(c, m)] for m in kc.KNN_MISTAKES}
    idx, dot, labels = kc.vote_case()
    good_u, good_s = kc.vote_f64(idx, dot, labels, mode="uniform")[0], kc.vote_f64(idx, dot, labels, mode="softmax")[0]
    shown["vote_tie_high"] = ["vote"] * (not np.array_equal(good_u, kc.vote_f64(idx, dot, labels, mode="uniform", mistake="vote_tie_high")[0]))
    shown["no_temperature"] = ["vote"] * (not np.array_equal(good_s, kc.vote_f64(idx, dot, labels, mode="softmax", mistake="no_temperature")[0]))
    print(shown)
    assert set(shown) == set(kc.MISTAKES)
    for m, where in shown.items():
        assert where, "no named case shows the planted mistake %r" % m
    assert shown["tie_high"] and "ties" in shown["tie_high"]
    assert shown["shard_base"] == ["shard"]                    # only a shard away from row 0 can tell
    assert good_u[0] == -1 and good_s[0] == -1                 # the row without a valid neighbour


# ------------------------------------------------------------------------------------------------- the filter cases
@pytest.mark.parametrize("name", list(kc.BLOBS))
def test_filter_cases_leave_half_the_slots_free(name):
    case = kc.blob_case(name)
    counts = kc.simulate_filter(case, SLOTS)
    print("%s: simulated candidates per row: max %d, mean %.1f (k = %d, %d slots)" % (name, counts.max(), counts.mean(), case["k"], SLOTS))
    assert counts.min() >= case["k"] and counts.max() <= SLOTS // 2


def test_simulated_filter_flags_rows_without_a_bound():
    case = kc.shape_cases()["n130_graph_k64"]                   # 18 kept columns < k = 64
    assert (kc.simulate_filter(case, SLOTS) == 2 * SLOTS + 1).all()
    assert (kc.simulate_filter(kc.overflow_case(SLOTS), SLOTS) == 2 * SLOTS + 2).all()    # every admissible column is a candidate


# ------------------------------------------------------------------------------------------------- score_features.py
def test_score_features_parser_and_cache_names():
    import score_features as sf
    a = sf.build_parser().parse_args(["--root_dir", "/r", "--dataset_name", "cub", "--feat_models", "clip", "dino_vit", "dinov2_vitb14"])
    assert (a.k, a.temperature, a.weights, a.clip_model) == (20, 0.07, "softmax", "ViT-B/16")
    assert a.feat_models == ["clip", "dino_vit", "dinov2_vitb14"]
    assert sf.cache_path(a, "clip") == "/r/extracted_features/clip_cub_all.pt"
    assert sf.cache_path(a, "dinov2_vitb14") == "/r/extracted_features/dinov2_vitb14_cub_all.pt"
    b = sf.build_parser().parse_args(["--root_dir", "/r", "--dataset_name", "cub", "--feat_models", "clip", "gcd", "--clip_model", "ViT-L/14",
                                      "--k", "5", "--weights", "uniform"])
    assert sf.cache_path(b, "clip") == "/r/extracted_features/clip_vit_l_14_cub_all.pt"
    assert sf.cache_path(b, "gcd") == "/r/extracted_features/gcd_cub_all.pt" and (b.k, b.weights) == (5, "uniform")
    with pytest.raises(SystemExit):
        sf.build_parser().parse_args(["--root_dir", "/r", "--dataset_name", "cub", "--feat_models", "clip", "--weights", "gaussian"])


def test_score_features_error_messages(tmp_path):
    import score_features as sf
    root = str(tmp_path)
    argv = ["--root_dir", root, "--dataset_name", "toy", "--feat_models", "dino_vit"]
    with pytest.raises(SystemExit) as ei:
        sf.main(argv)
    path = os.path.join(root, "extracted_features", "dino_vit_toy_all.pt")
    assert path in str(ei.value)
    os.makedirs(os.path.dirname(path))
    torch.save(dict(all_feats=np.zeros((6, 4), dtype=np.float32), mask_lab=np.zeros(6, dtype=bool), targets=np.arange(6)), path)
    with pytest.raises(SystemExit) as ei:
        sf.main(argv)
    msg = str(ei.value)
    assert "no labelled row" in msg and "estimate_k.py --criterion silhouette" in msg and path in msg
