"""CPU checks of the k-NN tests' own yardstick (tests/knn_cases.py) and of score_features.py's host side.  No device is used.

The restatement is compared with scikit-learn on blob cases whose margins make that a fair demand - the margins are asserted first, so
no row is left out of a comparison.  The two larger blob cases that the GPU test sends through the filter (knn_cases.BLOBS) have rows
whose k-th and (k + 1)-th values lie closer than 1e-5 (3,000 rows cannot all keep that distance), so they are not compared with
scikit-learn; for them this file asserts what the GPU test relies on: the simulated filter gives every row at most half the slots.
The cases named for a code path (several tiles per range, many chunks of the exact pass, negative dots) get their structural facts
asserted here, and each planted mistake of such a path must change the float64 answer on the cases named for it."""
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


# ------------------------------------------------------------------------------------------------- the cases named for a code path
# What tests/test_gpu_knn.py relies on when it says that a case runs a path: asserted here from the cases and the float64 answer alone.
@pytest.fixture(scope="module")
def tiles():
    return kc.tile_cases()


@pytest.fixture(scope="module")
def chunked():
    cases = kc.chunk_cases()
    return {name: (case, kc.knn_f64(case["q"], case["x"], case["k"], case["self_base"])) for name, case in cases.items()}


@pytest.fixture(scope="module")
def negative():
    cases = kc.negative_cases()
    return {name: (case, kc.knn_f64(case["q"], case["x"], case["k"], case["self_base"])) for name, case in cases.items()}


def test_ranges_rule():
    assert kc.ranges(3000, 3000, 20) == (24, 1) and kc.ranges(1000, 1000, 64) == (8, 1)        # the largest cases before: one tile per range
    assert kc.ranges(129, 4097, 17, cu=1) == (5, 7) and kc.ranges(4225, 4225, 20, cu=8) == (5, 7)       # k / 4 ranges at the least
    assert kc.ranges(4225, 4225, 20, cu=304) == (17, 2)         # 4 cu / panels = 36 ranges wanted, ny_max = 31 given
    assert kc.ranges(126976, 126976, 20) == (5, 199) and kc.ranges(1, 2, 1) == (1, 1)


# name -> (m, n, d, k, (ranges, tiles per range) on 256 compute units, tiles of the last range)
TILE_SHAPES = {"t33_q129": (129, 4097, 33, 17, (17, 2), 1), "t65_q129": (129, 8200, 64, 16, (22, 3), 2), "t34_k64": (260, 4225, 40, 64, (17, 2), 2),
               "border_shard": (260, 4300, 64, 12, (17, 2), 2), "graph_4225": (4225, 4225, 32, 20, (17, 2), 2)}
# the simulated candidates per row (least, most)
TILE_COUNTS = {"t33_q129": (17, 24), "t65_q129": (16, 20), "t34_k64": (67, 83), "border_shard": (12, 17), "graph_4225": (20, 26)}


@pytest.mark.parametrize("name", list(TILE_SHAPES))
def test_tile_cases_have_several_tiles_per_range(tiles, name):
    case = tiles[name]
    m, n, d, k, at256, last = TILE_SHAPES[name]
    assert (case["q"].shape, case["x"].shape, case["k"]) == ((m, d), (n, d), k)
    xtiles = -(-n // kc.TILE)
    assert xtiles > 32 and kc.ranges(m, n, k) == at256
    for cu in (64, 256, 304):
        ny, per = kc.ranges(m, n, k, cu)
        assert per >= 2 and ny * per >= xtiles > (ny - 1) * per and ny <= 32
    ny, per = at256
    assert xtiles - (ny - 1) * per == last                      # t33, t65: a last range cut short by the tile count
    counts = kc.simulate_filter(case, SLOTS)
    print("%s: simulated candidates per row %d .. %d" % (name, counts.min(), counts.max()))
    assert (int(counts.min()), int(counts.max())) == TILE_COUNTS[name]
    assert k <= counts.min() and counts.max() <= SLOTS // 2     # the filter decides every row: the exact pass alone cannot pass the case


def test_tile_case_plants(tiles):
    case = tiles["t33_q129"]
    assert 4097 - 32 * kc.TILE == 1                             # the last tile: ONE valid column next to 127 padding columns
    idx, dot = kc.knn_f64(case["q"], case["x"], case["k"], -1)
    assert idx[5][0] == 4096 and idx[77][0] == 4095
    case = tiles["border_shard"]
    a, b = kc.BORDER
    assert case["self_base"] == a and np.array_equal(case["q"], case["x"][a:b])
    assert {a // kc.TILE, (b - 1) // kc.TILE} == {31, 33} and 33 % kc.ranges(b - a, 4300, 12)[1] == 1        # tile 33: the second of its range
    idx, dot = kc.knn_f64(case["q"], case["x"], case["k"], a)
    ties = np.diff(dot, axis=1) == 0
    assert ties.sum() >= 100 and np.array_equal(dot * 64, np.round(dot * 64)) and np.abs(dot).max() < 16
    assert np.array_equal(kc.f16_flushed(case["x"]), case["x"])
    case = tiles["graph_4225"]
    assert case["q"] is case["x"] or np.array_equal(case["q"], case["x"])


# name -> (m, n, k, chunks, columns of the last chunk)
CHUNK_SHAPES = {"hub": (200, 4200, 10, 10, 168), "offset": (200, 4200, 10, 10, 168), "flagged_1345_k64": (1345, 1345, 64, 4, 1),
                "flagged_896": (896, 896, 64, 2, 448), "flagged_449": (449, 449, 64, 2, 1)}


@pytest.mark.parametrize("name", list(CHUNK_SHAPES))
def test_chunk_cases_cross_chunks(chunked, name):
    case, (idx, dot) = chunked[name]
    m, n, k, chunks, last = CHUNK_SHAPES[name]
    assert (case["q"].shape[0], case["x"].shape[0], case["k"], kc.chunks_of(case), n - kc.CHUNK * (chunks - 1)) == (m, n, k, chunks, last)
    assert kc.CHUNK + 64 == SLOTS                               # 64 best so far + a full chunk fill the LDS arrays exactly
    of = idx // kc.CHUNK
    both = ((of == 0).any(1) & (of == chunks - 1).any(1)).sum()
    later = (of[:, -1] > of[:, 0]).sum()
    print("%s: %d rows with columns of the first and the last chunk, %d rows whose last place comes from a later chunk than the first; "
          "%.3f of the columns in chunk 0, %.3f in the last" % (name, both, later, (of == 0).mean(), (of == chunks - 1).mean()))
    assert both >= 1 and later >= 1
    assert (np.diff(dot, axis=1) < 0).all()                     # distinct values: no tie decides anything here
    big = np.abs(case["x"]).max()
    if name == "hub":
        assert 65504 > big > 4000 and ((of == 0).sum(), (of == 9).sum()) == (222, 197)          # 11 % and 10 % of the 2,000 answer columns
    if name == "offset":
        assert (case["x"] > 7.5).all() and big < 8.5
    if name in ("hub", "offset"):                               # every row has a bound and far more candidates than slots
        counts, bounded = kc.simulate_filter(case, SLOTS, with_bound=True)
        print("%s: simulated candidates per row %d .. %d" % (name, counts.min(), counts.max()))
        assert bounded.all() and counts.min() > 6 * SLOTS
        assert kc.filter_info(case, SLOTS)[:2] == (m, m)
        if name == "hub":
            assert (int(counts.min()), int(counts.max())) == (4198, 4199)
    else:
        assert big == 131072.0 and k + kc.CHUNK == SLOTS
        assert (idx == n - 1).any(1).sum() == {"flagged_1345_k64": 54, "flagged_896": 20, "flagged_449": 65}[name]


def test_negative_cases_are_negative(negative):
    for name, (case, (idx, dot)) in negative.items():
        print("%s: largest dot of the answer %.6g" % (name, dot.max()))
        assert dot.max() < 0 and case["x"].shape[0] % kc.TILE != 0
    assert negative["neg_q130"][1][1].max() < -22 and negative["neg_flagged"][1][1].max() < -22
    case = negative["neg_q130"][0]
    assert case["x"].shape == (4200, 40) and kc.ranges(130, 4200, 9) == (17, 2) and 33 * kc.TILE - 4200 == 24
    counts = kc.simulate_filter(case, SLOTS)
    assert (int(counts.min()), int(counts.max())) == (9, 13)
    case = negative["neg_flagged"][0]
    assert np.abs(case["x"]).max() == 131072.0 and case["self_base"] == 300 and np.array_equal(case["q"], -case["x"][300:430])
    case, (idx, dot) = negative["simplex120"]
    assert case["x"].shape == (120, 128) and (dot == -1.0 / 128).all()
    assert list(idx[0]) == [1, 2, 3, 4, 5] and list(idx[3]) == [0, 1, 2, 4, 5] and list(idx[119]) == [0, 1, 2, 3, 4]
    g = case["x"].astype(np.float64) @ case["x"].astype(np.float64).T
    assert (g[~np.eye(120, dtype=bool)] == -1.0 / 128).all() and np.array_equal(kc.f16_flushed(case["x"]), case["x"])


def test_same_no_self_case():
    case = kc.same_no_self_case()
    assert case["self_base"] == -1 and case["x"].shape == (1000, 64)
    idx, dot = kc.knn_f64(case["q"], case["x"], case["k"], -1)
    first = np.arange(1000)
    first[11:14] = 10
    assert np.array_equal(idx[:, 0], first)
    for i in range(10, 14):
        assert list(idx[i][:4]) == [10, 11, 12, 13]


def model_cases():
    return {"border_shard": kc.tile_cases()["border_shard"], "ties": kc.tie_case(), "simplex120": kc.negative_cases()["simplex120"]}


@pytest.mark.parametrize("name", ["border_shard", "ties", "simplex120"])
def test_model_is_exact_and_stable_on_the_grid_cases(name):
    """What lets tests/test_gpu_knn.py demand info == the model: every fp16 copy is exact (e_i = 0), every dot is exact in fp32 in any
    order, and no count moves when B_i is scaled by 1 +- 2^-10 - far more than the float32 rounding of h_i and h_max (2^-23 relative)."""
    case = model_cases()[name]
    q, x = case["q"], case["x"]
    assert np.array_equal(kc.f16_flushed(x), x) and np.array_equal(kc.f16_flushed(q), q)
    g = q.astype(np.float64) @ x.astype(np.float64).T
    # multiples of 2^-14 below 2^9: 23 bits, as is every partial sum (sum |q_c x_c| obeys the same bound)
    assert np.array_equal(g * 2.0 ** 14, np.round(g * 2.0 ** 14)) and (np.abs(q).astype(np.float64) @ np.abs(x).astype(np.float64).T).max() < 2.0 ** 9
    for cu in (64, 256, 304):
        counts = kc.simulate_filter(case, SLOTS, cu)
        for scale in (1 - 2.0 ** -10, 1 + 2.0 ** -10):
            assert np.array_equal(kc.simulate_filter(case, SLOTS, cu, scale=scale), counts)
    print("%s: model info %s" % (name, kc.filter_info(case, SLOTS)))
    assert kc.filter_info(case, SLOTS) == {"border_shard": (0, 0, 17), "ties": (0, 0, 9), "simplex120": (0, 0, 119)}[name]


def test_every_path_mistake_shows_on_its_named_cases(tiles, chunked, negative):
    named = dict(tiles)
    named.update({n: c for n, (c, _) in chunked.items()})
    named.update({n: c for n, (c, _) in negative.items()})
    where = {"first_tile_only": ("t33_q129", "t65_q129", "border_shard"), "first_chunk_only": ("hub", "flagged_1345_k64"),
             "pad_cols": ("neg_q130", "simplex120"), "self_zero": ("neg_flagged",)}
    assert set(where) == set(kc.PATH_MISTAKES)
    for mistake, names in where.items():
        for name in names:
            assert _knn_differs(named[name], mistake), "%s does not show the planted mistake %r" % (name, mistake)


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
