"""CPU checks around the silhouette: the integer grid search, the float64 restatement against the scikit-learn golden, the sensitivity of
the GPU test's bounds to planted mistakes, the driver's parser and the ABI surface.  No GPU, no scikit-learn."""
import os
import re
import sys

import numpy as np
import pytest

import silhouette_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold(golden):
    return golden("silhouette.npz")


@pytest.fixture(scope="module")
def cases(gold):
    return sc.cases(gold)


@pytest.fixture(scope="module")
def dists(cases):
    """The float64 distance matrix of every case, computed once (blobs_true and blobs_fit share their rows)."""
    out = {}
    for name, (x, _, _) in cases.items():
        out[name] = out["blobs_true"] if name == "blobs_fit" else sc.distances_f64(x)
    return out


@pytest.fixture(scope="module")
def ek():
    from scd_amd import estimate_k
    return estimate_k


# ------------------------------------------------------------------------------------------------ grid_search
def test_grid_search_rounds_on_a_peak_at_20(ek):
    calls = []

    def f(K):
        calls.append(K)
        return -abs(K - 20)

    k, trace = ek.grid_search(f, 2, 64)
    assert k == 20
    assert [(ks, best) for ks, _, best in trace] == [([2, 10, 18, 25, 33, 41, 49, 56, 64], 18),
                                                      ([10, 12, 14, 16, 18, 19, 21, 23, 25], 19),      # 19 ties with 21: the lower K
                                                      ([18, 19, 20, 21], 20)]
    assert len(calls) == len(set(calls)) == 16 and sorted(calls) == sc.GRID_KS
    assert all(scores == [float(-abs(K - 20)) for K in ks] for ks, scores, _ in trace)


def test_grid_search_on_the_golden_table(ek, gold):
    table = {int(K): float(s) for K, s in zip(gold["blobs_ks"], gold["blobs_sil"])}
    assert sorted(table) == sc.GRID_KS
    k, trace = ek.grid_search(lambda K: table[K], 2, 64)               # a K outside the table would be a KeyError
    assert k == 20 and [best for _, _, best in trace] == [18, 19, 20]
    assert [ks for ks, _, _ in trace] == [[2, 10, 18, 25, 33, 41, 49, 56, 64], [10, 12, 14, 16, 18, 19, 21, 23, 25], [18, 19, 20, 21]]


def test_grid_search_edges(ek):
    assert ek.grid_search(lambda K: K, 2, 64)[0] == 64                  # best at the upper end
    assert ek.grid_search(lambda K: -K, 2, 64)[0] == 2                  # ... at the lower end
    k, trace = ek.grid_search(lambda K: -abs(K - 4), 2, 6)              # big_k - small_k < points: one round over every integer
    assert k == 4 and len(trace) == 1 and trace[0][0] == [2, 3, 4, 5, 6]
    k, trace = ek.grid_search(lambda K: 0.0, 3, 4)
    assert k == 3 and trace == [([3, 4], [0.0, 0.0], 3)]
    k, trace = ek.grid_search(lambda K: -abs(K - 700), 2, 1000, points=3)
    assert k == 700
    for ks, _, _ in trace:
        assert ks == sorted(set(ks)) and 2 <= ks[0] and ks[-1] <= 1000
    with pytest.raises(ValueError):
        ek.grid_search(lambda K: 0.0, 5, 5)
    with pytest.raises(ValueError):
        ek.grid_search(lambda K: 0.0, 6, 5)
    with pytest.raises(ValueError):
        ek.grid_search(lambda K: 0.0, 2, 64, points=2)


# ------------------------------------------------------------------------------------------------ oracle restatement, sensitivity
def test_restatement_equals_golden(gold, cases, dists):
    assert set(cases) == {"ragged", "long_segment", "pad_d", "odd_d", "many_tiny", "blobs_true", "blobs_fit", "duplicates", "shuffled"}
    for name, (x, labels, k) in cases.items():
        assert x.dtype == np.float16
        got = sc.silhouette_f64(x, labels, k, dist=dists[name])
        assert np.abs(got - gold["s_" + name]).max() <= 1e-12, name


def test_cases_hold_what_they_are_for(cases):
    sizes = {name: np.bincount(labels, minlength=k) for name, (x, labels, k) in cases.items()}
    assert sorted(sizes["ragged"]) == [0, 1, 2, 3, 5, 246] and sorted(sizes["shuffled"]) == [0, 1, 2, 3, 5, 246]
    assert sizes["long_segment"].max() >= 700
    assert cases["pad_d"][0].shape[1] % 32 != 0 and cases["odd_d"][0].shape[1] % 64 == 32
    assert sizes["many_tiny"].size > 128 and (sizes["many_tiny"] == 1).any()
    x, labels, _ = cases["duplicates"]
    same = (x[:, None, :] == x[None, :, :]).all(2) & ~np.eye(x.shape[0], dtype=bool)
    i, j = np.nonzero(same)
    assert (labels[i] == labels[j]).sum() == 12 and (labels[i] != labels[j]).sum() == 2


@pytest.mark.parametrize("mistake", ["cnt", "singleton_one", "empty_id", "sorted_order", "centroid"])
def test_bounds_catch_planted_mistakes(gold, cases, dists, mistake):
    """Each planted mistake moves some sample of some case by more than the GPU test allows there."""
    caught = []
    for name, (x, labels, k) in cases.items():
        if name == "duplicates":
            _, a, b = sc.silhouette_f64(x, labels, k, dist=dists[name], return_ab=True)
            lim = 3.0 * np.sqrt(4.0 * 64 * 2.0 ** -24) / np.maximum(a, b)
        else:
            lim = sc.bound(name)
        wrong = sc.silhouette_f64(x, labels, k, mistake=mistake, dist=dists[name])
        if np.any(np.abs(wrong - gold["s_" + name]) > lim):
            caught.append(name)
    print(mistake, "caught on", caught)
    assert caught, mistake


def test_measured_bounds_are_fp32_sized():
    """4 x the measured error stays at a few fp32 ulps of a value in [-1, 1]: far below anything a wrong formula produces."""
    assert set(sc.MEASURED) == {"ragged", "long_segment", "pad_d", "odd_d", "many_tiny", "blobs_true", "blobs_fit", "shuffled"}
    assert all(0 < sc.bound(n) < 1e-6 for n in sc.MEASURED)


# ------------------------------------------------------------------------------------------------ driver parser, ABI
def test_driver_parser_defaults():
    sys.path.insert(0, ROOT)
    import estimate_k as driver
    base = ["--root_dir", "r", "--dataset_name", "d"]
    a = driver.parse_args(base)
    assert (a.criterion, a.search_mode, a.min_classes, a.max_classes) == ("acc", "brent", None, 1000)
    a = driver.parse_args(base + ["--criterion", "acc"])
    assert a.search_mode == "brent" and a.min_classes is None
    a = driver.parse_args(base + ["--criterion", "silhouette"])
    assert (a.search_mode, a.min_classes) == ("grid", 2)
    a = driver.parse_args(base + ["--criterion", "silhouette", "--search_mode", "brent", "--min_classes", "5"])
    assert (a.search_mode, a.min_classes) == ("brent", 5)
    a = driver.parse_args(base + ["--search_mode", "grid"])
    assert (a.criterion, a.search_mode) == ("acc", "grid")
    assert driver.parse_args(base + ["--criterion", "silhouette", "--search_mode", "binary"]).search_mode == "binary"
    with pytest.raises(SystemExit):
        driver.parse_args(base + ["--criterion", "gap"])


def test_abi_declares_silhouette():
    from scd_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scd_hip.h")).read(), flags=re.S)
    for name in ("scd_silhouette_ws_bytes", "scd_silhouette"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    lib = _lib.load()
    assert lib.scd_silhouette_ws_bytes(126976, 768, 1000) > 126976 * 768 * 2
    assert lib.scd_silhouette_ws_bytes(126976, 768, 1000) < 260 * 2 ** 20          # the sorted fp16 copy is nearly all of it
    for n, d, k in ((1, 64, 2), (100, 0, 2), (100, 1025, 2), (100, 64, 1), (100, 64, 101)):
        assert lib.scd_silhouette_ws_bytes(n, d, k) == 0, (n, d, k)
    assert lib.scd_silhouette_ws_bytes(100, 1024, 100) > 0
