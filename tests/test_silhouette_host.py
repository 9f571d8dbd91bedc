"""CPU checks around the silhouette: the integer grid search, the float64 restatement against the scikit-learn golden, the sensitivity of
the GPU test's bounds to planted mistakes, the exact lattice and grid families of tests/test_gpu_silhouette_exact.py (their count-table
reference against brute force, their exactness conditions at the MI355X sizes, seven planted kernel mistakes), the driver's parser and
the ABI surface.  No GPU, no scikit-learn."""
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


# ------------------------------------------------------------------------------------------------ the exact families (silhouette_cases)
def mi355x_ranges(n, k):
    return sc.ranges(n, k, 256)


@pytest.fixture(scope="module")
def lattice():
    """Every lattice case at the MI355X sizes (256 CUs); lattice_case asserts the exactness conditions while it builds."""
    return {name: sc.lattice_case(name, mi355x_ranges) for name in sc.LATTICE_NAMES}


@pytest.fixture(scope="module")
def grid():
    """name -> (case, float64 distances of the sorted rows plus a zero row, float64 reference, bound)."""
    out = {}
    for name in sc.GRID_SHAPES:
        case = sc.grid_case(name)
        order, _ = sc.sorted_slots(case["labels"], case["k"])
        dist = sc.grid_distances(np.concatenate([case["x"][order].astype(np.float64), np.zeros((1, case["d"]))]))
        want = sc.silhouette_f64(case["x"], case["labels"], case["k"], dist=sc.grid_distances(case["x"]))
        out[name] = (case, dist, want, sc.grid_bound(case["labels"], case["k"]))
    return out


def test_lattice_cases_hold_what_they_are_for(lattice):
    def sizes(c):
        return np.bincount(c["labels"][(c["labels"] >= 0) & (c["labels"] < c["k"])], minlength=c["k"])

    def entries(c):
        return c["k"] * -(-c["n"] // 1024)

    assert set(lattice) == set(sc.LATTICE_NAMES)
    assert [entries(lattice[n]) for n in ("scan_piece2", "scan_piece3")] == [1200, 2800]       # pieces of 2 and 3 entries per thread
    for name in ("scan_piece2", "scan_piece3", "one_range_k1000"):
        s = sizes(lattice[name])
        assert (s == 0).any() and (s == 1).any() and np.any(np.diff(lattice[name]["labels"]) < 0)
    assert entries(lattice["one_range_k1000"]) >= 124000
    two = [n for n in sc.LATTICE_NAMES if n.startswith("two_ranges")]
    assert all(lattice[n]["n"] == 511 * 128 + 1 + 37 and lattice[n]["d"] == 64 and lattice[n]["ny"] == 2 for n in two)
    assert all(lattice[n]["n"] == 1023 * 128 + 1 + 37 and lattice[n]["d"] == 32 and lattice[n]["ny"] == 1
               for n in ("one_range_k2", "one_range_k1000"))
    assert sizes(lattice["one_range_k2"]).min() > 65000 and sizes(lattice["two_ranges_tiny_first"])[0] == 5
    s = sizes(lattice["two_ranges_99_1"])
    assert s[1] * 99 <= s[0] <= s[1] * 100
    for tag, delta in (("m1", -1), ("0", 0), ("p1", 1)):
        c = lattice["two_ranges_border_" + tag]
        assert sizes(c)[0] == -(-c["n"] // 2) + delta and c["k"] == 3
    c = lattice["two_ranges_bad_rows"]
    assert sizes(c).sum() == c["n"] - 300 and set(np.unique(c["labels"])) == {-1, 0, 1, 2}
    assert sorted(sizes(lattice["ranges32"]))[-2:] == [1, 259] and lattice["ranges32"]["n"] == 515
    for v in sc.N_VALID:
        c = lattice["valid_%d" % v]
        assert c["n"] == 1000 and sizes(c).sum() == v and (sizes(c) == 0).any() and (sizes(c) == 1).any()
    assert [lattice["d_%d" % d]["d"] for d in sc.D_SWEEP] == list(sc.D_SWEEP)
    assert lattice["d_65_fp32"]["x"].dtype == np.float32 and all(c["x"].dtype == np.float16 for n, c in lattice.items() if n != "d_65_fp32")
    assert (lattice["d_32"]["g"], lattice["d_1000"]["g"], lattice["d_1024"]["g"], lattice["d_1"]["g"]) == (7, 32, 32, 1)


@pytest.mark.parametrize("name", ["ranges32", "d_1", "d_33", "d_64", "d_1000"])
def test_count_table_reference_equals_brute_force(lattice, name):
    """At n <= 600 the count-table sums finished in float64 are the brute-force float64 silhouette of the same rows, and the float32
    finish is within one rounding per step of it: a's and b's division (u each, 2 u on their quotient), b - a and the last division."""
    c = lattice[name]
    assert c["n"] <= 600
    brute = sc.silhouette_f64(c["x"], c["labels"], c["k"])
    s64, m64 = sc.lattice_reference(c, dtype=np.float64)
    assert s64.dtype == np.float64 and np.abs(s64 - brute).max() <= 1e-13
    s32, m32 = sc.lattice_reference(c)
    assert s32.dtype == np.float32 and np.abs(s32.astype(np.float64) - s64).max() <= 4 * sc.U24 * (1 + 1e-3)
    assert abs(m32 - m64) <= 4 * sc.U24


def test_reference_does_not_depend_on_the_split(lattice, grid):
    for name in ("two_ranges_border_0", "ranges32", "scan_piece3", "valid_129"):
        one = sc.lattice_reference(lattice[name], ny=1)[0]
        for ny in (2, 3, 32):
            assert np.array_equal(one, sc.lattice_reference(lattice[name], ny=ny)[0])
    for name, (case, dist, want, lim) in grid.items():
        assert np.abs(sc.grid_model(case, 32, dist=dist) - want).max() <= 1e-12, name     # the slot model is the float64 reference


# mistake -> (lattice cases it must change, lattice cases it must leave alone, general grid cases it must push past the derived bound)
PLANTED = {
    "border_both": (["two_ranges_border_0"], ["two_ranges_border_m1", "two_ranges_border_p1", "two_ranges_99_1"], ["grid_37"]),
    "border_neither": (["two_ranges_border_0"], ["two_ranges_border_m1", "two_ranges_border_p1", "two_ranges_99_1"], ["grid_37"]),
    "drop_partial_subtile": (["one_range_k1000", "one_range_k2", "d_33"], [], sorted(sc.GRID_SHAPES)),
    "unmasked_tail": (["one_range_k1000", "two_ranges_99_1", "d_64"], [], sorted(sc.GRID_SHAPES)),
    "pad_slots_in_last": (["valid_127", "valid_129", "valid_400"], ["valid_128"], sorted(sc.GRID_SHAPES)),
    # with one entry per thread this makes every offset 0, which any case notices; named here are the scans with longer pieces
    "scan_restart": (["scan_piece2", "scan_piece3", "one_range_k1000"], [], sorted(sc.GRID_SHAPES)),
    "skip_second_kstep": (["d_64", "d_1000", "d_1024", "two_ranges_99_1"], ["d_32", "d_96", "d_65"],
                          ["grid_130", "grid_32_tiles", "grid_big_of_3"]),
}


@pytest.mark.parametrize("mistake", sc.MISTAKES)
def test_exact_cases_catch_planted_kernel_mistakes(lattice, grid, mistake):
    """Each mistake, planted on the count tables, changes the answer of the lattice cases named for it (array_equal fails), leaves the
    cases alone that do not reach the path, and moves a sample of the named general grid cases beyond the derived bound."""
    moved, kept, grid_names = PLANTED[mistake]
    for name in moved + kept:
        c = lattice[name]
        ny = c["ny"] or mi355x_ranges(c["n"], c["k"])
        right, wrong = sc.lattice_reference(c, ny=ny)[0], sc.lattice_reference(c, ny=ny, mistake=mistake)[0]
        differ = int((right != wrong).sum()) + int((np.isnan(wrong)).sum())
        print(mistake, name, "rows that differ:", differ)
        assert (differ > 0) == (name in moved), (mistake, name, differ)
    for name in grid_names:
        case, dist, want, lim = grid[name]
        wrong = sc.grid_model(case, mi355x_ranges(case["n"], case["k"]), mistake=mistake, dist=dist)
        err = np.abs(wrong - want)
        print(mistake, name, "largest change / bound: %.3g" % np.nanmax(err / lim))
        assert np.any(~(err <= lim)), (mistake, name)
    assert set(PLANTED) == set(sc.MISTAKES)


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


def test_abi_declares_silhouette_ranges():
    """The query for the range count sits beside the kernel's other entry points; without a handle it answers 0 and touches no device."""
    from scd_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scd_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+scd_silhouette_ranges\s*\(\s*scd_handle\s+h\s*,\s*int64_t\s+n\s*,\s*int\s+k\s*\)", hdr)
    assert len(_lib.SIGNATURES["scd_silhouette_ranges"][1]) == 3
    assert _lib.load().scd_silhouette_ranges(None, 126976, 1000) == 0
    from scd_amd import ops
    assert callable(ops.silhouette_ranges)
