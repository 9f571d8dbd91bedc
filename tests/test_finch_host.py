"""CPU checks of the FINCH restatement (tests/finch_cases.py) against the reference's recorded results (tests/golden/finch.npz,
tools/gen_finch_golden.py), of the sparse edge rule against the reference's dense A, of the planted mistakes, and of
scd_amd.estimate_k.finch_search.  docs/design/finch.md has the rules."""
import numpy as np
import pytest

import finch_cases as fc


@pytest.fixture(scope="module")
def gold(golden):
    return golden("finch.npz")


@pytest.fixture(scope="module")
def inputs():
    return {name: fc.case_input(name) for name in fc.CASES}


@pytest.mark.parametrize("name", list(fc.CASES))
def test_restatement_reproduces_the_reference(gold, inputs, name):
    c, num, _ = fc.finch_f64(inputs[name])
    assert num == fc.NUM_CLUST[name] == gold["num_" + name].tolist()
    assert np.array_equal(c, gold["c_" + name])
    nb, th = gold["margins_" + name]
    assert nb >= fc.MIN_NEIGHBOUR_MARGIN and th >= fc.MIN_THRESHOLD_MARGIN
    for r in fc.CASES[name][6]:
        _, _, req = fc.finch_f64(inputs[name], req_clust=r)
        assert np.array_equal(req, gold["req_%s_%d" % (name, r)]) and len(np.unique(req)) == r


def test_req_clust_above_first_partition_raises(inputs):
    with pytest.raises(ValueError):
        fc.finch_f64(inputs["b600"], req_clust=97)


def planted_exception():
    """Rule 3's exception: rows 0 and 1 are a mutual pair at distance d, row 2 is a sibling of 0 (nn[2] = 1) with d(0, 2) within
    min_sim, and d <= min_sim < 2 d cuts the pair.  Returns (u, min_sim)."""
    phi, t = np.deg2rad([0.0, 115.0, 236.0]), np.deg2rad(12.0)
    near = np.stack([np.sin(t) * np.cos(phi), np.sin(t) * np.sin(phi), np.cos(t) * np.ones(3)], 1)
    far = np.array([[0.0, 0.0, -1.0], [0.1, 0.0, -1.0]])
    u = fc.unit_rows(np.concatenate([near, far]).astype(np.float32))
    nn, d1 = fc.first_neighbor(u)
    assert nn[0] == 1 and nn[1] == 0 and nn[2] == 1
    d01, d02 = d1[0], fc.pair_dist(u, [0], [2])[0]
    min_sim = 0.5 * (d02 + 2 * d01)
    assert d01 <= d1[2] <= d02 <= min_sim < 2 * d01
    return u, min_sim


def test_sparse_edge_rule_equals_dense_a():
    r = np.random.RandomState(7)
    seen_exception = 0
    trials = [(fc.grid_rows(r, int(r.randint(2, 61)), int(r.randint(2, 6)), int(r.randint(1, 4))), None) for _ in range(200)]
    trials.append(planted_exception())
    for rows, min_sim in trials:
        u = fc.unit_rows(rows)
        nn, d1 = fc.first_neighbor(u)
        if min_sim is None:
            lo, hi = (2 * d1).min(), (2 * d1).max()
            min_sim = lo + (hi - lo) * r.rand()
        for ms in (None, min_sim):
            lab, k = fc.level_labels(u, nn, d1, ms)
            lab_d, k_d = fc.level_labels_dense(u, nn, ms)
            assert k == k_d and np.array_equal(lab, lab_d)
        ea, _ = fc.level_edges(u, nn, d1, min_sim)
        seen_exception += len(ea) > int((~(fc.mutual_weight(nn)[1] * d1 > min_sim)).sum())
    u, min_sim = planted_exception()
    nn, d1 = fc.first_neighbor(u)
    lab, _ = fc.level_labels(u, nn, d1, min_sim)
    assert lab[0] == lab[2] == lab[1]                           # 0 rejoins through its sibling 2, whose edge to 1 survives
    assert seen_exception >= 1


# which case catches which planted mistake (every blob case catches the first and the fifth; one is listed)
CAUGHT_BY = {"self": "b600", "tie_high": "ties", "mutual1": "b1500", "no_sibling": "s600", "root": "h1200", "prev_means": "b1500"}


@pytest.mark.parametrize("mistake", fc.MISTAKES)
def test_planted_mistake_changes_a_partition(gold, inputs, mistake):
    assert set(CAUGHT_BY) == set(fc.MISTAKES)
    name = CAUGHT_BY[mistake]
    if name == "ties":                                          # no blob case has an exact tie
        x = fc.tie_case()
        want = fc.finch_f64(x)[0]
    else:
        x, want = inputs[name], gold["c_" + name]
    c, _, _ = fc.finch_f64(x, mistake=mistake)
    assert c.shape != want.shape or not np.array_equal(c, want)


def test_finch_search():
    from scd_amd.estimate_k import finch_search
    calls = []

    def ev(table):
        def f(K):
            calls.append(K)
            return table[K]
        return f

    # clipping: 356 -> 64 and 1 -> 2; the first maximum
    k, trace = finch_search(ev({2: 0.1, 20: 0.5, 21: 0.4, 64: 0.2}), [356, 21, 20, 1], 2, 64)
    assert k == 20 and trace == [([2, 20, 21, 64], [0.1, 0.5, 0.4, 0.2], 20)] and calls == [2, 20, 21, 64]
    # a tie: the lowest K
    assert finch_search(ev({12: 0.3, 14: 0.3, 96: 0.1}), [96, 14, 12], 2, 100)[0] == 12
    # candidates that clip to one value are evaluated once
    del calls[:]
    assert finch_search(ev({50: 0.7}), [400, 90, 51], 2, 50)[0] == 50 and calls == [50]
    with pytest.raises(ValueError):
        finch_search(ev({}), [], 2, 64)
    with pytest.raises(ValueError):
        finch_search(ev({}), [5], 9, 3)


def test_finch_rejects_other_distances():
    from scd_amd.finch import Finch
    with pytest.raises(ValueError):
        Finch(distance="euclidean")
