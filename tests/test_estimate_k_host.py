"""CPU checks of the number-of-categories estimator: the two searches of scd_amd.estimate_k against the reference's own runs on a
fixed accuracy curve, and the NMI / ARI / purity rules of scd_amd.metrics on the statistics of golden tables
(tests/golden/cluster_scores.npz, written by tools/gen_cluster_scores_golden.py from the reference's `binary_search` and
`cluster_acc`, scikit-learn 1.7.2 and scipy's bounded Brent).  No device is used."""
import numpy as np
import pytest

from cluster_score_cases import cases
from scd_amd import estimate_k as ek
from scd_amd import metrics


@pytest.fixture(scope="module")
def gold(golden):
    return golden("cluster_scores.npz")


class Curve:
    """evaluate(K) of the golden curve, with the calls recorded."""

    def __init__(self, gold):
        self.acc = gold["curve"]
        self.calls = []

    def __call__(self, K):
        assert isinstance(K, int)
        self.calls.append(K)
        return float(self.acc[K])


def test_binary_search_reproduces_reference_trace(gold):
    ev = Curve(gold)
    small, big = (int(v) for v in gold["bs_range"])
    best, trace = ek.binary_search(ev, small, big)
    assert [t[:3] for t in trace] == [tuple(int(v) for v in row) for row in gold["bs_trace"]]
    for s, m, b, accs in trace:
        assert accs == (gold["curve"][s], gold["curve"][m], gold["curve"][b])
    assert best == int(gold["bs_best"][-1])
    # the reference evaluates big, small, middle and then every new middle: the first visit of every K comes in its order
    ref_calls = [int(k) for k in gold["bs_calls"]]
    assert ev.calls == list(dict.fromkeys(ref_calls))
    assert len(ev.calls) == len(set(ref_calls))             # memoised: one evaluation per distinct K


def test_binary_search_best_looks_at_current_triple_only(gold):
    """The per-iteration 'best so far' of the reference is the best of the CURRENT triple (estimate_k.py:215-217)."""
    small, big = (int(v) for v in gold["bs_range"])
    seen = []
    ek.binary_search(Curve(gold), small, big, log=seen.append)
    best = [int(s.rsplit(" ", 1)[1]) for s in seen if s.startswith("Best Acc so far")]
    assert best == [int(v) for v in gold["bs_best"]]
    assert sum(s.startswith("Iter ") for s in seen) == len(gold["bs_best"])


def test_binary_search_rejects_empty_range(gold):
    with pytest.raises(ValueError):
        ek.binary_search(Curve(gold), 20, 20)


def test_brent_reproduces_scipy_sequence(gold):
    ev = Curve(gold)
    small, big = (int(v) for v in gold["bs_range"])
    x, k, trace = ek.brent(ev, small, big)
    assert [t[1] for t in trace] == [int(v) for v in gold["brent_ks"]]
    assert np.float64(x).tobytes() == gold["brent_x"][0].tobytes()          # bit for bit
    assert k == int(gold["brent_x"][0])
    assert ev.calls == list(dict.fromkeys(int(v) for v in gold["brent_ks"]))
    assert len(ev.calls) == len(set(int(v) for v in gold["brent_ks"]))


def test_score_rules_on_golden_statistics(gold):
    for c, case in enumerate(cases(gold)):
        ints, info, want = case["ints"], case["info"], case["scores"]
        assert metrics.ari_from_stats(ints) == want[2], c
        assert metrics.purity_from_stats(ints) == want[3], c
        assert abs(metrics.nmi_from_stats(ints, info) - want[1]) <= 1e-12, c


def test_golden_statistics_belong_to_golden_tables(gold):
    """The fixture's integers are those of its tables, and its tables those of its labels (a numpy restatement)."""
    for case in cases(gold):
        pred, truth, w = case["pred"], case["truth"], case["table"]
        t = np.zeros_like(w)
        np.add.at(t, (pred, truth), 1)
        assert np.array_equal(t, w)
        a, b = w.sum(1), w.sum(0)
        assert list(case["ints"]) == [w.sum(), (w ** 2).sum(), (a ** 2).sum(), (b ** 2).sum(), w.max(1).sum(), (w > 0).sum()]


def test_nmi_special_cases():
    # one class on both sides: a single non-zero cell, zero entropies
    assert metrics.nmi_from_stats([50, 2500, 2500, 2500, 50, 1], [0.0, 0.0, 0.0]) == 1.0
    # no rows at all
    assert metrics.nmi_from_stats([0, 0, 0, 0, 0, 0], [0.0, 0.0, 0.0]) == 1.0
    # MI = 0 (one cluster against two classes), also when rounding left it a hair below zero
    assert metrics.nmi_from_stats([4, 8, 16, 8, 2, 2], [0.0, np.log(2.0), 0.0]) == 0.0
    assert metrics.nmi_from_stats([4, 8, 16, 8, 2, 2], [0.0, np.log(2.0), -1e-17]) == 0.0


def test_ari_special_cases_and_large_n():
    assert metrics.ari_from_stats([1, 1, 1, 1, 1, 1]) == 1.0               # one row
    assert metrics.ari_from_stats([50, 2500, 2500, 2500, 50, 1]) == 1.0    # one class on both sides
    # n = 2^31 - 4 rows, two equal clusters independent of two equal classes: the products pass 2^63, Python ints hold them
    n = 2 ** 31 - 4
    q = n // 4
    ints = [n, 4 * q * q, 2 * (2 * q) ** 2, 2 * (2 * q) ** 2, 2 * q, 4]
    assert abs(metrics.ari_from_stats(ints)) < 1e-9
