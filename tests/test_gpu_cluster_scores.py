"""GPU checks of the clustering scores (scd_contingency, scd_contingency_stats, scd_amd.metrics) and of the number-of-categories
estimator on top of them (scd_amd.estimate_k, estimate_k.py).

The tables are integers: they must equal a numpy restatement (`np.add.at`) exactly, on both kernel paths.  The three doubles of the
statistics are sums of at most 10^6 float64 terms that add up to at most ln N < 13, each rounding at most 2^-53 relative: a reordered
sum differs by less than 1.5e-9, at the 200 x 200 shape used here by 6e-11; the tests assert 1e-9.  The scores are checked against
tests/golden/cluster_scores.npz (the reference's cluster_acc, scikit-learn 1.7.2)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cluster_score_cases import cases
from oracle import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from scd_amd import ops as o
    return o


@pytest.fixture(scope="module")
def metrics():
    from scd_amd import metrics as m
    return m


@pytest.fixture(scope="module")
def gold(golden):
    return golden("cluster_scores.npz")


def np_tables(pred, truth, subset, kp, kt):
    """The numpy restatement: (tables int64 [S, kp, kt], n_bad)."""
    pred, truth = np.asarray(pred, dtype=np.int64), np.asarray(truth, dtype=np.int64)
    s = 1 if subset is None else 2
    t = np.zeros((s, kp, kt), dtype=np.int64)
    ok = (pred >= 0) & (pred < kp) & (truth >= 0) & (truth < kt)
    tab = np.zeros(pred.size, dtype=np.int64) if subset is None else np.where(np.asarray(subset) != 0, 0, 1)
    np.add.at(t, (tab[ok], pred[ok], truth[ok]), 1)
    return t, int((~ok).sum())


def dev32(x):
    return torch.as_tensor(np.asarray(x, dtype=np.int32)).cuda()


def run(ops, pred, truth, subset, kp, kt):
    sub = None if subset is None else torch.as_tensor(np.asarray(subset, dtype=np.uint8)).cuda()
    table, n_bad = ops.contingency(dev32(pred), dev32(truth), sub, kp, kt)
    return table.cpu().numpy().astype(np.int64), int(n_bad.item())


def labels(r, n, kp, kt):
    """Random labels that sit on 0 and on K - 1 at the ends of the array."""
    pred, truth = r.randint(0, kp, n), r.randint(0, kt, n)
    pred[0], truth[0] = 0, kt - 1
    pred[-1], truth[-1] = kp - 1, 0
    if n > 2:
        pred[n // 2], truth[n // 2] = kp - 1, kt - 1
    return pred, truth


def subsets(r, n):
    return {"none": None, "ones": np.ones(n, dtype=np.uint8), "zeros": np.zeros(n, dtype=np.uint8),
            "random": (r.rand(n) < 0.4).astype(np.uint8) * r.randint(1, 256, n).astype(np.uint8)}    # any non-zero byte means "inside"


@pytest.mark.parametrize("kp,kt", [(1, 1), (3, 7), (7, 3), (200, 200)])
def test_contingency_matches_numpy(ops, kp, kt):
    r = np.random.RandomState(kp * 1000 + kt)
    for n in (1, 63, 64, 65, 4097):
        pred, truth = labels(r, n, kp, kt)
        for name, sub in subsets(r, n).items():
            got, bad = run(ops, pred, truth, sub, kp, kt)
            want, _ = np_tables(pred, truth, sub, kp, kt)
            assert bad == 0
            assert np.array_equal(got, want), (n, name)
            if name == "ones":
                assert not got[1].any()
            if name == "zeros":
                assert not got[0].any()
            cells = (1 if sub is None else 2) * kp * kt
            assert ops.contingency_last_path() == (0 if cells <= ops.contingency_private_cells() else 1)


def test_contingency_both_sides_of_the_private_limit(ops):
    """A table of exactly contingency_private_cells() cells is counted in LDS, one cell more goes to the global path."""
    lim = ops.contingency_private_cells()
    assert lim >= 8 * 8 * 2 and lim % 256 == 0
    r = np.random.RandomState(1)
    n = 20011
    seen = set()
    for kp, kt, with_sub in ((lim // 256, 256, False), (1, lim + 1, False), (lim // 512, 256, True), (lim // 2 + 1, 1, True)):
        pred, truth = labels(r, n, kp, kt)
        sub = (r.rand(n) < 0.5).astype(np.uint8) if with_sub else None
        got, bad = run(ops, pred, truth, sub, kp, kt)
        want, _ = np_tables(pred, truth, sub, kp, kt)
        assert bad == 0 and np.array_equal(got, want), (kp, kt)
        cells = (2 if with_sub else 1) * kp * kt
        assert ops.contingency_last_path() == (0 if cells <= lim else 1), (kp, kt)
        seen.add(ops.contingency_last_path())
    assert seen == {0, 1}


@pytest.mark.parametrize("kp,kt", [(5, 6), (300, 300)])
def test_contingency_unaligned_arrays(ops, kp, kt):
    """Views that start 4 bytes (labels) or 1 byte (subset) into an allocation take the one-row-at-a-time loads."""
    r = np.random.RandomState(7)
    n = 5000
    pred, truth = labels(r, n, kp, kt)
    sub = (r.rand(n) < 0.5).astype(np.uint8)
    want, _ = np_tables(pred, truth, sub, kp, kt)
    p = torch.cat([torch.zeros(1, dtype=torch.int32), torch.as_tensor(pred.astype(np.int32))]).cuda()[1:]
    t = torch.cat([torch.zeros(1, dtype=torch.int32), torch.as_tensor(truth.astype(np.int32))]).cuda()[1:]
    s = torch.cat([torch.zeros(1, dtype=torch.uint8), torch.as_tensor(sub)]).cuda()[1:]
    assert p.data_ptr() % 16 and s.data_ptr() % 16
    table, n_bad = ops.contingency(p, t, s, kp, kt)
    assert int(n_bad.item()) == 0 and np.array_equal(table.cpu().numpy(), want)
    table, _ = ops.contingency(p, t, None, kp, kt)
    assert np.array_equal(table.cpu().numpy()[0], want.sum(0))


@pytest.mark.parametrize("kp,kt", [(4, 9), (250, 170)])
def test_contingency_out_of_range_labels(ops, metrics, kp, kt):
    r = np.random.RandomState(11)
    n = 1000
    pred, truth = labels(r, n, kp, kt)
    sub = (r.rand(n) < 0.5).astype(np.uint8)
    pred[17], pred[500], truth[998] = -1, kp, kt
    truth[3] = -5
    for s in (None, sub):
        got, bad = run(ops, pred, truth, s, kp, kt)
        want, nbad = np_tables(pred, truth, s, kp, kt)
        assert bad == nbad == 4
        assert np.array_equal(got, want) and got.sum() == n - 4
        with pytest.raises(ValueError):
            metrics.contingency(pred, truth, subset=s, kp=kp, kt=kt)


@pytest.mark.parametrize("kp,kt,path", [(8, 8, 0), (1100, 1000, 1)])
def test_contingency_maximum_contention(ops, kp, kt, path):
    """70,001 rows in one cell: a 16-bit cell, or a per-block count that is lost, cannot reach it."""
    n = 70001
    pred, truth = np.full(n, 3), np.full(n, 5)
    got, bad = run(ops, pred, truth, None, kp, kt)
    assert ops.contingency_last_path() == path
    assert bad == 0 and got[0, 3, 5] == n and got.sum() == n


def test_contingency_int64_labels_through_wrapper(metrics):
    r = np.random.RandomState(5)
    pred, truth = r.randint(0, 12, 3001), r.randint(0, 9, 3001)
    mask = r.rand(3001) < 0.3
    a = metrics.contingency(torch.as_tensor(pred, dtype=torch.int64).cuda(), torch.as_tensor(truth, dtype=torch.int64).cuda(),
                            subset=torch.as_tensor(mask).cuda())
    b = metrics.contingency(dev32(pred), dev32(truth), subset=mask)
    assert a.dtype == torch.int32 and a.is_cuda and tuple(a.shape) == (2, 12, 9)
    assert torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), np_tables(pred, truth, mask, 12, 9)[0])
    single = metrics.contingency(pred, truth)                          # numpy in, one table out
    assert tuple(single.shape) == (12, 9) and np.array_equal(single.cpu().numpy(), np_tables(pred, truth, None, 12, 9)[0][0])


# ------------------------------------------------------------------------------------------------ statistics
def np_stats(w):
    """(ints, info) of one table in numpy float64, term by term as sklearn's entropy / mutual_info_score."""
    w = np.asarray(w, dtype=np.int64)
    a, b, n = w.sum(1), w.sum(0), w.sum()
    ints = [n, (w ** 2).sum(), (a ** 2).sum(), (b ** 2).sum(), w.max(1).sum() if w.size else 0, (w > 0).sum()]
    if n == 0:
        return ints, [0.0, 0.0, 0.0]

    def ent(m):
        m = m[m > 0].astype(np.float64)
        return -np.sum((m / n) * (np.log(m) - np.log(n)))

    i, j = np.nonzero(w)
    v = w[i, j].astype(np.float64)
    outer = (a[i] * b[j]).astype(np.float64)
    mi = (v / n) * (np.log(v) - np.log(n)) + (v / n) * (-np.log(outer) + np.log(n) + np.log(n))
    mi = np.where(np.abs(mi) < np.finfo(np.float64).eps, 0.0, mi)
    return ints, [ent(a), ent(b), mi.sum()]


@pytest.mark.parametrize("kp,kt", [(1, 1), (3, 7), (7, 3), (200, 200), (1100, 1000)])
def test_contingency_stats_match_numpy(ops, kp, kt):
    r = np.random.RandomState(kp + kt)
    n = 4097
    truth = r.randint(0, kt, n)
    pred = np.where(r.rand(n) < 0.6, truth % kp, r.randint(0, kp, n))          # correlated: a mutual information well above 0
    sub = (r.rand(n) < 0.4).astype(np.uint8)
    for s in (None, sub, np.zeros(n, dtype=np.uint8)):                       # the last: table 0 is empty
        sd = None if s is None else torch.as_tensor(s).cuda()
        table, _ = ops.contingency(dev32(pred), dev32(truth), sd, kp, kt)
        ints, info = ops.contingency_stats(table)
        ints2, info2 = ops.contingency_stats(table)
        assert info.cpu().numpy().tobytes() == info2.cpu().numpy().tobytes()   # bit-identical from call to call
        assert torch.equal(ints, ints2)
        w = table.cpu().numpy()
        for q in range(w.shape[0]):
            want_i, want_f = np_stats(w[q])
            assert [int(x) for x in ints[q].cpu()] == [int(x) for x in want_i], (kp, kt, q)
            got_f = info[q].cpu().numpy()
            print("stats %dx%d table %d: |err| H(pred) %.3e H(truth) %.3e MI %.3e" % ((kp, kt, q) + tuple(abs(got_f - want_f))))
            assert np.all(np.abs(got_f - np.asarray(want_f)) <= 1e-9), (kp, kt, q, got_f, want_f)


# ------------------------------------------------------------------------------------------------ scores
def test_golden_scores(metrics, gold):
    for c, case in enumerate(cases(gold)):
        pred, truth, want = case["pred"], case["truth"], case["scores"]
        d = case["table"].shape[0]
        assert np.array_equal(metrics.contingency(pred, truth, kp=d, kt=d).cpu().numpy(), case["table"]), c
        assert metrics.cluster_acc(truth, pred) == want[0], c
        assert metrics.ari_score(truth, pred) == want[2], c
        assert metrics.purity_score(truth, pred) == want[3], c
        assert abs(metrics.nmi_score(truth, pred) - want[1]) <= 1e-9, c


def test_score_split_equals_single_subset_calls(metrics, gold):
    for c, case in enumerate(cases(gold)):
        pred, truth, mask = case["pred"], case["truth"], case["mask"]
        got = metrics.score_split(torch.as_tensor(pred).cuda(), truth, mask)
        for name, m in (("labelled", mask), ("unlabelled", ~mask)):
            if not m.any():
                assert got[name] is None
                continue
            p, t = pred[m], truth[m]
            want = dict(acc=metrics.cluster_acc(t, p), nmi=metrics.nmi_score(t, p), ari=metrics.ari_score(t, p),
                        purity=metrics.purity_score(t, p))
            assert got[name]["acc"] == want["acc"], (c, name)
            assert got[name]["ari"] == want["ari"], (c, name)
            assert got[name]["purity"] == want["purity"], (c, name)
            assert abs(got[name]["nmi"] - want["nmi"]) <= 1e-9, (c, name)


# ------------------------------------------------------------------------------------------------ the estimator, end to end
def blobs(n):
    """SURVEY.md 8d blobs: D = 64, 20 true classes, noise 0.6 / sqrt(D); classes < 10 labelled at 50 %, labelled rows first."""
    x, y, _ = synth.clustered_features(n, 64, 20, noise=0.6)
    perm, mask_lab = synth.labelled_split(y, 20, prop=0.5)
    return x[perm], y[perm], mask_lab


@pytest.mark.parametrize("mode", ["binary", "brent"])
def test_estimator_end_to_end(ops, mode):
    """Scoring on the device (score_split on labels_device_) and on the host (cluster_acc on labels_[mask_lab]) must drive the
    search through the same Ks with the same accuracies to the same K, and that K lies in [16, 24] (20 true classes; scikit-learn
    1.7.2 KMeans(random_state=0) + the reference's cluster_acc give 23 (binary) and 21 (Brent) on this input,
    docs/design/estimate_k.md)."""
    from scd_amd import estimate_k as ek
    from scd_amd.cluster import KMeans
    from scd_amd.gcd.project_utils.cluster_utils import cluster_acc
    x, y, mask_lab = blobs(3000)
    feats = ops.l2norm_rows(torch.as_tensor(x).cuda())
    targets, mask = torch.as_tensor(y).cuda(), torch.as_tensor(mask_lab).cuda()

    def on_device(K):
        return ek.evaluate_k(K, feats, targets, mask)[0]

    def on_host(K):
        labels = KMeans(n_clusters=int(K), random_state=0).fit(feats).labels_
        return cluster_acc(y.astype(int)[mask_lab], labels.astype(int)[mask_lab])

    search = (lambda ev: ek.binary_search(ev, 10, 64)) if mode == "binary" else (lambda ev: ek.brent(ev, 10, 64))
    dev_run, host_run = search(on_device), search(on_host)
    print(mode, dev_run)
    assert dev_run == host_run                      # Ks visited, accuracies as floats, the final K
    k = dev_run[0] if mode == "binary" else dev_run[1]
    assert 16 <= k <= 24, k


def test_estimate_k_driver(tmp_path):
    x, y, mask_lab = blobs(1200)
    fdir = tmp_path / "extracted_features"
    fdir.mkdir()
    torch.save(dict(all_feats=x, mask_lab=mask_lab, mask_cls=y < 10, targets=y.astype(np.float64)), str(fdir / "synth_blobs_all.pt"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "estimate_k.py"), "--root_dir", str(tmp_path), "--dataset_name", "blobs",
                        "--feat_model", "synth", "--max_classes", "64", "--search_mode", "binary"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.load(open(str(tmp_path / "cluster" / "estimated_k_synth_blobs.json")))
    assert out["search_mode"] == "binary" and out["min_classes"] == 10 and out["max_classes"] == 64
    assert 10 <= out["k"] <= 64
    assert len(out["trace"]) == int(np.log2(64 - 10)) + 1 and all(len(t["accs"]) == 3 for t in out["trace"])
    assert "--n_cluster %d" % out["k"] in r.stdout and "Iter 0: BigK 64" in r.stdout
