"""GPU checks of scd_silhouette (scd_amd/csrc/silhouette.hip), scd_amd.metrics.silhouette_samples / silhouette_score and the
label-free search for the number of categories on top of them (scd_amd.estimate_k.grid_search, estimate_k.py --criterion silhouette).

Expected values: tests/golden/silhouette.npz, scikit-learn 1.7.2's silhouette_samples in float64 on the fp16-rounded rows
(tools/gen_silhouette_golden.py).  The device works in fp32 with a summation order fixed by the labels; the per-case bounds are
4 x the largest per-sample error measured on an MI355X (silhouette_cases.MEASURED; docs/design/estimate_k.md), and
tests/test_silhouette_host.py checks that every planted mistake still exceeds them.

The duplicates case has a derived bound instead.  Near dist = 0 the square root amplifies the fp32 cancellation in
dist^2 = |x_i|^2 + |x_j|^2 - 2 dot: for unit rows each of the three terms is a sum of dp products accumulated in fp32, off by at most
dp * 2^-24 (the dot counts twice), so dist^2 is off by at most 4 dp 2^-24 and, since |sqrt(u + t) - sqrt(u)| <= sqrt(|t|), each
distance by at most e = sqrt(4 dp 2^-24) (3.9e-3 at dp = 64).  The means a and b are then off by at most e each, and
s = (b - a) / max(a, b) moves by at most (e_a + e_b) / max + |b - a| e / max^2 <= 3 e / max(a64, b64) to first order."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import silhouette_cases as sc

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
    return golden("silhouette.npz")


@pytest.fixture(scope="module")
def cases(gold):
    return sc.cases(gold)


def run(ops, x, labels, k):
    s, mean, info = ops.silhouette(torch.as_tensor(x).cuda(), torch.as_tensor(np.asarray(labels, dtype=np.int32)).cuda(), k)
    return s.cpu().numpy(), float(mean.item()), [int(v) for v in info.cpu()]


CASE_NAMES = ["ragged", "long_segment", "pad_d", "odd_d", "many_tiny", "blobs_true", "blobs_fit", "duplicates", "shuffled"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_samples_match_golden(ops, gold, cases, name):
    x, labels, k = cases[name]
    want = gold["s_" + name]
    got, mean, info = run(ops, x, labels, k)
    assert info == [0, int((np.bincount(labels, minlength=k) > 0).sum())]
    err = np.abs(got.astype(np.float64) - want)
    if name == "duplicates":
        _, a, b = sc.silhouette_f64(x, labels, k, return_ab=True)
        dp = (x.shape[1] + 31) // 32 * 32
        lim = 3.0 * np.sqrt(4.0 * dp * 2.0 ** -24) / np.maximum(a, b)
    else:
        lim = np.full(err.shape, sc.bound(name))
    print("silhouette %-13s max |err| %.3e (bound %.3e)  |mean err| %.3e" % (name, err.max(), lim.min(), abs(mean - want.mean())))
    assert np.all(err <= lim), (name, err.max(), int(err.argmax()))
    assert abs(mean - want.mean()) <= lim.max(), (name, mean, want.mean())
    assert abs(mean - got.astype(np.float64).mean()) <= 1e-12


@pytest.mark.parametrize("name", ["ragged", "pad_d", "many_tiny"])
def test_fp32_input_equals_fp16_input(ops, cases, name):
    x, labels, k = cases[name]
    lab = torch.as_tensor(labels.astype(np.int32)).cuda()
    x16 = torch.as_tensor(x).cuda()
    s16, m16, _ = ops.silhouette(x16, lab, k)
    s32, m32, _ = ops.silhouette(x16.float(), lab, k)
    assert s16.cpu().numpy().tobytes() == s32.cpu().numpy().tobytes()
    assert m16.cpu().numpy().tobytes() == m32.cpu().numpy().tobytes()


@pytest.mark.parametrize("name", ["ragged", "many_tiny"])
def test_two_calls_are_bit_identical(ops, cases, name):
    x, labels, k = cases[name]
    lab = torch.as_tensor(labels.astype(np.int32)).cuda()
    xd = torch.as_tensor(x).cuda()
    s1, m1, i1 = ops.silhouette(xd, lab, k)
    s2, m2, i2 = ops.silhouette(xd, lab, k)
    assert s1.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes()
    assert m1.cpu().numpy().tobytes() == m2.cpu().numpy().tobytes()
    assert torch.equal(i1, i2)


def test_wrappers_follow_sklearn_surface(metrics, gold, cases):
    x, labels, k = cases["pad_d"]
    want = gold["s_pad_d"]
    s = metrics.silhouette_samples(x.astype(np.float32), labels)                # numpy in
    assert s.is_cuda and s.dtype == torch.float32 and tuple(s.shape) == (x.shape[0],)
    assert np.abs(s.cpu().numpy() - want).max() <= sc.bound("pad_d")
    score = metrics.silhouette_score(torch.as_tensor(x).cuda(), torch.as_tensor(labels).cuda())   # device fp16, int64 labels
    assert isinstance(score, float) and abs(score - want.mean()) <= sc.bound("pad_d")


def test_errors(ops, metrics, cases):
    x, labels, k = cases["pad_d"]
    n = x.shape[0]
    bad = labels.copy()
    bad[17] = -1
    with pytest.raises(ValueError):
        metrics.silhouette_samples(x, bad)
    bad = labels.copy()
    bad[17] = k
    with pytest.raises(ValueError):
        metrics.silhouette_samples(x, bad, k=k)
    with pytest.raises(ValueError):
        metrics.silhouette_score(x, np.zeros(n, dtype=np.int64))                 # one non-empty cluster
    with pytest.raises(ValueError):
        metrics.silhouette_score(x, np.full(n, 3))                               # ... under another id
    with pytest.raises(ValueError):
        metrics.silhouette_score(x, np.arange(n))                                # all singletons
    # the ABI call: bad rows are counted and take part in nothing; one non-empty cluster gives zeros
    bad = labels.copy()
    bad[[3, 40]] = [-1, k]
    keep = np.ones(n, dtype=bool)
    keep[[3, 40]] = False
    got, mean, info = run(ops, x, bad, k)
    want, _, _ = run(ops, x[keep], labels[keep], k)
    assert info == [2, k] and got[3] == 0 and got[40] == 0
    assert got[keep].tobytes() == want.tobytes()
    got, mean, info = run(ops, x, np.full(n, 1), 2)
    assert info == [0, 1] and not got.any() and mean == 0.0


# ------------------------------------------------------------------------------------------------ the estimator, end to end
def search_blobs(ops, metrics, gold, monkeypatch, **kmeans_kw):
    """grid_search on the blobs over [2, 64] -> (K, number of visited K whose partition is not scikit-learn's).  Every K whose device
    partition equals the golden one (ARI 1.0) must score within 0.02 of the golden table."""
    from scd_amd import estimate_k as ek
    x, y, _ = sc.blobs(3000)
    feats = ops.l2norm_rows(torch.as_tensor(x).cuda())
    parts = {int(K): gold["blobs_part"][i].astype(np.int64) for i, K in enumerate(gold["blobs_ks"])}
    table = {int(K): float(gold["blobs_sil"][i]) for i, K in enumerate(gold["blobs_ks"])}
    fits = {}
    orig = metrics.silhouette_score

    def spy(X, labels, k=None):
        fits[len(fits)] = labels
        return orig(X, labels, k)

    monkeypatch.setattr(metrics, "silhouette_score", spy)
    visited = []

    def evaluate(K):
        visited.append(int(K))
        return ek.evaluate_k_unlabelled(K, feats, **kmeans_kw)[0]

    k, trace = ek.grid_search(evaluate, 2, 64)
    print("grid search", kmeans_kw, "->", k, [(ks, ["%.4f" % s for s in scores], best) for ks, scores, best in trace])
    assert len(visited) == len(set(visited)) == len(fits)
    scores = {K: s for ks, sc_, _ in trace for K, s in zip(ks, sc_)}
    skipped = 0
    for i, K in enumerate(visited):
        same = K in parts and metrics.ari_score(parts[K], fits[i]) == 1.0
        print("K = %2d: silhouette %.4f, golden %s, same partition as scikit-learn: %s" % (K, scores[K], table.get(K), same))
        if not same:
            skipped += 1
            continue
        assert abs(scores[K] - table[K]) <= 0.02, (K, scores[K], table[K])
    return k, skipped


def test_estimator_end_to_end(ops, metrics, gold, monkeypatch):
    """grid_search over the device silhouette finds the blobs' 20 classes to within [18, 22] (scikit-learn 1.7.2 with ten starts:
    exactly 20; with one start 18 / 19), and every visited K whose device partition is scikit-learn's scores within 0.02 of the golden
    table, with at most 4 K skipped because the partition differs.  The golden partitions are scikit-learn 1.7.2's
    `KMeans(random_state=0, n_init=10)`, so the fits run in the mode that restates that version (sklearn_compat='1.7.2', ten starts)."""
    k, skipped = search_blobs(ops, metrics, gold, monkeypatch, sklearn_compat="1.7.2", n_init=10)
    assert 18 <= k <= 22, k
    assert skipped <= 4, skipped


def test_estimator_end_to_end_default_fit(ops, metrics, gold, monkeypatch):
    """The same search with KMeans' defaults (sklearn_compat='1.0.2': ten starts seeded as scikit-learn 1.0.2 seeds them).  Those
    partitions are another version's, so few equal the golden ones (measured on an MI355X: 3 of the 16 visited K - 18, 19 and 20; the
    search visits the same 16 K and returns 20); where they do the score must agree, and the answer must lie in [18, 22]."""
    k, _ = search_blobs(ops, metrics, gold, monkeypatch)
    assert 18 <= k <= 22, k


def test_estimate_k_driver_without_labels(tmp_path):
    x, y, _ = sc.blobs(1200)
    fdir = tmp_path / "extracted_features"
    fdir.mkdir()
    torch.save(dict(all_feats=x, mask_lab=np.zeros(1200, dtype=bool), mask_cls=y < 10, targets=y.astype(np.float64)),
               str(fdir / "synth_blobs_all.pt"))
    cmd = [sys.executable, os.path.join(ROOT, "estimate_k.py"), "--root_dir", str(tmp_path), "--dataset_name", "blobs", "--feat_model", "synth",
           "--max_classes", "64"]
    r = subprocess.run(cmd + ["--criterion", "silhouette"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.load(open(str(tmp_path / "cluster" / "estimated_k_synth_blobs.json")))
    assert out["criterion"] == "silhouette" and out["search_mode"] == "grid" and out["min_classes"] == 2 and out["max_classes"] == 64
    assert 18 <= out["k"] <= 22, out["k"]
    assert "--n_cluster %d" % out["k"] in r.stdout
    assert out["trace"] and all(len(t["ks"]) == len(t["scores"]) for t in out["trace"])
    assert set(out["scores"][str(out["k"])]) == {"silhouette"}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)      # the default criterion still needs labelled rows
    assert r.returncode != 0 and "no labelled row" in r.stderr
