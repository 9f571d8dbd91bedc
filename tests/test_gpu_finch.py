"""GPU checks of the FINCH primitives (scd_amd/csrc/finch.hip), scd_amd.finch and the two drivers on top of them.

The kernels are checked bit for bit: first-neighbour and pair-distance inputs lie on a grid (multiples of 2^-4, or of 2^-20 for the
near-tie ladder and 2^-7 for the simplex, |x| <= 1), so every float64 dot is exact and every correct implementation agrees with tests/finch_cases.py's oracle in
nn AND d1, ties included - no row is excused.  End to end the expected values are the reference's own partitions
(tests/golden/finch.npz, tools/gen_finch_golden.py) on cases whose margins make that a fair demand; at a size where margins are not
controlled every level is checked against the oracle recomputed from that level's device inputs.  docs/design/finch.md has the rules."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import finch_cases as fc
import knn_cases as kc
import silhouette_cases as sc
from oracle import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from scd_amd import ops as o
    return o


@pytest.fixture(scope="module")
def gold(golden):
    return golden("finch.npz")


def grid(seed, n, d, amp=16, step=2.0 ** -4):
    return fc.grid_rows(np.random.RandomState(seed), n, d, amp, step)


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


# ------------------------------------------------------------------------------------------------- scd_first_neighbor
def neighbour_cases():
    out = {}
    out["n2"] = grid(1, 2, 8)
    out["partial_panel"] = grid(2, 257, 64)
    x = grid(3, 300, 40)                                        # d needs zero padding; a zero row at index 0 and one in the middle
    x[0] = 0
    x[150] = 0
    out["pad_d_zero_rows"] = x
    x = grid(4, 1000, 96)
    x[11] = x[12] = x[13] = x[10]                               # four identical rows
    x[900] = x[5]                                               # two identical rows far apart
    out["duplicates"] = x
    out["odd_d"] = grid(10, 130, 37)                            # d no multiple of 4: the float64 dot's scalar loads
    out["d768"] = grid(5, 640, 768)
    out["many_panels"] = grid(6, 5000, 64)
    # exact two-way ties: rows i with one best dot reached by two identical columns in different 16-column sub-tiles and tiles, below
    # i, above i and on both sides; the background rows are small, so the planted columns are the maximum (the oracle decides anyway)
    x = grid(7, 400, 64, amp=4)
    for t, (i, j1, j2) in enumerate(((200, 37, 310), (20, 150, 390), (380, 5, 100))):
        v = np.zeros(64, dtype=np.float32)
        v[8 * t:8 * t + 8] = [1, -1, 1, 1, -1, 1, -1, 1]
        x[j1] = x[j2] = v
        x[i] = 0.5 * v
    out["ties"] = x
    # the ladder: 64 rows whose best (the last row) and second-best (row 0) dots differ by 2^-40, far below fp16 resolution
    x = np.zeros((66, 8), dtype=np.float32)
    x[0, 0] = 1.0
    x[65, 0], x[65, 1] = 1.0, 2.0 ** -20
    x[1:65, 0] = (np.arange(64) + 1) / 128.0
    x[1:65, 1] = 2.0 ** -20
    out["ladder"] = x
    # every pair's dot is exactly -1 / 128: one of the 8 padding columns of the tile (approximate dot 0) would win if it were admitted
    out["simplex120"] = kc.simplex_rows()
    return out


NEIGHBOUR = neighbour_cases()


@pytest.mark.parametrize("name", list(NEIGHBOUR))
def test_first_neighbor_bit_for_bit(ops, name):
    x = NEIGHBOUR[name]
    want_nn, want_d1 = fc.first_neighbor(x)
    nn, d1, info = ops.first_neighbor(dev(x))
    nn2, d12, info2 = ops.first_neighbor(dev(x))
    nn, d1, info = nn.cpu().numpy(), d1.cpu().numpy(), info.cpu().numpy()
    print("first_neighbor %-16s n %5d d %4d: %d rows through the exact pass" % (name, x.shape[0], x.shape[1], info[0]))
    assert info[1] == 0 and 0 <= info[0] <= x.shape[0]
    assert np.array_equal(nn, want_nn)
    assert np.array_equal(d1, want_d1)                          # float64, exact
    assert np.array_equal(nn2.cpu().numpy(), nn) and np.array_equal(d12.cpu().numpy(), d1) and np.array_equal(info2.cpu().numpy(), info)
    if name == "ties":
        assert nn[200] == 37 and nn[20] == 150 and nn[380] == 5
    if name == "ladder":
        assert (nn[1:65] == 65).all() and nn[0] == 65 and nn[65] == 0
    if name == "pad_d_zero_rows":
        assert nn[0] == 1 and nn[150] == 0 and d1[0] == 1.0 and d1[150] == 1.0
    if name == "duplicates":
        assert list(nn[10:14]) == [11, 10, 10, 10] and nn[5] == 900 and nn[900] == 5
    if name == "simplex120":
        assert nn.max() < 120 and nn[0] == 1 and (nn[1:] == 0).all() and (d1 == 1.0 + 1.0 / 128).all()


def test_first_neighbor_limits(ops):
    from scd_amd._lib import ScdError
    with pytest.raises(ScdError):
        ops.first_neighbor(dev(grid(8, 1, 8)))
    with pytest.raises(ScdError):
        ops.first_neighbor(dev(grid(8, 4, 1025)))
    # a value that does not fit fp16: every row takes the exact pass and the answer is still the oracle's
    x = grid(9, 70, 8)
    x[3, 2] = 131072.0
    nn, d1, info = ops.first_neighbor(dev(x))
    want_nn, want_d1 = fc.first_neighbor(x)
    assert info.cpu().tolist() == [70, 1] and np.array_equal(nn.cpu().numpy(), want_nn) and np.array_equal(d1.cpu().numpy(), want_d1)


# ------------------------------------------------------------------------------------------------- scd_link_components
def component_cases():
    out = {}
    i = np.arange(1, 5000)
    out["chain"] = (5000, i, i - 1)
    i = np.arange(1, 3000)
    out["star"] = (3000, i, np.zeros_like(i))
    i = np.arange(2000)
    out["two_cycles"] = (2000, i, i ^ 1)
    r = np.random.RandomState(11)
    n = 10000
    nn = r.randint(0, 9900, size=n)                             # the last 100 nodes are nobody's neighbour ...
    nn = np.where(nn == np.arange(n), (nn + 1) % 9900, nn)
    keep = r.rand(n) > 1.0 / 3.0                                # ... a third of the edges is cut ...
    keep[9900:] = False                                         # ... and theirs are: isolated nodes
    sa, sb = r.randint(0, 9900, size=500), r.randint(0, 9900, size=500)
    ok = sa != sb
    out["random_cut_siblings"] = (n, np.concatenate([np.arange(n)[keep], sa[ok]]), np.concatenate([nn[keep], sb[ok]]))
    out["no_edges"] = (7, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    return out


COMPONENTS = component_cases()


@pytest.mark.parametrize("name", list(COMPONENTS))
def test_link_components(ops, name):
    n, ea, eb = COMPONENTS[name]
    want, k = fc.components(n, ea, eb)
    labels, ncomp = ops.link_components(n, dev(ea, torch.int32), dev(eb, torch.int32))
    assert ncomp == k and np.array_equal(labels.cpu().numpy(), want)
    if name == "random_cut_siblings":
        assert (np.bincount(want)[want[9900:]] == 1).all()      # the isolated nodes are singletons
    rev, ncomp2 = ops.link_components(n, dev(eb[::-1].copy(), torch.int32), dev(ea[::-1].copy(), torch.int32))
    assert ncomp2 == k and np.array_equal(rev.cpu().numpy(), want)


def test_link_components_rejects_bad_edge(ops):
    from scd_amd._lib import ScdError
    with pytest.raises(ScdError):
        ops.link_components(5, dev(np.array([0, 7]), torch.int32), dev(np.array([1, 2]), torch.int32))


# ------------------------------------------------------------------------------------------------- scd_pair_dist_f64
@pytest.mark.parametrize("m,d", [(1, 40), (300, 40), (300, 37)])
def test_pair_dist(ops, m, d):
    x = grid(12, 50, d)
    r = np.random.RandomState(13)
    a, b = r.randint(0, 50, size=m), r.randint(0, 50, size=m)
    got = ops.pair_dist_f64(dev(x), dev(a, torch.int32), dev(b, torch.int32)).cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, fc.pair_dist(x, a, b))


# ------------------------------------------------------------------------------------------------- scd_segment_mean_unit
def run_means(ops, x, labels, k):
    from scd_amd.finch import _segments
    order, offsets = _segments(dev(labels, torch.int32), k)
    assert np.array_equal(order.cpu().numpy(), np.argsort(labels, kind="stable"))
    mean, unit = ops.segment_mean_unit(dev(x), order, offsets)
    return mean.cpu().numpy(), unit.cpu().numpy()


def check_units(mean, unit):
    nrm = np.sqrt((unit.astype(np.float64) ** 2).sum(1))
    zero = ~mean.any(axis=1)
    assert (np.abs(nrm[~zero] - 1.0) <= 2.0 ** -23).all() and not unit[zero].any()
    want = fc.unit_rows(mean)
    assert (np.abs(unit - want) <= np.spacing(np.abs(want))).all()


def test_segment_means_exact_on_grid(ops):
    n, d = 3000, 70
    x = grid(14, n, d)
    r = np.random.RandomState(15)
    labels = np.empty(n, dtype=np.int64)
    labels[:2000] = 0                                           # a segment of 2,000 rows
    labels[2000:2100] = np.arange(1, 101)                       # singletons
    labels[2100:] = 101 + r.randint(0, 40, size=n - 2100)
    x[2100] = 0
    x[labels == labels[2100]] = 0                               # a segment whose mean is zero
    perm = r.permutation(n)
    x, labels = x[perm], labels[perm]
    k = int(labels.max()) + 1
    mean, unit = run_means(ops, x, labels, k)
    assert np.array_equal(mean, fc.segment_means(x, labels, k))     # the sums are exact: bit-equal
    assert not mean[labels[np.nonzero(perm == 2100)[0][0]]].any()
    check_units(mean, unit)


def test_segment_means_blobs_and_one_segment(ops):
    x, y, _ = synth.clustered_features(1500, 48, 37, seed=3, center_seed=4, noise=0.9)
    mean, unit = run_means(ops, x, y, 37)
    want = fc.segment_means(x, y, 37)
    assert (np.abs(mean - want) <= np.spacing(np.abs(want))).all()
    check_units(mean, unit)
    mean, unit = run_means(ops, x[:500], np.zeros(500, dtype=np.int64), 1)    # k = 1
    want = fc.segment_means(x[:500], np.zeros(500, dtype=np.int64), 1)
    assert mean.shape == (1, 48) and (np.abs(mean - want) <= np.spacing(np.abs(want))).all()
    check_units(mean, unit)


# ------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", list(fc.CASES))
def test_finch_matches_the_reference(ops, gold, name):
    from scd_amd.local_utils.finch import FINCH
    x = fc.case_input(name)
    c, num, req = FINCH(x, verbose=False)
    assert req is None and num == gold["num_" + name].tolist() and np.array_equal(c, gold["c_" + name])
    for r in fc.CASES[name][6]:
        c, num, req = FINCH(x, req_clust=r, verbose=False)
        assert np.array_equal(c, gold["c_" + name]) and np.array_equal(req, gold["req_%s_%d" % (name, r)])
    if fc.CASES[name][5]:                                       # fp16 input and its fp32 copy: the same partitions
        c16, num16, _ = FINCH(dev(x.astype(np.float16)), verbose=False)
        assert num16 == num and np.array_equal(c16, gold["c_" + name])


def test_finch_interface(ops, gold):
    from scd_amd.finch import FINCH, Finch
    x = fc.case_input("b600")
    f = Finch(keep_levels=True).fit(dev(x))
    assert f.partitions_device_.is_cuda and f.partitions_device_.dtype == torch.int32 and tuple(f.partitions_device_.shape) == (600, 3)
    assert f.num_clust_ == [96, 14, 12] and f.req_labels_device_ is None and len(f.levels_) == 3 and len(f.exact_rows_) == 3
    assert f.min_sim_ == pytest.approx(fc.finch_f64(x, return_levels=True)[4], rel=1e-12)
    # initial_rank = the level-0 neighbours reproduces level 0; there is no min_sim then (finch.py:22-23)
    g = Finch().fit(x, initial_rank=f.levels_[0]["nn"])
    assert g.min_sim_ is None and torch.equal(g.partitions_device_[:, 0], f.partitions_device_[:, 0])
    want = fc.finch_f64(x, initial_rank=f.levels_[0]["nn"].cpu().numpy())
    assert g.num_clust_ == want[1] and np.array_equal(g.partitions_device_.cpu().numpy(), want[0])
    with pytest.raises(ValueError):
        FINCH(x, req_clust=97, verbose=False)
    with pytest.raises(ValueError):
        FINCH(x, distance="euclidean", verbose=False)


def test_finch_stagewise_on_uncontrolled_blobs(ops):
    """3000 x 64, 20 classes: margins are not controlled here, so each level's kernels are pinned against the oracle recomputed from
    that level's DEVICE inputs: nn from the device U, the labels from the device nn and d1, the means from the composed labels."""
    from scd_amd.finch import Finch
    x, _, _ = synth.clustered_features(3000, 64, 20, noise=0.6)
    f = Finch(keep_levels=True).fit(x)
    print("stagewise: clusters %s, rows through the exact pass %s, min_sim %.6f" % (f.num_clust_, f.exact_rows_, f.min_sim_))
    assert len(f.levels_) == len(f.num_clust_) >= 2
    composed = None
    for li, lv in enumerate(f.levels_):
        u, nn, d1, lab, means = (lv[key].cpu().numpy() for key in ("U", "nn", "d1", "labels", "means"))
        want_nn, want_d1 = fc.first_neighbor(u)
        assert np.array_equal(nn, want_nn) and np.abs(d1 - want_d1).max() <= 1e-14
        if li == 0:
            assert abs(f.min_sim_ - fc.min_sim_of(u, nn, d1)) <= 1e-14
            assert np.array_equal(means, x)
        else:
            want_means = fc.segment_means(x, composed, f.num_clust_[li - 1])
            assert (np.abs(means - want_means) <= np.spacing(np.abs(want_means))).all()
        want_u = fc.unit_rows(means)
        assert (np.abs(u - want_u) <= np.spacing(np.abs(want_u))).all()
        want_lab, k = fc.level_labels(u, nn, d1, None if li == 0 else f.min_sim_)
        assert k == f.num_clust_[li] and np.array_equal(lab, want_lab)
        composed = lab if composed is None else lab[composed]
        assert np.array_equal(f.partitions_device_[:, li].cpu().numpy(), composed)


# ------------------------------------------------------------------------------------------------- drivers
def test_main_unsup_with_finch(ops, monkeypatch):
    import importlib
    mu = importlib.import_module("main_unsup")
    seen = {}
    inner = mu.run_clustering

    def spy(args, *a):
        out = inner(args, *a)
        seen["preds"] = np.asarray(out[1])
        return out

    monkeypatch.setattr(mu, "run_clustering", spy)
    cand, u_preds = mu.main(["--synthetic", "true", "--synthetic_images", "1536", "--synthetic_vocab", "600", "--n_cluster", "8",
                             "--cluster", "FINCH", "--topk", "3", "--num_common_vote", "10", "--num_common_linear", "2"])
    assert len(np.unique(seen["preds"])) == 8 and seen["preds"].min() == 0 and seen["preds"].max() == 7
    assert len(cand) == 8 and len(u_preds) == len(seen["preds"])


def test_estimate_k_driver_finch(tmp_path):
    x, y, _ = sc.blobs(3000)
    fdir = tmp_path / "extracted_features"
    fdir.mkdir()
    torch.save(dict(all_feats=x, mask_lab=np.zeros(3000, dtype=bool), mask_cls=y < 10, targets=y.astype(np.float64)),
               str(fdir / "synth_blobs_all.pt"))
    cmd = [sys.executable, os.path.join(ROOT, "estimate_k.py"), "--root_dir", str(tmp_path), "--dataset_name", "blobs", "--feat_model", "synth",
           "--max_classes", "64", "--criterion", "silhouette", "--search_mode", "finch"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.load(open(str(tmp_path / "cluster" / "estimated_k_synth_blobs.json")))
    print("estimate_k finch: partitions %s, K %d" % (out["finch_num_clust"], out["k"]))
    assert out["search_mode"] == "finch" and out["criterion"] == "silhouette"
    assert len(out["finch_num_clust"]) >= 2 and out["finch_num_clust"] == sorted(out["finch_num_clust"], reverse=True)
    assert 16 <= out["k"] <= 24, out
    assert out["k"] in [min(max(v, 2), 64) for v in out["finch_num_clust"]]
