"""GPU checks of scd_mr_nearest (scd_amd/csrc/hdbscan.hip), the fit loop and the estimator of scd_amd/hdbscan.py and main_unsup.py
--cluster HDBSCAN against the float64 restatement of tests/hdbscan_cases.py: indices equal and float64 values bit-equal on every case - the
restatement sums in fn_dot64's order, so no row is excused.  docs/design/hdbscan.md has the rules."""
import numpy as np
import pytest
import torch

import hdbscan_cases as hc

pytestmark = pytest.mark.gpu
UNIT_CASES = tuple(n for n in hc.CASES if n not in ("grid1000", "flagged449", "flagged1345"))


@pytest.fixture(scope="module")
def ops():
    from scd_amd import ops as o
    return o


def dev(a, dtype=None):
    t = torch.as_tensor(np.array(a)).cuda()                 # a copy: the cases' arrays are read-only
    return t if dtype is None else t.to(dtype)


def rounds(ops, case, comps, name):
    """scd_mr_nearest on each labelling of `comps` with one workspace (the fp16 copy made by the first call): every answer bit for bit."""
    u, core = dev(case["x"]), dev(case["core"])
    ws = ops.mr_nearest_workspace(u)
    infos = []
    for q, comp in enumerate(comps):
        comp = np.asarray(comp).astype(np.int32)
        nn, r, info = ops.mr_nearest(u, core, dev(comp), ws=ws, prepared=q > 0)
        nn, r, info = nn.cpu().numpy(), r.cpu().numpy(), info.cpu().numpy()
        want_nn, want_r = hc.nearest_round(case["r"], comp)
        print("mr_nearest %-12s labelling %d, %5d components: walked rows %d, flag %d, overflowed rows %d, most candidates %d"
              % (name, q, len(np.unique(comp)), info[0], info[1], info[2], info[3]))
        assert np.array_equal(nn, want_nn), (name, q)
        assert np.array_equal(r, want_r), (name, q)             # float64, bit for bit
        infos.append(info)
    return infos


@pytest.mark.parametrize("name", hc.CASES)
def test_one_round_bit_for_bit(ops, name):
    """The first round (every row its own component) and every later labelling of the restated fit."""
    case = hc.solved(name)
    n = len(case["x"])
    infos = rounds(ops, case, [np.arange(n)] + list(case["comps"][1:]), name)
    flagged = name.startswith("flagged")
    for info in infos:
        assert info[1] == int(flagged) and 0 <= info[0] <= n
        if flagged:
            assert info[0] == n                                 # every row walks all columns
    if name == "hub4200":
        assert infos[0][0] >= 3000 and infos[0][2] >= 3000      # the 3,000 tied copies overflow their slots and walk


def test_masks(ops):
    case = hc.solved("blobs1650")
    n = len(case["x"])
    m = hc.masks(n)
    infos = rounds(ops, case, list(m.values()), "masks")
    all_equal = list(m).index("all_equal")
    assert infos[all_equal][0] == n and infos[all_equal][3] == 0   # no foreign column: no bound, nothing emitted, -1 / -inf everywhere


def test_grid_filter_counts_equal_the_model(ops):
    """Every fp16 copy and every fp32 dot of grid1000 is exact, so the simulation is the device's filter: info equals its counts, and a
    bound 1 % larger or smaller gives the same counts (the float32 rounding of h_i cannot move them)."""
    case = hc.solved("grid1000")
    infos = rounds(ops, case, case["comps"], "grid1000")
    for comp, info in zip(case["comps"], infos):
        want = hc.filter_info(*hc.simulate_filter(case["x"], case["core"], comp)[:2])
        for scale in (0.99, 1.01):
            assert hc.filter_info(*hc.simulate_filter(case["x"], case["core"], comp, scale=scale)[:2]) == want
        assert (int(info[0]), int(info[2]), int(info[3])) == want


def fit_mst(case):
    from scd_amd.hdbscan import mutual_reachability_mst
    return mutual_reachability_mst(dev(case["x"]), case["min_samples"], normalize=False)


@pytest.mark.parametrize("name", hc.CASES)
def test_mst_bit_for_bit(name):
    case = hc.solved(name)
    lo, hi, r, w, info = fit_mst(case)
    print("mst %-12s n %5d: %d rounds, components %s, round info %s, knn info %s"
          % (name, len(case["x"]), info["rounds"], info["components"], info["round_info"], info["knn"]))
    assert lo.dtype == np.int32 and hi.dtype == np.int32 and r.dtype == np.float64 and w.dtype == np.float64
    assert np.array_equal(lo, case["lo"]) and np.array_equal(hi, case["hi"])
    assert np.array_equal(r, case["r_mst"]) and np.array_equal(w, case["weight"])
    assert info["rounds"] == len(case["comps"]) and info["components"] == [len(np.unique(c)) for c in case["comps"]]


@pytest.mark.parametrize("name", UNIT_CASES)
def test_labels_equal_the_restated_pipeline(name):
    from scd_amd.hdbscan import HDBSCAN
    case = hc.solved(name)
    variants = [("eom", False)] + ([("leaf", False), ("eom", True)] if name in ("blobs900", "dups900", "n2") else [])
    for method, single in variants:
        h = HDBSCAN(min_cluster_size=case["min_cluster_size"], min_samples=case["min_samples"], cluster_selection_method=method,
                    allow_single_cluster=single).fit(case["raw"])
        want, wprob = hc.sklearn_labels(case["lo"], case["hi"], case["weight"], case["min_cluster_size"], method, single)
        print("fit %-12s %s single=%s: %d clusters, %d noise rows" % (name, method, single, h.n_clusters_, int((h.labels_ < 0).sum())))
        assert all(np.array_equal(a, case[k]) for a, k in zip(h.mst_, ("lo", "hi", "r_mst", "weight")))    # the device's unit rows are the case's
        assert h.labels_.dtype == np.int64 and np.array_equal(h.labels_, want)
        assert np.array_equal(np.isnan(h.probabilities_), np.isnan(wprob))
        assert np.all(np.abs(h.probabilities_ - wprob)[~np.isnan(wprob)] <= 1e-12)
        assert h.n_clusters_ == int(want.max()) + 1
    if name in hc.SKLEARN_FINDS:
        h = HDBSCAN(min_cluster_size=case["min_cluster_size"], min_samples=case["min_samples"]).fit(case["raw"])
        assert (h.n_clusters_, int((h.labels_ < 0).sum())) == hc.SKLEARN_FINDS[name]


def test_min_samples_none_means_min_cluster_size():
    from scd_amd.hdbscan import HDBSCAN
    case = hc.solved("blobs660")                                # min_samples = min_cluster_size = 15
    a = HDBSCAN(min_cluster_size=15).fit_predict(dev(case["raw"]))
    assert np.array_equal(a, hc.sklearn_labels(case["lo"], case["hi"], case["weight"], 15)[0])


def test_two_fits_return_the_same_bits():
    from scd_amd.hdbscan import HDBSCAN
    case = hc.solved("blobs1650")
    a = HDBSCAN(min_cluster_size=20, min_samples=5).fit(case["raw"])
    b = HDBSCAN(min_cluster_size=20, min_samples=5).fit(case["raw"])
    assert a.labels_.tobytes() == b.labels_.tobytes() and a.probabilities_.tobytes() == b.probabilities_.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.mst_, b.mst_))


@pytest.mark.parametrize("name", hc.FILTER_CAP_CASES)
def test_filter_cap(name):
    """Rows through the exact walk plus overflowed rows, summed over the rounds, stay under 10 % of rows x rounds (the CPU simulation: 0)."""
    case = hc.solved(name)
    info = fit_mst(case)[4]
    walked = sum(i[0] + i[2] for i in info["round_info"])
    print("filter cap %-10s: %d walked or overflowed rows in %d rounds of %d rows" % (name, walked, info["rounds"], len(case["x"])))
    assert walked < 0.1 * len(case["x"]) * info["rounds"]


def test_attach_noise_gives_the_nearest_clustered_row():
    from scd_amd.hdbscan import attach_noise
    case = hc.solved("blobs660")
    labels = hc.sklearn_labels(case["lo"], case["hi"], case["weight"], 15)[0]
    full = attach_noise(case["raw"], labels)
    noise = labels < 0
    v = np.where(noise[None, :], -np.inf, case["v"])            # float64 values; argmax takes the lowest column of a tie, as scd_knn does
    assert np.array_equal(full[~noise], labels[~noise]) and np.array_equal(full[noise], labels[np.argmax(v[noise], axis=1)])
    assert full.min() >= 0


def test_main_unsup_hdbscan(tmp_path, capsys):
    """main_unsup.py --synthetic true --cluster HDBSCAN end to end: the saved dict has the new keys and a full partition, the number of
    clusters is a result and the naming stage runs on it."""
    import main_unsup as mu
    argv = ["--synthetic", "true", "--synthetic_images", "1024", "--synthetic_vocab", "600", "--n_cluster", "8", "--num_common_vote", "10",
            "--num_common_linear", "2", "--topk", "3", "--cluster", "HDBSCAN", "--min_cluster_size", "20", "--save_cluster", "true",
            "--root_dir", str(tmp_path), "--dataset_name", "synth"]
    cand, u_preds = mu.main(argv)
    out = capsys.readouterr().out
    print(out)
    a = mu.build_parser().parse_args(argv)
    assert mu.cluster_result_name(a).endswith("_synth_mcs20.pt") and mu.cluster_result_name(a).startswith("HDBSCAN_")
    res = torch.load(str(tmp_path / "cluster" / mu.cluster_result_name(a)), weights_only=False)
    k = res["n_cluster"]
    n = len(res["u_preds"])
    assert k >= 1 and "HDBSCAN: n_cluster = %d" % k in out
    assert res["noise"].dtype == bool and res["noise"].shape == (n,) and res["probabilities"].shape == (n,)
    assert res["u_preds"].min() >= 0 and res["u_preds"].max() == k - 1 and len(np.unique(res["u_preds"])) == k     # a full partition
    assert np.all(res["probabilities"][res["noise"]] == 0.0)
    assert len(cand) == k and len(u_preds) == n
    a2 = mu.build_parser().parse_args(argv + ["--min_samples", "7"])
    assert mu.cluster_result_name(a2).endswith("_synth_mcs20_ms7.pt")
