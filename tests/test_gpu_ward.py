"""GPU checks of scd_ward_nearest and scd_ward_merge (scd_amd/csrc/ward.hip), the fit loop and the estimator of scd_amd/ward.py,
main_unsup.py --cluster WARD and estimate_k.py --clusterer ward against the float64 restatement of tests/ward_cases.py: indices equal and
float64 values bit-equal on every case - the restatement sums in fn_dot64's order, so no row is excused.  docs/design/ward.md has the
rules."""
import json
import os

import numpy as np
import pytest
import torch

import ward_cases as wc

pytestmark = pytest.mark.gpu
ALL_CASES = wc.FIT_CASES + tuple(wc.PARTIAL_CASES)


@pytest.fixture(scope="module")
def ops():
    from scd_amd import ops as o
    return o


def dev(a, dtype=None):
    t = torch.as_tensor(np.array(a)).cuda()                 # a copy: the cases' arrays are read-only
    return t if dtype is None else t.to(dtype)


def search(ops, q, qcnt, qself, x, xcnt, ws=None, prepared=0):
    nn, cost, info = ops.ward_nearest(dev(q, torch.float32), dev(qcnt, torch.int32), dev(qself, torch.int32), x if torch.is_tensor(x) else dev(x),
                                      xcnt if torch.is_tensor(xcnt) else dev(xcnt, torch.int32), ws=ws, prepared=prepared)
    return nn.cpu().numpy(), cost.cpu().numpy(), info.cpu().numpy()


def table_part(ws, m, d):
    """The table's part of a workspace (ward_layout): H fp16 [m_alloc, ld], e, h float32, flag int32, q float64 [m_alloc]."""
    m_alloc, ld = -(-m // 128) * 128, -(-d // 64) * 64

    def al(b):
        return -(-b // 256) * 256
    off, out = 0, {}
    for name, dtype, count, size in (("H", torch.float16, m_alloc * ld, 2), ("e", torch.float32, m_alloc, 4), ("h", torch.float32, m_alloc, 4),
                                     ("flag", torch.int32, m_alloc, 4), ("q", torch.float64, m_alloc, 8)):
        out[name] = ws[off:off + count * size].view(dtype).cpu().numpy()
        off += al(count * size)
    return out


# ---------------------------------------------------------------------------------------------------- searches
@pytest.mark.parametrize("name", ALL_CASES)
def test_every_round_bit_for_bit(ops, name):
    """Every round of the restated fit, fed to the device as a table with its dead positions and sizes."""
    f = wc.solved(name)
    n, d = f["x"].shape
    ws = ops.ward_workspace(n, n, d, torch.device("cuda"))
    walked = queries = 0
    for t, r in enumerate(f["rounds"]):
        s = r["stale"]
        nn, cost, info = search(ops, r["x"][s], r["cnt"][s], s, r["x"], r["cnt"], ws=ws)
        print("ward_nearest %-10s round %2d, %5d queries, %5d live: walked %d, flag %d, overflowed %d, most candidates %d"
              % (name, t, len(s), int((r["cnt"] > 0).sum()), info[0], info[1], info[2], info[3]))
        assert np.array_equal(nn, r["nn"]), (name, t)
        assert np.array_equal(cost, r["cost"]), (name, t)       # float64, bit for bit
        assert info[1] == int(name.startswith("flagged")) and 0 <= info[0] <= len(s)
        if name.startswith("flagged"):
            assert info[0] == len(s)                            # every query walks all columns
        if name == "hub4200" and t == 0:
            assert info[0] >= 3000 and info[2] >= 3000          # the 3,000 tied copies overflow their slots and walk
        walked += info[0]
        queries += len(s)
    if name in wc.BLOBS:                                        # the filter path is the common one
        assert walked < 0.1 * queries, (walked, queries)
    if name == "t34_4300":
        assert f["rounds"][0]["nn"][wc.TWIN[name]] == 4299


@pytest.mark.parametrize("name", sorted(wc.search_cases()))
def test_single_searches(ops, name):
    c = wc.search_cases()[name]
    want_nn, want_cost = wc.nearest(c["q"], c["qcnt"], c["qself"], c["x"], c["xcnt"])
    nn, cost, info = search(ops, c["q"], c["qcnt"], c["qself"], c["x"], c["xcnt"])
    print("ward_nearest %-22s walked %d, flag %d, overflowed %d, most candidates %d" % (name, info[0], info[1], info[2], info[3]))
    assert np.array_equal(nn, want_nn) and np.array_equal(cost, want_cost)
    if name == "dead_all_but_self":
        assert nn.tolist() == [-1] and np.isposinf(cost).all()


# ---------------------------------------------------------------------------------------------------- merges
@pytest.mark.parametrize("name", ("n129", "blobs600", "blobs900", "grid1000", "dups900", "flagged449", "t34_4300"))
def test_merges_bit_for_bit(ops, name):
    """scd_ward_merge on the rounds' pairs: the table, the sizes and the workspace's data of the changed positions - the same bytes as a
    preparation of the merged table from nothing; the norms against the restatement's."""
    f = wc.solved(name)
    n, d = f["x"].shape
    cuda = torch.device("cuda")
    for t, r in enumerate(f["rounds"][:6] + f["rounds"][-2:]):
        if len(r["lo"]) == 0:
            continue
        x, cnt = dev(r["x"]), dev(r["cnt"], torch.int32)
        ws = ops.ward_workspace(1, n, d, cuda)
        search(ops, r["x"][:1], [1], [-1], x, cnt, ws=ws)       # prepares the table's part
        ops.ward_merge(x, cnt, dev(r["lo"], torch.int32), dev(r["hi"], torch.int32), ws)
        assert np.array_equal(x.cpu().numpy(), r["x_after"]), (name, t)
        assert np.array_equal(cnt.cpu().numpy(), r["cnt_after"]), (name, t)
        fresh = ops.ward_workspace(1, n, d, cuda)
        search(ops, r["x_after"][:1], [1], [-1], r["x_after"], r["cnt_after"], ws=fresh)
        got, want = table_part(ws, n, d), table_part(fresh, n, d)
        for key in want:
            assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), (name, t, key)
        assert np.array_equal(got["q"][:n], wc.norms(r["x_after"])), (name, t)


def test_merge_leaves_bad_pairs_alone(ops):
    r = wc.solved("blobs600")["rounds"][0]
    x, cnt = dev(r["x"]), dev(r["cnt"], torch.int32)
    cnt[5] = 0
    ws = ops.ward_workspace(1, 600, 16, torch.device("cuda"))
    search(ops, r["x"][:1], [1], [-1], x, cnt, ws=ws)
    before, cbefore = x.clone(), cnt.clone()
    ops.ward_merge(x, cnt, dev([7, 5, 3, -1, 10], torch.int32), dev([7, 9, 2, 4, 600], torch.int32), ws)   # lo == hi, dead, lo > hi, outside
    assert torch.equal(x, before) and torch.equal(cnt, cbefore)


# ---------------------------------------------------------------------------------------------------- whole fits
@pytest.mark.parametrize("name", wc.FIT_CASES)
def test_whole_fit_bit_for_bit(name):
    from scd_amd.ward import ward_tree
    f = wc.solved(name)
    z, info = ward_tree(f["x"])
    print("ward_tree %-10s rounds %d, queries %s, compactions %d, requeries %d, inversions %d"
          % (name, info["rounds"], info["queries"], info["compactions"], info["full_requeries"], info["inversions"]))
    assert np.array_equal(z, f["Z"])                            # float64 heights bit for bit, the same rows in the same order
    assert info["rounds"] == len(f["rounds"]) and info["queries"] == [len(r["stale"]) for r in f["rounds"]]
    assert info["live"] == [int((r["cnt"] > 0).sum()) for r in f["rounds"]]
    assert (info["full_requeries"], info["inversions"]) == (f["full_requeries"], f["inversions"])
    if len(f["x"]) >= 129:
        assert info["compactions"] >= 2                         # the renumbering changed no decision
    if name in ("blobs600", "dups900"):
        z2, _ = ward_tree(f["x"])
        assert np.array_equal(z.view(np.uint8), z2.view(np.uint8))
        z3, info3 = ward_tree(f["x"], compact=False, profile=True)
        assert np.array_equal(z.view(np.uint8), z3.view(np.uint8)) and info3["compactions"] == 0 and len(info3["nearest_ms"]) == info3["rounds"]


def test_normalize_takes_the_unit_rows():
    from scd_amd.ward import ward_tree
    import finch_cases as fc
    x = wc.solved("blobs600")["x"]
    z, _ = ward_tree(x * np.float32(3.0), normalize=True)
    want, _ = ward_tree(fc.unit_rows(x * np.float32(3.0)))
    assert np.array_equal(z, want)


# ---------------------------------------------------------------------------------------------------- the filter
def test_grid_filter_counts_equal_the_model(ops):
    """Exact-grid rows: every fp16 copy and every fp32 dot is exact, so the simulation is the device's count - in the first round and in
    later ones with dead positions and mixed sizes - and the bound's rounding cannot move it (1 % larger or smaller: the same counts)."""
    f = wc.solved("grid1000")
    for t in (0, 1, 3, 8, len(f["rounds"]) - 3):
        r = f["rounds"][t]
        s = r["stale"]
        nn, cost, info = search(ops, r["x"][s], r["cnt"][s], s, r["x"], r["cnt"])
        counts, bounded, _ = wc.simulate_filter(r["x"][s], r["cnt"][s], s, r["x"], r["cnt"])
        print("grid1000 round %d: info %s, model %s" % (t, info.tolist(), wc.filter_info(counts, bounded)))
        assert info.tolist() == wc.filter_info(counts, bounded), t
        for scale in (0.99, 1.01):
            c2, b2, _ = wc.simulate_filter(r["x"][s], r["cnt"][s], s, r["x"], r["cnt"], scale=scale)
            assert np.array_equal(c2, counts) and np.array_equal(b2, bounded)
        assert np.array_equal(nn, r["nn"]) and np.array_equal(cost, r["cost"])


# ---------------------------------------------------------------------------------------------------- end to end
def test_estimator_fit_predict_and_cut():
    from sklearn.metrics import adjusted_rand_score
    from scd_amd.ward import Ward, cut_tree
    import hdbscan_cases as hc
    f = wc.solved("blobs600")
    truth = hc._blobs(600, 16, 6, 0.5, 0)[1]
    w = Ward(n_clusters=6)
    labels = w.fit_predict(torch.as_tensor(f["x"]).cuda())
    assert labels is w.labels_ and np.array_equal(labels, cut_tree(f["Z"], 6)) and adjusted_rand_score(labels, truth) > 0.95
    assert np.array_equal(w.linkage_, f["Z"]) and w.n_leaves_ == 600 and w.children_.shape == (599, 2) and w.distances_.shape == (599,)
    assert np.array_equal(w.cut(18), cut_tree(f["Z"], 18)) and len(np.unique(w.cut(60))) == 60
    coarse, fine = w.cut(6), w.cut(18)                          # cuts are nested
    assert len(set(zip(fine.tolist(), coarse.tolist()))) == 18


def test_main_unsup_ward(tmp_path, capsys):
    """main_unsup.py --synthetic true --cluster WARD end to end: the saved dict holds the linkage next to the predictions, the predictions
    are its cut at --n_cluster, and the naming stage runs on them."""
    import main_unsup as mu
    from scd_amd.ward import cut_tree
    argv = ["--synthetic", "true", "--synthetic_images", "1024", "--synthetic_vocab", "600", "--n_cluster", "8", "--num_common_vote", "10",
            "--num_common_linear", "2", "--topk", "3", "--cluster", "WARD", "--save_cluster", "true", "--root_dir", str(tmp_path),
            "--dataset_name", "synth"]
    cand, u_preds = mu.main(argv)
    print(capsys.readouterr().out)
    a = mu.build_parser().parse_args(argv)
    res = torch.load(str(tmp_path / "cluster" / mu.cluster_result_name(a)), weights_only=False)
    n = len(res["u_preds"])
    assert res["linkage"].shape == (n - 1, 4) and res["all_preds"] is None
    assert np.array_equal(res["u_preds"], cut_tree(res["linkage"], 8)) and len(np.unique(res["u_preds"])) == 8
    assert len(cand) == 8 and len(u_preds) == n


def test_estimate_k_ward_finds_the_planted_k(tmp_path):
    import estimate_k
    import hdbscan_cases as hc
    x, y = hc._blobs(400, 16, 6, 0.4, 0, 7)                     # six separate blobs: the silhouette of the tree's cuts peaks at 6 (0.60)
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "extracted_features"))
    torch.save(dict(all_feats=x, mask_lab=np.zeros(400, dtype=bool), targets=y), os.path.join(root, "extracted_features", "clip_toy_all.pt"))
    out = estimate_k.main(["--root_dir", root, "--dataset_name", "toy", "--clusterer", "ward", "--criterion", "silhouette", "--max_classes", "12"])
    assert out["k"] == 6 and out["clusterer"] == "ward" and out["criterion"] == "silhouette"
    saved = json.load(open(os.path.join(root, "cluster", "estimated_k_clip_toy.json")))
    assert saved["clusterer"] == "ward" and saved["k"] == 6
    mask = np.arange(400) % 2 == 0
    torch.save(dict(all_feats=x, mask_lab=mask, targets=y), os.path.join(root, "extracted_features", "clip_toy_all.pt"))
    out = estimate_k.main(["--root_dir", root, "--dataset_name", "toy", "--clusterer", "ward", "--search_mode", "grid", "--max_classes", "12",
                           "--min_classes", "2"])
    assert out["clusterer"] == "ward" and out["criterion"] == "acc" and 2 <= out["k"] <= 12
    assert set(out["scores"][str(out["k"])]) == {"labelled", "unlabelled"}
