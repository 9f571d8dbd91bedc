"""GPU checks of scd_knn / scd_knn_vote (scd_amd/csrc/knn.hip), scd_amd.knn and score_features.py against the float64 restatement of
tests/knn_cases.py: indices equal and dots bit-equal on every case - the restatement sums in fn_dot64's order, so no row is excused.
docs/design/knn.md has the rules."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import finch_cases as fc
import knn_cases as kc

pytestmark = pytest.mark.gpu
GIB = 1 << 30


@pytest.fixture(scope="module")
def ops():
    from scd_amd import ops as o
    return o


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def run(ops, case):
    x = dev(case["x"])
    if case["q"].shape == case["x"].shape and np.array_equal(case["q"], case["x"]):
        q = x                                                   # the graph: one buffer, prepared once
    else:
        q = dev(case["q"])
    idx, dot, info = ops.knn(q, x, case["k"], case["self_base"])
    return idx.cpu().numpy(), dot.cpu().numpy(), info.cpu().numpy()


def check(ops, case, name):
    want_idx, want_dot = kc.knn_f64(case["q"], case["x"], case["k"], case["self_base"])
    idx, dot, info = run(ops, case)
    print("knn %-24s m %5d n %5d d %4d k %2d: exact rows %d, flag %d, overflowed rows %d, most candidates %d"
          % (name, case["q"].shape[0], case["x"].shape[0], case["x"].shape[1], case["k"], info[0], info[1], info[2], info[3]))
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(dot, want_dot)                        # float64, bit for bit
    return idx, dot, info


SHAPES = kc.shape_cases()


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_bit_for_bit(ops, name):
    case = SHAPES[name]
    _, _, info = check(ops, case, name)
    assert info[1] == 0 and 0 <= info[0] <= case["q"].shape[0]
    if name in ("n130_graph_k64", "n257_graph_k64", "n64_q129_k64"):
        assert info[0] == case["q"].shape[0]                    # fewer than k kept columns: no bound, the exact pass


def test_exact_ties(ops):
    case = kc.tie_case()
    idx, dot, info = check(ops, case, "ties")
    assert list(idx[10][:3]) == [11, 12, 13] and list(idx[13][:3]) == [10, 11, 12] and idx[5][0] == 390 and idx[390][0] == 5
    assert info[0] < case["q"].shape[0]                         # the filter decided rows here, ties included


def test_slot_overflow(ops):
    slots = ops._L().scd_knn_slots()
    assert slots == 512                                         # tests/test_knn_host.py sizes its cases by it
    case = kc.overflow_case(slots)
    n = case["x"].shape[0]
    idx, dot, info = check(ops, case, "overflow")
    assert n == 2 * slots + 3 and info[2] > 0 and info[0] >= info[2] and info[3] == n - 1
    assert list(idx[0]) == [1, 2, 3, 4, 5] and list(idx[3]) == [0, 1, 2, 4, 5] and list(idx[n - 1]) == [0, 1, 2, 3, 4]


DEGENERATE = kc.degenerate_cases()


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_inputs(ops, name):
    case = DEGENERATE[name]
    idx, dot, info = check(ops, case, name)
    m = case["q"].shape[0]
    if name == "zero_rows":
        assert list(idx[0]) == [1, 2, 3, 4, 5, 6, 7] and (dot[0] == 0).all() and (dot[150] == 0).all() and info[1] == 0
    if name == "tiny_2m20":
        assert info[1] == 0 and dot.max() < 2.0 ** -30 and dot.max() > 0
    if name == "fp16_overflow":
        assert info[1] == 1 and info[0] == m


def test_shard_equals_rows_of_the_graph(ops):
    case = kc.shard_case()
    a, b = kc.SHARD
    x = dev(case["x"])
    full_idx, full_dot, _ = ops.knn(x, x, case["k"], 0)
    idx, dot, info = ops.knn(x[a:b], x, case["k"], a)           # a view into x: rows a .. b
    assert torch.equal(idx, full_idx[a:b]) and torch.equal(dot, full_dot[a:b])
    want_idx, want_dot = kc.knn_f64(case["q"], case["x"], case["k"], a)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(dot.cpu().numpy(), want_dot)
    assert not (idx.cpu().numpy() == (a + np.arange(b - a))[:, None]).any()


def test_two_calls_same_bits(ops):
    case = SHAPES["n1000_graph_d64_k17"]
    first, second = run(ops, case), run(ops, case)
    for u, v in zip(first, second):
        assert np.array_equal(u, v)


@pytest.fixture(scope="module")
def blobs():
    return {name: kc.blob_case(name) for name in kc.BLOBS}


@pytest.mark.parametrize("name", list(kc.BLOBS))
def test_filter_path_decides(ops, blobs, name):
    """The filter must carry these cases: at most 10 % of the rows may take the exact pass, so the test cannot pass on it alone
    (tests/test_knn_host.py: the simulated filter gives every row at most half the slots)."""
    case = blobs[name]
    m = case["q"].shape[0]
    _, _, info = check(ops, case, name)
    assert info[1] == 0 and info[0] + info[2] <= m // 10
    assert case["k"] <= info[3] <= 512


# ------------------------------------------------------------------------------------------------- the paths that need n > 4096
# tests/test_knn_host.py asserts what each case is named for: the tiles per range on any device, the chunks, the negative maxima.
TILES = kc.tile_cases()


@pytest.mark.parametrize("name", list(TILES))
def test_several_tiles_per_range(ops, name):
    """More than 32 tiles: a range of both MFMA passes holds 2 or 3 tiles, so the running maximum is carried across tiles, the LDS ring
    is filled again behind the last barrier, the last range is cut short, and a self column lies in the second tile of its range.  The
    simulated filter gives every row at most 256 candidates, so the exact pass alone cannot pass these."""
    case = TILES[name]
    m = case["q"].shape[0]
    idx, dot, info = check(ops, case, name)
    assert info[1] == 0 and info[0] + info[2] <= m // 10
    if name == "t33_q129":
        assert idx[5][0] == 4096 and idx[77][0] == 4095         # the one valid column of the last tile, and the last of the tile before
    if name == "border_shard":                                  # again with Q a view into x: the same bits as with a copy of those rows
        a, b = kc.BORDER
        x = dev(case["x"])
        v_idx, v_dot, v_info = ops.knn(x[a:b], x, case["k"], a)
        assert x[a:b].data_ptr() == x.data_ptr() + a * x.shape[1] * 4
        assert np.array_equal(v_idx.cpu().numpy(), idx) and np.array_equal(v_dot.cpu().numpy(), dot)
        assert np.array_equal(v_info.cpu().numpy(), info)
        assert not (idx == (a + np.arange(b - a))[:, None]).any()


CHUNKED = kc.chunk_cases()


@pytest.mark.parametrize("name", list(CHUNKED))
def test_exact_pass_many_chunks(ops, name):
    """The exact pass over 2 to 10 chunks of 448 columns with distinct values: columns of later chunks displace earlier ones, 64 best
    so far + 448 fill the LDS arrays exactly, a last chunk of one column, the self entry in a later chunk."""
    case = CHUNKED[name]
    m = case["q"].shape[0]
    _, _, info = check(ops, case, name)
    if name in ("hub", "offset"):                               # every row has a bound, and more candidates than slots
        assert info[1] == 0 and info[0] == m and info[2] == m and info[3] > 512
    else:                                                       # a value that does not fit fp16: no row has a bound
        assert info[1] == 1 and info[0] == m and info[2] == 0


NEGATIVE = kc.negative_cases()


@pytest.mark.parametrize("name", list(NEGATIVE))
def test_negative_dots(ops, name):
    """Every admissible dot is negative, so a padding column (approximate dot 0) or the exact pass's self entry (value 0) would win."""
    case = NEGATIVE[name]
    n = case["x"].shape[0]
    idx, dot, info = run(ops, case)
    print("knn %-24s exact rows %d, flag %d, overflowed rows %d, most candidates %d" % (name, info[0], info[1], info[2], info[3]))
    assert idx.max() < n and idx.min() >= 0, "a padding column or an empty entry leaked into the answer"
    want_idx, want_dot = kc.knn_f64(case["q"], case["x"], case["k"], case["self_base"])
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(dot, want_dot)                        # float64, bit for bit
    assert dot.max() < 0
    if name == "neg_flagged":
        assert info[1] == 1 and info[0] == case["q"].shape[0]
        assert not (idx == (case["self_base"] + np.arange(idx.shape[0]))[:, None]).any()
    else:
        assert info[1] == 0 and info[0] == 0                    # the filter decided these
    if name == "simplex120":
        assert list(idx[0]) == [1, 2, 3, 4, 5] and list(idx[3]) == [0, 1, 2, 4, 5] and list(idx[119]) == [0, 1, 2, 3, 4]


def test_same_buffer_without_exclusion(ops):
    """One device buffer as Q and as X with self_base = -1: one preparation serves both sides and nothing is excluded."""
    case = kc.same_no_self_case()
    x = dev(case["x"])
    idx, dot, info = ops.knn(x, x, case["k"], -1)
    idx, dot = idx.cpu().numpy(), dot.cpu().numpy()
    want_idx, want_dot = kc.knn_f64(case["q"], case["x"], case["k"], -1)
    assert np.array_equal(idx, want_idx) and np.array_equal(dot, want_dot)
    first = np.arange(1000)
    first[11:14] = 10                                           # the lowest-index duplicate
    assert np.array_equal(idx[:, 0], first) and list(idx[12][:4]) == [10, 11, 12, 13]
    c_idx, c_dot, _ = ops.knn(x.clone(), x, case["k"], -1)      # two buffers: two preparations, the same bits
    assert np.array_equal(c_idx.cpu().numpy(), idx) and np.array_equal(c_dot.cpu().numpy(), dot)


@pytest.mark.parametrize("name", ["border_shard", "ties", "simplex120"])
def test_filter_counts_equal_the_model(ops, name):
    """Exact-grid rows: e_i = 0 and every approximate dot is exact in fp32 in any order, so knn_cases.simulate_filter is no simulation
    but the device's own count (tests/test_knn_host.py: no count moves when B_i is scaled by 1 +- 2^-10).  A bound too loose, or a
    threshold from another rank, still returns the right neighbours - and shows here."""
    case = {"border_shard": TILES["border_shard"], "ties": kc.tie_case(), "simplex120": NEGATIVE["simplex120"]}[name]
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    want = kc.filter_info(case, ops._L().scd_knn_slots(), cu)
    _, _, info = run(ops, case)
    print("knn %-24s on %d compute units: info %s, the model (exact rows, overflowed rows, most candidates) %s" % (name, cu, [int(v) for v in info], want))
    assert info[1] == 0
    assert (info[0], info[2], info[3]) == want


# ------------------------------------------------------------------------------------------------- the vote
@pytest.mark.parametrize("mode", ["uniform", "softmax"])
def test_vote_against_restatement(ops, mode):
    idx, dot, labels = kc.vote_case()
    for k_use in (8, 5, 1):
        want_pred, want_score = kc.vote_f64(idx, dot, labels, k_use=k_use, mode=mode, temperature=0.07)
        pred, score = ops.knn_vote(dev(idx, torch.int32), dev(dot), dev(labels, torch.int32), k_use=k_use,
                                   mode=ops.KNN_UNIFORM if mode == "uniform" else ops.KNN_SOFTMAX, temperature=0.07)
        pred, score = pred.cpu().numpy(), score.cpu().numpy()
        assert np.array_equal(pred, want_pred)
        if mode == "uniform":
            assert np.array_equal(score, want_score)
        else:                                                   # exp may differ from numpy's in the last place; sums of at most 8 terms
            np.testing.assert_allclose(score, want_score, rtol=1e-14 * 8, atol=0)
        assert pred[0] == -1 and score[0] == 0                  # no valid neighbour
    assert (want_pred == -1).sum() >= 1 and (labels < 0).any()


def test_vote_any_label_range(ops):
    idx, dot, labels = kc.vote_case()
    big = np.where(labels >= 0, labels * 500000000 + 7, -3)     # up to 1,500,000,007: no per-class table could hold it
    want, _ = kc.vote_f64(idx, dot, big, mode="softmax")
    pred, _ = ops.knn_vote(dev(idx, torch.int32), dev(dot), dev(big, torch.int32))
    assert np.array_equal(pred.cpu().numpy(), want)


def test_knn_accuracy_end_to_end(ops):
    from scd_amd import knn
    case = kc.blob_case("v500")
    raw, y, k = case["raw"], case["labels"], case["k"]
    idx, sim, info = knn.knn_graph(dev(raw), k)
    want_idx, want_dot = kc.knn_f64(case["q"], case["x"], k, 0)                             # case rows = finch_cases.unit_rows(raw)
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(sim.cpu().numpy(), want_dot)
    for weights in ("softmax", "uniform"):
        want_pred, _ = kc.vote_f64(want_idx, want_dot, y, mode=weights, temperature=0.07)
        pred = knn.knn_classify(raw, y, k=k, weights=weights)
        assert np.array_equal(pred.cpu().numpy(), want_pred)
        acc = knn.knn_accuracy(raw, y, k=k, weights=weights)
        assert acc == int((want_pred == y).sum()) / len(y) and 0.5 < acc < 1.0
    # held-out queries: nothing excluded
    tr, te = np.arange(100, 500), np.arange(0, 100)
    u = fc.unit_rows(raw)
    q_idx, q_dot = kc.knn_f64(u[te], u[tr], k, -1)
    want_pred, _ = kc.vote_f64(q_idx, q_dot, y[tr], mode="softmax", temperature=0.07)
    assert np.array_equal(knn.knn_classify(raw[tr], y[tr], raw[te], k=k).cpu().numpy(), want_pred)
    assert knn.knn_accuracy(raw[tr], y[tr], raw[te], y[te], k=k) == int((want_pred == y[te]).sum()) / len(te)


def test_score_features_ranks_the_better_tower(tmp_path):
    import score_features as sf
    from oracle import synth
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "extracted_features"))
    mask = np.zeros(700, dtype=bool)
    mask[:500] = True
    for name, d, noise in (("dino_vit", 48, 1.0), ("clip", 32, 3.0)):
        x, y, _ = synth.clustered_features(700, d, 6, seed=60, center_seed=160, noise=noise)
        torch.save(dict(all_feats=x, mask_lab=mask, targets=y), os.path.join(root, "extracted_features", f"{name}_toy_all.pt"))
    out = sf.main(["--root_dir", root, "--dataset_name", "toy", "--feat_models", "clip", "dino_vit", "--k", "10"])
    with open(os.path.join(root, "cluster", "knn_score_toy.json")) as fh:
        js = json.load(fh)
    assert js["towers"].keys() == {"clip", "dino_vit"} and js["best"] == "dino_vit" == out["best"]
    assert js["towers"]["dino_vit"]["acc"] > js["towers"]["clip"]["acc"] > 1.0 / 6
    t = js["towers"]["clip"]
    assert (t["N"], t["D"], len(t["info"])) == (500, 32, 4) and t["cache"].endswith("clip_toy_all.pt")
    assert js["args"]["k"] == 10 and js["args"]["temperature"] == 0.07 and js["args"]["weights"] == "softmax"


# ------------------------------------------------------------------------------------------------- limits
def test_workspace_at_full_size(ops):
    L = ops._L()
    nb = L.scd_knn_ws_bytes(126976, 126976, 768, 20)
    print("scd_knn workspace at 126,976 x 768, k = 20: %.1f MB (k = 64: %.1f MB); scd_first_neighbor: %.1f MB"
          % (nb / 1e6, L.scd_knn_ws_bytes(126976, 126976, 768, 64) / 1e6, L.scd_first_neighbor_ws_bytes(126976, 768) / 1e6))
    assert 0 < nb <= 2 * GIB and 0 < L.scd_knn_ws_bytes(126976, 126976, 768, 64) <= 2 * GIB
    assert L.scd_knn_ws_bytes(10, 10, 1025, 1) == 0 and L.scd_knn_ws_bytes(10, 10, 8, 65) == 0 and L.scd_knn_ws_bytes(10, 1, 8, 1) == 0


def test_limits_are_refused(ops):
    from scd_amd._lib import ScdError, SCD_EINVAL
    x = dev(kc._rand(70, 40, 8))

    def refused(fn):
        with pytest.raises(ScdError) as ei:
            fn()
        assert ei.value.code == SCD_EINVAL

    refused(lambda: ops.knn(x, x, 0, 0))
    refused(lambda: ops.knn(x, x, 65, 0))
    refused(lambda: ops.knn(x[:20], x[:20], 20, 0))             # 19 admissible columns
    ops.knn(x[:20], x[:20], 20, -1)                             # 20 without the exclusion
    refused(lambda: ops.knn(x[:20], x[:20], 21, -1))
    refused(lambda: ops.knn(x, x, 3, 1))                        # self_base + m beyond n
    refused(lambda: ops.knn(x, x, 3, -2))
    refused(lambda: ops.knn(x[:1], x[:1], 1, -1))               # n = 1
    wide = dev(kc._rand(71, 4, 1025))
    refused(lambda: ops.knn(wide, wide, 1, 0))
    # the C calls themselves: null pointers, a short and a misaligned workspace
    L, h, st = ops._L(), ops.handle(), ops.stream_ptr()
    idx = torch.empty((40, 3), dtype=torch.int32, device="cuda")
    dot = torch.empty((40, 3), dtype=torch.float64, device="cuda")
    info = torch.empty(4, dtype=torch.int32, device="cuda")
    nb = L.scd_knn_ws_bytes(40, 40, 8, 3)
    ws = torch.empty(nb + 16, dtype=torch.uint8, device="cuda")
    p = ops.ptr
    good = [h, p(x), 40, p(x), 40, 8, 3, 0, p(idx), p(dot), p(info), p(ws), nb, st]
    assert L.scd_knn(*good) == 0
    for at in (0, 1, 3, 8, 9, 10, 11):
        bad = list(good)
        bad[at] = None
        assert L.scd_knn(*bad) == SCD_EINVAL
    short = list(good)
    short[12] = nb - 1
    assert L.scd_knn(*short) == SCD_EINVAL
    odd = list(good)
    odd[11] = C.c_void_p(ws.data_ptr() + 8)
    assert L.scd_knn(*odd) == SCD_EINVAL
    labels = torch.zeros(40, dtype=torch.int32, device="cuda")
    pred = torch.empty(40, dtype=torch.int32, device="cuda")
    score = torch.empty(40, dtype=torch.float64, device="cuda")
    vgood = [h, p(idx), p(dot), 40, 3, 3, p(labels), 40, 1, 0.07, p(pred), p(score), st]
    assert L.scd_knn_vote(*vgood) == 0
    for at in (0, 1, 2, 6, 10, 11):
        bad = list(vgood)
        bad[at] = None
        assert L.scd_knn_vote(*bad) == SCD_EINVAL
    for at, val in ((5, 0), (5, 4), (8, 2), (9, 0.0), (9, -1.0)):
        bad = list(vgood)
        bad[at] = val
        assert L.scd_knn_vote(*bad) == SCD_EINVAL
    torch.cuda.synchronize()
