"""scd_silhouette (scd_amd/csrc/silhouette.hip) at the grid shapes real runs use, on inputs where the device arithmetic is exact
(tests/silhouette_cases.py, module docstring).

Lattice family: rows t_i * u with |u|^2 a perfect square, so every distance and every per-cluster sum is an integer below 2^24 in any
summation order; what is left are IEEE fp32 divisions, which numpy float32 repeats.  The device's samples must EQUAL the count-table
reference on every row: one to two cluster ranges (grid.y) at 65k / 131k rows, thirty-two ranges that mostly hold nothing, clusters
starting exactly on a range border, a one-block scan with several entries per thread, clusters of 65k rows, whole panels past the last
valid row on a workspace full of NaN bits, and the edges of d.  Sizes that depend on the CU count come from scd_silhouette_ranges.

General grid family: rows in general position whose dots, norms and dist^2 are exact in fp32; the samples must lie within the bound
derived from the square root's rounding and the fp32 summation, against float64.

tests/test_silhouette_host.py shows on the CPU that each of seven planted kernel mistakes changes one of these cases."""
import numpy as np
import pytest
import torch

import silhouette_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from scd_amd import ops as o
    return o


def run(ops, x, labels, k):
    s, mean, info = ops.silhouette(torch.as_tensor(x).cuda(), torch.as_tensor(np.asarray(labels, dtype=np.int32)).cuda(), k)
    return s.cpu().numpy(), float(mean.item()), [int(v) for v in info.cpu()]


def check_lattice(case, got, mean, info):
    labels, k = case["labels"], case["k"]
    valid = (labels >= 0) & (labels < k)
    want, _ = sc.lattice_reference(case)
    assert info == [int((~valid).sum()), int((np.bincount(labels[valid], minlength=k) > 0).sum())]
    assert got.dtype == want.dtype == np.float32
    bad = np.nonzero(got != want)[0]
    assert np.array_equal(got, want), (case["name"], "rows that differ: %d of %d" % (bad.size, got.size),
                                       [(int(i), float(got[i]), float(want[i])) for i in bad[:5]])
    assert abs(mean - got.astype(np.float64).mean()) <= 1e-12
    assert not got[~valid].any()


@pytest.mark.parametrize("name", [n for n in sc.LATTICE_NAMES if not n.startswith("valid_")])
def test_lattice_samples_are_bit_equal(ops, name):
    case = sc.lattice_case(name, ops.silhouette_ranges)
    ny = ops.silhouette_ranges(case["n"], case["k"])
    sizes = np.bincount(case["labels"][(case["labels"] >= 0) & (case["labels"] < case["k"])], minlength=case["k"])
    print("silhouette lattice %-22s n %6d d %4d k %4d ny %2d k*chunks %6d largest cluster %5d g %2d t < %d"
          % (name, case["n"], case["d"], case["k"], ny, case["k"] * -(-case["n"] // 1024), sizes.max(), case["g"], case["t"].max() + 1))
    if case["ny"] is not None:
        assert ny == case["ny"], (name, ny)
    check_lattice(case, *run(ops, case["x"], case["labels"], case["k"]))


def test_one_two_and_thirty_two_ranges_are_what_the_cases_run(ops):
    """The shapes of the one-range, two-range and 32-range cases, asked of the library: each case asserts its own count again."""
    n2, n1 = sc.smallest_n(2, ops.silhouette_ranges) + 37, sc.smallest_n(1, ops.silhouette_ranges) + 37
    assert n2 < n1
    assert [ops.silhouette_ranges(n2, 2), ops.silhouette_ranges(n2, 3), ops.silhouette_ranges(n1, 2), ops.silhouette_ranges(n1, 1000),
            ops.silhouette_ranges(515, 257)] == [2, 2, 1, 1, 32]
    assert ops.silhouette_ranges(1, 2) == 0 and ops.silhouette_ranges(100, 101) == 0 and ops.silhouette_ranges(100, 1) == 0


def call_abi(ops, case, ws):
    """scd_silhouette itself, on the caller's workspace."""
    x = torch.as_tensor(case["x"]).cuda()
    lab = torch.as_tensor(case["labels"].astype(np.int32)).cuda()
    n, d = x.shape
    ops._need_cuda(x)
    samples = torch.empty(n, dtype=torch.float32, device=x.device)
    mean = torch.empty(1, dtype=torch.float64, device=x.device)
    info = torch.empty(2, dtype=torch.int64, device=x.device)
    assert ws.numel() >= ops._L().scd_silhouette_ws_bytes(n, d, case["k"]) > 0
    ops.check(ops._L().scd_silhouette(ops.handle(), ops.ptr(x), ops.SCD_F16, ops.ptr(lab), n, d, case["k"], ops.ptr(samples), ops.ptr(mean),
                                      ops.ptr(info), ops.ptr(ws), ws.numel(), ops.stream_ptr()))
    return samples.cpu().numpy(), float(mean.item()), [int(v) for v in info.cpu()]


def poisoned(ops, case):
    """A workspace of 0xFF bytes: NaN as fp16 and as fp32, -1 as int32."""
    n, d = case["x"].shape
    return torch.full((int(ops._L().scd_silhouette_ws_bytes(n, d, case["k"])),), 0xFF, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("n_valid", sc.N_VALID)
def test_panels_past_the_last_valid_row_on_a_poisoned_workspace(ops, n_valid):
    """1,000 rows of which 127 / 128 / 129 / 400 carry a label inside [0, k): up to seven whole panels start past the last valid row,
    and nothing the kernels read may come from the workspace as it was found."""
    case = sc.lattice_case("valid_%d" % n_valid, ops.silhouette_ranges)
    assert case["n"] == 1000 and int(((case["labels"] >= 0) & (case["labels"] < case["k"])).sum()) == n_valid
    check_lattice(case, *call_abi(ops, case, poisoned(ops, case)))


def test_workspace_reused_for_a_smaller_label_set(ops):
    """400 valid rows, then 127 and 129 on the SAME workspace: the slots the larger set filled must not reach the smaller one."""
    big = sc.lattice_case("valid_400", ops.silhouette_ranges)
    ws = poisoned(ops, big)
    check_lattice(big, *call_abi(ops, big, ws))
    for v in (127, 129):
        small = sc.lattice_case("valid_%d" % v, ops.silhouette_ranges)
        check_lattice(small, *call_abi(ops, small, ws))


@pytest.mark.parametrize("name", sorted(sc.GRID_SHAPES))
def test_grid_samples_are_inside_the_derived_bound(ops, name):
    case = sc.grid_case(name)
    x, labels, k = case["x"], case["labels"], case["k"]
    want = sc.silhouette_f64(x, labels, k, dist=sc.grid_distances(x))
    lim = sc.grid_bound(labels, k)
    got, mean, info = run(ops, x, labels, k)
    err = np.abs(got.astype(np.float64) - want)
    print("silhouette grid %-14s n %5d d %4d k %4d ny %2d largest cluster %5d: max |err| %.3e, smallest bound %.3e, largest err / bound %.3f"
          % (name, case["n"], case["d"], k, ops.silhouette_ranges(case["n"], k), np.bincount(labels).max(), err.max(), lim.min(), (err / lim).max()))
    assert info == [0, int((np.bincount(labels, minlength=k) > 0).sum())]
    assert np.all(err <= lim), (name, float(err.max()), int((err > lim).sum()), int((err / lim).argmax()))
    assert abs(mean - got.astype(np.float64).mean()) <= 1e-12
