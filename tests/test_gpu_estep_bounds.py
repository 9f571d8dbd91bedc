"""The E-step filters' a-priori error bounds on adversarial inputs (tests/estep_cases.py): scd_kmeans_estep on every filter path and the
seeding filter (scd_kpp_update_filter) against the float64 oracle, on EVERY row - the cases lie on an exact grid, so the float64
difference-form argmin (ties to the lowest index) is the one right answer and there is no tolerance band.

Asserted per case: labels equal ko.estep's on all rows; rowdist bits equal the oracle's float32 minimum distance; the same labels and the
same refined count with the refine in the filter kernel's tail (expect_few); 0 < refined < n where the CPU model of
test_estep_cases_sensitivity.py says both outcomes occur; tie rows carry the lower index.  Paths are chosen by shape
(estep_cases.path); the split last round of estep_rb_kernel needs n > 65,536 and Kp >= 512: test_estep_rb_split_last_round_ladder, and
test_estep_rb_split_last_round_far_centre for estep_rb_merge_kernel's branch for a centre outside the filters' range.

Refined rows per family, summed over the family's cases: the CPU model's prediction (test_estep_cases_sensitivity.py, whose
`test_model_counts_are_the_recorded_ones` pins the sums) and what an MI355X returned - equal in every single case:
  family          cases    rows    model   device
  ladder             11    6859     6168     6168
  long_centres       13    6679     3584     3584
  subnormal_tie       6    2732     2724     2724
  same_sign           4    2240     1120     1120
  outlier_scale      16    8445     8445     8445     (the bound is far above one grid step^2 there: every row is re-evaluated)
  offset              7    3706     3485     3485
  degenerate         10    3758     1606     1606
  outside_box        12    4838     4838     4838     (a centre outside the filters' range: every row to the exact refine)
The Lloyd path (the default C loop, all restarts in lock-step): test_lloyd_paths_on_ladder_and_long_centres, at
D = 512, K = 40, R = 4 and at D = 448, K = 130, R = 4 (Dp = 512, Kp = 256: estep_rb_kernel).
"""
import numpy as np
import pytest
import torch

import estep_cases as ec
from oracle import kmeans_oracle as ko
from test_estep_cases_sensitivity import both_sides, check_labels, oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device; they must not be skipped on the GPU box"
    from scd_amd import ops as o
    return o


def dev(x):
    return torch.as_tensor(x).cuda()


def _run(ops, case):
    data = ops.KMeansData(dev(case.x))
    c = dev(case.c)
    lab, ref = data.estep(c, return_refined=True)
    refined = int(ref.item())
    print("%s %s: refined %d of %d" % (case.name, case.path, refined, case.x.shape[0]))
    check_labels(case, lab.cpu().numpy(), refined, both_sides(case))
    olab, omind = oracle(case)
    rd = data.rowdist(c, lab).cpu().numpy()
    assert np.array_equal(rd.view(np.uint32), omind.view(np.uint32))
    lab2, ref2 = data.estep(c, return_refined=True, expect_few=True)
    assert torch.equal(lab, lab2) and int(ref2.item()) == refined
    return refined


@pytest.mark.parametrize("case", ec.estep_cases(), ids=lambda c: c.name)
def test_estep_labels_equal_float64_on_every_row(ops, case):
    _run(ops, case)


@pytest.mark.parametrize("case", ec.outside_box_cases(), ids=lambda c: c.name)
def test_estep_outside_box_centres(ops, case):
    """Centres far outside the data box, among them centres whose c' overflows fp16 and centres whose ||c'||^2 / 8 does: the call succeeds
    and every row has the oracle's label.  A live centre outside the filters' range sends every row to the exact refine: refined == n."""
    assert _run(ops, case) == case.x.shape[0]


def test_estep_rb_split_last_round_ladder(ops):
    """The ladder family at the smaller shape of test_estep_rb_split_last_round (n = 75,700, K = 1000: 40 row blocks of the partial last
    round split in four, merged and decided by estep_rb_merge_kernel): every row equals the exact argmin."""
    case = ec.ladder(75700, 512, 1000, seed=11)
    assert case.path == "rb"
    lab, ref = ops.KMeansData(dev(case.x)).estep(dev(case.c), return_refined=True)
    olab, _, _ = ko.estep(case.x, case.c)
    assert np.array_equal(lab.cpu().numpy().astype(np.int64), olab)
    assert 0 < int(ref.item()) < 75700


def test_estep_rb_split_last_round_far_centre(ops):
    """A live centre outside the filters' range on the split last round: estep_rb_merge_kernel (rows 65,536 .. 65,699: one row block,
    two parts of 8 units at Kp = 512) finds the marked centre and sends its rows to the all-centres refine like estep_rb_kernel does
    for the rows before them.  The ladder family with one centre of the second part moved 2^17 grid units out in one coordinate
    (||c'||^2 ~ 4e6 > 300 Dp; still on the grid): every row equals the exact argmin, refined == n."""
    case = ec.ladder(65700, 512, 385, seed=12)
    assert case.path == "rb"
    c = case.c.copy()
    c[300, 5] = -128.0
    lab, ref = ops.KMeansData(dev(case.x)).estep(dev(c), return_refined=True)
    olab, _, _ = ko.estep(case.x, c)
    assert np.array_equal(lab.cpu().numpy().astype(np.int64), olab)
    assert int(ref.item()) == 65700


class _MarginOracle(ko.K_Means):
    """ko.K_Means that records the smallest relative margin any E-step of the fit saw: (second - best distance) / (||x||^2 + max ||c||^2)."""
    worst = np.inf

    def assign(self, x, centers):
        lab, inertia = super().assign(x, centers)
        if not np.isnan(np.asarray(centers, dtype=np.float64)).any():
            x64, c64 = np.asarray(x, dtype=np.float64), np.unique(np.asarray(centers, dtype=np.float64), axis=0)
            # (bit-identical centres - a row drawn twice by the seeding - tie in every summation order: the lower index, here and there)
            xn, cn = (x64 * x64).sum(1), (c64 * c64).sum(1)
            # the float64 GEMM form: within ~D 2^-52 (||x||^2 + ||c||^2) ~ 1e-13 of the difference form, relative to the denominator below
            two = np.partition(xn[:, None] + cn[None, :] - 2.0 * (x64 @ c64.T), 1, axis=1)[:, :2]
            rel = (two[:, 1] - two[:, 0]) / (xn + cn.max())
            self.worst = min(self.worst, float(rel.min()))
        return lab, inertia


def lloyd_data(n, d, k, far_labelled, scatter=24):
    """ladder + long_centres rows (fp16-exact: |integer| <= 2,048 at unit 2^-10), shuffled.  far_labelled: plus labelled rows of two
    classes 64 box widths away in coordinate 0, so that the classes' centres are live centres OUTSIDE the range of the filters.
    scatter: the ladder rows' random offset from their centre in the coordinates that carry no ladder (the ladder's margins
    -4 t g |J| do not depend on it).  The first E-step of a fit sees centres that are ROWS, so its squared distances are integers (in
    grid units): with +-24 they spread over ~7e3 values round 1.8e5, and among the ~30 seeds that K = 130 puts into each group of 250
    ladder rows some row finds its two nearest seeds at the SAME integer - an exact tie between distinct centres, where float64 has no
    margin.  +-200 spreads them over ~4e5 values (the chance of one such tie in a fit is a few per cent; the test asserts there is none)."""
    a, b = ec.ladder(n // 2, d, k, seed=21, W=scatter), ec.long_centres(n - n // 2, d, k, seed=22)
    x = np.concatenate([a.x, b.x])
    x = x[np.random.RandomState(23).permutation(len(x))]
    assert np.array_equal(x.astype(np.float16).astype(np.float32), x)
    if not far_labelled:
        return x, None, None
    lab_x = x[:40].copy()
    lab_x[:20, 0], lab_x[20:, 0] = 60.0, -60.0
    assert np.array_equal(lab_x.astype(np.float16).astype(np.float32), lab_x)
    return x[40:], lab_x, np.repeat(np.arange(2), 20)


@pytest.mark.parametrize("n,d,k,R,far_labelled,scatter", [(2000, 512, 40, 4, False, 24), (2000, 512, 40, 4, True, 24),
                                                          (2000, 448, 130, 4, False, 200)])
def test_lloyd_paths_on_ladder_and_long_centres(ops, n, d, k, R, far_labelled, scatter):
    """One KMeansEngine fit of a few iterations on ladder + long_centres rows through the default C loop (the restarts in lock-step):
    labels, centres and inertia equal ko.K_Means.  Means leave the grid, so the
    oracle's float64 is order-dependent here: the oracle records the smallest relative margin of all its E-steps, and the test asserts it
    is far above float64 round-off (D 2^-52 ~ 1e-13).  D = 448, K = 130 is Dp = 512, Kp = 256: estep_rb_kernel (D = 512, K = 40: the
    streaming filter).  far_labelled: two labelled classes whose centres lie outside the filters' range - every E-step of that fit sends
    all rows to the exact refine."""
    from scd_amd.kmeans import KMeansEngine
    x, lx, ly = lloyd_data(n, d, k, far_labelled, scatter)
    okm = _MarginOracle(k=k, tolerance=1e-4, max_iterations=4, n_init=R, random_state=6)
    if far_labelled:
        okm.fit_mix(x, lx, ly)
    else:
        okm.fit(x)
    print("smallest relative margin of the oracle's E-steps: %.3e" % okm.worst)
    assert okm.worst > 1e-10
    km = KMeansEngine(k=k, tolerance=1e-4, max_iterations=4, n_init=R, random_state=6)
    if far_labelled:
        km.fit_mix(dev(x), dev(lx), dev(ly))
    else:
        km.fit(dev(x))
    assert km.stats.get("lockstep_fits", 0) == 1
    assert np.array_equal(km.labels_.cpu().numpy(), okm.labels_)
    assert np.array_equal(km.cluster_centers_.cpu().numpy(), okm.cluster_centers_, equal_nan=True)
    assert float(km.inertia_) == float(okm.inertia_)


def _seed_cases():
    return [ec.ladder(700, 256, 129, seed=3), ec.long_centres(700, 512, 129, seed=4), ec.same_sign(700, 768, 128, seed=5),
            ec.degenerate("repeated", n=333, d=128, k=8), ec.degenerate("rows_as_centres", n=333, d=128, k=8)]


@pytest.mark.parametrize("R", [1, 4, 10])
@pytest.mark.parametrize("ci", range(5))
def test_seeding_filter_leaves_the_oracle_bits(ops, ci, R):
    """UpdateFilter.update (muf_filter_kernel + muf_exact_kernel) round after round leaves float32(ko.pairwise_distance64(x, c_new)),
    folded by minimum, in d2 - for centres that are rows, centres that are not rows, and one centre at a corner of the data box."""
    case = _seed_cases()[ci]
    x = case.x
    n, d = x.shape
    assert np.array_equal(x.astype(np.float16).astype(np.float32), x) and ops.UpdateFilter.serves(n, d, R)
    xt = dev(x)
    x16 = ops.f16_exact(xt)
    assert x16 is not None
    uf = ops.UpdateFilter(x16)
    rs = np.random.RandomState(n + R)
    d2 = torch.full((R, n), float("inf"), dtype=torch.float32, device="cuda")
    want = np.full((R, n), np.inf, dtype=np.float32)
    cfin = case.c[np.isfinite(case.c).all(axis=1)]
    for t in range(6):
        if t % 3 == 0:
            cn = x[rs.randint(0, n, size=R)]                               # rows
        elif t % 3 == 1:
            cn = cfin[rs.randint(0, len(cfin), size=R)]                    # the case's centres: not rows
        else:
            cn = x[rs.randint(0, n, size=R)].copy()
            cn[0] = np.abs(x).max() * np.where(rs.rand(d) < 0.5, -1.0, 1.0).astype(np.float32)      # a corner of the data box
        cn = np.ascontiguousarray(cn, dtype=np.float32)
        uf.update(dev(cn).contiguous(), d2)
        for r in range(R):
            want[r] = np.minimum(want[r], ko.pairwise_distance64(x, cn[r:r + 1])[:, 0].astype(np.float32))
        assert np.array_equal(d2.cpu().numpy().view(np.uint32), want.view(np.uint32)), (case.name, t)
