"""GPU checks of scd_tsne_calibrate / scd_tsne_gradient / scd_tsne_update (scd_amd/csrc/tsne.hip), scd_amd.tsne, save_tsne and
plot_features.py against the float64 restatement of tests/tsne_cases.py (itself checked against scipy and scikit-learn on the CPU:
tests/test_tsne_host.py).  docs/design/tsne.md has the definitions and the derivation of the repulsion kernel's bound."""
import json
import os

import numpy as np
import pytest
import torch

import tsne_cases as tc

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    from scd_amd import ops as o
    return o


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def dev_csr(P):
    return dev(P[0], torch.int64), dev(P[1], torch.int32), dev(P[2], torch.float64)


# ------------------------------------------------------------------------------------------------- 5. calibration
@pytest.mark.parametrize("k", [5, 60, 64])
def test_calibrate_against_restatement(ops, k):
    dist2, perplexity = tc.calibration_case(k)
    want_p, want_beta, unreached = tc.calibrate_f64(dist2, perplexity)
    p, beta, info = ops.tsne_calibrate(dev(dist2), perplexity)
    p2, beta2, info2 = ops.tsne_calibrate(dev(dist2), perplexity)
    assert torch.equal(p, p2) and torch.equal(beta, beta2) and torch.equal(info, info2)                 # the same bits
    p, beta, info = p.cpu().numpy(), beta.cpu().numpy(), info.cpu().numpy()
    # relative 1e-10; below 1e-300 a float64 has no ten digits to compare
    err = np.abs(p - want_p) - 1e-10 * want_p
    print("calibrate k = %d: largest relative difference %.3e, beta in [%.3g, %.3g], unreachable rows %d"
          % (k, np.max(np.abs(p - want_p)[want_p > 1e-300] / want_p[want_p > 1e-300]), beta.min(), beta.max(), info[0]))
    assert (err <= 1e-300).all()
    assert np.allclose(p.sum(1), 1.0, rtol=1e-13, atol=0)
    assert info[0] == int(unreached.sum()) == 2 and info[1] == 0                                        # the tied rows are reported
    ok = ~unreached
    assert np.allclose(beta[ok], want_beta[ok], rtol=1e-10, atol=0) and beta[4:20].min() > 1e4


def test_calibrate_limits(ops):
    from scd_amd._lib import ScdError, SCD_EINVAL
    d = dev(np.full((10, 6), 0.5))
    for perplexity in (1.0, 6.0, 0.0, float("nan")):
        with pytest.raises(ScdError) as ei:
            ops.tsne_calibrate(d, perplexity)
        assert ei.value.code == SCD_EINVAL
    with pytest.raises(ScdError):
        ops.tsne_calibrate(dev(np.full((10, 65), 0.5)), 20.0)
    bad = np.full((10, 6), 0.5)
    bad[3, 2], bad[7, 0] = np.nan, -1.0
    p, beta, info = ops.tsne_calibrate(dev(bad), 2.0)
    assert info.cpu().tolist() == [8, 2] and torch.isfinite(p).all() and bool(torch.isnan(beta[3])) and abs(float(p[3].sum()) - 1.0) < 1e-15


# ------------------------------------------------------------------------------------------------- 6. joint affinities
JOINT = {"n4": (lambda: tc.blob_rows(4, 8, 2, 77)[0], 2.0), "n65": (lambda: tc.blob_rows(65, 16, 3, 78)[0], 30.0),
         "hub1000": (tc.hub_rows, 5.0)}


@pytest.mark.parametrize("name", list(JOINT))
def test_joint_affinities_against_restatement(name):
    from scd_amd import tsne
    make, perplexity = JOINT[name]
    x = make()
    want = tc.affinities_f64(x, perplexity)
    indptr, indices, values, info = tsne.joint_affinities(x, perplexity)
    again = tsne.joint_affinities(x, perplexity)
    assert indptr.dtype == torch.int64 and indices.dtype == torch.int32 and values.dtype == torch.float64
    assert torch.equal(values, again[2]) and torch.equal(indices, again[1])                             # the same bits
    assert np.array_equal(indptr.cpu().numpy(), want[0]) and np.array_equal(indices.cpu().numpy(), want[1])      # the structure is EQUAL
    assert np.allclose(values.cpu().numpy(), want[2], rtol=1e-12, atol=0)
    assert info["k"] == tc.neighbours(x.shape[0], perplexity) and info["untied"] == want[3] and info["bad_rows"] == 0
    if name == "hub1000":
        assert int(indptr[1] - indptr[0]) >= 500                                                        # the long reverse list
    if name == "n65":
        assert info["k"] == 64


def test_two_rows_have_no_admissible_perplexity():
    from scd_amd import tsne
    with pytest.raises(ValueError):
        tsne.joint_affinities(tc.blob_rows(2, 8, 2, 77)[0], 2.0)                                        # k = n - 1 = 1: (1, k) is empty


# ------------------------------------------------------------------------------------------------- 7. the gradient
def sizes(ops):
    R, C = ops._L().scd_tsne_row_tile(), ops._L().scd_tsne_col_chunk()
    assert (R, C) == (1024, 1024)
    return sorted({2, R - 1, R, R + 1, C + 1, 3001})


_REF, _P = {}, {}


def reference(n, state):
    """The float64 sums at the float32 state, computed once per case."""
    if (n, state) not in _REF:
        Y = tc.state(state, n)
        if n not in _P:
            _P[n] = tc.sparse_p(n, 11)
        P = _P[n]
        _REF[(n, state)] = (Y, P) + tc.repulsion_f64(Y) + tc.attraction_f64(Y, P)
    return _REF[(n, state)]


@pytest.mark.parametrize("n", [2, 1023, 1024, 1025, 3001])
def test_gradient_against_restatement(ops, n):
    assert n in sizes(ops)
    for state in tc.STATES:
        Y, P, F, z, MF, A, klp, psum, MA = reference(n, state)
        a = 12.0 if state == "initial" else 1.0
        y, (indptr, indices, values) = dev(Y), dev_csr(P)
        # the all-pairs sums alone: an empty P leaves grad = -4 F / Z
        g0, z0, kl0, info0 = ops.tsne_gradient(y, torch.zeros(n + 1, dtype=torch.int64, device="cuda"), indices[:0], values[:0], 1.0)
        Zd = float(z0.item())
        Fd = -g0.cpu().numpy() * Zd / 4.0
        Z = float(z.sum())
        eF, eZ = np.abs(Fd - F), abs(Zd - Z)
        with np.errstate(divide="ignore", invalid="ignore"):
            used = np.nanmax(np.where(MF > 0, eF / (U * MF), 0.0))
        print("gradient n = %4d %-10s: force error at most %.2f x 2^-24 M_i, Z error %.2f x 2^-24 Z (bound %d)" % (n, state, used, eZ / (U * Z), tc.C_BOUND))
        assert (eF <= tc.C_BOUND * U * MF).all() and eZ <= tc.C_BOUND * U * Z
        assert info0.cpu().tolist() == [0, 0] and float(kl0.item()) == 0.0
        if state == "coincident":
            assert Zd == n * (n - 1) and not Fd.any()
        # the whole gradient: float64 attraction and KL on top of the device's own all-pairs sums
        g, z1, kl, info = ops.tsne_gradient(y, indptr, indices, values, a)
        assert float(z1.item()) == Zd and info.cpu().tolist() == [0, 0]
        want = 4.0 * (a * A - Fd / Zd)
        tol = 1e-12 * 4.0 * (a * MA + np.abs(Fd) / Zd)
        assert (np.abs(g.cpu().numpy() - want) <= tol).all()
        want_kl = klp + np.log(Zd) * psum
        assert abs(float(kl.item()) - want_kl) <= 1e-12 * (abs(klp) + abs(np.log(Zd) * psum))
        # float64 pairs: the restatement itself
        ge, ze, kle, _ = ops.tsne_gradient(y, indptr, indices, values, a, exact_pairs=True)
        assert abs(float(ze.item()) - Z) <= 1e-12 * Z
        assert (np.abs(ge.cpu().numpy() - 4.0 * (a * A - F / Z)) <= 1e-11 * 4.0 * (a * MA + MF / Z)).all()
        assert abs(float(kle.item()) - (klp + np.log(Z) * psum)) <= 1e-12 * (abs(klp) + abs(np.log(Z) * psum))


TORCH_RTOL = 1e-13              # tests/test_tsne_host.py: repulsion_f64_torch against repulsion_f64


def large_reference(name, state):
    """As reference() for a case of tc.LARGE: the float64 sums are tsne_cases.repulsion_f64_torch on the device (plain torch float64
    operations, no code of scd_amd), P is banded_p; computed once per case."""
    n = tc.LARGE[name]
    if (n, state) not in _REF:
        Y = tc.state(state, n)
        if n not in _P:
            _P[n] = tc.banded_p(n, seed=11)
        P = _P[n]
        _REF[(n, state)] = (Y, P) + tc.repulsion_f64_torch(Y, device="cuda") + tc.attraction_f64(Y, P)
    return _REF[(n, state)]


def assert_hub_row(g, Fd, Zd, a, A, MA, P, what):
    """Row 0 of banded_p alone: its attraction, taken out of the gradient with the device's own all-pairs sums, against attraction_f64."""
    entries = int(P[0][1] - P[0][0])
    got = g[0] / 4.0 + Fd[0] / Zd
    err = np.abs(got - a * A[0])
    tol = 1e-12 * (a * MA[0] + np.abs(Fd[0]) / Zd)
    share = float(np.max(err[tol > 0] / tol[tol > 0])) if (tol > 0).any() else 0.0
    print("%s: hub row 0 has %d entries (%d trips of the lane loop), attraction error %.3g of its bound" % (what, entries, -(-entries // 64), share))
    assert entries > 192 and (err <= tol).all()


@pytest.mark.parametrize("name", list(tc.LARGE))
def test_gradient_ranges_of_several_chunks(ops, name):
    """More than 32 chunks: every block of tsne_repulse_kernel walks a range of several chunks (the second trip of the chunk loop, `check`
    changing between the chunks of a block, the clamp of the last range, the range count after the 'no empty range' step, a last chunk
    of ONE column).  The same bound as test_gradient_against_restatement: its derivation does not depend on n."""
    n = tc.LARGE[name]
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    triple = tc.ranges(n, n_cu)
    print("gradient %s: n = %d on %d compute units: %d ranges of %d chunks, %d in the last" % ((name, n, n_cu) + triple))
    assert triple[1] >= 2
    rows = tc.range_rows(n)
    for state in tc.LARGE_STATES[name]:
        Y, P, F, z, MF, A, klp, psum, MA = large_reference(name, state)
        # the reference itself, on the rows of the host test's sensitivity check, against the numpy restatement
        Fn, zn, MFn = tc.repulsion_f64(Y, rows=rows)
        assert (np.abs(F[rows] - Fn) <= TORCH_RTOL * MFn).all() and (np.abs(MF[rows] - MFn) <= TORCH_RTOL * MFn).all()
        assert (np.abs(z[rows] - zn) <= TORCH_RTOL * zn).all()
        a = 12.0 if state == "initial" else 1.0
        y, (indptr, indices, values) = dev(Y), dev_csr(P)
        g0, z0, kl0, info0 = ops.tsne_gradient(y, torch.zeros(n + 1, dtype=torch.int64, device="cuda"), indices[:0], values[:0], 1.0)
        Zd = float(z0.item())
        Fd = -g0.cpu().numpy() * Zd / 4.0
        Z = float(z.sum())
        eF, eZ = np.abs(Fd - F), abs(Zd - Z)
        with np.errstate(divide="ignore", invalid="ignore"):
            used = np.nanmax(np.where(MF > 0, eF / (U * MF), 0.0))
        print("gradient %s %-10s: force error at most %.2f x 2^-24 M_i, Z error %.2f x 2^-24 Z (bound %d)" % (name, state, used, eZ / (U * Z), tc.C_BOUND))
        assert (eF <= tc.C_BOUND * U * MF).all() and eZ <= tc.C_BOUND * U * Z
        assert info0.cpu().tolist() == [0, 0] and float(kl0.item()) == 0.0
        if state == "coincident":                               # exact: a skipped or repeated chunk shows as a whole number
            assert Zd == n * (n - 1) and not Fd.any()
        g, z1, kl, info = ops.tsne_gradient(y, indptr, indices, values, a)
        assert float(z1.item()) == Zd and info.cpu().tolist() == [0, 0]
        g = g.cpu().numpy()
        want = 4.0 * (a * A - Fd / Zd)
        tol = 1e-12 * 4.0 * (a * MA + np.abs(Fd) / Zd)
        assert (np.abs(g - want) <= tol).all()
        assert_hub_row(g, Fd, Zd, a, A, MA, P, "%s %s" % (name, state))
        want_kl = klp + np.log(Zd) * psum
        assert abs(float(kl.item()) - want_kl) <= 1e-12 * (abs(klp) + abs(np.log(Zd) * psum))
        ge, ze, kle, _ = ops.tsne_gradient(y, indptr, indices, values, a, exact_pairs=True)
        assert abs(float(ze.item()) - Z) <= 1e-12 * Z
        assert (np.abs(ge.cpu().numpy() - 4.0 * (a * A - F / Z)) <= 1e-11 * 4.0 * (a * MA + MF / Z)).all()
        assert abs(float(kle.item()) - (klp + np.log(Z) * psum)) <= 1e-12 * (abs(klp) + abs(np.log(Z) * psum))
        if state == "coincident":
            assert float(ze.item()) == n * (n - 1)


def test_hub_row_attraction(ops):
    """The attract kernel's lane loop (e += 64) on a row of more than 192 entries, at the largest size of the numpy reference."""
    n = 3001
    Y, P = tc.state("converged", n), tc.banded_p(n, seed=11)
    A, klp, psum, MA = tc.attraction_f64(Y, P)
    y, (indptr, indices, values) = dev(Y), dev_csr(P)
    assert (MA[0] > 0).all()
    for a in (1.0, 12.0):
        g0, z0, _, _ = ops.tsne_gradient(y, torch.zeros(n + 1, dtype=torch.int64, device="cuda"), indices[:0], values[:0], 1.0)
        g, z1, kl, info = ops.tsne_gradient(y, indptr, indices, values, a)
        Zd = float(z0.item())
        Fd = -g0.cpu().numpy() * Zd / 4.0
        assert float(z1.item()) == Zd and info.cpu().tolist() == [0, 0]
        assert_hub_row(g.cpu().numpy(), Fd, Zd, a, A, MA, P, "n = %d, exaggeration %g" % (n, a))
        assert abs(float(kl.item()) - (klp + np.log(Zd) * psum)) <= 1e-12 * (abs(klp) + abs(np.log(Zd) * psum))


def test_gradient_two_calls_same_bits(ops):
    for Y, P in (reference(3001, "converged")[:2], large_reference("c33", "converged")[:2]):
        y, (indptr, indices, values) = dev(Y), dev_csr(P)
        first = ops.tsne_gradient(y, indptr, indices, values, 12.0)
        second = ops.tsne_gradient(y, indptr, indices, values, 12.0)
        for u, v in zip(first, second):
            assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------------- 8. the update step
def test_update_equals_numpy(ops):
    """tsne.hip is compiled without contraction, so every operation of the step is the IEEE float64 operation numpy performs: the bound
    is zero ulps, and the float32 copy is the round-to-nearest of the master."""
    n = 1000
    r = np.random.RandomState(12)
    grad, y, vel = 1e-3 * r.randn(n, 2), 30.0 * r.randn(n, 2), r.randn(n, 2)
    gains = r.uniform(0.01, 3.0, size=(n, 2))
    vel[:50] = 0.0                                              # vel * grad == 0: the gain shrinks
    gains[50:100] = 0.0101                                      # 0.8 * 0.0101 falls below the floor
    grad[100:120] = 0.0
    y[120] = (1.0 + 2.0 ** -24, -(1.0 + 3 * 2.0 ** -25))         # a tie and a near-tie of the float32 rounding
    vel[120], grad[120] = 0.0, 0.0
    for momentum, lr in ((0.5, 125.0), (0.8, 50.0)):
        want_y, want_vel, want_gains, want_gg = tc.update_f64(grad, y, vel, gains, momentum, lr)
        d_y, d_vel, d_gains = dev(y), dev(vel), dev(gains)
        y32 = torch.empty((n, 2), dtype=torch.float32, device="cuda")
        gg = torch.empty((n, 2), dtype=torch.float64, device="cuda")
        ops.tsne_update(dev(grad), d_y, d_vel, d_gains, y32, momentum, lr, 0.01, gg_out=gg)
        assert np.array_equal(d_y.cpu().numpy(), want_y) and np.array_equal(d_vel.cpu().numpy(), want_vel)
        assert np.array_equal(d_gains.cpu().numpy(), want_gains) and np.array_equal(gg.cpu().numpy(), want_gg)
        assert np.array_equal(y32.cpu().numpy(), want_y.astype(np.float32))
        assert want_gains.min() == 0.01
    wrong = tc.update_f64(grad, y, vel, gains, 0.5, 125.0, mistake="gains_inverted")[0]
    assert not np.array_equal(wrong, tc.update_f64(grad, y, vel, gains, 0.5, 125.0)[0])


# ------------------------------------------------------------------------------------------------- 9. bad input is refused or flagged
def test_bad_csr_is_refused_or_flagged(ops):
    """The Python layer refuses wrong types and lengths; the kernel compares every indptr pair with nnz and every column with n BEFORE it
    reads through them (tsne_attract_kernel), skips what is out of range and counts the row."""
    from scd_amd import tsne
    from scd_amd._lib import ScdError, SCD_EINVAL
    n = 70
    Y, P = tc.state("converged", n), tc.sparse_p(n, 11)
    y, (indptr, indices, values) = dev(Y), dev_csr(P)
    for args in ((y.double(), indptr, indices, values), (y, indptr.int(), indices, values), (y, indptr, indices.long(), values),
                 (y, indptr, indices, values.float()), (y, indptr[:-1], indices, values), (y, indptr, indices[:-1], values)):
        with pytest.raises(ScdError) as ei:
            ops.tsne_gradient(*args)
        assert ei.value.code == SCD_EINVAL
    L, h, st, p = ops._L(), ops.handle(), ops.stream_ptr(), ops.ptr
    nnz = indices.numel()
    nb = L.scd_tsne_gradient_ws_bytes(n, nnz)
    ws = torch.empty(nb + 16, dtype=torch.uint8, device="cuda")
    grad = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    zk = torch.empty(2, dtype=torch.float64, device="cuda")
    info = torch.empty(2, dtype=torch.int32, device="cuda")
    good = [h, p(y), p(indptr), p(indices), p(values), n, nnz, 1.0, 0, p(grad), p(zk[:1]), p(zk[1:]), p(info), p(ws), nb, st]
    assert L.scd_tsne_gradient(*good) == 0
    for at, val in ((0, None), (1, None), (2, None), (3, None), (4, None), (9, None), (10, None), (12, None), (13, None), (5, 1), (6, -1), (7, 0.0),
                    (7, float("inf")), (8, 2), (14, nb - 1)):
        bad = list(good)
        bad[at] = val
        assert L.scd_tsne_gradient(*bad) == SCD_EINVAL, at
    # entries out of range: flagged, skipped, and the Python layer raises
    wrong = indices.clone()
    lo3, lo9 = int(indptr[3]), int(indptr[9])
    wrong[lo3], wrong[lo9] = -1, n
    ptr2 = indptr.clone()
    ptr2[41] = nnz + 5                                           # rows 40 and 41 get a pair outside 0 <= lo <= hi <= nnz
    g, z, kl, inf = ops.tsne_gradient(y, ptr2, wrong, values, 1.0)
    assert inf.cpu().tolist() == [4, 0] and torch.isfinite(g).all()
    with pytest.raises(ValueError):
        tsne.tsne_gradient(y, (ptr2, wrong, values))
    Ybad = Y.copy()
    Ybad[5, 0], Ybad[6, 1] = np.nan, 2.0 ** 61
    assert ops.tsne_gradient(dev(Ybad), indptr, indices, values, 1.0)[3].cpu().tolist() == [0, 2]


# ------------------------------------------------------------------------------------------------- 10. end to end
def test_fit_on_the_blob_case():
    """The device TSNE on the committed blob case (perplexity 20: P is scikit-learn's own) must do at least as well as scikit-learn's
    Barnes-Hut runs for seeds 0 .. 4, whose KL and trustworthiness tests/golden/tsne_blobs.npz records."""
    from scd_amd import tsne
    g = tc.golden()
    x, perplexity = g["rows"], float(g["perplexity"])
    sk_kl, sk_tr = g["sklearn_kl"], g["sklearn_trust"]
    t = tsne.TSNE(perplexity=perplexity, random_state=0)
    Y = t.fit_transform(x)
    assert Y.shape == (1500, 2) and Y.dtype == np.float32 and np.isfinite(Y).all() and t.n_iter_ <= 999
    P = tc.affinities_f64(x, perplexity)
    _, _, kl = tc.gradient_f64(Y, P)
    trust = tc.trustworthiness_f64(x, Y, 5)
    print("fit: KL %.4f (scikit-learn %.4f .. %.4f), trustworthiness %.4f (scikit-learn %.4f .. %.4f), %d iterations, info %r"
          % (kl, sk_kl.min(), sk_kl.max(), trust, sk_tr.min(), sk_tr.max(), t.n_iter_, t.info_))
    assert abs(t.kl_divergence_ - kl) <= 1e-9 * kl
    assert kl <= sk_kl.max() + (sk_kl.max() - sk_kl.min())
    assert trust >= sk_tr.min() - (sk_tr.max() - sk_tr.min())
    Y2 = tsne.TSNE(perplexity=perplexity, random_state=0).fit_transform(x)
    assert np.array_equal(Y, Y2)                                # two fits, the same bits


def test_first_iterations_follow_the_restatement():
    """Six iterations of the device optimiser (PCA start, learning rate 'auto', exaggeration, momentum, gains) against the float64
    restatement.  The early phase expands: a perturbation of the gradient grows from step to step, so the comparison must be short.  With
    every gradient of the restatement perturbed by 5e-6 relative (the size of the kernel's bound, 80 x 2^-24) the six-step state moves by
    at most 4.2e-5 of its extent over five seeds, by 7.8e-4 after ten steps; a learning rate of 60 for 50 moves it by 1.05, exaggeration
    11 for 12 by 0.34, the inverted gain rule by 4.4 (all on the CPU, in float64).  The bound is 1e-3."""
    from scd_amd import tsne
    x, _ = tc.blob_rows(300, 16, 4, 79)
    P = tc.affinities_f64(x, 10.0)[:3]
    y0 = tc.pca_init_f64(x)
    start = tsne.pca_init(dev(tc.fc.unit_rows(x))).cpu().numpy()
    assert np.abs(start - y0).max() <= 1e-9 * np.abs(y0).max()
    want = tc.descend_f64(P, y0.astype(np.float32), 6)
    t = tsne.TSNE(perplexity=10.0, max_iter=6)
    got = t.fit_transform(x)
    rel = np.abs(got - want).max() / np.abs(want).max()
    print("6 iterations: relative difference to the restatement %.3e" % rel)
    assert rel <= 1e-3 and t.learning_rate_ == 50.0 and t.n_iter_ == 5
    for wrong in (tc.descend_f64(P, y0.astype(np.float32), 6, mistake="gains_inverted"), tc.descend_f64(P, y0.astype(np.float32), 6, learning_rate=60.0),
                  tc.descend_f64(P, y0.astype(np.float32), 6, early_exaggeration=11.0, learning_rate=50.0)):
        assert np.abs(wrong - want).max() / np.abs(want).max() > 0.1


def test_random_start_is_seeded():
    from scd_amd import tsne
    x, _ = tc.blob_rows(300, 16, 4, 79)
    a = tsne.TSNE(perplexity=10.0, init='random', random_state=3, max_iter=100).fit_transform(x)
    b = tsne.TSNE(perplexity=10.0, init='random', random_state=3, max_iter=100).fit_transform(x)
    c = tsne.TSNE(perplexity=10.0, init='random', random_state=4, max_iter=100).fit_transform(x)
    assert np.isfinite(a).all() and np.array_equal(a, b) and not np.array_equal(a, c)


# ------------------------------------------------------------------------------------------------- 11. the user's side
def png_size(path):
    with open(path, "rb") as fh:
        head = fh.read(24)
    assert head[:8] == b"\x89PNG\r\n\x1a\n" and head[12:16] == b"IHDR"
    return int.from_bytes(head[16:20], "big"), int.from_bytes(head[20:24], "big")


def test_save_tsne_writes_a_png(tmp_path):
    pytest.importorskip("matplotlib")
    from scd_amd.local_utils.util import save_tsne, save_tsne_wcolor
    x, y = tc.blob_rows(200, 16, 4, 79)
    for fn, name in ((save_tsne, "a.png"), (save_tsne_wcolor, "b.png")):
        path = str(tmp_path / name)
        fn(x, y, path)
        w, h = png_size(path)
        assert 400 <= w <= 1200 and 300 <= h <= 800             # an 8 x 6 inch figure at 100 dpi, cropped to its content and legend


def test_plot_features_writes_its_files(tmp_path):
    pytest.importorskip("matplotlib")
    import plot_features as pf
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "extracted_features"))
    x, y = tc.blob_rows(260, 16, 4, 79)
    mask = np.zeros(260, dtype=bool)
    mask[:100] = True
    torch.save(dict(all_feats=x, mask_lab=mask, targets=y), os.path.join(root, "extracted_features", "dino_vit_toy_all.pt"))
    with open(os.path.join(root, "names.json"), "w") as fh:
        json.dump(["ant", "bee", "cat", "dog"], fh)
    out = pf.main(["--root_dir", root, "--dataset_name", "toy", "--feat_model", "dino_vit", "--perplexity", "10", "--class_names",
                   os.path.join(root, "names.json")])
    base = os.path.join(root, "cluster", "tsne_dino_vit_toy")
    assert png_size(base + ".png")[0] > 100
    Y = np.load(base + ".npy")
    assert Y.shape == (260, 2) and Y.dtype == np.float32 and np.isfinite(Y).all()
    with open(base + ".json") as fh:
        js = json.load(fh)
    assert js["args"]["perplexity"] == 10.0 and js["n_iter_"] == out["n_iter_"] and js["kl_divergence_"] > 0 and js["info"]["k"] == 30
