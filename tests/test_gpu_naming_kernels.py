"""The kernels that turn clusters into names against exact references, on a real MI355X: every case of tests/naming_cases.py through
scd_amd.ops.  The vote tests and the bit movers assert array_equal on integers / fp16 bits; l2norm_rows and prompt_pool are bit-equal
on exact-grid rows and inside a bound derived from their operation counts on random rows (naming_cases' docstring).

  vote_hist        Counter.most_common(m) incl. the -1 / 0 padding: slots on both sides of bit 15 (40,000 requested ids), ids 0 and
                   65,535, predictions that vote for nothing, names 0 / 2^24 - 1 counted and -1 / 2^24 dropped, ld > top_k, m around the
                   64-lane output loop, `known`, ties (first-seen decides), n * top_k = 1, and ONE case with n * top_k = 2^24 - 1 and a
                   count above 2^23; the refusals
  vote_table       counts / first against Counter / first position; NEVER in unseen cells; v around 256; skipped names and predictions;
                   n = 0; 20,000 adds into one cell; positions above 2^32; row shards combined by + / minimum; the refusals
  vote_table_topm  crafted tables: counts up to 2^31 - 1, positions that differ above bit 32, the winner in the last column, padding,
                   the zeroing side effect, two calls identical
  transpose_f16, gather_rows_f16, select_rows, mean2_f16, l2norm_rows, prompt_pool
"""
import numpy as np
import pytest
import torch

import naming_cases as nc

pytestmark = pytest.mark.gpu
F16, F32, F64 = np.float16, np.float32, np.float64


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device; they must not be skipped on the GPU box"
    from scd_amd import ops as o
    return o


@pytest.fixture(scope="module")
def ScdError():
    from scd_amd._lib import ScdError as e
    return e


def dev(x):
    return torch.as_tensor(x).cuda()


def host(t):
    return t.cpu().numpy()


def f16_dev(bits):
    """uint16 bit patterns (or an fp16 array) -> fp16 device tensor with exactly those bits."""
    return dev(np.ascontiguousarray(bits).view(np.int16)).view(torch.float16)


def bits(t):
    return host(t.contiguous().view(torch.int16)).view(np.uint16)


def run_hist(ops, c):
    keys, counts = ops.vote_hist(dev(c.idx), c.top_k, dev(c.preds), c.clusters, c.m, c.known)
    return host(keys), host(counts)


# ------------------------------------------------------------------------------------------------ vote_hist
@pytest.mark.parametrize("c", nc.hist_cases(), ids=lambda c: c.name)
def test_vote_hist_equals_counter(ops, c):
    assert not nc.check_hist(c, *run_hist(ops, c))


def test_vote_hist_top_bit_of_position_and_count(ops):
    """n * top_k = 2^24 - 1: positions with bit 23 set decide ties, one count is above 2^23."""
    c = nc.big_case()
    want = nc.big_want()
    got = run_hist(ops, c)
    print("heavy row: got", got[0][2].tolist(), got[1][2].tolist(), "late row: got", got[0][3].tolist(), got[1][3].tolist())
    assert not nc.check_pair(c.name, got, want)


def test_vote_hist_refusals(ops, ScdError):
    """Host-side refusals (no launch): n * top_k = 2^24, top_k > ld, m = 0, a cluster id of 65,536 or -1, 65,537 clusters."""
    idx, preds = torch.zeros((8, 5), dtype=torch.int64, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(ScdError):
        ops.vote_hist(torch.zeros((1 << 22, 4), dtype=torch.int64, device="cuda"), 4, torch.zeros(1 << 22, dtype=torch.int64, device="cuda"), [0], 3)
    with pytest.raises(ScdError):
        ops.vote_hist(idx, 6, preds, [0], 3)
    with pytest.raises(ScdError):
        ops.vote_hist(idx, 5, preds, [0], 0)
    with pytest.raises(ScdError):
        ops.vote_hist(idx, 5, preds, [0, nc.MAX_CLUSTER_ID], 3)
    with pytest.raises(ScdError):
        ops.vote_hist(idx, 5, preds, [-1, 0], 3)
    with pytest.raises(ScdError):
        ops.vote_hist(idx, 5, preds, list(range(nc.MAX_CLUSTER_ID)) + [0], 3)
    keys, counts = ops.vote_hist(idx, 5, preds, [nc.MAX_CLUSTER_ID - 1, 0], 2)           # the largest id is served
    assert host(keys).tolist() == [[-1, -1], [0, -1]] and host(counts).tolist() == [[0, 0], [40, 0]]


# ------------------------------------------------------------------------------------------------ vote_table
def run_table(ops, c, rows=slice(None), row_offset=None):
    counts, first = ops.vote_table(dev(c.idx[rows]), c.top_k, dev(c.preds[rows]), c.clusters, c.n_slots,
                                   c.row_offset if row_offset is None else row_offset, c.v)
    return counts, first


@pytest.mark.parametrize("c", nc.table_cases(), ids=lambda c: c.name)
def test_vote_table_equals_counter_and_first_position(ops, c):
    counts, first = run_table(ops, c)
    want = nc.table_want(c)
    assert not nc.check_pair(c.name, (host(counts), host(first)), want, ("counts", "first"))
    assert (host(first)[want[0] == 0] == nc.NEVER).all()
    # and through the top-m: Counter.most_common of the rows
    if c.idx.shape[0]:
        h = nc.counts_as_hist(c, 5)
        keys, cnt = ops.vote_table_topm(counts, first, 5)
        assert not nc.check_pair(c.name, (host(keys), host(cnt)), nc.hist_counter(h))


@pytest.mark.parametrize("case", nc.shard_cases(), ids=lambda x: x[0].name)
def test_vote_table_row_shards_combine(ops, case):
    c, cuts = case
    want = nc.table_want(c)
    whole = run_table(ops, c)
    assert not nc.check_pair(c.name, (host(whole[0]), host(whole[1])), want, ("counts", "first"))
    parts = [run_table(ops, c, slice(a, b), c.row_offset + a) for a, b in zip(cuts[:-1], cuts[1:])]
    for (a, b), p in zip(zip(cuts[:-1], cuts[1:]), parts):
        assert not nc.check_pair("%s[%d:%d]" % (c.name, a, b), (host(p[0]), host(p[1])),
                                 nc.table_want(c, slice(a, b), c.row_offset + a), ("counts", "first"))
    counts, first = parts[0][0].clone(), parts[0][1].clone()
    for p in parts[1:]:
        counts, first = counts + p[0], torch.minimum(first, p[1])
    assert torch.equal(counts, whole[0]) and torch.equal(first, whole[1])
    for m in (1, 7):
        keys, cnt = ops.vote_table_topm(counts.clone(), first, m)
        assert not nc.check_pair(c.name, (host(keys), host(cnt)), nc.hist_counter(nc.counts_as_hist(c, m)))


def test_vote_table_refusals(ops, ScdError):
    """Host-side refusals (no launch): top_k beyond the columns, (row_offset + n) * top_k = 2^40."""
    idx, preds = torch.zeros((8, 4), dtype=torch.int64, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(ScdError):
        ops.vote_table(idx, 5, preds, [0], 1, 0, 3)
    with pytest.raises(ScdError):
        ops.vote_table(idx, 4, preds, [0], 1, (1 << 38) - 8, 3)
    counts, first = ops.vote_table(idx, 4, preds, [0], 1, (1 << 38) - 9, 3)              # one row less: the largest position, 2^40 - 5
    assert host(counts).tolist() == [[32, 0, 0]] and host(first).tolist() == [[((1 << 38) - 9) * 4, nc.NEVER, nc.NEVER]]


# ------------------------------------------------------------------------------------------------ vote_table_topm
@pytest.mark.parametrize("c", nc.topm_cases(), ids=lambda c: c.name)
def test_vote_table_topm_on_crafted_tables(ops, c):
    want = nc.topm_want(c.counts, c.first, c.m)
    counts, first = dev(c.counts), dev(c.first)
    keys, cnt = ops.vote_table_topm(counts, first, c.m)
    print(c.name, "got", host(keys)[0][:8].tolist(), host(cnt)[0][:8].tolist(), "want", want[0][0][:8].tolist(), want[1][0][:8].tolist())
    bad = nc.check_pair(c.name, (host(keys), host(cnt), host(counts)), want, ("keys", "counts", "table after"))
    assert not bad, bad
    assert np.array_equal(host(first), c.first)
    again = dev(c.counts)
    keys2, cnt2 = ops.vote_table_topm(again, first, c.m)
    assert torch.equal(keys, keys2) and torch.equal(cnt, cnt2) and torch.equal(counts, again)


# ------------------------------------------------------------------------------------------------ bit movers
@pytest.mark.parametrize("shape", nc.TRANSPOSE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_transpose_f16_moves_bits(ops, shape):
    src = nc.any_f16_bits(7, shape)
    got = ops.transpose_f16(f16_dev(src))
    assert tuple(got.shape) == shape[::-1] and got.dtype == torch.float16
    assert np.array_equal(bits(got), src.T)


@pytest.mark.parametrize("shape", nc.GATHER_SHAPES, ids=lambda s: "d=%d,m=%d" % s)
def test_gather_rows_f16_moves_bits(ops, shape):
    d, m = shape
    src = nc.any_f16_bits(8, (nc.SELECT_ROWS, d))
    wt = f16_dev(src)
    for idx in nc.select_index(100 + m, m):
        got = ops.gather_rows_f16(wt, dev(idx))
        assert np.array_equal(bits(got), src[idx])


@pytest.mark.parametrize("shape", nc.SELECT_SHAPES, ids=lambda s: "d=%d,k=%d,m=%d" % s)
def test_select_rows_equals_indexing(ops, shape):
    """Every combination of the three outputs; random (duplicate) and descending row numbers."""
    d, k, m = shape
    f = nc.finite_f16(9, (nc.SELECT_ROWS, d))
    names = np.random.RandomState(10).randint(-(1 << 62), 1 << 62, size=(nc.SELECT_ROWS, k)).astype(np.int64)
    fd, nd = f16_dev(f), dev(names)
    for idx in nc.select_index(200 + m, m):
        idd = dev(idx)
        for want16 in (True, False):
            for want32 in (True, False):
                for with_names in (True, False):
                    if not (want16 or want32 or with_names):
                        continue
                    o16, o32, on = ops.select_rows(fd, idd, nd if with_names else None, want16=want16, want32=want32)
                    assert (o16 is None) == (not want16) and (o32 is None) == (not want32) and (on is None) == (not with_names)
                    if want16:
                        assert np.array_equal(bits(o16), f[idx].view(np.uint16)), (want16, want32, with_names)
                    if want32:
                        assert o32.dtype == torch.float32 and np.array_equal(host(o32).view(np.uint32), f[idx].astype(F32).view(np.uint32))
                    if with_names:
                        assert on.dtype == torch.int64 and np.array_equal(host(on), names[idx])


def test_select_rows_empty_and_refusals(ops, ScdError):
    f = f16_dev(nc.finite_f16(9, (nc.SELECT_ROWS, 64)))
    names = torch.zeros((nc.SELECT_ROWS, 5), dtype=torch.int64, device="cuda")
    o16, o32, on = ops.select_rows(f, torch.zeros(0, dtype=torch.int64, device="cuda"), names)
    assert tuple(o16.shape) == (0, 64) and tuple(o32.shape) == (0, 64) and tuple(on.shape) == (0, 5)
    idx = torch.zeros(3, dtype=torch.int64, device="cuda")
    with pytest.raises(ScdError):
        ops.select_rows(f, idx, torch.zeros((nc.SELECT_ROWS, 65), dtype=torch.int64, device="cuda"))
    with pytest.raises(ScdError):
        ops.select_rows(f, idx, None, want16=False, want32=False)


# ------------------------------------------------------------------------------------------------ mean2
@pytest.mark.parametrize("numel", nc.MEAN2_NUMELS)
def test_mean2_f16_is_the_rounded_exact_mean(ops, ScdError, numel):
    a, b = nc.mean2_inputs(numel)
    want = nc.mean2_want(a, b)
    got = bits(ops.mean2_f16(f16_dev(a), f16_dev(b))).view(F16)
    k = min(numel, len(nc.MEAN2_PAIRS))
    wrong = [(nc.MEAN2_PAIRS[i], float(got[i]), float(want[i])) for i in range(k) if not nc.same_f16(got[i:i + 1], want[i:i + 1])]
    assert not wrong, wrong
    assert nc.same_f16(got, want)
    assert got[0] == F16(65504.0)
    if numel == 8:
        with pytest.raises(ScdError):
            ops.mean2_f16(f16_dev(a[:4]).repeat(3), f16_dev(b[:4]).repeat(3))              # 12 elements


# ------------------------------------------------------------------------------------------------ l2norm_rows
@pytest.mark.parametrize("d", nc.L2_GRID_D)
def test_l2norm_rows_exact_grid(ops, d):
    for n in nc.L2_GRID_N:
        x, want = nc.l2_grid(d, n)
        for t in (F32, F16):
            got = host(ops.l2norm_rows(dev(x.astype(t))))
            assert got.dtype == t and np.array_equal(got.view(np.uint32 if t is F32 else np.uint16), want.astype(t).view(np.uint32 if t is F32 else np.uint16)), (d, n, t)


@pytest.mark.parametrize("d", nc.L2_GRID_D)
def test_l2norm_rows_random_inside_derived_bound(ops, d):
    for f16 in (False, True):
        for n in (5, 1025) if d in (65, 1000) else (5,):
            x = nc.l2_random(d, n, 600 + d, f16)
            ref = nc.l2_want(x)
            tol = nc.l2_bound(ref, d, f16)
            err = np.abs(host(ops.l2norm_rows(dev(x))).astype(F64) - ref)
            print("d=%d n=%d f16=%s: max err / bound %.3f" % (d, n, f16, float((err / tol).max())))
            assert (err <= tol).all(), (d, n, f16, float((err / tol).max()))


# ------------------------------------------------------------------------------------------------ prompt_pool
def run_pool(ops, emb, n_names, t_per, d, col0, ld_out):
    out = torch.full((d, ld_out), float(nc.POOL_SENTINEL), dtype=torch.float16, device="cuda")
    ops.prompt_pool(f16_dev(emb), n_names, t_per, out, col0)
    return bits(out).view(F16)


@pytest.mark.parametrize("d", nc.POOL_D)
def test_prompt_pool_exact_grid(ops, d):
    for kind, t_pers in ((nc.pool_grid_same, (1, 2, 4, 8)), (nc.pool_grid_disjoint, (4, 8))):
        for t_per in t_pers:
            emb, want = kind(d, t_per)
            n_names = want.shape[1]
            out = run_pool(ops, emb, n_names, t_per, d, 2, n_names + 5)
            assert np.array_equal(out[:, 2:2 + n_names].view(np.uint16), want.view(np.uint16)), (kind.__name__, d, t_per)
            rest = np.delete(out, np.arange(2, 2 + n_names), axis=1)
            assert (rest == nc.POOL_SENTINEL).all(), (kind.__name__, d, t_per)


@pytest.mark.parametrize("c", nc.pool_cases(), ids=lambda c: c.name)
def test_prompt_pool_random_inside_derived_bound(ops, c):
    out = run_pool(ops, c.emb, c.n_names, c.t_per, c.d, c.col0, c.ld_out)
    ref, tol = nc.pool_want(c)
    err = np.abs(out[:, c.col0:c.col0 + c.n_names].astype(F64) - ref)
    print(c.name, "max err / bound %.3f" % float((err / tol).max()))
    bad = nc.check_pool(c, out)
    assert not bad, bad
    again = run_pool(ops, c.emb, c.n_names, c.t_per, c.d, c.col0, c.ld_out)
    assert np.array_equal(out.view(np.uint16), again.view(np.uint16))


def test_prompt_pool_refuses_d_above_1024(ops, ScdError):
    out = torch.zeros((1025, 4), dtype=torch.float16, device="cuda")
    with pytest.raises(ScdError):
        ops.prompt_pool(torch.ones((2, 1025), dtype=torch.float16, device="cuda"), 1, 2, out, 0)
