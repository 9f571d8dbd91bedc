"""Can the inputs of tests/naming_cases.py tell a wrong vote histogram or naming helper from a right one?  Small numpy models of the
DOCUMENTED data flow of the kernels (scd_amd/csrc/vote.hip, the end of scd_amd/csrc/sim.hip) are run on every case and judged by the
references and checkers tests/test_gpu_naming_kernels.py uses:
  vote_hist   key1 = slot << 48 | name << 24 | position, sorted; the heads of the (slot, name) runs become records
              slot << 48 | (2^24 - 1 - count) << 24 | first position, sorted; a slot's output is the m records from the lower bound of
              slot << 48 (unsigned compare) on; the element (i, j) is read at i * ld + j
  table/top-m per shard counts[slot, name] += 1 and first[slot, name] = min(.., (row_offset + i) * top_k + j); the shards are added /
              min-ed; m rounds of arg-max over (count desc, first asc) on cells with a count > 0, the taken cell zeroed
  mean2       float32 sum, times 0.5, rounded to fp16
  l2norm      per lane ceil(d / 64) float32 fmas, a six-step xor butterfly, 1 / max(sqrt(s), 1e-12f), one product per element
  prompt_pool per prompt row 16 fmas per lane + butterfly, inv = 1 / sqrt(s); wave w accumulates rows w, w + 4, .. by fma; the four
              waves are added, divided by t_per; second norm by 4 fmas per thread, butterfly, three additions; product; fp16
Also shown here: the vectorised reference (np.unique) equals Counter.most_common on every small case, the references equal
oracle/naming_oracle.cluster_counters and the restatements of tests/oracle_backend.py, and the float32 models stay inside the DERIVED
bounds of the toleranced cases (the reference alone fits).

The correct model passes every case.  Each planted fault fails the case named here, and the test asserts exactly that:
  fault         what is wrong                                              caught by
  tie_last      ties go to the name seen LAST                              vote_hist   ties_descending
  count_asc     count ascending                                            vote_hist   m=1
  no_known      `known` ignored                                            vote_hist   known[40],cluster_all_known
  stride_topk   row stride top_k instead of ld                             vote_hist   ld>top_k[ld=7,top_k=3]
  slot_signed   the slot's lower bound searched with a signed compare      vote_hist   slots_bit15
  pos23         position field of 23 bits                                  vote_hist   big[n*top_k=2^24-1] (vectorised model)
  topm24        top-m count packed into 24 bits of one 64-bit key          top-m       count_bits  (the kernel before this test existed)
  first32       first-seen position truncated to 32 bits                   top-m       first_above_bit32;  table  row_offset=2^37
  mean_f16      mean2 added in fp16                                        mean2       pair 0 (65504 + 65504), every numel
  no_clamp      l2norm without the 1e-12 clamp                             l2norm      the zero row of every grid with n > 1
  no_prompt_nrm prompt_pool without the per-prompt normalisation           prompt_pool d=512,t_per=4,n_names=7
The model is not the kernel; what is asserted on the device is asserted there on the device's own output.
"""
import numpy as np
import torch

import naming_cases as nc
from oracle import naming_oracle as no
from oracle_backend import OracleNamingOps

F16, F32, F64 = np.float16, np.float32, np.float64
U64 = np.uint64
SENT = U64(0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------------------------------------ vote_hist model
def _lower_bound(rec, targets, signed):
    a, t = (rec.view(np.int64), targets.view(np.int64)) if signed else (rec, targets)
    lo, hi = np.zeros(len(t), dtype=np.int64), np.full(len(t), len(a), dtype=np.int64)
    while (lo < hi).any():
        mid = (lo + hi) >> 1
        act, less = lo < hi, a[np.minimum(mid, len(a) - 1)] < t
        lo, hi = np.where(act & less, mid + 1, lo), np.where(act & ~less, mid, hi)
    return lo


def hist_model(c, mut=()):
    n, ld = c.idx.shape
    pos_bits = 23 if "pos23" in mut else nc.POS_BITS
    e = np.arange(n * c.top_k, dtype=np.int64)
    i, j = e // c.top_k, e % c.top_k
    name = c.idx.reshape(-1)[i * (c.top_k if "stride_topk" in mut else ld) + j]
    p = c.preds[i]
    slot_of = np.full(nc.MAX_CLUSTER_ID, -1, dtype=np.int64)
    slot_of[np.asarray(c.clusters, dtype=np.int64)] = np.arange(len(c.clusters))
    inside = (p >= 0) & (p < nc.MAX_CLUSTER_ID)
    slot = np.where(inside, slot_of[np.where(inside, p, 0)], -1)
    drop = (slot < 0) | (name < 0) | (name >= nc.NAME_LIM)
    if c.known is not None and len(c.known) and "no_known" not in mut:
        drop |= np.isin(name, np.asarray(c.known, dtype=np.int64))
    k1 = (slot.astype(U64) << U64(48)) | ((name & (nc.NAME_LIM - 1)).astype(U64) << U64(24)) | (e & ((1 << pos_bits) - 1)).astype(U64)
    k1 = np.sort(np.where(drop, SENT, k1))
    pre = k1 >> U64(24)
    head = (k1 != SENT) & np.concatenate([[True], pre[1:] != pre[:-1]])
    at = np.nonzero(head)[0]
    count = np.diff(np.concatenate([at, [int((k1 != SENT).sum())]])).astype(U64)
    low = k1[at] & U64(0xFFFFFF)
    if "tie_last" in mut:
        low = U64(0xFFFFFF) - low
    cnt_field = count if "count_asc" in mut else U64(0xFFFFFF) - count
    rec = (k1[at] & U64(0xFFFF000000000000)) | (cnt_field << U64(24)) | low
    order = np.argsort(rec, kind="stable")
    rec, rname = rec[order], ((k1[at] >> U64(24)) & U64(0xFFFFFF)).astype(np.int64)[order]
    nc_ = len(c.clusters)
    slots = np.arange(nc_, dtype=np.int64)
    keys = np.full((nc_, c.m), -1, dtype=np.int64)
    counts = np.zeros((nc_, c.m), dtype=np.int32)
    if len(rec):
        lo = _lower_bound(rec, slots.astype(U64) << U64(48), "slot_signed" in mut)
        pp = lo[:, None] + np.arange(c.m, dtype=np.int64)[None, :]
        ok = pp < len(rec)
        r = rec[np.minimum(pp, len(rec) - 1)]
        ok &= (r >> U64(48)).astype(np.int64) == slots[:, None]
        keys[ok] = rname[np.minimum(pp, len(rec) - 1)][ok]
        cf = ((r >> U64(24)) & U64(0xFFFFFF)).astype(np.int64)
        counts[ok] = (cf if "count_asc" in mut else 0xFFFFFF - cf)[ok].astype(np.int32)
    return keys, counts


HIST_FAULTS = {"tie_last": "ties_descending", "count_asc": "m=1", "no_known": "known[40],cluster_all_known",
               "stride_topk": "ld>top_k[ld=7,top_k=3]", "slot_signed": "slots_bit15"}


def test_vectorised_reference_equals_counter_on_every_small_case():
    for c in nc.hist_cases():
        assert not nc.check_pair(c.name, nc.hist_unique(c), nc.hist_counter(c)), c.name


def test_counter_reference_is_the_oracles():
    """hist_counter against oracle.naming_oracle.cluster_counters (which knows no name limit: the names the key has no room for are
    taken out of its most_common list)."""
    for c in nc.hist_cases():
        if len(c.clusters) > 100:
            continue
        ref = no.cluster_counters(c.idx, c.preds, c.clusters, c.top_k, known=c.known if c.known else None)
        keys, counts = nc.hist_counter(c)
        for s, cl in enumerate(c.clusters):
            mc = [(int(a), int(b)) for a, b in ref[cl].most_common() if 0 <= a < nc.NAME_LIM][:c.m]
            got = [(int(a), int(b)) for a, b in zip(keys[s], counts[s]) if a >= 0]
            assert got == mc and (counts[s][keys[s] < 0] == 0).all(), (c.name, cl)


def test_hist_cases_hold_what_they_are_named_for():
    by = {c.name: c for c in nc.hist_cases()}
    c = by["slots_bit15"]
    keys, _ = nc.hist_want(c)
    assert len(c.clusters) == 40000 and {0, nc.MAX_CLUSTER_ID - 1} <= set(c.clusters)
    assert sorted(np.nonzero(keys[:, 0] >= 0)[0].tolist()) == [0, 1, 32767, 32768, 32769, 39999]
    assert {int(x) for x in nc.BAD_PREDS} <= set(c.preds.tolist())
    counted = set(keys[keys >= 0].tolist())
    assert {0, nc.NAME_LIM - 1} <= set(c.idx.reshape(-1).tolist()) and counted <= set(range(40)) | {nc.NAME_LIM - 1}
    assert {-1, nc.NAME_LIM} <= set(c.idx.reshape(-1).tolist())
    keys, counts = nc.hist_want(by["known[40],cluster_all_known"])
    assert (keys[1] == -1).all() and (counts[1] == 0).all() and (keys[0] >= 0).all()
    keys, counts = nc.hist_want(by["ties_descending"])
    assert keys[1, :10].tolist() == list(range(9, -1, -1)) and (counts[1, :10] == 3).all()
    keys, _ = nc.hist_want(by["m=130"])
    assert (keys >= 0).all()
    keys, _ = nc.hist_want(by["m=700"])
    assert (keys[:, -1] == -1).all()
    for s in (31, 32, 33):
        _, counts = nc.hist_want(by["ties[seed=%d]" % s])
        assert any(len(set(r[r > 0].tolist())) < (r > 0).sum() for r in counts)


def test_hist_model_passes_and_every_fault_is_caught():
    cases = nc.hist_cases()
    for c in cases:
        assert not nc.check_hist(c, *hist_model(c)), c.name
    by = {c.name: c for c in cases}
    for fault, name in HIST_FAULTS.items():
        assert nc.check_hist(by[name], *hist_model(by[name], (fault,))), (fault, name)


def test_big_case_catches_a_23_bit_position():
    c = nc.big_case()
    assert c.idx.shape[0] * c.top_k == (1 << 24) - 1
    want = nc.big_want()
    assert not nc.check_pair(c.name, hist_model(c), want)
    got = hist_model(c, ("pos23",))
    assert nc.check_pair(c.name, got, want)
    late = c.clusters.index(nc.BIG_LATE)
    assert got[0][late, :2].tolist() == [nc.NAME_LIM - 3, nc.NAME_LIM - 2]


# ------------------------------------------------------------------------------------------------ table + top-m model
def table_model(c, rows=slice(None), row_offset=None, mut=()):
    counts, first = nc.table_loop(c._replace(idx=c.idx[rows], preds=c.preds[rows], row_offset=c.row_offset if row_offset is None else row_offset))
    if "first32" in mut:
        first = np.where(counts > 0, first & 0xFFFFFFFF, first)
    return counts, first


def topm_model(counts, first, m, mut=()):
    """m rounds of arg-max; -> (keys, cnt, counts after)."""
    counts = counts.copy()
    keys = np.full((counts.shape[0], m), -1, dtype=np.int64)
    cnt = np.zeros((counts.shape[0], m), dtype=np.int32)
    mask40 = U64((1 << 40) - 1)
    for s in range(counts.shape[0]):
        for j in range(m):
            live = np.nonzero(counts[s] > 0)[0]
            if "topm24" in mut:
                key = (counts[s, live].astype(U64) << U64(40)) | (mask40 - (first[s, live].astype(U64) & mask40))
                live = live[key > 0]
                key = key[key > 0]
                if not len(live):
                    continue
                b = int(np.argmax(key))
                keys[s, j], cnt[s, j] = live[b], int(key[b] >> U64(40))
                counts[s, live[b]] = 0
                continue
            if not len(live):
                continue
            f = first[s, live] & 0xFFFFFFFF if "first32" in mut else first[s, live]
            b = live[np.lexsort((live, f, -counts[s, live].astype(np.int64)))[0]]
            keys[s, j], cnt[s, j] = b, counts[s, b]
            counts[s, b] = 0
    return keys, cnt, counts


def test_table_reference_equals_the_loop_and_the_backend_restatement():
    be = OracleNamingOps()
    for c in nc.table_cases() + [x[0] for x in nc.shard_cases()]:
        want = nc.table_want(c)
        assert not nc.check_pair(c.name, nc.table_loop(c), want, ("counts", "first"))
        assert ((want[1] == nc.NEVER) == (want[0] == 0)).all()
        if 0 < c.idx.shape[0] <= 2000:
            # the backend's restatement indexes its table with every name and prediction: give it the rows it can take
            ok = (c.preds >= 0) & (c.preds < c.n_slots) & ((c.idx[:, :c.top_k] >= 0) & (c.idx[:, :c.top_k] < c.v)).all(axis=1)
            sub = c._replace(idx=c.idx[ok], preds=c.preds[ok])
            got = be.vote_table(torch.from_numpy(sub.idx), c.top_k, torch.from_numpy(sub.preds), c.clusters, c.n_slots, c.row_offset, c.v)
            assert not nc.check_pair(c.name, (got[0].numpy(), got[1].numpy()), nc.table_want(sub), ("counts", "first"))
    c = [x for x in nc.table_cases() if x.name == "row_offset=2^37"][0]
    _, first = nc.table_want(c)
    assert first[first != nc.NEVER].min() >= (1 << 37) * c.top_k > 1 << 32
    assert nc.check_pair(c.name, table_model(c, mut=("first32",)), nc.table_want(c), ("counts", "first"))


def test_sharded_flow_equals_counter():
    """tables per shard, added / min-ed, then the top-m: equal to the single table AND to Counter.most_common on the rows."""
    for c, cuts in nc.shard_cases():
        parts = [table_model(c, slice(a, b), c.row_offset + a) for a, b in zip(cuts[:-1], cuts[1:])]
        assert any(a == b for a, b in zip(cuts[:-1], cuts[1:]))
        counts, first = sum(p[0] for p in parts), np.minimum.reduce([p[1] for p in parts])
        assert not nc.check_pair(c.name, (counts, first), nc.table_want(c), ("counts", "first"))
        for m in (1, 7):
            keys, cnt, _ = topm_model(counts, first, m)
            assert not nc.check_pair(c.name, (keys, cnt), nc.hist_counter(nc.counts_as_hist(c, m)))


def test_topm_model_passes_and_faults_are_caught():
    be = OracleNamingOps()
    by = {}
    for c in nc.topm_cases():
        by[c.name] = c
        want = nc.topm_want(c.counts, c.first, c.m)
        assert not nc.check_pair(c.name, topm_model(c.counts, c.first, c.m), want, ("keys", "counts", "table after")), c.name
        k, n = be.vote_table_topm(torch.from_numpy(c.counts), torch.from_numpy(c.first), c.m)
        assert not nc.check_pair(c.name, (k.numpy(), n.numpy()), want[:2]), c.name
        taken = want[0][want[0] >= 0]
        assert (want[2] <= c.counts).all() and int((want[2] != c.counts).sum()) == len(taken)
    c = by["count_bits"]
    want = nc.topm_want(c.counts, c.first, c.m)
    assert want[1][0].tolist() == [(1 << 31) - 1, (1 << 24) + 5, 1 << 24, (1 << 24) - 1, 3, 1, 0, 0]
    got = topm_model(c.counts, c.first, c.m, ("topm24",))
    assert nc.check_pair(c.name, got, want, ("keys", "counts", "table after"))
    # the packed key of the kernel before the fix: 2^31 - 1 ranks as 2^24 - 1, 2^24 + 5 as 5, and 2^24 as 0 with count 0
    assert got[1][0].tolist()[:5] == [(1 << 24) - 1, (1 << 24) - 1, 5, 3, 1] and 0 in got[1][0].tolist()[:6]
    c = by["first_above_bit32"]
    assert nc.check_pair(c.name, topm_model(c.counts, c.first, c.m, ("first32",)), nc.topm_want(c.counts, c.first, c.m), ("keys", "counts", "table after"))
    for name in ("v=1", "v=255", "v=256", "v=257", "v=1031"):
        c = by[name]
        assert nc.topm_want(c.counts, c.first, c.m)[0][0, 0] == c.counts.shape[1] - 1


# ------------------------------------------------------------------------------------------------ float32 models
def _fma32(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)       # the product is exact in float64


def _butterfly(v):
    """[.., 64] float32 -> [..]: the six-step xor butterfly (every lane ends with the same sum)."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ o]).astype(F32)
    return v[..., 0]


def _lanes(x, slots):
    """[n, d] -> float32 [n, slots, 64], zero padded: lane l of slot i holds column i * 64 + l."""
    out = np.zeros((x.shape[0], slots * 64), dtype=F32)
    out[:, :x.shape[1]] = x.astype(F32)
    return out.reshape(x.shape[0], slots, 64)


def l2_model(x, mut=()):
    n, d = x.shape
    slots = -(-d // 64)
    v = _lanes(x, slots)
    s = np.zeros((n, 64), dtype=F32)
    for i in range(slots):
        s = _fma32(v[:, i], v[:, i], s)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(_butterfly(s))
        inv = F32(1.0) / (nrm if "no_clamp" in mut else np.maximum(nrm, F32(1e-12)))
        return (x.astype(F32) * inv[:, None]).astype(x.dtype)


def pool_model(emb, n_names, t_per, d, mut=()):
    """-> fp16 [d, n_names]"""
    out = np.zeros((d, n_names), dtype=F16)
    for name in range(n_names):
        v = _lanes(emb[name * t_per:(name + 1) * t_per], 16)                    # [t, 16, 64]
        s = np.zeros((t_per, 64), dtype=F32)
        for i in range(16):
            s = _fma32(v[:, i], v[:, i], s)
        inv = F32(1.0) / np.sqrt(_butterfly(s))
        if "no_prompt_nrm" in mut:
            inv = np.ones_like(inv)
        part = np.zeros((4, 16, 64), dtype=F32)
        for t in range(t_per):
            part[t % 4] = _fma32(v[t], np.broadcast_to(inv[t], v[t].shape), part[t % 4])
        part = part.reshape(4, 1024)
        mean = ((((part[0] + part[1]).astype(F32) + part[2]).astype(F32) + part[3]).astype(F32) / F32(t_per)).astype(F32)
        mean[d:] = 0
        mq = mean.reshape(4, 4, 64)                                             # [q, wave, lane]: column q * 256 + wave * 64 + lane
        s = np.zeros((4, 64), dtype=F32)
        for q in range(4):
            s = _fma32(mq[q], mq[q], s)
        red = _butterfly(s)
        inv2 = F32(1.0) / np.sqrt((((red[0] + red[1]).astype(F32) + red[2]).astype(F32) + red[3]).astype(F32))
        out[:, name] = (mean[:d] * inv2).astype(F32).astype(F16)
    return out


def test_mean2_model_and_fp16_addition():
    for numel in nc.MEAN2_NUMELS:
        a, b = nc.mean2_inputs(numel)
        want = nc.mean2_want(a, b)
        with np.errstate(all="ignore"):
            model = ((a.astype(F32) + b.astype(F32)) * F32(0.5)).astype(F16)
            fault = ((a + b).astype(F16) * F16(0.5)).astype(F16)
        assert nc.same_f16(model, want), numel
        assert not nc.same_f16(fault, want) and np.isinf(fault[0]) and want[0] == F16(65504.0), numel
    a, b = nc.mean2_inputs(8 * 257)
    want = nc.mean2_want(a, b)
    k = len(nc.MEAN2_PAIRS)
    assert want[1] == F16(1.0) and want[2] == F16(1.0 + 2.0 ** -9) and want[8] == 0 and not np.isinf(want[0])
    sub = np.abs(want[:k].astype(F64))
    assert ((sub > 0) & (sub < 2.0 ** -14)).sum() >= 5 and np.isnan(want[:k]).sum() >= 4 and np.isinf(want[:k]).sum() >= 3
    assert np.signbit(want[6]) and not np.signbit(want[5])                     # -0 + -0 = -0, 0 + -0 = +0


def test_l2_grid_is_exact_in_the_model_and_needs_the_clamp():
    for d in nc.L2_GRID_D:
        for n in nc.L2_GRID_N:
            x, want = nc.l2_grid(d, n)
            for t in (F32, F16):
                assert np.array_equal(l2_model(x.astype(t)).astype(F64), want), (d, n, t)
                if n > 1:
                    bad = l2_model(x.astype(t), ("no_clamp",))
                    assert np.isnan(bad[n - 2]).all() and not np.array_equal(bad.astype(F64), want), (d, n, t)


def test_l2_model_stays_inside_the_derived_bound():
    for f16 in (False, True):
        for d in nc.L2_GRID_D:
            x = nc.l2_random(d, 9, 500 + d, f16)
            ref = nc.l2_want(x)
            err = np.abs(l2_model(x).astype(F64) - ref)
            assert (err <= nc.l2_bound(ref, d, f16)).all(), (d, f16, float((err / nc.l2_bound(ref, d, f16)).max()))
            if not f16:
                assert np.abs(x).min() < 2.0 ** -30 and np.abs(x).max() > 2.0 ** 30 or d < 64


def test_pool_grids_are_exact_in_the_model():
    for d in nc.POOL_D:
        for t_per in (1, 2, 4, 8):
            emb, want = nc.pool_grid_same(d, t_per)
            assert np.array_equal(pool_model(emb, want.shape[1], t_per, d).view(np.uint16), want.view(np.uint16)), (d, t_per)
        for t_per in (4, 8):
            emb, want = nc.pool_grid_disjoint(d, t_per)
            assert np.array_equal(pool_model(emb, want.shape[1], t_per, d).view(np.uint16), want.view(np.uint16)), (d, t_per)


def _pool_out(c, mut=()):
    out = np.full((c.d, c.ld_out), nc.POOL_SENTINEL, dtype=F16)
    out[:, c.col0:c.col0 + c.n_names] = pool_model(c.emb, c.n_names, c.t_per, c.d, mut)
    return out


def test_pool_model_stays_inside_the_derived_bound_and_needs_the_prompt_norm():
    cases = nc.pool_cases()
    assert {c.d for c in cases} == set(nc.POOL_D) and {c.t_per for c in cases} == set(nc.POOL_T) and {c.n_names for c in cases} == {1, 7}
    for c in cases:
        assert c.col0 > 0 and c.ld_out > c.col0 + c.n_names
        assert not nc.check_pool(c, _pool_out(c)), c.name
        out = _pool_out(c)
        out[0, 0] = F16(1.0)                                                     # a write outside the columns is seen
        assert nc.check_pool(c, out)
    c = [x for x in cases if x.name == "d=512,t_per=4,n_names=7"][0]
    assert nc.check_pool(c, _pool_out(c, ("no_prompt_nrm",)))
