"""The encoder's attention kernels one by one against a float64 restatement (oracle/clip_oracle.py attention_f64 /
attention_single_query_f64), through the test entry points scd_attention_f16 (the dispatcher run_blocks uses: attention_short_kernel,
attention_kernel<2|3|7>, attention_persist_kernel<true|false>) and scd_attention_single_query_f16 (the last block's CLS / EOT row).

Error budget (derived from where the kernels round, not measured).  Per (query, head) the kernels compute the scores s_j in fp32
from fp16 Q and K (the products are exact), p_j = 2^((s_j - m) * log2(e) / 8) in fp32 with m the row maximum, S = sum_j p_j in fp32,
round every p_j to fp16 for the P V MFMA (fp32 accumulation of exact products) and round o = (sum_j fp16(p_j) v_j) / S to fp16 once.
With pi_j = p_j / S the exact probabilities and u = 2^-11 (half an fp16 ulp, relative):
  * rounding p_j to fp16 moves o by at most u * sum_j pi_j |v_j| while p_j is a normal fp16 number (p_j >= 2^-14), and by at most
    2^-25 |v_j| / S = 2^-25 pi_max |v_j| absolute below that (the subnormal spacing is 2^-24; p_j < 2^-25 flushes to 0 with the same
    bound; S = 1 / pi_max because the maximum key has p = 1);
  * rounding o to fp16: u |o| while |o| >= 2^-14, 2^-25 absolute below (covered by the 2^-24 term);
  * everything else is fp32 arithmetic: the score sums (a few 2^-24 relative of sum_d |q_d k_d|, times 0.18 in the exponent), the
    exponent argument, exp2, S, the P V accumulation: below 2^-20 relative for the scores used here, covered by the factor 2.
Hence, per element:  |o - ref| <= 2 * (2^-11 * (|ref| + sum_j pi_j |v_jd|) + 2^-25 * pi_max * sum_j |v_jd|) + 2^-24.
The subnormal term is part of rounding P to fp16: without it a row whose tail keys sit between 2^-25 and 2^-14 could legitimately
exceed the bound.  It is at most 2^-25 * T * max|v| and does not hide any of the planted failures below, each of which moves an output
by a large fraction of |v|.

Inputs (every kernel, both masks where the ladder serves them, widths 320 / 512 / 768 / 1024, item counts below, at and several times
256 and not a multiple of 4):
  * planted one-hot attention: query i gets 8 * code(pi(i)) with +-1 codes of 62 dims whose pairwise dot products are at most 20, so
    the target beats every other key by >= 336 raw units (p < 2^-60): the output row must EQUAL v_pi(i).  pi covers key 0, T - 1,
    191 / 192 and 196 / 197 where they exist, and causal targets pi(i) <= i including pi(i) = i (row 0 sees key 0 only);
  * exact ties: key T // 2 is a copy of key 1, so a query aiming at either gets fp16((v_1 + v_T//2) / 2) (causal: v_1 until T // 2 is
    visible).  V holds n * 2^(e-4) with |n| <= 1000, so the tie means are fp16 numbers and the exactness needs no rounding luck;
  * hidden keys: non-causal, key T - 1 is the runner-up ~24 raw units (3 in natural log) below every other target (the persistent
    kernels pad K with copies of row T - 1: one leaked copy moves the row by ~5 % of |v|); causal, one future key out-scores every
    visible key by >= 16 raw units;
  * stale keys: in persistent launches an item runs as step item // 256 of its block; keys of alternate steps carry +-13 in two more
    dims and their queries -+13, so the previous item's keys (the other half of the LDS double buffer) out-score every key of the
    current item by >= 20 raw units;
  * dense sharp attention: random Q, K with exp2-argument ranges of ~30-60 per row, V rows of magnitudes 2^-6 .. 2^6;
  * the largest scores fp16 Q K can produce at head dim 64: the one-hot codes scaled by 65504 (target score 62 * 65504^2 = 2.7e11).
    Before the fix of this case the kernels returned NaN rows: p_max = 2^(m * cs - fl(m * cs)) with an offset of up to
    +-2048 (encoder.hip max_offset_is_large).
"""
import os

import numpy as np
import pytest
import torch

from oracle import clip_oracle as co

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from scd_amd import ops as o
    return o


_CODES = {}


def _codes(n, seed=1234, dims=62, limit=20):
    """n +-1 codes of `dims` dims with |<c_a, c_b>| <= limit for a != b (greedy rejection sampling, cached)."""
    key = (n, seed, dims, limit)
    if key not in _CODES:
        rs = np.random.RandomState(seed)
        out = np.zeros((0, dims))
        while len(out) < n:
            for c in rs.choice([-1.0, 1.0], size=(256, dims)):
                if len(out) == 0 or np.abs(out @ c).max() <= limit:
                    out = np.vstack([out, c])
                    if len(out) == n:
                        break
        _CODES[key] = out
    return _CODES[key]


def _targets(T, causal, rs):
    """pi(i) for one (sequence, head): random (causal: <= i), with the edge keys forced in."""
    if causal:
        pi = np.array([rs.randint(0, i + 1) for i in range(T)])
        for i in (T - 1, 191, 192, 196, 197, 1, 0):
            if i < T:
                pi[i] = i                                            # the diagonal, incl. the padding edges
        if T > 3:
            pi[T - 2] = 0
            pi[T // 2 + 1] = 1                                       # sees both twins (1 and T // 2)
    else:
        pi = rs.randint(0, T, size=T)
        forced = [T - 1, 0, 191, 192, 196, 197, T - 2, 1]
        for i, t in enumerate(forced):
            if i < T and 0 <= t < T:
                pi[i] = t
    return pi


def _v_lattice(shape, rs):
    """V = n * 2^(e - 4), |n| <= 1000, e in [-8, 0] per key row: exact fp16 (>= 2^-12 or 0).  Returns V and e."""
    n = rs.randint(-1000, 1001, size=shape).astype(np.float64)
    e = rs.randint(-8, 1, size=shape[:-1] + (1,)).astype(np.float64)
    return n * 2.0 ** (e - 4), e


def _pack(Q, K, V):
    """[B, H, T, 64] x 3 -> qkv fp16 [B*T, 3*H*64] on the device (the QKV GEMM's layout)."""
    B, H, T, _ = Q.shape
    parts = [torch.from_numpy(np.ascontiguousarray(X)).permute(0, 2, 1, 3).reshape(B * T, H * 64) for X in (Q, K, V)]
    return torch.cat(parts, 1).half().cuda().contiguous()


def _planted(B, T, H, causal, mode, seed, stale, q_scale=1.0, k_scale=1.0):
    """mode 'onehot': one dominant key per query (exact), 'hidden': + runner-up T - 1 (non-causal) / key i + 1 above all (causal)."""
    rs = np.random.RandomState(seed)
    U = _codes(T).copy()
    Q = np.zeros((B, H, T, 64))
    K = np.zeros((B, H, T, 64))
    V, e = _v_lattice((B, H, T, 64), rs)
    if T >= 4:                                                       # twins: key T // 2 = key 1, its V row on the same lattice
        U[T // 2] = U[1]
        V[..., T // 2, :] = rs.randint(-1000, 1001, size=(B, H, 64)) * 2.0 ** (e[..., 1, :] - 4)
    K[..., :62] = U
    for b in range(B):
        for h in range(H):
            pi = _targets(T, causal, rs)
            Q[b, h, :, :62] = 8.0 * U[pi]
            if mode == "hidden":
                if causal:
                    Q[b, h, :T - 1, :62] += 16.0 * U[1:]
                else:
                    for i in np.nonzero(pi != T - 1)[0]:
                        c = float(U[pi[i]] @ U[T - 1])
                        Q[b, h, i, :62] += np.round((8.0 - 24.0 / (62.0 - c)) * 64) / 64 * U[T - 1]
    if stale:
        item = np.arange(B * H).reshape(B, H)
        sig = np.where((item // 256) % 2 == 0, 13.0, -13.0)[..., None, None]
        K[..., 62:] = sig
        Q[..., 62:] = -sig
    return _pack(Q * q_scale, K * k_scale, V)


def _dense(B, T, H, seed):
    rs = np.random.RandomState(seed)
    sig = np.array([2.0, 2.4, 3.0])[np.arange(H) % 3].reshape(1, H, 1, 1)
    Q = rs.randn(B, H, T, 64) * sig
    K = rs.randn(B, H, T, 64) * sig
    V = rs.randn(B, H, T, 64) * 2.0 ** rs.randint(-6, 7, size=(B, H, T, 1))
    return _pack(Q, K, V)


def _heads_view(x, B, T, H):
    """[B*T, H*64] -> [B, H, T, 64]"""
    return x.view(B, T, H, 64).permute(0, 2, 1, 3)


def _bound(ref, P, Vabs, visible):
    """the error budget of the module docstring, elementwise, [.., 64] float64"""
    u = 2.0 ** -11
    return 2 * (u * (ref.abs() + P @ Vabs) + 2.0 ** -25 * P.max(-1, keepdim=True).values * (visible.double() @ Vabs)) + 2.0 ** -24


def _check_full(ops, qkv, B, T, H, causal, exact=False, what=""):
    out = ops.attention_f16(qkv, B, T, H, causal)
    torch.cuda.synchronize()
    ref, P = co.attention_f64(qkv, B, T, H, causal)
    W = 64 * H
    V = _heads_view(qkv[:, 2 * W:].double(), B, T, H)
    vis = torch.ones(T, T, dtype=torch.bool, device=qkv.device)
    if causal:
        vis = vis.tril()
    o4, r4 = _heads_view(out.double(), B, T, H), _heads_view(ref, B, T, H)
    assert bool(torch.isfinite(o4).all()), what
    err = (o4 - r4).abs()
    bnd = _bound(r4, P, V.abs(), vis)
    bad = err > bnd
    assert not bool(bad.any()), "%s: %d elements over budget, worst err / bound %.3g" % (what, int(bad.sum()), float((err / bnd).max()))
    if exact:
        _check_exact(o4, P, V, what)
    return out


def _check_exact(o4, P, V, what):
    """rows whose probability mass sits on one key (or two exact twins) up to < 2^-36: the output is v of that key / the fp16 mean."""
    top = P.max(-1, keepdim=True).values
    on = P >= top * (1 - 1e-12)
    rest = torch.where(on, torch.zeros_like(P), P).sum(-1)
    sharp = rest < 2.0 ** -36
    assert bool(sharp.all()), "%s: %d planted rows are not one-hot" % (what, int((~sharp).sum()))
    want = ((on.double() @ V) / on.double().sum(-1, keepdim=True)).half().double()
    diff = (o4 != want).any(-1) & sharp
    assert not bool(diff.any()), "%s: %d one-hot rows differ from the selected V rows, first at %s" % (
        what, int(diff.sum()), tuple(torch.nonzero(diff)[0].tolist()))


# (T, causal, heads, batch): every branch of the ladder; items = batch * heads below 256, exactly 256, several times 256, odd
SHAPES = [
    (1, False, 8, 3), (1, True, 5, 7), (2, True, 8, 4), (2, False, 16, 2), (17, True, 12, 5), (17, False, 5, 7),
    (31, False, 8, 32), (31, True, 16, 3), (32, True, 5, 7), (32, False, 12, 9),                                   # short
    (33, True, 8, 5), (33, False, 5, 7), (48, False, 12, 3), (48, True, 16, 16), (64, True, 5, 7), (64, False, 8, 40),   # <2>
    (65, False, 16, 3), (65, True, 5, 7), (77, True, 8, 32), (77, False, 12, 5), (96, True, 12, 3), (96, False, 5, 9),   # <3>
    (197, False, 12, 3), (197, False, 8, 32), (197, False, 8, 100), (197, False, 5, 7), (197, False, 16, 70),         # persist<true>
    (193, False, 8, 100), (200, False, 12, 3), (200, False, 5, 111), (224, False, 16, 16), (224, False, 8, 70),       # persist<false>
    (197, True, 12, 3), (197, True, 5, 7),                                                                             # <7>
]


def _id(s):
    return "T%d%s_h%d_b%d" % (s[0], "c" if s[1] else "", s[2], s[3])


@pytest.mark.parametrize("shape", SHAPES, ids=[_id(s) for s in SHAPES])
def test_attention_matches_float64(ops, shape):
    T, causal, H, B = shape
    persist = T > 192 and not causal
    seed = T * 1000 + H * 10 + int(causal)
    qkv = _planted(B, T, H, causal, "onehot", seed, stale=persist)
    _check_full(ops, qkv, B, T, H, causal, exact=True, what="one-hot %s" % _id(shape))
    if T > 1:
        qkv = _planted(B, T, H, causal, "hidden", seed + 1, stale=persist)
        _check_full(ops, qkv, B, T, H, causal, what="hidden keys %s" % _id(shape))
    qkv = _dense(B, T, H, seed + 2)
    _check_full(ops, qkv, B, T, H, causal, what="dense %s" % _id(shape))


def test_attention_hidden_keys_would_be_seen():
    """The planted hidden keys are not decoration: on the float64 reference, one leaked copy of key T - 1 (the persistent kernels'
    K padding) or the causal mask opened by one key moves nearly every output row far beyond the budget."""
    B, T, H = 1, 200, 8
    qkv = _planted(B, T, H, False, "hidden", 7, stale=True)
    ref, P = co.attention_f64(qkv, B, T, H, False)
    W = 64 * H
    Vh = _heads_view(qkv[:, 2 * W:].double(), B, T, H)
    bnd = _bound(_heads_view(ref, B, T, H), P, Vh.abs(), torch.ones(T, T, dtype=torch.bool, device=qkv.device))
    # one leaked padding copy of key T - 1
    padded = torch.cat([qkv.view(B, T, -1), qkv.view(B, T, -1)[:, T - 1:]], 1).view(B * (T + 1), -1)
    leak, _ = co.attention_f64(padded, B, T + 1, H, False)
    leak = _heads_view(leak.view(B, T + 1, W)[:, :T].reshape(B * T, W), B, T, H)
    moved = ((leak - _heads_view(ref, B, T, H)).abs() > bnd).any(-1)
    assert float(moved.double().mean()) > 0.9
    # causal: query i sees key i + 1
    T = 77
    qkv = _planted(B, T, H, True, "hidden", 8, stale=False)
    ref, P = co.attention_f64(qkv, B, T, H, True)
    Vh = _heads_view(qkv[:, 2 * W:].double(), B, T, H)
    vis = torch.ones(T, T, dtype=torch.bool, device=qkv.device).tril()
    bnd = _bound(_heads_view(ref, B, T, H), P, Vh.abs(), vis)
    k, q = _heads_view(qkv[:, W:2 * W].double(), B, T, H), _heads_view(qkv[:, :W].double(), B, T, H)
    s = (q @ k.transpose(-1, -2)) / 8
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool, device=s.device).triu(2), float("-inf"))
    off = s.softmax(-1) @ Vh
    moved = ((off - _heads_view(ref, B, T, H)).abs() > bnd).any(-1)[..., :T - 1]
    assert float(moved.double().mean()) > 0.9


@pytest.mark.parametrize("shape", [(17, True, 8, 3), (48, False, 5, 7), (77, True, 12, 2), (96, False, 8, 3), (197, False, 8, 40),
                                   (224, False, 5, 7), (197, True, 5, 3)], ids=_id)
def test_attention_largest_scores(ops, shape):
    """Regression: scores up to 62 * 65504^2 = 2.7e11, the range of fp16 Q K at head dim 64.  The kernels subtracted the row maximum
    inside fma(s, cs, -fl(m * cs)), leaving the maximum key 2^(m * cs - fl(m * cs)) with an offset of up to +-2048: inf or 0, NaN rows."""
    T, causal, H, B = shape
    qkv = _planted(B, T, H, causal, "onehot", 99 + T, stale=False, q_scale=65504.0 / 8.0, k_scale=65504.0)
    assert float(qkv.abs().max()) >= 65504.0
    _check_full(ops, qkv, B, T, H, causal, exact=True, what="largest scores %s" % _id(shape))


# ------------------------------------------------------------------------------------------------ the last block's one query
SQ_SHAPES = [(197, False, 12, 3), (197, False, 5, 7), (197, False, 8, 64), (2, True, 5, 7), (9, True, 8, 6), (33, True, 5, 7),
             (77, True, 12, 5), (77, True, 8, 33)]


def _positions(B, T, causal, rs):
    """the query's position per sequence: the CLS row 0 (non-causal); causal: 0, 1 and T - 1 first, then random"""
    if not causal:
        return np.zeros(B, dtype=np.int64)
    pos = rs.randint(0, T, size=B)
    for i, p in enumerate((0, 1, T - 1)[:B]):
        pos[i] = min(p, T - 1)
    return pos


def _check_single(ops, qkv, B, T, H, causal, pos, exact, what):
    W = 64 * H
    rows = torch.as_tensor(np.arange(B) * T + pos, device="cuda")
    q = qkv[rows, :W].contiguous()
    kv = qkv[:, W:].contiguous()
    qrow = rows.to(torch.int32)
    out = ops.attention_single_query_f16(kv, q, qrow, T, H, causal)
    torch.cuda.synchronize()
    ref, P = co.attention_single_query_f64(kv, q, torch.as_tensor(pos, device="cuda"), T, H, causal)
    V = kv[:, W:].double().view(B, T, H, 64).permute(0, 2, 1, 3)                     # [B, H, T, 64]
    keys = torch.arange(T, device="cuda")
    vis = (keys.view(1, 1, 1, T) <= torch.as_tensor(pos, device="cuda").view(B, 1, 1, 1)) if causal else \
        torch.ones(B, 1, 1, T, dtype=torch.bool, device="cuda")
    o4, r4 = out.double().view(B, H, 1, 64), ref.view(B, H, 1, 64)
    P4 = P.view(B, H, 1, T)
    assert bool(torch.isfinite(o4).all()), what
    err = (o4 - r4).abs()
    bnd = _bound(r4, P4, V.abs(), vis)
    bad = err > bnd
    assert not bool(bad.any()), "%s: %d elements over budget, worst err / bound %.3g" % (what, int(bad.sum()), float((err / bnd).max()))
    if exact:
        _check_exact(o4, P4, V, what)


@pytest.mark.parametrize("shape", SQ_SHAPES, ids=[_id(s) for s in SQ_SHAPES])
def test_single_query_attention_matches_float64(ops, shape):
    T, causal, H, B = shape
    rs = np.random.RandomState(T + B)
    pos = _positions(B, T, causal, rs)
    seed = 5000 + T * 10 + H
    _check_single(ops, _planted(B, T, H, causal, "onehot", seed, stale=False), B, T, H, causal, pos, True, "one-hot %s" % _id(shape))
    if T > 1:
        _check_single(ops, _planted(B, T, H, causal, "hidden", seed + 1, stale=False), B, T, H, causal, pos, False,
                      "hidden keys %s" % _id(shape))
    _check_single(ops, _dense(B, T, H, seed + 2), B, T, H, causal, pos, False, "dense %s" % _id(shape))
    _check_single(ops, _planted(B, T, H, causal, "onehot", seed + 3, stale=False, q_scale=65504.0 / 8.0, k_scale=65504.0), B, T, H, causal, pos, True,
                  "largest scores %s" % _id(shape))


# ------------------------------------------------------------------------------------------------ what no kernel serves
@pytest.mark.parametrize("T,causal,H", [(200, True, 8), (150, True, 8), (97, False, 8), (97, True, 12), (192, False, 8), (225, False, 8),
                                        (300, False, 12), (224, True, 16), (32, False, 17)])
def test_attention_rejects_what_no_kernel_serves(ops, T, causal, H):
    from scd_amd._lib import ScdError
    qkv = torch.zeros((2 * T, 3 * 64 * H), dtype=torch.float16, device="cuda")
    with pytest.raises(ScdError) as e:
        ops.attention_f16(qkv, 2, T, H, causal)
    assert e.value.code == -1


def test_attention_rejects_bad_head_layouts(ops):
    from scd_amd import _lib
    from scd_amd._lib import ScdError
    qkv = torch.zeros((2 * 40, 3 * 512), dtype=torch.float16, device="cuda")
    out = torch.zeros((2 * 40, 512), dtype=torch.float16, device="cuda")
    L = _lib.load()
    h = _lib.handle(0)
    for width, heads in ((512, 7), (512, 0), (1088, 17)):
        assert L.scd_attention_f16(h, _lib.ptr(qkv), 2, 40, width, heads, 0, _lib.ptr(out), _lib.stream_ptr()) == _lib.SCD_EINVAL
    assert L.scd_attention_f16(h, _lib.ptr(qkv), 0, 40, 512, 8, 0, _lib.ptr(out), _lib.stream_ptr()) == _lib.SCD_EINVAL
    kv = torch.zeros((257, 2 * 512), dtype=torch.float16, device="cuda")
    q = torch.zeros((1, 512), dtype=torch.float16, device="cuda")
    with pytest.raises(ScdError):
        ops.attention_single_query_f16(kv, q, torch.zeros(1, dtype=torch.int32), 257, 8, False)
    with pytest.raises(ScdError):
        ops.attention_single_query_f16(kv[:200].contiguous(), q, None, 200, 8, True)      # causal needs the query rows
