"""The GEMM family of the encoder blocks kernel by kernel against float64 restatements (oracle/clip_oracle.py gemm_f64,
gemm_ln_folded_f64, ln_linear_f64, row_stats_int, patch_conv_f64, layernorm_f64, fold_ln_f64), through scd_gemm_f16 (with out=, so the
residual variants run in place as run_blocks runs them) and the test entry points scd_gemm_ln_apply_f16 (ln_finish_kernel +
gemm_w4_kernel LN = 1), scd_gemm_res_stats_f16 (LN = 2), scd_gemm_img_f16 (IMG), scd_fold_ln_f16 and scd_layernorm_f16.

A. Exact cases: torch.equal.  a in {-1, 0, 1}, w in {-2..2}, integer bias and residual, all fp16.  Each test first asserts on the
reference alone that max |c| <= 2048 and that sum_k |a_k w_k| (+ |bias| + |residual|), which bounds every intermediate sum, is below
2^24: then every product, every fp32 partial sum in any order and the fp16 result are exact, so a dropped, doubled or misplaced chunk,
tile, row or lane is a bit difference.  For the LN = 2 statistics |c| <= 256 on top (a wave's 128-column sum of squares stays below
2^24), and stats_out must equal {sum c * 2^24, sum c^2 * 2^20}.

B. Real-valued cases: per element against float64, with u = 2^-11 (fp16), v = 2^-24 (fp32):

  plain:   |c - ref| <= S * (L * (C1 * v * K_eff * sum_k |a_k w_k| + v * |pre|) + T_act(pre) + u * |x| + u * |x + r|) + 2^-24
    * the accumulation: the products of two fp16 numbers are exact in fp32; a product then passes through at most K_eff = K / 16 + 32
      fp32 additions - a chain of K / 16 v_mfma_f32_32x32x16_f16 (128-tile and LDS-DMA kernels; K / 32 v_mfma_f32_16x16x32_f16 in the
      four-wave kernel) plus at most 31 inside the instruction that sums its 16 / 32 products, in whatever order - C1 = 1;
    * pre = acc + bias: one packed fp32 addition, v * |pre|; L = 1.13 bounds the slope of both activations (1 without one);
    * T_act: QuickGELU x * rcp(1 + exp2(c x)): the product c x and the rounded constant (2 v |e| in the exponent e, i.e. a relative
      ln 2 * (1 - s) * 2 v |e| of the result, s the sigmoid), exp2 and rcp within one ulp (2 v each), the addition and the final
      product (v each): relative 6 v + ln 2 (1 - s) 2 v |e|.  gelu_erf_pair: the same shape with e = x p(x^2), p a degree-6 Horner
      form of seven packed fmas whose terms cancel: error v * (14 |x| sum_i |K_i| x^2i + 2 |e|) in e; plus the distance of the fitted
      formula from erf-GELU, computed on the CPU in float64 over [-40, 40] (gemm_cases.GELU_FIT, ~6e-7 absolute);
    * x = act(pre) is rounded to fp16 (u |x|); the residual variants add the fp16 residual and round again (u |x + r|; the 128-tile
      kernel adds in fp32 and rounds once, which is less);
    * S = 1 + 2^-9 covers second-order terms, 2^-24 the fp16 subnormal spacing.
  folded (LN = 1), against the float64 form of the same W', b', colsum and statistics:  pre = rstd * acc + nmr * colsum + b', and
    d pre <= rstd * C1 * v * K_eff * sum |a w'| + rho * |pre - b'| + 7 v * (|rstd acc| + |nmr colsum|) + 2 v |b'|
    * rho = the relative error of ln_finish_kernel's rstd: mean and E[x^2] each carry 3 v (int64 -> fp32, the rounded 1 / K, the
      product), so var = fma(-mean, mean, E[x^2]) is off by v * (3 E[x^2] + 6 mean^2 + var) <= 10 v E[x^2]; with kappa = E[x^2] /
      (var + eps) and t = 10 v kappa:  rho = t / (2 (1 - t)) + 2.5 v (the addition of eps, v_rsq_f32 within one ulp).  The rs output
      {rstd, nmr} is asserted directly: rstd within rho, nmr within rho + 4 v (the mean's 3 v and the product);
    * rstd is rounded once and nmr = -mean * rstd is formed from that same number, so rho is common to the two terms that cancel and
      moves their sum pre - b', not each of them.  What scales with the cancelling terms are the independent roundings only: 3 v of
      the mean and v of the product in nmr, v of nmr * colsum, v of the sum with b', up to 2 v of the final multiply-add: 7 v;
    * asserted for rows with kappa <= 2^18 (docs/design/gemm.md "Row conditioning of the folded LayerNorm"): beyond, t approaches 1
      and E[x^2] - mean^2 has no correct digit left in fp32.  Every row used here is below (gemm_cases.real_rows).
  true LayerNorm -> Linear (W' etc. from fold_ln_kernel, statistics = the exact row sums rounded to the fixed-point format): the folded
    budget with the rounding of sum x^2 to 2^-20 (t += 2^-21 / K / (var + eps)), plus rstd * sum_k |a_k - mean| (u |w_k gamma_k| +
    2^-25) for the fp16 rounding of W gamma, |nmr| * (K / 64 + 7) v sum |w'| for colsum and (K / 64 + 8) v (sum |beta w| + |b|) for b'
    (lane-strided fp32 sums, six wave-reduction steps).
  folded against unfused (layernorm_kernel -> scd_gemm_f16): within the SUM of the two budgets against the true form; the unfused
    budget is the plain one plus sum_k |d y_k| |w_k|, d y = layernorm_kernel's budget (gemm_cases.layernorm_error: two-pass fp32).

Shapes and run time: see EXACT_SHAPES / LAUNCH_SHAPES below.  Measured on the MI355X: the whole file (134 tests) takes 21 s, of which the three 786,432-row cases take under 1 s.
Operand memory at the 786,432-row cases (operands are freed between cases): fc2-like A 4.8 GB + C (= R, in place) 1.2 GB + the fp16
reference 1.2 GB + 0.7 GB of float64 chunk temporaries = 7.9 GB; QKV-like A 1.2 GB + C 3.6 GB + reference 3.6 GB + 0.8 GB = 9.2 GB peak.
"""
import numpy as np
import pytest
import torch

import gemm_cases as gc
from oracle import clip_oracle as co

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device; they must not be skipped on the GPU box"
    from scd_amd import ops as o
    return o


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host64(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ================================================================================================ A. exact cases
# (m, n, k): what each shape is there for.  Kernel reached: n % 256 == 128 -> gemm_f16_kernel; m % 256 == 128 -> gemm_dma_kernel<128>;
# otherwise gemm_w4_kernel.  Tiles = (m / 256) * (n / 256).
EXACT_SHAPES = [
    (128, 128, 64), (256, 384, 768), (384, 640, 192), (512, 1152, 1024),        # gemm_f16_kernel
    (128, 256, 128), (384, 768, 3072), (640, 512, 64), (1152, 2304, 768),        # gemm_dma_kernel<128>
    (256, 256, 64), (256, 256, 128), (512, 256, 192),                           # w4: nkc = 1 prologue, 2, 3 chunks; 1-2 tiles
    (256, 768, 768), (256, 1024, 1024), (256, 768, 3072), (256, 1024, 4096),    # w4: the encoders' depths; 3 / 4 tile columns
    (512, 2304, 128), (512, 3072, 128), (512, 4096, 64),                        # w4: 9 / 12 / 16 tile columns (one group), 18-32 tiles
    (768, 768, 128), (2560, 1280, 320),                                         # w4: 9 and 50 tiles: not multiples of 8
    (4096, 4096, 64), (16384, 1024, 128),                                       # w4: exactly 256 tiles
    (1280, 3072, 1024), (1280, 1024, 1024), (1280, 4096, 1024), (1280, 1024, 4096),   # ViT-L/14: 4 x 257 tokens padded, width 1024
]
# reference on the device in float64 (8,192 rows or more), two variants each: bias (non-residual) and bias + residual in place
EXACT_BIG_SHAPES = [
    (25600, 3072, 768),      # w4: 1,200 tiles = 4 * 256 + 176; choose_ng -> two groups of six tile columns
    (12800, 4096, 1024),     # w4: 800 tiles; choose_ng -> groups of 6, 6 and 4 tile columns
    (41472, 768, 128),       # 2 m n = 63.7e6: the last row count with plain stores
    (41728, 768, 128),       # 2 m n = 64.1e6: the first with non-temporal stores
]
# the bench's launch row count (3,990 images x 197 tokens padded to 256): one case per variant class
LAUNCH_SHAPES = [
    ("proj", 786432, 768, 768), ("fc2", 786432, 768, 3072), ("qkv", 786432, 2304, 768),
]


def _sid(s):
    return "x".join(str(v) for v in s)


def _ref_exact(a, w, bias, res):
    ref = co.gemm_f64(a, w, bias, 0, res)
    mag = np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
    if bias is not None:
        mag = mag + np.abs(bias)
    if res is not None:
        mag = mag + np.abs(res.astype(np.float64))
    gc.assert_exact_conditions(ref, mag)
    return torch.from_numpy(ref).half()


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=_sid)
def test_gemm_exact_every_variant(ops, shape):
    """every {bias, residual} combination, act = 0, out of place and in place: equal to the integer reference, bit for bit"""
    m, n, k = shape
    a, w, bias, res = gc.exact_operands(m, n, k, seed=m + 3 * n + 7 * k)
    refs = {(hb, hr): _ref_exact(a, w, bias if hb else None, res if hr else None) for hb in (0, 1) for hr in (0, 1)}
    da, dw, dbias, dres = dev(a), dev(w), dev(bias), dev(res)
    for (hb, hr), ref in refs.items():
        c = ops.gemm_f16(da, dw, dbias if hb else None, dres if hr else None, 0)
        assert torch.equal(c.cpu(), ref), "bias %d residual %d" % (hb, hr)
        if hr:
            x = dres.clone()
            assert ops.gemm_f16(da, dw, dbias if hb else None, x, 0, out=x) is x
            assert torch.equal(x, c), "in place differs from out of place (bias %d)" % hb
            assert torch.equal(dres.cpu(), torch.from_numpy(res))


def _device_exact(ops, m, n, k, seed, variants, stats=False):
    """operands drawn on the device; reference = float64 on the device in row chunks, kept as fp16 (exact: asserted <= 2048)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randint(-1, 2, (m, k), generator=g, device="cuda", dtype=torch.int8).half()
    w = torch.randint(-2, 3, (n, k), generator=g, device="cuda", dtype=torch.int8).half()
    bias = torch.randint(-8, 9, (n,), generator=g, device="cuda").float()
    for variant in variants:
        res = torch.randint(-8, 9, (m, n), generator=g, device="cuda", dtype=torch.int8).half() if variant == "bias_res_inplace" else None
        ref = torch.empty((m, n), dtype=torch.float16, device="cuda")
        for r0, c, mag in co.gemm_f64_device(a, w, bias, res):
            assert float(c.abs().max()) <= 2048 and float(mag.max()) < 2.0 ** 24
            ref[r0:r0 + c.shape[0]] = c.half()
        if res is None:
            c = ops.gemm_f16(a, w, bias, None, 0)
        else:
            c = ops.gemm_f16(a, w, bias, res, 0, out=res)
        torch.cuda.synchronize()
        assert torch.equal(c, ref), "%s %dx%dx%d: %d elements differ" % (variant, m, n, k, int((c != ref).sum()))
        del c, ref, res
    del a, w
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", EXACT_BIG_SHAPES, ids=_sid)
def test_gemm_exact_many_tiles(ops, shape):
    m, n, k = shape
    _device_exact(ops, m, n, k, seed=m + n + k, variants=("bias", "bias_res_inplace"))


@pytest.mark.parametrize("case", LAUNCH_SHAPES, ids=lambda c: c[0])
def test_gemm_exact_launch_row_count(ops, case):
    """786,432 rows (fc2's A operand is 4.8 GB: byte offsets beyond 32 bits), non-temporal stores in every variant"""
    name, m, n, k = case
    _device_exact(ops, m, n, k, seed=k + n, variants=("bias",) if name == "qkv" else ("bias_res_inplace",))


@pytest.mark.parametrize("ln", [1, 2])
def test_gemm_ln_exact_launch_row_count(ops, ln):
    """the LayerNorm variants at 786,432 rows, where C (and the statistics' rows) lie beyond 32-bit byte offsets: LN = 1 QKV-like
    (n = 2304, integer statistics as in test_gemm_ln_apply_exact_with_unit_statistics), LN = 2 proj-like in place with statistics"""
    m, k = 786432, 768
    n = 2304 if ln == 1 else 768
    g = torch.Generator(device="cuda").manual_seed(100 + ln)
    a = torch.randint(-1, 2, (m, k), generator=g, device="cuda", dtype=torch.int8)
    if ln == 2:
        a = a * (torch.rand((m, k), generator=g, device="cuda") < 0.25)
    a = a.half()
    w = torch.randint(-1, 2, (n, k), generator=g, device="cuda", dtype=torch.int8).half()
    bias = torch.randint(-8, 9, (n,), generator=g, device="cuda").float()
    ref = torch.empty((m, n), dtype=torch.float16, device="cuda")
    rows = torch.arange(m, device="cuda")
    if ln == 1:
        colsum = w.double().sum(1)
        scale = torch.where(rows % 3 == 0, 2.0, 1.0).double()
        mean = torch.where(rows % 3 == 2, 1.0, 0.0).double()
        for r0, c, mag in co.gemm_f64_device(a, w):
            sl = slice(r0, r0 + c.shape[0])
            c = scale[sl, None] * c - mean[sl, None] * colsum[None, :] + bias.double()
            assert float(c.abs().max()) <= 2048 and float((2 * mag + colsum.abs() + bias.abs()).max()) < 2.0 ** 24
            ref[sl] = c.half()
        stats = torch.zeros((m, 2), dtype=torch.int64, device="cuda")
        stats[:, 0] = (mean * k).long() << 24
        stats[:, 1] = torch.where(scale == 2.0, k // 4, torch.where(mean == 1.0, 2 * k, k)).long() << 20
        zero = torch.full((m, 2), 7, dtype=torch.int64, device="cuda")
        rs = torch.empty((m, 2), dtype=torch.float32, device="cuda")
        c = ops.gemm_ln_apply_f16(a, w, bias, colsum.float(), stats, 0.0, 0, rs=rs, zero_out=zero)
        torch.cuda.synchronize()
        assert torch.equal(rs, torch.stack([scale, -mean], 1).float()) and not bool(zero.any())
        assert torch.equal(c, ref), "%d elements differ" % int((c != ref).sum())
    else:
        res = torch.randint(-8, 9, (m, n), generator=g, device="cuda", dtype=torch.int8).half()
        want = torch.empty((m, 2), dtype=torch.int64, device="cuda")
        for r0, c, mag in co.gemm_f64_device(a, w, bias, res):
            assert float(c.abs().max()) <= 256 and float(mag.max()) < 2.0 ** 24
            ref[r0:r0 + c.shape[0]] = c.half()
            ci = c.long()
            want[r0:r0 + c.shape[0], 0] = ci.sum(1) << 24
            want[r0:r0 + c.shape[0], 1] = (ci * ci).sum(1) << 20
        pre = torch.stack([rows * 1000003 - 77, 5 - rows * 999983], 1)
        st = pre.clone()
        ops.gemm_res_stats_f16(a, w, bias, res, st, out=res)
        torch.cuda.synchronize()
        assert torch.equal(res, ref), "%d elements differ" % int((res != ref).sum())
        assert torch.equal(st - pre, want), "%d rows of statistics differ" % int((st - pre != want).any(1).sum())
    del a, w, ref
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ LN = 2: statistics
@pytest.mark.parametrize("shape", [(256, 256, 64), (512, 768, 768), (768, 768, 3072), (1280, 1024, 4096), (2560, 256, 320),
                                   (43520, 768, 128)], ids=_sid)
def test_gemm_stats_exact_and_accumulating(ops, shape):
    """proj / fc2 with statistics: C equals the integer reference (in place == out of place) and stats_out, pre-loaded with a non-zero
    pattern, grows by exactly {sum c * 2^24, sum c^2 * 2^20}; 2 / 6 / 8 partials per row; the same bits twice"""
    m, n, k = shape
    a, w, bias, res = gc.exact_operands(m, n, k, seed=11 * m + n + k, w_max=1, a_density=0.25)
    ref = co.gemm_f64(a, w, bias, 0, res)
    mag = np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64)).T + np.abs(bias) + np.abs(res.astype(np.float64))
    gc.assert_exact_conditions(ref, mag, cap=256)
    want = co.row_stats_int(ref)
    assert np.array_equal(want[:, 0], (ref.sum(1) * 2.0 ** 24).astype(np.int64)) and int(np.abs(want).max()) < 2 ** 62
    pre = (np.arange(2 * m, dtype=np.int64).reshape(m, 2) * 1000003 - 77) * np.array([[1, -1]])
    da, dw, dbias, dres = dev(a), dev(w), dev(bias), dev(res)
    outs = []
    for run in range(2):
        st = dev(pre)
        c = ops.gemm_res_stats_f16(da, dw, dbias, dres, st)
        x, st2 = dres.clone(), dev(pre)
        ops.gemm_res_stats_f16(da, dw, dbias, x, st2, out=x)
        torch.cuda.synchronize()
        assert torch.equal(c.cpu(), torch.from_numpy(ref).half())
        assert torch.equal(x, c), "in place differs from out of place"
        assert np.array_equal(st.cpu().numpy() - pre, want), "statistics are not the exact row sums added to what was there"
        assert torch.equal(st, st2)
        outs.append((c, st))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------ LN = 1 on integers
@pytest.mark.parametrize("shape", [(256, 256, 64), (512, 768, 768), (256, 2304, 768), (1280, 4096, 1024), (14080, 2304, 128)], ids=_sid)
def test_gemm_ln_apply_exact_with_unit_statistics(ops, shape):
    """LN = 1 with statistics that make rstd and mean small integers exactly (eps = 0): rows m % 3 == 1 have sum = 0, sum of squares
    = k (rstd 1, mean 0), rows m % 3 == 0 sum of squares k / 4 (rstd 2), rows m % 3 == 2 sum = k, sum of squares 2 k (mean 1, var 1:
    out = acc - colsum + b').  The tile walk, the per-row {rstd, nmr} loads, the colsum term and the stores are then checked bit for
    bit.  zero_out is cleared."""
    m, n, k = shape
    a, w, bias, _ = gc.exact_operands(m, n, k, seed=5 * m + n + 3 * k)
    colsum = w.astype(np.float64).sum(1).astype(np.float32)
    scale = np.where(np.arange(m) % 3 == 0, 2.0, 1.0)
    mean = np.where(np.arange(m) % 3 == 2, 1.0, 0.0)
    ref = scale[:, None] * (a.astype(np.float64) @ w.astype(np.float64).T) - mean[:, None] * colsum.astype(np.float64)[None, :] + bias
    mag = 2 * (np.abs(a.astype(np.float64)) @ np.abs(w.astype(np.float64)).T) + np.abs(colsum)[None, :] + np.abs(bias)
    gc.assert_exact_conditions(ref, mag)
    stats = np.zeros((m, 2), dtype=np.int64)
    stats[:, 0] = (mean * k).astype(np.int64) << 24
    stats[:, 1] = np.where(scale == 2.0, k // 4, np.where(mean == 1.0, 2 * k, k)) << 20
    zero = torch.full((m, 2), 12345, dtype=torch.int64, device="cuda")
    rs = torch.empty((m, 2), dtype=torch.float32, device="cuda")
    c = ops.gemm_ln_apply_f16(dev(a), dev(w), dev(bias), dev(colsum), dev(stats), 0.0, 0, rs=rs, zero_out=zero)
    torch.cuda.synchronize()
    assert np.array_equal(rs.cpu().numpy(), np.stack([scale, -mean], 1).astype(np.float32))
    assert torch.equal(c.cpu(), torch.from_numpy(ref).half())
    assert not bool(zero.any())


# ------------------------------------------------------------------------------------------------ IMG
# (image, batch, n): rows = batch * (image / 16)^2 below 256, not a multiple of 256, several thousand; the last case has 2 m n > 64e6
IMG_CASES = [(32, 5, 256), (224, 1, 768), (224, 3, 1024), (256, 2, 256), (32, 700, 768), (224, 20, 768), (256, 9, 1024), (224, 20, 256),
             (224, 220, 768)]


@pytest.mark.parametrize("case", IMG_CASES, ids=_sid)
def test_gemm_img_exact(ops, case):
    image, batch, n = case
    px, w = gc.img_pixels(batch, image, seed=image + batch + n), gc.img_weights(n)
    rows = batch * (image // 16) ** 2
    cols = co.im2col(px)
    ref = cols @ w.astype(np.float64).T
    assert np.array_equal(ref, co.patch_conv_f64(px, w))
    conv = torch.nn.functional.conv2d(torch.from_numpy(px).double(), torch.from_numpy(w).double().view(n, 3, 16, 16), stride=16)
    assert np.array_equal(conv.flatten(2).transpose(1, 2).reshape(rows, n).numpy(), ref)     # the restatement is the convolution
    gc.assert_exact_conditions(ref, np.abs(cols) @ np.abs(w.astype(np.float64)).T)
    c = ops.gemm_img_f16(dev(px), dev(w))
    m = c.shape[0]
    assert m % 256 == 0 and m >= rows
    padded = np.zeros((m, 768), dtype=np.float16)
    padded[:rows] = cols
    via_cols = ops.gemm_f16(dev(padded), dev(w))
    torch.cuda.synchronize()
    assert torch.equal(c[:rows].cpu(), torch.from_numpy(ref).half())
    assert torch.equal(c[:rows], via_cols[:rows])


# ------------------------------------------------------------------------------------------------ rejections
def test_gemm_family_rejects_before_launching(ops):
    """every rejected call returns SCD_EINVAL; all pointers are valid buffers of the largest shape named, so nothing could fault"""
    from scd_amd import _lib
    L, h, p, st = _lib.load(), _lib.handle(), _lib.ptr, _lib.stream_ptr()
    E = _lib.SCD_EINVAL
    a = torch.zeros((512, 512), dtype=torch.float16, device="cuda")
    w = torch.zeros((512, 512), dtype=torch.float16, device="cuda")
    c = torch.zeros((512, 512), dtype=torch.float16, device="cuda")
    r = torch.zeros((512, 512), dtype=torch.float16, device="cuda")
    f = torch.zeros(512, dtype=torch.float32, device="cuda")
    s = torch.zeros((512, 2), dtype=torch.int64, device="cuda")
    rs = torch.zeros((512, 2), dtype=torch.float32, device="cuda")
    for m, n, k in ((384, 256, 64), (256, 384, 64), (256, 256, 96), (0, 256, 64), (256, 0, 64)):
        assert L.scd_gemm_res_stats_f16(h, p(a), p(w), p(f), p(r), p(c), p(s), m, n, k, 0, st) == E, (m, n, k)
        assert L.scd_gemm_ln_apply_f16(h, p(a), p(w), p(f), p(f), p(s), p(rs), None, p(c), m, n, k, 1e-5, 0, st) == E, (m, n, k)
    for act in (1, 2):
        assert L.scd_gemm_res_stats_f16(h, p(a), p(w), p(f), p(r), p(c), p(s), 256, 256, 64, act, st) == E    # act with residual
    assert L.scd_gemm_res_stats_f16(h, p(a), p(w), None, p(r), p(c), p(s), 256, 256, 64, 0, st) == E           # missing bias
    assert L.scd_gemm_res_stats_f16(h, p(a), p(w), p(f), None, p(c), p(s), 256, 256, 64, 0, st) == E           # missing residual
    assert L.scd_gemm_res_stats_f16(h, p(a), p(w), p(f), p(r), p(a), p(s), 256, 256, 64, 0, st) == E           # C == A
    assert L.scd_gemm_res_stats_f16(h, p(a), p(w), p(f), p(r), p(c), None, 256, 256, 64, 0, st) == E
    assert L.scd_gemm_ln_apply_f16(h, p(a), p(w), None, p(f), p(s), p(rs), None, p(c), 256, 256, 64, 1e-5, 0, st) == E   # missing bias
    assert L.scd_gemm_ln_apply_f16(h, p(a), p(w), p(f), p(f), p(s), p(rs), None, p(a), 256, 256, 64, 1e-5, 0, st) == E   # C == A
    assert L.scd_gemm_ln_apply_f16(h, p(a), p(w), p(f), p(f), p(s), p(rs), None, p(c), 256, 256, 64, 1e-5, 3, st) == E
    assert L.scd_gemm_ln_apply_f16(h, p(a), p(w), p(f), p(f), None, p(rs), None, p(c), 256, 256, 64, 1e-5, 0, st) == E
    for m, n, k in ((192, 128, 64), (128, 192, 64), (128, 128, 96)):
        assert L.scd_gemm_f16(h, p(a), p(w), None, None, p(c), m, n, k, 0, st) == E
    assert L.scd_gemm_f16(h, p(a), p(w), None, None, p(a), 256, 256, 64, 0, st) == E
    px = torch.zeros((2, 3, 32, 32), dtype=torch.float16, device="cuda")
    w7 = torch.zeros((256, 768), dtype=torch.float16, device="cuda")
    for m, n, batch, image in ((128, 256, 2, 32), (256, 128, 2, 32), (256, 256, 2, 24), (256, 256, 0, 32), (256, 256, 2, 0),
                               (256, 256, 65, 32), (256, 0, 2, 32)):
        assert L.scd_gemm_img_f16(h, p(px), p(w7), p(c), m, n, batch, image, st) == E, (m, n, batch, image)
    for rows, width in ((4, 320), (4, 0), (0, 256), (4, 1280), (4, 128)):
        assert L.scd_layernorm_f16(h, p(a), None, rows, width, 1e-5, p(f), p(f), p(c), st) == E, (rows, width)
    assert L.scd_layernorm_f16(h, p(a), None, 4, 256, 1e-5, p(f), p(f), p(a), st) == E
    assert L.scd_fold_ln_f16(h, p(w), p(f), p(f), p(f), 0, 64, p(c), p(f), p(f), st) == E
    assert L.scd_fold_ln_f16(h, p(w), p(f), p(f), p(f), 64, 64, p(w), p(f), p(f), st) == E
    torch.cuda.synchronize()
    assert not bool(c.any()) and not bool(a.any())


# ================================================================================================ B. real-valued cases
def _over(c, ref, bnd, what):
    err = np.abs(host64(c) - ref)
    assert np.isfinite(err).all(), what
    ratio = float((err / bnd).max())
    print("%s: worst err / budget %.3f" % (what, ratio))
    assert ratio <= 1.0, "%s: %d elements over budget, worst err / budget %.3g" % (what, int((err > bnd).sum()), ratio)


@pytest.mark.parametrize("shape", [(128, 128, 64), (256, 384, 768), (384, 768, 3072), (512, 768, 768), (1024, 2304, 768),
                                   (256, 256, 64), (768, 512, 192), (512, 1024, 4096), (1280, 1024, 1024)], ids=_sid)
@pytest.mark.parametrize("variant", ["plain", "bias", "bias_qgelu", "bias_gelu", "res", "bias_res"])
def test_gemm_real_within_budget(ops, shape, variant):
    m, n, k = shape
    rs = np.random.RandomState(m + n + k)
    a, _ = gc.real_rows(m, k, seed=m + k)
    w = gc.f16(rs.randn(n, k) * k ** -0.5)
    bias = rs.randn(n).astype(np.float32) if "bias" in variant else None
    res = gc.f16(rs.randn(m, n) * 2.0 ** rs.randint(-6, 3, size=(m, 1))) if "res" in variant else None
    act = 1 if "qgelu" in variant else 2 if "gelu" in variant else 0
    ref = co.gemm_f64(a, w, bias, act, res)
    bnd = gc.budget_plain(a, w, bias, act, res)
    c = ops.gemm_f16(dev(a), dev(w), None if bias is None else dev(bias), None if res is None else dev(res), act)
    _over(c, ref, bnd, "%s %s" % (variant, _sid(shape)))
    if res is not None and m % 256 == 0 and n % 256 == 0 and bias is not None:
        st = torch.zeros((m, 2), dtype=torch.int64, device="cuda")
        c2 = ops.gemm_res_stats_f16(dev(a), dev(w), dev(bias), dev(res), st)
        assert torch.equal(c2, c), "LN = 2 stores other values than the plain residual variant"
        # the statistics of the stored rows: per 128-column partial exact products, four v_dot2 of at most two roundings each and
        # four DPP additions in fp32 (12 v, taken as 13), then one rounding to fixed point (half a unit per partial, taken as one)
        want = co.row_stats_int(c2)
        c64 = host64(c2)
        tol1 = 13 * gc.U32 * np.abs(c64).sum(1) * 2.0 ** 24 + n / 128
        tol2 = 13 * gc.U32 * (c64 * c64).sum(1) * 2.0 ** 20 + n / 128
        got = st.cpu().numpy()
        assert (np.abs(got[:, 0] - want[:, 0]) <= tol1).all() and (np.abs(got[:, 1] - want[:, 1]) <= tol2).all()


@pytest.mark.parametrize("shape", [(512, 768, 768), (256, 2304, 768), (512, 3072, 768), (256, 1024, 1024), (512, 256, 320)], ids=_sid)
@pytest.mark.parametrize("act", [0, 1, 2])
def test_gemm_ln_folded_and_true_within_budget(ops, shape, act):
    """LN = 1 from fold_ln_kernel's operands and the exact fixed-point statistics of the rows: against the float64 folded form, against
    the true LayerNorm -> Linear, and against the unfused kernels (layernorm_kernel -> scd_gemm_f16)"""
    m, n, k = shape
    eps = 1e-5 if act != 2 else 1e-6
    a, kind = gc.real_rows(m, k, seed=3 * m + k)
    w, gamma, beta, bias = gc.real_layer(n, k, seed=n + k)
    stats = co.row_stats_int(a)
    wf, colsum, biasf = ops.fold_ln_f16(dev(w), dev(gamma), dev(beta), dev(bias))
    zero = torch.full((m, 2), -1, dtype=torch.int64, device="cuda")
    rs = torch.empty((m, 2), dtype=torch.float32, device="cuda")
    c = ops.gemm_ln_apply_f16(dev(a), wf, biasf, colsum, dev(stats), eps, act, rs=rs, zero_out=zero)
    torch.cuda.synchronize()
    assert not bool(zero.any())
    wf_h, cs_h, bf_h = host64(wf), host64(colsum), host64(biasf)
    ref, parts = co.gemm_ln_folded_f64(a, wf_h, bf_h, cs_h, stats, eps, act)
    _, kappa = gc.rstd_rel_error(parts, eps, k, False)
    assert float(kappa.max()) <= gc.KAPPA_LIMIT
    assert float(parts["var"][kind == 5].max()) == 0.0 and float(parts["var"][kind == 6].max()) == 0.0      # constant and zero rows
    what = "act %d %s" % (act, _sid(shape))
    # ln_finish_kernel on its own: {rstd, -mean * rstd} within rho / rho + 4 v of float64, ill-conditioned rows included
    rho, _ = gc.rstd_rel_error(parts, eps, k, False)
    rs_h, nmr = host64(rs), -parts["mean"] * parts["rstd"]
    r_rstd = np.abs(rs_h[:, 0] - parts["rstd"]) / (rho * parts["rstd"])
    r_nmr = np.abs(rs_h[:, 1] - nmr) / ((rho + 4 * gc.U32) * np.abs(nmr) + 2.0 ** -126)
    print("rs %s: worst rstd err / rho %.3f, nmr %.3f; by row kind (rstd) %s" % (
        what, r_rstd.max(), r_nmr.max(), " ".join("%s %.2f" % (gc.ROW_KINDS[i], r_rstd[kind == i].max()) for i in range(7))))
    assert r_rstd.max() <= 1.0 and r_nmr.max() <= 1.0
    b_fold = gc.budget_folded(a, wf_h, bf_h, cs_h, parts, eps, act)
    _over(c, ref, b_fold, "folded " + what)
    for i in (4, 5):
        _over(c[torch.from_numpy(kind == i).cuda()], ref[kind == i], b_fold[kind == i], "folded %s rows %s" % (gc.ROW_KINDS[i], what))
    true = co.ln_linear_f64(a, w, gamma, beta, bias, eps, act)
    b_true = gc.budget_true(a, w, gamma, beta, bias, wf_h, bf_h, cs_h, parts, eps, act)
    _over(c, true, b_true, "true " + what)
    if k % 256 == 0:
        y = ops.layernorm_f16(dev(a), dev(gamma), dev(beta), eps)
        unf = ops.gemm_f16(y, dev(w), dev(bias), None, act)
        b_unf = gc.budget_unfused(a, w, gamma, beta, bias, eps, act)
        _over(unf, true, b_unf, "unfused " + what)
        _over(c, host64(unf), b_true + b_unf, "folded vs unfused " + what)


@pytest.mark.parametrize("width", [256, 512, 768, 1024])
def test_layernorm_within_budget(ops, width):
    rows = 263
    x, _ = gc.real_rows(rows, width, seed=width)
    _, gamma, beta, _ = gc.real_layer(8, width, seed=width + 1)
    for eps in (1e-5, 1e-6):
        y = ops.layernorm_f16(dev(x), dev(gamma), dev(beta), eps)
        _over(y, co.layernorm_f64(x, gamma, beta, eps), gc.layernorm_error(x, gamma, beta, eps), "layernorm %d" % width)
        idx = np.array([5, 5, 0, 262, 7, 7, 7, 100, 3, 261, 5], dtype=np.int32)       # repeats and skips rows
        yi = ops.layernorm_f16(dev(x), dev(gamma), dev(beta), eps, row_index=torch.from_numpy(idx))
        assert yi.shape == (len(idx), width) and torch.equal(yi, y[torch.from_numpy(idx).long().cuda()])


def test_layernorm_rejects_width_320(ops):
    """layernorm_kernel walks 256-column groups (the encoders require width % 256 == 0): width 320 is refused, not half served"""
    from scd_amd._lib import ScdError
    x = torch.zeros((8, 320), dtype=torch.float16, device="cuda")
    g = torch.ones(320, device="cuda")
    with pytest.raises(ScdError) as e:
        ops.layernorm_f16(x, g, g, 1e-5)
    assert e.value.code == -1


@pytest.mark.parametrize("shape", [(2304, 768), (3072, 768), (4096, 1024), (1283, 320), (7, 1024), (961, 768)], ids=_sid)
def test_fold_ln_within_budget(ops, shape):
    n, k = shape
    w, gamma, beta, bias = gc.real_layer(n, k, seed=n + 2 * k)
    wf, colsum, biasf = ops.fold_ln_f16(dev(w), dev(gamma), dev(beta), dev(bias))
    wg, bf = co.fold_ln_f64(w, gamma, beta, bias)
    d_w, d_cs, d_b = gc.fold_errors(w, gamma, beta, bias)
    assert (np.abs(host64(wf) - wg) <= d_w).all()
    assert (np.abs(host64(colsum) - host64(wf).sum(1)) <= d_cs + gc.U32 * np.abs(host64(colsum))).all()
    assert (np.abs(host64(biasf) - bf) <= d_b + gc.U32 * np.abs(bf)).all()
    # exact on integers: gamma in {1, 2, -1}, beta integers
    rs = np.random.RandomState(n)
    wi = rs.randint(-3, 4, size=(n, k)).astype(np.float16)
    gi = rs.choice([1.0, 2.0, -1.0], size=k).astype(np.float32)
    bi = rs.randint(-2, 3, size=k).astype(np.float32)
    bb = rs.randint(-9, 10, size=n).astype(np.float32)
    wf, colsum, biasf = ops.fold_ln_f16(dev(wi), dev(gi), dev(bi), dev(bb))
    wg, bf = co.fold_ln_f64(wi, gi, bi, bb)
    assert np.array_equal(host64(wf), wg) and np.array_equal(host64(colsum), wg.sum(1)) and np.array_equal(host64(biasf), bf)
