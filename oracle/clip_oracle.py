"""CPU oracle (torch, float32) for the encoder part of the hot path.

TEST INFRASTRUCTURE ONLY - never imported from scd_amd/.

* CLIP ViT-B/16 visual / text towers: the arithmetic lives in the third-party
  package `clip==1.0` (openai/CLIP, requirements.txt:27), which is NOT under
  /root/reference and not installed; call sites main_unsup.py:237,127 and
  local_utils/clip_lang_util.py:101-102.  This file restates the published
  model.py structure.  It is pinned against
  transformers.CLIPModel (an independent implementation of the same published
  architecture) on shared seeded random weights: tests/golden/clip_hf.npz,
  produced by oracle/gen_golden.py.  Parity against the true package/weights
  is unpinned (no checkpoint offline).
* DINO ViT-B/16: restates /root/reference/gcd/models/vision_transformer.py
  (VisionTransformer :135-219, Attention :67-91, Block :94-114, PatchEmbed
  :117-132), pinned against that file run in the build container
  (tests/golden/dino_ref.npz).

Weights are dicts keyed with the reference state-dict names.

* The GEMM family of the encoder blocks (tests/test_gpu_gemm.py, tests/test_gemm_budget_sensitivity.py): one plain numpy float64
  function per operation, no tiling - gemm_f64, gemm_ln_folded_f64, ln_linear_f64, row_stats_int, im2col / patch_conv_f64,
  layernorm_f64, fold_ln_f64.  Seven exact (integer) GEMM cases - the 25,600 / 12,800 / 41,472 / 41,728-row corner shapes and
  the three 786,432-row launch shapes of test_gpu_gemm.py - take their reference from gemm_f64_device instead: the same product in
  float64 on the device in row chunks through torch.matmul, which shares nothing with the library under test.
"""
import math
import numpy as np
import torch
import torch.nn.functional as F


def _ln(x, w, b, eps):
    return F.layer_norm(x.float(), (x.shape[-1],), w.float(), b.float(), eps)


def _act(x, kind):
    if kind == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)        # CLIP QuickGELU
    return F.gelu(x)                                # nn.GELU (vision_transformer.py:49)


def _attention(x, qkv_w, qkv_b, out_w, out_b, heads, causal):
    b, t, c = x.shape
    qkv = x @ qkv_w.float().t() + qkv_b.float()
    q, k, v = qkv.view(b, t, 3, heads, c // heads).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * (c // heads) ** -0.5
    if causal:
        s = s + torch.full((t, t), float("-inf")).triu_(1)
    p = s.softmax(dim=-1)
    o = (p @ v).transpose(1, 2).reshape(b, t, c)
    return o @ out_w.float().t() + out_b.float()


def attention_f64(qkv, batch, T, heads, causal):
    """float64 restatement of the encoder blocks' attention core on the fp16 values a kernel reads (scd_attention_f16):
    qkv [batch*T, 3*width] (Q | K | V, heads in 64-wide slices) -> per (sequence, head) P = softmax(Q K^T / 8) with query t
    seeing keys 0..t when causal, O = P V.  Returns O [batch*T, width] and P [batch, heads, T, T], both float64, on qkv's device."""
    width = qkv.shape[1] // 3
    q, k, v = qkv.double().view(batch, T, 3, heads, width // heads).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * (width // heads) ** -0.5
    if causal:
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool, device=s.device).triu_(1), float("-inf"))
    p = s.softmax(dim=-1)
    return (p @ v).transpose(1, 2).reshape(batch * T, width), p


def attention_single_query_f64(kv, q, pos, T, heads, causal):
    """float64 restatement of the last block's one-query attention (scd_attention_single_query_f16): kv [batch*T, 2*width]
    (K | V), q [batch, width], pos[b] = the query's position (causal: it sees keys 0..pos[b]).  Returns O [batch, width] and
    P [batch, heads, T], float64."""
    batch, width = q.shape
    k, v = kv.double().view(batch, T, 2, heads, width // heads).permute(2, 0, 3, 1, 4)
    s = (k @ q.double().view(batch, heads, width // heads, 1)).squeeze(-1) * (width // heads) ** -0.5
    if causal:
        keys = torch.arange(T, device=s.device)
        s = s.masked_fill(keys.view(1, 1, T) > torch.as_tensor(pos, device=s.device).view(batch, 1, 1), float("-inf"))
    p = s.softmax(dim=-1)
    return (p.unsqueeze(2) @ v).reshape(batch, width), p


def _block(x, g, heads, act, eps, causal):
    """g(name) -> tensor for the canonical per-block names."""
    x = x + _attention(_ln(x, g("ln1_w"), g("ln1_b"), eps), g("qkv_w"), g("qkv_b"), g("proj_w"), g("proj_b"),
                       heads, causal)
    h = _ln(x, g("ln2_w"), g("ln2_b"), eps) @ g("fc1_w").float().t() + g("fc1_b").float()
    return x + _act(h, act) @ g("fc2_w").float().t() + g("fc2_b").float()


_CLIP_BLOCK = {"ln1_w": "ln_1.weight", "ln1_b": "ln_1.bias", "qkv_w": "attn.in_proj_weight",
               "qkv_b": "attn.in_proj_bias", "proj_w": "attn.out_proj.weight", "proj_b": "attn.out_proj.bias",
               "ln2_w": "ln_2.weight", "ln2_b": "ln_2.bias", "fc1_w": "mlp.c_fc.weight", "fc1_b": "mlp.c_fc.bias",
               "fc2_w": "mlp.c_proj.weight", "fc2_b": "mlp.c_proj.bias"}
_DINO_BLOCK = {"ln1_w": "norm1.weight", "ln1_b": "norm1.bias", "qkv_w": "attn.qkv.weight", "qkv_b": "attn.qkv.bias",
               "proj_w": "attn.proj.weight", "proj_b": "attn.proj.bias", "ln2_w": "norm2.weight",
               "ln2_b": "norm2.bias", "fc1_w": "mlp.fc1.weight", "fc1_b": "mlp.fc1.bias",
               "fc2_w": "mlp.fc2.weight", "fc2_b": "mlp.fc2.bias"}


def _n_blocks(sd, prefix):
    i = 0
    while any(k.startswith("%s%d." % (prefix, i)) for k in sd):
        i += 1
    return i


@torch.no_grad()
def clip_encode_image(sd, images, heads=12):
    """VisionTransformer.forward of openai/CLIP model.py (appendix B 'Visual')."""
    x = F.conv2d(images.float(), sd["visual.conv1.weight"].float(), stride=sd["visual.conv1.weight"].shape[-1])
    b, c = x.shape[:2]
    x = x.reshape(b, c, -1).permute(0, 2, 1)
    cls = sd["visual.class_embedding"].float().expand(b, 1, c)
    x = torch.cat([cls, x], dim=1) + sd["visual.positional_embedding"].float()
    x = _ln(x, sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"], 1e-5)
    for i in range(_n_blocks(sd, "visual.transformer.resblocks.")):
        p = "visual.transformer.resblocks.%d." % i
        x = _block(x, lambda n: sd[p + _CLIP_BLOCK[n]], heads, "quick_gelu", 1e-5, False)
    x = _ln(x[:, 0], sd["visual.ln_post.weight"], sd["visual.ln_post.bias"], 1e-5)
    return x @ sd["visual.proj"].float()


@torch.no_grad()
def clip_encode_text(sd, tokens, heads=8):
    """CLIP.encode_text (appendix B 'Text'): EOT row = argmax token id."""
    x = sd["token_embedding.weight"].float()[tokens.long()] + sd["positional_embedding"].float()
    for i in range(_n_blocks(sd, "transformer.resblocks.")):
        p = "transformer.resblocks.%d." % i
        x = _block(x, lambda n: sd[p + _CLIP_BLOCK[n]], heads, "quick_gelu", 1e-5, True)
    x = _ln(x, sd["ln_final.weight"], sd["ln_final.bias"], 1e-5)
    x = x[torch.arange(x.shape[0]), tokens.long().argmax(dim=-1)]
    return x @ sd["text_projection"].float()


@torch.no_grad()
def dino_forward(sd, images, heads=12):
    """gcd/models/vision_transformer.py:210-219 (prepare_tokens, blocks, norm, [:,0])."""
    w = sd["patch_embed.proj.weight"].float()
    x = F.conv2d(images.float(), w, sd["patch_embed.proj.bias"].float(), stride=w.shape[-1])
    b, c = x.shape[:2]
    x = x.flatten(2).transpose(1, 2)
    x = torch.cat([sd["cls_token"].float().expand(b, -1, -1), x], dim=1) + sd["pos_embed"].float()
    for i in range(_n_blocks(sd, "blocks.")):
        p = "blocks.%d." % i
        x = _block(x, lambda n: sd[p + _DINO_BLOCK[n]], heads, "gelu", 1e-6, False)
    return _ln(x, sd["norm.weight"], sd["norm.bias"], 1e-6)[:, 0]


# ------------------------------------------------------------------------------------------------ the blocks' GEMM family, float64
def _np64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def act_f64(x, act):
    """0: identity, 1: QuickGELU x sigmoid(1.702 x), 2: erf-GELU x Phi(x) (cancellation-free in both tails)."""
    x = np.asarray(x, dtype=np.float64)
    if act == 0:
        return x
    if act == 1:
        with np.errstate(over="ignore"):
            return x / (1.0 + np.exp(-1.702 * x))
    from scipy.special import erfc
    return np.where(x >= 0, x - 0.5 * x * erfc(x / math.sqrt(2.0)), 0.5 * x * erfc(-x / math.sqrt(2.0)))


def gemm_f64(a, w, bias=None, act=0, residual=None):
    """C = act(a @ w^T + bias) + residual; a [m, k], w [n, k] (torch Linear layout)."""
    c = _np64(a) @ _np64(w).T
    if bias is not None:
        c = c + _np64(bias)
    c = act_f64(c, act)
    if residual is not None:
        c = c + _np64(residual)
    return c


def stats_moments(stats, k):
    """{mean, E[x^2]} of rows of length k from the fixed-point sums stats int64 [m, 2] = {sum * 2^24, sum of squares * 2^20}."""
    st = np.asarray(stats.cpu().numpy() if isinstance(stats, torch.Tensor) else stats, dtype=np.int64)
    return st[:, 0].astype(np.float64) * 2.0 ** -24 / k, st[:, 1].astype(np.float64) * 2.0 ** -20 / k


def gemm_ln_folded_f64(a, wf, biasf, colsum, stats, eps, act=0):
    """The folded LayerNorm -> Linear from the folded operands: rstd * (a @ wf^T - mean * colsum) + biasf, then the activation, with
    mean and var = max(E[x^2] - mean^2, 0) from the fixed-point row sums.  Returns the result and the parts a budget needs."""
    a, wf = _np64(a), _np64(wf)
    mean, ex2 = stats_moments(stats, a.shape[1])
    var = np.maximum(ex2 - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    acc = a @ wf.T
    pre = rstd[:, None] * acc - (mean * rstd)[:, None] * _np64(colsum)[None, :] + _np64(biasf)[None, :]
    return act_f64(pre, act), dict(pre=pre, acc=acc, mean=mean, ex2=ex2, var=var, rstd=rstd)


def layernorm_f64(x, gamma, beta, eps, row_index=None):
    """(x - mean) / sqrt(var + eps) * gamma + beta over the last axis (biased variance); row_index selects / repeats input rows."""
    x = _np64(x)
    if row_index is not None:
        x = x[np.asarray(row_index, dtype=np.int64)]
    mean = x.mean(-1, keepdims=True)
    d = x - mean
    var = (d * d).mean(-1, keepdims=True)
    return d / np.sqrt(var + eps) * _np64(gamma) + _np64(beta)


def ln_linear_f64(a, w, gamma, beta, bias, eps, act=0):
    """The true LayerNorm -> Linear -> activation from the unfolded parameters."""
    return act_f64(layernorm_f64(a, gamma, beta, eps) @ _np64(w).T + _np64(bias), act)


def fold_ln_f64(w, gamma, beta, bias):
    """W gamma (unrounded) and b + W beta."""
    w = _np64(w)
    return w * _np64(gamma)[None, :], _np64(bias) + w @ _np64(beta)


def row_stats_int(c):
    """The fixed-point statistics of the rows of an fp16 matrix as exact integers, int64 [m, 2]: {sum * 2^24, sum of squares * 2^20
    rounded to nearest (exact for integer-valued rows)}.  fp16 values are multiples of 2^-24, so the arithmetic is integer."""
    c = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
    c = c.astype(np.float64)
    n = np.rint(c * 2.0 ** 24)
    assert np.array_equal(n, c * 2.0 ** 24) and np.abs(n).max(initial=0) < 2.0 ** 41
    out = np.zeros((c.shape[0], 2), dtype=np.int64)
    out[:, 0] = n.astype(np.int64).sum(1)
    if np.array_equal(np.rint(c), c):
        out[:, 1] = (c.astype(np.int64) ** 2).sum(1) << 20
    else:
        for i, row in enumerate(n.astype(np.int64)):
            s48 = sum(int(v) * int(v) for v in row)                   # units of 2^-48
            q, r = divmod(s48, 1 << 28)
            out[i, 1] = q + (1 if (r > (1 << 27) or (r == (1 << 27) and q & 1)) else 0)
    return out


def im2col(pixels, patch=16):
    """[b, 3, h, w] -> [b * (h/p) * (w/p), 3 p p]: row = (b, py, px), column = c p p + i p + j (conv1.weight.reshape(width, -1))."""
    x = _np64(pixels)
    b, ch, hh, ww = x.shape
    gy, gx = hh // patch, ww // patch
    x = x.reshape(b, ch, gy, patch, gx, patch).transpose(0, 2, 4, 1, 3, 5)
    return np.ascontiguousarray(x).reshape(b * gy * gx, ch * patch * patch)


def patch_conv_f64(pixels, w, patch=16):
    """The stride-p patch convolution without bias as rows of tokens: [b * gp^2, n], w [n, 3 p p]."""
    return im2col(pixels, patch) @ _np64(w).T


def gemm_f64_device(a, w, bias=None, residual=None, chunk=16384):
    """gemm_f64 without activation for operands on the device, float64 torch.matmul over row chunks: yields (row0, C chunk, sum_k |a w|
    chunk).  For the shapes whose float64 product would take minutes on the host."""
    w64, wabs = w.double().t().contiguous(), w.double().abs().t().contiguous()
    for r0 in range(0, a.shape[0], chunk):
        a64 = a[r0:r0 + chunk].double()
        c = a64 @ w64
        mag = a64.abs() @ wabs
        if bias is not None:
            c += bias.double()
            mag += bias.double().abs()
        if residual is not None:
            c += residual[r0:r0 + chunk].double()
            mag += residual[r0:r0 + chunk].double().abs()
        yield r0, c, mag
