"""Plain torch restatement of the DINOv2 ViT-*/14 forward (facebookresearch/dinov2 state-dict layout, docs/design/dinov2.md) in a
given dtype: what the device towers and the load-time folds of scd_amd/clip/weights.py are tested against.

It knows nothing of the folds: LayerScale is applied as a multiplication where the `ls1.gamma` / `ls2.gamma` keys exist (and skipped
where a fold removed them), the pixels are taken as they come, and a `pos_embed` that does not have 1 + (image / patch)^2 rows is
resampled here, with its own F.interpolate call.
"""
import torch
import torch.nn.functional as F

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def normalise(raw, mean, std):
    """raw [B,3,H,W] in [0,1] -> (raw - mean) / std, in raw's dtype"""
    m = torch.tensor(mean, dtype=raw.dtype).view(1, 3, 1, 1)
    s = torch.tensor(std, dtype=raw.dtype).view(1, 3, 1, 1)
    return (raw - m) / s


def interpolate_pos(pos_embed, grid_out, mode):
    """pos_embed [1, 1 + G^2, W] -> float32 [1, 1 + grid_out^2, W]; the three modes of the loader's pos_interp."""
    pe = pos_embed.float()
    rows, width = pe.shape[1], pe.shape[2]
    if rows == grid_out * grid_out + 1:
        return pe
    G = int(round((rows - 1) ** 0.5))
    grid = pe[:, 1:].reshape(1, G, G, width).permute(0, 3, 1, 2)
    if mode == "size_antialias":
        out = F.interpolate(grid, size=(grid_out, grid_out), mode="bicubic", antialias=True, align_corners=False)
    elif mode == "size":
        out = F.interpolate(grid, size=(grid_out, grid_out), mode="bicubic", antialias=False, align_corners=False)
    elif mode == "offset":
        s = float(grid_out + 0.1) / G
        out = F.interpolate(grid, scale_factor=(s, s), mode="bicubic", antialias=False)
    else:
        raise ValueError(mode)
    return torch.cat([pe[:, :1], out.permute(0, 2, 3, 1).reshape(1, grid_out * grid_out, width)], dim=1)


def n_blocks(sd):
    i = 0
    while ("blocks.%d.norm1.weight" % i) in sd:
        i += 1
    return i


@torch.no_grad()
def forward(sd, x, dtype=torch.float32, pos_interp="size_antialias", heads=None, head_dim=64):
    """sd: DINOv2 state dict (any float dtype), x [B,3,H,W] -> norm(tokens)[:, 0] [B, W] in `dtype`.
    Tokens: [cls + pos[0]] | [registers, no position] | [patch + bias + pos[1 + p]]; block: x += ls1 * attn(norm1 x); x += ls2 *
    mlp(norm2 x); LayerNorm eps 1e-6, exact (erf) GELU, QKV bias."""
    g = lambda k: sd[k].to(dtype)
    w = g("patch_embed.proj.weight")
    width, patch = w.shape[0], w.shape[-1]
    heads = heads or width // head_dim
    hd = width // heads
    x = x.to(dtype)
    b = x.shape[0]
    grid = x.shape[-1] // patch
    tok = F.conv2d(x, w, g("patch_embed.proj.bias"), stride=patch).flatten(2).transpose(1, 2)           # [B, np, W]
    pos = interpolate_pos(sd["pos_embed"], grid, pos_interp).to(dtype)
    parts = [g("cls_token").expand(b, -1, -1) + pos[:, :1]]
    if "register_tokens" in sd:
        parts.append(g("register_tokens").expand(b, -1, -1))
    parts.append(tok + pos[:, 1:])
    h = torch.cat(parts, dim=1)
    T = h.shape[1]
    for i in range(n_blocks(sd)):
        p = "blocks.%d." % i
        y = F.layer_norm(h, (width,), g(p + "norm1.weight"), g(p + "norm1.bias"), 1e-6)
        qkv = (y @ g(p + "attn.qkv.weight").t() + g(p + "attn.qkv.bias")).view(b, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
        att = torch.softmax((qkv[0] @ qkv[1].transpose(-2, -1)) * hd ** -0.5, dim=-1)
        y = (att @ qkv[2]).transpose(1, 2).reshape(b, T, width)
        y = y @ g(p + "attn.proj.weight").t() + g(p + "attn.proj.bias")
        if p + "ls1.gamma" in sd:
            y = y * g(p + "ls1.gamma")
        h = h + y
        y = F.layer_norm(h, (width,), g(p + "norm2.weight"), g(p + "norm2.bias"), 1e-6)
        y = F.gelu(y @ g(p + "mlp.fc1.weight").t() + g(p + "mlp.fc1.bias"))
        y = y @ g(p + "mlp.fc2.weight").t() + g(p + "mlp.fc2.bias")
        if p + "ls2.gamma" in sd:
            y = y * g(p + "ls2.gamma")
        h = h + y
    return F.layer_norm(h, (width,), g("norm.weight"), g("norm.bias"), 1e-6)[:, 0]


def round_like_the_device(sd):
    """What the tower holds of a PREPARED state dict (weights.prepare_dinov2): matrices and the patch kernel in fp16, vectors, the class
    token, the register rows and the position table in fp32."""
    keep = ("pos_embed", "cls_token", "register_tokens")
    return {k: (v.half().float() if v.dim() >= 2 and k not in keep else v.float()) for k, v in sd.items()}
