"""Seeded random-init weights with the reference state-dict key names.

There are no checkpoints offline (the reference ships only download links:
zeroshot_weights/download_link.txt, GCD_pretrained_weights_VIT16/download_link.txt),
so benchmarks and parity tests use these.  The init follows the published
CLIP.initialize_parameters scales; biases and LayerNorm
parameters are perturbed so every fused epilogue term is exercised.
Real checkpoints with the same keys load through the same code path.
"""
import math
import re

import torch

CLIP_VITB16 = dict(embed_dim=512, image=224, patch=16, v_width=768, v_layers=12, v_heads=12,
                   context=77, vocab=49408, t_width=512, t_layers=12, t_heads=8)
CLIP_VITL14 = dict(embed_dim=768, image=224, patch=14, v_width=1024, v_layers=24, v_heads=16,
                   context=77, vocab=49408, t_width=768, t_layers=12, t_heads=12)


def _block(sd, g, prefix, width, layers, names):
    attn_std = width ** -0.5
    proj_std = (width ** -0.5) * ((2 * layers) ** -0.5)
    fc_std = (2 * width) ** -0.5
    r = lambda *s, std=1.0: torch.randn(*s, generator=g) * std
    sd[prefix + names["ln1_w"]] = 1.0 + 0.1 * r(width)
    sd[prefix + names["ln1_b"]] = 0.02 * r(width)
    sd[prefix + names["qkv_w"]] = r(3 * width, width, std=attn_std)
    sd[prefix + names["qkv_b"]] = 0.02 * r(3 * width)
    sd[prefix + names["proj_w"]] = r(width, width, std=proj_std)
    sd[prefix + names["proj_b"]] = 0.02 * r(width)
    sd[prefix + names["ln2_w"]] = 1.0 + 0.1 * r(width)
    sd[prefix + names["ln2_b"]] = 0.02 * r(width)
    sd[prefix + names["fc1_w"]] = r(4 * width, width, std=fc_std)
    sd[prefix + names["fc1_b"]] = 0.02 * r(4 * width)
    sd[prefix + names["fc2_w"]] = r(width, 4 * width, std=proj_std)
    sd[prefix + names["fc2_b"]] = 0.02 * r(width)


CLIP_BLOCK_KEYS = {"ln1_w": "ln_1.weight", "ln1_b": "ln_1.bias", "qkv_w": "attn.in_proj_weight",
                   "qkv_b": "attn.in_proj_bias", "proj_w": "attn.out_proj.weight",
                   "proj_b": "attn.out_proj.bias", "ln2_w": "ln_2.weight", "ln2_b": "ln_2.bias",
                   "fc1_w": "mlp.c_fc.weight", "fc1_b": "mlp.c_fc.bias", "fc2_w": "mlp.c_proj.weight",
                   "fc2_b": "mlp.c_proj.bias"}
DINO_BLOCK_KEYS = {"ln1_w": "norm1.weight", "ln1_b": "norm1.bias", "qkv_w": "attn.qkv.weight",
                   "qkv_b": "attn.qkv.bias", "proj_w": "attn.proj.weight", "proj_b": "attn.proj.bias",
                   "ln2_w": "norm2.weight", "ln2_b": "norm2.bias", "fc1_w": "mlp.fc1.weight",
                   "fc1_b": "mlp.fc1.bias", "fc2_w": "mlp.fc2.weight", "fc2_b": "mlp.fc2.bias"}


def synthetic_clip_state_dict(seed=0, cfg=None, visual=True, text=True):
    """float32 state dict with openai/CLIP key names (appendix B 'State-dict keys')."""
    c = dict(CLIP_VITB16)
    c.update(cfg or {})
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, std=1.0: torch.randn(*s, generator=g) * std
    sd = {}
    if visual:
        w, p = c["v_width"], c["patch"]
        sd["visual.conv1.weight"] = r(w, 3, p, p, std=(3 * p * p) ** -0.5)
        sd["visual.class_embedding"] = r(w, std=w ** -0.5)
        sd["visual.positional_embedding"] = r((c["image"] // p) ** 2 + 1, w, std=w ** -0.5)
        sd["visual.ln_pre.weight"] = 1.0 + 0.1 * r(w)
        sd["visual.ln_pre.bias"] = 0.02 * r(w)
        for i in range(c["v_layers"]):
            _block(sd, g, "visual.transformer.resblocks.%d." % i, w, c["v_layers"], CLIP_BLOCK_KEYS)
        sd["visual.ln_post.weight"] = 1.0 + 0.1 * r(w)
        sd["visual.ln_post.bias"] = 0.02 * r(w)
        sd["visual.proj"] = r(w, c["embed_dim"], std=w ** -0.5)
    if text:
        w = c["t_width"]
        sd["token_embedding.weight"] = r(c["vocab"], w, std=0.02)
        sd["positional_embedding"] = r(c["context"], w, std=0.01)
        for i in range(c["t_layers"]):
            _block(sd, g, "transformer.resblocks.%d." % i, w, c["t_layers"], CLIP_BLOCK_KEYS)
        sd["ln_final.weight"] = 1.0 + 0.1 * r(w)
        sd["ln_final.bias"] = 0.02 * r(w)
        sd["text_projection"] = r(w, c["embed_dim"], std=w ** -0.5)
        sd["logit_scale"] = torch.tensor(4.6052)
    return sd


DINOV2 = {"dinov2_vitb14": dict(width=768, layers=12, registers=0), "dinov2_vitl14": dict(width=1024, layers=24, registers=0),
          "dinov2_vitb14_reg": dict(width=768, layers=12, registers=4), "dinov2_vitl14_reg": dict(width=1024, layers=24, registers=4)}
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
POS_INTERP = ("offset", "size_antialias", "size")
INPUT_NORM = {"clip": (CLIP_MEAN, CLIP_STD), "imagenet": (IMAGENET_MEAN, IMAGENET_STD)}


def synthetic_dinov2_state_dict(seed=2, width=768, layers=12, registers=0, grid=37, patch=14, gamma=(1e-2, 2.0)):
    """float32 state dict in the facebookresearch/dinov2 layout (docs/design/dinov2.md): the DINO keys plus `register_tokens`
    (registers > 0), `mask_token`, a [1, 1 + grid^2, width] `pos_embed` (the released files: grid 37, trained at 518 px) and per block
    `ls1.gamma` / `ls2.gamma`, log-uniform in `gamma` (trained LayerScale gains spread over decades; none of them is 1)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, std=1.0: torch.randn(*s, generator=g) * std
    sd = {"patch_embed.proj.weight": r(width, 3, patch, patch, std=(3 * patch * patch) ** -0.5),
          "patch_embed.proj.bias": 0.02 * r(width),
          "cls_token": r(1, 1, width, std=0.02),
          "pos_embed": r(1, grid * grid + 1, width, std=0.02),
          "mask_token": torch.zeros(1, width)}
    if registers:
        sd["register_tokens"] = r(1, registers, width, std=0.02)
    lo, hi = math.log(gamma[0]), math.log(gamma[1])
    for i in range(layers):
        _block(sd, g, "blocks.%d." % i, width, layers, DINO_BLOCK_KEYS)
        for ls in ("ls1", "ls2"):
            sd["blocks.%d.%s.gamma" % (i, ls)] = torch.exp(lo + (hi - lo) * torch.rand(width, generator=g))
    sd["norm.weight"] = 1.0 + 0.1 * r(width)
    sd["norm.bias"] = 0.02 * r(width)
    return sd


def is_dinov2(sd):
    """A state dict that has to go through prepare_dinov2: LayerScale gains (every DINOv2 checkpoint has them), SwiGLU or chunked
    blocks.  What prepare_dinov2 returns has none of them (its `register_tokens` stay), so it is not prepared twice."""
    return any(k.endswith(".ls1.gamma") or ".mlp.w12." in k or re.match(r"blocks\.\d+\.\d+\.", k) for k in sd)


def dinov2_check(sd, image=224):
    """Refuse, with the reason, what the device towers do not serve; returns dict(width, layers, registers, grid, patch)."""
    if image != 224:
        raise ValueError("DINOv2: image size %s is not served: the towers run at 224 x 224 only (257 + registers tokens)" % (image,))
    if any(re.match(r"blocks\.\d+\.\d+\.", k) for k in sd):
        raise ValueError("DINOv2: chunked block keys (blocks.{chunk}.{i}.*, the block_chunks layout of ViT-g/14) are not served; "
                         "re-save the checkpoint with blocks.{i}.* keys")
    if any(".mlp.w12." in k for k in sd):
        raise ValueError("DINOv2: SwiGLU blocks (mlp.w12 / mlp.w3, ViT-g/14) are not served: the towers' MLP is fc1 -> GELU -> fc2")
    w = sd["patch_embed.proj.weight"]
    width, patch = int(w.shape[0]), int(w.shape[-1])
    if width % 256 != 0 or width > 1024:
        raise ValueError("DINOv2: width %d is not served: the encoder kernels need a multiple of 256 up to 1024 (ViT-B/14: 768, "
                         "ViT-L/14: 1024; ViT-S/14's 384 is not)" % width)
    if patch != 14:
        raise ValueError("DINOv2: patch size %d is not served (14 is)" % patch)
    registers = int(sd["register_tokens"].shape[1]) if "register_tokens" in sd else 0
    np_ = (image // patch) ** 2
    if np_ + 1 + registers > 288:
        raise ValueError("DINOv2: %d register tokens give %d tokens; the attention kernels serve at most 288 (at most %d registers)"
                         % (registers, np_ + 1 + registers, 288 - np_ - 1))
    rows = int(sd["pos_embed"].shape[1])
    grid = int(round((rows - 1) ** 0.5))
    if grid * grid + 1 != rows:
        raise ValueError("DINOv2: pos_embed has %d rows, not 1 + a square grid" % rows)
    layers = 0
    while ("blocks.%d.norm1.weight" % layers) in sd:
        layers += 1
    return dict(width=width, layers=layers, registers=registers, grid=grid, patch=patch)


def resample_pos_embed(pos_embed, grid_out=16, mode="size_antialias"):
    """[1, 1 + G^2, W] -> float32 [1, 1 + grid_out^2, W]: the class row kept, the patch rows resampled bicubically in float32.
    'size_antialias': size=(grid_out, grid_out), antialias=True (upstream's interpolate_offset=0.0, interpolate_antialias=True; also
    what transformers' Dinov2WithRegistersModel does); 'offset': scale_factor=(grid_out + 0.1) / G, antialias=False (upstream's
    interpolate_offset=0.1); 'size': size=(grid_out, grid_out), antialias=False (transformers' Dinov2Model).  A table that already has
    1 + grid_out^2 rows is returned as it is."""
    import torch.nn.functional as F
    if mode not in POS_INTERP:
        raise ValueError("pos_interp must be one of %s, got %r" % (POS_INTERP, mode))
    pe = pos_embed.float()
    rows, width = pe.shape[1], pe.shape[2]
    if rows == grid_out * grid_out + 1:
        return pe
    G = int(round((rows - 1) ** 0.5))
    assert G * G + 1 == rows, rows
    grid = pe[:, 1:].reshape(1, G, G, width).permute(0, 3, 1, 2)
    if mode == "offset":
        s = float(grid_out + 0.1) / G
        out = F.interpolate(grid, scale_factor=(s, s), mode="bicubic", antialias=False)
    else:
        out = F.interpolate(grid, size=(grid_out, grid_out), mode="bicubic", antialias=(mode == "size_antialias"), align_corners=False)
    assert out.shape[-2:] == (grid_out, grid_out), out.shape
    return torch.cat([pe[:, :1], out.permute(0, 2, 3, 1).reshape(1, grid_out * grid_out, width)], dim=1)


def fold_layerscale(sd):
    """x += gamma * (W y + b)  ==  x += (diag(gamma) W) y + gamma * b: every block's ls1.gamma into attn.proj, ls2.gamma into mlp.fc2,
    computed in float64 (the result stays float64: it is rounded once, to the device dtypes, when the tower is built).  Returns a new
    dict without the ls keys."""
    out = {k: v for k, v in sd.items() if not (k.endswith(".ls1.gamma") or k.endswith(".ls2.gamma"))}
    for k, gam in sd.items():
        for ls, lin in ((".ls1.gamma", ".attn.proj."), (".ls2.gamma", ".mlp.fc2.")):
            if k.endswith(ls):
                p = k[:-len(ls)] + lin
                gam64 = gam.double()
                out[p + "weight"] = gam64[:, None] * sd[p + "weight"].double()
                out[p + "bias"] = gam64 * sd[p + "bias"].double()
    return out


def fold_input_norm(sd, input_norm="imagenet"):
    """The ingest path hands every tower CLIP-normalised pixels x_clip = (p - mu_clip) / sigma_clip.  A tower trained on x_in = (p - mu_in)
    / sigma_in = x_clip * sigma_clip / sigma_in + (mu_clip - mu_in) / sigma_in gets, per input channel c, W'[:, c] = W[:, c] * sigma_clip,c
    / sigma_in,c and b' = b + sum_{c,kh,kw} W[:, c, kh, kw] * (mu_clip,c - mu_in,c) / sigma_in,c (float64): the patch embedding of the
    CLIP-normalised pixels is then exactly the one of the tower's own normalisation.  'clip': nothing to fold."""
    if input_norm not in INPUT_NORM:
        raise ValueError("input_norm must be one of %s, got %r" % (tuple(INPUT_NORM), input_norm))
    if input_norm == "clip":
        return sd
    mu_in, sd_in = (torch.tensor(v, dtype=torch.float64) for v in INPUT_NORM[input_norm])
    mu_c, sd_c = torch.tensor(CLIP_MEAN, dtype=torch.float64), torch.tensor(CLIP_STD, dtype=torch.float64)
    w = sd["patch_embed.proj.weight"].double()
    out = dict(sd)
    out["patch_embed.proj.weight"] = w * (sd_c / sd_in).view(1, 3, 1, 1)
    out["patch_embed.proj.bias"] = sd["patch_embed.proj.bias"].double() + (w * ((mu_c - mu_in) / sd_in).view(1, 3, 1, 1)).sum(dim=(1, 2, 3))
    return out


def prepare_dinov2(sd, pos_interp=None, input_norm="imagenet", image=224):
    """A facebookresearch/dinov2 state dict -> the plain DINO layout the device tower is built from (model.build_dino): LayerScale and the
    input normalisation folded into the weights, pos_embed resampled to the 16 x 16 patches of a 224-pixel image, `register_tokens`
    kept, `mask_token` dropped.

    pos_interp: 'offset' | 'size_antialias' | 'size' (resample_pos_embed).  None chooses by checkpoint: 'offset' without registers,
    'size_antialias' with.  That default follows what upstream's hub entry points are RECALLED to pass (interpolate_offset=0.1,
    interpolate_antialias=False for the plain models; 0.0 / True for the `_reg` ones); it could not be checked against upstream when
    this was written - pass the mode explicitly to match a given feature dump."""
    info = dinov2_check(sd, image)
    if pos_interp is None:
        pos_interp = "size_antialias" if info["registers"] else "offset"
    out = {k: v for k, v in sd.items() if k != "mask_token"}
    out = fold_input_norm(fold_layerscale(out), input_norm)
    out["pos_embed"] = resample_pos_embed(sd["pos_embed"], image // info["patch"], pos_interp)
    return out


def synthetic_dino_state_dict(seed=1, width=768, layers=12, image=224, patch=16):
    """float32 state dict with the key names of gcd/models/vision_transformer.py:135-219."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, std=1.0: torch.randn(*s, generator=g) * std
    sd = {"patch_embed.proj.weight": r(width, 3, patch, patch, std=(3 * patch * patch) ** -0.5),
          "patch_embed.proj.bias": 0.02 * r(width),
          "cls_token": r(1, 1, width, std=0.02),
          "pos_embed": r(1, (image // patch) ** 2 + 1, width, std=0.02)}
    for i in range(layers):
        _block(sd, g, "blocks.%d." % i, width, layers, DINO_BLOCK_KEYS)
    sd["norm.weight"] = 1.0 + 0.1 * r(width)
    sd["norm.bias"] = 0.02 * r(width)
    return sd
