"""DINOv2 ViT-B/14 / ViT-L/14 on the host side: the torch restatement (tests/dinov2_ref.py) against the `transformers` models, the
three load-time folds (LayerScale, position table, input normalisation) against it, what folding LayerScale costs in fp16, the
refusals, and the --feat_model names of both mains.  No GPU needed."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import dinov2_ref as ref  # noqa: E402
import tower_tolerances as tt  # noqa: E402
from scd_amd.clip import weights as W  # noqa: E402

NAMES = ["dinov2_vitb14", "dinov2_vitl14", "dinov2_vitb14_reg", "dinov2_vitl14_reg"]
# the LayerScale range of the synthetic state dicts and of the outlier tower of tests/test_gpu_dinov2.py: the one
# test_layerscale_fold_costs_a_tenth_of_the_north_star_in_fp16 holds on
GAMMA_RANGE = (1e-2, 2.0)


def _raw(n, seed, size=224):
    return torch.rand(n, 3, size, size, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ 1. the restatement
def _from_hf(hf_sd, layers):
    """transformers' Dinov2 keys -> the facebookresearch/dinov2 layout"""
    e = "embeddings."
    sd = {"cls_token": hf_sd[e + "cls_token"], "pos_embed": hf_sd[e + "position_embeddings"], "mask_token": hf_sd[e + "mask_token"],
          "patch_embed.proj.weight": hf_sd[e + "patch_embeddings.projection.weight"],
          "patch_embed.proj.bias": hf_sd[e + "patch_embeddings.projection.bias"],
          "norm.weight": hf_sd["layernorm.weight"], "norm.bias": hf_sd["layernorm.bias"]}
    if e + "register_tokens" in hf_sd:
        sd["register_tokens"] = hf_sd[e + "register_tokens"]
    for i in range(layers):
        s, d = "encoder.layer.%d." % i, "blocks.%d." % i
        a = s + "attention.attention."
        sd[d + "attn.qkv.weight"] = torch.cat([hf_sd[a + "query.weight"], hf_sd[a + "key.weight"], hf_sd[a + "value.weight"]])
        sd[d + "attn.qkv.bias"] = torch.cat([hf_sd[a + "query.bias"], hf_sd[a + "key.bias"], hf_sd[a + "value.bias"]])
        for src, dst in (("attention.output.dense.", "attn.proj."), ("norm1.", "norm1."), ("norm2.", "norm2."), ("mlp.fc1.", "mlp.fc1."),
                         ("mlp.fc2.", "mlp.fc2.")):
            for wb in ("weight", "bias"):
                sd[d + dst + wb] = hf_sd[s + src + wb]
        sd[d + "ls1.gamma"] = hf_sd[s + "layer_scale1.lambda1"]
        sd[d + "ls2.gamma"] = hf_sd[s + "layer_scale2.lambda1"]
    return sd


@pytest.mark.parametrize("registers", [0, 4])
def test_restatement_equals_transformers(registers):
    """Dinov2Model / Dinov2WithRegistersModel, random weights made unit-scale (LayerScale gains and embeddings included), 2 layers,
    hidden 128 / 2 heads, image_size 518, a 224 input: pooler_output to 1e-5 in fp32.  Dinov2WithRegistersModel resamples the position
    table with size + antialias ('size_antialias').  The installed Dinov2Model resamples with size and NO antialias, so its case uses
    the 'size' mode; with 'size_antialias' its table is a different one and the outputs differ by far more than rounding (printed)."""
    tf = pytest.importorskip("transformers")
    torch.manual_seed(11 + registers)
    kw = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, image_size=518, patch_size=14)
    if registers:
        model = tf.Dinov2WithRegistersModel(tf.Dinov2WithRegistersConfig(num_register_tokens=registers, **kw))
    else:
        model = tf.Dinov2Model(tf.Dinov2Config(**kw))
    model = model.eval().float()
    with torch.no_grad():
        for k, v in model.state_dict().items():          # random everywhere: the init leaves biases at 0 and the gains at 1
            if "lambda" in k:
                v.copy_(torch.empty_like(v).uniform_(0.2, 1.5))
            elif "norm" in k and k.endswith("weight"):
                v.copy_(1.0 + 0.1 * torch.randn_like(v))
            elif k.endswith("bias") or "token" in k or "position" in k:
                v.copy_(0.2 * torch.randn_like(v))
    x = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want = model(pixel_values=x).pooler_output
    sd = _from_hf(model.state_dict(), 2)
    assert ("register_tokens" in sd) == bool(registers)
    mode = "size_antialias" if registers else "size"
    got = ref.forward(sd, x, torch.float32, pos_interp=mode, heads=2)
    err = (got - want).abs().max().item()
    print("registers %d, %s: max|restatement - transformers| %.3e, max|ref| %.3f" % (registers, mode, err, want.abs().max().item()))
    assert 0.5 < want.abs().max().item() < 20
    assert err <= 1e-5
    if not registers:
        other = (ref.forward(sd, x, torch.float32, pos_interp="size_antialias", heads=2) - want).abs().max().item()
        print("registers 0, size_antialias against Dinov2Model: %.3e" % other)


# ------------------------------------------------------------------------------------------------ 2. folds
@pytest.fixture(scope="module")
def small_sd():
    return W.synthetic_dinov2_state_dict(seed=3, width=256, layers=2, registers=4, gamma=GAMMA_RANGE)


def test_synthetic_state_dict_has_the_upstream_layout():
    sd = W.synthetic_dinov2_state_dict(seed=2, width=768, layers=2, registers=4)
    shapes = {"cls_token": (1, 1, 768), "pos_embed": (1, 1370, 768), "register_tokens": (1, 4, 768), "mask_token": (1, 768),
              "patch_embed.proj.weight": (768, 3, 14, 14), "patch_embed.proj.bias": (768,), "blocks.1.attn.qkv.weight": (2304, 768),
              "blocks.1.attn.qkv.bias": (2304,), "blocks.0.ls1.gamma": (768,), "blocks.1.ls2.gamma": (768,),
              "blocks.1.mlp.fc1.weight": (3072, 768), "norm.weight": (768,)}
    for k, s in shapes.items():
        assert tuple(sd[k].shape) == s, k
    assert "blocks.2.norm1.weight" not in sd
    assert "register_tokens" not in W.synthetic_dinov2_state_dict(width=256, layers=1, registers=0, grid=16)
    g = sd["blocks.0.ls1.gamma"]
    assert g.min() >= 1e-2 and g.max() <= 2.0 and g.max() / g.min() > 20          # not all 1: spread over more than a decade
    assert W.is_dinov2(sd) and not W.is_dinov2(W.synthetic_dino_state_dict(layers=1))
    assert not W.is_dinov2(W.prepare_dinov2(sd))


def test_layerscale_fold_equals_the_unfolded_model_in_float64(small_sd):
    x = ref.normalise(_raw(2, 21), ref.IMAGENET_MEAN, ref.IMAGENET_STD)
    folded = W.fold_layerscale(small_sd)
    assert not any("gamma" in k for k in folded) and folded["blocks.0.attn.proj.weight"].dtype == torch.float64
    a = ref.forward(small_sd, x, torch.float64, pos_interp="size_antialias")
    b = ref.forward(folded, x, torch.float64, pos_interp="size_antialias")
    err = (a - b).abs().max().item()
    print("LayerScale fold, float64: max abs %.3e (max|ref| %.3f)" % (err, a.abs().max().item()))
    assert a.abs().max().item() > 0.5 and err <= 1e-10


def test_input_norm_fold_on_clip_pixels_equals_the_model_on_imagenet_pixels(small_sd):
    raw = _raw(2, 22)
    a = ref.forward(small_sd, ref.normalise(raw, ref.IMAGENET_MEAN, ref.IMAGENET_STD), torch.float64)
    folded = W.fold_input_norm(small_sd, "imagenet")
    b = ref.forward(folded, ref.normalise(raw, ref.CLIP_MEAN, ref.CLIP_STD), torch.float64)
    err = (a - b).abs().max().item()
    unfolded = (a - ref.forward(small_sd, ref.normalise(raw, ref.CLIP_MEAN, ref.CLIP_STD), torch.float64)).abs().max().item()
    print("input-norm fold, float64: max abs %.3e; without the fold %.3e" % (err, unfolded))
    assert err <= 1e-9 and unfolded > 1e-4                      # the fold matters: the two normalisations differ by ~17 % in scale
    assert W.fold_input_norm(small_sd, "clip") is small_sd
    assert W.CLIP_MEAN == ref.CLIP_MEAN and W.IMAGENET_STD == ref.IMAGENET_STD
    import scd_amd.clip as clip
    assert tuple(clip.MEAN) == W.CLIP_MEAN and tuple(clip.STD) == W.CLIP_STD     # what the ingest path normalises with
    with pytest.raises(ValueError):
        W.fold_input_norm(small_sd, "laion")


def test_pos_interp_modes_are_their_interpolate_calls_bit_for_bit(small_sd):
    pe = small_sd["pos_embed"]
    grid = pe[:, 1:].reshape(1, 37, 37, 256).permute(0, 3, 1, 2).float()
    calls = {"size_antialias": F.interpolate(grid, size=(16, 16), mode="bicubic", antialias=True, align_corners=False),
             "offset": F.interpolate(grid, scale_factor=((16 + 0.1) / 37, (16 + 0.1) / 37), mode="bicubic", antialias=False),
             "size": F.interpolate(grid, size=(16, 16), mode="bicubic", antialias=False, align_corners=False)}
    for mode, want in calls.items():
        got = W.resample_pos_embed(pe, 16, mode)
        assert got.shape == (1, 257, 256) and got.dtype == torch.float32
        assert torch.equal(got[:, 0], pe[:, 0])                                      # the class row is kept
        assert torch.equal(got[:, 1:], want.permute(0, 2, 3, 1).reshape(1, 256, 256)), mode
        assert torch.equal(got, ref.interpolate_pos(pe, 16, mode))
    assert not torch.equal(calls["offset"], calls["size_antialias"])
    t257 = torch.randn(1, 257, 256)
    for mode in W.POS_INTERP:
        assert torch.equal(W.resample_pos_embed(t257, 16, mode), t257)               # a 257-row table passes through
    with pytest.raises(ValueError):
        W.resample_pos_embed(pe, 16, "bilinear")
    # the default is by checkpoint
    assert torch.equal(W.prepare_dinov2(small_sd)["pos_embed"], W.resample_pos_embed(pe, 16, "size_antialias"))
    plain = {k: v for k, v in small_sd.items() if k != "register_tokens"}
    assert torch.equal(W.prepare_dinov2(plain)["pos_embed"], W.resample_pos_embed(pe, 16, "offset"))
    assert torch.equal(W.prepare_dinov2(plain, pos_interp="size_antialias")["pos_embed"], W.resample_pos_embed(pe, 16, "size_antialias"))


def test_prepared_state_dict_on_clip_pixels_equals_the_model(small_sd):
    """All three folds together: what the device tower is built from."""
    raw = _raw(2, 23)
    a = ref.forward(small_sd, ref.normalise(raw, ref.IMAGENET_MEAN, ref.IMAGENET_STD), torch.float64, pos_interp="size_antialias")
    prep = W.prepare_dinov2(small_sd)
    assert "mask_token" not in prep and prep["pos_embed"].shape == (1, 257, 256) and prep["register_tokens"].shape == (1, 4, 256)
    b = ref.forward(prep, ref.normalise(raw, ref.CLIP_MEAN, ref.CLIP_STD), torch.float64)
    assert (a - b).abs().max().item() <= 1e-9


# ------------------------------------------------------------------------------------------------ 3. the cost of folding in fp16
def test_layerscale_fold_costs_a_tenth_of_the_north_star_in_fp16():
    """The fp32 restatement on (a) weights where gamma * W is rounded to fp16 - what the tower holds - and (b) weights where W is rounded
    to fp16 and gamma stays fp32 - what a LayerScale kernel would hold.  Width 768, 2 blocks, gamma log-uniform in [1e-2, 2].
    Rounding gamma * W has the relative size of rounding W, so the two differ by fp16 rounding noise: below a tenth of NORTH_STAR.
    Measured: 1 - cos 8.5e-08, max|err| / max|ref| 3.9e-04 (bounds 1e-4 and 3e-3); the range did not have to be narrowed."""
    sd = W.synthetic_dinov2_state_dict(seed=4, width=768, layers=2, registers=4, gamma=GAMMA_RANGE)
    g = sd["blocks.0.ls1.gamma"]
    assert g.min() < 2e-2 and g.max() > 1.0
    x = ref.normalise(_raw(4, 24).float(), ref.IMAGENET_MEAN, ref.IMAGENET_STD)
    r16 = lambda v: v.half().float()
    mats = [k for k, v in sd.items() if v.dim() >= 2 and k not in ("pos_embed", "cls_token", "register_tokens", "mask_token")]
    folded = {k: v.float() for k, v in W.fold_layerscale(sd).items()}
    a_sd = {k: (r16(v) if k in mats else v) for k, v in folded.items()}                 # (gamma W) -> fp16
    b_sd = {k: (r16(v) if k in mats else v) for k, v in sd.items()}                     # W -> fp16, gamma fp32
    a = ref.forward(a_sd, x, torch.float32)
    b = ref.forward(b_sd, x, torch.float32)
    gap, rel = tt.metrics(a, b)
    print("LayerScale folded in fp16 against fp16 W with fp32 gamma: 1 - cos %.3e, max|err| / max|ref| %.3e" % (gap, rel))
    assert gap < tt.NORTH_STAR[0] / 10 and rel <= tt.NORTH_STAR[1] / 10


# ------------------------------------------------------------------------------------------------ 4. refusals
def _tiny(**kw):
    args = dict(seed=5, width=256, layers=1, registers=0, grid=16)
    args.update(kw)
    return W.synthetic_dinov2_state_dict(**args)


def test_refusals_name_the_reason(tmp_path):
    import scd_amd.clip as clip
    from scd_amd.clip.model import DinoViT
    with pytest.raises(ValueError, match="width 384"):
        DinoViT(_tiny(width=384))
    sd = _tiny()
    sd["blocks.0.mlp.w12.weight"] = torch.zeros(8, 256)
    with pytest.raises(ValueError, match="SwiGLU"):
        DinoViT(sd)
    sd = {("blocks.0." + k[len("blocks."):] if k.startswith("blocks.") else k): v for k, v in _tiny().items()}
    assert "blocks.0.0.norm1.weight" in sd
    with pytest.raises(ValueError, match="[Cc]hunked"):
        DinoViT(sd)
    with pytest.raises(ValueError, match="32 register tokens give 289 tokens"):
        DinoViT(_tiny(registers=32))
    DinoViT(_tiny(registers=31))                                  # 288 tokens: served (host side only here)
    with pytest.raises(ValueError, match="518"):
        DinoViT(_tiny(), image=518)
    with pytest.raises(ValueError, match="518"):
        clip.load_dinov2("dinov2_vitb14", synthetic=True, image=518)
    with pytest.raises(ValueError, match="pos_interp"):
        DinoViT(_tiny(grid=37), pos_interp="nearest")
    with pytest.raises(ValueError, match="dinov2_vits14"):
        clip.load_dinov2("dinov2_vits14", root=str(tmp_path))
    with pytest.raises(ValueError):
        clip.load_dinov2("dinov2_vitg14", synthetic=True)
    with pytest.raises(ValueError, match="DINOv2 state dicts only"):
        DinoViT(W.synthetic_dino_state_dict(layers=1), input_norm="imagenet")


def test_missing_checkpoint_names_the_file(tmp_path, monkeypatch):
    import scd_amd.clip as clip
    for name, fname in (("dinov2_vitb14", "dinov2_vitb14_pretrain.pth"), ("dinov2_vitl14_reg", "dinov2_vitl14_reg4_pretrain.pth")):
        with pytest.raises(FileNotFoundError) as e:
            clip.load_dinov2(name, root=str(tmp_path))
        assert os.path.join(str(tmp_path), "dinov2", fname) in str(e.value)
    monkeypatch.setenv("SCD_ROOT", str(tmp_path / "env"))
    assert clip.dinov2_checkpoint_path("dinov2_vitb14_reg") == str(tmp_path / "env" / "dinov2" / "dinov2_vitb14_reg4_pretrain.pth")
    assert clip.dinov2_models() == NAMES


def test_load_dinov2_reads_the_checkpoint_and_folds_it(tmp_path):
    import scd_amd.clip as clip
    sd = W.synthetic_dinov2_state_dict(seed=6, width=768, layers=1, registers=4)
    os.makedirs(tmp_path / "dinov2")
    torch.save(sd, tmp_path / "dinov2" / "dinov2_vitb14_reg4_pretrain.pth")
    torch.save(sd, tmp_path / "dinov2" / "dinov2_vitl14_reg4_pretrain.pth")
    with pytest.raises(ValueError, match="holds width 768"):                # a file that is not the model asked for
        clip.load_dinov2("dinov2_vitl14_reg", root=str(tmp_path))
    m = clip.load_dinov2("dinov2_vitb14_reg", root=str(tmp_path))
    assert not m.synthetic and m.name == "dinov2_vitb14_reg"
    want = W.prepare_dinov2(sd)
    assert set(m._sd) == set(want) and all(torch.equal(m._sd[k], want[k]) for k in want)
    m = clip.load_dinov2("dinov2_vitb14_reg", root=str(tmp_path), input_norm="clip", pos_interp="offset")
    assert torch.equal(m._sd["patch_embed.proj.weight"], sd["patch_embed.proj.weight"])
    assert torch.equal(m._sd["pos_embed"], W.resample_pos_embed(sd["pos_embed"], 16, "offset"))
    s = clip.load_dinov2("dinov2_vitb14", synthetic=True)
    assert s.synthetic and s._sd["pos_embed"].shape == (1, 257, 768) and "blocks.11.mlp.fc2.weight" in s._sd


# ------------------------------------------------------------------------------------------------ 5. the mains
def test_mains_take_the_dinov2_names_and_name_the_caches_after_them(tmp_path, monkeypatch):
    import main_unsup as mu
    import main_ptsup as mp
    asked = []
    monkeypatch.setattr(mu, "load_or_extract", lambda args, model, name, out: asked.append((name, out)))
    monkeypatch.setenv("SCD_ROOT", str(tmp_path))
    for parser in (mu.build_parser(), mp.build_parser()):
        assert "dinov2_vitb14_reg" in parser.format_help()
        for name in NAMES:
            a = parser.parse_args(["--root_dir", str(tmp_path), "--dataset_name", "cub", "--feat_model", name])
            assert a.feat_model == name and mu.feat_cache_name(a) == name
            asked.clear()
            mu.extract_or_load_all(a, None, None)
            assert asked == [(name, "%s_cub_all.pt" % name), ("clip", "clip_cub_all.pt")]
            with pytest.raises(FileNotFoundError) as e:                     # the loader the mains call, nothing on disk
                mu.load_feat_model(a, None)
            stem = name.replace("_reg", "_reg4")
            assert os.path.join(str(tmp_path), "dinov2", stem + "_pretrain.pth") in str(e.value)
    a = mu.build_parser().parse_args(["--feat_model", "dinov2_vits14"])
    with pytest.raises(ValueError):
        mu.load_feat_model(a, None)
