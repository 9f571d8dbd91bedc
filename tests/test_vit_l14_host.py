"""CLIP ViT-L/14 on the host side: the model entry, its synthetic state dict, and the --clip_model option of both mains with the
cache names it selects.  No GPU needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

L14_SHAPES = {"visual.conv1.weight": (1024, 3, 14, 14), "visual.positional_embedding": (257, 1024), "visual.proj": (1024, 768),
              "text_projection": (768, 768), "positional_embedding": (77, 768), "token_embedding.weight": (49408, 768),
              "visual.transformer.resblocks.23.attn.in_proj_weight": (3072, 1024), "transformer.resblocks.11.mlp.c_fc.weight": (3072, 768)}


def test_vit_l14_is_available_and_its_synthetic_state_dict_has_the_l14_shapes():
    import scd_amd.clip as clip
    from scd_amd.clip import weights as W
    assert "ViT-L/14" in clip.available_models() and "ViT-B/16" in clip.available_models()
    assert W.CLIP_VITL14 == dict(embed_dim=768, image=224, patch=14, v_width=1024, v_layers=24, v_heads=16, context=77, vocab=49408,
                                 t_width=768, t_layers=12, t_heads=12)
    sd = W.synthetic_clip_state_dict(cfg=W.CLIP_VITL14)
    for k, shape in L14_SHAPES.items():
        assert tuple(sd[k].shape) == shape, k
    assert "visual.transformer.resblocks.24.ln_1.weight" not in sd and "transformer.resblocks.12.ln_1.weight" not in sd


def test_load_builds_the_requested_model(monkeypatch):
    import scd_amd.clip as clip
    from scd_amd.clip import model as M
    seen = {}

    class Probe:                                   # stands in for the device-side model: load() hands it the state dict
        def __init__(self, sd):
            seen["sd"] = sd

        def cuda(self):
            return self

    monkeypatch.setattr(clip, "CLIP", Probe)
    monkeypatch.setattr(M, "CLIP", Probe)
    model, pre = clip.load("ViT-L/14", synthetic=True, device="cpu")
    assert model.synthetic
    for k, shape in L14_SHAPES.items():
        assert tuple(seen["sd"][k].shape) == shape, k
    clip.load("ViT-B/16", synthetic=True, device="cpu")
    assert tuple(seen["sd"]["visual.conv1.weight"].shape) == (768, 3, 16, 16)
    assert tuple(seen["sd"]["visual.proj"].shape) == (768, 512)


def test_missing_checkpoint_names_the_requested_model(tmp_path):
    import scd_amd.clip as clip
    with pytest.raises(FileNotFoundError) as e:
        clip.load("ViT-L/14", download_root=str(tmp_path), synthetic=False, device="cpu")
    assert "ViT-L-14.pt" in str(e.value) and "ViT-B-16" not in str(e.value)
    with pytest.raises(RuntimeError):
        clip.load("ViT-L/14@336px", synthetic=True, device="cpu")


def test_mains_parse_clip_model_and_tag_the_clip_caches():
    import main_unsup as mu
    import main_ptsup as mp
    for parser in (mu.build_parser(), mp.build_parser()):
        assert parser.parse_args([]).clip_model == "ViT-B/16"
        assert parser.parse_args(["--clip_model", "ViT-L/14"]).clip_model == "ViT-L/14"
        with pytest.raises(SystemExit):
            parser.parse_args(["--clip_model", "RN50"])
    # the default backbone keeps the reference's file names
    a = mu.build_parser().parse_args(["--root_dir", "/r", "--dataset_name", "cub", "--feat_model", "clip", "--corpus", "wikibird"])
    assert mu.clip_cache_name(a) == "clip" and mu.feat_cache_name(a) == "clip"
    assert mu.zeroshot_path(a) == "/r/zeroshot_weights/zeroshot_weights_all_wikibird_vit_b_16.pt"
    a = mp.build_parser().parse_args(["--root_dir", "/r"])
    assert mu.feat_cache_name(a) == "clip" and mu.zeroshot_path(a) == "/r/zeroshot_weights/zeroshot_weights_all_nouns_vit_b_16.pt"
    a = mu.build_parser().parse_args([])
    assert mu.feat_cache_name(a) == "dino_vit" and mu.clip_cache_name(a) == "clip"
    # another backbone: every CLIP-derived cache carries its tag
    a = mu.build_parser().parse_args(["--root_dir", "/r", "--clip_model", "ViT-L/14"])
    assert mu.clip_cache_name(a) == "clip_vit_l_14" and mu.feat_cache_name(a) == "dino_vit"
    assert mu.zeroshot_path(a) == "/r/zeroshot_weights/zeroshot_weights_all_nouns_vit_l_14.pt"
    a = mp.build_parser().parse_args(["--root_dir", "/r", "--clip_model", "ViT-L/14", "--corpus", "wikidog"])
    assert mu.feat_cache_name(a) == "clip_vit_l_14" and mu.clip_cache_name(a) == "clip_vit_l_14"
    assert mu.zeroshot_path(a) == "/r/zeroshot_weights/zeroshot_weights_all_wikidog_vit_l_14.pt"


def test_mains_read_the_tagged_caches(tmp_path, monkeypatch):
    """Without --extract_feat the mains load `{feat}_{dataset}_all.pt` and `clip..._{dataset}_all.pt`: the L/14 run asks for the
    tagged files and never reads a B/16 cache."""
    import main_unsup as mu
    asked = []
    monkeypatch.setattr(mu, "load_or_extract", lambda args, model, name, out: asked.append(out))
    a = mu.build_parser().parse_args(["--root_dir", str(tmp_path), "--dataset_name", "cifar100", "--clip_model", "ViT-L/14"])
    mu.extract_or_load_all(a, None, None)
    assert asked == ["dino_vit_cifar100_all.pt", "clip_vit_l_14_cifar100_all.pt"]
    asked.clear()
    a = mu.build_parser().parse_args(["--root_dir", str(tmp_path), "--dataset_name", "cifar100"])
    mu.extract_or_load_all(a, None, None)
    assert asked == ["dino_vit_cifar100_all.pt", "clip_cifar100_all.pt"]
