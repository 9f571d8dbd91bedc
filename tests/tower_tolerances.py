"""Tolerances of the tower-vs-oracle tests, and the weights and inputs those tests use (tests/test_gpu_parity.py,
tests/tower_cos.py and the CPU test tests/test_tower_tolerance_sensitivity.py build them here, so all three see the same data).

Each tolerance is a pair (1 - cos, max|err| / max|ref|) over the rows of one feature matrix, about 10 x the worst value the HIP
towers reached against the fp32 oracle (oracle/clip_oracle.py) on an MI355X.  The features are deterministic
and batch-invariant (test_encoder_batch_invariance), so each measured value is exact for these inputs.  `python tests/tower_cos.py`
prints them; the values measured on 2026-10-16 are noted next to each bound.
Every bound is inside the product's north-star tolerance (1 - cos < 1e-3, max|err| <= 3e-2 max|ref|): NORTH_STAR below.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NORTH_STAR = (1e-3, 3e-2)

# name -> (1 - cos, max|err| / max|ref|); measured: the HIP towers against the oracle, 2026-10-16
TOL = {
    "clip2_image": (2e-6, 8e-3),               # measured 1.74e-7 / 7.66e-4
    "clip2_text": (4e-6, 9e-3),                # measured 3.79e-7 / 8.23e-4
    "clip12_image": (7e-6, 1.3e-2),            # measured 6.44e-7 / 1.25e-3
    "clip12_text": (1e-5, 1.2e-2),             # measured 9.00e-7 / 1.15e-3
    "dino12": (1e-5, 1.5e-2),                  # measured 9.32e-7 / 1.47e-3
    "outlier_clip_image": (8e-6, 1.7e-2),      # measured 7.65e-7 / 1.66e-3
    "outlier_clip_text": (6e-6, 1.2e-2),       # measured 5.13e-7 / 1.18e-3
    "outlier_dino": (2e-5, 2.1e-2),            # measured 1.95e-6 / 2.09e-3
    "zeroshot_text": (2e-6, 7e-3),             # measured 1.55e-7 / 6.12e-4
    "outlier_feat_dino": (9e-5, 2.5e-2),       # measured 8.30e-6 / 2.50e-3
    "outlier_feat_clip_image": (1e-5, 1.5e-2), # measured 9.59e-7 / 1.41e-3
    "outlier_feat_text": (7e-6, 1.2e-2),       # measured 6.95e-7 / 1.17e-3
}
assert all(c < NORTH_STAR[0] and e <= NORTH_STAR[1] for c, e in TOL.values())


def metrics(out, ref):
    """(max over rows of 1 - cos, max|out - ref| / max|ref|), in float64"""
    a, b = out.double().cpu(), ref.double().cpu()
    gap = (1 - torch.nn.functional.cosine_similarity(a, b, dim=-1)).max().item()
    return gap, ((a - b).abs().max() / b.abs().max()).item()


def check(name, out, ref):
    """assert the HIP features `out` are within TOL[name] of the oracle's `ref`"""
    assert out.shape == ref.shape, (name, out.shape, ref.shape)
    assert bool(torch.isfinite(out.float()).all()), name
    gap, rel = metrics(out, ref)
    tc, te = TOL[name]
    assert gap <= tc and rel <= te, "%s: 1 - cos %.3e (bound %.1e), max|err| / max|ref| %.3e (bound %.1e)" % (name, gap, tc, rel, te)
    return gap, rel


# ----------------------------------------------------------------------------------------------- weights and inputs
def _round_clip(sd):
    return {k: (v.half().float() if v.dim() >= 2 and "positional" not in k and "class_emb" not in k else v) for k, v in sd.items()}


def _prompts(lengths, seed, n=None):
    tok = torch.zeros(len(lengths), 77, dtype=torch.int32)
    g = torch.Generator().manual_seed(seed)
    for i, ln in enumerate(lengths):
        tok[i, 0] = 49406
        tok[i, 1:1 + ln] = torch.randint(1, 49405, (ln,), generator=g, dtype=torch.int32)
        tok[i, 1 + ln] = 49407
    return tok


def clip_case(layers):
    """test_clip_towers_match_oracle: (state dict, its device-rounded copy for the oracle, 5 images, 4 prompts)"""
    from scd_amd.clip import weights as W
    sd = W.synthetic_clip_state_dict(seed=0, cfg=dict(v_layers=layers, t_layers=layers))
    img = torch.randn(5, 3, 224, 224, generator=torch.Generator().manual_seed(78))
    return sd, _round_clip(sd), img, _prompts((3, 8, 20, 75), 79)


def dino_case():
    """test_dino_tower_matches_oracle: (state dict, rounded copy, 3 images)"""
    from scd_amd.clip import weights as W
    sd = W.synthetic_dino_state_dict(seed=1, layers=12)
    sd16 = {k: (v.half().float() if v.dim() >= 2 and "pos_embed" not in k and "cls_token" not in k else v) for k, v in sd.items()}
    return sd, sd16, torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(77))


def outlier_case(tower):
    """test_towers_with_outlier_weights_match_oracle: (state dict, rounded copy, inputs: 5 fp16-exact images or 6 prompts)"""
    import outlier_weights as ow
    if tower == "dino":
        sd, _ = ow.dino_outlier_state_dict(seed=1, layers=12)
    else:
        sd, _, _ = ow.clip_outlier_state_dict(seed=0, layers=12)
    if tower == "clip_text":
        x = _prompts((1, 3, 8, 20, 40, 75), 79)
    else:
        x = torch.randn(5, 3, 224, 224, generator=torch.Generator().manual_seed(78)).half().float()
    return sd, ow.round_like_the_device(sd), x


def zeroshot_case():
    """test_zeroshot_classifier_pooling: (state dict (text tower, 2 blocks), rounded copy, names, templates)"""
    from scd_amd.clip import weights as W
    from scd_amd.local_utils import clip_lang_util as clu
    sd = W.synthetic_clip_state_dict(seed=0, cfg=dict(t_layers=2), visual=False)
    sd16 = {k: (v.half().float() if v.dim() >= 2 and "positional" not in k else v) for k, v in sd.items()}
    return sd, sd16, ["red_fox", "tabby", "kit_fox", "zebra", "grey_whale"], clu.imagenet_templates[:9]


def outlier_features_case():
    """test_outlier_weight_features_give_the_oracle_features_labels_and_names: (class ids y, 60 fp16-exact images in 6 classes,
    48 prompts)"""
    n_cls, per = 6, 10
    g = torch.Generator().manual_seed(321)
    base = torch.randn(n_cls, 3, 224, 224, generator=g)
    y = np.repeat(np.arange(n_cls), per)
    img = (base[torch.from_numpy(y)] + 0.6 * torch.randn(n_cls * per, 3, 224, 224, generator=g)).half().float()
    tok = torch.zeros(48, 77, dtype=torch.int32)
    gt = torch.Generator().manual_seed(5)
    for i in range(48):
        ln = 2 + i % 9
        tok[i, 0] = 49406
        tok[i, 1:1 + ln] = torch.randint(1, 49405, (ln,), generator=gt, dtype=torch.int32)
        tok[i, 1 + ln] = 49407
    return y, img, tok
