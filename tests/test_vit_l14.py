"""CLIP ViT-L/14 on the device: attention at T = 257 (and the rest of 256 < T <= 288) against float64, the image and text towers
against the fp32 oracle, the d = 768 similarity + top-k against the float64 oracle, the zero-shot classifier build, and both mains
end to end with --clip_model ViT-L/14."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import tower_tolerances as tt  # noqa: E402
from oracle import clip_oracle as co  # noqa: E402
from oracle import naming_oracle as no  # noqa: E402
from test_gpu_attention import _planted, _dense, _check_full  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device; they must not be skipped on the GPU box"
    from scd_amd import ops as o
    return o


def dev(x):
    return torch.as_tensor(x).cuda()


def north_star(out, ref, what):
    gap, rel = tt.metrics(out, ref)
    assert bool(torch.isfinite(out.float()).all()), what
    assert gap < tt.NORTH_STAR[0] and rel <= tt.NORTH_STAR[1], "%s: 1 - cos %.3e, max|err| / max|ref| %.3e" % (what, gap, rel)
    print("%s: 1 - cos %.3e, max|err| / max|ref| %.3e" % (what, gap, rel))
    return gap, rel


# ------------------------------------------------------------------------------------------------ attention, 256 < T <= 288
# (T, heads, batch): the tower's 16 heads with items below, at and over 256; 12 and 5 heads; the ends of the range
SHAPES = [(257, 16, 3), (257, 16, 16), (257, 16, 40), (257, 12, 5), (257, 5, 7), (270, 8, 5), (288, 12, 3), (288, 16, 17)]


def _id(s):
    return "T%d_h%d_b%d" % s


@pytest.mark.parametrize("shape", SHAPES, ids=[_id(s) for s in SHAPES])
def test_attention_long_matches_float64(ops, shape):
    """One-hot rows (the output is exactly the selected V row), hidden keys (key T - 1 as runner-up of every row: a padded key that
    leaked in would move the rows beyond the budget), stale signs in the two spare dims, and dense inputs, against
    oracle.clip_oracle.attention_f64 with the error budget of test_gpu_attention.py."""
    T, H, B = shape
    seed = T * 1000 + H * 10 + 7
    qkv = _planted(B, T, H, False, "onehot", seed, stale=True)
    _check_full(ops, qkv, B, T, H, False, exact=True, what="one-hot %s" % _id(shape))
    qkv = _planted(B, T, H, False, "hidden", seed + 1, stale=True)
    _check_full(ops, qkv, B, T, H, False, what="hidden keys %s" % _id(shape))
    qkv = _dense(B, T, H, seed + 2)
    _check_full(ops, qkv, B, T, H, False, what="dense %s" % _id(shape))


@pytest.mark.parametrize("shape", [(257, 16, 3), (288, 5, 7)], ids=_id)
def test_attention_long_largest_scores(ops, shape):
    """Scores up to 62 * 65504^2: the large-offset branch of the softmax keeps the rows finite and one-hot."""
    T, H, B = shape
    qkv = _planted(B, T, H, False, "onehot", 99 + T, stale=False, q_scale=65504.0 / 8.0, k_scale=65504.0)
    _check_full(ops, qkv, B, T, H, False, exact=True, what="largest scores %s" % _id(shape))


@pytest.mark.parametrize("T,causal,H", [(289, False, 16), (257, True, 16), (270, True, 12), (256, False, 16)])
def test_attention_long_rejects_what_no_kernel_serves(ops, T, causal, H):
    from scd_amd._lib import ScdError
    qkv = torch.zeros((2 * T, 3 * 64 * H), dtype=torch.float16, device="cuda")
    with pytest.raises(ScdError) as e:
        ops.attention_f16(qkv, 2, T, H, causal)
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------------ towers
def _l14(v_layers=24, t_layers=12, visual=True, text=True):
    from scd_amd.clip import weights as W
    cfg = dict(W.CLIP_VITL14, v_layers=v_layers, t_layers=t_layers)
    return W.synthetic_clip_state_dict(seed=0, cfg=cfg, visual=visual, text=text)


def _images(n, seed):
    return torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(seed)).half().float()


@pytest.fixture(scope="module")
def l14_2blocks():
    from scd_amd.clip.model import CLIP
    sd = _l14(v_layers=2, t_layers=2)
    return sd, tt._round_clip(sd), CLIP(sd).cuda()


def test_l14_visual_tower_2_blocks_matches_oracle(l14_2blocks):
    """2-block L/14 image tower (257 tokens, patch 14 through the zero-padded K = 640 patch GEMM, width 1024 / 16 heads, out 768)
    against the fp32 oracle.  Measured on MI355X: 1 - cos 1.9e-7, max|err| / max|ref| 5.9e-4."""
    sd, sd16, model = l14_2blocks
    img = _images(6, 141)
    out = model.encode_image(img.cuda()).float().cpu()
    assert out.shape == (6, 768)
    north_star(out, co.clip_encode_image(sd16, img, heads=16), "L/14 visual 2 blocks")


def test_l14_visual_tower_pixels_batch_and_stale_scratch(l14_2blocks):
    """fp16 and fp32 pixels give identical features; an image's features are the same bits alone and inside a batch of 37; and the
    padded columns 588..639 of the patch matrix are written on every call: batch A, then batch B of another size and scale, then A
    again give A's bits twice."""
    _, _, model = l14_2blocks
    enc = model.visual.enc
    img = _images(37, 142)
    a32 = enc.encode_image(img.cuda())
    a16 = enc.encode_image(img.cuda().half())
    assert torch.equal(a32, a16)
    for i in (0, 17, 36):
        one = enc.encode_image(img[i:i + 1].cuda().half())
        assert torch.equal(one[0], a16[i]), i
    A = img[:5].cuda().half()
    B = (_images(11, 143) * 30).cuda().half()
    first = enc.encode_image(A).clone()
    enc.encode_image(B)
    assert torch.equal(enc.encode_image(A), first)


def test_l14_visual_tower_24_blocks_matches_oracle():
    """The full 24-block L/14 image tower on 4 images.  Measured on MI355X: 1 - cos 1.1e-6, max|err| / max|ref| 1.9e-3."""
    from scd_amd.clip.model import CLIP
    sd = _l14(text=False)
    model = CLIP(sd).cuda()
    img = _images(4, 144)
    out = model.encode_image(img.cuda()).float().cpu()
    del model
    north_star(out, co.clip_encode_image(tt._round_clip(sd), img, heads=16), "L/14 visual 24 blocks")


def test_l14_text_tower_matches_oracle_and_trims_bit_exactly():
    """The full 12-block L/14 text tower (width 768, 12 heads, out 768) against the oracle; host ids (trimmed to the batch's last EOT)
    and device ids (all 77 positions) give the same bits.  Measured on MI355X: 1 - cos 8.5e-7, max|err| / max|ref| 1.3e-3."""
    from scd_amd.clip.model import CLIP
    sd = _l14(visual=False)
    model = CLIP(sd).cuda()
    tok = tt._prompts((1, 3, 8, 20, 40, 75), 145)
    short = tt._prompts((2, 5, 9, 11), 146)
    out = model.encode_text(tok).float().cpu()
    assert out.shape == (6, 768)
    north_star(out, co.clip_encode_text(tt._round_clip(sd), tok, heads=12), "L/14 text 12 blocks")
    assert torch.equal(model.encode_text(short), model.encode_text(short.cuda()))


def test_l14_zeroshot_classifier_matches_oracle(l14_2blocks):
    """clip_lang_util.zeroshot_classifier on a 2-block L/14 text tower: per name normalise -> mean -> normalise, [768, names].
    Measured on MI355X: 1 - cos 1.6e-7, max|err| / max|ref| 5.8e-4."""
    import scd_amd.clip as clip
    from scd_amd.local_utils import clip_lang_util as clu
    clip.allow_synthetic()
    sd, sd16, model = l14_2blocks
    names, tmpl = ["red_fox", "tabby", "kit_fox", "zebra", "grey_whale"], clu.imagenet_templates[:9]
    zs = clu.zeroshot_classifier(names, tmpl, model, names_per_batch=2)
    assert zs.shape == (768, 5) and zs.dtype == torch.float16
    ref = no.zeroshot_classifier(names, tmpl, lambda t: co.clip_encode_text(sd16, t.long(), heads=12).numpy(), clip.tokenize)
    north_star(zs.float().cpu().t(), torch.from_numpy(ref).t(), "L/14 zero-shot classifier")


# ------------------------------------------------------------------------------------------------ similarity + top-k at d = 768
@pytest.mark.parametrize("n,v,k", [(300, 21000, 5), (129, 1031, 3), (33100, 1031, 8), (66000, 1031, 1), (300, 21000, 2)])
def test_sim_topk_d768_shapes(ops, n, v, k):
    """Ragged n and V, duplicated names (ties to the lower index), both modes and the argmax, index for index against the float64
    oracle."""
    rs = np.random.RandomState(n + v + 768)
    d = 768
    f = (rs.randn(n, d) / np.sqrt(d)).astype(np.float16)
    w = (rs.randn(d, v) / np.sqrt(d)).astype(np.float16)
    w[:, 5] = w[:, 3]
    wt = ops.transpose_f16(dev(w))
    for mode in ("raw", "softmax"):
        idx, val, fb = ops.sim_topk(dev(f), wt, k, mode, return_fallback=True)
        oi, ov = no.sim_topk(f, w, k, mode)
        assert np.array_equal(idx.cpu().numpy(), oi), mode
        assert np.allclose(val.cpu().numpy(), ov, rtol=1e-5 if mode == "raw" else 2e-4, atol=1e-5 if mode == "raw" else 1e-6), mode
        assert int(fb.item()) <= n // 20
    a, _ = ops.sim_argmax(dev(f), wt)
    assert np.array_equal(a.cpu().numpy(), no.sim_argmax(f, w)[0])


@pytest.mark.parametrize("mode", ["raw", "softmax"])
def test_sim_topk_d768_fallback_rows_exact(ops, mode):
    """40 names one fp16 ulp apart (two identical): rows the certificate cannot settle take the exact float64 pass."""
    n, d, v, k = 100, 768, 3000, 5
    rs = np.random.RandomState(1768)
    base = (rs.randn(d) / np.sqrt(d)).astype(np.float16)
    w = (rs.randn(d, v) / np.sqrt(d)).astype(np.float16)
    for j in range(40):
        col = base.copy()
        pos = rs.randint(0, d, size=3)
        col[pos] = np.nextafter(col[pos], np.float16(10), dtype=np.float16)
        w[:, 100 + 7 * j] = col
    w[:, 100 + 7 * 13] = w[:, 100 + 7 * 2]
    f = (base[None, :].astype(np.float32) * 2 + rs.randn(n, d) * 0.01).astype(np.float16)
    wt = ops.transpose_f16(dev(w))
    idx, val, fb = ops.sim_topk(dev(f), wt, k, mode, return_fallback=True)
    oi, ov = no.sim_topk(f, w, k, mode)
    assert int(fb.item()) >= 3
    assert np.array_equal(idx.cpu().numpy(), oi)
    assert np.allclose(val.cpu().numpy(), ov, rtol=2e-4, atol=1e-6)


def test_sim_topk_d768_frozen_vocabulary(ops):
    n, v, d, k = 700, 5000, 768, 3
    rs = np.random.RandomState(769)
    f = (rs.randn(n, d) / np.sqrt(d)).astype(np.float16)
    w = (rs.randn(d, v) / np.sqrt(d)).astype(np.float16)
    wt = ops.freeze_vocab(ops.transpose_f16(dev(w)))
    try:
        idx, _ = ops.sim_topk(dev(f), wt, k, "softmax")
        oi, _ = no.sim_topk(f, w, k, "softmax")
        assert np.array_equal(idx.cpu().numpy(), oi)
    finally:
        ops.unfreeze_vocab(wt)


# ------------------------------------------------------------------------------------------------ end to end
def test_mains_with_vit_l14_find_the_planted_names(ops):
    import main_unsup as mu
    import main_ptsup as mp
    common = ["--synthetic", "true", "--synthetic_images", "1536", "--synthetic_vocab", "600", "--n_cluster", "8",
              "--clip_model", "ViT-L/14", "--num_common_vote", "10", "--num_common_linear", "2"]
    cand, _ = mu.main(common + ["--cluster", "SSKM", "--topk", "3"])
    assert len(cand) == 8 and set(int(c.split("_")[1]) for c in cand) == set(range(8))
    cand, _ = mu.main(common + ["--cluster", "KM", "--topk", "3"])
    assert set(int(c.split("_")[1]) for c in cand) == set(range(8))
    cand, _ = mp.main(common + ["--cluster", "ConSSKM", "--cluster_size_min", "50", "--cluster_size_max", "400", "--topk", "5"])
    assert set(int(c.split("_")[1]) for c in cand) == set(range(8))
