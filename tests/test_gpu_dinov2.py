"""DINOv2 ViT-B/14 / ViT-L/14 on the device: the register-aware token assembly bit for bit, attention at T = 261, the towers against
the fp32 restatement (tests/dinov2_ref.py) on device-rounded weights, bit-stability, what scd_encoder_create refuses, and the ingest
path and main_unsup.py end to end with --feat_model dinov2_vitb14_reg."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import dinov2_ref as ref  # noqa: E402
import tower_tolerances as tt  # noqa: E402
from oracle import clip_oracle as co  # noqa: E402
from oracle import kmeans_oracle as ko  # noqa: E402
from oracle import synth  # noqa: E402
from test_gpu_attention import _planted, _dense, _check_full  # noqa: E402
from test_dinov2_host import GAMMA_RANGE  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device; they must not be skipped on the GPU box"
    from scd_amd import ops as o
    return o


def north_star(out, want, what):
    gap, rel = tt.metrics(out, want)
    print("%s: 1 - cos %.3e, max|err| / max|ref| %.3e" % (what, gap, rel))
    assert bool(torch.isfinite(out.float()).all()), what
    assert gap < tt.NORTH_STAR[0] and rel <= tt.NORTH_STAR[1], "%s: 1 - cos %.3e, max|err| / max|ref| %.3e" % (what, gap, rel)
    return gap, rel


def _images(n, seed):
    return torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(seed)).half().float()


# ------------------------------------------------------------------------------------------------ 1. token assembly
def _assembly_case(width, R, batch, integer):
    """operands on the host, and the rows the kernels must store: fp32 additions in the order ((patch + bias) + pos), one rounding"""
    T, n_p = 257 + R, 256
    g = torch.Generator().manual_seed(width + 10 * R + batch + (1000 if integer else 0))
    if integer:                                       # sums of three integers in [-3, 3]: every fp32 partial sum of a row is exact
        r = lambda *s: torch.randint(-3, 4, s, generator=g).float()
    else:
        r = lambda *s: torch.randn(*s, generator=g)
    patch, bias, cls, pos = r(batch * n_p, width).half(), r(width), r(width), r(1 + n_p, width)
    reg = r(R, width) if R else None
    if R and not integer:
        reg[0, :8] = torch.tensor([0.0, -0.0, 1e-9, -1e-9, 65504.0, -3.0, 2.0 ** -24, 1.0])         # stored as they are
    want = torch.empty(batch, T, width)
    want[:, 0] = cls + pos[0]
    if R:
        want[:, 1:1 + R] = reg
    want[:, 1 + R:] = (patch.float().view(batch, n_p, width) + bias) + pos[1:]
    return T, patch, bias, cls, pos, reg, want.half().view(batch * T, width)


@pytest.mark.parametrize("width", [768, 1024])
@pytest.mark.parametrize("R", [0, 1, 4])
@pytest.mark.parametrize("batch", [1, 3, 37])
def test_assembly_bit_for_bit(ops, width, R, batch):
    """x[b][0] = cls + pos[0]; x[b][1..R] = registers (no position row); x[b][1 + R + p] = (patch + bias) + pos[1 + p], rounded to
    fp16 once; zero padding rows; the rows' fixed-point LayerNorm statistics.  37 images are no multiple of the kernel's 4 (or 8)
    images per wave.  R = 0 is the launch of every tower without registers: same entry into the same launcher, nreg = 0.

    Statistics: on integer-valued operands every fp32 partial sum is exact and the statistics EQUAL oracle.clip_oracle.row_stats_int of
    the stored rows.  On real-valued operands the kernel's fp32 sums round (a lane adds its 4 * width / 256 <= 16 values in turn, the
    wave reduction adds 6 more times: at most 22 roundings of 2^-24 relative to sum |x| resp. sum x^2, taken as 24, plus the
    rounding to fixed point), so there they are held to that bound around the exact sums."""
    dev = lambda t: None if t is None else t.cuda()
    for integer in (True, False):
        T, patch, bias, cls, pos, reg, want = _assembly_case(width, R, batch, integer)
        out, stats = ops.vit_assemble_f16(dev(patch), dev(bias), dev(cls), dev(pos), dev(reg), batch, T, stats=True)
        torch.cuda.synchronize()
        rows = (batch * T + 255) // 256 * 256
        assert out.shape == (rows, width) and stats.shape == (rows, 2)
        out, stats = out.cpu(), stats.cpu()
        assert torch.equal(out[:batch * T].view(torch.int16), want.view(torch.int16)), integer
        assert not out[batch * T:].view(torch.int16).any() and not stats[batch * T:].any()
        got = stats[:batch * T].numpy()
        if integer:
            assert np.array_equal(got, co.row_stats_int(out[:batch * T]))
        else:
            x = out[:batch * T].double().numpy()
            assert (np.abs(got[:, 0] - x.sum(1) * 2.0 ** 24) <= 24 * 2.0 ** -24 * np.abs(x).sum(1) * 2.0 ** 24 + 1).all()
            assert (np.abs(got[:, 1] - (x * x).sum(1) * 2.0 ** 20) <= 24 * 2.0 ** -24 * (x * x).sum(1) * 2.0 ** 20 + 1).all()
    # without statistics and without a patch bias: the same rows
    n_p = 256
    out2 = ops.vit_assemble_f16(dev(patch), None, dev(cls), dev(pos), dev(reg), batch, T).cpu()
    want2 = want.view(batch, T, width).clone()
    want2[:, 1 + R:] = (patch.float().view(batch, n_p, width) + pos[1:]).half()
    assert torch.equal(out2[:batch * T].view(torch.int16), want2.view(batch * T, width).view(torch.int16))


_CHILD = """
import sys, torch
sys.path.insert(0, %r)
import test_gpu_dinov2 as t
from scd_amd import ops
dev = lambda x: None if x is None else x.cuda()
for width, R, batch in ((768, 4, 37), (1024, 1, 3), (768, 0, 5)):
    for integer in (True, False):
        T, patch, bias, cls, pos, reg, want = t._assembly_case(width, R, batch, integer)
        out, stats = ops.vit_assemble_f16(dev(patch), dev(bias), dev(cls), dev(pos), dev(reg), batch, T, stats=True)
        torch.cuda.synchronize()
        assert torch.equal(out[:batch * T].cpu().view(torch.int16), want.view(torch.int16)), (width, R, batch, integer)
        assert not out[batch * T:].any() and not stats[batch * T:].any()
        if integer:
            assert (stats[:batch * T].cpu().numpy() == t.co.row_stats_int(out[:batch * T].cpu())).all()
print("ASSEMBLY_CHILD_OK")
"""


@pytest.mark.parametrize("rows_per_wave", ["1", "8"])
def test_assembly_other_kernels_child(rows_per_wave):
    """SCD_ASSEMBLE_ROWS (read once per process) selects assemble_visual_kernel (1: a row per wave) or assemble_visual_rows_kernel<8>
    instead of the default <4>: the same rows and statistics, registers included, in a fresh process."""
    import subprocess
    env = dict(os.environ, SCD_ASSEMBLE_ROWS=rows_per_wave)
    r = subprocess.run([sys.executable, "-c", _CHILD % HERE], env=env, cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ASSEMBLY_CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_assembly_refuses_bad_shapes(ops):
    """SCD_EINVAL before anything is launched: registers without their rows, no patch row left, a width the kernels do not take.
    (Every buffer is large enough for the shape asked for.)"""
    from scd_amd._lib import load
    z = torch.zeros(512, 1024, device="cuda")
    z16, out = torch.zeros(512, 1024, dtype=torch.float16, device="cuda"), torch.zeros(512, 1024, dtype=torch.float16, device="cuda")
    for nreg, T, width, reg in ((1, 258, 768, None), (0, 1, 768, None), (4, 5, 768, z.data_ptr()), (0, 257, 640, None), (-1, 257, 768, None)):
        rc = load().scd_vit_assemble_f16(ops.handle(), z16.data_ptr(), None, z.data_ptr(), z.data_ptr(), reg, nreg, 1, T, width,
                                         out.data_ptr(), None, None)
        assert rc == -1, (nreg, T, width)
    torch.cuda.synchronize()
    assert not out.view(torch.int16).any()


# ------------------------------------------------------------------------------------------------ 2. attention at T = 261
@pytest.mark.parametrize("heads,batch", [(12, 5), (16, 3)])
def test_attention_261_tokens(ops, heads, batch):
    """257 + 4 registers, inside the non-causal 256 < T <= 288 range of attention_kernel<9>, with the B/14 and L/14 head counts: one-hot
    rows, key T - 1 hidden as every row's runner-up, dense inputs - the cases and budgets of test_gpu_attention.py."""
    T = 261
    seed = T * 1000 + heads * 10 + 3
    _check_full(ops, _planted(batch, T, heads, False, "onehot", seed, stale=True), batch, T, heads, False, exact=True, what="one-hot")
    _check_full(ops, _planted(batch, T, heads, False, "hidden", seed + 1, stale=True), batch, T, heads, False, what="hidden keys")
    _check_full(ops, _dense(batch, T, heads, seed + 2), batch, T, heads, False, what="dense")


# ------------------------------------------------------------------------------------------------ 3. towers
def _tower(width, layers, registers, seed, **kw):
    """(model on the device, the prepared state dict rounded like the device holds it)"""
    from scd_amd.clip import weights as W
    from scd_amd.clip.model import DinoViT
    sd = W.synthetic_dinov2_state_dict(seed=seed, width=width, layers=layers, registers=registers, gamma=GAMMA_RANGE)
    model = DinoViT(sd, **kw)
    return model.cuda(), ref.round_like_the_device(model._sd)


@pytest.fixture(scope="module")
def b14_reg_2blocks():
    return _tower(768, 2, 4, 31)


@pytest.mark.parametrize("width,registers", [(768, 0), (768, 4), (1024, 4)], ids=["b14", "b14_reg", "l14_reg"])
def test_towers_2_blocks_match_the_restatement(width, registers, b14_reg_2blocks):
    """Two-block towers, 6 images, against the fp32 restatement on the weights the device holds (LayerScale and the input normalisation
    folded, matrices in fp16).  Measured on MI355X (1 - cos, max|err| / max|ref|): B/14 4.1e-7 / 7.5e-4, B/14 reg 4.7e-7 / 6.1e-4,
    L/14 reg 3.4e-7 / 1.2e-3."""
    model, sd16 = b14_reg_2blocks if (width, registers) == (768, 4) else _tower(width, 2, registers, 30 + registers + width // 512)
    img = _images(6, 151)
    out = model.features(img.cuda()).cpu()
    assert out.shape == (6, width) and out.dtype == torch.float32
    assert model._enc.desc["tokens"] == 257 + registers and model._enc.desc.get("registers", 0) == registers
    north_star(out, ref.forward(sd16, img, torch.float32), "DINOv2 width %d, %d registers, 2 blocks" % (width, registers))
    unit = model.features(img.cuda(), normalize=True)
    assert torch.allclose(unit.norm(dim=-1), torch.ones(6, device="cuda"), atol=2e-3)


def test_tower_b14_reg_12_blocks_matches_the_restatement():
    """The full-depth B/14 tower with four registers, 4 images.  Measured on MI355X: 1 - cos 9.4e-7, max|err| / max|ref| 1.7e-3."""
    model, sd16 = _tower(768, 12, 4, 33)
    img = _images(4, 152)
    out = model.features(img.cuda()).cpu()
    del model
    north_star(out, ref.forward(sd16, img, torch.float32), "DINOv2 B/14 reg, 12 blocks")


def test_tower_b14_reg_12_blocks_with_outlier_weights_matches_the_restatement():
    """The pathologies of trained checkpoints (tests/outlier_weights.py, DINO keys: massive-activation channels, LayerNorm gains over
    two decades, sharp heads, bias spikes) under LayerScale gains in GAMMA_RANGE, the range test_dinov2_host.py's fold-cost test
    holds on.  Measured on MI355X: 1 - cos 9.6e-7, max|err| / max|ref| 7.4e-4."""
    import outlier_weights as ow
    from scd_amd.clip import weights as W
    from scd_amd.clip.model import DinoViT
    sd = W.synthetic_dinov2_state_dict(seed=34, width=768, layers=12, registers=4, gamma=GAMMA_RANGE)
    ch = ow.pathologise(sd, "blocks.", ow.DINO_KEYS, 768, 12, 134, emb_keys=("cls_token", "pos_embed", "register_tokens"))
    sd["patch_embed.proj.bias"][ch] += 3.0
    sd["norm.weight"] = ow._loguniform(np.random.RandomState(334), 768, 0.02, 8.0)
    model = DinoViT(sd)
    sd16 = ref.round_like_the_device(model._sd)
    img = _images(4, 153)
    out = model.cuda().features(img.cuda()).cpu()
    del model
    north_star(out, ref.forward(sd16, img, torch.float32), "DINOv2 B/14 reg, 12 blocks, outlier weights")


# ------------------------------------------------------------------------------------------------ 4. bits
def test_tower_pixels_batch_and_stale_scratch(b14_reg_2blocks):
    """fp16 and fp32 pixels give identical features; an image's features are the same bits alone and inside a batch of 37; batch A,
    then batch B of another size and scale, then A again give A's bits twice (stale scratch, the zero-padded patch columns 588..639)."""
    model, _ = b14_reg_2blocks
    enc = model._enc
    img = _images(37, 154)
    a32 = enc.encode_image(img.cuda())
    a16 = enc.encode_image(img.cuda().half())
    assert torch.equal(a32, a16)
    for i in (0, 17, 36):
        one = enc.encode_image(img[i:i + 1].cuda().half())
        assert torch.equal(one[0], a16[i]), i
    A = img[:5].cuda().half()
    B = (_images(11, 155) * 30).cuda().half()
    first = enc.encode_image(A).clone()
    enc.encode_image(B)
    assert torch.equal(enc.encode_image(A), first)


# ------------------------------------------------------------------------------------------------ 5. scd_encoder_create
def _create(ops, desc, n_extra=0, null_registers=False):
    from scd_amd import _lib
    import ctypes as C
    z = torch.zeros(4 * 1024 * 1024, dtype=torch.float32, device="cuda")      # every pointer: large enough for any weight of the towers below
    n = 9 + 12 * desc["layers"] + n_extra
    ptrs = [z.data_ptr()] * n
    if desc["kind"] == 2:
        ptrs[8] = None                                                       # no projection
    if null_registers:
        ptrs[-1] = None
    arr = (C.c_void_p * n)(*ptrs)
    enc = C.c_void_p()
    d = _lib.EncoderDesc(**desc)
    rc = _lib.load().scd_encoder_create(ops.handle(), C.byref(d), arr, n, C.byref(enc))
    if rc == 0:
        _lib.load().scd_encoder_destroy(enc)
    return rc


def test_encoder_create_refuses_bad_register_descriptors(ops):
    base = dict(kind=2, width=768, layers=1, heads=12, mlp_dim=3072, tokens=261, patch=14, image=224, vocab=0, out_dim=0, act=1,
                ln_eps=1e-6, registers=4)
    assert _create(ops, base, 1) == 0
    assert _create(ops, dict(base, tokens=257, registers=0), 0) == 0
    assert _create(ops, dict(base, tokens=288, registers=31), 1) == 0
    assert _create(ops, base, 0) == -1                                        # the register rows' pointer is missing
    assert _create(ops, dict(base, tokens=257, registers=0), 1) == -1         # one pointer too many
    assert _create(ops, base, 1, null_registers=True) == -1
    assert _create(ops, dict(base, tokens=257), 1) == -1                      # tokens != 256 + 1 + registers
    assert _create(ops, dict(base, tokens=262), 1) == -1
    assert _create(ops, dict(base, tokens=289, registers=32), 1) == -1        # beyond the attention ladder
    assert _create(ops, dict(base, registers=-1, tokens=256), 0) == -1
    assert _create(ops, dict(base, kind=0, out_dim=512), 1) == -1             # registers with a CLIP visual tower
    assert _create(ops, dict(base, kind=1, tokens=77, vocab=49408, out_dim=512, patch=0, image=0), 1) == -1
    assert _create(ops, dict(base, patch=16, tokens=201), 1) == -1            # 196 + 1 + 4: no attention kernel for T = 201


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_files_to_dinov2_features_equal_extract_feature(tmp_path, b14_reg_2blocks):
    import argparse
    from scd_amd import images, naming
    from scd_amd.clip import weights as W
    from scd_amd.clip.model import CLIP
    from test_image_ingest import _write_files, _reference_tensor
    paths = _write_files(str(tmp_path))
    n = len(paths)
    targets, mask_lab = np.arange(n) % 3, np.arange(n) < 4
    ref_imgs = _reference_tensor(paths)
    dino, _ = b14_reg_2blocks
    clip_model = CLIP(W.synthetic_clip_state_dict(seed=0, cfg=dict(v_layers=2, t_layers=2))).cuda()
    models = {"dinov2_vitb14_reg": dino, "clip": clip_model}
    got = images.extract_features_from_files(paths, targets, mask_lab, models, batch_size=4, threads=3)
    for name, model in models.items():
        args = argparse.Namespace(feat_model=name, train_classes=sorted(set(targets[mask_lab].tolist())))
        want = naming.extract_feature(model, ((ref_imgs[s:s + 4], targets[s:s + 4], None, mask_lab[s:s + 4]) for s in range(0, n, 4)), args)
        for k in want:
            assert got[name][k].dtype == want[k].dtype and np.array_equal(got[name][k], want[k]), (name, k)
    assert got["dinov2_vitb14_reg"]["all_feats"].shape == (n, 768) and got["dinov2_vitb14_reg"]["all_feats"].dtype == np.float32


def test_main_unsup_with_dinov2_vitb14_reg(tmp_path, monkeypatch):
    """A 2-block synthetic dinov2_vitb14_reg4_pretrain.pth (37 x 37 position table) under $SCD_ROOT: --extract_feat true --image_list
    writes dinov2_vitb14_reg_{dataset}_all.pt (float32 unit rows [N, 768]), clusters it with KM and completes the vote."""
    import importlib
    import scd_amd.clip as clip
    from scd_amd.clip import weights as W
    from test_image_ingest import _write_files
    imgdir = tmp_path / "imgs"
    imgdir.mkdir()
    paths = _write_files(str(imgdir))
    n = len(paths)
    targets, mask_lab = np.arange(n) % 2, np.arange(n) < 4
    with open(tmp_path / "list.csv", "w") as f:
        f.write("path,target,labelled\n")
        for p, t, m in zip(paths, targets, mask_lab):
            f.write("imgs/%s,%d,%d\n" % (os.path.basename(p), t, int(m)))
    model_root = tmp_path / "models"
    for sub in ("clip", "dinov2", "data"):
        (model_root / sub).mkdir(parents=True)
    sd = W.synthetic_clip_state_dict(seed=0, cfg=dict(v_layers=2, t_layers=2))
    torch.save({k: (v.half() if v.dim() >= 2 else v) for k, v in sd.items()}, model_root / "clip" / "ViT-B-16.pt")
    dsd = W.synthetic_dinov2_state_dict(seed=35, width=768, layers=2, registers=4, grid=37)
    torch.save(dsd, model_root / "dinov2" / "dinov2_vitb14_reg4_pretrain.pth")
    nouns = ["noun_%03d" % i for i in range(40)]
    (model_root / "data" / "wordnet_all_noun.txt").write_text("\n".join(nouns) + "\n")
    zw = torch.nn.functional.normalize(torch.randn(512, 40, generator=torch.Generator().manual_seed(2)), dim=0)
    monkeypatch.setenv("SCD_ROOT", str(model_root))
    monkeypatch.setenv("SCD_DATA", str(model_root / "data"))
    monkeypatch.setattr(clip, "_tokenizer", None)
    mu = importlib.import_module("main_unsup")
    root = tmp_path / "run"
    (root / "zeroshot_weights").mkdir(parents=True)
    torch.save(zw, root / "zeroshot_weights" / "zeroshot_weights_all_nouns_vit_b_16.pt")
    cand, u_preds = mu.main(["--root_dir", str(root), "--dataset_name", "tiny", "--feat_model", "dinov2_vitb14_reg", "--extract_feat", "true",
                             "--run_cluster", "true", "--cluster", "KM", "--n_cluster", "2", "--topk", "3",
                             "--image_list", str(tmp_path / "list.csv")])
    assert len(cand) == 2 and len(u_preds) == int((~mask_lab).sum())
    cache = torch.load(root / "extracted_features" / "dinov2_vitb14_reg_tiny_all.pt", weights_only=False)
    feats = cache["all_feats"]
    assert feats.shape == (n, 768) and feats.dtype == np.float32
    assert np.allclose(np.linalg.norm(feats.astype(np.float64), axis=1), 1.0, atol=2e-3)
    assert (root / "extracted_features" / "clip_tiny_all.pt").exists()
    # the cache holds the loader's tower: the file's weights, default folds
    model = clip.load_dinov2("dinov2_vitb14_reg").cuda()
    from test_image_ingest import _reference_tensor
    want = model.features(_reference_tensor(paths).cuda(), normalize=True).cpu().numpy()
    assert np.array_equal(feats, want)


def test_kmeans_at_1024_dimensions_equals_the_oracle(ops, monkeypatch):
    """The L/14 towers' features are 1024-d: one small sklearn-surface K-Means fit at D = 1024 (above the 768 the fast E-step serves)
    gives the oracle's labels."""
    from scd_amd.cluster import KMeans
    monkeypatch.setenv("SCD_SKLEARN_COMPAT", "1.7.2")
    x, _, _ = synth.clustered_features(700, 1024, 6, seed=41, noise=0.5)
    x = np.ascontiguousarray(x, dtype=np.float32)
    lab = KMeans(n_clusters=6, random_state=0).fit(x).labels_
    olab, _, _, _ = ko.sklearn_kmeans(x, 6, 0, "auto", compat="1.7.2")
    assert np.array_equal(np.asarray(lab), olab)
