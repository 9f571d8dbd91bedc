"""Image files -> feature caches (scd_amd/images.py, scd_amd/csrc/image.hip): the reference's ImageFolder + CLIP `preprocess` path
(main_unsup.py:237,271-311) restated on the device, pinned bit for bit against Pillow and the numpy restatement in image_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pil():
    try:
        from PIL import Image
    except ImportError:
        pytest.fail("these tests decode and resize with Pillow (PIL), which is not installed")
    return Image


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ CPU: restatement and planner
RESIZE_SHAPES = [(500, 375), (375, 500), (100, 80), (80, 100), (224, 300), (300, 224), (224, 224), (225, 225), (223, 223), (1, 7),
                 (7, 1), (3, 500), (224, 5000), (5000, 224), (2000, 1500), (4100, 300), (300, 4500), (16, 16), (1, 1), (640, 427)]


@pytest.mark.parametrize("w,h", RESIZE_SHAPES)
def test_restatement_equals_pil_resize(w, h):
    Image = _pil()
    img = _noise(w, h, w * 7919 + h)
    rw, rh = R.resize_size(w, h)
    want = np.asarray(Image.fromarray(img, "RGB").resize((rw, rh), Image.BICUBIC)) if (rw, rh) != (w, h) else img
    assert np.array_equal(R.pil_resize(img, rw, rh), want)


def test_size_and_crop_rules():
    from scd_amd import images
    assert R.resize_size(500, 375) == (298, 224) and R.resize_size(375, 500) == (224, 298)     # int(224 * 500 / 375) = int(298.67)
    assert R.resize_size(224, 300) == (224, 300)                                               # short edge already 224: unchanged
    assert R.crop_offset(299) == 38 and R.crop_offset(297) == 36                               # 37.5 -> 38, 36.5 -> 36 (ties to even)
    assert images.geometry(500, 375)[:4] == (298, 224, 37, 0)
    assert images.geometry(334, 250)[:4] == (299, 224, 38, 0)
    assert images.geometry(250, 332)[:4] == (224, 297, 0, 36)
    assert images.geometry(224, 300)[:4] == (224, 300, 0, 38)
    rng = np.random.default_rng(3)
    for w, h in [tuple(int(v) for v in rng.integers(1, 3000, 2)) for _ in range(300)] + RESIZE_SHAPES:
        rw, rh = R.resize_size(w, h)
        assert images.geometry(w, h)[:4] == (rw, rh, R.crop_offset(rw), R.crop_offset(rh)), (w, h)


def test_planner_taps_equal_restatement():
    from scd_amd import images
    pairs = [(500, 298), (375, 224), (80, 224), (100, 280), (7, 1568), (1, 224), (2000, 298), (1500, 224), (4100, 3061), (16384, 224),
             (16384, 300), (225, 224), (223, 224), (3, 37333), (5000, 224)]
    rng = np.random.default_rng(5)
    pairs += [(int(a), int(b)) for a, b in zip(rng.integers(1, 4096, 40), rng.integers(1, 700, 40))]
    for n_in, n_out in pairs:
        n = min(n_out, 224)
        off = (n_out - n) // 2
        want = R.coeffs(n_in, n_out)[off:off + n]
        got = images.plan_axis(n_in, n_out, off, n)
        assert len(got) == n
        for (f0, k0), (f1, k1) in zip(want, got):
            assert f0 == f1 and np.array_equal(k0, k1.astype(np.int64)), (n_in, n_out)
    big = images.plan_axis(4000, 224)
    assert max(len(k) for _, k in big) >= 70                      # no tap cap: a 4,000 px edge needs ~75 taps


def test_plan_cache_key_and_size_bounds():
    from scd_amd import _lib, images
    assert images.geometry(500, 375, 256, 224)[:4] == (341, 256, 58, 16)          # size and crop are part of the cached plan's key
    assert images.geometry(500, 375, 224, 224)[:4] == (298, 224, 37, 0)
    assert images.geometry(500, 375, 256, 200)[:4] == (341, 256, 70, 28)
    for size, crop in ((65536 + 224, 224), (224, 225), (0, 0)):
        with pytest.raises(_lib.ScdError):
            images.geometry(500, 375, size, crop)
    with pytest.raises(_lib.ScdError):
        images.geometry(65537, 300)


def test_normalize_lut_is_torch_recipe():
    from scd_amd import images
    lut = images.normalize_lut()
    assert lut.dtype == torch.float16 and lut.shape == (3, 256)
    assert np.array_equal(lut.numpy().view(np.uint16), R.normalize_lut().astype(np.float16).view(np.uint16))


def test_batch_plan_layout():
    from scd_amd import images
    sizes = [(500, 375), (375, 500), (500, 375), (224, 300)]
    descs, plan, pb, wb = images.batch_plan(sizes)
    assert pb == sum(w * h * 3 for w, h in sizes)
    assert list(descs["src_off"]) == [0, 562500, 1125000, 1687500]
    assert descs["plan_x"][0] == descs["plan_x"][2] and descs["plan_x"][0] != descs["plan_x"][1]     # one plan per size in a batch
    assert wb == int((descs["rows"] * 224 * 3).sum())
    for d, (w, h) in zip(descs, sizes):
        g = images.geometry(w, h)
        assert (d["w"], d["h"], d["row0"], d["rows"]) == (w, h, g[4], g[5])
        assert 0 <= d["row0"] and d["row0"] + d["rows"] <= h
    assert descs["rows"][3] == 224                                   # identity: exactly the crop's rows


def test_image_folder_listing_and_csv(tmp_path):
    from scd_amd import images
    for rel in ["b/x2.JPG", "b/x1.png", "b/sub/z.jpeg", "a/q.webp", "a/notes.txt", "c/.keep"]:
        p = tmp_path / "tree" / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")
    paths, targets, c2i = images.list_image_folder(str(tmp_path / "tree"))
    rel = [os.path.relpath(p, tmp_path / "tree") for p in paths]
    assert c2i == {"a": 0, "b": 1, "c": 2}
    assert rel == ["a/q.webp", "b/x1.png", "b/x2.JPG", os.path.join("b", "sub", "z.jpeg")] and targets == [0, 1, 1, 1]
    (tmp_path / "list.csv").write_text("path,target,labelled\ntree/a/q.webp,0,1\ntree/b/x1.png,1,0\n")
    p, t, m = images.read_image_list(str(tmp_path / "list.csv"))
    assert p == [str(tmp_path / "tree/a/q.webp"), str(tmp_path / "tree/b/x1.png")]
    assert t.tolist() == [0, 1] and m.tolist() == [True, False]


def test_unreadable_file_names_its_path(tmp_path):
    _pil()
    from scd_amd import images
    bad = tmp_path / "broken.jpg"
    bad.write_bytes(b"not a jpeg at all")
    with pytest.raises(OSError, match="broken.jpg"):
        images.load_rgb(str(bad))


# ------------------------------------------------------------------------------------------------ GPU
def _run_kernel(imgs):
    from scd_amd import images
    out = images.Preprocessor()(imgs)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


@pytest.mark.gpu
def test_kernel_equals_pillow_fixture():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    z = np.load(os.path.join(ROOT, "tests", "golden", "image_preprocess.npz"))
    imgs, o = [], 0
    for h, w in z["shapes"]:
        imgs.append(z["src"][o:o + h * w * 3].reshape(h, w, 3))
        o += h * w * 3
    got = _run_kernel(imgs)
    assert got.shape == z["out"].shape and np.array_equal(_bits(got), _bits(z["out"]))
    for i, im in enumerate(imgs):                                    # a batch of 1 gives the same image
        assert np.array_equal(_bits(_run_kernel([im])[0]), _bits(z["out"][i]))


@pytest.mark.gpu
def test_kernel_equals_restatement_mixed_batch():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    # odd crop offset (334x250), identity (224x300, 5000x224), upscale (100x80, 3x500: 224x37333), an edge over 4k (4500x230,
    # 230x4200), ImageNet sizes, a 1-px edge
    shapes = [(334, 250), (224, 300), (100, 80), (4500, 230), (500, 375), (375, 500), (3, 500), (5000, 224), (230, 4200), (1, 7),
              (250, 332)]
    imgs = [_noise(w, h, 100 + i) for i, (w, h) in enumerate(shapes)]
    got = _run_kernel(imgs)
    for i, im in enumerate(imgs):
        assert np.array_equal(_bits(got[i]), _bits(R.preprocess_f16(im))), shapes[i]
    one = _run_kernel([imgs[0]])
    assert np.array_equal(_bits(one[0]), _bits(got[0]))


@pytest.mark.gpu
def test_kernel_out_of_range_descriptor_gives_nan():
    """An image whose descriptor reaches past the declared pixel bytes is not read: its pixels are NaN, the others exact.  (The
    buffer itself holds every image: only the declared size is short.)"""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from scd_amd import images
    imgs = [_noise(500, 375, 1), _noise(100, 80, 2), _noise(334, 250, 3)]
    descs, plan, pb, wb = images.batch_plan([(im.shape[1], im.shape[0]) for im in imgs])
    lay = images._Layout(descs, plan, pb)
    host = np.zeros(lay.total, dtype=np.uint8)
    images._pack(host, lay, descs, plan, imgs)
    lay.pixel_bytes = pb - 1
    out = images.Preprocessor().run(torch.from_numpy(host).cuda(), lay, wb)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.isnan(out[2].astype(np.float32)).all()
    for i in range(2):
        assert np.array_equal(_bits(out[i]), _bits(R.preprocess_f16(imgs[i])))


def _write_files(d):
    """JPEG and PNG files of several sizes and modes (RGB, grayscale, RGBA, CMYK, palette)."""
    Image = _pil()
    specs = [("rgb.jpg", "RGB", (500, 375)), ("gray.jpg", "L", (375, 500)), ("cmyk.jpg", "CMYK", (334, 250)), ("rgba.png", "RGBA", (224, 300)),
             ("rgb.png", "RGB", (100, 80)), ("pal.png", "P", (640, 427)), ("gray.png", "L", (260, 230)), ("big.jpg", "RGB", (4300, 240)),
             ("tiny.png", "RGB", (3, 9)), ("rgb2.jpg", "RGB", (500, 333)), ("la.png", "LA", (230, 230))]
    paths = []
    for i, (name, mode, (w, h)) in enumerate(specs):
        rng = np.random.default_rng(i)
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(xx * (3 + c) + yy * (5 - c)) % 256 for c in range(3)], -1) + rng.integers(-20, 21, (h, w, 3))
        im = Image.fromarray(np.clip(base, 0, 255).astype(np.uint8), "RGB")
        if mode == "RGBA":
            im = im.convert("RGBA")
            im.putalpha(Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8), "L"))
        elif mode == "P":
            im = im.convert("P")
        elif mode != "RGB":
            im = im.convert(mode)
        p = os.path.join(d, name)
        im.save(p, quality=90) if name.endswith(".jpg") else im.save(p)
        paths.append(p)
    return paths


def _reference_tensor(paths):
    """The reference's fp32 [N, 3, 224, 224]: pil_loader, Resize(224, BICUBIC) with torchvision's size rule on the PIL image,
    CenterCrop(224), ToTensor, Normalize(CLIP mean / std) - with Pillow and torch, not the library."""
    Image = _pil()
    from scd_amd.images import CLIP_MEAN, CLIP_STD
    out = []
    for p in paths:
        with open(p, "rb") as f:
            im = Image.open(f).convert("RGB")
        w, h = im.size
        rw, rh = R.resize_size(w, h)
        if (rw, rh) != (w, h):
            im = im.resize((rw, rh), Image.BICUBIC)
        top, left = R.crop_offset(rh), R.crop_offset(rw)
        im = im.crop((left, top, left + 224, top + 224))
        t = torch.from_numpy(np.array(im, dtype=np.uint8, copy=True)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        out.append(t.sub_(torch.as_tensor(CLIP_MEAN).view(-1, 1, 1)).div_(torch.as_tensor(CLIP_STD).view(-1, 1, 1)))
    return torch.stack(out)


def _towers():
    from scd_amd.clip import weights as W
    from scd_amd.clip.model import CLIP, DinoViT
    clip_model = CLIP(W.synthetic_clip_state_dict(seed=0, cfg=dict(v_layers=2, t_layers=2))).cuda()
    dino = DinoViT(W.synthetic_dino_state_dict(seed=1, layers=2)).cuda()
    return clip_model, dino


@pytest.mark.gpu
def test_files_to_features_equal_extract_feature(tmp_path):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import argparse
    from scd_amd import images, naming
    paths = _write_files(str(tmp_path))
    n = len(paths)
    targets = np.arange(n) % 3
    mask_lab = np.arange(n) < 4
    ref_imgs = _reference_tensor(paths)
    clip_model, dino = _towers()
    for bs in (256, 4):                                              # 4: three batches through both staging slots
        got = images.extract_features_from_files(paths, targets, mask_lab, {"dino_vit": dino, "clip": clip_model}, batch_size=bs,
                                                 threads=3)
        for name, model in (("dino_vit", dino), ("clip", clip_model)):
            args = argparse.Namespace(feat_model=name, train_classes=sorted(set(targets[mask_lab].tolist())))

            def loader():
                for s in range(0, n, bs):
                    yield ref_imgs[s:s + bs], targets[s:s + bs], None, mask_lab[s:s + bs]
            want = naming.extract_feature(model, loader(), args)
            g = got[name]
            assert set(g) == set(want) == {"all_feats", "mask_lab", "mask_cls", "targets"}
            for k in want:
                assert g[k].dtype == want[k].dtype and g[k].shape == want[k].shape, (name, k)
                assert np.array_equal(g[k], want[k]), (name, k, bs)
            assert g["all_feats"].dtype == (np.float16 if name == "clip" else np.float32)


@pytest.mark.gpu
def test_files_to_features_growing_batches(tmp_path):
    """Files in ascending size, two per batch: the staging slots are reallocated at batches 2, 3, ... while the towers of earlier
    batches are still queued on the compute stream.  The features stay bit-equal to naming.extract_feature."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import argparse
    from scd_amd import images, naming
    paths = _write_files(str(tmp_path))
    sizes = [images.load_rgb(p).shape for p in paths]
    paths = [p for _, p in sorted(zip([h * w for h, w, _ in sizes], paths))]
    n = len(paths)
    targets = np.arange(n) % 3
    mask_lab = np.arange(n) < 4
    ref_imgs = _reference_tensor(paths)
    clip_model, dino = _towers()
    models = {"dino_vit": dino, "clip": clip_model}
    got = images.extract_features_from_files(paths, targets, mask_lab, models, batch_size=2, threads=2)
    for name, model in models.items():
        args = argparse.Namespace(feat_model=name, train_classes=sorted(set(targets[mask_lab].tolist())))
        want = naming.extract_feature(model, ((ref_imgs[s:s + 2], targets[s:s + 2], None, mask_lab[s:s + 2]) for s in range(0, n, 2)),
                                      args)
        for k in want:
            assert got[name][k].dtype == want[k].dtype and np.array_equal(got[name][k], want[k]), (name, k)


@pytest.mark.gpu
def test_main_unsup_image_list_writes_the_images_pt_caches(tmp_path, monkeypatch):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import importlib
    import scd_amd.clip as clip
    from scd_amd.clip import weights as W
    imgdir = tmp_path / "imgs"
    imgdir.mkdir()
    paths = _write_files(str(imgdir))
    n = len(paths)
    targets = np.arange(n) % 2
    mask_lab = np.arange(n) < 4                                       # labelled rows first (MergedDataset order)
    with open(tmp_path / "list.csv", "w") as f:
        f.write("path,target,labelled\n")
        for p, t, m in zip(paths, targets, mask_lab):
            f.write("imgs/%s,%d,%d\n" % (os.path.basename(p), t, int(m)))
    torch.save(dict(images=_reference_tensor(paths), targets=targets, mask_lab=mask_lab), tmp_path / "images.pt")
    model_root = tmp_path / "models"
    for sub in ("clip", "dino", "data"):
        (model_root / sub).mkdir(parents=True)
    sd = W.synthetic_clip_state_dict(seed=0, cfg=dict(v_layers=2, t_layers=2))
    torch.save({k: (v.half() if v.dim() >= 2 else v) for k, v in sd.items()}, model_root / "clip" / "ViT-B-16.pt")
    torch.save(W.synthetic_dino_state_dict(seed=1, layers=2), model_root / "dino" / "dino_vitbase16_pretrain.pth")
    nouns = ["noun_%03d" % i for i in range(40)]
    (model_root / "data" / "wordnet_all_noun.txt").write_text("\n".join(nouns) + "\n")
    zw = torch.nn.functional.normalize(torch.randn(512, 40, generator=torch.Generator().manual_seed(2)), dim=0)
    monkeypatch.setenv("SCD_ROOT", str(model_root))
    monkeypatch.setenv("SCD_DATA", str(model_root / "data"))
    monkeypatch.setattr(clip, "_tokenizer", None)
    mu = importlib.import_module("main_unsup")
    caches = {}
    for tag, extra in (("pt", ["--images_pt", str(tmp_path / "images.pt")]), ("list", ["--image_list", str(tmp_path / "list.csv")])):
        root = tmp_path / tag
        (root / "zeroshot_weights").mkdir(parents=True)
        torch.save(zw, root / "zeroshot_weights" / "zeroshot_weights_all_nouns_vit_b_16.pt")
        mu.main(["--root_dir", str(root), "--dataset_name", "tiny", "--feat_model", "dino_vit", "--extract_feat", "true", "--run_cluster",
                 "true", "--cluster", "KM", "--n_cluster", "2", "--topk", "3"] + extra)
        caches[tag] = {f: torch.load(root / "extracted_features" / f, weights_only=False)
                       for f in ("dino_vit_tiny_all.pt", "clip_tiny_all.pt")}
    for f, want in caches["pt"].items():
        got = caches["list"][f]
        assert set(got) == set(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (f, k)
