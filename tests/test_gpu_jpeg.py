"""The device JPEG decoder (scd_amd/jpeg.py, scd_amd/csrc/jpeg.hip) against Pillow's pixels in tests/golden/jpeg_decode.npz (files
Pillow's encoder wrote, up to 250 x 187) and tests/golden/jpeg_decode_foreign.npz (photograph sizes, scans laid against the entropy
kernel's byte window, other encoders' headers and streams), its status path on the reject fixtures, and decode='device' of the ingest
path against decode='pil' (docs/design/ingest.md)."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from jpeg_cases import ACCEPTED, CASES, FOREIGN, FOREIGN_ACCEPTED, first_bad_band  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _decode(datas):
    from scd_amd import jpeg
    images, status = jpeg.JpegDecoder().decode(datas)
    torch.cuda.synchronize()
    return [im.cpu().numpy() for im in images], status


def _check(case, got):
    assert got.dtype == np.uint8 and got.shape == (case.h, case.w, 3), case.name
    if case.pixels is not None:
        assert np.array_equal(got, case.pixels), case.name
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == case.sha, (case.name, "first band that differs",
                                                                                            first_bad_band(case, got))


@pytest.fixture(scope="module")
def mixed_batch():
    """Every accepted fixture in one batch, decoded once and shared."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _decode([c.data for c in ACCEPTED])


def test_all_accepted_fixtures_in_one_batch(mixed_batch):
    images, status = mixed_batch
    assert status.dtype == np.int32 and not status.any(), status
    assert len(images) == len(ACCEPTED) >= 50
    for c, got in zip(ACCEPTED, images):
        _check(c, got)


def test_batch_of_one_and_repeat_give_the_same_bytes(mixed_batch):
    for tail in ("250x187_420_q90", "_420_q3", "_422_q75rst", "_gray_q100"):
        c = next(c for c in ACCEPTED if c.name.endswith(tail))
        images, status = _decode([c.data])
        assert status.tolist() == [0]
        _check(c, images[0])
    again, status = _decode([c.data for c in ACCEPTED])
    assert not status.any()
    for a, b in zip(mixed_batch[0], again):
        assert np.array_equal(a, b)


def test_reject_fixtures_get_a_status_and_leave_the_rest_exact():
    """The fixtures that pass the parser but not the decoder (cut scan, bad code, both range-guard files), between good ones: each gets
    the status the CPU decoder gives it (tests/test_jpeg_host.py: the same bytes through the same functions on the host, and under the
    host sanitizers), its pixels are not written, and the other images are exact."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from scd_amd import jpeg
    bad = [c for c in CASES if c.reason == 0 and c.status != 0]
    assert sorted(c.name for c in bad) == ["rej_bad_code", "rej_cut_scan", "rej_range_guard", "rej_sample_range"]
    for c in bad:                                                   # the host first: the device sees only what the CPU run has ended on
        with pytest.raises(jpeg.JpegDecodeError) as e:
            jpeg.decode_jpeg_host(c.data)
        assert e.value.status == c.status
    good = [c for c in ACCEPTED if c.w <= 64][:9]
    order = [good[0], bad[0], good[1], good[2], bad[1], bad[2], good[3], good[4], good[5], bad[3], good[6], good[7], good[8]]
    images, status = _decode([c.data for c in order])
    assert status.tolist() == [c.status for c in order]
    for c, got in zip(order, images):
        if c.status:
            assert not got.any(), c.name                            # untouched: the decoder's buffer starts as zeros
        else:
            _check(c, got)


def test_unsupported_file_is_the_callers_to_sort_out():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from scd_amd import jpeg
    prog = next(c for c in CASES if c.name == "rej_progressive")
    with pytest.raises(jpeg.JpegUnsupported):
        jpeg.JpegDecoder().decode([ACCEPTED[0].data, prog.data])


# ------------------------------------------------------------------------------------------------ the second fixture file
def _interleaved():
    """Every accepted case of the second file with the accepted cases of the first between them."""
    out = []
    for k, c in enumerate(FOREIGN_ACCEPTED):
        out.append(c)
        out += ACCEPTED[k:k + 1]
    return out + ACCEPTED[len(FOREIGN_ACCEPTED):]


@pytest.fixture(scope="module")
def foreign_batch():
    """The mixed batch, decoded once and shared: (cases, images, status)."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    order = _interleaved()
    images, status = _decode([c.data for c in order])
    return order, images, status


def test_foreign_fixtures_mixed_with_the_old_in_one_batch(foreign_batch):
    """Photograph sizes and strips (the second to fifth trip of the colour kernel's x loop, 18 trips of its y loop), groups of blocks
    that read past the LDS window into global memory, stuffed pairs and RSTn markers across the window's end and across a 16-byte
    line, and the header and stream variants of other encoders: all equal to Pillow, status 0.  A large image that differs is reported
    with its first band of 16 rows that does."""
    order, images, status = foreign_batch
    assert len(order) == len(FOREIGN_ACCEPTED) + len(ACCEPTED) and len(FOREIGN_ACCEPTED) >= 80
    assert status.dtype == np.int32 and not status.any(), [(c.name, int(s)) for c, s in zip(order, status) if s]
    for c, got in zip(order, images):
        _check(c, got)


def test_foreign_batch_reversed_gives_the_same_bytes(foreign_batch):
    order, images, _ = foreign_batch
    again, status = _decode([c.data for c in order[::-1]])
    assert not status.any()
    for c, a, b in zip(order, images, again[::-1]):
        assert np.array_equal(a, b), c.name


def test_window_and_size_cases_alone_and_last_in_a_batch(foreign_batch):
    """Each window case and each size case as a batch of one, and each window case as the last file of a batch behind a file whose
    length is no multiple of 16 (its window then ends in the data section's last bytes, which are loaded byte by byte): the same bytes
    as in the mixed batch."""
    order, images, _ = foreign_batch
    mixed = {c.name: im for c, im in zip(order, images)}
    before = next(c for c in ACCEPTED if len(c.data) % 16 != 0 and c.w <= 64)
    solo = [c for c in FOREIGN_ACCEPTED if c.name.startswith(("win_", "size_"))]
    assert len(solo) == 55
    for c in solo:
        got, status = _decode([c.data])
        assert status.tolist() == [0], c.name
        _check(c, got[0])
        assert np.array_equal(got[0], mixed[c.name]), c.name
        if c.name.startswith("win_"):
            got, status = _decode([before.data, c.data])
            assert status.tolist() == [0, 0], c.name
            assert np.array_equal(got[0], mixed[before.name]) and np.array_equal(got[1], mixed[c.name]), c.name


def test_foreign_status_cases_get_the_hosts_status_and_leave_the_rest_exact():
    """A fill byte before an RSTn inside the scan, and an RSTn with the wrong number: Pillow decodes both, the entropy decoder follows
    neither (marker_in_scan).  Between good files each gets the status the CPU decoder gives it, its pixels are not written, and its
    neighbours are exact."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from scd_amd import jpeg
    bad = [c for c in FOREIGN if c.reason == 0 and c.status != 0]
    assert [c.name for c in bad] == ["s_rst_fill", "s_rst_wrong_number"] and [c.status for c in bad] == [4, 4]
    for c in bad:                                                   # the host first: the device sees only what the CPU run has ended on
        with pytest.raises(jpeg.JpegDecodeError) as e:
            jpeg.decode_jpeg_host(c.data)
        assert e.value.status == c.status
    good = [c for c in FOREIGN_ACCEPTED if c.name.startswith("s_")][:4]
    order = [good[0], bad[0], good[1], good[2], bad[1], good[3]]
    images, status = _decode([c.data for c in order])
    assert status.tolist() == [c.status for c in order]
    for c, got in zip(order, images):
        if c.status:
            assert not got.any(), c.name                            # untouched: the decoder's buffer starts as zeros
        else:
            _check(c, got)


# ------------------------------------------------------------------------------------------------ ingest: decode='device' against 'pil'
def _write_tree(d):
    """About 40 small files: baseline JPEGs in the three samplings and grayscale, a progressive and a CMYK JPEG, a PNG, and a JPEG cut
    inside its scan (returned apart: it is the one file neither mode can read)."""
    from PIL import Image
    sizes = [(50, 37), (33, 17), (16, 16), (7, 5), (5, 40), (41, 63), (64, 48), (97, 31), (30, 120)]
    paths = []

    def picture(w, h, seed):
        rng = np.random.default_rng(seed)
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(xx * (3 + c) + yy * (5 - c)) % 256 for c in range(3)], -1) + rng.integers(-40, 41, (h, w, 3))
        return Image.fromarray(np.clip(base, 0, 255).astype(np.uint8), "RGB")
    k = 0
    for w, h in sizes:
        for sub in (0, 1, 2, None):
            p = os.path.join(d, "f%02d.jpg" % k)
            kw = [dict(quality=90), dict(quality=40, optimize=True), dict(quality=75, restart_marker_blocks=2), dict(quality=5)][k % 4]
            im = picture(w, h, k)
            im.convert("L").save(p, **kw) if sub is None else im.save(p, subsampling=sub, **kw)
            paths.append(p)
            k += 1
    extra = [("prog.jpg", lambda p: picture(60, 44, 90).save(p, quality=80, progressive=True)),
             ("cmyk.jpg", lambda p: picture(52, 40, 91).convert("CMYK").save(p, quality=80)), ("plain.png", lambda p: picture(45, 33, 92).save(p))]
    for pos, (name, save) in zip((3, 17, 30), extra):
        p = os.path.join(d, name)
        save(p)
        paths.insert(pos, p)
    cut = os.path.join(d, "cut.jpg")
    picture(80, 60, 93).save(cut, quality=85)
    data = open(cut, "rb").read()
    open(cut, "wb").write(data[:len(data) * 2 // 3])
    return paths, cut


def test_files_to_features_device_decode_equals_pil(tmp_path):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    pytest.importorskip("PIL.Image")
    from scd_amd import images
    from scd_amd.clip import weights as W
    from scd_amd.clip.model import CLIP
    paths, cut = _write_tree(str(tmp_path))
    n = len(paths)
    assert n == 39
    targets, mask_lab = np.arange(n) % 3, np.arange(n) < 4
    models = {"clip": CLIP(W.synthetic_clip_state_dict(seed=0, cfg=dict(v_layers=2, t_layers=2))).cuda()}
    want = images.extract_features_from_files(paths, targets, mask_lab, models, batch_size=64, threads=3)["clip"]
    for bs in (4, 64):
        stats = {}
        got = images.extract_features_from_files(paths, targets, mask_lab, models, batch_size=bs, threads=3, decode="device", stats=stats)["clip"]
        assert stats == dict(files=n, device_decoded=36, fallback_parser=3, fallback_status=0), stats
        for k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, bs)
    with_cut = paths[:20] + [cut] + paths[20:]
    t2, m2 = np.arange(n + 1) % 3, np.arange(n + 1) < 4
    errors = {}
    for mode in ("pil", "device"):
        with pytest.raises(OSError, match="cut.jpg") as e:
            images.extract_features_from_files(with_cut, t2, m2, models, batch_size=64, threads=3, decode=mode)
        errors[mode] = str(e.value)
    assert errors["pil"] == errors["device"]
    with pytest.raises(ValueError, match="decode"):
        images.extract_features_from_files(paths, targets, mask_lab, models, decode="hardware")


def test_files_to_features_device_decode_equals_pil_at_photograph_sizes(tmp_path):
    """Six Pillow-written files at 500 x 375, 375 x 500 and 640 x 427, each size in two of the three samplings: every one is decoded
    on the device and the features are those of decode='pil', bit for bit."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    Image = pytest.importorskip("PIL.Image")
    from scd_amd import images
    from scd_amd.clip import weights as W
    from scd_amd.clip.model import CLIP
    paths = []
    for k, ((w, h), sub) in enumerate(zip([(500, 375), (375, 500), (640, 427)] * 2, (0, 1, 2, 2, 0, 1))):
        rng = np.random.default_rng(300 + k)
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(xx * (3 + c) + yy * (5 - c)) % 256 for c in range(3)], -1) + rng.integers(-40, 41, (h, w, 3))
        paths.append(str(tmp_path / ("p%d.jpg" % k)))
        Image.fromarray(np.clip(base, 0, 255).astype(np.uint8), "RGB").save(paths[-1], quality=(85, 60, 92)[k % 3], subsampling=sub,
                                                                           **(dict(restart_marker_blocks=7) if k == 4 else {}))
    n = len(paths)
    targets, mask_lab = np.arange(n) % 3, np.arange(n) < 2
    models = {"clip": CLIP(W.synthetic_clip_state_dict(seed=0, cfg=dict(v_layers=2, t_layers=2))).cuda()}
    want = images.extract_features_from_files(paths, targets, mask_lab, models, batch_size=64, threads=3)["clip"]
    for bs in (2, 64):
        stats = {}
        got = images.extract_features_from_files(paths, targets, mask_lab, models, batch_size=bs, threads=3, decode="device", stats=stats)["clip"]
        assert stats == dict(files=6, device_decoded=6, fallback_parser=0, fallback_status=0), stats
        for k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, bs)


def test_main_unsup_decode_device_writes_the_same_caches(tmp_path, monkeypatch):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    pytest.importorskip("PIL.Image")
    import importlib
    import scd_amd.clip as clip
    from scd_amd.clip import weights as W
    imgdir = tmp_path / "imgs"
    imgdir.mkdir()
    paths, _ = _write_tree(str(imgdir))
    paths = [p for p in paths if not p.endswith("cut.jpg")][:16]
    n = len(paths)
    targets, mask_lab = np.arange(n) % 2, np.arange(n) < 4
    with open(tmp_path / "list.csv", "w") as f:
        f.write("path,target,labelled\n")
        for p, t, m in zip(paths, targets, mask_lab):
            f.write("imgs/%s,%d,%d\n" % (os.path.basename(p), t, int(m)))
    model_root = tmp_path / "models"
    for sub in ("clip", "dino", "data"):
        (model_root / sub).mkdir(parents=True)
    sd = W.synthetic_clip_state_dict(seed=0, cfg=dict(v_layers=2, t_layers=2))
    torch.save({k: (v.half() if v.dim() >= 2 else v) for k, v in sd.items()}, model_root / "clip" / "ViT-B-16.pt")
    torch.save(W.synthetic_dino_state_dict(seed=1, layers=2), model_root / "dino" / "dino_vitbase16_pretrain.pth")
    (model_root / "data" / "wordnet_all_noun.txt").write_text("\n".join("noun_%03d" % i for i in range(40)) + "\n")
    zw = torch.nn.functional.normalize(torch.randn(512, 40, generator=torch.Generator().manual_seed(2)), dim=0)
    monkeypatch.setenv("SCD_ROOT", str(model_root))
    monkeypatch.setenv("SCD_DATA", str(model_root / "data"))
    monkeypatch.setattr(clip, "_tokenizer", None)
    mu = importlib.import_module("main_unsup")
    caches = {}
    for mode in ("pil", "device"):
        root = tmp_path / mode
        (root / "zeroshot_weights").mkdir(parents=True)
        torch.save(zw, root / "zeroshot_weights" / "zeroshot_weights_all_nouns_vit_b_16.pt")
        mu.main(["--root_dir", str(root), "--dataset_name", "tiny", "--feat_model", "dino_vit", "--extract_feat", "true", "--run_cluster",
                 "true", "--cluster", "KM", "--n_cluster", "2", "--topk", "3", "--image_list", str(tmp_path / "list.csv"), "--decode", mode])
        caches[mode] = {f: torch.load(root / "extracted_features" / f, weights_only=False) for f in ("dino_vit_tiny_all.pt", "clip_tiny_all.pt")}
    for f, want in caches["pil"].items():
        got = caches["device"][f]
        assert set(got) == set(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (f, k)
