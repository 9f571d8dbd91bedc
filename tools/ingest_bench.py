#!/usr/bin/env python
"""Image-file ingest, stage by stage (docs/design/ingest.md).
`python tools/ingest_bench.py [--images 2048] [--decode {pil,device}] [--out FILE.json]`

Writes ImageNet-like JPEGs (500x375 and 375x500, quality 90) to a temporary directory and reports
  decode      PIL decode + convert('RGB') only, images/s at 1, 4, 8 and 16 threads;
  kernel      scd_image_preprocess, us per batch of 256 (HIP events, pixels already on the device);
  towers      CLIP ViT-B/16 + DINO ViT-B/16 (synthetic weights, full depth) on a resident fp16 batch, images/s;
  ingest      files -> CLIP + DINO features through scd_amd.images.extract_features_from_files, images/s;
  host route  the same job the way --images_pt is fed today: per-image PIL Resize + CenterCrop + ToTensor + Normalize on the host
              (same thread count), fp32 batches copied to the device, naming.extract_feature per tower;
and which stage limits the end-to-end rate.  With --decode device the same run adds, under "jpeg",
  ingest      files -> CLIP + DINO features with decode='device', beside the decode='pil' line above, and whether the features are equal;
  decode      scd_jpeg_decode of a staged batch of 256 alone, ms (HIP events, median of 10 after 2 warm-ups);
  host side   read + parse only (what the host threads do with decode='device'), images/s at 1, 4, 8 and 16 threads;
  fallback    the share of files Pillow decoded after all.
One JSON document on stdout (and in --out)."""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_jpegs(d, n, threads):
    from PIL import Image

    def one(i):
        rng = np.random.default_rng(i)
        w, h = (500, 375) if i % 4 else (375, 500)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        ph = rng.uniform(0, 6.3, 3)
        base = np.stack([127 + 100 * np.sin(xx / (17 + 5 * c) + yy / (23 + 3 * c) + ph[c]) for c in range(3)], -1)
        img = np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)      # photo-like: smooth structure plus grain
        p = os.path.join(d, "img_%05d.jpg" % i)
        Image.fromarray(img, "RGB").save(p, quality=90)
        return p
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(one, range(n)))


def host_preprocess(path):
    """The reference's per-image host path (pil_loader, Resize(224, BICUBIC), CenterCrop(224), ToTensor, Normalize) on Pillow + torch."""
    from PIL import Image
    from scd_amd.images import CLIP_MEAN, CLIP_STD
    with open(path, "rb") as f:
        im = Image.open(f).convert("RGB")
    w, h = im.size
    s, l = (w, h) if w <= h else (h, w)
    if s != 224:
        ns, nl = 224, int(224 * l / s)
        im = im.resize((ns, nl) if w <= h else (nl, ns), Image.BICUBIC)
    w, h = im.size
    top, left = int(round((h - 224) / 2.0)), int(round((w - 224) / 2.0))
    im = im.crop((left, top, left + 224, top + 224))
    t = torch.from_numpy(np.array(im, dtype=np.uint8, copy=True)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return t.sub_(torch.as_tensor(CLIP_MEAN).view(-1, 1, 1)).div_(torch.as_tensor(CLIP_STD).view(-1, 1, 1))


def jpeg_lines(paths, targets, mask_lab, models, got_pil, pil_rate, dev):
    """The device JPEG decoder's lines of the document (same process, same files as the decode='pil' ingest line)."""
    from scd_amd import images, jpeg
    n = len(paths)
    out = dict(ingest_pil_images_per_s=pil_rate)
    images.extract_features_from_files(paths[:512], targets[:512], mask_lab[:512], models, decode="device")          # warm-up
    torch.cuda.synchronize()
    stats = {}
    t = time.perf_counter()
    got = images.extract_features_from_files(paths, targets, mask_lab, models, decode="device", stats=stats)
    out["ingest_device_images_per_s"] = round(n / (time.perf_counter() - t), 1)
    out["same_features_as_pil"] = all(np.array_equal(got[k]["all_feats"], got_pil[k]["all_feats"]) for k in models)
    out["files"] = stats
    out["fallback_share"] = round((stats["fallback_parser"] + stats["fallback_status"]) / n, 5)

    # host side alone: read + parse
    out["read_parse_images_per_s"] = {}
    for th in (1, 4, 8, 16):
        m = min(n, 512 * th)
        with ThreadPoolExecutor(th) as ex:
            list(ex.map(images.read_for_device, paths[:th]))
            t = time.perf_counter()
            list(ex.map(images.read_for_device, paths[:m]))
            out["read_parse_images_per_s"][str(th)] = round(m / (time.perf_counter() - t), 1)

    # the decoder alone on staged batches of 256 and of 1,024: one wave per image, so a larger batch fills the same time
    for nb in (256, 1024):
        if nb > n:
            continue
        items = [images.read_for_device(p) for p in paths[:nb]]
        datas, infos = [it[1] for it in items], np.array([it[2] for it in items], dtype=jpeg.INFO)
        sizes = [3 * int(i["w"]) * int(i["h"]) for i in infos]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        descs, tables, db, wb = jpeg.batch_plan(datas, infos, offs[:-1])
        lay = jpeg.JpegLayout(descs, tables, db, wb)
        host = np.zeros(lay.total, dtype=np.uint8)
        jpeg.pack(host, lay, descs, tables, datas)
        staged = torch.from_numpy(host).to(dev)
        pixels = torch.zeros(int(offs[-1]), dtype=torch.uint8, device=dev)
        status = torch.zeros(nb, dtype=torch.int32, device=dev)
        times = []
        for rep in range(12):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            jpeg.run(staged, lay, pixels, int(offs[-1]), status=status)
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:
                times.append(e0.elapsed_time(e1))
        out["decode_ms_per_%d_median" % nb] = round(float(np.median(times)), 3)
        out["decode_ms_per_%d_min_max" % nb] = [round(min(times), 3), round(max(times), 3)]
        out["decode_images_per_s_at_%d" % nb] = round(nb / float(np.median(times)) * 1000, 1)
        out["decode_status_nonzero_at_%d" % nb] = int(status.count_nonzero().item())
        out["bytes_per_%d" % nb] = dict(compressed=int(sum(len(d) for d in datas)), tables=int(tables.nbytes), planes=int(wb), rgb_out=int(offs[-1]))
        del staged, pixels

    # the same ingest with batches of 1,024, both ways
    for mode in ("pil", "device"):
        torch.cuda.synchronize()
        t = time.perf_counter()
        images.extract_features_from_files(paths, targets, mask_lab, models, decode=mode, batch_size=1024)
        out["ingest_%s_images_per_s_batch_1024" % mode] = round(n / (time.perf_counter() - t), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--decode", default="pil", choices=["pil", "device"], help="device: also measure the device JPEG decoder")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.set_num_threads(1)                       # host-route threads are the pool's; no intra-op fan-out on top
    from bench import PowerSampler
    from scd_amd import images, naming
    from scd_amd.clip import weights as W
    from scd_amd.clip.model import CLIP, DinoViT
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cpus = len(os.sched_getaffinity(0))
    res = dict(tool="tools/ingest_bench.py", images=a.images, usable_cpus=cpus, gpu=torch.cuda.get_device_name(0),
               default_threads=images.default_threads())
    with tempfile.TemporaryDirectory() as d:
        t = time.perf_counter()
        paths = write_jpegs(d, a.images, images.default_threads())
        res["write_s"] = round(time.perf_counter() - t, 2)
        res["jpeg_bytes_mean"] = int(np.mean([os.path.getsize(p) for p in paths]))
        targets = np.arange(a.images) % 100
        mask_lab = np.arange(a.images) < a.images // 2

        # decode only
        res["decode_images_per_s"] = {}
        for th in (1, 4, 8, 16):
            n = min(a.images, 256 * th)
            with ThreadPoolExecutor(th) as ex:
                list(ex.map(images.load_rgb, paths[:th]))
                t = time.perf_counter()
                list(ex.map(images.load_rgb, paths[:n]))
                res["decode_images_per_s"][str(th)] = round(n / (time.perf_counter() - t), 1)

        # the preprocessing kernel on a staged batch of 256
        pre = images.Preprocessor(dev)
        with ThreadPoolExecutor(images.default_threads()) as ex:
            batch = list(ex.map(images.load_rgb, paths[:256]))
        descs, plan, pb, wb = images.batch_plan([(im.shape[1], im.shape[0]) for im in batch])
        lay = images._Layout(descs, plan, pb)
        host = np.zeros(lay.total, dtype=np.uint8)
        images._pack(host, lay, descs, plan, batch)
        staged = torch.from_numpy(host).to(dev)
        out = pre.run(staged, lay, wb)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 50
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(reps):
            pre.run(staged, lay, wb, out=out)
        ev1.record()
        torch.cuda.synchronize()
        kus = ev0.elapsed_time(ev1) * 1000 / reps
        res["kernel_us_per_256"] = round(kus, 1)
        res["kernel_bytes_per_256"] = dict(pixels_in=pb, band=wb, out=out.numel() * 2)
        res["kernel_gb_per_s_in_plus_out"] = round((pb + out.numel() * 2) / (kus * 1e-6) / 1e9, 1)

        # the two towers on a resident fp16 batch
        clip_model = CLIP(W.synthetic_clip_state_dict(seed=0)).cuda()
        dino = DinoViT(W.synthetic_dino_state_dict(seed=1)).cuda()
        models = {"dino_vit": dino, "clip": clip_model}
        for _ in range(2):
            clip_model.visual.enc.encode_image(out, normalize=True)
            dino.features(out, normalize=True)
        torch.cuda.synchronize()
        ev0.record()
        for _ in range(10):
            clip_model.visual.enc.encode_image(out, normalize=True)
            dino.features(out, normalize=True)
        ev1.record()
        torch.cuda.synchronize()
        tower_ms = ev0.elapsed_time(ev1) / 10
        res["towers_ms_per_256"] = round(tower_ms, 2)
        res["towers_images_per_s"] = round(256 / tower_ms * 1000, 1)
        res["kernel_share_of_towers"] = round(kus / 1000 / tower_ms, 5)

        # files -> features: the new path
        images.extract_features_from_files(paths[:512], targets[:512], mask_lab[:512], models)          # warm-up
        torch.cuda.synchronize()
        ps = PowerSampler(0)
        ps.start()
        t = time.perf_counter()
        got = images.extract_features_from_files(paths, targets, mask_lab, models)
        ingest_s = time.perf_counter() - t
        res["power"] = ps.stop()
        res["ingest_images_per_s"] = round(a.images / ingest_s, 1)

        if a.decode == "device":
            res["jpeg"] = jpeg_lines(paths, targets, mask_lab, models, got, res["ingest_images_per_s"], dev)

        # today's route: host preprocessing, fp32 H2D, naming.extract_feature per tower
        t = time.perf_counter()
        with ThreadPoolExecutor(images.default_threads()) as ex:
            imgs = torch.stack(list(ex.map(host_preprocess, paths)))
        host_pre_s = time.perf_counter() - t
        ref = {}
        for name, m in models.items():
            args = argparse.Namespace(feat_model=name, train_classes=sorted(set(targets[mask_lab].tolist())))

            def loader():
                for s in range(0, a.images, 256):
                    yield imgs[s:s + 256], targets[s:s + 256], None, mask_lab[s:s + 256]
            ref[name] = naming.extract_feature(m, loader(), args)
        host_s = time.perf_counter() - t
        res["host_route_images_per_s"] = round(a.images / host_s, 1)
        res["host_route_preprocess_images_per_s"] = round(a.images / host_pre_s, 1)
        res["same_features_as_host_route"] = all(np.array_equal(got[k]["all_feats"], ref[k]["all_feats"]) for k in models)

    th = str(images.default_threads()) if str(images.default_threads()) in res["decode_images_per_s"] else "16"
    stages = {"decode (%s threads)" % th: res["decode_images_per_s"][th], "preprocess kernel": 256 / (kus * 1e-6),
              "CLIP + DINO towers": res["towers_images_per_s"]}
    res["limiting_stage"] = min(stages, key=stages.get)
    res["stage_images_per_s"] = {k: round(v, 1) for k, v in stages.items()}
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
