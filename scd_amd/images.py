"""Image files -> feature caches: the reference's extraction (main_unsup.py:114-147,237,271-311: ImageFolder + CLIP's `preprocess` in
a DataLoader, then the towers) from files on disk, with the preprocessing on the device (docs/design/ingest.md).

Host: PIL decodes (torchvision's pil_loader: Image.open(f).convert('RGB')) in a thread pool, in file order - or, with decode='device',
the host threads only read and parse the files and baseline JPEGs are decoded on the device to the same pixels (scd_amd/jpeg.py).
Device: the decoded
uint8 pixels of a batch go up in one copy on a side stream from pinned, double-buffered staging; scd_image_preprocess resizes, crops
and normalises them bit for bit as Resize(224, BICUBIC) + CenterCrop(224) + ToTensor + Normalize do on the host; every requested
tower encodes the same fp16 batch.  One decode per image feeds all towers; features stay on the device until the end.
"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib, jpeg, ops
from ._lib import check, ptr

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
# torchvision 0.11 datasets/folder.py
IMG_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.ppm', '.bmp', '.pgm', '.tif', '.tiff', '.webp')
_DESC = np.dtype(_lib.IMAGE_DESC_FIELDS)
assert _DESC.itemsize == 40


def default_threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def list_image_folder(root):
    """torchvision's ImageFolder listing (find_classes + make_dataset): sorted class directories, sorted os.walk (links followed), files
    with IMG_EXTENSIONS.  Returns (paths, targets, class_to_idx); class_to_idx is what --class_names takes as JSON."""
    classes = sorted(e.name for e in os.scandir(root) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"Couldn't find any class folder in {root}.")
    class_to_idx = {c: i for i, c in enumerate(classes)}
    paths, targets = [], []
    for c in classes:
        for dirpath, _, fnames in sorted(os.walk(os.path.join(root, c), followlinks=True)):
            for f in sorted(fnames):
                p = os.path.join(dirpath, f)
                if p.lower().endswith(IMG_EXTENSIONS):
                    paths.append(p)
                    targets.append(class_to_idx[c])
    return paths, targets, class_to_idx


def read_image_list(csv_path):
    """--image_list: CSV rows `path,target,labelled` (an optional header row), paths relative to the CSV's directory.  Returns
    (paths, targets int64, mask_lab bool) in file order."""
    import csv
    base = os.path.dirname(os.path.abspath(csv_path))
    paths, targets, lab = [], [], []
    with open(csv_path, newline='') as fh:
        for i, row in enumerate(csv.reader(fh)):
            if not row or (i == 0 and row[0].strip().lower() == 'path'):
                continue
            if len(row) != 3:
                raise ValueError(f"{csv_path}:{i + 1}: expected path,target,labelled, got {row}")
            paths.append(os.path.join(base, row[0].strip()))
            targets.append(int(row[1]))
            v = row[2].strip().lower()
            if v not in ('0', '1', 'true', 'false'):
                raise ValueError(f"{csv_path}:{i + 1}: labelled must be 0/1/true/false, got {row[2]!r}")
            lab.append(v in ('1', 'true'))
    return paths, np.asarray(targets, dtype=np.int64), np.asarray(lab, dtype=bool)


def load_rgb(path):
    """pil_loader: uint8 [H, W, 3].  A file PIL cannot read raises OSError naming the path."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("image ingest decodes with Pillow (PIL), which is not installed") from e
    try:
        with open(path, 'rb') as f:
            img = Image.open(f)
            return np.asarray(img.convert('RGB'))
    except Exception as e:
        raise OSError(f"cannot read image {path}: {type(e).__name__}: {e}") from e


def read_for_device(path):
    """decode='device', one file on a host thread: ('jpeg', bytes, info) for a file the device decoder takes, else ('rgb', pixels of
    load_rgb, None).  A file that cannot be read at all fails in load_rgb, with load_rgb's error."""
    try:
        with open(path, 'rb') as f:
            data = f.read()
        info = jpeg.parse(data)
    except OSError:
        return 'rgb', load_rgb(path), None
    # a frame above Pillow's MAX_IMAGE_PIXELS (a header may claim 65,535 x 65,535 whatever the file holds) meets Pillow's policy as
    # with decode='pil': its warning, or its DecompressionBombError as load_rgb's OSError
    if info["reason"] != 0 or jpeg.over_pillow_limit(info):
        return 'rgb', load_rgb(path), None
    return 'jpeg', data, info


def normalize_lut(device=None):
    """[3, 256] fp16: ToTensor + Normalize(CLIP mean / std) of every uint8 value, with torch's own ops on the host (ToTensor:
    .to(float32).div(255); Normalize: .sub_(mean).div_(std)), then .half()."""
    v = torch.arange(256, dtype=torch.uint8).view(1, 1, 256).expand(3, 1, 256).contiguous()
    x = v.to(dtype=torch.float32).div(255)
    mean = torch.as_tensor(CLIP_MEAN, dtype=torch.float32).view(-1, 1, 1)
    std = torch.as_tensor(CLIP_STD, dtype=torch.float32).view(-1, 1, 1)
    lut = x.sub_(mean).div_(std).half().view(3, 256)
    return lut if device is None else lut.to(device)


def geometry(w, h, size=224, crop=224):
    """(resized w, resized h, crop left, crop top, first source row read, source rows read) - scd_image_geometry."""
    g = np.zeros(6, dtype=np.int32)
    check(_lib.load().scd_image_geometry(int(w), int(h), int(size), int(crop), ptr(g)))
    return tuple(int(x) for x in g)


def plan_axis(in_size, out_size, off=0, n=None):
    """Pillow's int32 taps of outputs off .. off + n - 1 of a bicubic in_size -> out_size resize: list of (first, taps int32)."""
    n = out_size - off if n is None else n
    L = _lib.load()
    nt = C.c_int64(0)
    check(L.scd_image_plan_axis(int(in_size), int(out_size), int(off), int(n), None, None, None, 0, C.byref(nt)))
    first, ntaps = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    taps = np.zeros(max(nt.value, 1), dtype=np.int32)
    check(L.scd_image_plan_axis(int(in_size), int(out_size), int(off), int(n), ptr(first), ptr(ntaps), ptr(taps), nt.value, None))
    ends = np.cumsum(ntaps)
    return [(int(first[i]), taps[ends[i] - ntaps[i]:ends[i]]) for i in range(n)]


def batch_plan(sizes, size=224, crop=224):
    """sizes [(w, h), ...] -> (descs (scd_image_desc records), plan int32, pixel_bytes, ws_bytes) - scd_image_batch_plan."""
    L = _lib.load()
    wh = np.ascontiguousarray(np.asarray(sizes, dtype=np.int32).reshape(-1, 2))
    b = wh.shape[0]
    n, pb, wb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    check(L.scd_image_batch_plan(ptr(wh), b, int(size), int(crop), None, None, 0, C.byref(n), C.byref(pb), C.byref(wb)))
    descs = np.zeros(b, dtype=_DESC)
    plan = np.zeros(n.value, dtype=np.int32)
    check(L.scd_image_batch_plan(ptr(wh), b, int(size), int(crop), ptr(descs), ptr(plan), n.value, C.byref(n), C.byref(pb), C.byref(wb)))
    return descs, plan, pb.value, wb.value


def _a256(n):
    return (n + 255) // 256 * 256


class _Layout:
    """One batch's staging bytes: [descs | plan | pixels], each section 256-byte aligned."""

    def __init__(self, descs, plan, pixel_bytes):
        self.b = len(descs)
        self.plan_off = _a256(descs.nbytes)
        self.pix_off = self.plan_off + _a256(plan.nbytes)
        self.plan_len = plan.size
        self.pixel_bytes = pixel_bytes
        self.total = self.pix_off + pixel_bytes


def _pack(buf, lay, descs, plan, images):
    """Write one batch into the uint8 numpy view `buf` (pinned host memory)."""
    buf[:descs.nbytes] = descs.view(np.uint8)
    buf[lay.plan_off:lay.plan_off + plan.nbytes] = plan.view(np.uint8)
    o = lay.pix_off
    for im in images:
        nb = im.size
        buf[o:o + nb] = np.ascontiguousarray(im).reshape(-1)
        o += nb


class Preprocessor:
    """scd_image_preprocess on one device: CLIP's `preprocess` of decoded uint8 RGB images -> fp16 [B, 3, crop, crop]."""

    def __init__(self, device=None, size=224, crop=224):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.size, self.crop = size, crop
        self.lut = normalize_lut(self.device)

    def run(self, staged, lay, ws_bytes, out=None):
        """staged: the device copy of a batch's staging bytes (_Layout); returns fp16 [B, 3, crop, crop] on the current stream."""
        ops._need_cuda(staged)
        b, c = lay.b, self.crop
        if out is None:
            out = torch.empty((b, 3, c, c), dtype=torch.float16, device=self.device)
        assert out.dtype == torch.float16 and out.shape == (b, 3, c, c) and out.is_contiguous()
        ws = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device=self.device)
        base = staged.data_ptr()
        check(_lib.load().scd_image_preprocess(ops.handle(), C.c_void_p(base + lay.pix_off), lay.pixel_bytes, C.c_void_p(base),
                                               C.c_void_p(base + lay.plan_off), lay.plan_len, b, c, ptr(self.lut), ptr(out), ptr(ws),
                                               ws.numel(), ops.stream_ptr()))
        return out

    def __call__(self, images):
        """Decoded uint8 [H, W, 3] arrays -> fp16 [B, 3, crop, crop] (one synchronous-free upload; for tests and small batches)."""
        descs, plan, pb, wb = batch_plan([(im.shape[1], im.shape[0]) for im in images], self.size, self.crop)
        lay = _Layout(descs, plan, pb)
        host = np.zeros(lay.total, dtype=np.uint8)
        _pack(host, lay, descs, plan, images)
        staged = torch.from_numpy(host).to(self.device)
        return self.run(staged, lay, wb)


def _encode(model, feat_model, pixels):
    """naming.extract_feature's three tower calls (main_unsup.py:127-130)."""
    if feat_model == 'clip':
        return model.visual.enc.encode_image(pixels, normalize=True)
    if hasattr(model, "features"):
        return model.features(pixels, normalize=True)
    return ops.l2norm_rows(model(pixels).float())


def extract_features_from_files(paths, targets, mask_lab, models, train_classes=None, batch_size=256, threads=None, device=None,
                                size=224, crop=224, decode='pil', stats=None):
    """Image files -> {feat_model name: naming.extract_feature dict (all_feats, mask_lab, mask_cls, targets)} for every entry of
    `models` ({'clip': clip model, 'dino_vit': DinoViT, ...}), each bit-equal to naming.extract_feature on the reference-preprocessed
    images.  train_classes (the mask_cls classes) default to the targets of the labelled rows, as main_unsup.load_or_extract does.

    Decoding runs in `threads` host threads (default min(16, usable CPUs)) two batches ahead of the device; the result order is
    the file order whatever the thread timing.

    decode='device': the host threads read the files and parse their headers; a baseline JPEG inside the device decoder's scope goes up
    as bytes and is decoded into the batch's pixel section by scd_jpeg_decode, to the pixels Pillow gives.  Every other file, every
    file whose frame is above Pillow's MAX_IMAGE_PIXELS, and
    every file whose device status comes back non-zero, is decoded by load_rgb and uploaded into its slot before the batch is
    preprocessed - a file Pillow cannot read raises load_rgb's OSError, as with decode='pil'.  stats (a dict, optional) receives
    'files', 'device_decoded', 'fallback_parser' and 'fallback_status' counts."""
    if decode not in ('pil', 'device'):
        raise ValueError(f"extract_features_from_files: decode must be 'pil' or 'device', got {decode!r}")
    paths = [os.fspath(p) for p in paths]
    n = len(paths)
    if n == 0:
        raise ValueError("extract_features_from_files: no image files")
    targets = np.asarray(targets).astype(np.float64)
    mask_lab = np.asarray(mask_lab).astype(bool)
    if targets.shape != (n,) or mask_lab.shape != (n,):
        raise ValueError(f"extract_features_from_files: {n} paths, {targets.shape} targets, {mask_lab.shape} mask_lab")
    if train_classes is None:
        train_classes = sorted(set(targets[mask_lab].tolist()))
    train_classes = set(int(c) for c in train_classes)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    pre = Preprocessor(dev, size, crop)
    threads = default_threads() if threads is None else max(1, int(threads))
    starts = list(range(0, n, batch_size))
    cur = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(dev)
    pinned = [None, None]
    status_pin = [None, None]                                # pinned int32: the device decoder's status of the slot's batch
    staged = [None, None]
    copied = [torch.cuda.Event(), torch.cuda.Event()]        # H2D (and device decode) of the slot's batch done (side stream)
    consumed = [torch.cuda.Event(), torch.cuda.Event()]      # preprocess of the slot's batch done (compute stream)
    feats = {name: [] for name in models}
    pool = ThreadPoolExecutor(max_workers=threads, thread_name_prefix="scd-decode")
    pending = {}

    def submit(i):
        if i < len(starts) and i not in pending:
            pending[i] = [pool.submit(load_rgb if decode == 'pil' else read_for_device, p) for p in paths[starts[i]:starts[i] + batch_size]]

    counts = dict(files=n, device_decoded=0, fallback_parser=0, fallback_status=0)

    def stage(i):
        """Batch i up to the device: wait for its host threads, plan, pack, upload on the side stream and, with decode='device',
        queue the JPEG decode and the status read-back behind the upload.  Returns what finish() needs."""
        images = [f.result() for f in pending.pop(i)]             # file order; raises the first unreadable file's error
        jidx, jlay, items, status_host = [], None, None, None
        if decode == 'device':
            items, images = images, None
            jidx = [k for k, it in enumerate(items) if it[0] == 'jpeg']
            counts['fallback_parser'] += len(items) - len(jidx)
            wh = [(int(it[2]["w"]), int(it[2]["h"])) if it[0] == 'jpeg' else (it[1].shape[1], it[1].shape[0]) for it in items]
        else:
            wh = [(im.shape[1], im.shape[0]) for im in images]
        descs, plan, pb, wb = batch_plan(wh, size, crop)
        lay = _Layout(descs, plan, pb)
        total, joff = lay.total, _a256(lay.total)
        if jidx:
            jdatas = [items[k][1] for k in jidx]
            jdescs, jtables, jdb, jwb = jpeg.batch_plan(jdatas, np.array([items[k][2] for k in jidx], dtype=jpeg.INFO),
                                                        [int(descs["src_off"][k]) for k in jidx])
            jlay = jpeg.JpegLayout(jdescs, jtables, jdb, jwb)
            total = joff + jlay.total
        s = i % 2
        copied[s].synchronize()                                    # the slot's previous upload has left the pinned buffer
        if pinned[s] is None or pinned[s].numel() < total:
            pinned[s] = torch.empty(int(total * 1.25) + 4096, dtype=torch.uint8, pin_memory=True)
        if jidx:
            # [descs | plan | pixels | jpeg descs | tables | files]: the pixel section is filled on the device, except for the
            # slots of the files Pillow decoded; only the written ranges are copied up
            buf = pinned[s].numpy()
            buf[:descs.nbytes] = descs.view(np.uint8)
            buf[lay.plan_off:lay.plan_off + plan.nbytes] = plan.view(np.uint8)
            ranges = [(0, lay.pix_off), (joff, total)]
            for k, it in enumerate(items):
                if it[0] == 'rgb':
                    o = lay.pix_off + int(descs["src_off"][k])
                    buf[o:o + it[1].size] = np.ascontiguousarray(it[1]).reshape(-1)
                    ranges.append((o, o + it[1].size))
            jpeg.pack(buf[joff:], jlay, jdescs, jtables, jdatas)
        else:
            _pack(pinned[s].numpy(), lay, descs, plan, images if decode == 'pil' else [it[1] for it in items])
            ranges = [(0, lay.total)]
        del images, items
        if staged[s] is None or staged[s].numel() < total:
            # allocated from the side stream's pool (the stream that writes it): a block freed on the compute stream - a
            # previous batch's pixels, still read by towers queued there - cannot come back here.  The compute stream reads the
            # buffer, so it is recorded there; and the side stream first catches up with everything queued so far.
            staged[s] = None
            with torch.cuda.stream(side):
                staged[s] = torch.empty(pinned[s].numel(), dtype=torch.uint8, device=dev)
            staged[s].record_stream(cur)
            side.wait_stream(cur)
        side.wait_event(consumed[s])                               # the slot's previous batch has been preprocessed
        with torch.cuda.stream(side):
            for a, b in ranges:
                staged[s][a:b].copy_(pinned[s][a:b], non_blocking=True)
            if jidx:
                # The decode follows the upload on the side stream, beside the towers of earlier batches on the compute stream.
                # Its status goes to pinned memory behind it, so that finish() waits for this batch's decode alone.
                status_dev = jpeg.run(staged[s][joff:total], jlay, staged[s].data_ptr() + lay.pix_off, pb)
                if status_pin[s] is None or status_pin[s].numel() < len(jidx):
                    status_pin[s] = torch.empty(max(len(jidx), batch_size), dtype=torch.int32, pin_memory=True)
                status_host = status_pin[s][:len(jidx)]
                status_host.copy_(status_dev, non_blocking=True)
        copied[s].record(side)                                     # upload, and with decode='device' the decoded pixels, complete
        return dict(i=i, s=s, lay=lay, wb=wb, descs=descs, wh=wh, jidx=jidx, status=status_host)

    def finish(c):
        """Batch c['i'] from the staged bytes to features: the fallbacks of the device decode, preprocessing, the towers."""
        i, s, lay, descs = c['i'], c['s'], c['lay'], c['descs']
        if c['jidx']:
            copied[s].synchronize()                                # this batch's decode and status read-back, not the towers
            status = c['status'].numpy().copy()
            bad = np.nonzero(status)[0]
            if len(bad):
                with torch.cuda.stream(side):
                    for j in bad:                                  # the decoder could not follow the stream: Pillow's file
                        k = c['jidx'][int(j)]
                        im = load_rgb(paths[starts[i] + k])
                        if (im.shape[1], im.shape[0]) != c['wh'][k]:
                            raise OSError(f"cannot read image {paths[starts[i] + k]}: Pillow decodes {im.shape[1]} x {im.shape[0]}, "
                                          f"the frame header says {c['wh'][k][0]} x {c['wh'][k][1]}")
                        o = lay.pix_off + int(descs["src_off"][k])
                        staged[s][o:o + im.size].copy_(torch.from_numpy(np.ascontiguousarray(im).reshape(-1)))
                side_done = torch.cuda.Event()
                side_done.record(side)
                cur.wait_event(side_done)
            counts['fallback_status'] += len(bad)
            counts['device_decoded'] += len(status) - len(bad)
        cur.wait_event(copied[s])
        pixels = pre.run(staged[s], lay, c['wb'])
        consumed[s].record(cur)
        for name, model in models.items():
            feats[name].append(_encode(model, name, pixels))

    try:
        submit(0)
        submit(1)
        if decode == 'pil':
            for i in range(len(starts)):
                submit(i + 2)
                finish(stage(i))
        else:
            # One batch ahead: batch i + 1 is read, packed, uploaded and its decode queued before the host waits for the status of
            # batch i, so the decodes run back to back on the side stream while the host packs and the towers run.  (Reading and
            # parsing is cheap; with decode='pil' the same order would make the towers wait for the next batch's host decode.)
            submit(2)
            nxt = stage(0)
            for i in range(len(starts)):
                submit(i + 3)
                this, nxt = nxt, (stage(i + 1) if i + 1 < len(starts) else None)
                finish(this)
    finally:
        for fs in pending.values():
            for f in fs:
                f.cancel()
        pool.shutdown(wait=True)
    if stats is not None:
        stats.update(counts)
    mask_cls = np.array([int(x) in train_classes for x in targets], dtype=bool)
    return {name: dict(all_feats=torch.cat(f).cpu().numpy(), mask_lab=mask_lab.copy(), mask_cls=mask_cls.copy(), targets=targets.copy())
            for name, f in feats.items()}
