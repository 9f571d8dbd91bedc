"""Baseline JPEG decoding bit-equal to Pillow's Image.open(f).convert('RGB') (scd_amd/csrc/jpeg.h, jpeg.hip; docs/design/ingest.md):
the host parser, the CPU decoder for one file, and the device decoder for a batch of byte strings.

A file outside the device decoder's scope (progressive, CMYK, ...) has jpeg_info(data)['reason'] != 0; a stream the entropy decoder
cannot follow, or one that trips the range guard, ends in a non-zero per-image status.  Both kinds are Pillow's to decode
(images.load_rgb): there is no other decoder behind this one."""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, ptr

INFO = np.dtype(_lib.JPEG_INFO_FIELDS)
DESC = np.dtype(_lib.JPEG_DESC_FIELDS)
assert INFO.itemsize == 96 and DESC.itemsize == 104

REASONS = {0: "ok", 1: "not_jpeg", 2: "truncated_header", 3: "bad_marker", 4: "progressive", 5: "arithmetic", 6: "unsupported_sof",
           7: "precision", 8: "components", 9: "sampling", 10: "colourspace", 11: "multiscan", 12: "missing_table", 13: "bad_table",
           14: "chroma_width", 15: "dnl"}
TOO_LARGE = 16      # not a parser reason: the frame is above Pillow's MAX_IMAGE_PIXELS, so Pillow decides (a Python-side policy)
REASONS[TOO_LARGE] = "above_pillow_pixel_limit"
STATUS = {0: "ok", 1: "undefined_code", 2: "index_past_63", 3: "past_end", 4: "marker_in_scan", 5: "range_guard", 6: "descriptor"}


class JpegUnsupported(ValueError):
    """The parser's verdict: the file is outside the device decoder's scope (.reason: SCD_JPEG_*)."""

    def __init__(self, reason):
        super().__init__("JPEG not device-decodable: %s (reason %d)" % (REASONS.get(reason, "?"), reason))
        self.reason = reason


class JpegDecodeError(ValueError):
    """The decoder's per-image status was not 0 (.status: SCD_JPEG_E*)."""

    def __init__(self, status):
        super().__init__("JPEG stream rejected: %s (status %d)" % (STATUS.get(status, "?"), status))
        self.status = status


def _buf(data):
    """bytes-like -> (uint8 numpy view, length)."""
    a = np.frombuffer(data, dtype=np.uint8)
    return (a, a.size) if a.size else (np.zeros(1, dtype=np.uint8), 0)       # an empty file still gets a verdict (not_jpeg)


def parse(data, restarts=False):
    """scd_jpeg_parse: the scd_jpeg_info record of one file (and the file offsets of its RSTn markers)."""
    a, n = _buf(data)
    info = np.zeros(1, dtype=INFO)
    L = _lib.load()
    check(L.scd_jpeg_parse(ptr(a), n, ptr(info), None, 0))
    if not restarts:
        return info[0]
    rst = np.zeros(max(int(info[0]["n_restarts"]), 1), dtype=np.int32)
    check(L.scd_jpeg_parse(ptr(a), n, ptr(info), ptr(rst), rst.size))
    return info[0], rst[:int(info[0]["n_restarts"])]


def jpeg_info(data):
    """The parser's view of a JPEG file as a dict: reason (0 = device-decodable) and its name, w, h, ncomp, hs, vs (luma sampling),
    restart_interval, n_restarts, scan_off, scan_end, has_eoi."""
    i = parse(data)
    out = {k: int(i[k]) for k in ("reason", "w", "h", "ncomp", "hs", "vs", "restart_interval", "n_restarts", "scan_off", "scan_end", "has_eoi")}
    out["reason_name"] = REASONS.get(out["reason"], "?")
    return out


PIL_MAX_IMAGE_PIXELS = 89478485     # Pillow's default Image.MAX_IMAGE_PIXELS


def max_image_pixels():
    """Pillow's size policy, which a file decoded here never meets otherwise: Image.open warns above Image.MAX_IMAGE_PIXELS and raises
    DecompressionBombError above twice that.  Returns the installed Pillow's current value (None: no limit), or its default without
    Pillow."""
    try:
        from PIL import Image
    except ImportError:
        return PIL_MAX_IMAGE_PIXELS
    return Image.MAX_IMAGE_PIXELS


def over_pillow_limit(info):
    """Would Pillow warn about or refuse an image of this frame size?  Such a file is Pillow's to judge (images.read_for_device)."""
    lim = max_image_pixels()
    return lim is not None and int(info["w"]) * int(info["h"]) > lim


def decode_jpeg_host(data):
    """One file on the CPU through the functions the kernels run -> uint8 [H, W, 3].  JpegUnsupported / JpegDecodeError otherwise."""
    a, n = _buf(data)
    i = parse(data)
    if i["reason"] != 0:
        raise JpegUnsupported(int(i["reason"]))
    if over_pillow_limit(i):
        raise JpegUnsupported(TOO_LARGE)
    out = np.zeros((int(i["h"]), int(i["w"]), 3), dtype=np.uint8)
    st = C.c_int32(0)
    check(_lib.load().scd_jpeg_decode_host(ptr(a), n, ptr(out), out.size, C.byref(st)))
    if st.value != 0:
        raise JpegDecodeError(st.value)
    return out


def _a16(n):
    return (n + 15) // 16 * 16


def batch_plan(datas, infos, out_offs):
    """scd_jpeg_batch_plan -> (descs, tables uint8, data_bytes, ws_bytes).  datas: bytes-like per file; infos: INFO records (reason 0);
    out_offs: byte offset of every image's RGB in the pixel section."""
    L = _lib.load()
    n = len(datas)
    views = [np.frombuffer(d, dtype=np.uint8) for d in datas]
    files = (C.c_void_p * n)(*[v.ctypes.data for v in views])
    infos = np.ascontiguousarray(np.asarray(infos, dtype=INFO))
    offs = np.ascontiguousarray(np.asarray(out_offs, dtype=np.int64))
    tb, db, wb = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    check(L.scd_jpeg_batch_plan(files, ptr(infos), ptr(offs), n, None, None, 0, C.byref(tb), C.byref(db), C.byref(wb)))
    descs = np.zeros(n, dtype=DESC)
    tables = np.zeros(max(tb.value, 16), dtype=np.uint8)
    check(L.scd_jpeg_batch_plan(files, ptr(infos), ptr(offs), n, ptr(descs), ptr(tables), tables.size, C.byref(tb), C.byref(db), C.byref(wb)))
    return descs, tables[:max(tb.value, 16)], db.value, wb.value


class JpegLayout:
    """One batch's compressed section: [descs | tables | data], each part 256-byte aligned (so 16-byte aligned on the device)."""

    def __init__(self, descs, tables, data_bytes, ws_bytes):
        self.n = len(descs)
        self.tab_off = (descs.nbytes + 255) // 256 * 256
        self.data_off = self.tab_off + (tables.nbytes + 255) // 256 * 256
        self.tables_bytes = tables.nbytes
        self.data_bytes = data_bytes
        self.ws_bytes = ws_bytes
        self.total = self.data_off + (data_bytes + 255) // 256 * 256


def pack(buf, lay, descs, tables, datas):
    """Write one batch's compressed section into the uint8 numpy view `buf`."""
    buf[:descs.nbytes] = descs.view(np.uint8).reshape(-1)
    buf[lay.tab_off:lay.tab_off + tables.nbytes] = tables
    for d, data in zip(descs, datas):
        o = lay.data_off + int(d["data_off"])
        buf[o:o + int(d["data_len"])] = np.frombuffer(data, dtype=np.uint8)


def run(staged, lay, pixels, pixel_bytes, status=None):
    """scd_jpeg_decode on the current stream.  staged: device copy of a JpegLayout section; pixels: device uint8 tensor (or a raw
    pointer) of the pixel section.  Returns the device int32 status tensor."""
    ops._need_cuda(staged)
    dev = staged.device
    if status is None:
        status = torch.empty(lay.n, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lay.ws_bytes), 16), dtype=torch.uint8, device=dev)
    base = staged.data_ptr()
    pix = pixels.data_ptr() if hasattr(pixels, "data_ptr") else int(pixels)
    check(_lib.load().scd_jpeg_decode(ops.handle(), C.c_void_p(base + lay.data_off), lay.data_bytes, C.c_void_p(base),
                                      C.c_void_p(base + lay.tab_off), lay.tables_bytes, lay.n, C.c_void_p(pix), int(pixel_bytes),
                                      ptr(status), ptr(ws), ws.numel(), ops.stream_ptr()))
    return status


class JpegDecoder:
    """scd_jpeg_decode on one device: a batch of JPEG byte strings -> uint8 RGB on the device.

    decode(datas) -> (images, status): images[i] is a device uint8 [H, W, 3] view of the batch's pixel buffer, status a numpy int32
    array; an image whose status is not 0 was not written (its pixels are zero).  A file the parser rejects raises JpegUnsupported:
    sort those out with jpeg_info first."""

    def __init__(self, device=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)

    def decode(self, datas):
        datas = list(datas)
        if not datas:
            return [], np.zeros(0, dtype=np.int32)
        infos = np.zeros(len(datas), dtype=INFO)
        for k, d in enumerate(datas):
            infos[k] = parse(d)
            if infos[k]["reason"] != 0:
                raise JpegUnsupported(int(infos[k]["reason"]))
            if over_pillow_limit(infos[k]):
                raise JpegUnsupported(TOO_LARGE)
        sizes = [3 * int(i["w"]) * int(i["h"]) for i in infos]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        descs, tables, db, wb = batch_plan(datas, infos, offs[:-1])
        lay = JpegLayout(descs, tables, db, wb)
        host = np.zeros(lay.total, dtype=np.uint8)
        pack(host, lay, descs, tables, datas)
        staged = torch.from_numpy(host).to(self.device)
        pixels = torch.zeros(max(int(offs[-1]), 1), dtype=torch.uint8, device=self.device)
        status = run(staged, lay, pixels, int(offs[-1]))
        st = status.cpu().numpy()
        images = [pixels[int(offs[k]):int(offs[k + 1])].view(int(i["h"]), int(i["w"]), 3) for k, i in enumerate(infos)]
        return images, st
