"""numpy restatement of the reference's image preprocessing (torchvision 0.11 `Resize(224, BICUBIC)` + `CenterCrop(224)` on a PIL
RGB image, then CLIP's `ToTensor` + `Normalize`), used by tests/test_image_ingest.py and tools/gen_image_golden.py.

Resize is Pillow's `ImagingResample` for uint8 RGB (Resample.c): per axis `precompute_coeffs` (double, bicubic a = -0.5, support
2 * max(scale, 1)), `normalize_coeffs_8bpc` (int32 taps, PRECISION_BITS = 22), a horizontal pass over the source rows the vertical
pass reads, the intermediate rounded to uint8, then the vertical pass.  Each output is clip8((1 << 21) + sum(in * k)).
"""
import math

import numpy as np

PRECISION_BITS = 22
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the box (0, in_size): per output (first input index, int32 taps)."""
    scale = float(np.float32(in_size)) / out_size          # (double)(in1 - in0) / outSize with float box ends
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = sum_seq(w)
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
        out.append((xmin, np.array(k, dtype=np.int64)))
    return out


def sum_seq(w):
    s = 0.0
    for v in w:                                         # left to right, as the C loop adds
        s += v
    return s


def _clip8(acc):
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def _pass(img, taps, axis):
    """One separable pass over `axis` (0 rows, 1 columns) of a uint8 [H, W, 3] image with the taps of coeffs()."""
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((len(taps),) + src.shape[1:], dtype=np.uint8)
    for i, (first, k) in enumerate(taps):
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for t in range(len(k)):
            acc += src[first + t] * k[t]
        out[i] = _clip8(acc)
    return np.moveaxis(out, 0, axis)


def pil_resize(img, w_out, h_out):
    """PIL.Image.resize((w_out, h_out), BICUBIC) of a uint8 RGB array [H, W, 3]."""
    h, w = img.shape[:2]
    if (w, h) == (w_out, h_out):
        return img.copy()
    ty = coeffs(h, h_out)
    if w_out != w:
        r0 = ty[0][0]
        r1 = ty[-1][0] + len(ty[-1][1])
        tmp = _pass(img[r0:r1], coeffs(w, w_out), 1)        # only the rows the vertical pass reads
        ty = [(f - r0, k) for f, k in ty]
    else:
        tmp = img
    return _pass(tmp, ty, 0) if h_out != h else tmp


def resize_size(w, h, size=224):
    """torchvision 0.11 F_pil.resize with an int size: the short edge becomes `size`, the long one int(size * long / short)."""
    short, long_ = (w, h) if w <= h else (h, w)
    if short == size:
        return w, h
    new_short, new_long = size, int(size * long_ / short)
    return (new_short, new_long) if w <= h else (new_long, new_short)


def crop_offset(length, crop=224):
    """CenterCrop: int(round((length - crop) / 2.0)) - Python's round ties to even."""
    return int(round((length - crop) / 2.0))


def resize_crop(img, size=224, crop=224):
    """uint8 [H, W, 3] RGB -> uint8 [crop, crop, 3]: Resize(size, BICUBIC) then CenterCrop(crop)."""
    h, w = img.shape[:2]
    rw, rh = resize_size(w, h, size)
    r = pil_resize(img, rw, rh)
    top, left = crop_offset(rh, crop), crop_offset(rw, crop)
    return r[top:top + crop, left:left + crop]


def normalize_lut():
    """[3, 256] float32 ((x / 255) - mean) / std, each step rounded to float32 as torch's ToTensor + Normalize do."""
    x = np.arange(256, dtype=np.float32) / np.float32(255)
    mean = np.asarray(CLIP_MEAN, dtype=np.float32)[:, None]
    std = np.asarray(CLIP_STD, dtype=np.float32)[:, None]
    return ((x[None, :] - mean) / std).astype(np.float32)


def preprocess_f32(img, size=224, crop=224):
    """The reference's float32 [3, crop, crop] tensor for one uint8 RGB image."""
    c = resize_crop(img, size, crop)
    return normalize_lut()[np.arange(3)[:, None, None], np.moveaxis(c, 2, 0)]


def preprocess_f16(img, size=224, crop=224):
    return preprocess_f32(img, size, crop).astype(np.float16)
