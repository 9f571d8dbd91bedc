#!/usr/bin/env python
"""Writes tests/golden/image_preprocess.npz: uint8 RGB source images and Pillow's fp16 preprocessing of them (Resize(224, BICUBIC) with
torchvision's size rule, CenterCrop(224), then ToTensor + Normalize(CLIP mean / std) and .half()), so that the GPU test pins
scd_image_preprocess against Pillow even where Pillow is not installed.  `python tools/gen_image_golden.py` (needs Pillow and torch).

Keys: src (uint8, all images' HWC bytes back to back), shapes int32 [B, 2] (h, w), out fp16 [B, 3, 224, 224], pil (Pillow's version)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

# (w, h): odd crop offset (334x250 -> 299x224, left 37.5 -> 38), identity (224x300), upscale (100x80), an edge over 4k px (24x4100),
# ImageNet's commonest size, a 1-px edge (1x7)
SHAPES = [(334, 250), (224, 300), (100, 80), (24, 4100), (500, 375), (1, 7)]


def image(w, h, seed):
    """Colour bands in 9 levels with hard-edged 0 / 255 blocks (bicubic over- and undershoot, so clip8 is exercised); flat regions
    and no noise, so the file compresses."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = [127 + 127 * np.sin(x / (23.0 + 7 * c) + y / (31.0 + 5 * c) + c) for c in range(3)]
    img = (np.rint(np.stack(ch, axis=-1) / 32) * 32).clip(0, 255).astype(np.uint8)
    blocks = ((x // 9 + y // 13 + seed) % 5 == 0)
    img[blocks] = 255 * (rng.integers(0, 2, size=3)).astype(np.uint8)
    return img


def pil_preprocess(img):
    import PIL
    from PIL import Image
    import torch
    import image_ref
    from scd_amd.images import CLIP_MEAN, CLIP_STD
    h, w = img.shape[:2]
    rw, rh = image_ref.resize_size(w, h)
    im = Image.fromarray(img, "RGB")
    if (rw, rh) != (w, h):
        im = im.resize((rw, rh), Image.BICUBIC)
    top, left = image_ref.crop_offset(rh), image_ref.crop_offset(rw)
    im = im.crop((left, top, left + 224, top + 224))
    t = torch.from_numpy(np.array(im, dtype=np.uint8, copy=True)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    t = t.sub_(torch.as_tensor(CLIP_MEAN).view(-1, 1, 1)).div_(torch.as_tensor(CLIP_STD).view(-1, 1, 1))
    return t.half().numpy(), PIL.__version__


def main():
    imgs = [image(w, h, i) for i, (w, h) in enumerate(SHAPES)]
    outs, ver = [], None
    for im in imgs:
        o, ver = pil_preprocess(im)
        outs.append(o)
    path = os.path.join(ROOT, "tests", "golden", "image_preprocess.npz")
    np.savez_compressed(path, src=np.concatenate([im.reshape(-1) for im in imgs]),
                        shapes=np.array([im.shape[:2] for im in imgs], dtype=np.int32), out=np.stack(outs), pil=np.array(ver))
    print(path, os.path.getsize(path), "bytes, Pillow", ver)


if __name__ == "__main__":
    main()
