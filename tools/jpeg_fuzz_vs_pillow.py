#!/usr/bin/env python
"""The CPU JPEG decoder against the installed Pillow on corrupted files (docs/design/ingest.md, "Device JPEG decode": scope).
`python tools/jpeg_fuzz_vs_pillow.py [--n 40000] [--seed 11]`

Every fixture of tests/golden/jpeg_decode.npz is corrupted n times in all, seeded: one byte replaced anywhere (one in five), one byte
replaced in the last two thirds of the file, where the scan lies (three in five), or the file cut at a random length (one in five).
A corrupted file that the parser and scd_jpeg_decode_host accept must decode in Pillow too, to the same pixels.  The decoder runs the
functions the kernels run, so this is the device decoder's verdict.  Prints every disagreement (Pillow raises, or other pixels) with the
byte that was changed, and exits 1 if there was one.  No GPU is used."""
import argparse
import io
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=40000)
    ap.add_argument("--seed", type=int, default=11)
    a = ap.parse_args()
    from PIL import Image
    from scd_amd import jpeg
    warnings.simplefilter("ignore")
    z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz"))
    off = np.concatenate([[0], np.cumsum(z["data_len"])])
    files = [z["data"][off[i]:off[i + 1]].tobytes() for i in range(len(off) - 1)]
    rng = np.random.default_rng(a.seed)
    accepted = bad = 0
    for t in range(a.n):
        fi = int(rng.integers(len(files)))
        d, pos = bytearray(files[fi]), None
        if t % 5 == 4:
            d = d[:int(rng.integers(len(d) + 1))]
        else:
            pos = int(rng.integers(0 if t % 5 == 0 else len(d) // 3, len(d)))
            d[pos] = int(rng.integers(256))
        d = bytes(d)
        try:
            got = jpeg.decode_jpeg_host(d)
        except (jpeg.JpegUnsupported, jpeg.JpegDecodeError):
            continue
        accepted += 1
        try:
            want, err = np.asarray(Image.open(io.BytesIO(d)).convert("RGB")), None
        except Exception as e:
            want, err = None, e
        if err is not None or want.shape != got.shape or not np.array_equal(want, got):
            bad += 1
            what = "Pillow raises %s: %s" % (type(err).__name__, err) if err is not None else "%d values differ" % int((want != got).sum())
            where = "cut to %d bytes" % len(d) if pos is None else "byte %d: %#04x -> %#04x" % (pos, files[fi][pos], d[pos])
            print("%s, %s: %s" % (z["names"][fi], where, what))
    print("%d corruptions, %d accepted by the decoder, %d disagreements with Pillow %s" % (a.n, accepted, bad, Image.__version__ if hasattr(Image, "__version__") else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
